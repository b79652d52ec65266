"""
tests/philox_oracle.py without a GPU: the Random123 known answers of philox4x32-10, the uniform and the Box-Muller pair at
their edges, the order and the distinctness of the streams, and the conditions on the inputs of
tests/test_gpu_device_streams.py (tests/device_stream_cases.py), so that the GPU test cannot pass emptily.
`-s` prints what each oracle call took and the fragile counts.
"""
import time

import numpy as np
import pytest

import device_stream_cases as DS
import gauss_sim_cases as GS
import philox_oracle as PO

KNOWN = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


def test_known_answers():
    for ctr, key, want in KNOWN:
        got = PO.block(*ctr, key[0] | (key[1] << 32))
        assert got.dtype == np.uint32 and got.shape == (4,)
        assert tuple(int(v) for v in got) == want
    # vectorised over the counters: the three answers of the all-zero key's neighbours in one call agree with single calls
    c0 = np.array([0, 1, 0xffffffff], dtype=np.uint64)
    both = PO.block(c0, 7, c0[::-1], 3, DS.MIXED)
    for r in range(3):
        assert np.array_equal(both[r], PO.block(int(c0[r]), 7, int(c0[2 - r]), 3, DS.MIXED))
    # nine rounds, or the key words exchanged, give other words (the answers pin both)
    assert tuple(int(v) for v in PO.block(*KNOWN[2][0], KNOWN[2][1][1] | (KNOWN[2][1][0] << 32))) != KNOWN[2][2]


def test_uniform():
    assert PO.uniform(0, 0) == 0.0
    assert PO.uniform(0xffffffff, 0xffffffff) == 1.0 - 2.0 ** -53
    assert PO.uniform(0x12345678, 0x9abcd000) == PO.uniform(0x12345678, 0x9abcd7ff)      # the low 11 bits are dropped
    assert PO.uniform(0x12345678, 0x9abcd000) != PO.uniform(0x12345678, 0x9abcd800)
    assert PO.uniform(0x80000000, 0) == 0.5 and PO.uniform(0, 0x800) == 2.0 ** -53
    hi, lo = np.array([1, 2], dtype=np.uint32), np.array([3, 4], dtype=np.uint32)
    assert np.array_equal(PO.uniform(hi, lo), [((1 << 32 | 3) >> 11) * 2.0 ** -53, ((2 << 32 | 4) >> 11) * 2.0 ** -53])


def test_normal_pair():
    # u1 = 2^-53, the smallest: words (0, 1) all ones
    for u2, (c, s) in ((0.0, (1, 0)), (0.25, (0, 1)), (0.5, (-1, 0)), (0.75, (0, -1))):
        n0, n1 = PO.normal_pair_of(2.0 ** -53, u2)
        r = 8.571674348652905
        assert abs(n0 - c * r) <= 1e-15 * r and abs(n1 - s * r) <= 1e-15 * r
        assert (n0 == 0) == (c == 0) and (n1 == 0) == (s == 0)        # the zeros are exact
        assert max(abs(n0), abs(n1)) <= 8.5717
    words = np.array([0xffffffff, 0xffffffff, 0x40000000, 0], dtype=np.uint32)
    n0, n1 = PO.normal_pair(words)
    assert n0 == 0 and abs(n1 - 8.571674348652905) < 1e-14
    # u1 = 1 gives r = 0
    assert PO.normal_pair(np.zeros(4, dtype=np.uint32)) == (0.0, 0.0)
    # against the double-precision formula, everywhere else
    rng = np.random.default_rng(1)
    u1, u2 = 1.0 - rng.random(10000), rng.random(10000)
    n0, n1 = PO.normal_pair_of(u1, u2)
    r = np.sqrt(-2 * np.log(u1))
    assert np.max(np.abs(n0 - r * np.cos(2 * np.pi * u2))) < 1e-14 and np.max(np.abs(n1 - r * np.sin(2 * np.pi * u2))) < 1e-14
    assert abs(np.mean(n0 * n0 + n1 * n1) - 2.0) < 0.1
    if PO.WIDE:     # the quadrant reduction against the direct long-double evaluation
        ang = 2 * PO.PI * u2.astype(PO.LD)
        rl = np.sqrt(-2 * np.log(u1.astype(PO.LD)))
        assert np.max(np.abs(n0 - (rl * np.cos(ang)).astype(float))) < 4e-16 * 9 and np.max(np.abs(n1 - (rl * np.sin(ang)).astype(float))) < 4e-16 * 9


def test_stream_order_and_distinctness():
    seed = DS.MIXED
    u = PO.stream_uniforms(seed, 5, 6, 7, 7)
    assert u.shape == (7,)
    for b in range(4):
        w = PO.block(5, 6, 7, b, seed)
        assert u[2 * b] == PO.uniform(w[2], w[3])
        if 2 * b + 1 < 7:
            assert u[2 * b + 1] == PO.uniform(w[0], w[1])
    assert np.array_equal(PO.stream_uniforms(seed, 5, 6, 7, 8)[:7], u)
    # rows of different c0, c1, c2 and seed halves are distinct
    rows = [PO.stream_uniforms(s, c0, c1, c2, 8) for s, c0, c1, c2 in (
        (seed, 5, 6, 7), (seed, 6, 5, 7), (seed, 7, 6, 5), (seed, 5, 7, 6), (seed, 5, 6, 8), (seed, 4, 6, 7), (seed, 5, 5, 7),
        (DS.swap_halves(seed), 5, 6, 7), (seed & 0xFFFFFFFF, 5, 6, 7), (seed >> 32 << 32, 5, 6, 7), (seed ^ (1 << 32), 5, 6, 7),
        (seed ^ 1, 5, 6, 7))]
    assert len(np.unique(np.concatenate(rows))) == 8 * len(rows)
    # the layouts do not collide at the shapes of the GPU test: 16 j + k < 2^31 for N <= 256 and d <= 8, injective in (j, k)
    N, d = 256, 8
    words = (16 * np.arange(N)[:, None] + np.arange(d)[None, :]).ravel()
    assert len(np.unique(words)) == N * d and words.max() < PO.NOISE_BASE
    assert all(N_ <= N and d_ <= d for N_, d_, _ in DS.ROUSE_CASES)
    z = PO.rouse_normals(seed, 3, 4, 20, 8)
    assert z.shape == (4 * 21 * 8,) and len(np.unique(z)) == len(z)
    # the sub-streams of the draws: draw r and stream index r are the same counter below 2^32, the high word counts beyond
    assert np.array_equal(PO.segdraw_uniforms(seed, np.arange(3), 5), PO.dwelldraw_uniforms(seed, np.arange(3), 5))
    hi = PO.dwelldraw_uniforms(seed, [5, 2 ** 32 + 5, 2 ** 40 + 5], 4)
    assert len(np.unique(hi)) == 12 and np.array_equal(hi[1], PO.stream_uniforms(seed, 5, 1, 0, 4))
    assert np.array_equal(hi[2], PO.stream_uniforms(seed, 5, 256, 0, 4))


def test_layouts():
    seed = DS.SEEDS[1]
    T, N, d, i = 5, 3, 2, 4
    z = PO.rouse_normals(seed, i, T, N, d)
    dyn, noise = z[:T * N * d].reshape(T, N, d), z[T * N * d:].reshape(T, d)
    for t in range(T):
        for j in range(N):
            for k in range(d):
                assert dyn[t, j, k] == PO.normal_pair(PO.block(i, t // 2, 16 * j + k, 0, seed))[t % 2]
        for k in range(d):
            assert noise[t, k] == PO.normal_pair(PO.block(i, t // 2, 2 ** 31 + k, 0, seed))[t % 2]
    # the mutations state other streams
    for kw in (dict(swap=True), dict(mode_stride=8), dict(noise_base=0)):
        assert not np.array_equal(PO.rouse_normals(seed, i, T, N, d, **kw), z)
    assert np.array_equal(PO.rouse_normals(seed, i, T, N, d, mode_stride=8)[:d], z[:d])        # mode 0 keeps its streams
    order = np.array([[0, 1], [1, 0]])
    g = PO.gauss_normals(seed, i, [(0, 3, 1), (3, 5, 0)], order)
    want = [(t, k) for k, f0 in ((0, 1), (1, 0)) for t in range(f0, 3)] + [(t, k) for k in (0, 1) for t in (3, 4)]
    assert len(g) == len(want) == 9
    for v, (t, k) in zip(g, want):
        assert v == PO.normal_pair(PO.block(i, t // 2, k, 1, seed))[t % 2]


@pytest.mark.parametrize('N,d,seed', DS.ROUSE_CASES)
def test_rouse_inputs_let_every_normal_move_the_data(N, d, seed):
    arrays, w = DS.rouse_inputs(N, d)
    cond = DS.rouse_condition(arrays, w)
    com = DS.rouse_condition([a for a in DS.rouse_model(N, d)._modal_arrays()][:3] + [arrays[3]], np.linspace(0.2, 1.0, N))
    print(f"N={N} d={d}: smallest weight or scale / largest = {cond:.2e} (with the centre-of-mass weights {com:.1e})")
    assert cond > DS.CONDITION
    assert seed != DS.swap_halves(seed) and seed in DS.SEEDS
    T, seg_start, seg_state, missing, loc_err = DS.rouse_call(N, d)
    assert tuple(T) == DS.ROUSE_LENGTHS and {1, 2, 3, 65, 257} <= set(T.tolist())
    states = DS.rouse_profiles(N, d)
    cuts = np.concatenate([np.flatnonzero(np.diff(s)) + 1 for s in states])
    assert np.any(cuts % 2 == 1) and np.any(cuts % 2 == 0) and len({int(s[0]) for s in states}) == 3
    assert missing.any() and not missing.all() and np.all(loc_err > 0)
    t0 = time.perf_counter()
    z = DS.rouse_oracle(N, d, seed)
    print(f"    oracle normals of the call: {time.perf_counter() - t0:.2f} s")
    assert z.shape == (int(T.sum()) * (N + 1) * d,) and np.all(np.isfinite(z))


@pytest.mark.parametrize('model_seed,seed', DS.GAUSS_CASES)
def test_gauss_inputs(model_seed, seed):
    model = DS.gauss_model(model_seed)
    assert set(np.unique(model.ss_order)) == {0, 1}
    states = DS.gauss_states()
    assert {len(s) for s in states} == {1, 2, 3, 64, 65, 700}
    starts = [t0 for s in states for t0, _, _ in GS.intervals(s) if t0 > 0]
    assert any(t % 2 for t in starts) and any(t % 2 == 0 for t in starts)
    # profiles start in dimensions of both orders
    first_orders = {int(o) for s in states for o in model.ss_order[s[0]]}
    assert first_orders == {0, 1}
    for (n, k), L in GS.factors(model, 700).items():
        assert np.all(np.diag(L) > 0) and np.all(np.isfinite(L))
    t0 = time.perf_counter()
    z = DS.gauss_oracle(model, seed)
    print(f"gauss model {model_seed}: oracle normals {time.perf_counter() - t0:.2f} s")
    T = np.array([len(s) for s in states])
    assert len(z) == int(T.sum()) * 3 - sum(int(model.ss_order[s[0]].sum()) for s in states)
    assert seed != DS.swap_halves(seed)


def test_seeds_of_the_cases():
    """ every consumer has a case whose high key word is neither 0 nor the low word; all four seeds are used """
    mixed = lambda s: (s >> 32) not in (0, s & 0xFFFFFFFF)
    assert mixed(DS.MIXED) and not mixed(DS.SEEDS[0]) and not mixed(DS.SEEDS[3])
    groups = ([s for _, _, s in DS.ROUSE_CASES], [s for _, s in DS.GAUSS_CASES], [s for _, s in DS.DRAW_CASES],
              [c[3] for c in DS.AMIS_CASES.values()])
    assert all(any(mixed(s) for s in g) for g in groups)
    assert {s for g in groups for s in g} | {DS.SEEDS[3]} == set(DS.SEEDS)


@pytest.mark.parametrize('name', list(DS.AMIS_CASES))
def test_amis_cases_are_firm(name):
    trans, a0, logp0, seed = DS.amis_case(name)
    t0 = time.perf_counter()
    ss, thetas, used, fragile = DS.amis_oracle(name)
    print(f"{name}: fragile {int(fragile.sum())} of {DS.AMIS_N}, uniforms a sample {used.min()} ... {used.max()}, "
          f"oracle {time.perf_counter() - t0:.2f} s")
    assert fragile.sum() <= DS.FRAGILE_CAP * DS.AMIS_N
    k1 = len(a0)
    assert np.allclose(ss.sum(axis=1), 1.0, rtol=0, atol=1e-14) and np.all(ss >= 0)
    assert np.all(trans[thetas[:, :-1], thetas[:, 1:]])
    if name.startswith('corner'):
        assert np.all(np.sort(ss, axis=1)[:, -1] == 1.0) and np.all(used >= 4 * k1 + 1 + k1)
        assert len(np.unique(np.argmax(ss, axis=1))) == k1
    else:
        assert np.all(used >= 3 * k1 + k1 + np.sum(a0 < 1))
        # the law: E ss_j = a_j / sum(a) within 5 standard errors
        mean, var = a0 / a0.sum(), a0 * (a0.sum() - a0) / a0.sum() ** 2 / (a0.sum() + 1)
        assert np.all(np.abs(ss.mean(axis=0) - mean) < 5 * np.sqrt(var / DS.AMIS_N))
    assert len(np.unique(thetas[:, 0])) == trans.shape[0]


def test_amis_gamma_regimes_and_fragility():
    """ the flag: a comparison moved onto its boundary is fragile, one off it is not """
    assert PO._near(1.0, 1.0 + 1e-10, 1.0) and not PO._near(1.0, 1.0 + 1e-8, 1.0) and PO._near(float('nan'), 1.0, 1.0)
    s = PO._Stream(DS.MIXED, 4, 2 ** 33 + 1)
    assert s.key == (DS.MIXED, 1, 2, 4)
    first = [s.uniform() for _ in range(40)]
    assert np.array_equal(first, PO.stream_uniforms(DS.MIXED, 1, 2, 4, 40))
    # gamma(a <= 0) consumes nothing; a >= 1 at least three uniforms, a < 1 one more
    for a, least in ((0.0, 0), (1.0, 3), (0.5, 4)):
        t = PO._Stream(1, 2, 0)
        g = t.gamma(a)
        assert t.used >= least and (t.used == 0) == (least == 0) and (g > 0) == (a > 0)
    prob = PO.amis_prob(np.log(np.array([[0.2, 0.5], [0.8, 0.5]])))
    assert np.allclose(prob, [[0.2, 0.5], [0.8, 0.5]], rtol=1e-15, atol=0)
