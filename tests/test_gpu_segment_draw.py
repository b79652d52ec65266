"""
The exact posterior draws on the GPU (bild_amd.exact.exact_draw, csrc/gauss_segdraw.hip): replay
against the NumPy oracle tests/segment_draw_oracle.py draw for draw, device mode as replay of its own uniforms, the
distribution against the enumeration and against the exact marginals, bit-identity across calls, batches and chunking, the
NaN modes, T = 1000 with k_max = 20, `posterior_distance`, and the refusals of the C call.

The count bound of the distribution tests is that of tests/test_segment_draw.py: |count - N p| <= 5.5 sqrt(N p (1 - p)) + 3 per
comparison, 5.5 binomial standard deviations (two-sided normal tail 4e-8) plus 3 for the Poisson regime of small N p.  All
distribution tests of this file together make 16 273 comparisons, so a
correct implementation fails with probability below 1e-3, and with the fixed seeds not at all once it has passed.
"""
import ctypes

import numpy as np
import pytest

import bild_amd
import segment_cases as C
import segment_draw_oracle as DO
import segment_oracle as SO
from bild_amd import _lib
from test_gpu_segment_dp import order0_gap_case
from test_segment_draw import check_counts, enumeration_posterior
from test_segment_dp import CASES, build

pytestmark = pytest.mark.gpu

K_MAX = 5
N_REPLAY = 4096
REPLAY_CASES = ('s2_T200_gapfree', 's2_T64_isolated_gaps', 's3_T44_forbidden', 's2_T56_order0_gap')


def replay_case(name):
    """ (model, x, uniforms, ks) of a replay case: the models and trajectories of tests/test_gpu_segment_dp.py """
    if name == 's2_T56_order0_gap':
        model, x = order0_gap_case(np.random.default_rng(33), 56)
    else:
        S, T, missing = {'s2_T200_gapfree': (2, 200, ()), 's2_T64_isolated_gaps': (2, 64, (0, 9, 30)),
                         's3_T44_forbidden': (3, 44, ())}[name]
        rng = np.random.default_rng(100 * S + T)
        model = C.random_model(rng, S, T + 8)
        x = C.random_traj(rng, T, missing)
    rng = np.random.default_rng(sum(map(ord, name)))
    return model, x, rng.random((N_REPLAY, 2 * K_MAX)), np.arange(N_REPLAY) % (K_MAX + 1)


def oracle_replay(model, x, uniforms, ks):
    W, F = C.tables(model, x)
    G = SO.backward(W, model.transitions, K_MAX)
    return DO.draws(W, F, G, model.transitions, ks, uniforms)


def check_replay(label, d, x, model, ks, want_start, want_state, fragile, consumed, allowed):
    """
    The replay assertions (shared with tests/test_gpu_segment_wide.py): `ExactDraws` d of uniforms and ks against the oracle's
    replay of them; `allowed` is the number of fragile draws excused, a condition on the inputs
    """
    n = len(ks)
    assert fragile.sum() <= allowed
    assert np.all(want_start[:, 0] == 0)        # every k asked for has profiles of positive weight
    firm = ~fragile
    assert np.array_equal(d.seg_start[firm], want_start[firm]) and np.array_equal(d.seg_state[firm], want_state[firm])
    assert np.array_equal(d.k, ks) and d.n_switches is d.k
    assert np.array_equal(d.uniforms, consumed)
    logL = model.logL_segments(d.seg_start, d.seg_state, x)
    print(f"{label}: fragile {int(fragile.sum())}, max |logL - logL_segments| = {np.max(np.abs(d.logL - logL)):.3e}")
    assert not np.any(np.isnan(d.logL))
    assert np.max(np.abs(d.logL - logL)) < 1e-10
    states = d.states()
    assert states.shape == (n, len(x)) and np.array_equal(np.count_nonzero(np.diff(states, axis=1), axis=1), ks)
    profiles = d.profiles()
    assert len(profiles) == n and np.array_equal(np.asarray(profiles[7][:]), states[7])
    return states


@pytest.mark.parametrize('name', REPLAY_CASES)
def test_replay_against_oracle(name):
    model, x, u, ks = replay_case(name)
    want_start, want_state, fragile, consumed = oracle_replay(model, x, u, ks)
    r = bild_amd.exact_sample(x, model, k_max=K_MAX, nan='omit', marginals=False)
    d = r.draw(N_REPLAY, k=ks, uniforms=u)
    # the excused share: a condition on the inputs (expectation 2 DELTA T per uniform: under 0.1 draws per case)
    check_replay(name, d, x, model, ks, want_start, want_state, fragile, consumed, 0.001 * N_REPLAY)


def same_draws(a, b):
    for name in ('k', 'seg_start', 'seg_state', 'logL', 'uniforms'):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name


def test_device_mode_is_replay_of_its_own_uniforms():
    model, x, _, ks = replay_case('s3_T44_forbidden')
    r = bild_amd.exact_sample(x, model, k_max=K_MAX, marginals=False)
    d = r.draw(N_REPLAY, k=ks, seed=7)
    used = np.arange(2 * K_MAX)[None, :] < np.maximum(1, 2 * ks)[:, None]
    assert np.all((d.uniforms >= 0) & (d.uniforms < 1)) and np.all(d.uniforms[~used] == 0)
    assert np.all(d.uniforms[used] > 0) and len(np.unique(d.uniforms[used])) == used.sum()      # (53 random bits each)
    assert abs(np.mean(d.uniforms[used]) - 0.5) < 5 / np.sqrt(12 * used.sum())
    same_draws(d, r.draw(N_REPLAY, k=ks, uniforms=d.uniforms))
    same_draws(d, r.draw(N_REPLAY, k=ks, seed=7))
    other = r.draw(N_REPLAY, k=ks, seed=8)
    assert not np.array_equal(other.uniforms, d.uniforms) and not np.array_equal(other.seg_start, d.seg_start)
    assert not np.any(np.isnan(d.logL))
    assert np.max(np.abs(d.logL - model.logL_segments(d.seg_start, d.seg_state, x))) < 1e-10
    # the same consumed uniforms through the oracle
    want_start, want_state, fragile, _ = oracle_replay(model, x, d.uniforms, ks)
    assert fragile.sum() <= 0.001 * N_REPLAY
    assert np.array_equal(d.seg_start[~fragile], want_start[~fragile]) and np.array_equal(d.seg_state[~fragile], want_state[~fragile])


def check_marginals(d, log_post, N):
    """ the draws' state counts per frame against exp(log_post) (S, T) """
    states = d.states()
    assert len(states) == N
    counts = np.array([np.sum(states == s, axis=0) for s in range(log_post.shape[0])])
    with np.errstate(under='ignore'):
        p = np.exp(log_post)
    excess = np.abs(counts - N * p) - (5.5 * np.sqrt(N * p * (1 - p)) + 3)
    assert np.all(excess <= 0), (np.unravel_index(np.argmax(excess), excess.shape), float(np.max(excess)))
    return float(np.max(np.abs(counts - N * p) / (5.5 * np.sqrt(N * p * (1 - p)) + 3)))


@pytest.mark.parametrize('name', list(CASES))
def test_distribution_against_enumeration(name):
    model, x = build(name)
    W, F = C.tables(model, x)
    T, N = len(x), 200000
    r = bild_amd.exact_sample(x, model, k_max=3, nan='omit', marginals=False)
    worst = 0.0
    for k in range(4):
        seg_start, seg_state, p, bad = enumeration_posterior(W, F, T, k, model.transitions)
        d = r.draw(N, k=k, seed=1000 + k)
        assert np.all(d.seg_start[:, k + 1:] == T) and np.all(d.seg_state[:, k + 1:] == 0)
        rows, counts_u = np.unique(np.concatenate([d.seg_start[:, :k + 1], d.seg_state[:, :k + 1]], axis=1), axis=0, return_counts=True)
        index = {tuple(a) + tuple(b): i for i, (a, b) in enumerate(zip(seg_start.tolist(), seg_state.tolist()))}
        counts = np.zeros(len(p), dtype=np.int64)
        for row, c in zip(rows.tolist(), counts_u):
            counts[index[tuple(row)]] = c       # (a row that is no profile of k switches: KeyError)
        assert np.all(counts[bad] == 0)         # a NaN profile is never drawn
        worst = max(worst, check_counts(counts, p, N))
    print(f"{name}: largest |count - N p| / bound = {worst:.3f}")


def test_distribution_against_marginals_T200():
    model, x, _, _ = replay_case('s2_T200_gapfree')
    r = bild_amd.exact_sample(x, model, k_max=K_MAX)
    N = 20000
    worst = 0.0
    for k in range(K_MAX + 1):
        worst = max(worst, check_marginals(r.draw(N, k=k, seed=50 + k), r.log_marginal_posterior_k(k), N))
    # 'average': each draw's k by evidence
    d = r.draw(N, k='average', seed=9)
    with np.errstate(under='ignore'):
        w = np.exp(r.evidence - np.max(r.evidence))
    w /= w.sum()
    worst_k = check_counts(np.bincount(d.k, minlength=K_MAX + 1), w, N)
    assert np.array_equal(np.count_nonzero(np.diff(d.states(), axis=1), axis=1), d.k)
    worst = max(worst, check_marginals(d, r.log_marginal_posterior('average'), N))
    print(f"T = 200: largest |count - N p| / bound = {worst:.3f} (frames), {worst_k:.3f} (k by evidence)")
    # the default is best_k
    assert np.all(r.draw(10).k == r.best_k()) and np.all(r.draw(10, dE=1e6).k == 0)


def test_bit_identity():
    rng = np.random.default_rng(3)
    lengths = [60, 3, 131, 45, 72]
    k_max, n = 6, 300
    model = C.random_model(rng, 2, 140)
    trajs = [C.random_traj(rng, T, (0, 5) if T > 10 else ()) for T in lengths]
    res = bild_amd.exact_sample(trajs, model, k_max=k_max, marginals=False)
    ks = np.array([rng.integers(0, min(k_max, T - 1) + 1, size=n) for T in lengths])
    u = rng.random((len(trajs), n, 2 * k_max))
    first = bild_amd.exact_draw(res, n, k=ks, uniforms=u)
    assert isinstance(first, list) and len(first) == len(trajs)
    for j, d in enumerate(first):
        assert np.array_equal(d.k, ks[j]) and np.all(d.seg_start[:, 0] == 0) and d.T == lengths[j]
        assert np.max(np.abs(d.logL - model.logL_segments(d.seg_start, d.seg_state, trajs[j]))) < 1e-10
    for a, b in zip(first, bild_amd.exact_draw(res, n, k=ks, uniforms=u)):      # a repeated call
        same_draws(a, b)
    for j in (0, 1, 2):     # a trajectory alone, on a set of its own: the index of the draw in the call does not matter
        alone = bild_amd.exact_sample(trajs[j], model, k_max=k_max, marginals=False)
        same_draws(first[j], alone.draw(n, k=ks[j], uniforms=u[j]))
    for a, b in zip(first, bild_amd.exact_draw(res, n, k=ks, uniforms=u, scratch_bytes=1)):     # one trajectory per chunk
        same_draws(a, b)
    perm = [2, 0, 4, 1, 3]
    permuted = bild_amd.exact_sample([trajs[j] for j in perm], model, k_max=k_max, marginals=False)
    for j, b in zip(perm, bild_amd.exact_draw(permuted, n, k=ks[perm], uniforms=u[perm])):
        same_draws(first[j], b)
    # draws on some of the set's trajectories only: the others are skipped
    ts = model.trajset(trajs)
    part = _lib.gauss_segment_draw(model.handle(), ts, k_max, model.transitions, np.full(n, 3), ks[3], uniforms=u[3])
    assert np.array_equal(part['seg_start'], first[3].seg_start) and np.array_equal(part['logl'], first[3].logL)
    # device mode: the same seed, whatever the chunks
    dev = bild_amd.exact_draw(res, n, k=ks, seed=5)
    for a, b in zip(dev, bild_amd.exact_draw(res, n, k=ks, seed=5, scratch_bytes=1)):
        same_draws(a, b)


def test_nan_modes():
    model, x = order0_gap_case(np.random.default_rng(33), 56)
    r = bild_amd.exact_sample(x, model, k_max=K_MAX)
    assert r.nan == 'propagate' and np.all(np.isnan(r.evidence[2:]))
    for k in (2, 5):
        with pytest.raises(ValueError, match="nan='omit'"):
            r.draw(10, k=k)
    assert len(r.draw(10, k=1)) == 10
    r = bild_amd.exact_sample(x, model, k_max=K_MAX, nan='omit')
    assert r.nan == 'omit' and sum(r.n_omitted[2:]) > 0
    N = 20000
    worst = 0.0
    for k in range(K_MAX + 1):
        d = r.draw(N, k=k, seed=20 + k)
        assert not np.any(np.isnan(d.logL))
        assert not np.any(np.isnan(model.logL_segments(d.seg_start, d.seg_state, x)))
        worst = max(worst, check_marginals(d, r.log_marginal_posterior_k(k), N))
    print(f"nan='omit': largest |count - N p| / bound = {worst:.3f}")


def test_T1000_kmax20():
    T, k_max, N = 1000, 20, 10000
    rng = np.random.default_rng(11)
    model = C.random_model(rng, 2, T + 8)
    x = C.random_traj(rng, T, (0, 500))
    r = bild_amd.exact_sample(x, model, k_max=k_max)
    best = r.best_k()
    for k in (k_max, best):
        d = r.draw(N, k=k, seed=k)
        switches = d.seg_start[:, 1:k + 1]
        assert np.all(d.seg_start[:, 0] == 0) and np.all(d.seg_start[:, k + 1:] == T) and np.all(d.seg_state[:, k + 1:] == 0)
        assert np.all(switches >= 1) and np.all(switches <= T - 1) and np.all(np.diff(d.seg_start[:, :k + 1], axis=1) > 0)
        assert np.all(model.transitions[d.seg_state[:, :k], d.seg_state[:, 1:k + 1]])
        assert np.array_equal(np.count_nonzero(np.diff(d.states(), axis=1), axis=1), np.full(N, k))
        # the walk's left-to-right order of addition: bit for bit
        assert np.array_equal(d.logL, model.logL_segments(d.seg_start, d.seg_state, x))
        if k == best:
            worst = check_marginals(d, r.log_marginal_posterior_k(best), N)
            print(f"T = 1000: best_k = {best}, largest |count - N p| / bound = {worst:.3f}")
        else:
            assert len(np.unique(d.seg_start, axis=0)) > N // 2


def test_posterior_distance():
    model, x = order0_gap_case(np.random.default_rng(33), 56)
    x[40] = np.nan
    r = bild_amd.exact_sample(x, model, k_max=K_MAX, nan='omit')
    for dE, k in ((None, None), (1e6, None), ('average', 'average')):
        mean, var = r.posterior_distance(n=500, dE=dE, seed=3)
        d = r.draw(500, k=k, dE=None if k else dE, seed=3)
        if dE == 1e6:
            assert np.all(d.k == 0)
        want_mean, want_var = model.kalman_mixture((d.seg_start, d.seg_state), [x], np.zeros(500))
        assert mean.shape == var.shape == x.shape
        assert np.array_equal(mean, want_mean[0]) and np.array_equal(var, want_var[0])
        valid = ~np.isnan(x)
        assert np.array_equal(mean[valid], x[valid]) and np.all(var[valid] == 0)
        assert np.all(np.isfinite(mean)) and np.all(var[~valid] > 0)
    assert len(np.unique(r.draw(500, k='average', seed=3).k)) > 1


def test_c_level_refusals():
    model, x, _, _ = replay_case('s3_T44_forbidden')
    ts = model.trajset([x, x[:30]])
    h = model.handle()
    n = 8
    ks, tj, u = np.arange(n) % (K_MAX + 1), np.arange(n) % 2, np.full((n, 2 * K_MAX), 0.5)

    def refused(match, code=_lib.ERR_INVALID, k_max=K_MAX, draw_traj=tj, draw_k=ks, uniforms=u, scratch_bytes=0):
        with pytest.raises(_lib.BildAmdError, match=match) as e:
            _lib.gauss_segment_draw(h, ts, k_max, model.transitions, draw_traj, draw_k, uniforms=uniforms, scratch_bytes=scratch_bytes)
        assert e.value.code == code

    for bad in (2, -1):
        refused('draw_traj', draw_traj=np.where(np.arange(n) == 5, bad, tj))
    for bad in (K_MAX + 1, -1):
        refused('draw_k', draw_k=np.where(np.arange(n) == 3, bad, ks))
    for bad in (1.0, np.nan, -0.25):
        v = u.copy()
        v[6, 4] = bad
        refused('uniforms', uniforms=v)
    refused('scratch_bytes', scratch_bytes=-1)
    refused('k_max', code=_lib.ERR_UNSUPPORTED, k_max=65, uniforms=None)
    spec = _lib.SegdrawOut()
    lib = _lib.lib()
    tr = np.ascontiguousarray(model.transitions, dtype=np.uint8)
    assert lib.bild_gauss_segment_draw(h._h, ts._h, K_MAX, _lib.aptr(tr), 44, 0, -1, None, None, None, 0, ctypes.byref(spec)) == _lib.ERR_INVALID
    assert lib.bild_gauss_segment_draw(h._h, ts._h, K_MAX, _lib.aptr(tr), 43, 0, 0, None, None, None, 0, ctypes.byref(spec)) == _lib.ERR_INVALID
    assert lib.bild_gauss_segment_draw(h._h, ts._h, K_MAX, _lib.aptr(tr), 44, 0, 0, None, None, None, 0, ctypes.byref(spec)) == _lib.OK     # n = 0
    # the set is still usable
    res = _lib.gauss_segment_draw(h, ts, K_MAX, model.transitions, tj, ks, uniforms=u)
    assert np.all(res['seg_start'][:, 0] == 0) and not np.any(np.isnan(res['logl']))
    trajs = [x, x[:30]]
    for j in range(2):
        rows = tj == j
        want = model.logL_segments(res['seg_start'][rows], res['seg_state'][rows], trajs[j])
        assert np.max(np.abs(res['logl'][rows] - want)) < 1e-10
