"""
Conditions on the inputs of tests/test_gpu_segment_wide.py, without a GPU: the fast oracle `segment_oracle.solve_fast`
against the loops of `segment_oracle.solve` on every output, the cases of tests/segment_wide_cases.py built as described,
the oracle's evidences finite where the cases say, the share of fragile replay draws, the uniqueness of the MAP profiles
that the GPU tests compare state by state, and the 20 s allowed to an oracle answer.

The file adds about 35 s to the tier on 8 cores, so none of the agreement cases the design names sits behind a switch;
`BILD_WIDE_SLOW=1` adds two more beyond 128 frames, (2, 257) and (4, 130) at k_max = 2, whose `solve` takes longest.
"""
import math
import os

import numpy as np
import pytest

import segment_cases as C
import segment_oracle as SO
import segment_wide_cases as WC
from bild_amd.amis import CFC
from bild_amd.exact import profile_count

TILE = 64       # kSegdpTile of csrc/gauss_segdp.h


def agreement_inputs(name):
    """ (W, F, transitions, k_max, nan) """
    if name.startswith('gap_T56'):
        model, x = WC.gap_case(56, 20, 26)
        return WC.fast_tables(model, x) + (model.transitions, 4, name.rsplit('_', 1)[1])
    if name == 'ties':      # ss_order 1 with a leading and an inner gap: F[s][1] = F[s][2] = 0, switch frames inside a gap tie
        model, x = WC.make(3, 40, (0, 1, 20, 21, 22), 'no02')
        return WC.fast_tables(model, x) + (model.transitions, 4, 'propagate')
    if name.startswith('ragged'):
        model, xs, tabs = WC.ragged_case()
        return tabs[int(name[-1])] + (model.transitions, WC.RAGGED_K_MAX, 'propagate')
    case, _, k_max = name.partition('@')
    model, x, W, F, km, nan = WC.segment_case(case)
    return W, F, model.transitions, int(k_max) if k_max else km, nan


AGREEMENT = ['s1_T1', 's1_T65', 's4_T3', 's4_T65@4', 's4_T65_ring', 's4_T70_sink', 's5_T70_source@3', 'gap_T56_propagate', 'gap_T56_omit',
             'ties', 'ragged0', 'ragged4']
SLOW = ['s2_T257@2', 's4_T130@2']


@pytest.mark.parametrize('name', AGREEMENT + (SLOW if os.environ.get('BILD_WIDE_SLOW') else []))
def test_solve_fast_agrees_with_solve(name):
    W, F, transitions, k_max, nan = agreement_inputs(name)
    fast = SO.solve_fast(W, F, transitions, k_max, nan=nan)
    slow = SO.solve(W, F, transitions, k_max, nan=nan)
    finite = W[np.isfinite(W)]
    scale = max(1.0, float(np.max(np.abs(finite)))) if finite.size else 1.0
    assert fast['n_profiles'] == slow['n_profiles'] and fast['n_omitted'] == slow['n_omitted']
    assert all(isinstance(n, int) for n in fast['n_profiles'] + fast['n_omitted'])
    for a, b in zip(fast['map_states'], slow['map_states']):
        assert (a is None) == (b is None) and (a is None or np.array_equal(a, b))
    for key in ('logev', 'KL', 'map_logL', 'log_post'):
        a, b = fast[key], slow[key]
        assert a.shape == b.shape and a.dtype == b.dtype
        assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a == -np.inf, b == -np.inf), key
        fin = np.isfinite(b)
        worst = float(np.max(np.abs(a[fin] - b[fin]))) if fin.any() else 0.0
        print(f"{name}: {key} {worst:.2e} (bar {1e-12 * scale:.2e})")
        assert worst <= 1e-12 * scale, (key, worst)
    # without marginals: the same numbers, no table of completions
    bare = SO.solve_fast(W, F, transitions, k_max, nan=nan, with_marginals=False)
    assert np.array_equal(bare['logev'], fast['logev'], equal_nan=True) and np.all(np.isnan(bare['log_post']))


def test_transition_matrices():
    full, ring, sink, source = (WC.transitions_of(n, S) for n, S in (('full', 4), ('ring', 4), ('sink', 4), ('source', 5)))
    assert np.array_equal(full, ~np.eye(4, dtype=bool))
    assert ring.sum() == 4 and all(ring[s, (s + 1) % 4] for s in range(4))
    assert not sink[3].any() and not sink[0, 3] and sink[1, 3] and sink[2, 3] and sink[:3, :3].sum() == 6 and not np.diag(sink).any()
    assert not source[:, 0].any() and source[0, 1:].all() and source[1:, 1:].sum() == 12 and not np.diag(source).any()
    assert np.array_equal(WC.transitions_of('full', 1), [[False]]) and np.array_equal(WC.transitions_of('ring', 1), [[False]])
    for name, (S, T, missing, trans, k_max, nan) in WC.SEGMENT_CASES.items():
        model, x, W, F, _, _ = WC.segment_case(name)
        assert np.array_equal(model.transitions, WC.transitions_of(trans, S)) and model.nStates == S and x.shape == (T, 2)
        assert W.shape == (S, T, T + 1) and F.shape == (S, T + 1)
        if missing == 'gap':
            assert np.array_equal(np.nonzero(np.isnan(x[:, 0]))[0], np.arange(61, 67)) and not np.any(np.isnan(x[:, 1]))
            assert np.any(np.isnan(W)) and 61 // TILE != 66 // TILE
        else:
            assert np.array_equal(np.nonzero(np.isnan(x).any(axis=1))[0], missing) and not np.any(np.isnan(W)) and not np.any(np.isnan(F))
            assert all(t + 1 not in missing for t in missing)                   # isolated
            assert not len(missing) or np.all(model.ss_order == 1)
    # the S = 3 rule of `random_model` reaches no four-state matrix, and (3, 321) forbids 0 -> 2 by name
    assert WC.segment_case('s4_T65')[0].transitions.sum() == 12 and not WC.segment_case('s3_T321')[0].transitions[0, 2]


def test_launch_shapes():
    tiles = lambda T: (T + TILE - 1) // TILE
    assert tiles(257) == 5 and tiles(321) == 6 and tiles(257) % 4 and tiles(321) % 4        # the last workgroup of four tiles is partial
    assert tiles(256) == 4 and tiles(1000) % 4 == 0 and tiles(2048) % 4 == 0                # what stood before: whole workgroups
    assert [T for T, _ in WC.RAGGED] == [1, 257, 64, 130, 2, 65]
    n_rows = len(WC.BACKTRACK_T) * (WC.BACKTRACK_K_MAX + 1)
    assert n_rows == 264 > 256 and WC.BACKTRACK_T == tuple(range(5, 49))
    assert all(j * (WC.BACKTRACK_K_MAX + 1) >= 256 - WC.BACKTRACK_K_MAX for j in WC.BACKTRACK_ORACLE[1:])
    assert 42 * 6 < 256 <= 42 * 6 + 5 and 43 * 6 >= 256       # trajectory 42 straddles the workgroups, 43 lies in the second
    full4 = WC.transitions_of('full', 4)
    assert profile_count(1025, 1, full4) == 12 * 1024 == 3 * 4096 and profile_count(1026, 1, full4) == 3 * 4096 + 12
    assert profile_count(18, 15, WC.transitions_of('full', 2)) == 272 and profile_count(17, 15, WC.transitions_of('full', 2)) == 32
    assert profile_count(12, 5, full4) == 449064
    assert profile_count(20, 0, [[False]]) == 1 and profile_count(20, 1, [[False]]) == 0
    lds = lambda S, T, K1: S * T * 8 + 256 * 8 + 256 * K1 * 8       # exact_reduce_lds of csrc/exact.hip
    assert lds(4, 1800, 2) == 63744 < 65536 < 63744 + 10240 and lds(4, 2048, 2) == 71680 and 4 * 2048 == 8192 < 5 * 1639


def test_oracle_evidence_finite_where_the_case_says():
    """
    -inf: S = 1 from k = 1 on (no switch without a second state) and k > T - 1 (`s4_T3` at k = 3, 4); NaN: the gap case under
    'propagate' from k = 2 on.  `ring`, `sink` and `source` admit every k: each holds a cycle (0 1 2 3 0; 0 1 0; 1 2 1).
    """
    for name, (S, T, missing, trans, k_max, nan) in WC.SEGMENT_CASES.items():
        out = WC.segment_answer(name)
        want_inf = np.array([S == 1 and k >= 1 or k > T - 1 for k in range(k_max + 1)])
        want_nan = np.array([name == 'gap_T130_propagate' and k >= 2 for k in range(k_max + 1)])
        assert np.array_equal(out['logev'] == -np.inf, want_inf), name
        assert np.array_equal(np.isnan(out['logev']), want_nan), name
        traces = CFC(WC.transitions_of(trans, S))
        assert all((traces.N_total(k) > 0) == (S > 1) for k in range(1, k_max + 1))
        assert out['n_profiles'] == [math.comb(T - 1, k) * traces.N_total(k) for k in range(k_max + 1)] or nan == 'omit'
        if name == 'gap_T130_omit':
            assert out['n_omitted'][:2] == [0, 0] and all(n > 0 for n in out['n_omitted'][2:])
        lp = out['log_post']
        for k in range(k_max + 1):
            assert np.all(np.isnan(lp[k])) if want_inf[k] or want_nan[k] else not np.any(np.isnan(lp[k])), (name, k)
    for j, out in enumerate(WC.ragged_answers()):
        T = WC.RAGGED[j][0]
        assert np.array_equal(np.isfinite(out['logev']), np.arange(WC.RAGGED_K_MAX + 1) <= T - 1)


def test_log_marginals_within_the_range_of_linear_weights():
    """
    The device sums the marginal weights of a level in linear scale, exp(. - map_logL_k), so a log marginal below about -700
    is 0 there and finite in the oracle, and one below -600 loses digits ("Range").
    `check_against_oracle` holds every finite log marginal to 1e-10, so the cases that go through it keep theirs above -600.
    The sharp case is the one that does not, held by `test_marginals_below_the_linear_range` of the GPU file: it has
    entries between -700 and -600, entries below -760, where every weight of the entry is below 2^-1074 whatever the level's
    evidence adds, a unique MAP at every k, and `sharp_bar` is 1e-10 at -600 and at most 1e-5 at -700.
    """
    answers = [WC.segment_answer(name) for name in WC.SEGMENT_CASES] + WC.ragged_answers() + \
        [WC.backtrack_answer(j)[2] for j in WC.BACKTRACK_ORACLE]
    lows = [float(np.min(lp[np.isfinite(lp)], initial=0.0)) for lp in (out['log_post'] for out in answers)]
    print([round(v, 1) for v in lows])
    assert min(lows) > WC.SHARP_FIRM
    out = WC.sharp_answer()
    lp = out['log_post']
    model, x, W, F = WC.sharp_case()
    assert len(x) == 257 and model.nStates == 4 and np.array_equal(np.nonzero(np.isnan(x).any(axis=1))[0], [100])
    assert not np.any(np.isnan(lp)) and np.all(np.isfinite(out['logev'])) and all(out['map_unique'])
    band = (lp < WC.SHARP_FIRM) & (lp >= WC.SHARP_FLOOR)
    print(f"sharp: lowest per k {[round(float(np.min(l[np.isfinite(l)])), 1) for l in lp]}, {int(band.sum())} in the band, "
          f"{int(np.sum(lp < -760))} below -760, oracle {WC.ORACLE_SECONDS['sharp']:.2f} s")
    assert band.sum() >= 10 and np.sum(lp < -760) >= 10 and np.sum(lp >= WC.SHARP_FIRM) > 0.8 * lp.size
    for k in range(WC.SHARP_K_MAX + 1):
        n = out['n_profiles'][k]
        assert abs(WC.sharp_bar(-600.0, k, 257, n) - 1e-10) < 1e-20 and WC.sharp_bar(-700.0, k, 257, n) < 1e-5


def test_map_unique_where_compared_state_by_state():
    for name in WC.SAME_MAP:
        assert not WC.SEGMENT_CASES[name][2] and all(WC.segment_answer(name)['map_unique']), name
    for j in WC.RAGGED_SAME_MAP:
        assert not WC.RAGGED[j][1] and all(WC.ragged_answers()[j]['map_unique'])
    # the test sees a tie: every state of a one-frame trajectory of ss_order 1 has F = 0
    assert not WC.ragged_answers()[0]['map_unique'][0]


def test_replay_draws_are_firm():
    for name in WC.REPLAY_CASES:
        u, ks, want_start, want_state, fragile, consumed = WC.replay_answer(name)
        S, T, _, _, k_max, _ = WC.SEGMENT_CASES[name]
        print(f"{name}: fragile {int(fragile.sum())}, oracle {WC.ORACLE_SECONDS['replay', name]:.1f} s")
        assert u.shape == (WC.N_REPLAY, 2 * k_max) and fragile.sum() <= 0.001 * WC.N_REPLAY
        assert np.all(want_start[:, 0] == 0)        # every drawn k has profiles of positive weight
        assert np.all(ks == 0) if S == 1 else np.array_equal(np.bincount(ks) > 0, np.ones(k_max + 1, dtype=bool))
    for j in WC.RAGGED_DRAWN:
        want_start, want_state, fragile, consumed = WC.ragged_replay_answer(j)
        assert fragile.sum() <= 1 and len(fragile) == WC.N_RAGGED_DRAWS and np.all(want_start[:, 0] == 0)


def test_oracle_answers_within_their_time():
    for name in WC.SEGMENT_CASES:
        WC.segment_answer(name)
    WC.ragged_answers()
    WC.sharp_answer()
    for j in WC.BACKTRACK_ORACLE:
        WC.backtrack_answer(j)
    print({k: round(v, 2) for k, v in WC.ORACLE_SECONDS.items()})
    assert max(WC.ORACLE_SECONDS.values()) < WC.ORACLE_LIMIT


def test_enumeration_logl_of_the_tables():
    """ `table_logl` on the fast tables equals the reference loop of the likelihood on an expanded profile (T <= 40) """
    import exact_oracle as X
    import gauss_oracle as G
    model, x, _, k = WC.enum_case('s4_T40_k4_ring')
    W, F = WC.fast_tables(model, x)
    seg_start, seg_state = X.enumerate_profiles(len(x), k, model.transitions)
    rows = np.random.default_rng(0).choice(len(seg_start), 20, replace=False)
    got = C.table_logl(W, F, seg_start[rows], seg_state[rows], len(x))
    states = X.states_from_segments(seg_start[rows], seg_state[rows], len(x))
    slow = C.tables(model, x)
    assert np.max(np.abs(got - [G.logl_tables(*slow, s) for s in states])) < 1e-10
    assert len(seg_start) == math.comb(39, 4) * 4 and np.all(np.diff(seg_state, axis=1) % 4 == 1)
