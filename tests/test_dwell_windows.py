"""
The exact window support under a dwell-time prior without a GPU (bild_amd.exact.exact_dwell_windows): the
two formulations of the NumPy oracle tests/dwell_window_oracle.py against the enumeration of every profile on the cases of
tests/test_dwell.py, the five identities of section 29 against `dwell_oracle`, `dwell_event_oracle` and
`dwell_occupancy_oracle`, an impossible event, `DwellWindowSupport.p_not_all`, `ExactDwellResults.map_support` assembled from
oracle answers on a hand-checked profile, `ExactDwellDraws.all_in` on hand-made states, the argument errors, and the binding
of bild_gauss_dwell_windows against include/bild_amd_windows.h.  Deviations seen: tests/README_dwell_windows.md.
"""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import bild_amd
import dwell_cases as DC
import dwell_event_cases as DEC
import dwell_event_oracle as DE
import dwell_occupancy_oracle as DQ
import dwell_oracle as DO
import dwell_window_cases as DWC
import dwell_window_oracle as DW
import segment_cases as C
import test_abi_header as AH
import test_dwell as TD
from bild_amd import _lib
from bild_amd import exact as EX

# the issue's bound against enumeration and on the identities, the siblings' CPU bound
TOL = 1e-12

TARGETS = {2: ((0,), (1,)), 3: ((2,), (0, 2), (1,))}
NAMES = [n for n in TD.CASES if 'order0' not in n]


def eight_windows(T):
    """ one frame at either end and inside, the whole trajectory, both halves with a shared frame, windows that touch one end """
    return [(0, 1), (T - 1, T), (T // 2, T // 2 + 1), (0, T), (0, T // 2 + 1), (T // 2, T), (1, T - 2), (2, 5)]


def close_logs(got, want, what):
    """ every finite log within TOL, -inf exactly; returns the worst deviation """
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    assert got.shape == want.shape, what
    assert not np.any(np.isnan(got)) and not np.any(np.isnan(want)), what
    assert np.array_equal(got == -np.inf, want == -np.inf), what
    fin = want > -np.inf
    worst = float(np.max(np.abs(got[fin] - want[fin]), initial=0.0))
    assert worst < TOL, (what, worst)
    return worst


def profile_weights(W, F, prior):
    """ (states (n, T), weights (n,)) of every profile, normalised: an enumeration that shares no code with the oracle's """
    T = F.shape[1] - 1
    states, joint = [], []
    for _, seg_start, seg_state, st in DO.all_profiles(T, F.shape[0]):
        logl = C.table_logl(W, F, seg_start, seg_state, T)
        lp = np.array([prior.log_prob(row) for row in st])
        states.append(st)
        joint.append(np.where(lp == -np.inf, -np.inf, lp + logl))
    states, joint = np.concatenate(states), np.concatenate(joint)
    w = np.exp(joint - joint.max())
    return states, w / w.sum()


@pytest.mark.parametrize('kind', ['markov', 'nongeometric', 'minlength'])
@pytest.mark.parametrize('name', NAMES)
def test_oracle_against_enumeration(name, kind):
    model, x, prior = TD.build(name, kind)
    S, T = TD.CASES[name][:2]
    W, F = C.tables(model, x)
    windows = [(u, v, target) for target in TARGETS[S] for u, v in eight_windows(T)]
    want = DW.enumerate_all(W, F, prior, windows)
    assert want['n_nan'] == 0
    for solve in (DW.solve, DW.solve_masked):
        got = solve(W, F, prior, windows)
        assert got['n_nan_windows'] == 0 and abs(got['logev'] - want['logev']) < TOL
        worst = close_logs(got['log_all'], want['log_all'], (name, kind, solve.__name__))
        print(f"{solve.__name__}: worst deviation of a log from the enumeration {worst:.1e}")


@pytest.mark.parametrize('name', [n for n in DEC.SMALL if DEC.SMALL[n][0] > 1])
def test_oracle_against_enumeration_at_four_states_and_hard_priors(name):
    """ both formulations are the statement at these shapes too: `dwell_event_cases.SMALL`, every (u, v) with every target of S """
    S, T, gap, kind = DEC.SMALL[name]
    model, x, prior, W, F = DEC.small_case(name)
    assert model.nStates == prior.nStates == S and np.array_equal(np.flatnonzero(np.isnan(x[:, 0])), [gap]) and F.shape == (S, T + 1)
    windows = [(u, v, target) for target in DEC.SMALL_TARGETS[S] for u in range(T) for v in range(u + 1, T + 1)]
    want = DW.enumerate_all(W, F, prior, windows)
    assert want['n_nan'] == 0 and np.isfinite(want['logev'])
    for solve in (DW.solve, DW.solve_masked):
        got = solve(W, F, prior, windows)
        assert got['n_nan_windows'] == 0 and abs(got['logev'] - want['logev']) < TOL
        worst = close_logs(got['log_all'], want['log_all'], (name, solve.__name__))
        print(f"{solve.__name__}: {len(windows)} windows, {int(np.sum(got['log_all'] == -np.inf))} at -inf, worst deviation of a log from the enumeration {worst:.1e}")
    empty = {w for w, v in zip(windows, want['log_all']) if v == -np.inf}
    if kind in ('nongeometric', 'minlength'):
        assert not empty
    if kind == 'flip':          # the states alternate: one frame alone stays in one state
        assert empty == {w for w in windows if w[1] - w[0] > 1}
    if kind == 'bounded3':      # no segment longer than 3 frames
        assert empty == {w for w in windows if w[1] - w[0] > 3}
    if kind == 'one_start':     # every profile starts in state 2
        assert empty == {w for w in windows if w[0] == 0 and 2 not in w[2]}
    if kind == 'absorbing':     # state 2 is never left, and 0 -> 2 is forbidden: nothing is excluded outright but a return
        assert not empty and np.all(prior.log_jump[2] == -np.inf)


@pytest.mark.parametrize('kind', ['markov', 'nongeometric', 'minlength'])
@pytest.mark.parametrize('nan', ['propagate', 'omit'])
def test_oracle_nan_windows_against_enumeration(nan, kind):
    model, x, prior = TD.build('s2_order0_inner_gap', kind)
    W, F = C.tables(model, x)
    T = F.shape[1] - 1
    windows = [(u, v, target) for target in TARGETS[2] for u, v in eight_windows(T)]
    want = DW.enumerate_all(W, F, prior, windows, nan=nan)
    for solve in (DW.solve, DW.solve_masked):
        got = solve(W, F, prior, windows, nan=nan)
        assert got['n_nan_windows'] == DO.solve(W, F, prior, nan=nan)['n_nan_windows'] > 0 and want['n_nan'] > 0
        if nan == 'propagate':
            assert np.isnan(got['logev']) and np.all(np.isnan(got['log_all'])) and np.all(np.isnan(want['log_all']))
            continue
        assert abs(got['logev'] - want['logev']) < TOL
        close_logs(got['log_all'], want['log_all'], (nan, kind, solve.__name__))


@pytest.mark.parametrize('kind', ['markov', 'nongeometric', 'minlength'])
@pytest.mark.parametrize('name', NAMES)
def test_identities(name, kind):
    """ section 29's five identities, each against a number that the window oracle did not compute """
    model, x, prior = TD.build(name, kind)
    S, T = TD.CASES[name][:2]
    W, F = C.tables(model, x)
    ref = DO.solve(W, F, prior)
    logev = ref['logev']
    devs = {}
    for target in TARGETS[S]:
        rest = tuple(s for s in range(S) if s not in target)
        # [t, t + 1): the marginals over G
        frames = DW.solve(W, F, prior, [(t, t + 1, target) for t in range(T)])['log_all']
        devs['one frame = marginal'] = close_logs(frames, [DE._lse(ref['log_post'][list(target), t]) for t in range(T)], 'marginal')
        # [0, T): never outside G, and all T frames in G
        whole = DW.solve(W, F, prior, [(0, T, target)])['log_all'][0]
        devs['whole = never'] = close_logs(whole, DE.solve(W, F, prior, target=rest)['log_never'], 'never')
        devs['whole = pmf[T]'] = close_logs(whole, DE._lse(DQ.solve(W, F, prior, target)['log_occupancy'][T]), 'occupancy')
        # for fixed u non-increasing in v
        for u in (0, 1, T // 2):
            run = DW.solve(W, F, prior, [(u, v, target) for v in range(u + 1, T + 1)])['log_all']
            assert np.all(np.diff(run) <= TOL), (target, u, run)
    # the windows of one state, all S of them: no switch at the frames u + 1 ... v - 1
    states, weight = profile_weights(W, F, prior)
    al = np.full((T + 1, S), -np.inf)
    A, _ = DE.forward(W, F, prior, prior.log_init, prior.log_jump)
    for c in range(1, T):
        al[c] = DE._mix(A[c], prior.log_jump)
    _, gamma = DE.backward(W, prior)
    for u, v in eight_windows(T):
        single = DW.solve(W, F, prior, [(u, v, (s,)) for s in range(S)])['log_all']
        constant = np.all(states[:, u:v] == states[:, u:u + 1], axis=1)
        devs['sum over states = no switch'] = max(devs.get('sum over states = no switch', 0.0),
                                                  abs(np.exp(single).sum() - weight[constant].sum()))
        if S != 2:
            continue
        for s in range(S):      # section 21's Q(a, b, s) over a <= u, b >= v
            terms = []
            for a in range(u + 1):
                for b in range(v, T + 1):
                    w = F[s, b] if a == 0 else W[s, a - 1, b]
                    if not np.isnan(w):
                        terms.append((prior.log_init[s] if a == 0 else al[a, s]) + DE._omega(prior, s, a, b, T) + w + gamma[b, s] - logev)
            devs['sum of Q'] = max(devs.get('sum of Q', 0.0), close_logs(single[s], DE._lse(terms), 'Q'))
    print(', '.join(f"{k}: {v:.1e}" for k, v in devs.items()))
    assert all(v < TOL for v in devs.values()), devs


def test_an_impossible_event_is_minus_infinity():
    """ every profile starts in state 1 ('one_start'): a window from frame 0 in state 0 has no profile, one from frame 1 has """
    rng = np.random.default_rng(12)
    model = C.random_model(rng, 2, 14)
    x = C.random_traj(rng, 10)
    prior = DC.prior_of('one_start', rng, 2, 12, 10)
    assert prior.log_init[0] == -np.inf
    W, F = C.tables(model, x)
    windows = [(0, 1, (0,)), (0, 4, (0,)), (0, 10, (0,)), (1, 4, (0,)), (0, 1, (1,))]
    want = DW.enumerate_all(W, F, prior, windows)
    for solve in (DW.solve, DW.solve_masked):
        got = solve(W, F, prior, windows)['log_all']
        assert np.all(got[:3] == -np.inf) and np.isfinite(got[3]) and abs(got[4]) < TOL
        close_logs(got, want['log_all'], solve.__name__)


def hand_made(log_all):
    n = len(log_all)
    return bild_amd.DwellWindowSupport(traj=np.zeros((6, 1)), model=None, prior=None, nan='propagate', windows=np.tile([0, 6], (n, 1)),
                                       targets=((1,),) * n, log_evidence=-3.0, n_nan_windows=0, log_all=np.asarray(log_all, dtype=float))


def test_p_all_and_p_not_all():
    r = hand_made([-np.inf, 0.0, np.log(0.25), -1e-12, -1e-300, np.nan])
    assert np.array_equal(r.p_all()[:3], [0.0, 1.0, 0.25])
    p = r.p_not_all()
    assert p[0] == 1.0 and p[1] == 0.0 and abs(p[2] - 0.75) < 1e-16 and np.isnan(p[5])
    # no cancellation near 0: 1 - exp(-1e-12) in floating point is 1.000088900582341e-12, -expm1 gives 1e-12 (1 - 5e-13)
    assert abs(p[3] / 1e-12 - (1 - 5e-13)) < 1e-15 and p[4] == 1e-300
    assert 'absolute error' in bild_amd.DwellWindowSupport.p_not_all.__doc__ and 'relative error' in bild_amd.DwellWindowSupport.p_not_all.__doc__
    assert 'windows=6' in repr(r)


def test_all_in_of_draws_on_hand_made_states():
    states = np.array([[0, 0, 1, 1, 0, 255], [1, 0, 0, 0, 0, 255], [0, 0, 0, 0, 0, 255], [0, 2, 2, 1, 0, 255]], dtype=np.uint8)
    n = len(states)
    draws = bild_amd.ExactDwellDraws(5, states, np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n), None)
    for (u, v, target), want in (((0, 2, 0), 0.5), ((0, 5, 0), 0.25), ((2, 4, 1), 0.25), ((2, 4, (1, 2)), 0.5), ((1, 5, [0]), 0.5),
                                 ((4, 5, {0}), 1.0), ((0, 1, 2), 0.0), ((1, 3, (0, 2)), 0.75)):
        assert draws.all_in(u, v, target) == want, (u, v, target)
    for u, v in ((0, 0), (3, 2), (-1, 2), (0, 6), (5, 6)):      # (the padding behind T is no frame)
        with pytest.raises(ValueError):
            draws.all_in(u, v, 0)
    empty = bild_amd.ExactDwellDraws(5, np.zeros((0, 5), dtype=np.uint8), np.zeros(0), np.zeros(0), np.zeros(0), np.zeros(0), None)
    assert np.isnan(empty.all_in(0, 2, 0))


def test_map_support_on_a_hand_checked_profile(monkeypatch):
    """
    T = 10, the called profile 0 0 0 1 1 1 1 0 0 0: segments [0, 3), [3, 7), [7, 10), switches at 3 and 7.  Radii 0, 2, 5 around
    c = 3 are the frames [2, 4), [0, 6), [-3, 9) -> [0, 9); around c = 7: [6, 8), [4, 10), [1, 13) -> [1, 10).
    """
    rng = np.random.default_rng(5)
    model = C.random_model(rng, 2, 14)
    x = C.random_traj(rng, 10)
    prior = DC.make_prior('markov', rng, 2, 12)
    W, F = C.tables(model, x)
    called = [0, 0, 0, 1, 1, 1, 1, 0, 0, 0]
    asked = []

    def from_oracle(trajs, m, p, windows, nan='propagate', scratch_bytes=0):
        assert trajs is x and m is model and p is prior and nan == 'propagate'
        asked.extend(windows)
        ans = DW.solve(W, F, prior, windows, nan=nan)
        return bild_amd.DwellWindowSupport(traj=x, model=model, prior=prior, nan=nan, windows=np.array([w[:2] for w in windows]),
                                           targets=tuple(w[2] for w in windows), log_evidence=ans['logev'],
                                           n_nan_windows=ans['n_nan_windows'], log_all=ans['log_all'])
    monkeypatch.setattr(EX, 'exact_dwell_windows', from_oracle)

    def results(profile, m=model):
        return bild_amd.ExactDwellResults(traj=x, model=m, prior=prior, nan='propagate', log_evidence=0.0, map_profile=profile,
                                          map_log_joint=0.0, log_marginal_posterior=None, expected_jumps=None, expected_stay=None,
                                          n_nan_windows=0)
    sup = results(bild_amd.Loopingprofile(called)).map_support()
    assert asked == [(0, 3, (0,)), (0, 3, (1,)), (3, 7, (1,)), (3, 7, (0,)), (7, 10, (0,)), (7, 10, (1,)),
                     (2, 4, (0,)), (2, 4, (1,)), (0, 6, (0,)), (0, 6, (1,)), (0, 9, (0,)), (0, 9, (1,)),
                     (6, 8, (0,)), (6, 8, (1,)), (4, 10, (0,)), (4, 10, (1,)), (1, 10, (0,)), (1, 10, (1,))]
    assert sup.n_queries == 18 and sup.radii == (0, 2, 5) and 'segments=3' in repr(sup)
    assert sup.seg_start.tolist() == [0, 3, 7] and sup.seg_end.tolist() == [3, 7, 10] and sup.seg_state.tolist() == [0, 1, 0]
    assert sup.switch_frames.tolist() == [3, 7] and sup.p_switch_within.shape == (2, 3)
    states, weight = profile_weights(W, F, prior)
    for i, (a, b, s) in enumerate(((0, 3, 0), (3, 7, 1), (7, 10, 0))):
        assert abs(sup.p_whole()[i] - weight[np.all(states[:, a:b] == s, axis=1)].sum()) < TOL
        assert abs(sup.p_present()[i] - weight[np.any(states[:, a:b] == s, axis=1)].sum()) < TOL
    switch = np.diff(states, axis=1) != 0        # column t - 1: a switch at frame t
    for i, c in enumerate((3, 7)):
        for j, r in enumerate((0, 2, 5)):
            lo, hi = max(c - r, 1), min(c + r, 9)
            assert abs(sup.p_switch_within[i, j] - weight[switch[:, lo - 1:hi].any(axis=1)].sum()) < TOL, (c, r)
    assert np.all(np.diff(sup.p_switch_within, axis=1) >= -TOL)         # a wider range holds no fewer switches
    assert results(bild_amd.Loopingprofile([1] * 10)).map_support(radii=()).p_switch_within.shape == (0, 0)
    with pytest.raises(ValueError, match='MAP profile'):
        results(None).map_support()
    with pytest.raises(ValueError, match='one state'):
        results(bild_amd.Loopingprofile([0] * 10), C.random_model(rng, 1, 14)).map_support()
    for radii in ((-1,), (1.5,), (True,)):
        with pytest.raises(ValueError, match='radii'):
            results(bild_amd.Loopingprofile(called)).map_support(radii=radii)


def test_refusals_come_before_any_upload(monkeypatch):
    def no_upload(*a, **k):
        raise AssertionError("a trajectory set was made")
    monkeypatch.setattr(_lib, 'GaussTrajSetHandle', no_upload)
    rng = np.random.default_rng(3)
    model = C.random_model(rng, 2, 24)
    x = C.random_traj(rng, 20)
    prior = DC.symmetric_chain(0.1, 20)
    rouse = bild_amd.MultiStateRouse(8, 1, 5, d=2, localization_error=0.1)
    factorized = bild_amd.FactorizedModel([np.array([1.0, 2.0]), np.array([1.0, 4.0])], d=2)
    call = bild_amd.exact_dwell_windows
    good = [(0, 5, 1)]
    for other in (rouse, factorized):
        with pytest.raises(TypeError):
            call(x, other, prior, good)
    with pytest.raises(TypeError):
        call(x, model, (prior.log_init, prior.log_jump), good)
    with pytest.raises(ValueError):
        call(x, model, prior, good, nan='drop')
    with pytest.raises(ValueError):         # the tables are shorter than the trajectory
        call(x, model, DC.symmetric_chain(0.1, 19), good)
    with pytest.raises(ValueError):         # the states do not match
        call(x, model, DC.make_prior('markov', rng, 3, 20), good)
    with pytest.raises(ValueError):         # beyond the model's lags
        call(C.random_traj(rng, 30), model, DC.symmetric_chain(0.1, 40), good)
    with pytest.raises(ValueError):         # more states than the recursion supports
        call(x, C.random_model(rng, 5, 24), DC.make_prior('markov', rng, 5, 20), good)
    for target in ((), [], (0, 1), [1, 0, 1], 2, -1, (1, 2), 1.0, True, (0.5,)):     # empty, full, out of range, not a state
        with pytest.raises(ValueError):
            call(x, model, prior, [(0, 5, target)])
    for u, v in ((0, 0), (5, 5), (6, 5), (-1, 5), (0, 21), (20, 21), (0.0, 5), (0, 5.0), (True, 5)):     # outside 0 <= u < v <= T = 20
        with pytest.raises(ValueError, match='window 1'):
            call(x, model, prior, [(0, 5, 1), (u, v, 1)])
    for windows in ([(0, 5)], [(0, 5, 1, 1)], [3], 3):       # no (u, v, target)
        with pytest.raises(ValueError):
            call(x, model, prior, windows)
    one = C.random_model(rng, 1, 24)            # one state has no proper subset
    with pytest.raises(ValueError):
        call(x, one, DC.make_prior('markov', rng, 1, 20), [(0, 5, 0)])
    # a list of trajectories needs a list of as many sequences, each checked against its own trajectory
    y = C.random_traj(rng, 10)
    for windows in ([good], [good, good, good], good, 7):
        with pytest.raises(ValueError):
            call([x, y], model, prior, windows)
    with pytest.raises(ValueError, match='of trajectory 1'):
        call([x, y], model, prior, [good, [(0, 11, 1)]])
    assert call([], model, prior, []) == []
    with pytest.raises(ValueError):
        call([], model, prior, [good])


# ---------------------------------------------------------------- the conditions on the inputs of the wide GPU cases

# per wide case what the oracle gives over all parts: (finite windows, windows at -inf).  Listed, so that a change of a
# generator that empties a comparison is seen here.
WIDE_FINITE = {
    (4, 64, (), 'minlength'): (21, 0), (4, 129, (64, 100), 'markov'): (54, 0), (4, 257, (100,), 'nongeometric'): (75, 0),
    (2, 256, (), 'markov'): (42, 0), (2, 257, (255,), 'minlength'): (50, 0), (3, 321, (128,), 'markov'): (81, 0),
    (2, 65, (), 'nongeometric'): (18, 0), (3, 193, (3,), 'nongeometric'): (63, 0), (2, 130, (), 'bounded'): (36, 2),
    (3, 193, (), 'bounded'): (56, 7), (2, 65, (), 'one_start'): (15, 3), (3, 130, (20,), 'absorbing'): (57, 0), (2, 70, (), 'flip'): (8, 18),
}


@pytest.mark.parametrize('case', [c for c in DEC.WIDE if c[0] > 1], ids=DEC.wide_id)
def test_gpu_wide_cases_meet_their_conditions(case):
    """ what tests/test_gpu_dwell_windows.py compares the device with is what it is meant to be, and no comparison is vacuous """
    S, T, missing, kind = case
    model, x, prior, W, F = DC.oracle_case(case)
    assert model.nStates == prior.nStates == S and x.shape == (T, 2) and prior.L == T + 5
    assert np.array_equal(np.flatnonzero(np.isnan(x[:, 0])), missing)
    spans = DWC.wide_spans(T)
    assert spans[:len(DWC.spans(T))] == DWC.spans(T) and len(set(spans)) == len(spans) and all(0 <= u < v <= T for u, v in spans)
    if T >= 257:
        assert {(0, T), (192, T), (255, T), (256, T), (T - 66, T - 1), (191, 257), (192, min(258, T))} <= set(spans)
        assert max(v - u - 1 for u, v in spans) // 64 + 1 == -(-T // 64)         # a chain of as many tiles as the trajectory has
    items = [item for item in DWC.WIDE_CASES if item[0] == case]
    windows = [w for item in items for w in DWC.wide_windows(item)]
    assert windows == [(u, v, target) for u, v in spans for target in DEC.WIDE_TARGETS[S]] and [item[1] for item in items] == list(range(len(items)))
    values = np.concatenate([DWC.wide_answer(item)['log_all'] for item in items])
    for item in items:
        want = DWC.wide_answer(item)
        assert want['n_nan_windows'] == 0 and np.isfinite(want['logev']) and DWC.ORACLE_SECONDS[item] < 20
    assert values.shape == (len(windows),) and not np.any(np.isnan(values)) and np.all(values <= 1e-12)
    print(f"{case}: {len(items)} parts, {len(windows)} windows, {int(np.sum(values == -np.inf))} at -inf, slowest part "
          f"{max(DWC.ORACLE_SECONDS[item] for item in items):.2f} s")
    assert (int(np.sum(values > -np.inf)), int(np.sum(values == -np.inf))) == WIDE_FINITE[case] and WIDE_FINITE[case][0] > 0
    empty = {w for w, v in zip(windows, values) if v == -np.inf}
    if kind in ('bounded', 'one_start', 'flip'):    # the oracle decides which windows are -inf, and there are some
        assert empty
    if kind == 'flip':      # every window of two or more frames: the case keeps its one-frame windows
        assert empty == {w for w in windows if w[1] - w[0] > 1} and any(w[1] - w[0] == 1 for w in windows)
    if kind == 'one_start':
        assert empty == {w for w in windows if w[0] == 0 and S - 1 not in w[2]}
    if kind == 'bounded':   # a window in one state longer than the bound
        assert {w for w in windows if len(w[2]) == 1 and w[1] - w[0] > DC.BOUND} <= empty
    if case == (2, 130, (), 'bounded'):
        more = [(0, 130, (1,)), (0, 129, (1,)), (1, 130, (1,)), (3, 129, (1,)), (63, 128, (1,))]
        got = DW.solve(W, F, prior, more)['log_all']
        assert np.all(got[:4] == -np.inf) and np.isfinite(got[4]) and (63, 128, (1,)) in windows and (0, 130, (1,)) in empty


def test_gpu_ragged_batch_meets_its_conditions():
    _, _, xs, _ = DC.ragged_case()
    counts = []
    for j, x in enumerate(xs):
        T = len(x)
        windows, want = DWC.ragged_windows(T), DWC.ragged_answer(j)
        assert all(0 <= u < v <= T and target in DEC.RAGGED_TARGETS for u, v, target in windows)
        assert want['n_nan_windows'] == 0 and np.isfinite(want['logev']) and np.all(np.isfinite(want['log_all'])) and len(want['log_all']) == len(windows)
        assert DWC.ORACLE_SECONDS['ragged', j] < 20
        counts.append(len(windows))
    assert counts == [2, 42, 14, 38, 6, 18]       # T = 1 and T = 2 get only what fits


def test_gpu_wide_siblings_are_wide_cases():
    import test_gpu_dwell_windows as GW
    assert all(len(t) == 1 and t[0] in DEC.WIDE and t[0][0] == 4 for t in GW.WIDE_SIBLINGS) and 4 in DWC.TARGETS
    assert DWC.TARGETS[4] == DEC.WIDE_TARGETS[4] and set(DWC.TARGETS[2]) == set(DEC.WIDE_TARGETS[2]) and set(DWC.TARGETS[3]) < set(DEC.WIDE_TARGETS[3])


# ---------------------------------------------------------------- the binding against include/bild_amd_windows.h

def windows_header():
    """ include/bild_amd_windows.h without its comments: ({struct: fields}, {function: (return type, parameters)}) """
    text = open(os.path.join(AH.ROOT, 'include', 'bild_amd_windows.h')).read()
    text = re.sub(r'//[^\n]*', '', re.sub(r'/\*.*?\*/', '', text, flags=re.S))
    structs = {tag: [f for part in body.split(';') if part.strip() for f in AH._declarations(part)]
               for tag, body, name in re.findall(r'typedef\s+struct\s+(bild_\w+_out)\s*\{(.*?)\}\s*(\w+)\s*;', text, flags=re.S) if tag == name}
    text = re.sub(r'typedef\s+struct\s*\w*\s*\{.*?\}\s*\w+\s*;', '', text, flags=re.S)
    text = '\n'.join(line for line in text.splitlines() if not line.lstrip().startswith('#'))
    prototypes = {name: (' '.join(ret.split()), [AH._declarations(a)[0] for a in args.split(',')])
                  for ret, name, args in re.findall(r'([\w\s*]+?)\b(bild_\w+)\s*\(([^()]*)\)\s*;', text)}
    return structs, prototypes


def test_binding_matches_the_new_header(monkeypatch):
    structs, prototypes = windows_header()
    assert list(structs) == ['bild_dwell_windows_out'] and list(prototypes) == ['bild_gauss_dwell_windows'] == list(_lib._SIGNATURES_EXT)
    assert '#include "bild_amd.h"' in open(os.path.join(AH.ROOT, 'include', 'bild_amd_windows.h')).read()
    # the first table and what it exports stay those of include/bild_amd.h
    assert not set(_lib._SIGNATURES_EXT) & set(_lib._SIGNATURES) and _lib.exported_symbols() == list(_lib._SIGNATURES)
    fields = structs['bild_dwell_windows_out']
    assert [f[0] for f in _lib.DwellWindowsOut._fields_] == [f[0] for f in fields] == ['logev', 'log_all', 'n_nan_windows']
    assert all(f[1] is ctypes.c_void_p for f in _lib.DwellWindowsOut._fields_) and all(f[2] for f in fields)
    ret, params = prototypes['bild_gauss_dwell_windows']
    restype, argtypes = _lib._SIGNATURES_EXT['bild_gauss_dwell_windows']
    assert ret == 'int' and restype is ctypes.c_int and len(argtypes) == len(params) == 16
    for (pname, ctype, pointer), t in zip(params, argtypes):
        assert AH._is_pointer(t) if pointer else t is AH.SCALARS[ctype], pname
    assert [p[0] for p in params] == ['m', 'ts', 'L', 'log_init', 'log_jump', 'log_dwell', 'log_surv', 'T_max', 'scratch_bytes', 'n_win',
                                      'win_traj', 'win_u', 'win_v', 'win_target', 'flags', 'out']
    assert {p[0]: p[1] for p in params if p[0].startswith('win_')} == {'win_traj': 'int32_t', 'win_u': 'int32_t', 'win_v': 'int32_t',
                                                                       'win_target': 'uint32_t'}

    # the wrapper on a recorder in place of the library: every argument at the position the header names
    rec = AH.Recorder()
    monkeypatch.setattr(_lib, 'lib', lambda: rec)
    S, T, L = 2, [1, 5], 5
    model = types.SimpleNamespace(_h=0x1000, S=S, d=1, Tmax=7)
    ts = types.SimpleNamespace(_h=0x2000, n_traj=len(T), T=np.array(T, dtype=np.int32))
    tables = (np.zeros(S), np.zeros((S, S)), np.zeros((S, L)), np.zeros((S, L)))
    traj, u, v = np.array([0, 1, 1], dtype=np.int32), np.array([0, 0, 2], dtype=np.int32), np.array([1, 5, 4], dtype=np.int32)
    target = np.array([1, 2, 1], dtype=np.uint32)
    for omit, scratch in ((True, 31), (False, 0)):
        res = _lib.gauss_dwell_windows(model, ts, *tables, traj, u, v, target, omit=omit, scratch_bytes=scratch)
        name, args = rec.calls[-1]
        assert name == 'bild_gauss_dwell_windows' and len(args) == len(params)
        named = dict(zip([p[0] for p in params], args))
        given = dict(m=model._h, ts=ts._h, L=L, T_max=max(T), scratch_bytes=scratch, n_win=3, flags=int(omit), log_init=tables[0],
                     log_jump=tables[1], log_dwell=tables[2], log_surv=tables[3], win_traj=traj, win_u=u, win_v=v, win_target=target)
        for key, want in given.items():
            got = named[key]
            if isinstance(want, np.ndarray):
                assert got == want.ctypes.data, key
            else:
                assert got == want and type(got) is type(want), (key, got)
        spec = named['out']._obj
        assert type(spec) is _lib.DwellWindowsOut and list(res) == [f[0] for f in fields]
        for field, ctype, _ in fields:
            assert res[field].dtype == AH.DTYPES[ctype] and getattr(spec, field) == res[field].ctypes.data, field
        assert res['logev'].shape == (2,) and res['log_all'].shape == (3,) and res['n_nan_windows'].shape == (2,)
    assert len(rec.calls) == 2
