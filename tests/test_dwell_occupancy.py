"""
The exact posterior of the looped time under a dwell-time prior without a GPU (bild_amd.exact.exact_dwell_occupancy,
DESIGN.md section 28): the NumPy oracle tests/dwell_occupancy_oracle.py against the enumeration of every profile on the cases
of tests/test_dwell.py, its identities against `dwell_oracle.solve` and `dwell_event_oracle.solve`, the support under the
minimum-length prior, `DwellOccupancy`'s derived numbers, `ExactDwellDraws.occupancy` on hand-made states,
`pooled_occupancy`, and the argument errors.
"""
import numpy as np
import pytest

import bild_amd
import dwell_cases as DC
import dwell_event_cases as DEC
import dwell_event_oracle as DE
import dwell_occupancy_cases as DQC
import dwell_occupancy_oracle as DQ
import dwell_oracle as DO
import segment_cases as C
import test_dwell as TD
from bild_amd import _lib

# the issue's bound against enumeration and on the identities, the siblings' CPU bound
TOL = 1e-12

TARGETS = {2: ((1,),), 3: ((2,), (0, 2))}


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


def result(answer, model, prior, x, target):
    """ the oracle's answer as the `DwellOccupancy` that the device call would return """
    return bild_amd.DwellOccupancy(traj=x, model=model, prior=prior, nan='propagate', target=tuple(target), log_evidence=answer['logev'],
                                   n_nan_windows=answer['n_nan_windows'], log_occupancy=answer['log_occupancy'])


def identities(W, F, prior, target, model, x, nan='propagate'):
    """ the identities of section 28 against `dwell_oracle.solve`'s marginals and `dwell_event_oracle.solve`'s never """
    S, T = F.shape[0], F.shape[1] - 1
    rest = tuple(s for s in range(S) if s not in target)
    got, other = DQ.solve(W, F, prior, target, nan=nan), DQ.solve(W, F, prior, rest, nan=nan)
    ref = DO.solve(W, F, prior, nan=nan)
    post = np.exp(ref['log_post'])
    r, c = result(got, model, prior, x, target), result(other, model, prior, x, rest)
    pmf = r.pmf()
    assert pmf.shape == (T + 1,) and np.array_equal(r.fraction(), np.arange(T + 1) / T)
    devs = {'sum pmf = 1': abs(pmf.sum() - 1),
            'mean = sum of the marginals over G': abs(r.mean() - post[list(target)].sum()),
            'sum_n occupancy = last marginal': np.max(np.abs(np.exp(got['log_occupancy']).sum(axis=0) - post[:, T - 1])),
            'pmf[0] = never in G': abs(pmf[0] - np.exp(DE.solve(W, F, prior, target=target, nan=nan)['log_never'])),
            'pmf[T] = never outside G': abs(pmf[T] - np.exp(DE.solve(W, F, prior, target=rest, nan=nan)['log_never'])),
            'complement reversed': np.max(np.abs(c.pmf()[::-1] - pmf))}
    print(f"{target}: " + ', '.join(f"{k}: {v:.1e}" for k, v in devs.items()))
    for name, v in devs.items():
        assert v < TOL, (name, v)
    assert abs(got['logev'] - ref['logev']) < TOL


@pytest.mark.parametrize('kind', ['markov', 'nongeometric', 'minlength'])
@pytest.mark.parametrize('name', [n for n in TD.CASES if 'order0' not in n])
def test_oracle_against_enumeration_and_identities(name, kind):
    model, x, prior = TD.build(name, kind)
    S, T = TD.CASES[name][:2]
    W, F = C.tables(model, x)
    for target in TARGETS[S]:
        got, want = DQ.solve(W, F, prior, target), DQ.enumerate_all(W, F, prior, target)
        assert got['n_nan_windows'] == 0 and want['n_nan'] == 0 and got['log_occupancy'].shape == (T + 1, S)
        assert abs(got['logev'] - want['logev']) < TOL
        worst = close_logs(got['log_occupancy'], want['log_occupancy'], (name, kind, target))
        print(f"{target}: worst deviation of a log from the enumeration {worst:.1e}")
        identities(W, F, prior, target, model, x)


@pytest.mark.parametrize('name', [n for n in DEC.SMALL if DEC.SMALL[n][0] > 1])
def test_oracle_against_enumeration_at_four_states_and_hard_priors(name):
    """ the oracle is the statement at these shapes too: `dwell_event_cases.SMALL`, every target of S, one frame missing """
    S, T, gap, kind = DEC.SMALL[name]
    model, x, prior, W, F = DEC.small_case(name)
    assert model.nStates == prior.nStates == S and np.array_equal(np.flatnonzero(np.isnan(x[:, 0])), [gap]) and F.shape == (S, T + 1)
    n_inf = 0
    for target in DEC.SMALL_TARGETS[S]:
        got, want = DQ.solve(W, F, prior, target), DQ.enumerate_all(W, F, prior, target)
        assert got['n_nan_windows'] == 0 and want['n_nan'] == 0 and got['log_occupancy'].shape == (T + 1, S)
        assert np.isfinite(want['logev']) and abs(got['logev'] - want['logev']) < TOL
        worst = close_logs(got['log_occupancy'], want['log_occupancy'], (name, target))
        print(f"{target}: worst deviation of a log from the enumeration {worst:.1e}")
        identities(W, F, prior, target, model, x)
        assert np.array_equal(got['log_occupancy'] > -np.inf, DQ.prior_support(prior, target, S, T)), target
        n_inf += int(np.sum(got['log_occupancy'] == -np.inf))
    print(f"{name}: {n_inf} entries at -inf")
    assert n_inf > 0        # (n = 0 and n = T end in one state set alone, under every prior)
    if kind == 'flip':      # the states alternate: T / 2 frames in either, T even
        assert T % 2 == 0 and np.all(np.isfinite(got['log_occupancy'][T // 2])) and np.all(np.delete(got['log_occupancy'], T // 2, axis=0) == -np.inf)


@pytest.mark.parametrize('kind', ['markov', 'nongeometric', 'minlength'])
@pytest.mark.parametrize('nan', ['propagate', 'omit'])
def test_oracle_nan_windows_against_enumeration(nan, kind):
    model, x, prior = TD.build('s2_order0_inner_gap', kind)
    W, F = C.tables(model, x)
    got, want = DQ.solve(W, F, prior, (1,), nan=nan), DQ.enumerate_all(W, F, prior, (1,), nan=nan)
    assert got['n_nan_windows'] == DO.solve(W, F, prior, nan=nan)['n_nan_windows'] > 0 and want['n_nan'] > 0
    if nan == 'propagate':
        assert np.isnan(got['logev']) and np.all(np.isnan(got['log_occupancy'])) and np.all(np.isnan(want['log_occupancy']))
        return
    assert abs(got['logev'] - want['logev']) < TOL
    close_logs(got['log_occupancy'], want['log_occupancy'], (nan, kind))
    identities(W, F, prior, (1,), model, x, nan=nan)


@pytest.mark.parametrize('name', [n for n in TD.CASES if 'order0' not in n])
def test_support_under_the_minimum_length_prior(name):
    """
    The minimum-length prior gives weight 0 to a completed segment of one frame and to nothing else (the last segment is
    censored and may have one frame).  With two states, both allowed at the start, and G = {1}: a profile that ends in G is one
    segment (n = T), or has its T - n frames outside G in completed segments, T - n >= 2, and n >= 1; so n = T - 1 and n = 0
    are out.  A profile that ends outside G mirrors that: n = 0 or 2 <= n <= T - 1.  Three states (with the jump 0 -> 2
    forbidden): the support is listed from the prior's weights of every profile.  The likelihood excludes nothing, so the -inf
    pattern of the answer is the prior's.
    """
    model, x, prior = TD.build(name, 'minlength')
    S, T = TD.CASES[name][:2]
    W, F = C.tables(model, x)
    for target in TARGETS[S]:
        support = DQ.prior_support(prior, target, S, T)
        if S == 2:
            n = np.arange(T + 1)
            assert np.array_equal(support[:, 1], (n == T) | ((n >= 1) & (n <= T - 2)))
            assert np.array_equal(support[:, 0], (n == 0) | ((n >= 2) & (n <= T - 1)))
        assert not support.all() and support.any(axis=0).all()
        got, want = DQ.solve(W, F, prior, target), DQ.enumerate_all(W, F, prior, target)
        assert np.array_equal(got['log_occupancy'] > -np.inf, support), target
        assert np.array_equal(want['log_occupancy'] > -np.inf, support), target


def hand_made(occ, target=(1,)):
    with np.errstate(divide='ignore'):
        return bild_amd.DwellOccupancy(traj=np.zeros((len(occ) - 1, 1)), model=None, prior=None, nan='propagate', target=target,
                                       log_evidence=0.0, n_nan_windows=0, log_occupancy=np.log(np.asarray(occ, dtype=float)))


def test_derived_numbers_on_a_hand_made_pmf():
    # T = 4: P(N = n) = 0.1, 0.2, 0.4, 0.25, 0.05, split over two last states
    r = hand_made([[0.1, 0.0], [0.05, 0.15], [0.3, 0.1], [0.0, 0.25], [0.0, 0.05]])
    assert np.allclose(r.pmf(), [0.1, 0.2, 0.4, 0.25, 0.05], atol=1e-15)
    assert np.allclose(r.cdf(), [0.1, 0.3, 0.7, 0.95, 1.0], atol=1e-15)
    assert np.array_equal(r.fraction(), [0.0, 0.25, 0.5, 0.75, 1.0])
    mean = 0.2 + 0.8 + 0.75 + 0.2
    assert abs(r.mean() - mean) < 1e-15
    assert abs(r.var() - (0.2 + 1.6 + 2.25 + 0.8 - mean ** 2)) < 1e-14
    # the smallest n whose cdf reaches the tail's share: 0.025 -> 0 and 0.975 -> 4; 0.2 -> 1 and 0.8 -> 3; 0.35 -> 2 and 0.65 -> 2
    assert r.interval() == (0, 4) and r.interval(0.6) == (1, 3) and r.interval(0.3) == (2, 2)
    assert r.interval(0.8) == (0, 3)        # 0.1 is reached at n = 0 (cdf = 0.1), 0.9 at n = 3
    spike = hand_made([[0.0, 0.0], [0.0, 0.0], [1.0, 0.0]])
    assert spike.interval() == (2, 2) and spike.mean() == 2.0 and spike.var() == 0.0
    for level in (0, 1, -0.5, 1.5):
        with pytest.raises(ValueError):
            r.interval(level)
    with pytest.raises(ValueError):
        hand_made([[np.nan, np.nan], [np.nan, np.nan]]).interval()
    assert 'target=(1,)' in repr(r) and 'T=4' in repr(r)


def test_occupancy_of_draws_on_hand_made_states():
    states = np.array([[0, 0, 1, 1, 0, 255], [1, 0, 0, 0, 0, 255], [0, 0, 0, 0, 0, 255], [0, 2, 2, 1, 0, 255], [2, 1, 1, 1, 1, 255]],
                      dtype=np.uint8)
    n = len(states)
    draws = bild_amd.ExactDwellDraws(5, states, np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n), None)
    for target, want in ((1, [2, 1, 0, 1, 4]), ([1], [2, 1, 0, 1, 4]), ((1, 2), [2, 1, 0, 3, 5]), ({2}, [0, 0, 0, 2, 1]),
                         (0, [3, 4, 5, 2, 0]), (3, [0] * 5), (255, [0] * 5)):      # (a state that never occurs; the padding behind T)
        got = draws.occupancy(target)
        assert got.dtype == np.int64 and got.tolist() == want, target
    empty = bild_amd.ExactDwellDraws(5, np.zeros((0, 5), dtype=np.uint8), np.zeros(0), np.zeros(0), np.zeros(0), np.zeros(0), None)
    assert empty.occupancy(1).shape == (0,)


def test_pooled_occupancy():
    a = hand_made([[0.1, 0.0], [0.05, 0.15], [0.3, 0.1], [0.0, 0.3]])
    b = hand_made([[0.2, 0.2], [0.0, 0.5], [0.1, 0.0]])
    want = np.zeros(3 + 2 + 1)
    for i, p in enumerate(a.pmf()):
        for j, q in enumerate(b.pmf()):
            want[i + j] += p * q
    got = bild_amd.pooled_occupancy([a, b])
    assert got.shape == (6,) and np.max(np.abs(got - want)) < 1e-15 and abs(got.sum() - 1) < 1e-15
    assert np.max(np.abs(bild_amd.pooled_occupancy([b, a]) - want)) < 1e-15
    assert np.array_equal(bild_amd.pooled_occupancy([a]), a.pmf())
    assert np.array_equal(bild_amd.pooled_occupancy(iter([a])), a.pmf())
    with pytest.raises(ValueError, match='no result'):
        bild_amd.pooled_occupancy([])
    with pytest.raises(ValueError, match='differing targets'):
        bild_amd.pooled_occupancy([a, hand_made([[0.5, 0.5], [0.0, 0.0]], target=(0,))])
    with pytest.raises(ValueError, match='NaN'):
        bild_amd.pooled_occupancy([a, hand_made([[np.nan, np.nan], [np.nan, np.nan]])])


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
    call = bild_amd.exact_dwell_occupancy
    for other in (rouse, factorized):
        with pytest.raises(TypeError):
            call(x, other, prior, 1)
    with pytest.raises(TypeError):
        call(x, model, (prior.log_init, prior.log_jump), 1)
    with pytest.raises(ValueError):
        call(x, model, prior, 1, nan='drop')
    with pytest.raises(ValueError):         # the tables are shorter than the trajectory
        call(x, model, DC.symmetric_chain(0.1, 19), 1)
    with pytest.raises(ValueError):         # the states do not match
        call(x, model, DC.make_prior('markov', rng, 3, 20), 1)
    with pytest.raises(ValueError):         # beyond the model's lags
        call(C.random_traj(rng, 30), model, DC.symmetric_chain(0.1, 40), 1)
    with pytest.raises(ValueError):         # more states than the recursion supports
        call(x, C.random_model(rng, 5, 24), DC.make_prior('markov', rng, 5, 20), 1)
    for target in ((), [], (0, 1), [1, 0, 1], 2, -1, (1, 2), 1.0, True, (0.5,)):     # empty, full, out of range, not a state
        with pytest.raises(ValueError):
            call(x, model, prior, target)
    one = C.random_model(rng, 1, 24)            # one state has no proper subset
    with pytest.raises(ValueError):
        call(x, one, DC.make_prior('markov', rng, 1, 20), 0)
    assert call([], model, prior, 1) == []
    with pytest.raises(ValueError):
        call([], model, prior, 2)


# ---------------------------------------------------------------- the conditions on the inputs of the wide GPU cases

# per wide case and target, in the order of `dwell_event_cases.WIDE_TARGETS`, the finite entries of log_occupancy that the oracle
# gives, of (T + 1) S.  Listed, so that a change of a generator that empties a comparison is seen here.
WIDE_FINITE = {
    (4, 64, (), 'minlength'): (252, 252, 252), (4, 129, (64, 100), 'markov'): (516, 516, 516),
    (4, 257, (100,), 'nongeometric'): (1028, 1028, 1028), (2, 256, (), 'markov'): (512, 512), (2, 257, (255,), 'minlength'): (512, 512),
    (3, 321, (128,), 'markov'): (963, 963, 963), (2, 65, (), 'nongeometric'): (130, 130), (3, 193, (3,), 'nongeometric'): (579, 579, 579),
    (2, 130, (), 'bounded'): (256, 256), (3, 193, (), 'bounded'): (573, 570, 570), (2, 65, (), 'one_start'): (128, 128),
    (3, 130, (20,), 'absorbing'): (132, 390, 390), (2, 70, (), 'flip'): (2, 2),
}


@pytest.mark.parametrize('case', [c for c in DEC.WIDE if c[0] > 1], ids=DEC.wide_id)
def test_gpu_wide_cases_meet_their_conditions(case):
    """ what tests/test_gpu_dwell_occupancy.py compares the device with is what it is meant to be, and no comparison is vacuous """
    S, T, missing, kind = case
    model, x, prior, W, F = DC.oracle_case(case)
    assert model.nStates == prior.nStates == S and x.shape == (T, 2) and prior.L == T + 5
    assert np.array_equal(np.flatnonzero(np.isnan(x[:, 0])), missing)
    targets = DEC.WIDE_TARGETS[S]
    assert [item for item in DQC.WIDE_CASES if item[0] == case] == [(case, target) for target in targets]
    assert len(WIDE_FINITE[case]) == len(targets)
    for target, finite in zip(targets, WIDE_FINITE[case]):
        want = DQC.wide_answer(case, target)
        occ = want['log_occupancy']
        assert want['n_nan_windows'] == 0 and np.isfinite(want['logev']) and occ.shape == (T + 1, S) and not np.any(np.isnan(occ))
        assert abs(np.exp(occ).sum() - 1) < 1e-10
        print(f"{case} {target}: oracle {DQC.ORACLE_SECONDS[case, target]:.1f} s, {finite} of {(T + 1) * S} entries finite")
        assert DQC.ORACLE_SECONDS[case, target] < 20
        # n = 0 ends outside the target and n = T inside it, so every case compares entries at -inf as well as finite ones;
        # the hard priors empty more than those 2 S rows' worth
        assert 0 < int(np.sum(occ > -np.inf)) == finite <= (T + 1) * S - S
    if kind in DEC.HARD:    # (under some target; 'absorbing' under (2,))
        assert min(WIDE_FINITE[case]) < (T + 1) * S - S
    if kind == 'absorbing':     # state 2 is never left: n frames in it, ending elsewhere, is n = 0 alone
        assert np.all(DQC.wide_answer(case, (2,))['log_occupancy'][1:, :2] == -np.inf)
    if kind == 'flip':
        assert np.all(np.isfinite(DQC.wide_answer(case, (1,))['log_occupancy'][T // 2])) and T % 2 == 0


def test_gpu_ragged_batch_meets_its_conditions():
    _, _, xs, _ = DC.ragged_case()
    for j, x in enumerate(xs):
        T = len(x)
        for target in DEC.RAGGED_TARGETS:
            want = DQC.ragged_answer(j, target)
            occ = want['log_occupancy']
            assert want['n_nan_windows'] == 0 and np.isfinite(want['logev']) and occ.shape == (T + 1, 4) and not np.any(np.isnan(occ))
            # non-geometric tables exclude nothing: -inf is n = 0 ending in the target, n = T ending outside it, and nothing else
            inside = np.isin(np.arange(4), target)
            empty = np.zeros((T + 1, 4), dtype=bool)
            empty[0, inside] = empty[T, ~inside] = True
            assert np.array_equal(occ == -np.inf, empty)
            assert DQC.ORACLE_SECONDS['ragged', j, target] < 20
