"""
Exact fixed-lag smoothing under a dwell-time prior without a GPU (bild_amd.exact.exact_dwell_lag): the
NumPy oracle tests/dwell_lag_oracle.py against `dwell_oracle.solve` on every truncation x[:u] of a trajectory (the tables rebuilt
from the truncated data), its identities, `settling_lag`, the refusals, and the conditions on the inputs of the GPU test's cases
(tests/dwell_lag_cases.py), whose oracle answers are computed here as there.  Notes: tests/README_dwell_lag.md.
"""
import functools

import numpy as np
import pytest
from scipy.special import logsumexp

import bild_amd
import dwell_cases as DC
import dwell_filter_cases as FC
import dwell_filter_oracle as FO
import dwell_lag_cases as LC
import dwell_lag_oracle as LO
import dwell_oracle as DO
import segment_cases as C
from bild_amd import _lib
from bild_amd import exact

# the issue's bound; observed on these cases: at most 4e-14
TOL = 1e-12

SHAPES = [(2, 12, ()), (3, 20, (7,))]
KINDS = ('markov', 'minlength', 'nongeometric', 'bounded')
TRUNCATION_CASES = [shape + (kind, lag) for shape in SHAPES for kind in KINDS for lag in (0, 3, shape[1] + 2)]
TRUNCATION_CASES.append((2, 80, (), 'bounded', 10))     # (the bound of 70 frames bites beyond T = 70 only)


def build(S, T, missing, kind):
    rng = np.random.default_rng(100 * S + T + len(kind))
    model = C.random_model(rng, S, T + 8)
    x = C.random_traj(rng, T, missing)
    return model, x, DC.prior_of(kind, rng, S, T + 5, T)


@functools.lru_cache(maxsize=None)
def truncation_answers(S, T, missing, kind):
    """ `dwell_oracle.solve` of every x[:u], the tables rebuilt from the truncated data: shared by the lags of a shape """
    model, x, prior = build(S, T, missing, kind)
    return [DO.solve(*C.tables(model, x[:u]), prior) for u in range(1, T + 1)]


def against_truncations(got, cuts, lag):
    """ every (t, l) of `got` against frame t of the truncation's answer cuts[u - 1]; returns the worst deviation """
    S, T, n = got['log_lagged'].shape
    assert n == lag + 1
    worst = 0.0
    for t in range(T):
        assert got['n_nan_windows'][t] == cuts[t]['n_nan_windows'], t
        for l in range(lag + 1):
            a, ref = got['log_lagged'][:, t, l], cuts[LC.cut_of(T, t, l) - 1]['log_post'][:, t]
            fin = np.isfinite(ref)
            assert np.array_equal(a[~fin], ref[~fin], equal_nan=True), (t, l, a, ref)
            if fin.any():
                worst = max(worst, float(np.max(np.abs(a[fin] - ref[fin]))))
    return worst


@pytest.mark.parametrize('S,T,missing,kind,lag', TRUNCATION_CASES)
def test_oracle_against_truncation(S, T, missing, kind, lag):
    model, x, prior = build(S, T, missing, kind)
    got = LO.solve(*C.tables(model, x), prior, lag)
    assert np.all(got['n_nan_windows'] == 0) and not np.isnan(got['log_lagged']).any()
    worst = against_truncations(got, truncation_answers(S, T, missing, kind), lag)
    print(worst)
    assert worst < TOL


@pytest.mark.parametrize('nan', ['propagate', 'omit'])
def test_oracle_against_truncation_gap(nan):
    model, x, prior, W, F = FC.gap_case()
    T = len(x)
    got = LC.gap_answer(nan)
    cuts = [DO.solve(*C.tables(model, x[:u]), prior, nan=nan) for u in range(1, T + 1)]
    worst = against_truncations(got, cuts, LC.GAP_LAG)
    print(worst, got['n_nan_windows'])
    assert worst < TOL
    assert np.array_equal(got['n_nan_windows'], FC.gap_answer(nan)['n_nan_windows'])
    bad = got['n_nan_windows'] > 0
    assert bad.any() and not bad[:60].any()
    # NaN exactly where the entry's truncation has skipped a window, under 'propagate'; nowhere under 'omit'
    cut_bad = np.array([[bad[LC.cut_of(T, t, l) - 1] for l in range(LC.GAP_LAG + 1)] for t in range(T)])
    want = cut_bad if nan == 'propagate' else np.zeros_like(cut_bad)
    assert np.array_equal(np.isnan(got['log_lagged']), np.broadcast_to(want, (2,) + want.shape))
    # a frame before the gap is NaN in its late columns alone
    assert nan == 'omit' or (cut_bad.any(axis=1) & ~cut_bad.all(axis=1)).any()


@pytest.mark.parametrize('S,T,missing,kind', [(2, 30, (5,), 'nongeometric'), (3, 20, (7,), 'minlength'), (2, 80, (), 'bounded')])
def test_identities(S, T, missing, kind):
    model, x, prior = build(S, T, missing, kind)
    W, F = C.tables(model, x)
    lag = T + 1
    r = LO.solve(W, F, prior, lag)
    ll = r['log_lagged']
    assert ll.shape == (S, T, lag + 1)
    assert np.max(np.abs(logsumexp(ll, axis=0))) < TOL                      # every column is a distribution
    filt = FO.solve(W, F, prior)
    assert np.max(np.abs(ll[:, :, 0] - filt['log_filtered'])) < TOL         # column 0 is the filter
    assert np.array_equal(r['n_nan_windows'], filt['n_nan_windows'])
    assert np.max(np.abs(r['prefix_logev'] - filt['prefix_logev'])) < TOL
    full = DO.solve(W, F, prior)['log_post']
    fin = np.isfinite(full)
    for col in (T - 1, lag):                                                # with lag >= T - 1 the last column is the smoother
        assert np.array_equal(ll[:, :, col][~fin], full[~fin]) and np.max(np.abs(ll[:, :, col][fin] - full[fin])) < 1e-10
    for t in range(T):                                                      # the tail columns repeat
        first = T - 1 - t
        assert np.array_equal(ll[:, t, first:], np.repeat(ll[:, t, first:first + 1], lag + 1 - first, axis=1))
    for small in (0, 4):                                                    # a smaller lag gives the same leading columns
        s = LO.solve(W, F, prior, small)['log_lagged']
        both = np.isfinite(s)
        assert np.array_equal(both, np.isfinite(ll[:, :, :small + 1])) and np.max(np.abs(s[both] - ll[:, :, :small + 1][both])) < TOL


def test_one_state_is_all_zeros():
    model, x, prior = build(1, 15, (4,), 'nongeometric')
    assert np.all(LO.solve(*C.tables(model, x), prior, 6)['log_lagged'] == 0)


@pytest.mark.parametrize('case,lag', LC.GPU_CASES)
def test_gpu_cases_meet_their_conditions(case, lag):
    """
    Some frame's columns 0, 1 and `lag` differ pairwise by more than 1e-3 in probability, so that a shifted column cannot pass.
    The columns of one frame that speak of the same truncation are equal by definition: columns 1 and `lag` at lag = 1, and at
    T = 2 every column behind the first; so the condition is asked of the different truncations among the three, at a frame
    where they are as many as the trajectory allows.  Nothing can differ at lag 0 and at T = 1 (one column, one truncation), at
    S = 1 (every entry is 0) and under 'impossible' (one profile before the last cut, none at it).
    """
    S, T, missing, kind = case
    want = LC.oracle_answer(case, lag)
    print(f"{case} lag {lag}: oracle {LC.ORACLE_SECONDS[case, lag]:.1f} s")
    assert LC.ORACLE_SECONDS[case, lag] < 20
    ll = want['log_lagged']
    assert ll.shape == (S, T, lag + 1) and np.all(want['n_nan_windows'] == 0)
    if kind == 'impossible':
        # every entry whose truncation is the whole trajectory is NaN, the others hold the one profile
        whole = np.array([[LC.cut_of(T, t, l) == T for l in range(lag + 1)] for t in range(T)])
        assert np.array_equal(np.isnan(ll), np.broadcast_to(whole, ll.shape)) and whole.any() and not whole.all()
        assert np.all(ll[0][~whole] == 0) and np.all(ll[1][~whole] == -np.inf)
        return
    assert not np.isnan(ll).any() and np.max(np.abs(logsumexp(ll, axis=0))) < TOL
    if S == 1:
        assert np.all(ll == 0)
        return
    step, n_cuts = LC.column_steps(ll, lag)
    print(f"columns 0, 1 and {lag}: {n_cuts} truncations, smallest pairwise step at the best frame {step:.3g}")
    assert n_cuts == min(3, T, lag + 1)
    if lag == 0 or T == 1:
        return
    assert step > 1e-3
    full = DC.oracle_answer(case)['log_post']           # the columns of the whole trajectory are the smoothed marginals
    for t in range(max(T - 1 - lag, 0), T):
        a = ll[:, t, T - 1 - t]
        fin = np.isfinite(full[:, t])
        assert np.array_equal(a[~fin], full[:, t][~fin]) and np.max(np.abs(a[fin] - full[:, t][fin]), initial=0.0) < 1e-10
    if kind == 'one_start':
        assert np.all(ll[:S - 1, 0, :] == -np.inf) and np.max(np.abs(ll[S - 1, 0, :])) < TOL


def test_gpu_ragged_batch_meets_its_conditions():
    model, prior, xs, tabs = DC.ragged_case()
    for j, want in enumerate(LC.ragged_answers()):
        print(f"trajectory {j}: oracle {LC.ORACLE_SECONDS['ragged', j]:.1f} s")
        assert LC.ORACLE_SECONDS['ragged', j] < 20
        T = len(xs[j])
        assert want['log_lagged'].shape == (4, T, LC.RAGGED_LAG + 1) and np.all(want['n_nan_windows'] == 0)
        assert not np.isnan(want['log_lagged']).any()
        if T > 2:
            assert LC.column_steps(want['log_lagged'], LC.RAGGED_LAG)[0] > 1e-3


def test_gpu_gap_case_meets_its_conditions():
    omit, prop = LC.gap_answer('omit'), LC.gap_answer('propagate')
    assert LC.ORACLE_SECONDS['gap', 'omit'] < 20 and LC.ORACLE_SECONDS['gap', 'propagate'] < 20
    assert not np.isnan(omit['log_lagged']).any() and np.array_equal(omit['n_nan_windows'], prop['n_nan_windows'])
    bad = np.isnan(prop['log_lagged'])
    assert bad.any() and not bad.all() and np.array_equal(prop['log_lagged'][~bad], omit['log_lagged'][~bad])
    assert LC.column_steps(omit['log_lagged'], LC.GAP_LAG)[0] > 1e-3


def test_settling_lag():
    # two states, five frames, lag 3; the probabilities of state 0 per column
    p0 = np.array([[0.50, 0.50, 0.50, 0.50],        # settled from the start: 0
                   [0.10, 0.30, 0.3004, 0.30],      # within 1e-3 from column 1 on
                   [0.30, 0.10, 0.30, 0.20],        # only the last column: lag
                   [0.20, 0.40, 0.40, 0.40],        # 1
                   [0.70, 0.70, 0.70, 0.70]])
    with np.errstate(divide='ignore'):
        ll = np.log(np.stack([p0, 1 - p0]))
    ll[:, 4, 2] = np.nan                            # a NaN frame
    want = np.array([0, 1, 3, 1, -1])
    for fn in (exact.settling_lag, LO.settling_lag):
        got = fn(ll)
        assert got.dtype == np.int64 and np.array_equal(got, want), got
    assert np.array_equal(exact.settling_lag(ll, tol=0.15), [0, 1, 0, 1, -1])
    assert np.array_equal(LO.settling_lag(ll, tol=0.15), [0, 1, 0, 1, -1])
    # a column that comes back within the tolerance and leaves again does not count
    back = np.log(np.stack([np.array([[0.3, 0.5, 0.3, 0.5, 0.3]]), np.array([[0.7, 0.5, 0.7, 0.5, 0.7]])]))
    assert np.array_equal(exact.settling_lag(back), [4]) and np.array_equal(LO.settling_lag(back), [4])
    r = bild_amd.DwellLagResults(traj=np.zeros((5, 2)), model=None, prior=None, nan='propagate', lag=3, log_evidence=0.0,
                                 log_lagged=ll, n_nan_windows=np.zeros(5, dtype=np.int64))
    assert np.array_equal(r.settling_lag(), want) and np.array_equal(r.fixed_lag(2), ll[:, :, 2], equal_nan=True)
    assert r.fixed_lag(0).shape == (2, 5)
    for lag in (-1, 4, 1.5):
        with pytest.raises(ValueError):
            r.fixed_lag(lag)


def test_refusals_come_before_any_upload(monkeypatch):
    def no_upload(*a, **k):
        raise AssertionError("a trajectory set was made")
    monkeypatch.setattr(_lib, 'GaussTrajSetHandle', no_upload)
    rng = np.random.default_rng(3)
    model = C.random_model(rng, 2, 24)
    x = C.random_traj(rng, 20)
    prior = DC.symmetric_chain(0.1, 20)
    smooth = bild_amd.exact_dwell_lag
    rouse = bild_amd.MultiStateRouse(8, 1, 5, d=2, localization_error=0.1)
    factorized = bild_amd.FactorizedModel([np.array([1.0, 2.0]), np.array([1.0, 4.0])], d=2)
    for other in (rouse, factorized):
        with pytest.raises(TypeError):
            smooth(x, other, prior, 3)
    with pytest.raises(TypeError):
        smooth(x, model, (prior.log_init, prior.log_jump), 3)
    with pytest.raises(ValueError):
        smooth(x, model, prior, 3, nan='drop')
    with pytest.raises(ValueError):         # the tables are shorter than the trajectory
        smooth(x, model, DC.symmetric_chain(0.1, 19), 3)
    with pytest.raises(ValueError):         # the states do not match
        smooth(x, model, DC.make_prior('markov', rng, 3, 20), 3)
    with pytest.raises(ValueError):         # beyond the model's lags
        smooth(C.random_traj(rng, 30), model, DC.symmetric_chain(0.1, 40), 3)
    five = C.random_model(rng, 5, 24)
    with pytest.raises(ValueError):
        smooth(x, five, DC.make_prior('markov', rng, 5, 20), 3)
    for lag in (-1, 2.5, 64):
        with pytest.raises(ValueError):
            smooth(x, model, prior, lag)
    assert smooth([], model, prior, 3) == []
    assert exact.MAX_DWELL_LAG == _lib.DWELL_LAG_MAX == LC.LAG_MAX == 63
    for lag in (0, 63):                     # (what is not refused goes on to the upload)
        with pytest.raises(AssertionError, match='a trajectory set was made'):
            smooth(x, model, prior, lag)
