"""
The exact online filter under a dwell-time prior without a GPU (bild_amd.exact.exact_dwell_filter): the
NumPy oracle tests/dwell_filter_oracle.py against `dwell_oracle.solve` on every truncation x[:b] of a trajectory (the tables
rebuilt from the truncated data), its identities, the refusals, and the conditions on the inputs of the GPU test's cases
(tests/dwell_filter_cases.py), whose oracle answers are computed here as there.  Notes: tests/README_dwell_filter.md.
"""
import numpy as np
import pytest
from scipy.special import logsumexp

import bild_amd
import dwell_cases as DC
import dwell_filter_cases as FC
import dwell_filter_oracle as FO
import dwell_oracle as DO
import segment_cases as C
from bild_amd import _lib

# the issue's bound; observed on these cases: at most 3e-14
TOL = 1e-12

SHAPES = [(2, 12, ()), (3, 20, (7,))]
TRUNCATION_CASES = [shape + (kind,) for shape in SHAPES for kind in ('markov', 'minlength', 'nongeometric', 'bounded')]
TRUNCATION_CASES.append((2, 80, (), 'bounded'))     # (the bound of 70 frames bites beyond T = 70 only)


def build(S, T, missing, kind):
    rng = np.random.default_rng(100 * S + T + len(kind))
    model = C.random_model(rng, S, T + 8)
    x = C.random_traj(rng, T, missing)
    return model, x, DC.prior_of(kind, rng, S, T + 5, T)


def against_truncations(model, x, prior, got, nan):
    """ every frame of the filter's answer `got` against `dwell_oracle.solve` of the tables of x[:b]; returns the worst deviations """
    worst = {'logev': 0.0, 'log_post': 0.0}
    for b in range(1, len(x) + 1):
        Wb, Fb = C.tables(model, x[:b])
        want = DO.solve(Wb, Fb, prior, nan=nan)
        assert got['n_nan_windows'][b - 1] == want['n_nan_windows'], b
        for name, a, ref in (('logev', got['prefix_logev'][b - 1], want['logev']),
                             ('log_post', got['log_filtered'][:, b - 1], want['log_post'][:, -1])):
            a, ref = np.atleast_1d(a), np.atleast_1d(ref)
            fin = np.isfinite(ref)
            assert np.array_equal(a[~fin], ref[~fin], equal_nan=True), (name, b, a, ref)
            if fin.any():
                worst[name] = max(worst[name], float(np.max(np.abs(a[fin] - ref[fin]))))
    return worst


@pytest.mark.parametrize('S,T,missing,kind', TRUNCATION_CASES)
def test_oracle_against_truncation(S, T, missing, kind):
    model, x, prior = build(S, T, missing, kind)
    W, F = C.tables(model, x)
    got = FO.solve(W, F, prior)
    assert np.all(got['n_nan_windows'] == 0) and np.all(np.isfinite(got['prefix_logev']))
    worst = against_truncations(model, x, prior, got, 'propagate')
    print(worst)
    assert worst['logev'] < TOL and worst['log_post'] < TOL


@pytest.mark.parametrize('nan', ['propagate', 'omit'])
def test_oracle_against_truncation_gap(nan):
    model, x, prior, W, F = FC.gap_case()
    got = FC.gap_answer(nan)
    worst = against_truncations(model, x, prior, got, nan)
    print(worst, got['n_nan_windows'])
    assert worst['logev'] < TOL and worst['log_post'] < TOL
    bad = got['n_nan_windows'] > 0
    assert bad.any() and not bad[:60].any() and np.all(np.diff(got['n_nan_windows']) >= 0)
    for name in ('prefix_logev', 'run_mean'):
        assert np.array_equal(np.isnan(got[name]), bad if nan == 'propagate' else np.zeros(70, dtype=bool))
    assert np.array_equal(np.isnan(got['log_filtered']).all(axis=0), np.isnan(got['prefix_logev']))
    assert np.array_equal(np.isnan(got['log_run']).all(axis=(0, 2)), np.isnan(got['prefix_logev']))


@pytest.mark.parametrize('S,T,missing,kind', [(2, 30, (5,), 'nongeometric'), (3, 20, (7,), 'minlength'), (2, 80, (), 'bounded')])
def test_identities(S, T, missing, kind):
    model, x, prior = build(S, T, missing, kind)
    W, F = C.tables(model, x)
    r = FO.solve(W, F, prior, run_max=T)
    assert np.max(np.abs(logsumexp(r['log_filtered'], axis=0))) < TOL
    run = np.exp(r['log_run'])
    assert run.shape == (S, T, T)
    assert np.max(np.abs(run.sum(axis=(0, 2)) - 1)) < TOL
    assert np.max(np.abs(np.tensordot(run.sum(axis=0), np.arange(1, T + 1), axes=1) - r['run_mean'])) < TOL * T
    assert np.max(np.abs(run.sum(axis=2) - np.exp(r['log_filtered']))) < TOL
    for t in range(T):      # no run is longer than the data
        assert np.all(r['log_run'][:, t, t + 1:] == -np.inf)
    # a shorter run_max cuts the same table
    short = FO.solve(W, F, prior, run_max=7)
    assert np.array_equal(short['log_run'], r['log_run'][:, :, :7]) and np.array_equal(short['run_mean'], r['run_mean'])


def test_flip_prior_has_runs_of_one_frame():
    model, x, prior = build(2, 20, (), 'flip')
    r = FO.solve(*C.tables(model, x), prior, run_max=20)
    assert np.max(np.abs(r['run_mean'] - 1)) < TOL
    assert np.max(np.abs(logsumexp(r['log_run'][:, :, 0], axis=0))) < TOL and np.all(r['log_run'][:, 1:, 1:] == -np.inf)


def test_markov_predictive_terms_add_up_to_the_evidence():
    """ tables consistent under truncation: the one-step terms are log-probabilities of one frame and sum to the evidence """
    model, x, prior = build(2, 30, (5,), 'markov')
    W, F = C.tables(model, x)
    r = FO.solve(W, F, prior)
    assert abs(np.sum(np.diff(r['prefix_logev'], prepend=0.0)) - DO.solve(W, F, prior)['logev']) < TOL


@pytest.mark.parametrize('S,T,missing,kind', FC.GPU_CASES)
def test_gpu_cases_meet_their_conditions(S, T, missing, kind):
    case = (S, T, missing, kind)
    model, x, prior, W, F = DC.oracle_case(case)
    assert model.nStates == prior.nStates == S and x.shape == (T, 2)
    assert np.array_equal(np.flatnonzero(np.isnan(x[:, 0])), missing)
    want = FC.oracle_answer(case)
    R = FC.run_max_of(T)
    print(f"{case}: oracle {FC.ORACLE_SECONDS[case]:.1f} s, run_max {R}")
    assert FC.ORACLE_SECONDS[case] < 20
    assert R == (T if T < 200 else 70) and want['log_run'].shape == (S, T, R)
    assert np.all(want['n_nan_windows'] == 0)
    full = DC.oracle_answer(case)
    if kind == 'impossible':    # every prefix but the whole trajectory has the profile of one segment
        assert np.all(np.isfinite(want['prefix_logev'][:-1])) and want['prefix_logev'][-1] == -np.inf == full['logev']
        assert np.all(np.isnan(want['log_filtered'][:, -1])) and np.isnan(want['run_mean'][-1]) and np.all(np.isnan(want['log_run'][:, -1]))
        assert np.array_equal(want['run_mean'][:-1], np.arange(1.0, T))
        return
    assert np.all(np.isfinite(want['prefix_logev'])) and abs(want['logev'] - full['logev']) < TOL
    last, ref = want['log_filtered'][:, -1], full['log_post'][:, -1]       # the last frame's filtered marginal is the smoothed one
    fin = np.isfinite(ref)
    assert np.array_equal(last[~fin], ref[~fin]) and np.max(np.abs(last[fin] - ref[fin])) < 1e-10
    assert np.max(np.abs(logsumexp(want['log_filtered'], axis=0))) < TOL
    assert np.all((want['run_mean'] >= 1 - TOL) & (want['run_mean'] <= np.arange(1, T + 1) + TOL))
    if kind == 'flip' and T > 1:
        assert np.max(np.abs(want['run_mean'] - 1)) < TOL
    if kind == 'bounded':
        assert np.all(want['log_run'][:, :, DC.BOUND:] == -np.inf) and want['run_mean'].max() <= DC.BOUND
    if kind == 'one_start':
        assert np.all(want['log_filtered'][:S - 1, 0] == -np.inf) and want['log_filtered'][S - 1, 0] == 0
    if S == 1:
        assert np.all(want['log_filtered'] == 0) and np.array_equal(want['run_mean'], np.arange(1.0, T + 1))


def test_gpu_ragged_batch_meets_its_conditions():
    model, prior, xs, tabs = DC.ragged_case()
    for j, (want, full) in enumerate(zip(FC.ragged_answers(), DC.ragged_answers())):
        print(f"trajectory {j}: oracle {FC.ORACLE_SECONDS['ragged', j]:.1f} s")
        assert FC.ORACLE_SECONDS['ragged', j] < 20
        assert np.all(want['n_nan_windows'] == 0) and np.all(np.isfinite(want['prefix_logev']))
        assert abs(want['logev'] - full['logev']) < TOL and want['log_run'].shape == (4, len(xs[j]), FC.RAGGED_RUN_MAX)


def test_gpu_gap_case_meets_its_conditions():
    model, x, prior, W, F = FC.gap_case()
    assert len(x) == 70 and np.array_equal(np.flatnonzero(np.isnan(x[:, 0])), np.arange(60, 68)) and not np.any(np.isnan(x[:, 1]))
    omit, prop = FC.gap_answer('omit'), FC.gap_answer('propagate')
    assert FC.ORACLE_SECONDS['gap', 'omit'] < 20 and FC.ORACLE_SECONDS['gap', 'propagate'] < 20
    # under 'omit' every prefix evidence is finite and the pass skips at least one window
    assert np.all(np.isfinite(omit['prefix_logev'])) and omit['nG'].sum() >= 1
    print('skipped under log_surv', int(omit['nG'].sum()), 'at end frames', np.flatnonzero(omit['nG']).tolist())
    assert np.array_equal(omit['n_nan_windows'], prop['n_nan_windows'])
    assert omit['n_nan_windows'][-1] == DO.solve(W, F, prior, nan='omit')['n_nan_windows'] > 0
    bad = prop['n_nan_windows'] > 0
    assert np.array_equal(np.isnan(prop['prefix_logev']), bad) and 0 < bad.sum() < 70
    assert np.array_equal(prop['prefix_logev'][~bad], omit['prefix_logev'][~bad])


def test_refusals_come_before_any_upload(monkeypatch):
    def no_upload(*a, **k):
        raise AssertionError("a trajectory set was made")
    monkeypatch.setattr(_lib, 'GaussTrajSetHandle', no_upload)
    rng = np.random.default_rng(3)
    model = C.random_model(rng, 2, 24)
    x = C.random_traj(rng, 20)
    prior = DC.symmetric_chain(0.1, 20)
    filt = bild_amd.exact_dwell_filter
    rouse = bild_amd.MultiStateRouse(8, 1, 5, d=2, localization_error=0.1)
    factorized = bild_amd.FactorizedModel([np.array([1.0, 2.0]), np.array([1.0, 4.0])], d=2)
    for other in (rouse, factorized):
        with pytest.raises(TypeError):
            filt(x, other, prior)
    with pytest.raises(TypeError):
        filt(x, model, (prior.log_init, prior.log_jump))
    with pytest.raises(ValueError):
        filt(x, model, prior, nan='drop')
    with pytest.raises(ValueError):         # the tables are shorter than the trajectory
        filt(x, model, DC.symmetric_chain(0.1, 19))
    with pytest.raises(ValueError):         # the states do not match
        filt(x, model, DC.make_prior('markov', rng, 3, 20))
    with pytest.raises(ValueError):         # beyond the model's lags
        filt(C.random_traj(rng, 30), model, DC.symmetric_chain(0.1, 40))
    five = C.random_model(rng, 5, 24)
    with pytest.raises(ValueError):
        filt(x, five, DC.make_prior('markov', rng, 5, 20))
    for run_max in (-1, 2.5):
        with pytest.raises(ValueError):
            filt(x, model, prior, run_max=run_max)
    assert filt([], model, prior) == []
    with pytest.raises(AssertionError, match='a trajectory set was made'):      # (what is not refused goes on to the upload)
        filt(x, model, prior, run_max=3)
