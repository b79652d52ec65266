"""
The dwell-time recursion without a GPU (bild_amd.exact.exact_dwell): the NumPy oracle
tests/dwell_oracle.py against the enumeration of every profile of every k, its identities, the symmetric two-state chain
against the segment recursion's oracle, `DwellPrior`, the refusals, and the conditions on the inputs of the GPU test's oracle
cases (`dwell_cases.ORACLE_CASES`, the ragged batch and the sharp case), whose oracle answers are computed here as there.
"""
import numpy as np
import pytest
from scipy.special import logsumexp

import bild_amd
import dwell_cases as DC
import dwell_oracle as DO
import gauss_oracle as G
import segment_cases as C
import segment_oracle as SO
from bild_amd import _lib

# the issue's bound; observed on these cases: logev 4e-15, log marginals 8e-15, counts 3e-14, MAP log joint 4e-15
TOL = 1e-12

# name: (S, T, missing frames, orders (None: ss_order 1 everywhere))
CASES = {
    's2_gapfree': (2, 10, (), None),
    's3_gapfree': (3, 8, (), None),
    's2_leading_gap': (2, 10, (0, 1), None),
    's3_leading_gap': (3, 8, (0, 1), None),
    's2_inner_gap': (2, 12, (4, 5, 6), None),
    's3_inner_gap': (3, 8, (3, 4), None),
    's2_order0_inner_gap': (2, 11, (4, 5, 6), [[0, 1], [1, 0]]),
}


def build(name, kind):
    S, T, missing, orders = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name + kind)))
    model = C.random_model(rng, S, T + 4, orders=np.ones((S, 2), dtype=int) if orders is None else orders)
    return model, C.random_traj(rng, T, missing), DC.make_prior(kind, rng, S, T + 3)


def compare(got, want, same_map):
    for name in ('logev', 'map_logjoint'):
        a, b = got[name], want[name]
        if np.isfinite(b):
            assert abs(a - b) < TOL, (name, a, b)
        else:
            assert np.array_equal(a, b, equal_nan=True), (name, a, b)
    for name in ('log_post', 'exp_jumps', 'exp_stay'):
        a, b = got[name], want[name]
        fin = np.isfinite(b)
        assert np.array_equal(fin, np.isfinite(a)) and np.array_equal(np.isnan(a), np.isnan(b)), name
        if fin.any():
            assert np.max(np.abs(a[fin] - b[fin])) < TOL, (name, np.max(np.abs(a[fin] - b[fin])))
    if want['map_states'] is None:
        assert got['map_states'] is None
    elif same_map:
        assert np.array_equal(got['map_states'], want['map_states'])


@pytest.mark.parametrize('kind', ['markov', 'nongeometric', 'minlength'])
@pytest.mark.parametrize('name', [n for n in CASES if 'order0' not in n])
def test_oracle_against_enumeration(name, kind):
    model, x, prior = build(name, kind)
    W, F = C.tables(model, x)
    got, want = DO.solve(W, F, prior), DO.enumerate_all(W, F, prior)
    assert got['n_nan_windows'] == 0 and want['n_nan'] == 0 and np.isfinite(want['logev'])
    compare(got, want, same_map=want['n_max'] == 1)
    if not CASES[name][2]:
        assert want['n_max'] == 1
    # the MAP profile re-evaluated
    assert abs(prior.log_prob(got['map_states']) + G.logl_tables(W, F, got['map_states']) - got['map_logjoint']) < TOL
    # the identities
    post = np.exp(got['log_post'])
    assert np.max(np.abs(post.sum(axis=0) - 1)) < TOL
    occupancy = post[:, :-1].sum(axis=1)
    assert np.max(np.abs(got['exp_stay'] + got['exp_jumps'].sum(axis=1) - occupancy)) < TOL
    if CASES[name][0] == 3:
        assert got['exp_jumps'][0, 2] == 0.0        # the forbidden transition


@pytest.mark.parametrize('kind', ['markov', 'minlength'])
@pytest.mark.parametrize('nan', ['propagate', 'omit'])
def test_oracle_nan_windows_against_enumeration(nan, kind):
    model, x, prior = build('s2_order0_inner_gap', kind)
    W, F = C.tables(model, x)
    assert np.isnan(W[:, 4:6, 6:8]).any()
    got, want = DO.solve(W, F, prior, nan=nan), DO.enumerate_all(W, F, prior, nan=nan)
    assert got['n_nan_windows'] > 0 and want['n_nan'] > 0
    if nan == 'propagate':
        assert np.isnan(got['logev']) and np.all(np.isnan(got['log_post'])) and np.all(np.isnan(got['exp_stay']))
    else:
        assert np.isfinite(got['logev'])
    compare(got, want, same_map=want['n_max'] == 1)      # the MAP among the profiles without a NaN window, in both modes
    assert np.isfinite(got['map_logjoint'])


@pytest.mark.parametrize('S,T', [(1, 6), (2, 8), (3, 7)])
def test_markov_prior_sums_to_one(S, T):
    rng = np.random.default_rng(S * 100 + T)
    prior = bild_amd.DwellPrior.markov(DC.markov_matrix(rng, S), rng.dirichlet(np.ones(S)), n=T)
    total = [prior.log_prob(row) for _, _, _, st in DO.all_profiles(T, S) for row in st]
    assert abs(logsumexp(total)) < 1e-13
    # ... and the tables serve every shorter trajectory as well
    total = [prior.log_prob(row) for _, _, _, st in DO.all_profiles(T - 2, S) for row in st]
    assert abs(logsumexp(total)) < 1e-13


def test_markov_tables():
    P = np.array([[0.9, 0.1, 0.0], [0.05, 0.8, 0.15], [0.0, 0.0, 1.0]])
    prior = bild_amd.DwellPrior.markov(P, [0.2, 0.3, 0.5], n=5)
    assert prior.nStates == 3 and prior.L == 5
    assert np.allclose(prior.log_dwell[1], np.arange(5) * np.log(0.8) + np.log(0.2), rtol=0, atol=1e-15)
    assert np.allclose(prior.log_surv[0], np.arange(5) * np.log(0.9), rtol=0, atol=1e-15)
    assert abs(prior.log_jump[1, 2] - np.log(0.15 / 0.2)) < 1e-15 and prior.log_jump[0, 2] == -np.inf
    assert np.all(prior.log_jump[2] == -np.inf) and np.all(prior.log_dwell[2] == -np.inf) and np.all(prior.log_surv[2] == 0)
    # a state that never stays: segments of one frame only
    flip = bild_amd.DwellPrior.markov([[0.0, 1.0], [1.0, 0.0]], n=4)
    assert flip.log_dwell[0, 0] == 0 and np.all(flip.log_dwell[0, 1:] == -np.inf) and flip.log_surv[0, 0] == 0
    assert abs(flip.log_prob([0, 1, 0, 1]) - np.log(0.5)) < 1e-15 and flip.log_prob([0, 0, 1, 0]) == -np.inf


def test_symmetric_chain_is_the_k_mixture_of_the_segment_recursion():
    T, p = 14, 0.17
    rng = np.random.default_rng(5)
    model = C.random_model(rng, 2, T + 4, orders=np.ones((2, 2), dtype=int))
    x = C.random_traj(rng, T, (6,))
    W, F = C.tables(model, x)
    per_k = SO.solve(W, F, model.transitions, T - 1)
    logev, post = DC.symmetric_mixture(p, T, per_k['logev'], per_k['log_post'])
    got = DO.solve(W, F, DC.symmetric_chain(p, T))
    assert abs(got['logev'] - logev) < TOL
    assert np.max(np.abs(np.exp(got['log_post']) - post)) < TOL


def test_prior_refusals():
    li, lj = np.log([0.5, 0.5]), np.array([[-np.inf, 0.0], [0.0, -np.inf]])
    tab = np.zeros((2, 6))
    bild_amd.DwellPrior(li, lj, tab, tab)
    for args in ((li, lj, tab, np.zeros((2, 5))), (li, np.zeros((2, 2)), tab, tab), (li, lj[:1], tab, tab), (li[:1], lj, tab, tab),
                 (np.array([-np.inf, -np.inf]), lj, tab, tab), (li, lj, np.full((2, 6), np.nan), tab),
                 (li, lj, tab, np.full((2, 6), np.inf)), (li, lj, np.zeros((2, 0)), np.zeros((2, 0)))):
        with pytest.raises(ValueError):
            bild_amd.DwellPrior(*args)
    for P in ([[0.5, 0.6], [0.5, 0.5]], [[1.0, 0.0]], [[1.2, -0.2], [0.5, 0.5]]):
        with pytest.raises(ValueError):
            bild_amd.DwellPrior.markov(P)
    with pytest.raises(ValueError):
        bild_amd.DwellPrior.markov([[0.5, 0.5], [0.5, 0.5]], init=[0.7, 0.7])
    with pytest.raises(ValueError):
        bild_amd.DwellPrior.markov([[0.5, 0.5], [0.5, 0.5]], n=0)
    prior = bild_amd.DwellPrior.markov([[0.5, 0.5], [0.5, 0.5]], n=4)
    for profile in ([0, 1, 0, 1, 0], [0, 2], []):
        with pytest.raises(ValueError):
            prior.log_prob(profile)


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
    for other in (rouse, factorized):
        with pytest.raises(TypeError):
            bild_amd.exact_dwell(x, other, prior)
        with pytest.raises(TypeError):
            bild_amd.fit_markov_prior([x], other)
        with pytest.raises(TypeError):      # the error `exact_sample` gives them
            bild_amd.exact_sample(x, other)
    with pytest.raises(TypeError):
        bild_amd.exact_dwell(x, model, (prior.log_init, prior.log_jump))
    with pytest.raises(ValueError):
        bild_amd.exact_dwell(x, model, prior, nan='drop')
    with pytest.raises(ValueError):         # the tables are shorter than the trajectory
        bild_amd.exact_dwell(x, model, DC.symmetric_chain(0.1, 19))
    with pytest.raises(ValueError):         # the states do not match
        bild_amd.exact_dwell(x, model, DC.make_prior('markov', rng, 3, 20))
    with pytest.raises(ValueError):         # beyond the model's lags
        bild_amd.exact_dwell(C.random_traj(rng, 30), model, DC.symmetric_chain(0.1, 40))
    five = C.random_model(rng, 5, 24)
    with pytest.raises(ValueError):
        bild_amd.exact_dwell(x, five, DC.make_prior('markov', rng, 5, 20))
    with pytest.raises(ValueError):
        bild_amd.fit_markov_prior([x], model, start=np.full((3, 3), 1 / 3))
    with pytest.raises(ValueError):
        bild_amd.fit_markov_prior([x], model, tol=0)
    with pytest.raises(ValueError):
        bild_amd.fit_markov_prior([], model)
    three = C.random_model(rng, 3, 24)
    with pytest.raises(ValueError):         # a start that uses the forbidden transition 0 -> 2
        bild_amd.fit_markov_prior([x], three, start=np.full((3, 3), 1 / 3))
    assert bild_amd.exact_dwell([], model, prior) == []


def test_hard_priors():
    rng = np.random.default_rng(8)
    T = 150
    prior = DC.prior_of('bounded', rng, 2, T + 5, T)
    assert DC.BOUND == 70 and np.all(np.isfinite(prior.log_dwell[:, :70])) and np.all(prior.log_surv[:, 70:] == -np.inf)
    st = np.zeros(T, dtype=int)
    st[10:80] = 1       # 70 frames, completed; the first and the last segment have 10 and 70
    assert np.isfinite(prior.log_prob(st))
    st[80] = 1          # 71
    assert prior.log_prob(st) == -np.inf
    st = np.repeat([1, 0, 1], [40, 39, 71])     # a censored last segment of 71 frames
    assert len(st) == T and prior.log_prob(st) == -np.inf
    assert np.isfinite(prior.log_prob(np.repeat([1, 0, 1], [40, 40, 70])))
    for kind in ('markov', 'minlength', 'nongeometric'):    # passed through unchanged, the same numbers drawn
        a, b = DC.prior_of(kind, np.random.default_rng(9), 3, 20, 15), DC.make_prior(kind, np.random.default_rng(9), 3, 20)
        assert all(np.array_equal(getattr(a, n), getattr(b, n)) for n in ('log_init', 'log_jump', 'log_dwell', 'log_surv'))
    one = DC.prior_of('one_start', rng, 3, 20, 15)
    assert one.log_init.tolist() == [-np.inf, -np.inf, 0.0] and one.log_prob([0, 0, 1]) == -np.inf and np.isfinite(one.log_prob([2, 1, 1]))
    flip = DC.prior_of('flip', rng, 2, 20, 15)
    assert abs(flip.log_prob([1, 0, 1, 0]) - np.log(0.7)) < 1e-15 and flip.log_prob([1, 1, 0, 1]) == -np.inf
    no = DC.prior_of('impossible', rng, 2, 10, 6)
    assert all(no.log_prob(row) == -np.inf for _, _, _, states in DO.all_profiles(6, 2) for row in states)
    assert np.isfinite(no.log_prob(np.zeros(5, dtype=int)))       # (a shorter trajectory has the profile of one segment)
    assert np.all(DC.prior_of('absorbing', rng, 3, 20, 15).log_jump[2] == -np.inf)


@pytest.mark.parametrize('S,T,missing,kind', DC.ORACLE_CASES[DC.N_ORACLE_CASES_BEFORE:])
def test_gpu_oracle_cases_meet_their_conditions(S, T, missing, kind):
    """ conditions on the GPU test's inputs: what tests/test_gpu_dwell.py compares the device with is what it is meant to be """
    case = (S, T, missing, kind)
    model, x, prior, W, F = DC.oracle_case(case)
    assert model.nStates == prior.nStates == S and x.shape == (T, 2) and prior.L == T + 5
    assert np.array_equal(np.flatnonzero(np.isnan(x[:, 0])), missing)
    want = DC.oracle_answer(case)
    print(f"{case}: oracle {DC.ORACLE_SECONDS[case]:.1f} s, logev {want['logev']}")
    assert DC.ORACLE_SECONDS[case] < 20
    assert want['n_nan_windows'] == 0
    post = want['log_post']
    if kind == 'impossible':
        assert want['logev'] == -np.inf and want['map_states'] is None and np.isnan(want['map_logjoint'])
        assert np.all(np.isnan(post)) and np.all(np.isnan(want['exp_jumps'])) and np.all(np.isnan(want['exp_stay']))
        return
    assert np.isfinite(want['logev']) and np.isfinite(want['map_logjoint']) and want['map_states'] is not None
    assert not np.any(np.isnan(post)) and np.all(np.isfinite(want['exp_jumps'])) and np.all(np.isfinite(want['exp_stay']))
    assert np.max(np.abs(np.exp(post).sum(axis=0) - 1)) < 1e-9
    if kind == 'one_start':
        assert np.all(post[:S - 1, 0] == -np.inf) and abs(post[S - 1, 0]) < 1e-12 and 0.99 < np.mean(np.isfinite(post)) < 1
    else:
        assert np.all(np.isfinite(post))
    if kind == 'bounded':       # every tile seam is crossed by a switch
        runs = np.diff(np.concatenate(([0], np.flatnonzero(np.diff(want['map_states'])) + 1, [T])))
        assert runs.max() <= DC.BOUND and len(runs) >= T / DC.BOUND
    if kind == 'flip':
        assert np.all(np.diff(want['map_states']) != 0) and abs(want['exp_jumps'].sum() - (T - 1)) < 1e-9
    if kind == 'absorbing':
        assert np.all(want['exp_jumps'][2] == 0) and want['exp_jumps'][0, 2] == 0
    if S == 1:
        assert np.all(post == 0) and np.array_equal(want['exp_jumps'], [[0.0]]) and want['exp_stay'][0] == T - 1


def test_gpu_ragged_batch_meets_its_conditions():
    model, prior, xs, tabs = DC.ragged_case()
    assert [len(x) for x in xs] == [T for T, _ in DC.RAGGED] and model.nStates == 4 and prior.L == 262
    for j, want in enumerate(DC.ragged_answers()):
        print(f"trajectory {j}: oracle {DC.ORACLE_SECONDS['ragged', j]:.1f} s, logev {want['logev']}")
        assert DC.ORACLE_SECONDS['ragged', j] < 20
        assert want['n_nan_windows'] == 0 and np.isfinite(want['logev']) and np.isfinite(want['map_logjoint'])
        assert np.all(np.isfinite(want['log_post'])) and np.all(np.isfinite(want['exp_jumps'])) and np.all(np.isfinite(want['exp_stay']))


def test_gpu_sharp_case_meets_its_conditions():
    model, x, prior, st, W, F = DC.sharp_case()
    want = DC.sharp_answer()
    post = want['log_post']
    low = post < -600       # (-inf among them)
    print(f"sharp: oracle {DC.ORACLE_SECONDS['sharp']:.1f} s, logev {want['logev']}, min finite W {np.min(W[np.isfinite(W)]):.4g}, "
          f"finite log_post {np.mean(np.isfinite(post)):.3f}, below -600: {int(low.sum())}, -inf: {int(np.sum(post == -np.inf))}, lowest finite {np.min(post[np.isfinite(post)]):.1f}")
    assert DC.ORACLE_SECONDS['sharp'] < 20
    assert want['n_nan_windows'] == 0 and abs(want['logev'] + 207.416) < 1e-3
    assert np.array_equal(want['map_states'], st)
    assert -1.2e5 < np.min(W[np.isfinite(W)]) < -1.0e5
    assert not np.any(np.isnan(post)) and 0.8 < np.mean(np.isfinite(post)) < 0.95
    assert 20 <= low.sum() <= 60
