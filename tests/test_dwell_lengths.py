"""
The expected segment-length counts and the fit of the dwell-time prior without a GPU (bild_amd.exact.exact_dwell_lengths,
fit_dwell_prior): the NumPy oracle tests/dwell_length_oracle.py against the enumeration of every profile
on the cases of tests/test_dwell.py, its identities against `dwell_oracle.solve`, Fisher's identity by central differences of
the oracle's evidence, `DwellPrior.from_hazard`, the M-step on hand-made counts, and the argument errors.
"""
import numpy as np
import pytest
from scipy.special import logsumexp

import bild_amd
import dwell_cases as DC
import dwell_length_cases as DLC
import dwell_length_oracle as DL
import dwell_oracle as DO
import segment_cases as C
import test_dwell as TD
from bild_amd import _lib
from bild_amd.exact import hazard_m_step

# the issue's bound against enumeration; observed on these cases: 6e-15
TOL = 1e-12


def compare(got, want):
    assert abs(got['logev'] - want['logev']) < TOL
    worst = 0.0
    for name in ('dwell', 'cens', 'init'):
        assert got[name].shape == want[name].shape and np.all(np.isfinite(got[name]))
        worst = max(worst, float(np.max(np.abs(got[name] - want[name]))))
    print(f"worst deviation of a count from the enumeration {worst:.1e}")
    assert worst < TOL


def identities(got, ref, T, tol):
    """ the six identities of section 24 against `dwell_oracle.solve`'s jumps, stays and marginals """
    D, Cn, first = got['dwell'], got['cens'], got['init']
    lengths = np.arange(1, T + 1)
    post = np.exp(ref['log_post'])
    devs = {'sum D = jumps out': np.max(np.abs(D.sum(axis=1) - ref['exp_jumps'].sum(axis=1))),
            'sum C = 1': abs(Cn.sum() - 1),
            'sum_l C = last marginal': np.max(np.abs(Cn.sum(axis=1) - post[:, T - 1])),
            'sum (l - 1)(D + C) = stay': np.max(np.abs(((D + Cn) * (lengths - 1)).sum(axis=1) - ref['exp_stay'])),
            'sum l (D + C) = T': abs(((D + Cn) * lengths).sum() - T),
            'I = first marginal': np.max(np.abs(first - post[:, 0]))}
    print(', '.join(f"{k}: {v:.1e}" for k, v in devs.items()))
    for name, v in devs.items():
        assert v < tol, (name, v)
    assert np.all(D[:, T - 1] == 0)


@pytest.mark.parametrize('kind', ['markov', 'nongeometric', 'minlength'])
@pytest.mark.parametrize('name', [n for n in TD.CASES if 'order0' not in n])
def test_oracle_against_enumeration_and_identities(name, kind):
    model, x, prior = TD.build(name, kind)
    T = len(x)
    W, F = C.tables(model, x)
    got, want = DL.solve(W, F, prior), DL.enumerate_all(W, F, prior)
    assert got['n_nan_windows'] == 0 and want['n_nan'] == 0
    compare(got, want)
    identities(got, DO.solve(W, F, prior), T, TOL)
    if kind == 'minlength':
        assert np.all(got['dwell'][:, 0] == 0) and np.any(got['cens'][:, 0] > 0)    # no completed segment of one frame


@pytest.mark.parametrize('kind', ['markov', 'minlength'])
@pytest.mark.parametrize('nan', ['propagate', 'omit'])
def test_oracle_nan_windows_against_enumeration(nan, kind):
    model, x, prior = TD.build('s2_order0_inner_gap', kind)
    W, F = C.tables(model, x)
    got, want = DL.solve(W, F, prior, nan=nan), DL.enumerate_all(W, F, prior, nan=nan)
    assert got['n_nan_windows'] > 0 and want['n_nan'] > 0
    if nan == 'propagate':
        for name in ('dwell', 'cens', 'init'):
            assert np.isnan(got['logev']) and np.all(np.isnan(got[name])) and np.all(np.isnan(want[name]))
        return
    compare(got, want)
    identities(got, DO.solve(W, F, prior, nan=nan), len(x), TOL)


@pytest.mark.parametrize('name,kind', [('s2_gapfree', 'nongeometric'), ('s3_inner_gap', 'markov')])
def test_fisher_identity_by_central_differences_of_the_oracle(name, kind):
    """ D[s][l] = d logev / d log_dwell[s][l] and C[s][l] = d logev / d log_surv[s][l], every finite entry: step 1e-5, bound 1e-6 """
    model, x, prior = TD.build(name, kind)
    T, h = len(x), 1e-5
    W, F = C.tables(model, x)
    got = DL.solve(W, F, prior)
    worst = 0.0
    for table, counts, top in (('log_dwell', got['dwell'], T - 1), ('log_surv', got['cens'], T)):
        for s in range(prior.nStates):
            for length in range(1, top + 1):
                ev = []
                for sign in (1, -1):
                    tabs = {n: getattr(prior, n).copy() for n in ('log_init', 'log_jump', 'log_dwell', 'log_surv')}
                    tabs[table][s, length - 1] += sign * h
                    ev.append(DO.solve(W, F, bild_amd.DwellPrior(**tabs))['logev'])
                rate = (ev[0] - ev[1]) / (2 * h)
                worst = max(worst, abs(rate - counts[s, length - 1]))
                assert abs(rate - counts[s, length - 1]) < 1e-6, (table, s, length, rate, counts[s, length - 1])
    print(f"worst deviation of a difference quotient from its count {worst:.1e}")


# ---------------------------------------------------------------- DwellPrior.from_hazard

def test_from_hazard_constant_is_markov():
    n = 300
    for P in (np.array([[0.9, 0.1, 0.0], [0.05, 0.8, 0.15], [0.3, 0.2, 0.5]]), np.array([[0.97, 0.03], [0.4, 0.6]]),
              np.array([[0.9, 0.1, 0.0], [0.05, 0.8, 0.15], [0.0, 0.0, 1.0]])):      # (the last: an absorbing state)
        S = len(P)
        init = np.arange(1, S + 1) / np.arange(1, S + 1).sum()
        leave = 1 - np.diag(P)
        off = P - np.diag(np.diag(P))
        jump = np.where(leave[:, None] > 0, off / np.where(leave > 0, leave, 1)[:, None], 0.0)
        a = bild_amd.DwellPrior.markov(P, init, n=n)
        b = bild_amd.DwellPrior.from_hazard(np.repeat(leave[:, None], n, axis=1), jump, init)
        for name in ('log_init', 'log_jump', 'log_dwell', 'log_surv'):
            u, v = getattr(a, name), getattr(b, name)
            assert np.array_equal(np.isfinite(u), np.isfinite(v)), name
            assert np.max(np.abs(u[np.isfinite(u)] - v[np.isfinite(u)])) < 1e-12, name
    assert np.array_equal(bild_amd.DwellPrior.from_hazard(np.full((2, 3), 0.5), [[0, 1], [1, 0]]).log_init, np.log([0.5, 0.5]))


@pytest.mark.parametrize('S,T', [(1, 6), (2, 8), (3, 7)])
def test_from_hazard_is_normalised(S, T):
    rng = np.random.default_rng(40 + S)
    hazard = rng.uniform(0, 0.7, size=(S, T))
    hazard[0, 2] = 0.0
    jump = rng.uniform(0.2, 1, size=(S, S))
    np.fill_diagonal(jump, 0.0)
    if S == 1:
        hazard[:] = 0.0
    else:
        hazard[S - 1, 3] = 1.0      # no segment of the last state lasts longer than 4 frames
        jump /= jump.sum(axis=1, keepdims=True)
    prior = bild_amd.DwellPrior.from_hazard(hazard, jump, rng.dirichlet(np.ones(S)))
    for n in (T, T - 3):            # the tables serve every shorter trajectory as well
        assert abs(logsumexp([prior.log_prob(row) for _, _, _, st in DO.all_profiles(n, S) for row in st])) < 1e-13


def test_from_hazard_one_admits_no_longer_segment():
    hazard = np.full((2, 8), 0.2)
    hazard[0, 2] = 1.0      # state 0 ends at 3 frames at the latest
    prior = bild_amd.DwellPrior.from_hazard(hazard, [[0, 1], [1, 0]], [0.5, 0.5])
    assert np.all(np.isfinite(prior.log_dwell[0, :3])) and np.all(prior.log_dwell[0, 3:] == -np.inf)
    assert np.all(np.isfinite(prior.log_surv[0, :3])) and np.all(prior.log_surv[0, 3:] == -np.inf)
    assert abs(prior.log_dwell[0, 2] - 2 * np.log(0.8)) < 1e-15 and np.all(np.isfinite(prior.log_dwell[1]))
    assert np.isfinite(prior.log_prob([0, 0, 0, 1, 1, 1, 1, 0])) and prior.log_prob([0, 0, 0, 0, 1, 1, 1, 0]) == -np.inf
    assert np.isfinite(prior.log_prob([1, 0, 0, 0])) and prior.log_prob([1, 0, 0, 0, 0]) == -np.inf     # censored as well
    # a hazard of 0 ends nothing: no completed segment of that length, the survival goes on
    hazard[1, 0] = 0.0
    prior = bild_amd.DwellPrior.from_hazard(hazard, [[0, 1], [1, 0]])
    assert prior.log_dwell[1, 0] == -np.inf and prior.log_surv[1, 1] == 0.0 and np.isfinite(prior.log_dwell[1, 1])


def test_from_hazard_refusals():
    good = dict(hazard=np.full((2, 5), 0.3), jump=np.array([[0.0, 1.0], [1.0, 0.0]]), init=[0.4, 0.6])
    bild_amd.DwellPrior.from_hazard(**good)
    bild_amd.DwellPrior.from_hazard(np.array([[0.3] * 5, [0.0] * 5]), [[0, 1], [0, 0]])      # a state that never leaves
    for change in (dict(hazard=np.full(5, 0.3)), dict(hazard=np.full((2, 0), 0.3)), dict(hazard=np.full((2, 5), 1.1)),
                   dict(hazard=np.full((2, 5), -0.1)), dict(hazard=np.full((2, 5), np.nan)),
                   dict(jump=np.zeros((3, 3))), dict(jump=np.array([[0.1, 0.9], [1.0, 0.0]])),
                   dict(jump=np.array([[0.0, 0.7], [1.0, 0.0]])), dict(jump=np.array([[0.0, -1.0], [1.0, 0.0]])),
                   dict(jump=np.array([[0.0, np.nan], [1.0, 0.0]])),
                   dict(jump=np.array([[0.0, 1.0], [0.0, 0.0]])),      # never leaves, with a positive hazard
                   dict(init=[0.5, 0.6]), dict(init=[1.0]), dict(init=[-0.5, 1.5])):
        with pytest.raises(ValueError):
            bild_amd.DwellPrior.from_hazard(**{**good, **change})


# ---------------------------------------------------------------- the M-step

def markov_counts(rng, n):
    """ hand-made counts of two states: D, C (2, n), jumps (2, 2) with sum_l D = the jumps out, first (2,) """
    D, Cn = rng.uniform(0, 2, size=(2, n)), rng.uniform(0, 0.1, size=(2, n))
    D[:, n - 1] = 0.0
    jumps = np.array([[0.0, D[0].sum()], [D[1].sum(), 0.0]])
    return D, Cn, jumps, np.array([3.0, 5.0])


def test_m_step_one_bin_is_fit_markov_priors_formula():
    n = 12
    D, Cn, jumps, first = markov_counts(np.random.default_rng(1), n)
    stay = ((D + Cn) * (np.arange(1, n + 1) - 1)).sum(axis=1)       # section 24's fourth identity
    hazard, jump, init, supported = hazard_m_step(D, Cn, jumps, first, [1], np.full((2, 1), 0.5), np.zeros((2, 2)), [0.5, 0.5])
    P_ss = stay / (stay + jumps.sum(axis=1))                        # `fit_markov_prior`: P_ss = stay / (stay + jumps)
    assert np.max(np.abs(1 - hazard[:, 0] - P_ss)) < 1e-14 and supported.all()
    assert np.array_equal(jump, [[0, 1], [1, 0]]) and np.max(np.abs(init - [3 / 8, 5 / 8])) < 1e-16
    # three states: the jumps of a row in proportion, a forbidden one left at 0
    j3 = np.array([[0.0, 2.0, 1.0], [1.0, 0.0, 3.0], [4.0, 4.0, 0.0]])
    allowed = np.array([[0, 1, 0], [1, 0, 1], [1, 1, 0]], dtype=bool)
    _, jump, _, _ = hazard_m_step(np.ones((3, 4)), np.ones((3, 4)), j3, np.ones(3), [1], np.full((3, 1), 0.5), np.zeros((3, 3)), np.ones(3) / 3,
                                  allowed=allowed)
    assert np.array_equal(jump, [[0, 1, 0], [0.25, 0, 0.75], [0.5, 0.5, 0]])


def test_m_step_one_bin_per_length_is_kaplan_meier():
    # 10 segments of state 0: observed lengths 1, 2, 2, 4, 4, 4 and censored at 2, 3, 5, 5; state 1: nothing ends
    n = 5
    D = np.array([[1, 2, 0, 3, 0], [0, 0, 0, 0, 0]], dtype=float)
    Cn = np.array([[0, 1, 1, 0, 2], [0, 0, 4, 0, 0]], dtype=float)
    start = np.full((2, n), 0.5)
    hazard, _, _, supported = hazard_m_step(D, Cn, np.zeros((2, 2)), np.ones(2), np.arange(1, n + 1), start, np.zeros((2, 2)), [0.5, 0.5])
    # at risk at l: the segments that end at l or run on behind it; one censored AT l met no decision there (log_surv[l] holds the
    # hazards below l alone) -- Kaplan-Meier with the censoring counted before the event
    at_risk = np.array([10, 8, 6, 5])
    assert np.array_equal(hazard[0, :4], D[0, :4] / at_risk) and np.array_equal(hazard[0, :4], [0.1, 0.25, 0.0, 0.6])
    assert hazard[0, 4] == 0.5 and np.array_equal(supported[0], [True, True, True, True, False])    # nobody runs on behind l = 5
    survival = np.cumprod(1 - hazard[0, :4])
    assert np.allclose(survival, [0.9, 0.675, 0.675, 0.27], rtol=0, atol=1e-15)     # the Kaplan-Meier curve of these data
    assert np.array_equal(hazard[1], [0, 0, 0.5, 0.5, 0.5]) and np.array_equal(supported[1], [True, True, False, False, False])


def test_m_step_min_risk_holds_a_bin_and_rows_without_mass():
    D = np.array([[2.0, 1.0, 1e-9, 0.0], [0.0, 0.0, 0.0, 0.0]])
    Cn = np.array([[0.0, 1.0, 1e-9, 0.0], [0.0, 0.0, 0.0, 0.0]])
    start, jump0 = np.array([[0.3, 0.4], [0.6, 0.7]]), np.array([[0.0, 1.0], [1.0, 0.0]])
    hazard, jump, init, supported = hazard_m_step(D, Cn, np.array([[0.0, 3.0], [0.0, 0.0]]), np.zeros(2), [1, 3], start, jump0, [0.2, 0.8])
    assert np.array_equal(supported, [[True, False], [False, False]])
    # bin 0 of state 0: 3 end at the lengths 1 and 2, 2 + 2e-9 and 2e-9 run on behind them; bin 1 has 1e-9 at risk and keeps 0.4
    assert abs(hazard[0, 0] - 3 / (5 + 4e-9)) < 1e-15 and hazard[0, 1] == 0.4 and np.array_equal(hazard[1], [0.6, 0.7])
    assert np.array_equal(jump, jump0) and np.array_equal(init, [0.2, 0.8])         # state 1 never jumped; no first frame
    assert start[0, 0] == 0.3                                                         # the arguments are not written
    hazard, _, _, supported = hazard_m_step(D, Cn, np.zeros((2, 2)), np.ones(2), [1, 3], start, jump0, [0.2, 0.8], min_risk=1e-10)
    assert supported[0, 1] and hazard[0, 1] == 1.0      # the one segment that reached the bin ends in it


# ---------------------------------------------------------------- the arguments

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
    lengths, fit = bild_amd.exact_dwell_lengths, bild_amd.fit_dwell_prior
    for other in (rouse, factorized):
        with pytest.raises(TypeError):
            lengths(x, other, prior)
        with pytest.raises(TypeError):
            fit([x], other)
    with pytest.raises(TypeError):
        lengths(x, model, (prior.log_init, prior.log_jump))
    with pytest.raises(ValueError):
        lengths(x, model, prior, nan='drop')
    with pytest.raises(ValueError):         # the tables are shorter than the trajectory
        lengths(x, model, DC.symmetric_chain(0.1, 19))
    with pytest.raises(ValueError):         # the states do not match
        lengths(x, model, DC.make_prior('markov', rng, 3, 20))
    with pytest.raises(ValueError):         # beyond the model's lags
        lengths(C.random_traj(rng, 30), model, DC.symmetric_chain(0.1, 40))
    five = C.random_model(rng, 5, 24)
    with pytest.raises(ValueError):
        lengths(x, five, DC.make_prior('markov', rng, 5, 20))
    assert lengths([], model, prior) == []

    good = (np.full((2, 2), 0.1), [[0, 1], [1, 0]], [0.5, 0.5])
    for kw in (dict(edges=[2, 4]), dict(edges=[1, 4, 4]), dict(edges=[1, 8, 4]), dict(edges=[1.0, 4.5]), dict(edges=[]), dict(edges=[[1, 2]]),
               dict(tol=0), dict(max_iter=0), dict(max_iter=2.5), dict(min_risk=0), dict(nan='drop'),
               dict(edges=[1, 4], start=(np.full((2, 3), 0.1),) + good[1:]),            # a hazard of another number of bins
               dict(edges=[1, 4], start=(np.full((2, 2), 1.5),) + good[1:]),            # not a probability
               dict(edges=[1, 4], start=(good[0], [[0, 0.5], [1, 0]], good[2])),        # a row that is no distribution
               dict(edges=[1, 4], start=(good[0], good[1], [0.5, 0.6])),
               dict(edges=[1, 4], start=(good[0], good[1])), dict(start=np.full((2, 2), 0.5))):
        with pytest.raises(ValueError):
            fit([x], model, **kw)
    with pytest.raises(ValueError):
        fit([], model)
    with pytest.raises(ValueError):         # beyond the model's lags
        fit([C.random_traj(rng, 30)], model)
    with pytest.raises(ValueError):         # more states than the recursion supports
        fit([x], five)
    three = C.random_model(rng, 3, 24)
    with pytest.raises(ValueError):         # a start that uses the forbidden transition 0 -> 2
        fit([x], three, edges=[1], start=(np.full((3, 1), 0.1), (1 - np.eye(3)) / 2, np.ones(3) / 3))
    markov = bild_amd.MarkovPriorFit(P=np.full((3, 3), 1 / 3), init=np.ones(3) / 3, log_evidence=np.zeros(1), n_iter=1, converged=True)
    with pytest.raises(ValueError):         # a Markov fit of another number of states
        fit([x], model, start=markov)


def test_default_edges_and_the_fits_prior():
    """ what `fit_dwell_prior` would start from, without a device: the doubling edges, the starts, `DwellPriorFit.prior` """
    from bild_amd.exact import DwellPriorFit, _hazard_edges, _hazard_start
    assert [_hazard_edges(None, n).tolist() for n in (1, 2, 3, 16, 17, 200)] == [[1], [1], [1, 2], [1, 2, 4, 8], [1, 2, 4, 8, 16],
                                                                                 [1, 2, 4, 8, 16, 32, 64, 128]]
    model = C.random_model(np.random.default_rng(2), 3, 24)     # forbids 0 -> 2
    allowed, hazard, jump, init = _hazard_start(model, None, 3)
    assert np.array_equal(hazard, np.full((3, 3), 0.1)) and np.array_equal(jump, [[0, 1, 0], [0.5, 0, 0.5], [0.5, 0.5, 0]])
    assert np.array_equal(init, np.ones(3) / 3) and not allowed[0, 2] and not allowed.diagonal().any()
    P = np.array([[0.9, 0.1, 0.0], [0.05, 0.8, 0.15], [0.2, 0.2, 0.6]])
    markov = bild_amd.MarkovPriorFit(P=P, init=np.array([0.2, 0.3, 0.5]), log_evidence=np.zeros(1), n_iter=1, converged=True)
    _, hazard, jump, init = _hazard_start(model, markov, 2)
    fit = DwellPriorFit(edges=np.array([1, 4]), hazard=hazard, jump=jump, init=init, log_evidence=np.zeros(1), n_iter=1, converged=True,
                        expected_dwell=np.zeros((3, 30)), expected_censored=np.zeros((3, 30)), supported=np.ones((3, 2), dtype=bool))
    a, b = fit.prior(), markov.prior(30)
    assert a.L == 30 and fit.prior(50).L == 50
    for name in ('log_init', 'log_jump', 'log_dwell', 'log_surv'):
        u, v = getattr(a, name), getattr(b, name)
        assert np.array_equal(np.isfinite(u), np.isfinite(v)) and np.max(np.abs(u[np.isfinite(u)] - v[np.isfinite(u)])) < 1e-12
    # two bins that differ: the hazard of a length is that of its bin
    fit.hazard = np.array([[0.0, 0.2]] * 3)
    p = fit.prior(8)
    assert np.all(p.log_dwell[:, :3] == -np.inf) and np.all(p.log_surv[:, :4] == 0)
    assert np.max(np.abs(p.log_dwell[:, 3:] - (np.arange(5) * np.log(0.8) + np.log(0.2)))) < 1e-15
    with pytest.raises(ValueError):
        fit.prior(0)


def test_generator_of_semi_markov_profiles():
    """ conditions on the input of the GPU test's fit: the profiles have the dwell times they are meant to have """
    profiles = DLC.hazard_profiles(np.random.default_rng(71), 64, 200, DLC.HAZARD_EDGES, DLC.HAZARD_TRUE)
    assert len(profiles) == 64 and all(p.shape == (200,) and set(np.unique(p)) <= {0, 1} for p in profiles)
    runs = {0: [], 1: []}
    for p in profiles:
        cuts = np.concatenate(([0], np.flatnonzero(np.diff(p)) + 1))
        for a, b in zip(cuts[:-1], cuts[1:]):       # the completed segments
            runs[p[a]].append(b - a)
    assert min(runs[0]) >= 4 and min(runs[1]) >= 4 and len(runs[0]) > 300 and len(runs[1]) > 300
    # far from geometric: a geometric law of the same mean puts (1 - 1 / mean)^3 of its mass above 3, these put all of it there
    assert all(10 < np.mean(r) < 25 for r in runs.values())
    prior = DLC.hazard_prior(DLC.HAZARD_EDGES, DLC.HAZARD_TRUE, 200)
    assert all(np.isfinite(prior.log_prob(p)) for p in profiles)
