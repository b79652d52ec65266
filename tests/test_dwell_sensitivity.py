"""
The evidence gradient under a dwell-time prior without a GPU (bild_amd.exact.exact_dwell_sensitivities,
GenericGaussianModel.fit_dwell): the NumPy oracle tests/dwell_sensitivity_oracle.py against the enumeration
of every profile on the cases of tests/test_dwell.py, its gradient against central differences of `dwell_oracle.solve`'s
evidence, the sums of its segment weights against `dwell_oracle.solve`'s marginals, and the refusals.
"""
import numpy as np
import pytest

import bild_amd
import dwell_cases as DC
import dwell_oracle as DO
import dwell_sensitivity_cases as DSC
import dwell_sensitivity_oracle as DS
import gauss_oracle as G
import segment_cases as C
import segment_sensitivity_cases as SC
from bild_amd import _lib
from test_dwell import CASES, build

# Worst seen on these cases: 5.1e-15 against the enumeration, 9.6e-10 against the central differences, 2.2e-16 in the sums of the
# segment weights against the marginals (bound 1e-12).  The two T = 12 enumerations take 18 s each, everything else under 8 s.
TOL = 1e-10             # relative; section 20's bar for the recursion oracle against the enumeration
H, FD_TOL = 1e-5, 1e-6  # section 20's step and absolute bound of the central differences


def rel(got, want):
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    scale = np.max(np.abs(want)) if want.size else 0.0
    return 0.0 if want.size == 0 else float(np.max(np.abs(got - want))) / (scale if scale > 0 else 1.0)


def arrays(model):
    return model.msd, model.msd_inf, model.mean, model.ss_order


def check_against_enumeration(model, x, prior, nan):
    derivs = DSC.derivatives(model, 4)
    got = DS.solve(*arrays(model), x, prior, *derivs, nan=nan)
    want = DS.enumerate_all(*arrays(model), x, prior, *derivs, nan=nan)
    if np.isnan(want['logev']):
        assert np.isnan(got['logev']) and np.all(np.isnan(got['grad'])) and np.isnan(got['exp_logl']) and np.all(np.isnan(got['fisher']))
        return got, want
    devs = {'logev': rel(got['logev'], want['logev']), 'grad': rel(got['grad'], want['grad']),
            'exp_logl': rel(got['exp_logl'], want['exp_logl']), 'fisher': rel(got['fisher'], want['fisher'])}
    print(', '.join(f"{k} {v:.1e}" for k, v in devs.items()))
    for name, v in devs.items():
        assert v < TOL, (name, v)
    return got, want


@pytest.mark.parametrize('kind', ['markov', 'nongeometric', 'minlength'])
@pytest.mark.parametrize('name', [n for n in CASES if 'order0' not in n])
def test_oracle_against_enumeration(name, kind):
    model, x, prior = build(name, kind)
    got, want = check_against_enumeration(model, x, prior, 'propagate')
    assert got['n_nan_windows'] == 0 and want['n_nan'] == 0 and np.isfinite(want['logev'])
    # every frame lies in one segment: the segment weights add up to the expected number of segments, 1 + expected jumps
    ref = DO.solve(*C.tables(model, x), prior)
    assert abs(got['logev'] - ref['logev']) < 1e-12
    assert abs(got['n_segments'] - 1 - ref['exp_jumps'].sum()) < 1e-12


@pytest.mark.parametrize('kind', ['markov', 'minlength'])
@pytest.mark.parametrize('nan', ['propagate', 'omit'])
def test_oracle_nan_windows_against_enumeration(nan, kind):
    model, x, prior = build('s2_order0_inner_gap', kind)
    got, want = check_against_enumeration(model, x, prior, nan)
    assert got['n_nan_windows'] > 0 and want['n_nan'] > 0
    assert got['n_nan_windows'] == DO.solve(*C.tables(model, x), prior, nan=nan)['n_nan_windows']
    assert np.isnan(got['logev']) == (nan == 'propagate')
    if nan == 'omit':
        assert np.all(np.isfinite(got['grad'])) and np.all(np.isfinite(got['fisher']))


@pytest.mark.parametrize('kind', ['markov', 'nongeometric', 'minlength'])
@pytest.mark.parametrize('name', list(CASES))
def test_gradient_against_differences_of_the_evidence(name, kind):
    """ the four-parameter family of tests/segment_sensitivity_cases.py through `dwell_oracle.solve`'s evidence """
    model, x, prior = build(name, kind)
    nan = 'omit' if 'order0' in name else 'propagate'
    got = DS.solve(*arrays(model), x, prior, *DSC.derivatives(model, 4), nan=nan)

    def logev(theta):
        W, F = G.tables(*SC.family_arrays(model, theta), model.ss_order, x)
        return DO.solve(W, F, prior, nan=nan)['logev']

    quot = np.zeros(4)
    for p in range(4):
        e = np.zeros(4)
        e[p] = H
        quot[p] = (logev(SC.BASE + e) - logev(SC.BASE - e)) / (2 * H)
    dev = float(np.max(np.abs(got['grad'] - quot)))
    print(f"{name} {kind}: grad {got['grad']}, quotient {quot}, deviation {dev:.2e}")
    assert dev < FD_TOL, dev


@pytest.mark.parametrize('kind', ['markov', 'nongeometric', 'minlength'])
@pytest.mark.parametrize('name', list(CASES))
def test_segment_weights_add_up_to_the_marginals(name, kind):
    """ sum_{a <= t} Omega(s, a, t) = P(theta_t = s) of `dwell_oracle.solve` """
    model, x, prior = build(name, kind)
    nan = 'omit' if 'order0' in name else 'propagate'
    W, F = C.tables(model, x)
    w = DS.segment_weights(W, F, prior, nan=nan)
    post = np.exp(DO.solve(W, F, prior, nan=nan)['log_post'])
    dev = float(np.max(np.abs(DS.occupancy(w['q0'], w['q']) - post)))
    print(f"{name} {kind}: {dev:.1e}")
    assert dev < 1e-12


def test_one_profile_priors():
    """ the priors of the GPU test's second check admit the profile they are meant to, and no other """
    prior, states = DSC.one_profile_prior(9, (3, 2), 12)
    assert states.tolist() == [0, 0, 0, 1, 1, 0, 0, 0, 1]
    weights = [prior.log_prob(row) for _, _, _, st in DO.all_profiles(9, 2) for row in st]
    assert np.sum(np.isfinite(weights)) == 1 and prior.log_prob(states) == 0.0
    prior, states = DSC.one_profile_prior(193, (70, 60), 200)
    assert np.array_equal(states, np.repeat([0, 1, 0], [70, 60, 63])) and prior.log_prob(states) == 0.0
    flat = DSC.flat_prior(8)
    weights = [flat.log_prob(row) for _, _, _, st in DO.all_profiles(6, 2) for row in st]
    assert np.sum(np.isfinite(weights)) == 1 and flat.log_prob(np.zeros(6, dtype=int)) == 0.0
    # the symmetric chain's prior depends on k alone: 0.5 p^k (1 - p)^(T - 1 - k) a profile, so the weights of the k add up to 2
    assert abs(DSC.k_weights_of_symmetric_chain(0.07, 60).sum() - 2) < 1e-12


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
    sens = bild_amd.exact_dwell_sensitivities
    for other in (rouse, factorized):
        with pytest.raises(TypeError, match='GenericGaussianModel'):
            sens(x, other, prior)
    with pytest.raises(TypeError):
        sens(x, model, (prior.log_init, prior.log_jump))
    with pytest.raises(ValueError):
        sens(x, model, prior, nan='drop')
    with pytest.raises(ValueError):         # the tables are shorter than the trajectory
        sens(x, model, DC.symmetric_chain(0.1, 19))
    with pytest.raises(ValueError):         # the states do not match
        sens(x, model, DC.make_prior('markov', rng, 3, 20))
    with pytest.raises(ValueError):         # beyond the model's lags
        sens(C.random_traj(rng, 30), model, DC.symmetric_chain(0.1, 40))
    five = C.random_model(rng, 5, 24)
    with pytest.raises(ValueError):
        sens(x, five, DC.make_prior('markov', rng, 5, 20))
    # the derivative arrays: `_derivative_arrays`' checks
    S, d, n_lags = model.msd.shape
    with pytest.raises(ValueError, match='shape'):
        sens(x, model, prior, dmsd=np.zeros((1, S, d, n_lags + 1)))
    with pytest.raises(ValueError, match='disagree'):
        sens(x, model, prior, dmsd_inf=np.zeros((1, S, d)), dmean=np.zeros((2, S, d)))
    with pytest.raises(ValueError, match='not finite'):
        sens(x, model, prior, dmean=np.full((1, S, d), np.nan))
    with pytest.raises(_lib.BildAmdError, match='at most 4'):
        sens(x, model, prior, dmean=np.zeros((5, S, d)))
    empty = sens([], model, prior, dmean=np.zeros((2, S, d)))
    assert empty.grad.shape == (0, 2) and empty.fisher.shape == (0, 2, 2) and len(empty.log_evidence) == 0

    # fit_dwell
    family, derivs = DSC.exp_family(24)
    fit = bild_amd.GenericGaussianModel.fit_dwell
    start = dict(t0=1.0, t1=1.0)
    for bad in (dict(), dict(a=1, b=1, c=1, d=1, e=1), dict(t0=-1.0, t1=1.0), dict(t0=np.nan, t1=1.0)):
        with pytest.raises(ValueError):
            fit([x], family, bad)
    for kw in (dict(tol=0), dict(max_iter=0), dict(prior_tol=0), dict(prior_max_iter=0), dict(nan='drop'),
               dict(prior=DC.symmetric_chain(0.1, 19)), dict(prior=DC.make_prior('markov', rng, 3, 20)),
               dict(prior=prior, markov_start=np.full((2, 2), 0.5)), dict(markov_start=np.full((3, 3), 1 / 3))):
        with pytest.raises(ValueError):
            fit([x], family, start, **kw)
    with pytest.raises(ValueError):
        fit([], family, start)
    with pytest.raises(TypeError):
        fit([x], family, start, prior=(prior.log_init, prior.log_jump))
    with pytest.raises(ValueError):         # beyond the family's lags
        fit([C.random_traj(rng, 30)], family, start, prior=DC.symmetric_chain(0.1, 40))
    with pytest.raises(ValueError, match='shape'):      # derivatives of the wrong shape, with either kind of prior
        fit([x], family, start, prior=prior, derivatives=lambda t0, t1: (np.zeros((2, 2, 2, 7)), None, None))
    with pytest.raises(ValueError, match='shape'):
        fit([x], family, start, derivatives=lambda t0, t1: (np.zeros((2, 2, 2, 7)), None, None))
    assert bild_amd.models.FitResult(None, {}, {}, None, 0.0, 0, True, [], ()).prior_fit is None
    # what `fit_dwell` catches from the inner fit: a ValueError of its own type that carries the total and the pointer
    err = bild_amd.exact.EvidenceNotFinite(np.nan)
    assert isinstance(err, ValueError) and np.isnan(err.total) and "nan='omit'" in str(err)
    assert bild_amd.exact.EvidenceNotFinite(-np.inf).total == -np.inf
