"""
The evidence gradient under a dwell-time prior on the GPU (bild_amd.exact.exact_dwell_sensitivities, csrc/gauss_dwellsens.hip,
DESIGN.md section 23): against the NumPy oracle tests/dwell_sensitivity_oracle.py around the 64-frame tiles of the weight
kernel, against `logL_sensitivities` under a prior that admits one profile, against `exact_sensitivities` on the symmetric
two-state chain, against central differences of `exact_dwell`'s own evidence, the bit-identity properties, the refusals, and
`GenericGaussianModel.fit_dwell`.
"""
import numpy as np
import pytest

import bild_amd
import dwell_cases as DC
import dwell_sensitivity_cases as DSC
import segment_cases as C
import segment_sensitivity_cases as SC
from bild_amd import _lib
from bild_amd.profiles import Loopingprofile

pytestmark = pytest.mark.gpu

# Absolute, in units of the row's largest entry: the bar section 21 gives its own sums of segment weights, the counts.
# Worst seen on these cases: 1.3e-13 (S = 3, T = 193), far inside the bar, which is not tightened to it.
TOL = 1e-9

FIELDS = ('log_evidence', 'n_nan_windows', 'grad', 'expected_logL', 'fisher')


def rel(got, want):
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    scale = np.max(np.abs(want)) if want.size else 0.0
    return 0.0 if want.size == 0 else float(np.max(np.abs(got - want))) / (scale if scale > 0 else 1.0)


@pytest.mark.parametrize('case', DSC.ORACLE_CASES, ids=lambda c: f"S{c[0]}_T{c[1]}_{c[3]}_{c[4]}" + ('_order0_gap' if c[2] == 'order0_gap' else ''))
def test_against_oracle(case):
    """ P = 0 ... 4 against the oracle's answer at P = 4; log_evidence and n_nan_windows against `exact_dwell` bit for bit """
    nan = case[4]
    model, x, prior = DSC.oracle_case(*case[:4])
    want = DSC.oracle_answer(case)
    ref = bild_amd.exact_dwell(x, model, prior, marginals=False, nan=nan)
    assert want['n_nan_windows'] == ref.n_nan_windows and (want['n_nan_windows'] > 0) == (case[2] == 'order0_gap')
    base = None
    for P in range(5):
        dmsd, dinf, dmean = DSC.derivatives(model, P)
        r = bild_amd.exact_dwell_sensitivities(x, model, prior, dmsd=dmsd, dmsd_inf=dinf, dmean=dmean, nan=nan)
        assert np.array_equal(r.log_evidence, [ref.log_evidence], equal_nan=True)       # bit for bit
        assert r.n_nan_windows.dtype == np.int64 and r.n_nan_windows[0] == ref.n_nan_windows
        assert r.grad.shape == (1, P) and r.fisher.shape == (1, P, P)
        if np.isnan(want['logev']):
            assert nan == 'propagate' and np.isnan(r.expected_logL[0]) and np.all(np.isnan(r.grad)) and np.all(np.isnan(r.fisher))
            continue
        devs = {'log_evidence': rel(r.log_evidence[0], want['logev']), 'expected_logL': rel(r.expected_logL[0], want['exp_logl']),
                'grad': rel(r.grad[0], want['grad'][:P]), 'fisher': rel(r.fisher[0], want['fisher'][:P, :P])}
        print(f"{case} P={P}: " + ', '.join(f"{k} {v:.1e}" for k, v in devs.items()))
        for name, v in devs.items():
            assert v < TOL, (case, P, name, v)
        # the sums of one parameter do not depend on how many others ride along
        if base is None:
            base = r
        assert r.expected_logL[0] == base.expected_logL[0]
    assert (base is None) == (case[2] == 'order0_gap' and nan == 'propagate')


@pytest.mark.parametrize('T,flat', [(193, False), (260, True)])
def test_prior_that_admits_one_profile(T, flat):
    """ all posterior weight on one profile: the outputs are `logL_sensitivities` of that profile.  Independent of the oracle. """
    rng = np.random.default_rng(T)
    model = C.random_model(rng, 2, T + 8)
    x = C.random_traj(rng, T, (30, 131))
    if flat:        # every jump at -inf: jobs of more than 256 rows
        prior, states = DSC.flat_prior(T + 3), np.zeros(T, dtype=int)
    else:           # 70 frames of state 0, 60 of state 1, and a censored last segment of 63
        prior, states = DSC.one_profile_prior(T, (70, 60), T + 3)
        assert np.array_equal(states, np.repeat([0, 1, 0], [70, 60, 63]))
    dmsd, dinf, dmean = SC.derivatives(model, 4)
    logl, g, F = model.logL_sensitivities(states[None], x, dmsd=dmsd, dmsd_inf=dinf, dmean=dmean)
    r = bild_amd.exact_dwell_sensitivities(x, model, prior, dmsd=dmsd, dmsd_inf=dinf, dmean=dmean)
    devs = {'log_evidence': rel(r.log_evidence[0], logl[0]), 'expected_logL': rel(r.expected_logL[0], logl[0]),
            'grad': rel(r.grad[0], g[0]), 'fisher': rel(r.fisher[0], F[0])}
    print(f"T={T}: " + ', '.join(f"{k} {v:.1e}" for k, v in devs.items()))
    for name, v in devs.items():
        assert v < 1e-10, (name, v)


def test_symmetric_chain_against_exact_sensitivities():
    """ the symmetric chain's prior depends on k alone: the outputs are `exact_sensitivities`' under the matching prior over k """
    T, p = 60, 0.07
    rng = np.random.default_rng(60)
    model = C.random_model(rng, 2, T + 8)
    x = C.random_traj(rng, T, (25,))
    dmsd, dinf, dmean = SC.derivatives(model, 4)
    kw = dict(dmsd=dmsd, dmsd_inf=dinf, dmean=dmean)
    r = bild_amd.exact_dwell_sensitivities(x, model, DC.symmetric_chain(p, T), **kw)
    w = DSC.k_weights_of_symmetric_chain(p, T)
    s = bild_amd.exact_sensitivities(x, model, k_max=T - 1, k_prior=w, **kw)
    devs = {'log_evidence': rel(r.log_evidence[0], s.log_marginal[0]), 'grad': rel(r.grad[0], s.grad[0]),
            'expected_logL': rel(r.expected_logL[0], s.expected_logL[0]), 'fisher': rel(r.fisher[0], s.fisher[0])}
    print(', '.join(f"{k} {v:.1e}" for k, v in devs.items()))
    assert devs['grad'] < 1e-9 and devs['expected_logL'] < 1e-9
    assert devs['log_evidence'] < 1e-9 and devs['fisher'] < 1e-9


@pytest.mark.parametrize('missing', [None, 0.1])
def test_gradient_against_differences_of_exact_dwell(missing):
    T = 260
    nan = 'propagate' if missing is None else 'omit'
    family, derivs = DSC.exp_family(T)
    rng = np.random.default_rng(260)
    truth = bild_amd.GenericGaussianModel(family(1.0, 1.0, DSC.NOISE))
    profile = DSC.markov_profiles(rng, 1, T, DSC.FIT_P)
    x = truth.trajectories_from_loopingprofiles(profile, missing_frames=missing, seed=77)[0][:]
    prior = bild_amd.DwellPrior.markov(DSC.FIT_P, n=T)
    theta = np.array([1.5, 1 / 1.5, 1.5 * DSC.NOISE])

    def logev(th):
        return bild_amd.exact_dwell(x, bild_amd.GenericGaussianModel(family(*th)), prior, marginals=False, nan=nan).log_evidence

    r = bild_amd.exact_dwell_sensitivities(x, bild_amd.GenericGaussianModel(family(*theta)), prior, *derivs(*theta)[:2], nan=nan)
    assert r.log_evidence[0] == logev(theta)
    g_log = r.grad[0] * theta
    quot = {}
    for h in (1e-4, 2e-4):
        q = np.zeros(3)
        for p in range(3):
            e = np.zeros(3)
            e[p] = h
            q[p] = (logev(theta * np.exp(e)) - logev(theta * np.exp(-e))) / (2 * h)
        quot[h] = q
    norm = np.linalg.norm(g_log)
    dev = np.max(np.abs(g_log - quot[1e-4])) / norm
    spread = np.max(np.abs(quot[1e-4] - quot[2e-4])) / norm
    print(f"missing={missing}: grad (log theta) {g_log}, quotient(1e-4) {quot[1e-4]}, deviation {dev:.2e} of the norm, "
          f"spread of the two quotients {spread:.2e}")
    assert norm > 10            # far from the optimum
    assert dev < 1e-5, (dev, spread)


def bit_case():
    rng = np.random.default_rng(21)
    family, derivs = DSC.exp_family(200)
    model = bild_amd.GenericGaussianModel(family(1.2, 0.9, 0.03))
    xs = [C.random_traj(rng, 40, (7,)), C.random_traj(rng, 65), C.random_traj(rng, 193, (0, 1, 64, 65, 130)), C.random_traj(rng, 65, (30, 31))]
    return model, xs, DC.make_prior('nongeometric', rng, 2, 200), derivs(1.2, 0.9, 0.03)[:2]


def test_bit_identity_across_calls_orders_batches_and_scratch():
    model, xs, prior, (dmsd, dinf) = bit_case()
    kw = dict(dmsd=dmsd, dmsd_inf=dinf, nan='omit')
    sens = bild_amd.exact_dwell_sensitivities
    a = sens(xs, model, prior, **kw)
    assert np.all(np.isfinite(a.grad)) and np.all(np.isfinite(a.fisher)) and np.all(np.isfinite(a.log_evidence))
    b = sens(xs, model, prior, **kw)
    perm = [2, 0, 3, 1]
    c = sens([xs[i] for i in perm], model, prior, **kw)
    small = sens(xs, model, prior, scratch_bytes=1 << 19, **kw)     # one trajectory and one factorisation a chunk
    for f in FIELDS:
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
        assert np.array_equal(getattr(a, f)[perm], getattr(c, f)), f
        assert np.array_equal(getattr(a, f), getattr(small, f)), f
    for i, x in enumerate(xs):
        one = sens(x, model, prior, **kw)
        for f in FIELDS:
            assert np.array_equal(getattr(a, f)[i], getattr(one, f)[0]), (i, f)
    # without the Fisher matrix, and with fewer parameters: the same sums
    nof = sens(xs, model, prior, fisher=False, **kw)
    assert nof.fisher is None and np.array_equal(nof.grad, a.grad) and np.array_equal(nof.expected_logL, a.expected_logL)
    p1 = sens(xs, model, prior, dmsd=dmsd[:1], dmsd_inf=dinf[:1], nan='omit')
    assert np.array_equal(p1.expected_logL, a.expected_logL) and np.array_equal(p1.grad[:, 0], a.grad[:, 0])
    assert np.array_equal(p1.fisher[:, 0, 0], a.fisher[:, 0, 0])
    ev = bild_amd.exact_dwell(xs, model, prior, marginals=False, nan='omit')
    assert np.array_equal(a.log_evidence, [e.log_evidence for e in ev])


def test_nan_trajectory_and_trajectory_without_a_profile():
    rng = np.random.default_rng(3)
    model, bad = SC.order0_gap_case(rng, 56)
    good = [C.random_traj(rng, 50), C.random_traj(rng, 56)]
    prior = DC.make_prior('markov', rng, 2, 60)
    dmsd, dinf, dmean = SC.derivatives(model, 3)
    kw = dict(dmsd=dmsd, dmsd_inf=dinf, dmean=dmean)
    sens = bild_amd.exact_dwell_sensitivities
    r = sens([good[0], bad, good[1]], model, prior, **kw)
    assert r.n_nan_windows[1] > 0 and r.n_nan_windows[0] == 0 and r.n_nan_windows[2] == 0
    assert np.isnan(r.log_evidence[1]) and np.all(np.isnan(r.grad[1])) and np.all(np.isnan(r.fisher[1])) and np.isnan(r.expected_logL[1])
    for i, x in ((0, good[0]), (2, good[1])):
        one = sens(x, model, prior, **kw)
        for f in FIELDS:
            assert np.all(np.isfinite(getattr(r, f)[i])) and np.array_equal(getattr(r, f)[i], getattr(one, f)[0]), (i, f)
    omit = sens(bad, model, prior, nan='omit', **kw)
    assert np.all(np.isfinite(omit.grad)) and np.isfinite(omit.log_evidence[0]) and omit.n_nan_windows[0] == r.n_nan_windows[1]
    # no profile of positive weight: the evidence is -inf, the rest NaN, and the neighbours are untouched
    T = 50
    no = DC.prior_of('impossible', rng, 2, 60, T)
    r = sens([good[0], good[1]], model, no, **kw)
    assert r.log_evidence[0] == -np.inf and np.all(np.isnan(r.grad[0])) and np.all(np.isnan(r.fisher[0])) and np.isnan(r.expected_logL[0])
    one = sens(good[1], model, no, **kw)            # 56 frames: the one segment survives
    for f in FIELDS:
        assert np.all(np.isfinite(getattr(r, f)[1])) and np.array_equal(getattr(r, f)[1], getattr(one, f)[0]), f


def test_library_refusals():
    rng = np.random.default_rng(4)
    model = C.random_model(rng, 2, 40)
    x = C.random_traj(rng, 30)
    ts = model.trajset(x)
    h = model.handle()
    prior = DC.symmetric_chain(0.1, 30)
    tabs = [prior.log_init, prior.log_jump, prior.log_dwell, prior.log_surv]
    call = _lib.gauss_dwell_sensitivities
    call(h, ts, [x], *tabs)
    with pytest.raises(_lib.BildAmdError, match='negative'):
        call(h, ts, [x], *tabs, scratch_bytes=-1)
    with pytest.raises(_lib.BildAmdError, match='more than the L = 29'):
        call(h, ts, [x], tabs[0], tabs[1], tabs[2][:, :29], tabs[3][:, :29])
    with pytest.raises(_lib.BildAmdError, match='diagonal'):
        call(h, ts, [x], tabs[0], np.zeros((2, 2)), tabs[2], tabs[3])
    with pytest.raises(_lib.BildAmdError, match='finite or -inf'):
        call(h, ts, [x], tabs[0], tabs[1], np.full((2, 30), np.nan), tabs[3])
    with pytest.raises(_lib.BildAmdError, match='-inf everywhere'):
        call(h, ts, [x], np.full(2, -np.inf), tabs[1], tabs[2], tabs[3])
    with pytest.raises(_lib.BildAmdError, match='at most 4'):
        call(h, ts, [x], *tabs, dmean=np.zeros((5, 2, 2)), P=5)
    with pytest.raises(_lib.BildAmdError, match='not finite'):
        call(h, ts, [x], *tabs, dmean=np.full((1, 2, 2), np.nan), P=1)
    five = C.random_model(rng, 5, 40)
    p5 = DC.make_prior('markov', rng, 5, 30)
    with pytest.raises(_lib.BildAmdError, match='at most 4'):
        call(five.handle(), five.trajset(x), [x], p5.log_init, p5.log_jump, p5.log_dwell, p5.log_surv)


# ---------------------------------------------------------------- the fit

@pytest.fixture(scope='module')
def fit_data():
    T, n = 128, 32
    family, derivs = DSC.exp_family(T, with_noise=False)
    rng = np.random.default_rng(128)
    truth = bild_amd.GenericGaussianModel(family(1.0, 1.0))
    profiles = DSC.markov_profiles(rng, n, T, DSC.FIT_P)
    trajs = [t[:] for t in truth.trajectories_from_loopingprofiles(profiles, seed=9)]
    return family, derivs, truth, profiles, trajs


def count_builds(monkeypatch):
    made = []
    real = _lib.GaussTrajSetHandle

    def counting(*a, **k):
        made.append(1)
        return real(*a, **k)
    monkeypatch.setattr(_lib, 'GaussTrajSetHandle', counting)
    return made


def check_fit(res, at_truth):
    assert res.converged
    objective = [h[1] for h in res.history]
    assert all(b >= a for a, b in zip(objective, objective[1:])), objective
    assert res.logL == objective[-1]
    print(f"objective at the generating point {at_truth!r}, at the fit {res.logL!r}")
    assert res.logL >= at_truth - 1e-6, (res.logL, at_truth)


def test_fit_dwell_with_a_fitted_markov_prior(fit_data, monkeypatch):
    family, derivs, truth, profiles, trajs = fit_data
    T = len(trajs[0])
    start = dict(t0=1.5, t1=1 / 1.5)
    markov_start = np.array([[0.9, 0.1], [0.2, 0.8]])       # the switching probabilities 2x off
    made = count_builds(monkeypatch)
    res = bild_amd.GenericGaussianModel.fit_dwell(trajs, family, start, markov_start=markov_start, derivatives=derivs)
    assert len(made) == res.n_iter      # one trajectory-set build per evaluation, the inner EM and the gradient call on it
    pf = res.prior_fit
    known = bild_amd.GenericGaussianModel.fit(trajs, [Loopingprofile(p) for p in profiles], family, start, derivatives=derivs)
    print(f"\nfit_dwell, prior=None: {res}\n  P {pf.P.tolist()}, init {pf.init.tolist()}, inner iterations of the accepted evaluation "
          f"{pf.n_iter}\nknown profiles: {known}\nhistory of the objective: {[round(h[1], 4) for h in res.history]}")
    assert isinstance(pf, bild_amd.MarkovPriorFit) and pf.converged
    at_truth = bild_amd.exact_dwell_sensitivities(trajs, truth, bild_amd.DwellPrior.markov(DSC.FIT_P, n=T)).log_evidence.sum()
    check_fit(res, at_truth)
    # the accepted evaluation sits at an EM fixed point: one further step moves P by less than prior_tol
    again = bild_amd.fit_markov_prior(trajs, res.model, start=(pf.P, pf.init), max_iter=1, tol=1e-10)
    step = float(np.max(np.abs(again.P - pf.P)))
    print(f"one further EM step moves P by {step:.2e}")
    assert step < 1e-10
    # the objective is the evidence at (theta^, P^)
    ev = bild_amd.exact_dwell(trajs, res.model, pf.prior(T), marginals=False)
    assert res.logL == float(np.sum([e.log_evidence for e in ev]))
    assert set(res.se) == set(start) and all(np.isfinite(v) and v > 0 for v in res.se.values())


def test_fit_dwell_under_a_fixed_prior(fit_data, monkeypatch):
    family, derivs, truth, profiles, trajs = fit_data
    T = len(trajs[0])
    prior = bild_amd.DwellPrior.markov(DSC.FIT_P, n=T)
    made = count_builds(monkeypatch)
    res = bild_amd.GenericGaussianModel.fit_dwell(trajs, family, dict(t0=1.5, t1=1 / 1.5), prior=prior, derivatives=derivs)
    assert len(made) == res.n_iter and res.prior_fit is None
    print(f"\nfit_dwell, the generating prior held fixed: {res}\nhistory of the objective: {[round(h[1], 4) for h in res.history]}")
    at_truth = bild_amd.exact_dwell_sensitivities(trajs, truth, prior).log_evidence.sum()
    check_fit(res, at_truth)


def test_fit_dwell_refuses_a_nan_start():
    rng = np.random.default_rng(5)
    T = 56
    lags = np.arange(T + 8)

    def family(a):
        return [[(np.append(a * (lags * 0.5 + 0.1), 50.0 * a), 0.3 * s, 0), (a * lags * (0.5 + s), 0.0, 1)] for s in range(2)]

    x = C.random_traj(rng, T)
    x[20:26, 0] = np.nan
    prior = DC.make_prior('markov', rng, 2, T)
    for pr in (prior, None):
        with pytest.raises(ValueError, match="nan='omit'"):
            bild_amd.GenericGaussianModel.fit_dwell([x], family, dict(a=1.0), prior=pr)
