"""
The evidence gradient on the GPU (bild_amd.exact.exact_sensitivities, csrc/gauss_segsens.hip):
against the NumPy oracle tests/segment_sensitivity_oracle.py on the cases of tests/test_segment_dp.py and at T = 52 ... 60 with
k_max = 12, against central differences of `exact_sample`'s own evidence at T = 1000, the bit-identity properties, the NaN
trajectory, the refusals, the calibration of the score and `GenericGaussianModel.fit_marginal`.
"""
import numpy as np
import pytest
from scipy.special import logsumexp

import bild_amd
import segment_cases as C
import segment_sensitivity_cases as SC
from bild_amd import _lib
from bild_amd.profiles import Loopingprofile
from test_segment_dp import CASES, build

pytestmark = pytest.mark.gpu

TOL = 1e-10     # relative to the largest entry of the row


def rel(got, want):
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    scale = np.max(np.abs(want)) if want.size else 0.0
    return 0.0 if want.size == 0 else float(np.max(np.abs(got - want))) / (scale if scale > 0 else 1.0)


def check_against_oracle(model, x, k_max, nan, k_prior=None, label='', want=None):
    """
    P = 0 ... 4 on one trajectory against the oracle (computed once at P = 4, or given as `want`); returns the worst relative
    deviation
    """
    K = k_max + 1
    if want is None:
        want = SC.oracle(model, x, k_max, P=4, log_k_prior=SC.log_prior(k_prior, K), nan=nan)      # (an integer: that k alone)
    ref = bild_amd.exact_sample(x, model, k_max=k_max, marginals=False, nan=nan)
    worst, base = 0.0, None
    for P in range(5):
        dmsd, dinf, dmean = SC.derivatives(model, P)
        r = bild_amd.exact_sensitivities(x, model, dmsd=dmsd, dmsd_inf=dinf, dmean=dmean, k_max=k_max, k_prior=k_prior, nan=nan)
        assert np.array_equal(r.logev[0], ref.evidence, equal_nan=True)          # bit for bit
        assert r.grad.shape == (1, P) and r.fisher.shape == (1, P, P) and r.k_posterior.shape == (1, K)
        if np.isnan(want['log_marginal']):
            assert np.isnan(r.log_marginal[0]) and np.isnan(r.expected_logL[0]) and np.all(np.isnan(r.k_posterior))
            assert np.all(np.isnan(r.grad)) and np.all(np.isnan(r.fisher))
            continue
        devs = {'log_marginal': rel(r.log_marginal[0], want['log_marginal']), 'k_posterior': rel(r.k_posterior[0], want['k_post']),
                'expected_logL': rel(r.expected_logL[0], want['exp_logl']), 'grad': rel(r.grad[0], want['grad'][:P]),
                'fisher': rel(r.fisher[0], want['fisher'][:P, :P])}
        print(f"{label} nan={nan} P={P}: " + ', '.join(f"{k} {v:.1e}" for k, v in devs.items()))
        for name, v in devs.items():
            assert v < TOL, (label, P, name, v)
        worst = max(worst, *devs.values())
        # the sums of one parameter do not depend on how many others ride along
        if base is None:
            base = r
        assert r.expected_logL[0] == base.expected_logL[0] and r.log_marginal[0] == base.log_marginal[0]
        assert np.array_equal(r.k_posterior, base.k_posterior)
    return worst


@pytest.mark.parametrize('name', list(CASES))
def test_against_oracle_small(name):
    model, x = build(name)
    modes = ('propagate', 'omit') if 'order0' in name else ('propagate',)
    for nan in modes:
        check_against_oracle(model, x, 4, nan, label=name)
        check_against_oracle(model, x, 4, nan, k_prior=[0.1, 0.4, 0.0, 0.0, 0.0] if nan == 'propagate' else [0.1, 0.4, 0.0, 0.3, 0.2],
                             label=name + ' prior')
        check_against_oracle(model, x, 4, nan, k_prior=1, label=name + ' k=1')


@pytest.mark.parametrize('T', [1, 2, 3, 6])
def test_short_trajectories(T):
    """ k beyond T - 1 has no profile and no weight; T = 1 has a first interval and nothing else """
    rng = np.random.default_rng(T)
    model = C.random_model(rng, 2, 12)
    x = C.random_traj(rng, T)
    check_against_oracle(model, x, 4, 'propagate', label=f'T={T}')
    r = bild_amd.exact_sensitivities(x, model, k_max=4)
    assert np.all(r.k_posterior[0, T:] == 0) and np.all(r.logev[0, T:] == -np.inf)


@pytest.mark.parametrize('case', ['s2_gapfree', 's3_gapfree', 's2_inner_gap', 's3_leading_and_inner_gap', 's2_order0_gap'])
def test_against_oracle_k12(case):
    S = int(case[1])
    rng = np.random.default_rng(sum(map(ord, case)))
    T = 60 if S == 2 else 52
    if 'order0' in case:
        model, x = SC.order0_gap_case(rng, 56)
        check_against_oracle(model, x, 12, 'propagate', label=case)                  # NaN: k >= 2 has NaN profiles
        check_against_oracle(model, x, 12, 'propagate', k_prior=[1, 1] + [0] * 11, label=case + ' k<=1')
        check_against_oracle(model, x, 12, 'omit', label=case)
        return
    model = C.random_model(rng, S, T + 8, orders=None if 'gapfree' in case else np.ones((S, 2), dtype=int))
    missing = () if 'gapfree' in case else (24, 25, 26, 27) if 'leading' not in case else (0, 1, 30, 31, 32, 33)
    x = C.random_traj(rng, T, missing)
    for nan in ('propagate', 'omit'):
        check_against_oracle(model, x, 12, nan, label=case)


# ---------------------------------------------------------------- a family with a known truth

BASE, TAU, NOISE = (0.5, 4.0), (3.0, 6.0), 0.02


def exp_family(L, d=2, with_noise=True):
    """ two ss_order-0 states with exponentially saturating MSDs a factor 8 apart: theta = (t0, t1[, n]), truth (1, 1[, NOISE]) """
    lags = np.arange(L, dtype=np.float64)

    def family(t0, t1, n=NOISE):
        return [[(np.append(t * b * (1 - np.exp(-lags / tau)) + n * (lags > 0), t * b + n), 0.0, 0)] * d
                for t, b, tau in zip((t0, t1), BASE, TAU)]

    def derivatives(t0, t1, n=NOISE):
        P = 3 if with_noise else 2
        dmsd, dinf = np.zeros((P, 2, d, L)), np.zeros((P, 2, d))
        for s in range(2):
            dmsd[s, s] = BASE[s] * (1 - np.exp(-lags / TAU[s]))
            dinf[s, s] = BASE[s]
        if with_noise:
            dmsd[2, :, :, 1:] = 1.0
            dinf[2] = 1.0
        return dmsd, dinf, None

    return family, derivatives


def prior_profiles(rng, n, T, k_max):
    """ profiles from the prior of the recursion: k uniform, switch frames a uniform k-subset of 1 ... T - 1, a uniform trace """
    out = []
    for _ in range(n):
        k = int(rng.integers(0, k_max + 1))
        sw = np.sort(rng.choice(np.arange(1, T), size=k, replace=False))
        s = int(rng.integers(0, 2))
        states = np.zeros(T, dtype=int)
        edges = [0, *sw, T]
        for i in range(k + 1):
            states[edges[i]:edges[i + 1]] = (s + i) % 2
        out.append(states)
    return out


@pytest.mark.parametrize('missing', [None, 0.1])
def test_T1000_gradient_against_differences_of_exact_sample(missing):
    T, k_max = 1000, 20
    nan = 'propagate' if missing is None else 'omit'
    family, derivatives = exp_family(T)
    rng = np.random.default_rng(1000)
    truth = bild_amd.GenericGaussianModel(family(1.0, 1.0, NOISE))
    x = truth.trajectories_from_loopingprofiles(prior_profiles(rng, 1, T, 6), missing_frames=missing, seed=77)[0][:]
    theta = np.array([1.5, 1 / 1.5, 1.5 * NOISE])

    def log_marginal(th):
        r = bild_amd.exact_sample(x, bild_amd.GenericGaussianModel(family(*th)), k_max=k_max, marginals=False, nan=nan)
        return logsumexp(r.evidence) - np.log(k_max + 1), r

    model = bild_amd.GenericGaussianModel(family(*theta))
    r = bild_amd.exact_sensitivities(x, model, *derivatives(*theta)[:2], k_max=k_max, nan=nan)
    lm, ref = log_marginal(theta)
    assert np.array_equal(r.logev[0], ref.evidence)
    assert abs(r.log_marginal[0] - lm) <= 1e-12 * abs(lm)
    want_el = r.k_posterior[0] @ (ref.KL + ref.evidence)
    print(f"expected_logL {r.expected_logL[0]!r} against sum_k k_post (KL + logev) {want_el!r}")
    assert abs(r.expected_logL[0] - want_el) <= 1e-10 * abs(want_el)
    g_log = r.grad[0] * theta
    quot = {}
    for h in (1e-4, 2e-4):
        q = np.zeros(3)
        for p in range(3):
            e = np.zeros(3)
            e[p] = h
            q[p] = (log_marginal(theta * np.exp(e))[0] - log_marginal(theta * np.exp(-e))[0]) / (2 * h)
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
    L = 160
    family, derivatives = exp_family(L)
    model = bild_amd.GenericGaussianModel(family(1.2, 0.9, 0.03))
    xs = [C.random_traj(rng, 150, (40, 41, 90)), C.random_traj(rng, 120), C.random_traj(rng, 97, (0, 1, 50, 51, 52))]
    return model, xs, derivatives(1.2, 0.9, 0.03)[:2]


FIELDS = ('log_marginal', 'k_posterior', 'logev', 'grad', 'expected_logL', 'fisher')


def test_bit_identity_across_calls_orders_batches_and_scratch():
    model, xs, (dmsd, dinf) = bit_case()
    kw = dict(dmsd=dmsd, dmsd_inf=dinf, k_max=6, nan='omit')
    a = bild_amd.exact_sensitivities(xs, model, **kw)
    assert np.all(np.isfinite(a.grad)) and np.all(np.isfinite(a.fisher))
    b = bild_amd.exact_sensitivities(xs, model, **kw)
    perm = [2, 0, 1]
    c = bild_amd.exact_sensitivities([xs[i] for i in perm], model, **kw)
    small = bild_amd.exact_sensitivities(xs, model, scratch_bytes=1 << 19, **kw)       # one trajectory and one factorisation a chunk
    for f in FIELDS:
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
        assert np.array_equal(getattr(a, f)[perm], getattr(c, f)), f
        assert np.array_equal(getattr(a, f), getattr(small, f)), f
    for i, x in enumerate(xs):
        one = bild_amd.exact_sensitivities(x, model, **kw)
        for f in FIELDS:
            assert np.array_equal(getattr(a, f)[i], getattr(one, f)[0]), (i, f)
    # without the Fisher matrix, and with fewer parameters: the same sums
    nof = bild_amd.exact_sensitivities(xs, model, fisher=False, **kw)
    assert nof.fisher is None and np.array_equal(nof.grad, a.grad)
    p1 = bild_amd.exact_sensitivities(xs, model, dmsd=dmsd[:1], dmsd_inf=dinf[:1], k_max=6, nan='omit')
    assert np.array_equal(p1.expected_logL, a.expected_logL) and np.array_equal(p1.grad[:, 0], a.grad[:, 0])


def test_nan_trajectory_alone():
    rng = np.random.default_rng(3)
    model, bad = SC.order0_gap_case(rng, 56)
    good = [C.random_traj(rng, 50), C.random_traj(rng, 56)]
    dmsd, dinf, dmean = SC.derivatives(model, 3)
    kw = dict(dmsd=dmsd, dmsd_inf=dinf, dmean=dmean, k_max=5)
    r = bild_amd.exact_sensitivities([good[0], bad, good[1]], model, **kw)
    assert np.isnan(r.log_marginal[1]) and np.all(np.isnan(r.grad[1])) and np.all(np.isnan(r.fisher[1]))
    assert np.isnan(r.expected_logL[1]) and np.all(np.isnan(r.k_posterior[1]))
    assert np.all(np.isfinite(r.logev[1, :2])) and np.all(np.isnan(r.logev[1, 2:]))
    for i, x in ((0, good[0]), (2, good[1])):
        one = bild_amd.exact_sensitivities(x, model, **kw)
        for f in FIELDS:
            assert np.all(np.isfinite(getattr(r, f)[i])) and np.array_equal(getattr(r, f)[i], getattr(one, f)[0]), (i, f)
    # no weight on the NaN ks, or nan='omit': finite
    assert np.all(np.isfinite(bild_amd.exact_sensitivities(bad, model, k_prior=[1, 1, 0, 0, 0, 0], **kw).grad))
    assert np.all(np.isfinite(bild_amd.exact_sensitivities(bad, model, nan='omit', **kw).grad))


def test_library_refusals():
    rng = np.random.default_rng(4)
    model = C.random_model(rng, 2, 40)
    x = C.random_traj(rng, 30)
    ts = model.trajset(x)
    h, tr = model.handle(), model.transitions
    for bad in (np.nan, np.inf):
        prior = np.zeros((1, 4))
        prior[0, 2] = bad
        with pytest.raises(_lib.BildAmdError, match='NaN or \\+inf'):
            _lib.gauss_segment_sensitivities(h, ts, [x], 3, tr, log_k_prior=prior)
    with pytest.raises(_lib.BildAmdError, match='-inf everywhere'):
        _lib.gauss_segment_sensitivities(h, ts, [x], 3, tr, log_k_prior=np.full((1, 4), -np.inf))
    with pytest.raises(_lib.BildAmdError, match='k_max = 65'):
        _lib.gauss_segment_sensitivities(h, ts, [x], 65, tr)
    with pytest.raises(_lib.BildAmdError, match='negative'):
        _lib.gauss_segment_sensitivities(h, ts, [x], 3, tr, scratch_bytes=-1)
    with pytest.raises(_lib.BildAmdError, match='at most 4'):
        _lib.gauss_segment_sensitivities(h, ts, [x], 3, tr, dmean=np.zeros((5, 2, 2)), P=5)
    with pytest.raises(_lib.BildAmdError, match='not finite'):
        _lib.gauss_segment_sensitivities(h, ts, [x], 3, tr, dmean=np.full((1, 2, 2), np.nan), P=1)


def test_score_is_calibrated_under_the_prior():
    """ the score of the marginal likelihood has mean zero for data drawn from the model, the prior over profiles included """
    T, k_max, n = 100, 3, 2000
    family, derivatives = exp_family(T)
    rng = np.random.default_rng(2000)
    truth = bild_amd.GenericGaussianModel(family(1.0, 1.0, NOISE))
    trajs = [t[:] for t in truth.trajectories_from_loopingprofiles(prior_profiles(rng, n, T, k_max), seed=5)]
    r = bild_amd.exact_sensitivities(trajs, truth, *derivatives(1.0, 1.0, NOISE)[:2], k_max=k_max)
    assert np.all(np.isfinite(r.grad))
    mean, se = r.grad.mean(axis=0), r.grad.std(axis=0, ddof=1) / np.sqrt(n)
    print(f"score: mean {mean}, standard error {se}, z {mean / se}")
    assert np.all(np.abs(mean) < 4 * se), (mean, se)
    # Fisher's other identity: the variance of the score is what the posterior-weighted matrix overstates
    print(f"var(score) diag {r.grad.var(axis=0, ddof=1)}, mean weighted Fisher diag {np.diagonal(r.fisher.mean(axis=0))}")


def test_fit_marginal_recovers_the_truth():
    T, k_max, n = 200, 3, 64
    family, derivatives = exp_family(T, with_noise=False)
    rng = np.random.default_rng(64)
    truth = bild_amd.GenericGaussianModel(family(1.0, 1.0))
    profiles = prior_profiles(rng, n, T, k_max)
    trajs = [t[:] for t in truth.trajectories_from_loopingprofiles(profiles, seed=9)]
    start = dict(t0=1.5, t1=1 / 1.5)
    fit = bild_amd.GenericGaussianModel.fit_marginal
    an = fit(trajs, family, start, derivatives=derivatives, k_max=k_max)
    fd = fit(trajs, family, start, k_max=k_max)
    known = bild_amd.GenericGaussianModel.fit(trajs, [Loopingprofile(p) for p in profiles], family, start, derivatives=derivatives)
    print(f"\nmarginal, analytic derivatives: {an}\nmarginal, difference derivatives: {fd}\nknown profiles: {known}")
    print(f"history of the log marginal: {[round(h[1], 4) for h in an.history]}")
    for res in (an, fd):
        assert res.converged
        for name in start:
            assert abs(res.params[name] - 1.0) < 4 * res.se[name], (name, res.params[name], res.se[name])
            assert abs(res.params[name] - known.params[name]) < 4 * res.se[name], (name, res.params[name], known.params[name])
    assert an.params['t1'] / an.params['t0'] * BASE[1] / BASE[0] >= 4
    for name in start:
        assert abs(fd.params[name] - an.params[name]) <= 1e-5 * abs(an.params[name])
