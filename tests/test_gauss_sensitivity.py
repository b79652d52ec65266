"""
The NumPy oracle of GenericGaussianModel's sensitivities (tests/gauss_sensitivity_oracle.py), pinned to the likelihood
oracle and the reference goldens, to finite differences and to the exact Gaussian Fisher information; the finite
differences of `GenericGaussianModel.fit`; argument errors of `logL_sensitivities` before any device work.  CPU only.
"""
import glob
import os

import numpy as np
import pytest

import gauss_oracle as G
import gauss_sensitivity_oracle as GS
from gauss_sim_cases import msd_exp, msd_pow

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDENS = sorted(glob.glob(os.path.join(HERE, 'golden', 'gauss', '*.npz')))


def load(path):
    z = np.load(path)
    return {k: z[k] for k in z.files}


def golden_family(g):
    """ parameters every golden admits: a scale of each state's MSD (and msd(inf)), and one shift of all the means """
    S, d, L = g['msd'].shape
    P = S + 1
    dmsd, dmsd_inf, dmean = np.zeros((P, S, d, L)), np.zeros((P, S, d)), np.zeros((P, S, d))
    for s in range(S):
        dmsd[s, s], dmsd_inf[s, s] = g['msd'][s], g['msd_inf'][s]
    dmean[S] = 1.0
    return dict(dmsd=dmsd, dmsd_inf=dmsd_inf, dmean=dmean)


def moved(g, derivs, p, h):
    """ the golden's arrays moved by h along parameter p of golden_family (which is linear) """
    return (g['msd'] + h * derivs['dmsd'][p], g['msd_inf'] + h * derivs['dmsd_inf'][p], g['mean'] + h * derivs['dmean'][p],
            g['order'])


def test_goldens_present():
    assert len(GOLDENS) == 4


@pytest.mark.parametrize('path', GOLDENS, ids=os.path.basename)
def test_oracle_logl_matches_reference_and_goldens(path):
    g = load(path)
    args = (g['msd'], g['msd_inf'], g['mean'], g['order'])
    for p, want in list(zip(g['profiles'], g['logL']))[:12]:
        ll, grad, F = GS.sensitivities(*args, g['x'], p, **golden_family(g))
        ref = G.logl_reference(*args, g['x'], p)
        if np.isnan(want):
            assert np.isnan(ll) and np.isnan(ref) and np.all(np.isnan(grad))
            continue
        assert abs(ll - ref) <= 1e-10 * max(1.0, abs(ref))
        assert abs(ll - want) <= 1e-10 * max(1.0, abs(want))


@pytest.mark.parametrize('path', GOLDENS, ids=os.path.basename)
def test_oracle_gradient_matches_finite_differences(path):
    g = load(path)
    derivs = golden_family(g)
    P = len(derivs['dmsd'])
    h = 1e-5
    checked = 0
    for p in g['profiles'][:4]:
        ll, grad, F = GS.sensitivities(g['msd'], g['msd_inf'], g['mean'], g['order'], g['x'], p, **derivs)
        if not np.isfinite(ll):
            continue
        fd = np.array([(G.logl_reference(*moved(g, derivs, q, h), g['x'], p) -
                        G.logl_reference(*moved(g, derivs, q, -h), g['x'], p)) / (2 * h) for q in range(P)])
        scale = max(1.0, float(np.max(np.abs(fd))))
        assert np.max(np.abs(grad - fd)) <= 1e-6 * scale, (grad, fd)
        assert np.allclose(F, F.T) and np.min(np.linalg.eigvalsh(F)) >= -1e-9 * np.max(np.abs(F))
        checked += 1
    assert checked >= 2


@pytest.mark.parametrize('order', [0, 1])
def test_innovations_fisher_expectation_is_the_exact_fisher(order):
    """ one unconditioned interval: the mean over data of the innovations form is 1/2 tr(C^-1 dC_p C^-1 dC_q) + dmu^T C^-1 dmu """
    rng = np.random.default_rng(7 + order)
    T, L = 24, 64
    msd = msd_exp(1.0, 6.0, 0.3, L) if order == 0 else msd_pow(0.6, 0.8, 0.3, L)
    table, inf = (msd[:-1], msd[-1]) if order == 0 else (msd, 0.0)
    m = 0.2
    dmsd = np.stack([table, np.zeros(L)])
    dinf = np.array([inf, 0.0])
    dmean = np.array([0.0, 1.0])
    u = np.arange(T)
    C = G.covariance(table, inf, u, order)
    dC = [G.covariance(dmsd[p], dinf[p], u, order) for p in range(2)]
    Ci = np.linalg.inv(C)
    n = len(C)
    exact = np.array([[0.5 * np.trace(Ci @ dC[p] @ Ci @ dC[q]) + dmean[p] * dmean[q] * np.ones(n) @ Ci @ np.ones(n)
                       for q in range(2)] for p in range(2)])
    chol = np.linalg.cholesky(C)
    draws = []
    for _ in range(400):
        y = chol @ rng.standard_normal(n) + m
        draws.append(GS.window_terms(table, inf, order, u, y, 0, False, dmsd, dinf, dmean)[2])
    draws = np.array(draws)
    mean, err = draws.mean(axis=0), draws.std(axis=0) / np.sqrt(len(draws))
    assert np.all(np.abs(mean - exact) <= 4 * err + 1e-12 * np.abs(exact)), (mean, exact, err)


def test_fit_finite_differences_match_analytic_derivatives():
    from bild_amd import GenericGaussianModel
    from bild_amd.gauss import _log_differences

    L = 300

    def family(A, G_):
        return [[(msd_exp(A, 10.0, 0.3, L), 0.1, 0), (msd_pow(G_, 0.8, 0.3, L), -0.2, 1)],
                [(msd_exp(2 * A, 5.0, 0.3, L), 0.0, 0), (msd_pow(0.5 * G_, 1.2, 0.3, L), 0.3, 1)]]

    theta = np.array([1.3, 0.7])
    dmsd, dinf, dmean = _log_differences(GenericGaussianModel, family, ('A', 'G_'), theta)
    t = np.arange(L, dtype=np.float64)
    want = np.zeros_like(dmsd)
    want_inf = np.zeros_like(dinf)
    want[0, 0, 0] = 2 * (1 - np.exp(-t / 10.0))
    want[0, 1, 0] = 4 * (1 - np.exp(-t / 5.0))
    want_inf[0, 0, 0], want_inf[0, 1, 0] = 2.0, 4.0
    want[1, 0, 1] = t ** 0.8
    want[1, 1, 1] = 0.5 * t ** 1.2
    want[..., 0] = 0.0
    assert np.max(np.abs(dmsd - want)) <= 1e-8 * np.max(np.abs(want))
    assert np.max(np.abs(dinf - want_inf)) <= 1e-8 * np.max(np.abs(want_inf))
    assert np.all(dmean == 0)


def test_argument_errors_before_device_work(built_lib):
    """ refusals on the host or in the library's checks: none of these reaches a device (there may be none) """
    from bild_amd import _lib
    from gauss_sim_cases import make_model
    model = make_model(2, 2, 3, L=64)
    S, d, L = model.msd.shape
    x = np.zeros((30, d))
    st = np.zeros((1, 30), dtype=np.int64)
    with pytest.raises(ValueError, match='disagree'):
        model.logL_sensitivities(st, x, dmsd=np.zeros((2, S, d, L)), dmean=np.zeros((1, S, d)))
    with pytest.raises(ValueError, match='shape'):
        model.logL_sensitivities(st, x, dmsd=np.zeros((2, S, d, L + 1)))
    with pytest.raises(ValueError, match='finite'):
        model.logL_sensitivities(st, x, dmean=np.full((1, S, d), np.nan))
    with pytest.raises(_lib.BildAmdError, match='at most 4'):
        model.logL_sensitivities(st, x, dmean=np.zeros((5, S, d)))
    with pytest.raises(ValueError, match='at most'):
        model.logL_sensitivities(np.zeros((1, 70), dtype=np.int64), np.zeros((70, d)))
    with pytest.raises(ValueError, match='states out of range'):
        model.logL_sensitivities(np.full((1, 30), 2), x)
    # the library's own checks, reached through the raw wrapper
    h = model.handle()
    seg = (np.zeros((1, 1), dtype=np.int32), np.zeros((1, 1), dtype=np.int32))
    with pytest.raises(_lib.BildAmdError, match='at most 4'):
        _lib.gauss_logl_sensitivities(h, [x], *seg, dmean=np.zeros((5, S, d)), P=5)
    with pytest.raises(_lib.BildAmdError, match='not finite'):
        _lib.gauss_logl_sensitivities(h, [x], *seg, dmsd_inf=np.full((1, S, d), np.inf), P=1)
    with pytest.raises(_lib.BildAmdError, match='MSD tables end'):
        _lib.gauss_logl_sensitivities(h, [np.zeros((70, d))], *seg)
    with pytest.raises(_lib.BildAmdError, match='state 5 out of range'):
        _lib.gauss_logl_sensitivities(h, [x], seg[0], np.full((1, 1), 5, dtype=np.int32))
    with pytest.raises(_lib.BildAmdError, match='traj_id'):
        _lib.gauss_logl_sensitivities(h, [x], *seg, traj_id=np.array([3], dtype=np.int32))
    with pytest.raises(ValueError, match='positive'):
        type(model).fit([x], 0, lambda a: model.state_spec, {'a': -1.0})
