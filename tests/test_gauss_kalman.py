"""
The NumPy oracle of GenericGaussianModel's per-frame moments (tests/gauss_kalman_oracle.py), pinned to the likelihood
oracle and the reference goldens, its explicit conditioning pinned to the Cholesky form the kernels compute, and the
argument errors of `kalman` and `kalman_mixture` before any device work.  CPU only.
"""
import glob
import os

import numpy as np
import pytest

import gauss_kalman_oracle as GK
import gauss_oracle as G

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDENS = sorted(glob.glob(os.path.join(HERE, 'golden', 'gauss', '*.npz')))


def load(path):
    z = np.load(path)
    return {k: z[k] for k in z.files}


def arrays(model):
    return model.msd, model.msd_inf, model.mean, model.ss_order


def _agree(a, b, tol):
    """ equal NaN patterns and |a - b| <= tol max(1, |b|) elsewhere """
    a, b = np.asarray(a), np.asarray(b)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(b)
    assert np.all(np.abs(a[ok] - b[ok]) <= tol * np.maximum(1.0, np.abs(b[ok])))


@pytest.mark.parametrize('path', GOLDENS, ids=os.path.basename)
def test_terms_sum_to_the_goldens(path):
    g = load(path)
    arr = (g['msd'], g['msd_inf'], g['mean'], g['order'])
    for states, want in zip(g['profiles'][:12], g['logL'][:12]):
        got = np.sum(GK.kalman(*arr, g['x'], states)['terms'])
        ref = G.logl_reference(*arr, g['x'], states)
        if np.isnan(want):
            assert np.isnan(got) and np.isnan(ref)
            continue
        assert abs(got - want) <= 1e-8 * max(1.0, abs(want))
        assert abs(got - ref) <= 1e-10 * max(1.0, abs(ref))


@pytest.mark.parametrize('seed', [0, 1])
def test_oracle_on_the_cases(seed):
    model, cases = GK.cases(seed)
    arr = arrays(model)
    n_nan = 0
    for x, states_list in cases:
        for states in states_list:
            out = GK.kalman(*arr, x, states)
            chol = GK.kalman(*arr, x, states, cholesky=True)
            for name in GK.OUTPUTS:      # prefix and Schur conditioning against the Cholesky form
                _agree(out[name], chol[name], 1e-10)
            ref = G.logl_reference(*arr, x, states)
            total = np.sum(out['terms'])
            if np.isnan(ref):
                n_nan += 1
                assert np.isnan(total)
            else:
                assert abs(total - ref) <= 1e-10 * max(1.0, abs(ref))
            valid = ~np.isnan(x)
            assert np.array_equal(out['smooth_mean'][valid], x[valid]) and np.all(out['smooth_var'][valid] == 0)
            # predictive moments and innovations exist exactly where a term is counted
            counted = (out['terms'] != 0) & ~np.isnan(out['terms'])
            assert np.array_equal(~np.isnan(out['innov']), counted)
            assert np.all(out['smooth_var'][~valid & ~np.isnan(out['smooth_var'])] > 0)
    assert n_nan >= 1         # the cases include a window without a valid frame


def test_gap_moments_are_gaussian_conditionals():
    """ one ss_order-0 window: the Schur complement equals conditioning the joint Gaussian by sampling-free algebra """
    from bild_amd.gauss import covariance
    model, _ = GK.cases(0)
    msd, msd_inf = model.msd[0, 0], model.msd_inf[0, 0]
    u = np.array([0, 1, 4, 5, 9])
    t = 7
    y = np.array([0.3, -0.2, 0.5, 0.1, -0.4])
    J = covariance(msd, msd_inf, np.array([0, 1, 4, 5, 9, 7]), 0)
    P = np.linalg.inv(J)         # precision: the conditional of the last coordinate is N(-P_tu y / P_tt, 1 / P_tt)
    want_m, want_v = -P[-1, :-1] @ y / P[-1, -1], 1.0 / P[-1, -1]
    x = np.full(10, np.nan)
    x[u] = y
    res = GK.window_moments(msd, msd_inf, 0, 0.0, x, u, y, 0, 0, 10)
    assert abs(res['smooth_mean'][t] - want_m) < 1e-10 and abs(res['smooth_var'][t] - want_v) < 1e-10


def test_argument_errors_before_device_work(built_lib):
    """ refusals on the host or in the library's checks: none of these reaches a device (there may be none) """
    from bild_amd import _lib
    from gauss_sim_cases import make_model
    model = make_model(2, 2, 3, L=64)
    d = model.d
    x = np.zeros((30, d))
    st = np.zeros((1, 30), dtype=np.int64)
    with pytest.raises(ValueError, match='filt'):
        model.kalman(st, x, outputs=('smooth', 'filt'))
    with pytest.raises(ValueError, match='unknown output'):
        model.kalman(st, x, outputs='nope')
    with pytest.raises(ValueError, match='states out of range'):
        model.kalman(np.full((1, 30), 2), x)
    with pytest.raises(ValueError, match='segment starts'):
        model.kalman((np.array([[1, 3]]), np.array([[0, 1]])), [x])
    with pytest.raises(ValueError, match='at most'):
        model.kalman(np.zeros((1, 70), dtype=np.int64), np.zeros((70, d)))
    with pytest.raises(ValueError, match='finite or -inf'):
        model.kalman_mixture(np.zeros((2, 30), dtype=np.int64), x, [0.0, np.nan])
    with pytest.raises(ValueError, match='finite or -inf'):
        model.kalman_mixture(np.zeros((2, 30), dtype=np.int64), x, [np.inf, 0.0])
    with pytest.raises(ValueError, match='log-weights'):
        model.kalman_mixture(np.zeros((2, 30), dtype=np.int64), x, [0.0])
    # the library's own checks, reached through the raw wrappers
    h = model.handle()
    seg = (np.zeros((1, 1), dtype=np.int32), np.zeros((1, 1), dtype=np.int32))
    with pytest.raises(_lib.BildAmdError, match='filt'):
        _lib.gauss_kalman_segments(h, [x], *seg, outputs=('smooth_mean', 'filt_mean'))
    with pytest.raises(_lib.BildAmdError, match='MSD tables end'):
        _lib.gauss_kalman_segments(h, [np.zeros((70, d))], *seg)
    with pytest.raises(_lib.BildAmdError, match='state 5 out of range'):
        _lib.gauss_kalman_segments(h, [x], seg[0], np.full((1, 1), 5, dtype=np.int32))
    with pytest.raises(_lib.BildAmdError, match='first segment'):
        _lib.gauss_kalman_segments(h, [x], np.ones((1, 1), dtype=np.int32), seg[1])
    with pytest.raises(_lib.BildAmdError, match='traj_id'):
        _lib.gauss_kalman_segments(h, [x], *seg, traj_id=np.array([3], dtype=np.int32))
    with pytest.raises(_lib.BildAmdError, match='T_max'):
        _lib.gauss_kalman_segments(h, [x], *seg, T_max=20)
    with pytest.raises(_lib.BildAmdError, match='log-weights'):
        _lib.gauss_kalman_mixture(h, [x], *seg, np.array([np.nan]))
    with pytest.raises(_lib.BildAmdError, match='log-weights'):
        _lib.gauss_kalman_mixture(h, [x], *seg, np.array([np.inf]))
    with pytest.raises(_lib.BildAmdError, match='traj_id'):
        _lib.gauss_kalman_mixture(h, [x], *seg, np.zeros(1), traj_id=np.array([1], dtype=np.int32))
