"""
Kalman filter and smoother of MultiStateRouse profiles, without a GPU: the NumPy oracle (tests/kalman_oracle.py) against
the reference's log-likelihoods and against the conditionals of the joint Gaussian of a whole trajectory, the MBF
recursion the device runs against the oracle's classical RTS smoother, and the argument and envelope checks of
MultiStateRouse.kalman, which all happen before any trajectory set (and so any device work) exists.
"""
import numpy as np
import pytest

import goldens
import kalman_oracle as KO

import bild_amd
from bild_amd import _lib


@pytest.mark.parametrize('name', goldens.names())
def test_oracle_terms_sum_to_reference_logL(name):
    g = goldens.load(name)
    for r, states in enumerate(g['states']):
        out = KO.filter_smoother(g['arrays'], g['w'], g['localization_error'], g['x'], states)
        total = out['terms'].sum()
        assert abs(total - g['logL_ref_numpy'][r]) < 1e-8
        if np.isfinite(g['logL_ref_cython'][r]):
            assert abs(total - g['logL_ref_cython'][r]) < 1e-8


def _tiny_case(seed, T=12, N=6):
    rng = np.random.default_rng(seed)
    model = bild_amd.MultiStateRouse(N, 1.0, 2.0, d=2, localization_error=[0.3, 0.5])
    a = model.arrays()
    states = np.zeros(T, dtype=int)
    states[T // 2:] = 1                       # one switch
    x = rng.normal(size=(T, 2)) * 2.0
    x[[2, 3, 7]] = np.nan                     # missing frames, one gap of two
    return a, model.measurement, np.array([0.3, 0.5]), x, states


def _joint(a, w, s2, k, states):
    """ mean and covariance of the full states x_0..x_{T-1} (dimension k), and the observation map """
    B, G, Sig, M0, C0 = (a[n] for n in ('B', 'G', 'Sig', 'M0', 'C0'))
    T, N = len(states), len(w)
    mu = np.zeros((T, N))
    cov = np.zeros((T, N, T, N))
    for t in range(T):
        s = states[t]
        if t == 0:
            mu[0], cov[0, :, 0, :] = M0[s][:, k], C0[s]
            continue
        mu[t] = B[s] @ mu[t - 1] + G[s][:, k]
        for u in range(t):
            cov[t, :, u, :] = B[s] @ cov[t - 1, :, u, :]
            cov[u, :, t, :] = cov[t, :, u, :].T
        cov[t, :, t, :] = B[s] @ cov[t - 1, :, t - 1, :] @ B[s].T + Sig[s]
    Wm = np.kron(np.eye(T), w[None, :])             # y = Wm X
    my = Wm @ mu.reshape(-1)
    cy = Wm @ cov.reshape(T * N, T * N) @ Wm.T
    return my, cy


def _conditional(my, cy, s2, x, t, cond, noise):
    """ moments of y_t (+ noise s2 when `noise`) given the observations z_u, u in cond """
    cond = np.asarray(cond, dtype=int)
    m, v = my[t], cy[t, t] + (s2 if noise else 0.0)
    if len(cond):
        czz = cy[np.ix_(cond, cond)] + s2 * np.eye(len(cond))
        cyz = cy[t, cond]
        sol = np.linalg.solve(czz, x[cond] - my[cond])
        m = m + cyz @ sol
        v = v - cyz @ np.linalg.solve(czz, cyz)
    return m, v


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_oracle_moments_are_the_joint_gaussian_conditionals(seed):
    a, w, err, x, states = _tiny_case(seed)
    out = KO.filter_smoother(a, w, err, x, states)
    T = len(x)
    obs = np.flatnonzero(~np.any(np.isnan(x), axis=1))
    for k in range(x.shape[1]):
        s2 = err[k] ** 2
        my, cy = _joint(a, w, s2, k, states)
        xk = np.where(np.isnan(x[:, k]), 0.0, x[:, k])
        scale_m, scale_v = 1.0 + np.max(np.abs(xk)), np.max(np.diag(cy)) + s2
        for t in range(T):
            for key, cond, noise in (('pred', obs[obs < t], True), ('filt', obs[obs <= t], False), ('smooth', obs, False)):
                m, v = _conditional(my, cy, s2, xk, t, cond, noise)
                assert abs(out[key + '_mean'][t, k] - m) < 1e-10 * scale_m, (key, t, k)
                assert abs(out[key + '_var'][t, k] - v) < 1e-10 * scale_v, (key, t, k)


def _mbf(a, w, err, x, states):
    """ the recursion of csrc/kalman.hip, restated densely: smoothed y-moments from filtered ones, nothing inverted """
    B = a['B']
    T, d = x.shape
    N = len(w)
    fo = KO.filter_smoother(a, w, err, x, states)
    mean, var = np.zeros((T, d)), np.zeros((T, d))
    obs = ~np.any(np.isnan(x), axis=1)
    for k in range(d):
        s2 = err[k] ** 2
        # forward quantities: predicted c = C- w, S, e, filtered y-mean, u = P w
        Cs, Ss, es, fm, us = [], [], [], [], []
        Gk, M0, C0, Sig = a['G'][:, :, k], a['M0'][:, :, k], a['C0'], a['Sig']
        for t in range(T):
            s = states[t]
            if t == 0:
                m, P = M0[s].copy(), C0[s].copy()
            else:
                m, P = B[s] @ m + Gk[s], B[s] @ P @ B[s].T + Sig[s]
            c = P @ w
            S = w @ c + s2
            e = x[t, k] - w @ m if obs[t] else 0.0
            if obs[t]:
                K = c / S
                m, P = m + K * e, P - np.outer(K, c)
            Cs.append(c), Ss.append(S), es.append(e), fm.append(w @ m), us.append(c * s2 / S if obs[t] else c)
        lam, Lam = np.zeros(N), np.zeros((N, N))
        for t in range(T - 1, -1, -1):
            u = us[t]
            mean[t, k] = fm[t] + u @ lam
            var[t, k] = w @ u - u @ Lam @ u
            if t == 0:
                break
            if obs[t]:
                K = Cs[t] / Ss[t]
                A = np.eye(N) - np.outer(K, w)
                lam = w * es[t] / Ss[t] + A.T @ lam
                Lam = np.outer(w, w) / Ss[t] + A.T @ Lam @ A
            Bt = B[states[t]]
            lam, Lam = Bt.T @ lam, Bt.T @ Lam @ Bt
    return mean, var, fo


@pytest.mark.parametrize('seed', [0, 1, 2, 3])
def test_mbf_restatement_equals_classical_rts(seed):
    a, w, err, x, states = _tiny_case(seed, T=12, N=6)
    if seed == 3:
        x[8:] = np.nan                        # missing to the end
    mean, var, fo = _mbf(a, w, err, x, states)
    scale = 1.0 + np.nanmax(np.abs(x))
    assert np.max(np.abs(mean - fo['smooth_mean'])) < 1e-10 * scale
    assert np.max(np.abs(var - fo['smooth_var'])) < 1e-10 * np.max(fo['pred_var'])


def test_mbf_restatement_on_a_golden():
    g = goldens.load('s2_dstar2_missing_T150')
    mean, var, fo = _mbf(g['arrays'], g['w'], g['localization_error'], g['x'], g['states'][1])
    assert np.max(np.abs(mean - fo['smooth_mean'])) < 1e-9 * np.nanmax(np.abs(g['x']))
    assert np.max(np.abs(var - fo['smooth_var'])) < 1e-9 * np.max(fo['pred_var'])


# ---- argument and envelope checks (no trajectory set is created, so no GPU is needed) ----

def _model():
    return bild_amd.MultiStateRouse(10, 1.0, 5.0, d=3, localization_error=0.1)


def test_refuses_a_model_without_modal_path():
    a = _model().arrays()
    B = a['B'].copy()
    B[0, 0, 1] += 0.05                        # not symmetric
    m = bild_amd.MultiStateRouse.from_arrays(B, a['G'], a['Sig'], a['M0'], a['C0'], _model().measurement, 0.1)
    x = np.zeros((20, 3))
    with pytest.raises(_lib.BildAmdError) as ei:
        m.kalman(np.zeros((1, 20), dtype=int), x)
    assert ei.value.code == _lib.ERR_UNSUPPORTED and 'modal' in str(ei.value)
    assert len(m._trajsets) == 0


def test_refuses_more_than_32_modes():
    m = bild_amd.MultiStateRouse(80, 1.0, 5.0, d=3, localization_error=0.1)
    assert m.handle().query(_lib.Q_NEFF) == 40
    with pytest.raises(_lib.BildAmdError) as ei:
        m.kalman(np.zeros((1, 20), dtype=int), np.zeros((20, 3)))
    assert ei.value.code == _lib.ERR_UNSUPPORTED and '32' in str(ei.value)
    assert len(m._trajsets) == 0


def test_argument_errors():
    m = _model()
    x = np.zeros((20, 3))
    with pytest.raises(ValueError):
        m.kalman(np.zeros((2, 19), dtype=int), x)                       # wrong profile length
    seg = (np.zeros((2, 1), dtype=np.int32), np.zeros((2, 1), dtype=np.int32))
    with pytest.raises(ValueError):
        m.kalman(seg, [x, x], traj_id=[0, 2])                           # traj_id out of range
    with pytest.raises(ValueError):
        m.kalman(seg, [x, x], traj_id=[0])                              # traj_id length
    with pytest.raises(ValueError):
        m.kalman(np.zeros((1, 20), dtype=int), x, outputs=('smooth', 'posterior'))  # unknown output
    with pytest.raises(ValueError):
        m.kalman(np.full((1, 20), 2), x)                                # state out of range
    with pytest.raises(ValueError):
        m.kalman_mixture(seg, [x], [0.0, np.nan])                       # NaN log-weight
    with pytest.raises(ValueError):
        m.kalman_mixture(seg, [x], [0.0, np.inf])                       # +inf log-weight
    assert len(m._trajsets) == 0


def test_posterior_distance_needs_a_rouse_model():
    from bild_amd.amis import FixedkSampler

    class OtherModel:
        pass
    s = FixedkSampler.__new__(FixedkSampler)
    s.model = OtherModel()
    with pytest.raises(TypeError, match='OtherModel'):
        s.posterior_distance()
