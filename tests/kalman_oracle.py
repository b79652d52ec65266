"""
Dense NumPy Kalman filter and CLASSICAL Rauch-Tung-Striebel smoother over the full model arrays (B, G, Sig, M0, C0, w):
the checker of MultiStateRouse.kalman.  The device runs the modified Bryson-Frazier form in the modal basis; this is
deliberately the other formulation (gain J = P_{t|t} B^T P_{t+1|t}^{-1} through `solve`).

Conventions of the reference filter (bild/src/MSRouse_logL_py.py): frame 0 starts from the steady state of states[0]
with no predict, frame t >= 1 is predicted with the propagator of states[t], a frame with any NaN coordinate is
predicted but not updated.  One covariance per dimension (equal localization errors give equal covariances).
"""
import numpy as np

LOG_2PI = np.log(2 * np.pi)
OUTPUTS = ('terms', 'pred_mean', 'pred_var', 'filt_mean', 'filt_var', 'smooth_mean', 'smooth_var', 'innov')


def filter_smoother(arrays, w, loc_err, x, states):
    """ one candidate: every output of the device entry, each (T, d) """
    B, G, Sig, M0, C0 = (np.asarray(arrays[k], dtype=np.float64) for k in ('B', 'G', 'Sig', 'M0', 'C0'))
    w = np.asarray(w, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    states = np.asarray(states)
    T, d = x.shape
    N = len(w)
    out = {k: np.zeros((T, d)) for k in OUTPUTS}
    observed = ~np.any(np.isnan(x), axis=1)
    for k in range(d):
        s2 = float(loc_err[k]) ** 2
        mp, Pp = np.zeros((T, N)), np.zeros((T, N, N))
        mf, Pf = np.zeros((T, N)), np.zeros((T, N, N))
        for t in range(T):
            s = states[t]
            if t == 0:
                m, P = M0[s][:, k].copy(), C0[s].copy()
            else:
                m = B[s] @ mf[t - 1] + G[s][:, k]
                P = B[s] @ Pf[t - 1] @ B[s].T + Sig[s]
            mp[t], Pp[t] = m, P
            Pw = P @ w
            S = w @ Pw + s2
            out['pred_mean'][t, k] = w @ m
            out['pred_var'][t, k] = S
            if observed[t]:
                e = x[t, k] - w @ m
                K = Pw / S
                m = m + K * e
                P = P - np.outer(K, Pw)
                out['terms'][t, k] = -0.5 * (e * e / S + np.log(S) + LOG_2PI)
                out['innov'][t, k] = e / np.sqrt(S)
            else:
                out['innov'][t, k] = np.nan
            mf[t], Pf[t] = m, P
            out['filt_mean'][t, k] = w @ m
            out['filt_var'][t, k] = w @ P @ w
        ms, Ps = mf[T - 1].copy(), Pf[T - 1].copy()
        out['smooth_mean'][T - 1, k] = w @ ms
        out['smooth_var'][T - 1, k] = w @ Ps @ w
        for t in range(T - 2, -1, -1):
            Bn = B[states[t + 1]]
            # J = Pf_t Bn^T Pp_{t+1}^{-1}  (Pp symmetric: J^T = solve(Pp, Bn Pf_t))
            J = np.linalg.solve(Pp[t + 1], Bn @ Pf[t]).T
            ms = mf[t] + J @ (ms - mp[t + 1])
            Ps = Pf[t] + J @ (Ps - Pp[t + 1]) @ J.T
            out['smooth_mean'][t, k] = w @ ms
            out['smooth_var'][t, k] = w @ Ps @ w
    return out


def batch(arrays, w, loc_err, trajs, states_list, traj_id=None, T_max=None):
    """ many candidates: dict of (n, T_max, d) arrays, NaN behind each trajectory's length """
    trajs = [np.asarray(t, dtype=np.float64) for t in trajs]
    n = len(states_list)
    tid = np.zeros(n, dtype=int) if traj_id is None else np.asarray(traj_id)
    T_max = max(len(t) for t in trajs) if T_max is None else T_max
    d = trajs[0].shape[1]
    res = {k: np.full((n, T_max, d), np.nan) for k in OUTPUTS}
    for r in range(n):
        x = trajs[tid[r]]
        o = filter_smoother(arrays, w, loc_err, x, np.asarray(states_list[r])[:len(x)])
        for k in OUTPUTS:
            res[k][r, :len(x)] = o[k]
    return res


def mixture(means, variances, log_weights):
    """ law of total variance over candidates (axis 0) with weights exp(log_weights), normalised """
    lw = np.asarray(log_weights, dtype=np.float64)
    w = np.exp(lw - np.max(lw))
    w = w / w.sum()
    mean = np.tensordot(w, means, axes=1)
    var = np.tensordot(w, variances, axes=1) + np.tensordot(w, (means - mean) ** 2, axes=1)
    return mean, var
