"""
NumPy oracle of GenericGaussianModel's log-likelihood sensitivities, on host arrays: per interval
and dimension the window of the decomposition in tests/gauss_oracle.py, its dense Cholesky factor and the factor's
tangents dL = L Phi(L^-1 dC L^-T) (Phi: the lower triangle with the diagonal halved), then per counted entry
tau_j = log L_jj + z_j^2 / 2 + log(2 pi) / 2, dtau_j = dL_jj / L_jj + z_j dz_j, and the innovations Fisher
dS_p dS_q / (2 S^2) + de_p de_q / S with S = L_jj^2, e = L_jj z_j.

The model is given as arrays like tests/gauss_oracle.py takes them: msd (S, d, L), msd_inf, mean, order (S, d); the
derivatives as dmsd (P, S, d, L), dmsd_inf and dmean (P, S, d).
"""
import numpy as np

from bild_amd.gauss import covariance

from gauss_oracle import LOG2PI, intervals


def window(x, a, b, first, order, mean):
    """
    The vector of the window [a, b) of one dimension x (T,): (times u, data y, counted entries from `skip`, raw: whether
    entry 0 is the raw conditioning value), or None when it has no counted entry; NaN for a later ss_order-0 window
    without a valid frame.
    """
    u = np.nonzero(~np.isnan(x))[0]
    u = u[(u >= a) & (u < b)]
    if order == 0:
        if not first and len(u) == 0:
            return np.nan
        skip = 0 if first else 1
        if len(u) <= skip:
            return None
        y = x[u] - mean
        if not first:
            y[0] = x[u[0]]
        return u, y, skip, not first
    if len(u) < 2:
        return None
    return u, np.diff(x[u]) - mean, 0, False


def tangent_factor(C, dC):
    """ L = chol(C) and dL_p = L Phi(L^-1 dC_p L^-T) """
    L = np.linalg.cholesky(C)
    Li = np.linalg.inv(L)
    dL = []
    for D in dC:
        X = Li @ D @ Li.T
        Phi = np.tril(X, -1) + 0.5 * np.diag(np.diag(X))
        dL.append(L @ Phi)
    return L, dL


def window_terms(msd, msd_inf, order, u, y, skip, raw, dmsd, dmsd_inf, dmean):
    """ (sum tau, sum dtau (P,), Fisher (P, P)) of one window; dmsd (P, L), dmsd_inf, dmean (P,) """
    P = len(dmsd)
    C = covariance(msd, msd_inf, u, order)
    dC = [covariance(dmsd[p], dmsd_inf[p], u, order) for p in range(P)]
    L, dL = tangent_factor(C, dC)
    z = np.linalg.solve(L, y)
    d = np.diag(L)
    tau = np.log(d) + 0.5 * z ** 2 + 0.5 * LOG2PI
    dtau = np.zeros((P, len(y)))
    de = np.zeros((P, len(y)))
    dS = np.zeros((P, len(y)))
    for p in range(P):
        dy = np.full(len(y), -dmean[p])
        if raw:
            dy[0] = 0.0
        dz = np.linalg.solve(L, dy - dL[p] @ z)
        dd = np.diag(dL[p])
        dtau[p] = dd / d + z * dz
        dS[p] = 2 * d * dd
        de[p] = dd * z + d * dz
    S = d ** 2
    m = slice(skip, None)
    F = (dS[:, m] / S[m]) @ (dS[:, m] / S[m]).T / 2 + (de[:, m] / np.sqrt(S[m])) @ (de[:, m] / np.sqrt(S[m])).T
    return tau[m].sum(), dtau[:, m].sum(axis=1), F


def sensitivities(msd, msd_inf, mean, order, x, states, dmsd=None, dmsd_inf=None, dmean=None):
    """ (logL, grad (P,), fisher (P, P)) of one expanded profile on one trajectory x (T, d); NaN where the reference raises """
    S, d = order.shape
    P = 0 if dmsd is None else len(dmsd)
    dmsd = np.zeros((P,) + msd.shape) if dmsd is None else dmsd
    dmsd_inf = np.zeros((P, S, d)) if dmsd_inf is None else dmsd_inf
    dmean = np.zeros((P, S, d)) if dmean is None else dmean
    x = np.asarray(x, dtype=np.float64)
    ll, g, F = 0.0, np.zeros(P), np.zeros((P, P))
    for i, (t0, t1, n) in enumerate(intervals(states)):
        a = 0 if i == 0 else t0 - 1
        for k in range(d):
            w = window(x[:, k], a, t1, i == 0, order[n, k], mean[n, k])
            if w is None:
                continue
            if not isinstance(w, tuple):
                return np.nan, np.full(P, np.nan), np.full((P, P), np.nan)
            t, dt, f = window_terms(msd[n, k], msd_inf[n, k], order[n, k], *w, dmsd[:, n, k], dmsd_inf[:, n, k], dmean[:, n, k])
            ll -= t
            g -= dt
            F += f
    return ll, g, F


def batch(msd, msd_inf, mean, order, trajs, profiles, traj_id=None, **derivs):
    """ many profiles: lists of trajectories and of expanded profiles (traj_id: per profile) -> (n,), (n, P), (n, P, P) """
    out = [sensitivities(msd, msd_inf, mean, order, trajs[0 if traj_id is None else traj_id[r]], p, **derivs)
           for r, p in enumerate(profiles)]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out])
