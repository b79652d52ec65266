"""
NumPy oracle of GenericGaussianModel's likelihood (reference bild/models.py:608-663), on host arrays.

* `logl_reference`: the reference loop restated: per interval and dimension a dense covariance, the reference's
  conditioning on the first valid value of the window (taken raw), slogdet and solve.
* `tables` / `logl_tables`: the decomposition the GPU build computes ("GenericGaussianModel"): per state the
  term W[a][b] of every window [a, b) and F[b] of every first interval, summed over the dimensions, from one Cholesky
  factor per window start; a profile is then F[n0][t1_0] + sum of W[n_i][t0_i - 1][t1_i].

The model is given as arrays: msd (S, d, L) at integer lags, msd_inf (S, d), mean (S, d), order (S, d).
"""
import numpy as np

from bild_amd.gauss import covariance

LOG2PI = np.log(2 * np.pi)


def intervals(states):
    """ runs of equal state of an expanded profile, (t0, t1, state), the last one ending at T """
    states = np.asarray(states)
    cuts = list(np.nonzero(np.diff(states))[0] + 1)
    edges = [0] + cuts + [len(states)]
    return [(edges[i], edges[i + 1], int(states[edges[i]])) for i in range(len(edges) - 1)]


def logl_reference(msd, msd_inf, mean, order, x, states):
    """ the reference's loop; NaN where it would raise IndexError (ss_order 0, later interval, no valid frame) """
    x = np.asarray(x, dtype=np.float64)
    total = 0.0
    for i, (t0, t1, n) in enumerate(intervals(states)):
        t_start = 0 if i == 0 else t0 - 1
        for k in range(x.shape[1]):
            trace = x[t_start:t1, k]
            ti = np.nonzero(~np.isnan(trace))[0]
            trace = trace[ti]
            m, o = mean[n, k], order[n, k]
            if o == 0:
                if i > 0 and len(ti) == 0:
                    return np.nan
                C = covariance(msd[n, k], msd_inf[n, k], ti, 0)
                v = trace - m
                if i > 0:
                    mu = trace[0] * C[1:, 0] / C[0, 0]
                    v = v[1:] - mu
                    C = (C - C[:, [0]] * C[[0], :] / C[0, 0])[1:, 1:]
            else:
                if len(ti) < 2:
                    continue
                C = covariance(msd[n, k], msd_inf[n, k], ti, 1)
                v = np.diff(trace) - m
            if len(C) == 0:
                continue
            _, logdet = np.linalg.slogdet(C)
            total += -0.5 * (v @ np.linalg.solve(C, v) + logdet + len(C) * LOG2PI)
    return total


def _tau(C, y):
    L = np.linalg.cholesky(C)
    z = np.linalg.solve(L, y)   # triangular, dense solve is exact enough here
    return np.log(np.diag(L)) + 0.5 * z ** 2 + 0.5 * LOG2PI


def tables(msd, msd_inf, mean, order, x):
    """ W (S, T, T + 1) with W[n, a, b] for a < b (NaN elsewhere), F (S, T + 1) """
    x = np.asarray(x, dtype=np.float64)
    T, d = x.shape
    S = msd.shape[0]
    W = np.zeros((S, T, T + 1))
    F = np.zeros((S, T + 1))
    for n in range(S):
        for k in range(d):
            valid = np.nonzero(~np.isnan(x[:, k]))[0]
            m, o = mean[n, k], order[n, k]
            for a in range(T + 1):          # a == T: the first interval
                first = a == T
                u = valid[valid >= (0 if first else a)]
                if o == 0:
                    y = x[u, k] - m
                    if not first and len(u):
                        y[0] = x[u[0], k]
                    tau = _tau(covariance(msd[n, k], msd_inf[n, k], u, 0), y) if len(u) else np.zeros(0)
                    ends = u                  # entry j lies in the window once u_j < b
                    skip = 0 if first else 1
                else:
                    y = np.diff(x[u, k]) - m
                    tau = _tau(covariance(msd[n, k], msd_inf[n, k], u, 1), y) if len(u) > 1 else np.zeros(0)
                    ends = u[1:]
                    skip = 0
                lo = 0 if first else a
                b = np.arange(lo + 1, T + 1)
                part = np.concatenate(([0.0], np.cumsum(np.where(np.arange(len(tau)) >= skip, tau, 0.0))))
                val = -part[np.searchsorted(ends, b, side='left')]    # entries with ends < b
                if o == 0 and not first:
                    val = np.where(np.searchsorted(u, b, side='left') == 0, np.nan, val)
                if first:
                    F[n, b] += val
                else:
                    W[n, a, b] += val
    return W, F


def logl_tables(W, F, states):
    total = 0.0
    for i, (t0, t1, n) in enumerate(intervals(states)):
        total += F[n, t1] if i == 0 else W[n, t0 - 1, t1]
    return total
