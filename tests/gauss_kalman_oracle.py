"""
NumPy oracle of GenericGaussianModel's per-frame moments, on host arrays, by explicit Gaussian
conditioning: per interval and dimension the window of tests/gauss_oracle.py (its valid frames, data vector y read as
zero-mean with covariance C), and

* the predictive moments of each counted entry by conditioning on the entries before it (a prefix of the window);
* the moments of a missing frame by the Schur complement of the joint Gaussian of y and the missing coordinate (x_t - m,
  ss_order 0; the increment from the last valid frame before t minus its prior mean, ss_order 1);
* `window_cholesky`: the same from one Cholesky factor (u = L^-1 c_t, z = L^-1 y), the form the kernels compute.

The model is given as arrays like tests/gauss_oracle.py takes them: msd (S, d, L), msd_inf, mean, order (S, d).
"""
import numpy as np

from bild_amd.gauss import covariance

from gauss_oracle import LOG2PI, intervals

OUTPUTS = ('terms', 'pred_mean', 'pred_var', 'smooth_mean', 'smooth_var', 'innov')


def window(x, t0, t1, first, order, mean):
    """
    The window of interval [t0, t1) of one dimension x (T,): (times u, data y, first counted entry), or NaN for a later
    ss_order-0 window without a valid frame
    """
    a = 0 if first else t0 - 1
    u = np.nonzero(~np.isnan(x))[0]
    u = u[(u >= a) & (u < t1)]
    if order == 0:
        if not first and len(u) == 0:
            return np.nan
        y = x[u] - mean
        if not first and len(u):
            y[0] = x[u[0]]
        return u, y, 0 if first else 1
    return u, (np.diff(x[u]) - mean) if len(u) > 1 else np.zeros(0), 0


def _increment_cov(msd, a1, b1, a2, b2):
    """ covariance of the increments a1 -> b1 and a2 -> b2 by the increment rule """
    f = lambda p, q: msd[np.abs(np.asarray(p) - np.asarray(q))]
    return 0.5 * (f(b1, a2) + f(a1, b2) - f(b1, b2) - f(a1, a2))


def missing_prior(msd, msd_inf, order, mean, u, t):
    """
    For the missing frame t of a window with valid frames u: (c, var, ...) with c the covariance of the missing coordinate
    with y and var its prior variance; ss_order 0 adds the mean, ss_order 1 the last valid frame vb before t and the prior
    mean of the increment vb -> t.  None when there is no valid frame before t (ss_order 1).
    """
    if order == 0:
        return 0.5 * (msd_inf - msd[np.abs(t - u)]), 0.5 * (msd_inf - msd[0]), mean
    before = np.nonzero(u < t)[0]
    if len(before) == 0:
        return None
    j = before[-1]
    vb = u[j]
    c = _increment_cov(msd, u[:-1], u[1:], vb, t) if len(u) > 1 else np.zeros(0)
    prior = mean * (t - vb) / (u[j + 1] - vb) if j + 1 < len(u) else mean * (t - vb)
    return c, msd[t - vb], vb, prior


def _solve(C, b):
    return np.linalg.solve(C, b) if len(C) else np.zeros(0)


def window_moments(msd, msd_inf, order, mean, x, u, y, skip, t0, t1):
    """ per frame of [t0, t1): the outputs of one window by explicit conditioning -> dict of (t1 - t0,) arrays """
    C = covariance(msd, msd_inf, u, order) if len(y) else np.zeros((0, 0))
    out = {k: np.full(t1 - t0, np.nan) for k in OUTPUTS}
    out['terms'][:] = 0.0
    for j in range(skip, len(y)):
        t = u[j] if order == 0 else u[j + 1]
        Cp, c = C[:j, :j], C[j, :j]
        w = _solve(Cp, c)
        m = w @ y[:j]
        v = C[j, j] - c @ w
        shift = mean if order == 0 else x[u[j]] + mean
        out['pred_mean'][t - t0] = m + shift
        out['pred_var'][t - t0] = v
        out['innov'][t - t0] = (y[j] - m) / np.sqrt(v)
        out['terms'][t - t0] = -0.5 * ((y[j] - m) ** 2 / v + np.log(v) + LOG2PI)
    for t in range(t0, t1):
        if not np.isnan(x[t]):
            out['smooth_mean'][t - t0], out['smooth_var'][t - t0] = x[t], 0.0
            continue
        pr = missing_prior(msd, msd_inf, order, mean, u, t)
        if pr is None:
            continue
        c, var = pr[0], pr[1]
        w = _solve(C, c)
        mm, vv = w @ y, var - c @ w
        out['smooth_mean'][t - t0] = mm + mean if order == 0 else x[pr[2]] + (pr[3] + mm)
        out['smooth_var'][t - t0] = vv
    return out


def window_cholesky(msd, msd_inf, order, mean, x, u, y, skip, t0, t1):
    """ the same from one Cholesky factor: pred = y_j - L_jj z_j, var L_jj^2; a missing frame from u = L^-1 c_t """
    C = covariance(msd, msd_inf, u, order) if len(y) else np.zeros((0, 0))
    L = np.linalg.cholesky(C) if len(C) else np.zeros((0, 0))
    z = np.linalg.solve(L, y) if len(y) else np.zeros(0)
    out = {k: np.full(t1 - t0, np.nan) for k in OUTPUTS}
    out['terms'][:] = 0.0
    for j in range(skip, len(y)):
        t = u[j] if order == 0 else u[j + 1]
        ljj = L[j, j]
        shift = mean if order == 0 else x[u[j]] + mean
        out['pred_mean'][t - t0] = (y[j] - ljj * z[j]) + shift
        out['pred_var'][t - t0] = ljj * ljj
        out['innov'][t - t0] = z[j]
        out['terms'][t - t0] = -(np.log(ljj) + 0.5 * z[j] ** 2 + 0.5 * LOG2PI)
    for t in range(t0, t1):
        if not np.isnan(x[t]):
            out['smooth_mean'][t - t0], out['smooth_var'][t - t0] = x[t], 0.0
            continue
        pr = missing_prior(msd, msd_inf, order, mean, u, t)
        if pr is None:
            continue
        w = np.linalg.solve(L, pr[0]) if len(L) else np.zeros(0)
        mm, vv = w @ z, pr[1] - w @ w
        out['smooth_mean'][t - t0] = mm + mean if order == 0 else x[pr[2]] + (pr[3] + mm)
        out['smooth_var'][t - t0] = vv
    return out


def kalman(msd, msd_inf, mean, order, x, states, T_max=None, cholesky=False):
    """ the outputs of one candidate (expanded states) on x (T, d): dict of (T_max, d) arrays, NaN behind T """
    x = np.asarray(x, dtype=np.float64)
    T, d = x.shape
    T_max = T if T_max is None else T_max
    out = {k: np.full((T_max, d), np.nan) for k in OUTPUTS}
    fn = window_cholesky if cholesky else window_moments
    for i, (t0, t1, n) in enumerate(intervals(states)):
        for k in range(d):
            w = window(x[:, k], t0, t1, i == 0, order[n, k], mean[n, k])
            if not isinstance(w, tuple):
                continue        # NaN everywhere
            u, y, skip = w
            res = fn(msd[n, k], msd_inf[n, k], order[n, k], mean[n, k], x[:, k], u, y, skip, t0, t1)
            for name in OUTPUTS:
                out[name][t0:t1, k] = res[name]
    return out


def batch(msd, msd_inf, mean, order, trajs, states_list, traj_id=None, T_max=None, cholesky=False):
    """ many candidates: dict of (n, T_max, d) arrays """
    T_max = max(len(x) for x in trajs) if T_max is None else T_max
    tid = np.zeros(len(states_list), dtype=int) if traj_id is None else traj_id
    res = [kalman(msd, msd_inf, mean, order, trajs[j], s, T_max, cholesky) for s, j in zip(states_list, tid)]
    return {k: np.stack([r[k] for r in res]) for k in OUTPUTS}


# ---------------------------------------------------------------------------------------------------- test cases
def cases(seed):
    """
    (model, x, states list) covering the corners of the definitions: S = 3 with both orders across dimensions, means
    != 0, a later ss_order-0 interval whose conditioning frame is missing, leading, inner and trailing gaps, a window
    without a valid frame (NaN), adjacent switches, T = 1
    """
    from gauss_sim_cases import make_model, profile
    rng = np.random.default_rng(seed)
    model = make_model(3, 3, seed, L=64)
    out = []
    for T in (40, 23):
        x = rng.normal(size=(T, 3)) * 0.7 + 0.3
        x[:3, 0] = np.nan                   # leading gap
        x[10:13, 1] = np.nan                # inner gap
        x[-4:, 2] = np.nan                  # trailing gap
        x[rng.random((T, 3)) < 0.15] = np.nan
        x[15:20, :] = np.nan                # an interval [16, 20) without a valid frame (its conditioning frame missing)
        states = [profile(rng, T, 3, sw) for sw in (0, 1, 3, 6) for _ in range(3)]
        st = np.zeros(T, dtype=int)
        st[16:20] = 1                       # window 15..19 all missing: NaN for its ss_order-0 dimensions
        st[20:] = 2
        states.append(st)
        st = np.zeros(T, dtype=int)
        st[5], st[6], st[7:] = 1, 2, 0       # adjacent switches; the interval at 16 conditions on missing frame 15
        st[16:] = 1
        states.append(st)
        out.append((x, states))
    x1 = np.array([[0.2, np.nan, -0.4]])
    out.append((x1, [np.array([s]) for s in range(3)]))
    return model, out
