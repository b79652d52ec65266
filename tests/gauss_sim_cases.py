"""
Shared by tests/test_gauss_simulate.py (CPU) and tests/test_gpu_gauss_simulate.py: GenericGaussianModels with well
conditioned MSDs, random profiles, and the generator's algebra restated in NumPy -- one Toeplitz
Cholesky factor per (state, dimension), fed with the loop's normals scattered to their (frame, dimension).
"""
import numpy as np

import bild_amd
from bild_amd import gauss


def msd_exp(A, tau, sig, L):
    """ ss_order 0: 2A (1 - exp(-t/tau)) + 2 sig^2 at t >= 1, 0 at t = 0; msd(inf) last """
    t = np.arange(L, dtype=np.float64)
    m = 2 * A * (1 - np.exp(-t / tau)) + 2 * sig ** 2
    m[0] = 0.0
    return np.append(m, 2 * A + 2 * sig ** 2)


def msd_pow(G, alpha, sig, L):
    """ ss_order 1: G t^alpha + 2 sig^2 at t >= 1, 0 at t = 0 """
    t = np.arange(L, dtype=np.float64)
    m = G * t ** alpha + 2 * sig ** 2
    m[0] = 0.0
    return m


def make_model(S, d, seed, L=2048, means=True, zero_order0_means=False):
    """ mixed ss_order per state and dimension (both orders occur whenever S d >= 2), well conditioned """
    rng = np.random.default_rng(seed)
    spec = []
    for n in range(S):
        row = []
        for k in range(d):
            o = (n + k + seed) % 2
            if o == 0:
                msd = msd_exp(rng.uniform(0.5, 2.0), rng.uniform(2.0, 30.0), rng.uniform(0.2, 0.5), L)
            else:
                msd = msd_pow(rng.uniform(0.2, 1.0), rng.uniform(0.5, 1.5), rng.uniform(0.2, 0.5), L)
            m = rng.uniform(-0.5, 0.5) if means else 0.0
            if o == 0 and zero_order0_means:
                m = 0.0
            row.append((msd, m, o))
        spec.append(row)
    return bild_amd.GenericGaussianModel(spec)


def profile(rng, T, S, switches):
    st = np.full(T, rng.integers(S))
    if T > 1 and switches:
        for t in np.sort(rng.choice(np.arange(1, T), size=min(switches, T - 1), replace=False)):
            st[t:] = (st[t - 1] + 1 + rng.integers(S - 1)) % S
    return st


def intervals(states):
    """ runs of equal state as (t0, t1, state) """
    states = np.asarray(states)
    cut = np.flatnonzero(states[1:] != states[:-1]) + 1
    lo = np.concatenate([[0], cut])
    hi = np.concatenate([cut, [len(states)]])
    return [(int(a), int(b), int(states[a])) for a, b in zip(lo, hi)]


def factors(model, T):
    """ per (state, dimension): the lower Cholesky factor of the Toeplitz covariance of the longest window """
    S, d = model.ss_order.shape
    out = {}
    for n in range(S):
        for k in range(d):
            o = int(model.ss_order[n, k])
            C = gauss.covariance(model.msd[n, k], model.msd_inf[n, k], np.arange(T), o)
            out[n, k] = np.linalg.cholesky(C) if len(C) else np.zeros((0, 0))
    return out


def scatter_normals(model, states, z):
    """
    The loop's normals of one trajectory (interval-major, then dimension) -> (T, d): entry j of a first ss_order-1
    interval belongs to frame j + 1, every other entry j of an interval [t0, t1) to frame t0 + j; NaN where none
    """
    T, d = len(states), model.d
    Z = np.full((T, d), np.nan)
    zo = 0
    for t0, t1, n in intervals(states):
        for k in range(d):
            f0 = int(model.ss_order[n, k]) if t0 == 0 else t0
            Z[f0:t1, k] = z[zo:zo + t1 - f0]
            zo += t1 - f0
    assert zo == len(z)
    return Z


def restate(model, states, z, L=None):
    """ the generator's algebra for one trajectory (no missing frames applied) """
    T, d = len(states), model.d
    L = factors(model, T) if L is None else L
    Z = scatter_normals(model, states, z)
    x = np.empty((T, d))
    for t0, t1, n in intervals(states):
        for k in range(d):
            m, o, F = model.mean[n, k], int(model.ss_order[n, k]), L[n, k]
            nn = t1 - t0
            if t0 == 0 and o == 0:
                x[:t1, k] = F[:t1, :t1] @ Z[:t1, k] + m
            elif t0 == 0:
                x[0, k] = 0.0
                x[1:t1, k] = np.cumsum(F[:t1 - 1, :t1 - 1] @ Z[1:t1, k] + m)
            elif o == 0:
                a = (x[t0 - 1, k] - m) / F[0, 0]
                x[t0:t1, k] = m + (F[:nn + 1, :nn + 1] @ np.concatenate([[a], Z[t0:t1, k]]))[1:]
            else:
                x[t0:t1, k] = x[t0 - 1, k] + np.cumsum(F[:nn, :nn] @ Z[t0:t1, k] + m)
    return x


def compare(got, want, tol):
    """ NaN masks equal, values within tol x max |value| of each trajectory; -> worst relative deviation """
    assert len(got) == len(want)
    worst = 0.0
    for g, w in zip(got, want):
        assert g[:].shape == w[:].shape
        assert np.array_equal(np.isnan(g[:]), np.isnan(w[:]))
        ok = ~np.isnan(w[:])
        if ok.any():
            scale = np.max(np.abs(w[:][ok]))
            dev = np.max(np.abs(g[:][ok] - w[:][ok]))
            assert dev <= tol * scale, (dev, scale)
            worst = max(worst, dev / scale) if scale > 0 else worst
        assert g.meta['loopingprofile'] is w.meta['loopingprofile']
    return worst
