"""
The switch tail (csrc/tail.hip "switch tails") as mathematics, on the CPU: the backward recursion of the
first-order tail taken along a path WITH one switch -- state s up to frame t2 - 1, state s' from t2 on -- against finite differences
of a plain NumPy Kalman filter whose state varies in time; and the construction the device uses for it (terminal value: the
switch-free tail of s' where the transient behind the switch has converged, then back through the transient and across the switch)
against the recursion run over the whole path.  Full coordinates: the basis change R of the modal path is the identity here.
"""
import numpy as np
import pytest

import bild_amd


def _path_tail(Bs, Sigs, w, s2, x, prof, C, M, t0):
    """ sum of the log-likelihoods of frames t0 .. T-1 of a filter in state prof[t] at frame t whose state AFTER frame t0 - 1 is
        (C, M); NaN rows of x are missing frames """
    L = 0.0
    C, M = C.copy(), M.copy()
    for t in range(t0, len(x)):
        B, Sig = Bs[prof[t]], Sigs[prof[t]]
        C = B @ C @ B.T + Sig
        M = B @ M
        if np.isnan(x[t, 0]):
            continue
        S = s2 + w @ C @ w
        K = C @ w / S
        e = x[t] - w @ M
        L += -0.5 * np.sum(np.log(2 * np.pi * S) + e * e / S)
        M = M + np.outer(K, e)
        C = C - np.outer(K, w @ C)
    return L


def _forward(Bs, Sigs, w, s2, x, prof, C, M, t0, t1):
    """ frames t0 .. t1 - 1 from the state (C, M) after frame t0 - 1: the states after every frame and (S, K, e) or None per frame """
    states, per_frame = {t0 - 1: (C.copy(), M.copy())}, {}
    C, M = C.copy(), M.copy()
    for t in range(t0, t1):
        B, Sig = Bs[prof[t]], Sigs[prof[t]]
        C = B @ C @ B.T + Sig
        M = B @ M
        if np.isnan(x[t, 0]):
            per_frame[t] = None
        else:
            S = s2 + w @ C @ w
            K = C @ w / S
            e = x[t] - w @ M
            per_frame[t] = (S, K, e)
            M = M + np.outer(K, e)
            C = C - np.outer(K, w @ C)
        states[t] = (C.copy(), M.copy())
    return states, per_frame


def _step_back(B, w, frame, g):
    """ g_{t-1} = B_t^T [ (e_t / S_t) w + (I - w K_t^T) g_t ]      (missing frame: B_t^T g_t) """
    if frame is None:
        return B.T @ g
    S, K, e = frame
    return B.T @ (np.outer(w, e / S) + g - np.outer(w, K @ g))


@pytest.mark.parametrize('N,T,t2,missing', [(8, 60, 30, ()), (12, 80, 40, (38, 39, 41, 44, 45, 60))])
def test_switch_tail_vectors_against_finite_differences(N, T, t2, missing):
    rng = np.random.default_rng(N + T)
    model = bild_amd.MultiStateRouse(N, 1., 5., d=3, localization_error=0.1)
    A = model.arrays()
    Bs, Sigs = A['B'], A['Sig']
    w = np.asarray(model.measurement, dtype=float)
    s2 = 0.1 ** 2
    s, sn = 1, 0
    prof = np.where(np.arange(T) < t2, s, sn)
    x = np.array(model.trajectory_from_loopingprofile(bild_amd.Loopingprofile(prof.astype(int)), rng=rng)[:], dtype=float)
    x[list(missing)] = np.nan
    # the path's own filter from the steady state of s, and the recursion over the whole path
    st, fr = _forward(Bs, Sigs, w, s2, x, prof, A['C0'][s], A['M0'][s], 1, T)
    g = {T - 1: np.zeros((N, 3))}
    for t in range(T - 1, 0, -1):
        g[t - 1] = _step_back(Bs[prof[t]], w, fr[t], g[t])
    # looks at frames t2 - j: in front of the switch (j = 0), behind missing frames, far in front
    for j in (0, 1, 3, 12, 25):
        t0 = t2 - j
        C, M = st[t0 - 1]
        base = _path_tail(Bs, Sigs, w, s2, x, prof, C, M, t0)
        dM = rng.standard_normal(M.shape)
        errs = []
        for eps in (1e-3, 1e-4):
            got = _path_tail(Bs, Sigs, w, s2, x, prof, C, M + eps * dM, t0) - base
            errs.append(abs(got - eps * np.sum(g[t0 - 1] * dM)))
        # second order: the error falls by 100 when the deviation falls by 10
        assert errs[0] < 1e-4 * max(1.0, abs(base)) and errs[1] < 0.02 * errs[0] + 1e-12, (j, errs)
    # the device's construction: the switch-free filter of sn from ITS steady state gives the terminal value where the transient
    # has converged onto it (m frames behind the switch); back through the transient's own frames, then along the filter of s
    free = np.full(T, sn)
    _, fr_free = _forward(Bs, Sigs, w, s2, x, free, A['C0'][sn], A['M0'][sn], 1, T)
    h = np.zeros((N, 3))
    m = T - t2 - 8
    for t in range(T - 1, t2 + m - 1, -1):
        h = _step_back(Bs[sn], w, fr_free[t], h)
    # (both filters have run >= m frames of the same data in the same state there: their gains agree, so do the vectors)
    assert np.max(np.abs(h - g[t2 + m - 1])) < 1e-9 * max(1.0, np.max(np.abs(h)))
    for t in range(t2 + m - 1, t2 - 1, -1):
        h = _step_back(Bs[sn], w, fr[t], h)
    for j in range(0, 26):
        assert np.max(np.abs(h - g[t2 - j - 1])) < 1e-9 * max(1.0, np.max(np.abs(h))), j
        h = _step_back(Bs[s], w, fr[t2 - j - 1], h) if t2 - j - 1 >= 1 else h
