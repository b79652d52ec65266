"""
Dense NumPy tangent filter over the full model arrays (B, G, Sig, M0, C0, w) and their derivatives: the checker of
MultiStateRouse.logL_sensitivities.  The device runs the same recursion in each state's modal basis; this restates it in
the original N-basis, one dimension at a time (a covariance chain carries dimensions of equal variance, which here simply
repeat), beside the filter of tests/kalman_oracle.py and with its conventions: frame 0 starts from the steady state of
states[0] without a predict, frame t >= 1 is predicted with the propagator of states[t], a frame with any NaN coordinate is
predicted but not updated.
"""
import numpy as np

LOG_2PI = np.log(2 * np.pi)
KEYS = ('dB', 'dG', 'dSig', 'dM0', 'dC0')


def tangent_filter(arrays, w, loc_err, x, states, derivs=None, ds2=None):
    """
    one candidate -> (logL, grad (P,), fisher (P, P)).  derivs: dict of (P, S, N, N) / (P, S, N, d) arrays (absent: 0);
    ds2: (P, d) derivatives of each dimension's variance (None: 0)
    """
    B, G, Sig, M0, C0 = (np.asarray(arrays[k], dtype=np.float64) for k in ('B', 'G', 'Sig', 'M0', 'C0'))
    w = np.asarray(w, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    states = np.asarray(states)
    T, d = x.shape
    N = len(w)
    S_ = len(B)
    derivs = {} if derivs is None else derivs
    P = next((len(v) for v in derivs.values()), 0 if ds2 is None else len(ds2))
    D = {k: (np.asarray(derivs[k], dtype=np.float64) if derivs.get(k) is not None
             else np.zeros((P, S_, N, N if k in ('dB', 'dSig', 'dC0') else d))) for k in KEYS}
    ds2 = np.zeros((P, d)) if ds2 is None else np.asarray(ds2, dtype=np.float64).reshape(P, d)
    observed = ~np.any(np.isnan(x), axis=1)
    ll, grad, fisher = 0.0, np.zeros(P), np.zeros((P, P))
    for k in range(d):
        s2 = float(loc_err[k]) ** 2
        m, C = None, None
        for t in range(T):
            s = states[t]
            if t == 0:
                m, C = M0[s][:, k].copy(), C0[s].copy()
                dm = [D['dM0'][p, s][:, k].copy() for p in range(P)]
                dC = [D['dC0'][p, s].copy() for p in range(P)]
            else:
                Bs, dBs = B[s], D['dB'][:, s]
                dm = [dBs[p] @ m + Bs @ dm[p] + D['dG'][p, s][:, k] for p in range(P)]
                dC = [dBs[p] @ C @ Bs.T + Bs @ dC[p] @ Bs.T + Bs @ C @ dBs[p].T + D['dSig'][p, s] for p in range(P)]
                m = Bs @ m + G[s][:, k]
                C = Bs @ C @ Bs.T + Sig[s]
            if not observed[t]:
                continue
            c = C @ w
            S = w @ c + s2
            e = x[t, k] - w @ m
            dc = [dC[p] @ w for p in range(P)]
            dS = np.array([w @ dc[p] + ds2[p, k] for p in range(P)])
            de = np.array([-(w @ dm[p]) for p in range(P)])
            ll += -0.5 * (e * e / S + np.log(S) + LOG_2PI)
            grad += -e * de / S + 0.5 * e * e * dS / S ** 2 - 0.5 * dS / S
            fisher += np.outer(dS, dS) / (2 * S ** 2) + np.outer(de, de) / S
            K = c / S
            dK = [dc[p] / S - c * dS[p] / S ** 2 for p in range(P)]
            dm = [dm[p] + dK[p] * e + K * de[p] for p in range(P)]
            dC = [dC[p] - (np.outer(dc[p], c) + np.outer(c, dc[p])) / S + np.outer(c, c) * dS[p] / S ** 2 for p in range(P)]
            m = m + K * e
            C = C - np.outer(K, c)
    return ll, grad, fisher


def batch(arrays, w, loc_errs, trajs, states_list, traj_id=None, derivs=None, ds2=None):
    """ many candidates: (logL (n,), grad (n, P), fisher (n, P, P)); loc_errs (n_traj, d), ds2 (P, n_traj, d) or None """
    n = len(states_list)
    tid = np.zeros(n, dtype=int) if traj_id is None else np.asarray(traj_id)
    out = [tangent_filter(arrays, w, loc_errs[tid[r]], trajs[tid[r]], np.asarray(states_list[r])[:len(trajs[tid[r]])], derivs,
                          None if ds2 is None else np.asarray(ds2)[:, tid[r]]) for r in range(n)]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out])


def innovations(arrays, w, loc_err, x, states):
    """ per frame and dimension: (e, S) of the filter of tests/kalman_oracle.py, NaN on missing frames """
    import kalman_oracle as KO
    o = KO.filter_smoother(arrays, w, loc_err, x, states)
    e = np.asarray(x, dtype=np.float64) - o['pred_mean']
    return e, o['pred_var']


def rouse_family(N, S_loops, d=3, w=None):
    """ (arrays(D, k), derivs(D, k) for ('D', 'k')) of bild_amd.rouse models, one per loop entry """
    from bild_amd import rouse

    def models(D, k):
        return [rouse.Model(N, D, k, d, add_bonds=None if lp is None else [lp]) for lp in S_loops]

    def arrays(D, k):
        return rouse.stack_dynamics(models(D, k))

    def derivs(D, k, params=('D', 'k')):
        out = {key: [] for key in KEYS}
        for name in params:
            per = [m.dynamics_derivatives(name) for m in models(D, k)]
            for key in KEYS:
                out[key].append(np.stack([p[key] for p in per]))
        return {key: np.stack(v) for key, v in out.items()}

    return arrays, derivs


def affine_family(rng, N, S, d, P, G_nonzero=True):
    """
    A from_arrays model whose arrays are affine in theta (P,) and diagonal in one orthonormal basis per state (so the
    device accepts the derivatives): B_s = Q_s diag(b0 + theta.b1) Q_s^T, and so on for Sig and C0; G and M0 (N x d) affine
    in theta as well.  -> (arrays(theta), derivs) with derivs independent of theta.
    """
    Qs = [np.linalg.qr(rng.standard_normal((N, N)))[0] for _ in range(S)]
    b0 = rng.uniform(0.3, 0.9, (S, N))
    sg0 = rng.uniform(0.5, 1.5, (S, N))
    c0 = rng.uniform(1.0, 3.0, (S, N))
    b1 = rng.uniform(-0.05, 0.05, (P, S, N))
    sg1 = rng.uniform(-0.2, 0.2, (P, S, N))
    c1 = rng.uniform(-0.3, 0.3, (P, S, N))
    g0 = rng.standard_normal((S, N, d)) * (0.3 if G_nonzero else 0.0)
    m0 = rng.standard_normal((S, N, d)) * (0.5 if G_nonzero else 0.0)
    g1 = rng.standard_normal((P, S, N, d)) * (0.1 if G_nonzero else 0.0)
    m1 = rng.standard_normal((P, S, N, d)) * (0.2 if G_nonzero else 0.0)

    def mat(Q, v):
        X = (Q * v) @ Q.T
        return 0.5 * (X + X.T)

    def arrays(theta):
        theta = np.asarray(theta, dtype=np.float64)
        return {'B': np.stack([mat(Qs[s], b0[s] + theta @ b1[:, s]) for s in range(S)]),
                'Sig': np.stack([mat(Qs[s], sg0[s] + theta @ sg1[:, s]) for s in range(S)]),
                'C0': np.stack([mat(Qs[s], c0[s] + theta @ c1[:, s]) for s in range(S)]),
                'G': g0 + np.tensordot(theta, g1, axes=1), 'M0': m0 + np.tensordot(theta, m1, axes=1)}

    derivs = {'dB': np.stack([np.stack([mat(Qs[s], b1[p, s]) for s in range(S)]) for p in range(P)]),
              'dSig': np.stack([np.stack([mat(Qs[s], sg1[p, s]) for s in range(S)]) for p in range(P)]),
              'dC0': np.stack([np.stack([mat(Qs[s], c1[p, s]) for s in range(S)]) for p in range(P)]),
              'dG': g1, 'dM0': m1}
    return arrays, derivs
