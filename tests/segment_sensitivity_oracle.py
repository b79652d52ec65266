"""
NumPy statement of the evidence gradient (bild_amd.exact.exact_sensitivities), straight loops on top
of tests/gauss_oracle.py, tests/gauss_sensitivity_oracle.py and tests/segment_oracle.py.

By Fisher's identity the gradient of the log evidence of k switches is the posterior mean of the gradient of the
log-likelihood, and the log-likelihood is a sum of table entries F[s][b] and W[s][a - 1][b]:

    grad logev_k = sum over segments (a, b, s) of q_k(a, b, s) * dW[s][a - 1][b]        (a = 0: dF[s][b])

with q_k(a, b, s) the posterior probability that a profile of k switches has the segment [a, b) in state s, from the
forward and backward tables of the segment recursion.  `tangent_tables` differentiates `gauss_oracle.tables` entry by
entry (and forms the same tables of tau itself and of the innovations Fisher terms), `segment_weights` gives q_k,
`omega` its suffix sums along b (the weight of each tau entry), `solve` the outputs per k and for a prior over k.
"""
import numpy as np
from scipy.special import logsumexp

from bild_amd.gauss import covariance

import gauss_oracle as G
import gauss_sensitivity_oracle as GS
import segment_oracle as SO


def tangent_tables(msd, msd_inf, mean, order, x, dmsd, dmsd_inf, dmean):
    """
    The tables of `gauss_oracle.tables` (NaN rule left out: such entries carry no weight) with their tangents and Fisher
    terms: tW (S, T, T + 1), tF (S, T + 1) = minus the sums of tau; dW (P, S, T, T + 1), dF (P, S, T + 1) = minus the sums of
    dtau_p; IW (P, P, S, T, T + 1), IF (P, P, S, T + 1) = the sums of 2 a_p a_q + g_p g_q.
    """
    x = np.asarray(x, dtype=np.float64)
    T, d = x.shape
    S = msd.shape[0]
    P = len(dmsd)
    tW, tF = np.zeros((S, T, T + 1)), np.zeros((S, T + 1))
    dW, dF = np.zeros((P, S, T, T + 1)), np.zeros((P, S, T + 1))
    IW, IF = np.zeros((P, P, S, T, T + 1)), np.zeros((P, P, S, T + 1))
    for n in range(S):
        for k in range(d):
            valid = np.nonzero(~np.isnan(x[:, k]))[0]
            m, o = mean[n, k], order[n, k]
            for a in range(T + 1):          # a == T: the first interval
                first = a == T
                u = valid[valid >= (0 if first else a)]
                if o == 0:
                    y = x[u, k] - m
                    raw = (not first) and len(u) > 0
                    if raw:
                        y[0] = x[u[0], k]
                    ends, skip, n_e = u, (0 if first else 1), len(u)
                else:
                    y = np.diff(x[u, k]) - m
                    raw = False
                    ends, skip, n_e = u[1:], 0, max(len(u) - 1, 0)
                tau, dtau, aa, gg = np.zeros(n_e), np.zeros((P, n_e)), np.zeros((P, n_e)), np.zeros((P, n_e))
                if n_e:
                    C = covariance(msd[n, k], msd_inf[n, k], u, o)
                    dC = [covariance(dmsd[p, n, k], dmsd_inf[p, n, k], u, o) for p in range(P)]
                    L, dL = GS.tangent_factor(C, dC)
                    z = np.linalg.solve(L, y)
                    dg = np.diag(L)
                    tau = np.log(dg) + 0.5 * z ** 2 + 0.5 * G.LOG2PI
                    for p in range(P):
                        dy = np.full(len(y), -dmean[p, n, k])
                        if raw:
                            dy[0] = 0.0
                        dz = np.linalg.solve(L, dy - dL[p] @ z)
                        aa[p] = np.diag(dL[p]) / dg
                        gg[p] = aa[p] * z + dz
                        dtau[p] = aa[p] + z * dz
                lo = 0 if first else a
                b = np.arange(lo + 1, T + 1)
                idx = np.searchsorted(ends, b, side='left')       # entries with ends < b
                counted = np.arange(n_e) >= skip

                def cum(v):
                    return np.concatenate(([0.0], np.cumsum(np.where(counted, v, 0.0))))[idx]
                (tF[n] if first else tW[n, a])[b] -= cum(tau)
                for p in range(P):
                    (dF[p, n] if first else dW[p, n, a])[b] -= cum(dtau[p])
                    for q in range(P):
                        (IF[p, q, n] if first else IW[p, q, n, a])[b] += cum(2 * aa[p] * aa[q] + gg[p] * gg[q])
    return tW, tF, dW, dF, IW, IF


def segment_weights(W, F, transitions, A, Gb, k):
    """
    q0 (S, T + 1): the posterior probability, among the profiles of k switches without a NaN window, of a first segment [0, b)
    in state s; q (S, T, T + 1), indexed [s, a - 1, b]: of a later segment [a, b) in state s
    """
    S, T = F.shape[0], F.shape[1] - 1
    tot = SO._lse(list(A[k, T]))
    q0, q = np.zeros((S, T + 1)), np.zeros((S, T, T + 1))
    if tot == -np.inf:
        return q0, q
    with np.errstate(invalid='ignore', divide='ignore'):     # (rows without a term: masked below)
        for s in range(S):
            for b in range(1, T + 1):
                if not np.isnan(F[s, b]):
                    q0[s, b] = np.exp(F[s, b] + Gb[k, b, s] - tot)
            if k == 0:
                continue
            for a in range(1, T):
                # log alpha_j(a, s): the partial profiles whose j-th switch is at a, into s; then the row over b at once
                la = np.array([SO._lse([A[j - 1, a, r] for r in range(S) if transitions[r, s]]) for j in range(1, k + 1)])
                b = np.arange(a + 1, T + 1)
                terms = la[:, None] + np.array([Gb[k - j, b, s] for j in range(1, k + 1)])      # (k, len(b))
                top = np.max(terms, axis=0)
                lse = np.where(top > -np.inf, top + np.log(np.sum(np.exp(terms - np.where(top > -np.inf, top, 0.0)), axis=0)), -np.inf)
                w = W[s, a - 1, b]
                q[s, a - 1, b] = np.where(np.isnan(w), 0.0, np.exp(lse + np.nan_to_num(w, nan=0.0) - tot))
    return q0, q


def omega(q0, q):
    """ Omega0 (S, T): sum_{b > t} q0[s, b]; Omega (S, T, T), indexed [s, a - 1, t]: sum_{b > t} q[s, a - 1, b] """
    S, T = q0.shape[0], q0.shape[1] - 1
    om0, om = np.zeros((S, T)), np.zeros((S, T, T))
    for t in range(T):
        om0[:, t] = q0[:, t + 1:].sum(axis=1)
        om[:, :, t] = q[:, :, t + 1:].sum(axis=2)
    return om0, om


def contract(q0, q, tabF, tabW):
    """ sum over the segments of q * table (leading axes of the table are kept); NaN entries carry no weight """
    return np.sum(q0 * np.nan_to_num(tabF), axis=(-2, -1)) + np.sum(q * np.nan_to_num(tabW), axis=(-3, -2, -1))


def solve(msd, msd_inf, mean, order, x, transitions, k_max, dmsd, dmsd_inf, dmean, log_k_prior=None, nan='propagate'):
    """
    dict: logev (K,), and per k (NaN rows where logev is not finite) grad_k (K, P), exp_logl_k (K,), fisher_k (K, P, P),
    n_segments (K,) = sum of q_k; for the prior over k (log weights (K,), None: uniform) log_marginal, k_post (K,), grad (P,),
    exp_logl, fisher (P, P) -- NaN where a k of positive prior weight has a NaN evidence.
    """
    transitions = np.asarray(transitions, dtype=bool)
    K, P = k_max + 1, len(dmsd)
    W, F = G.tables(msd, msd_inf, mean, order, x)
    tW, tF, dW, dF, IW, IF = tangent_tables(msd, msd_inf, mean, order, x, dmsd, dmsd_inf, dmean)
    logev = SO.solve(W, F, transitions, k_max, nan=nan, with_marginals=False)['logev']
    A = SO.forward(W, F, transitions, k_max)[0]
    Gb = SO.backward(W, transitions, k_max)
    out = {'logev': logev, 'grad_k': np.full((K, P), np.nan), 'exp_logl_k': np.full(K, np.nan),
           'fisher_k': np.full((K, P, P), np.nan), 'n_segments': np.full(K, np.nan)}
    for k in range(K):
        if not np.isfinite(logev[k]):
            continue
        q0, q = segment_weights(W, F, transitions, A, Gb, k)
        out['n_segments'][k] = q0.sum() + q.sum()
        out['grad_k'][k] = contract(q0, q, dF, dW)
        out['exp_logl_k'][k] = contract(q0, q, tF, tW)
        out['fisher_k'][k] = contract(q0, q, IF, IW)
    lp = np.zeros(K) if log_k_prior is None else np.asarray(log_k_prior, dtype=np.float64)
    use = lp > -np.inf
    lp = lp - logsumexp(lp[use])
    if np.any(np.isnan(logev[use])):
        out.update(log_marginal=np.nan, k_post=np.full(K, np.nan), grad=np.full(P, np.nan), exp_logl=np.nan,
                   fisher=np.full((P, P), np.nan))
        return out
    lw = np.where(use, lp + np.where(use, logev, 0.0), -np.inf)
    out['log_marginal'] = float(logsumexp(lw[use]))
    post = np.where(lw > -np.inf, np.exp(lw - out['log_marginal']), 0.0)
    out['k_post'] = post
    on = post > 0
    out['grad'] = post[on] @ out['grad_k'][on]
    out['exp_logl'] = float(post[on] @ out['exp_logl_k'][on])
    out['fisher'] = np.tensordot(post[on], out['fisher_k'][on], axes=1)
    return out
