"""
NumPy statement of the evidence gradient under a dwell-time prior (bild_amd.exact.exact_dwell_sensitivities, DESIGN.md section
23): straight loops on top of tests/gauss_oracle.py's tables, tests/segment_sensitivity_oracle.py's tangent tables and
tests/gauss_sensitivity_oracle.py.

By Fisher's identity the gradient of the log evidence is the posterior mean of the gradient of the log-likelihood, and the
log-likelihood is a sum of table entries F[s][b] and W[s][a - 1][b]; the prior does not depend on the model's parameters.  So

    grad logev = sum over segments (a, b, s) of Q(a, b, s) dW[s][a - 1][b]        (a = 0: dF[s][b])

with Q the posterior probability of the segment [a, b) in state s under the prior.  `segment_weights` restates section 21's
recursions to get Q (`dwell_oracle.solve` does not return it), `solve` contracts Q with the tangent tables, and
`enumerate_all` gives the same three outputs from the list of every profile.
"""
import numpy as np
from scipy.special import logsumexp

import dwell_oracle as DO
import gauss_oracle as G
import gauss_sensitivity_oracle as GS
import segment_sensitivity_oracle as SS


def _lse(terms):
    terms = [t for t in terms if t > -np.inf]
    return float(logsumexp(terms)) if terms else -np.inf


def segment_weights(W, F, prior, nan='propagate'):
    """
    dict: logev (NaN under nan='propagate' with n_nan_windows > 0), n_nan_windows, and, where logev is finite, q0 (S, T + 1):
    the posterior probability of a first segment [0, b) in state s, and q (S, T, T + 1), indexed [s, a - 1, b]: of a later segment
    [a, b) in state s (None otherwise).  A NaN window weighs 0.
    """
    S, T = F.shape[0], F.shape[1] - 1
    init, jump, dwell, surv = prior.log_init, prior.log_jump, prior.log_dwell, prior.log_surv

    def om(s, a, b):
        return surv[s, T - a - 1] if b == T else dwell[s, b - a - 1]

    # forward: A(b, s) over the partial profiles that end a segment of state s at b; alpha(c, s) those that jump into s at c
    A = np.full((T + 1, S), -np.inf)
    al = np.full((T + 1, S), -np.inf)
    n_nan = 0
    for b in range(1, T + 1):
        for s in range(S):
            terms = []
            if init[s] + om(s, 0, b) > -np.inf:
                if np.isnan(F[s, b]):
                    n_nan += 1
                else:
                    terms.append(init[s] + om(s, 0, b) + F[s, b])
            for c in range(1, b):
                if al[c, s] == -np.inf or om(s, c, b) == -np.inf:
                    continue
                if np.isnan(W[s, c - 1, b]):
                    n_nan += 1
                else:
                    terms.append(al[c, s] + om(s, c, b) + W[s, c - 1, b])
            A[b, s] = _lse(terms)
        if b < T:
            for s in range(S):
                al[b, s] = _lse([A[b, r] + jump[r, s] for r in range(S)])
    logev = _lse(list(A[T]))
    out = {'logev': logev, 'n_nan_windows': n_nan, 'q0': None, 'q': None}
    if nan == 'propagate' and n_nan:
        out['logev'] = np.nan
        return out
    if logev == -np.inf:
        return out

    # backward: beta(a, s) over the continuations of a segment of state s that starts at a; gamma(b, s) behind a segment that ends at b
    gam = np.full((T + 1, S), -np.inf)
    gam[T] = 0.0
    for a in range(T - 1, 0, -1):
        beta = [_lse([om(s, a, b) + W[s, a - 1, b] + gam[b, s] for b in range(a + 1, T + 1) if not np.isnan(W[s, a - 1, b])])
                for s in range(S)]
        for s in range(S):
            gam[a, s] = _lse([jump[s, r] + beta[r] for r in range(S)])

    q0, q = np.zeros((S, T + 1)), np.zeros((S, T, T + 1))
    for s in range(S):
        for b in range(1, T + 1):
            if not np.isnan(F[s, b]):
                q0[s, b] = np.exp(init[s] + om(s, 0, b) + F[s, b] + gam[b, s] - logev)
            for a in range(1, b):
                if not np.isnan(W[s, a - 1, b]):
                    q[s, a - 1, b] = np.exp(al[a, s] + om(s, a, b) + W[s, a - 1, b] + gam[b, s] - logev)
    out['q0'], out['q'] = q0, q
    return out


def occupancy(q0, q):
    """ (S, T): sum_{a <= t} Omega(s, a, t), the posterior probability of state s at frame t """
    om0, om = SS.omega(q0, q)
    T = om0.shape[1]
    return om0 + np.array([[om[s, :t, t].sum() for t in range(T)] for s in range(om0.shape[0])])


def solve(msd, msd_inf, mean, order, x, prior, dmsd, dmsd_inf, dmean, nan='propagate'):
    """
    dict: logev, n_nan_windows, grad (P,), exp_logl, fisher (P, P), n_segments = sum of Q, q0, q; the three sums are NaN where
    logev is not finite
    """
    x = np.asarray(x, dtype=np.float64)
    P = len(dmsd)
    W, F = G.tables(msd, msd_inf, mean, order, x)
    out = segment_weights(W, F, prior, nan=nan)
    out.update(grad=np.full(P, np.nan), exp_logl=np.nan, fisher=np.full((P, P), np.nan), n_segments=np.nan)
    if out['q0'] is None:
        return out
    tW, tF, dW, dF, IW, IF = SS.tangent_tables(msd, msd_inf, mean, order, x, dmsd, dmsd_inf, dmean)
    q0, q = out['q0'], out['q']
    out['n_segments'] = q0.sum() + q.sum()
    out['grad'] = SS.contract(q0, q, dF, dW)
    out['exp_logl'] = float(SS.contract(q0, q, tF, tW))
    out['fisher'] = SS.contract(q0, q, IF, IW)
    return out


def enumerate_all(msd, msd_inf, mean, order, x, prior, dmsd, dmsd_inf, dmean, nan='propagate'):
    """
    logev, grad, exp_logl and fisher from `gauss_sensitivity_oracle.batch` of every profile of every k, weighted by
    exp(`DwellPrior.log_prob` + logL); n_nan: profiles of finite prior weight whose logL is NaN (they weigh 0 under 'omit')
    """
    x = np.asarray(x, dtype=np.float64)
    S, T, P = msd.shape[0], len(x), len(dmsd)
    states = np.concatenate([st for _, _, _, st in DO.all_profiles(T, S)])
    lp = np.array([prior.log_prob(row) for row in states])
    states, lp = states[lp > -np.inf], lp[lp > -np.inf]
    logl, g, fi = GS.batch(msd, msd_inf, mean, order, [x], list(states), dmsd=dmsd, dmsd_inf=dmsd_inf, dmean=dmean)
    bad = np.isnan(logl)
    out = {'n_nan': int(bad.sum()), 'logev': np.nan, 'grad': np.full(P, np.nan), 'exp_logl': np.nan, 'fisher': np.full((P, P), np.nan)}
    if (nan == 'propagate' and bad.any()) or bad.all():
        if not len(lp) or (bad.all() and nan == 'omit'):
            out['logev'] = -np.inf
        return out
    lp, logl, g, fi = lp[~bad], logl[~bad], g[~bad], fi[~bad]
    out['logev'] = float(logsumexp(lp + logl))
    w = np.exp(lp + logl - out['logev'])
    out['grad'], out['exp_logl'], out['fisher'] = w @ g, float(w @ logl), np.tensordot(w, fi, axes=1)
    return out
