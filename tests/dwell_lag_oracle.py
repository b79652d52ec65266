"""
NumPy statement of exact fixed-lag smoothing under a dwell-time prior (bild_amd.exact.exact_dwell_lag) on
the tables (W, F) that `gauss_oracle.tables` returns.  Loops over the frames, the cuts and the states; one axis (the starts a of a
sum, or its ends b) is handed to one NumPy reduction or to `np.logaddexp.accumulate`, because plain loops over T^2 lag^2 terms would pass
the 20 s a designed case may take.

A cut u = 1 ... T is the truncated trajectory x[:u].  With alpha(a, s) of the forward pass (`dwell_oracle.solve`'s), head(0, s) =
log_init[s], w(0, b, s) = F[s][b], head(a, s) = alpha(a, s) and w(a, b, s) = W[s][a - 1][b] for a >= 1:

    Pd(b, t, s) = log sum_{a <= t} exp(head(a, s) + log_dwell[s][b - a] + w(a, b, s))      t < b      (a running sum over a)
    Ps(b, t, s) = the same with log_surv[s][b - a]
    gamma_u(u, s) = 0
    beta_u(a, s) = log sum_{a < b <= u} exp(omega_u(a, b, s) + W[s][a - 1][b] + gamma_u(b, s)),  omega_u = log_dwell, log_surv at b = u
    gamma_u(a, s) = log sum_s'' exp(log_jump[s][s''] + beta_u(a, s''))
    J_u(t, s) = log( exp Ps(u, t, s) + sum_{t < b < u} exp(Pd(b, t, s) + gamma_u(b, s)) ),      E(u) = log sum_s exp J_u(u - 1, s)

log_lagged[s][t][l] = J_u(t, s) - E(u) with u = min(t + l + 1, T).  The running sums are split at no lag: the device code's split
of the starts at the left edge of the window (Hbase, Kbase) is not used here.  A NaN window never enters a sum; the counts are
those of tests/dwell_filter_oracle.py, written again.
"""
import numpy as np


def _lse(terms):
    """ (written out: `scipy.special.logsumexp` costs ten times as much a call, and the largest case makes 130 000 of them) """
    terms = np.asarray(terms, dtype=float)
    top = np.max(terms, initial=-np.inf)
    return float(top + np.log(np.sum(np.exp(terms - top)))) if top > -np.inf else -np.inf


def forward(W, F, prior):
    """ alpha (T + 1, S), and nG, nA (T + 1,) indexed by the end frame b: the NaN windows skipped under log_surv and log_dwell """
    S, T = F.shape[0], F.shape[1] - 1
    init, jump, dwell, surv = prior.log_init, prior.log_jump, prior.log_dwell, prior.log_surv
    al = np.full((T + 1, S), -np.inf)
    reach = np.zeros((T + 1, S), dtype=bool)
    nG, nA = np.zeros(T + 1, dtype=np.int64), np.zeros(T + 1, dtype=np.int64)
    for b in range(1, T + 1):
        A = np.full(S, -np.inf)
        has = np.zeros(S, dtype=bool)
        for s in range(S):
            # the starts a = 0 ... b - 1 at once
            head = np.concatenate(([init[s]], al[1:b, s]))
            ok = np.concatenate(([init[s] > -np.inf], reach[1:b, s]))
            w = np.concatenate(([F[s, b]], W[s, np.arange(b - 1), b]))
            length = b - np.arange(b)
            sv, dv = surv[s, length - 1], dwell[s, length - 1]
            bad = np.isnan(w)
            nG[b] += np.sum(ok & bad & (sv > -np.inf))
            nA[b] += np.sum(ok & bad & (dv > -np.inf))
            use = ok & ~bad & (dv > -np.inf)
            has[s] = use.any()
            A[s] = _lse((head + dv + np.where(bad, 0.0, w))[use])
        if b == T:
            break
        for s in range(S):
            al[b, s] = _lse([A[q] + jump[q, s] for q in range(S)])
            reach[b, s] = any(has[q] and jump[q, s] > -np.inf for q in range(S))
    return al, nG, nA


def solve(W, F, prior, lag, nan='propagate'):
    """
    dict: log_lagged (S, T, lag + 1), n_nan_windows (T,) int64 (per prefix, as the filter's), prefix_logev (T,) = E(t + 1) without
    the NaN rule.  Under nan='propagate' an entry whose cut u has n_nan_windows[u - 1] > 0 is NaN; a cut with E(u) = -inf has NaN
    in all its entries; an entry of probability 0 is -inf.
    """
    S, T = F.shape[0], F.shape[1] - 1
    lag = int(lag)
    init, jump, dwell, surv = prior.log_init, prior.log_jump, prior.log_dwell, prior.log_surv
    al, nG, nA = forward(W, F, prior)
    n_nan = nG[1:] + np.concatenate(([0], np.cumsum(nA[1:T])))

    # the running sums over the starts: Pd[s][b][t], Ps[s][b][t], t < b
    Pd = np.full((S, T + 1, T), -np.inf)
    Ps = np.full((S, T + 1, T), -np.inf)
    for s in range(S):
        for b in range(1, T + 1):
            head = np.concatenate(([init[s]], al[1:b, s]))
            w = np.concatenate(([F[s, b]], W[s, np.arange(b - 1), b]))
            length = b - np.arange(b)
            with np.errstate(invalid='ignore'):
                common = np.where(np.isnan(w), -np.inf, head + w)
                Pd[s, b, :b] = np.logaddexp.accumulate(common + dwell[s, length - 1])
                Ps[s, b, :b] = np.logaddexp.accumulate(common + surv[s, length - 1])

    J = {}      # per cut u: (lo, array (u - lo, S)) of J_u(t, s), t = lo ... u - 1
    E = np.full(T + 1, -np.inf)
    for u in range(1, T + 1):
        lo = max(u - 1 - lag, 0)
        g = np.full((u + 1, S), -np.inf)
        g[u] = 0.0
        for a in range(u - 1, lo, -1):
            beta = np.full(S, -np.inf)
            for s in range(S):
                b = np.arange(a + 1, u + 1)
                om = np.where(b == u, surv[s, u - a - 1], dwell[s, b - a - 1])
                w = W[s, a - 1, b]
                with np.errstate(invalid='ignore'):
                    beta[s] = _lse(np.where(np.isnan(w), -np.inf, om + w + g[b, s]))
            for s in range(S):
                g[a, s] = _lse(jump[s] + beta)
        Ju = np.full((u - lo, S), -np.inf)
        for t in range(lo, u):
            for s in range(S):
                b = np.arange(t + 1, u)
                Ju[t - lo, s] = _lse(np.concatenate(([Ps[s, u, t]], Pd[s, b, t] + g[b, s])))
        J[u] = (lo, Ju)
        E[u] = _lse(Ju[u - 1 - lo])

    out = np.full((S, T, lag + 1), np.nan)
    for t in range(T):
        for l in range(lag + 1):
            u = min(t + l + 1, T)
            if E[u] == -np.inf or (nan == 'propagate' and n_nan[u - 1] > 0):
                continue
            lo, Ju = J[u]
            out[:, t, l] = Ju[t - lo] - E[u]
    return {'log_lagged': out, 'n_nan_windows': n_nan, 'prefix_logev': E[1:].copy()}


def settling_lag(log_lagged, tol=1e-3):
    """ `DwellLagResults.settling_lag` in loops: per frame the smallest l from which every later computed column stays within tol of the last """
    S, T, n = log_lagged.shape
    lag = n - 1
    out = np.full(T, -1, dtype=np.int64)
    for t in range(T):
        p = np.exp(log_lagged[:, t, :])
        if np.isnan(p).any():
            continue
        out[t] = lag
        for l in range(lag, -1, -1):        # (the columns behind T - 1 - t repeat column `lag`)
            if np.max(np.abs(p[:, l] - p[:, lag])) > tol:
                break
            out[t] = l
    return out
