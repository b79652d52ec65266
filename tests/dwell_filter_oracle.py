"""
NumPy statement of the exact online filter under a dwell-time prior (bild_amd.exact.exact_dwell_filter)
on the tables (W, F) that `gauss_oracle.tables` returns.  Straight loops and `logsumexp`; the forward pass is written as in
`dwell_oracle.solve`.

For the prefix ends b = 1 ... T (frame t = b - 1), with alpha(c, s) of the forward pass (log_dwell on every completed segment):

    G(b, s) = log( init_s e^log_surv[s][b] e^F[s][b] + sum_{c=1}^{b-1} e^alpha(c, s) e^log_surv[s][b - c] e^W[s][c-1][b] )
    E(b) = log sum_s e^G(b, s)

E(b) is what `dwell_oracle.solve` gives as the evidence of x[:b]: a window's table entry depends on the data inside the window
alone.  A NaN window never enters a sum; it is counted where a partial profile of finite prior weight without a NaN window
reaches its start, once under its log_surv weight (nG(b)) and once under its log_dwell weight (nA(b)).  The truncation x[:t + 1]
has skipped nG(t + 1) + sum_{e <= t} nA(e) windows.
"""
import numpy as np
from scipy.special import logsumexp


def _lse(terms):
    terms = [t for t in terms if t > -np.inf]
    return float(logsumexp(terms)) if terms else -np.inf


def solve(W, F, prior, nan='propagate', run_max=0):
    """
    dict: prefix_logev (T,), log_filtered (S, T), run_mean (T,), log_run (S, T, run_max) or None, n_nan_windows (T,) int64,
    nG and nA (T + 1,) int64 indexed by b, logev (= prefix_logev[-1]).  Under nan='propagate' every output at a frame with
    n_nan_windows > 0 is NaN; a frame with E = -inf has NaN in log_filtered, run_mean and its rows of log_run.
    """
    S, T = F.shape[0], F.shape[1] - 1
    R = int(run_max)
    init, jump, dwell, surv = prior.log_init, prior.log_jump, prior.log_dwell, prior.log_surv
    al = np.full((T + 1, S), -np.inf)
    reach = np.zeros((T + 1, S), dtype=bool)    # a partial profile of finite prior weight without a NaN window jumps into s at c
    nG, nA = np.zeros(T + 1, dtype=np.int64), np.zeros(T + 1, dtype=np.int64)
    E = np.full(T + 1, -np.inf)
    G = np.full((T + 1, S), -np.inf)
    length = np.full(T + 1, np.nan)
    run = np.full((S, T, R), -np.inf) if R else None
    for b in range(1, T + 1):
        A = np.full(S, -np.inf)
        has = np.zeros(S, dtype=bool)
        weighted = 0.0
        cens = [[] for _ in range(S)]       # (c, log weight) of the windows [c, b) as the last, censored segment
        for s in range(S):
            done = []                       # the same windows as completed segments
            for c in range(b):
                if c == 0:
                    if init[s] == -np.inf:
                        continue
                    head, w = init[s], F[s, b]
                else:
                    if not reach[c, s]:
                        continue
                    head, w = al[c, s], W[s, c - 1, b]
                sv, dv = surv[s, b - c - 1], dwell[s, b - c - 1]
                if np.isnan(w):
                    nG[b] += sv > -np.inf
                    nA[b] += dv > -np.inf
                    continue
                if sv > -np.inf:
                    cens[s].append((c, head + sv + w))
                if dv > -np.inf:
                    done.append(head + dv + w)
                    has[s] = True
            G[b, s] = _lse([v for _, v in cens[s]])
            A[s] = _lse(done)
        E[b] = _lse(list(G[b]))
        if E[b] > -np.inf:
            for s in range(S):
                for c, v in cens[s]:
                    if v > -np.inf:
                        weighted += (b - c) * np.exp(v - E[b])
                        if b - c <= R:
                            run[s, b - 1, b - c - 1] = v - E[b]
            length[b] = weighted
        if b == T:
            break
        for s in range(S):
            al[b, s] = _lse([A[q] + jump[q, s] for q in range(S)])
            reach[b, s] = any(has[q] and jump[q, s] > -np.inf for q in range(S))

    n_nan = nG[1:] + np.concatenate(([0], np.cumsum(nA[1:T])))
    live = E[1:] > -np.inf
    keep = np.ones(T, dtype=bool) if nan == 'omit' else n_nan == 0
    with np.errstate(invalid='ignore'):
        filt = np.where(live & keep, (G[1:] - E[1:, None]).T, np.nan)
    out = {'prefix_logev': np.where(keep, E[1:], np.nan), 'log_filtered': filt, 'run_mean': np.where(live & keep, length[1:], np.nan),
           'log_run': None, 'n_nan_windows': n_nan, 'nG': nG, 'nA': nA}
    if R:
        out['log_run'] = np.where((live & keep)[None, :, None], run, np.nan)
    out['logev'] = out['prefix_logev'][-1]
    return out
