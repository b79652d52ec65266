"""
NumPy statement of the exact posterior of the number of visits to a set G of states under a dwell-time prior
(bild_amd.exact.exact_dwell_visits) on the tables (W, F) that `gauss_oracle.tables` returns, and the
same answer from the list of every profile.  A visit is a maximal run of consecutive frames in G.  Loops over the end frames,
the states and the switch frames; the numbers n of visits are one array, and the terms of one sum are gathered before they
are added (from their maximum).

With omega_s(a, b) = log_dwell[s][b - a] for b < T and log_surv[s][T - a] for b = T, and g_s = 1 for s in G and 0 otherwise:

    A(b, s, n) = [n = g_s] init_s e^omega_s(0, b) e^F[s][b] + sum_{c=1}^{b-1} e^alpha(c, s, n) e^omega_s(c, b) e^W[s][c-1][b]
    alpha(c, s, n) = sum_r A(c, r, n - [r not in G and s in G]) jump[r][s]                  1 <= c < T
    log_visits[n][s] = A(T, s, n) - logev

Rows n > n_max are neither kept nor fed.  logev and the count of NaN windows are those of the ordinary forward pass
(`dwell_event_oracle.forward`).  A NaN window enters no sum.
"""
import numpy as np

import dwell_event_oracle as DE
import dwell_oracle as DO
import segment_cases as C


def _lse_rows(rows, width):
    """ log sum exp over the rows (arrays of `width` entries), entry by entry; no row: -inf """
    if not rows:
        return np.full(width, -np.inf)
    rows = np.asarray(rows, dtype=float)
    top = rows.max(axis=0)
    safe = np.where(top > -np.inf, top, 0.0)
    with np.errstate(divide='ignore'):
        return np.where(top > -np.inf, safe + np.log(np.sum(np.exp(rows - safe), axis=0)), -np.inf)


def _one_up(row):
    """ row n - 1 at n: a visit begins; what leaves the last row is dropped """
    return np.concatenate(([-np.inf], row[:-1]))


def solve(W, F, prior, target, n_max=None, nan='propagate'):
    """
    dict: logev, n_nan_windows, log_visits (n_max + 1, S) and log_tail for the collection of states `target`.  n_max None:
    (T + 1) // 2, complete.  NaN where the NaN rule refuses and where no profile has positive weight.
    """
    S, T = F.shape[0], F.shape[1] - 1
    n_max = (T + 1) // 2 if n_max is None else n_max
    init, jump = prior.log_init, prior.log_jump
    full, n_nan = DE.forward(W, F, prior, init, jump)
    logev = DE._lse(full[T])
    out = {'logev': logev, 'n_nan_windows': n_nan, 'log_visits': np.full((n_max + 1, S), np.nan), 'log_tail': np.nan}
    if nan == 'propagate' and n_nan:
        out['logev'] = np.nan
        return out
    if logev == -np.inf:
        return out

    inside = np.isin(np.arange(S), list(target))
    N = min(n_max, (T + 1) // 2) + 1        # rows kept
    al = np.full((T + 1, S, N), -np.inf)    # alpha(c, s, n)
    A = np.full((S, N), -np.inf)
    for b in range(1, T + 1):
        for s in range(S):
            rows = []
            first = 1 if inside[s] else 0
            if not np.isnan(F[s, b]) and first < N:
                row = np.full(N, -np.inf)
                row[first] = init[s] + DE._omega(prior, s, 0, b, T) + F[s, b]
                rows.append(row)
            for c in range(1, b):
                w = W[s, c - 1, b]
                if np.isnan(w):
                    continue
                rows.append(al[c, s] + (DE._omega(prior, s, c, b, T) + w))
            A[s] = _lse_rows(rows, N)
        if b < T:
            for s in range(S):
                al[b, s] = _lse_rows([(_one_up(A[r]) if inside[s] and not inside[r] else A[r]) + jump[r, s] for r in range(S)], N)
    visits = np.full((n_max + 1, S), -np.inf)
    visits[:N] = A.T - logev
    out['log_visits'] = visits
    with np.errstate(divide='ignore'):
        out['log_tail'] = -np.inf if n_max >= (T + 1) // 2 else float(np.log(max(0.0, 1.0 - np.sum(np.exp(visits)))))
    return out


def count_visits(states, inside):
    """ the visits of a row of states to the set `inside` (bool per state): 0 -> 1 steps of the indicator plus the indicator at frame 0 """
    hit = inside[np.asarray(states)]
    return int(hit[0]) + int(np.count_nonzero(hit[1:] & ~hit[:-1]))


def enumerate_all(W, F, prior, target, nan='propagate'):
    """
    the answer of `solve` at complete n_max from every profile of every k, weighted by exp(`DwellPrior.log_prob` +
    `segment_cases.table_logl` - logev) and binned by (visits to the target, last state): dict with logev, n_nan (profiles of
    finite prior weight whose logL is NaN: they weigh 0 under 'omit') and log_visits ((T + 1) // 2 + 1, S)
    """
    S, T = F.shape[0], F.shape[1] - 1
    states, joint = [], []
    for k, seg_start, seg_state, st in DO.all_profiles(T, S):
        logl = C.table_logl(W, F, seg_start, seg_state, T)
        prior_lp = np.array([prior.log_prob(row) for row in st])
        states.append(st)
        with np.errstate(invalid='ignore'):
            joint.append(np.where(prior_lp == -np.inf, -np.inf, prior_lp + logl))
    states, joint = np.concatenate(states), np.concatenate(joint)
    bad = np.isnan(joint)
    rows = (T + 1) // 2 + 1
    out = {'n_nan': int(bad.sum()), 'logev': np.nan, 'log_visits': np.full((rows, S), np.nan)}
    states, joint = states[~bad], joint[~bad]
    if (nan == 'propagate' and out['n_nan']) or not np.any(joint > -np.inf):
        return out
    out['logev'] = DE._lse(joint)
    weight = np.exp(joint - out['logev'])
    inside = np.isin(np.arange(S), list(target))
    vis = np.zeros((rows, S))
    for row, w in zip(states, weight):
        vis[count_visits(row, inside), row[-1]] += w
    with np.errstate(divide='ignore'):
        out['log_visits'] = np.log(vis)
    return out


def prior_support(prior, target, S, T):
    """ ((T + 1) // 2 + 1, S) bool: some profile of T frames that the prior gives positive weight has n visits to the target and ends in s """
    inside = np.isin(np.arange(S), list(target))
    out = np.zeros(((T + 1) // 2 + 1, S), dtype=bool)
    for _, _, _, st in DO.all_profiles(T, S):
        for row in st:
            if prior.log_prob(row) > -np.inf:
                out[count_visits(row, inside), row[-1]] = True
    return out
