"""
NumPy statement of the exact posterior of the number of frames in a set G of states under a dwell-time prior
(bild_amd.exact.exact_dwell_occupancy) on the tables (W, F) that `gauss_oracle.tables` returns, and the
same answer from the list of every profile.  Loops over the end frames, the states and the switch frames; the numbers n of
frames in G are one array, and the terms of one sum are gathered before they are added (from their maximum).

With omega_s(a, b) = log_dwell[s][b - a] for b < T and log_surv[s][T - a] for b = T, and g_s = 1 for s in G and 0 otherwise:

    A(b, s, n) = [n = g_s b] init_s e^omega_s(0, b) e^F[s][b]
                 + sum_{c=1}^{b-1} e^alpha(c, s, n - g_s (b - c)) e^omega_s(c, b) e^W[s][c-1][b]
    alpha(c, s, n) = log sum_s' e^A(c, s', n) jump[s'][s]                  1 <= c < T, empty outside 0 <= n <= c
    log_occupancy[n][s] = A(T, s, n) - logev

logev and the count of NaN windows are those of the ordinary forward pass (`dwell_event_oracle.forward`).  A NaN window
enters no sum.
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


def solve(W, F, prior, target, nan='propagate'):
    """
    dict: logev, n_nan_windows, log_occupancy (T + 1, S) for the collection of states `target`.  NaN where the NaN rule refuses
    and where no profile has positive weight.
    """
    S, T = F.shape[0], F.shape[1] - 1
    init, jump = prior.log_init, prior.log_jump
    full, n_nan = DE.forward(W, F, prior, init, jump)
    logev = DE._lse(full[T])
    out = {'logev': logev, 'n_nan_windows': n_nan, 'log_occupancy': np.full((T + 1, S), np.nan)}
    if nan == 'propagate' and n_nan:
        out['logev'] = np.nan
        return out
    if logev == -np.inf:
        return out

    inside = np.isin(np.arange(S), list(target))
    al = np.full((T + 1, S, T + 1), -np.inf)       # alpha(c, s, n)
    A = np.full((S, T + 1), -np.inf)
    for b in range(1, T + 1):
        for s in range(S):
            rows = []
            if not np.isnan(F[s, b]):
                row = np.full(T + 1, -np.inf)
                row[b if inside[s] else 0] = init[s] + DE._omega(prior, s, 0, b, T) + F[s, b]
                rows.append(row)
            for c in range(1, b):
                w = W[s, c - 1, b]
                if np.isnan(w):
                    continue
                row = np.full(T + 1, -np.inf)
                if inside[s]:
                    row[b - c:] = al[c, s, :T + 1 - (b - c)]
                else:
                    row[:] = al[c, s]
                rows.append(row + (DE._omega(prior, s, c, b, T) + w))
            A[s] = _lse_rows(rows, T + 1)
        if b < T:
            for s in range(S):      # (A(b, ., n) is empty behind n = b, and so is alpha)
                al[b, s] = _lse_rows([A[r] + jump[r, s] for r in range(S)], T + 1)
    out['log_occupancy'] = A.T - logev
    return out


def enumerate_all(W, F, prior, target, nan='propagate'):
    """
    the answer of `solve` from every profile of every k, weighted by exp(`DwellPrior.log_prob` + `segment_cases.table_logl` -
    logev) and binned by (frames in the target, last state): dict with logev, n_nan (profiles of finite prior weight whose logL
    is NaN: they weigh 0 under 'omit') and log_occupancy (T + 1, S)
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
    out = {'n_nan': int(bad.sum()), 'logev': np.nan, 'log_occupancy': np.full((T + 1, S), np.nan)}
    states, joint = states[~bad], joint[~bad]
    if (nan == 'propagate' and out['n_nan']) or not np.any(joint > -np.inf):
        return out
    out['logev'] = DE._lse(joint)
    weight = np.exp(joint - out['logev'])
    inside = np.isin(np.arange(S), list(target))
    occ = np.zeros((T + 1, S))
    for row, w in zip(states, weight):
        occ[inside[row].sum(), row[-1]] += w
    with np.errstate(divide='ignore'):
        out['log_occupancy'] = np.log(occ)
    return out


def prior_support(prior, target, S, T):
    """ (T + 1, S) bool: some profile of T frames that the prior gives positive weight has n frames in the target and ends in s """
    inside = np.isin(np.arange(S), list(target))
    out = np.zeros((T + 1, S), dtype=bool)
    for _, _, _, st in DO.all_profiles(T, S):
        for row in st:
            if prior.log_prob(row) > -np.inf:
                out[inside[row].sum(), row[-1]] = True
    return out
