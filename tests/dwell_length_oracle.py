"""
NumPy statement of the expected segment-length counts under a dwell-time prior (bild_amd.exact.exact_dwell_lengths, DESIGN.md
section 24): the segment weights of tests/dwell_sensitivity_oracle.py (`segment_weights`: q0, q) summed along the diagonals
b - a = l, and the same counts from the list of every profile.

    D[s][l] = sum_{a=0}^{T-l-1} Q(a, a + l, s)      completed segments of l frames, 1 <= l <= T - 1
    C[s][l] = Q(T - l, T, s)                        the last segment, censored at l frames, 1 <= l <= T
    I[s]    = sum_{b=1}^{T} Q(0, b, s)              P(theta_0 = s)

All three are (.., T) arrays with length l at column l - 1; D is 0 at l = T.
"""
import numpy as np
from scipy.special import logsumexp

import dwell_oracle as DO
import dwell_sensitivity_oracle as DS
import segment_cases as C


def diagonals(q0, q):
    """ (D (S, T), C (S, T), I (S,)) from q0 (S, T + 1), a first segment [0, b), and q (S, T, T + 1) indexed [s, a - 1, b] """
    S, T = q0.shape[0], q0.shape[1] - 1
    D, Cn = np.zeros((S, T)), np.zeros((S, T))
    for s in range(S):
        for length in range(1, T + 1):
            a = T - length
            Cn[s, length - 1] = q0[s, T] if a == 0 else q[s, a - 1, T]
            if length < T:
                D[s, length - 1] = q0[s, length] + sum(q[s, a - 1, a + length] for a in range(1, T - length))
    return D, Cn, q0[:, 1:].sum(axis=1)


def solve(W, F, prior, nan='propagate'):
    """
    dict: logev, n_nan_windows (as `dwell_sensitivity_oracle.segment_weights` gives them), dwell (S, T), cens (S, T), init (S,);
    the counts are NaN where logev is not finite
    """
    S, T = F.shape[0], F.shape[1] - 1
    out = DS.segment_weights(W, F, prior, nan=nan)
    if out['q0'] is None:
        out.update(dwell=np.full((S, T), np.nan), cens=np.full((S, T), np.nan), init=np.full(S, np.nan))
    else:
        out['dwell'], out['cens'], out['init'] = diagonals(out['q0'], out['q'])
    return out


def enumerate_all(W, F, prior, nan='propagate'):
    """
    the counts from every profile of every k, weighted by exp(`DwellPrior.log_prob` + `segment_cases.table_logl`): dict with
    logev, dwell, cens, init and n_nan (profiles of finite prior weight whose logL is NaN: they weigh 0 under 'omit')
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
    out = {'n_nan': int(bad.sum()), 'logev': np.nan, 'dwell': np.full((S, T), np.nan), 'cens': np.full((S, T), np.nan),
           'init': np.full(S, np.nan)}
    states, joint = states[~bad], joint[~bad]
    if (nan == 'propagate' and out['n_nan']) or not np.any(joint > -np.inf):
        return out
    out['logev'] = float(logsumexp(joint))
    weight = np.exp(joint - out['logev'])
    D, Cn, first = np.zeros((S, T)), np.zeros((S, T)), np.zeros(S)
    for row, w in zip(states, weight):
        cuts = np.concatenate(([0], np.flatnonzero(np.diff(row)) + 1, [T]))
        first[row[0]] += w
        for i in range(len(cuts) - 1):
            (D if i + 2 < len(cuts) else Cn)[row[cuts[i]], cuts[i + 1] - cuts[i] - 1] += w
    out['dwell'], out['cens'], out['init'] = D, Cn, first
    return out
