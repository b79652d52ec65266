"""
NumPy statement of the exact evidence by enumeration (bild_amd.exact): the profiles of one
trajectory in enumeration order, and what the library reports from their log-likelihoods.
"""
import itertools
import math

import numpy as np

from bild_amd.amis import CFC
from bild_amd.profiles import states_from_segments


def enumerate_profiles(T, k, transitions):
    """ (seg_start, seg_state), each (n, k + 1) int32: traces outer (CFC.full_sample order), combinations inner """
    if T - 1 < k:
        return np.zeros((0, k + 1), np.int32), np.zeros((0, k + 1), np.int32)
    traces = CFC(transitions).full_sample(k, Nmax=np.inf)
    combos = np.array(list(itertools.combinations(range(1, T), k)), dtype=np.int32).reshape(math.comb(T - 1, k), k)
    n_c = len(combos)
    seg_start = np.concatenate([np.zeros((len(traces) * n_c, 1), np.int32), np.tile(combos, (len(traces), 1))], axis=1)
    seg_state = np.repeat(np.asarray(traces, dtype=np.int32), n_c, axis=0)
    return seg_start, seg_state


def reduce(logL, seg_start, seg_state, T, S, marginals=True):
    """ logev, KL, MAP index and logL, n_nan and the (S, T) log marginals from the logLs in enumeration order """
    logL = np.asarray(logL, dtype=np.float64)
    n = len(logL)
    nan = np.isnan(logL)
    out = {'n_profiles': n, 'n_nan': int(nan.sum()), 'map_index': -1, 'map_logL': np.nan, 'logev': -np.inf, 'KL': np.nan,
           'log_post': np.full((S, T), np.nan) if marginals else None}
    if n == 0:
        return out
    ok = np.nonzero(~nan)[0]
    if len(ok):
        j = ok[np.argmax(logL[ok])]         # the first of the largest non-NaN values
        out['map_index'], out['map_logL'] = int(j), float(logL[j])
    if out['n_nan']:
        out['logev'] = np.nan
        return out
    top = np.max(logL)
    if top == -np.inf:
        return out
    with np.errstate(under='ignore'):
        w = np.exp(logL - top)
    ev = np.mean(w)
    out['logev'] = float(np.log(ev) + top)
    lw = np.where(w > 0, logL * np.where(w > 0, w, 1.0), 0.0)
    out['KL'] = float(np.mean(lw) / ev - out['logev'])
    if marginals:
        post = np.zeros((S, T))
        chunk = max(1, (1 << 22) // T)
        for lo in range(0, n, chunk):
            hi = min(lo + chunk, n)
            states = states_from_segments(seg_start[lo:hi], seg_state[lo:hi], T)
            for s in range(S):
                post[s] += w[lo:hi] @ (states == s)
        with np.errstate(divide='ignore'):
            out['log_post'] = np.log(post) - np.log(np.sum(post, axis=0))
    return out
