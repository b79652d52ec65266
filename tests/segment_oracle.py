"""
NumPy statement of the segment recursion (bild_amd.exact.exact_sample) on the tables (W, F) that
`gauss_oracle.tables` returns: W (S, T, T + 1) with W[s, a, b] the term of a later segment [a + 1, b) in state s, F (S, T + 1)
with F[s, b] the term of a first segment [0, b).  Straight loops and `logsumexp`.

A profile of k switches is F[n_0][t1_0] + sum_i W[n_i][t0_i - 1][t1_i].  Forward, j switches so far, last segment in state s
ending at b:

    A_0(b, s) = F[s][b],    A_j(b, s) = log sum_{c = j}^{b - 1} sum_{s': transitions[s', s]} exp(A_{j-1}(c, s') + W[s][c - 1][b])

Profiles that use a NaN window are left out of every sum and counted apart (exact integers); `nan='propagate'` then reports NaN
for a k that has any, `nan='omit'` divides by the count of the others.
"""
import math

import numpy as np
from scipy.special import logsumexp

from bild_amd.amis import CFC


def _lse(terms):
    terms = [t for t in terms if t > -np.inf]
    return float(logsumexp(terms)) if terms else -np.inf


def forward(W, F, transitions, k_max):
    """
    A (log sum), V (max), R (posterior mean logL of the partial profiles), ok / bad (counts of partial profiles without / with a
    NaN window, Python integers) and ptr (the (c, s') of the maximum: the first in ascending c, then ascending s'), each
    indexed [j][b][s]
    """
    S, T = F.shape[0], F.shape[1] - 1
    K = k_max + 1
    A = np.full((K, T + 1, S), -np.inf)
    V = np.full((K, T + 1, S), -np.inf)
    R = np.zeros((K, T + 1, S))
    ok = [[[0] * S for _ in range(T + 1)] for _ in range(K)]
    bad = [[[0] * S for _ in range(T + 1)] for _ in range(K)]
    ptr = [[[None] * S for _ in range(T + 1)] for _ in range(K)]
    for b in range(1, T + 1):
        for s in range(S):
            if np.isnan(F[s, b]):
                bad[0][b][s] = 1
                continue
            A[0, b, s] = V[0, b, s] = F[s, b]
            R[0, b, s] = F[s, b] if F[s, b] > -np.inf else 0.0
            ok[0][b][s] = 1
            ptr[0][b][s] = (0, -1)
    for j in range(1, K):
        for b in range(j + 1, T + 1):
            for s in range(S):
                terms, rs = [], []
                for c in range(j, b):
                    w = W[s, c - 1, b]
                    for q in range(S):
                        if not transitions[q, s]:
                            continue
                        if np.isnan(w):
                            bad[j][b][s] += ok[j - 1][c][q] + bad[j - 1][c][q]
                            continue
                        ok[j][b][s] += ok[j - 1][c][q]
                        bad[j][b][s] += bad[j - 1][c][q]
                        if ok[j - 1][c][q] == 0:
                            continue
                        t = V[j - 1, c, q] + w
                        if ptr[j][b][s] is None or t > V[j, b, s]:
                            V[j, b, s] = t
                            ptr[j][b][s] = (c, q)
                        if A[j - 1, c, q] + w > -np.inf:
                            terms.append(A[j - 1, c, q] + w)
                            rs.append(R[j - 1, c, q] + w)
                A[j, b, s] = _lse(terms)
                if terms:
                    p = np.exp(np.array(terms) - A[j, b, s])
                    R[j, b, s] = float(np.sum(p * np.array(rs)))
    return A, V, R, ok, bad, ptr


def backward(W, transitions, k_max):
    """ G[m][b][s]: log sum over the completions, m switches to come, of a profile whose segment in state s ends at b """
    S, T = W.shape[0], W.shape[1]
    K = k_max + 1
    G = np.full((K, T + 1, S), -np.inf)
    G[0, T, :] = 0.0
    for m in range(1, K):
        for b in range(1, T):
            for s in range(S):
                terms = []
                for q in range(S):
                    if not transitions[s, q]:
                        continue
                    for e in range(b + 1, T + 1):
                        w = W[q, b - 1, e]
                        if not np.isnan(w):
                            terms.append(w + G[m - 1, e, q])
                G[m, b, s] = _lse(terms)
    return G


def marginals(W, F, transitions, A, G, k):
    """ (S, T) unnormalised log weight of state s at frame t over the profiles of k switches (NaN windows left out) """
    S, T = F.shape[0], F.shape[1] - 1
    post = np.full((S, T), -np.inf)
    for s in range(S):
        # logQ[a, b]: all profiles of k switches with a segment [a, b) in state s
        logQ = np.full((T, T + 1), -np.inf)
        for b in range(1, T + 1):
            if not np.isnan(F[s, b]):
                logQ[0, b] = F[s, b] + G[k, b, s]
        for a in range(1, T):
            for b in range(a + 1, T + 1):
                w = W[s, a - 1, b]
                if np.isnan(w):
                    continue
                terms = [A[j - 1, a, q] + w + G[k - j, b, s] for j in range(1, k + 1) for q in range(S) if transitions[q, s]]
                logQ[a, b] = _lse(terms)
        for t in range(T):
            post[s, t] = _lse(logQ[:t + 1, t + 1:].ravel())
    return post


def solve(W, F, transitions, k_max, nan='propagate', with_marginals=True):
    """
    dict of lists / arrays over k = 0 ... k_max: logev, KL, map_logL, map_states (expanded profile or None), n_profiles,
    n_omitted (Python integers), log_post ((S, T) normalised, NaN where undefined)
    """
    transitions = np.asarray(transitions, dtype=bool)
    S, T = F.shape[0], F.shape[1] - 1
    K = k_max + 1
    A, V, R, ok, bad, ptr = forward(W, F, transitions, k_max)
    G = backward(W, transitions, k_max) if with_marginals else None
    cfc = CFC(transitions)
    out = {'logev': np.full(K, -np.inf), 'KL': np.full(K, np.nan), 'map_logL': np.full(K, np.nan), 'map_states': [None] * K,
           'n_profiles': [0] * K, 'n_omitted': [0] * K, 'log_post': np.full((K, S, T), np.nan)}
    for k in range(K):
        n_all = math.comb(T - 1, k) * int(cfc.N_total(k)) if k <= T - 1 else 0
        n_ok, n_bad = sum(ok[k][T]), sum(bad[k][T])
        assert n_ok + n_bad == n_all
        if n_all == 0:
            continue
        # MAP: the smallest final state of the largest value, then back along the pointers
        cand = [s for s in range(S) if ptr[k][T][s] is not None]
        if cand:
            s = max(cand, key=lambda q: (V[k, T, q], -q))
            out['map_logL'][k] = V[k, T, s]
            states = np.empty(T, dtype=int)
            b = T
            for j in range(k, -1, -1):
                c, q = ptr[j][b][s]
                states[c:b] = s
                b, s = c, q
            out['map_states'][k] = states
        if nan == 'propagate':
            out['n_profiles'][k] = n_all
            if n_bad:
                out['logev'][k] = np.nan
                continue
            count = n_all
        else:
            out['n_profiles'][k], out['n_omitted'][k] = n_ok, n_bad
            count = n_ok
        tot = _lse(list(A[k, T]))
        if count == 0 or tot == -np.inf:
            continue
        out['logev'][k] = tot - math.log(count)
        p = np.exp(A[k, T] - tot)
        out['KL'][k] = float(np.sum(np.where(p > 0, p * R[k, T], 0.0))) - out['logev'][k]
        if with_marginals:
            post = marginals(W, F, transitions, A, G, k)
            with np.errstate(divide='ignore'):
                out['log_post'][k] = post - logsumexp(post, axis=0)
    return out


# --------------------------------------------------------------------------------------------------------- fast twin
# The same definitions, vectorised over the switch frame c and the end frame b of a level.  `solve` above is the statement;
# tests/test_segment_wide.py holds `solve_fast` to it on every output.  The sums run in another order than the loops', so the
# two agree to rounding, not bit for bit; the counts are exact (object arrays of Python integers) and the pointers follow the
# loops' tie rule.  `dtype=np.longdouble` runs every sum in extended precision: the oracle's own noise is the difference.

def _lse_over(x, axis):
    """ log sum exp over `axis` in the array's own precision; -inf where every term is """
    m = np.max(x, axis=axis, keepdims=True)
    m = np.where(m > -np.inf, m, 0)
    with np.errstate(divide='ignore', under='ignore'):
        return np.squeeze(np.log(np.sum(np.exp(x - m), axis=axis, keepdims=True)) + m, axis=axis)


def forward_fast(W, F, transitions, k_max):
    """
    `forward` as arrays indexed [j, b, s]: A, V, R in the dtype of W, ok / bad as object arrays of Python integers, and the
    pointer (ptr_c, ptr_q), ptr_c = -1 where `forward` has None
    """
    S, T = F.shape[0], F.shape[1] - 1
    K = k_max + 1
    A = np.full((K, T + 1, S), -np.inf, dtype=W.dtype)
    V = np.full((K, T + 1, S), -np.inf, dtype=W.dtype)
    R = np.zeros((K, T + 1, S), dtype=W.dtype)
    ok = np.zeros((K, T + 1, S), dtype=object)
    bad = np.zeros((K, T + 1, S), dtype=object)
    ptr_c = np.full((K, T + 1, S), -1, dtype=np.int64)
    ptr_q = np.full((K, T + 1, S), -1, dtype=np.int64)
    nanF = np.isnan(F[:, 1:]).T                     # (b - 1, s)
    A[0, 1:] = V[0, 1:] = np.where(nanF, -np.inf, F[:, 1:].T)
    R[0, 1:] = np.where(nanF | (F[:, 1:].T == -np.inf), 0.0, F[:, 1:].T)
    ok[0, 1:] = (~nanF).astype(int).astype(object)
    bad[0, 1:] = nanF.astype(int).astype(object)
    ptr_c[0, 1:] = np.where(nanF, -1, 0)
    cs, bs = np.arange(1, T), np.arange(T + 1)
    for j in range(1, min(K, T)):       # (level j needs j + 1 <= T)
        valid = (cs[:, None] >= j) & (cs[:, None] < bs[None, :])        # (c, b)
        for s in range(S):
            preds = np.nonzero(transitions[:, s])[0]
            if not len(preds):
                continue
            P = len(preds)
            w = W[s, :T - 1, :]                      # row c - 1 for c = 1 ... T - 1
            nanw = valid & np.isnan(w)
            good = valid & ~nanw
            ok_p, bad_p = ok[j - 1, 1:T][:, preds], bad[j - 1, 1:T][:, preds]      # (c, p)
            okq, badq = ok_p.sum(axis=1), bad_p.sum(axis=1)
            ok[j, :, s] = np.dot(okq, good.astype(int).astype(object))
            bad[j, :, s] = np.dot(badq, valid.astype(int).astype(object)) + np.dot(okq, nanw.astype(int).astype(object))
            w3 = np.where(good, w, -np.inf)[:, None, :]                             # (c, 1, b)
            # the maximum: the first in ascending c, then ascending s', among the predecessors that hold a profile
            cand = (good[:, None, :] & (ok_p > 0).astype(bool)[:, :, None]).reshape((T - 1) * P, T + 1)
            tv = np.where(cand, (V[j - 1, 1:T][:, preds][:, :, None] + w3).reshape((T - 1) * P, T + 1), -np.inf)
            top = np.max(tv, axis=0)
            at = np.where(top > -np.inf, np.argmax(tv, axis=0), np.argmax(cand, axis=0))
            some = cand.any(axis=0)
            V[j, :, s] = np.where(some, top, -np.inf)
            ptr_c[j, :, s] = np.where(some, cs[at // P], -1)
            ptr_q[j, :, s] = np.where(some, preds[at % P], -1)
            terms = A[j - 1, 1:T][:, preds][:, :, None] + w3                        # (c, p, b)
            A[j, :, s] = _lse_over(terms, (0, 1))
            live = terms > -np.inf
            with np.errstate(invalid='ignore', under='ignore'):
                p = np.where(live, np.exp(terms - np.where(A[j, :, s] > -np.inf, A[j, :, s], 0)), 0.0)
                rs = np.where(live, R[j - 1, 1:T][:, preds][:, :, None] + w3, 0.0)
            R[j, :, s] = np.sum(p * rs, axis=(0, 1))
    return A, V, R, ok, bad, ptr_c, ptr_q


def backward_fast(W, transitions, k_max):
    """ `backward` in the dtype of W """
    S, T = W.shape[0], W.shape[1]
    K = k_max + 1
    G = np.full((K, T + 1, S), -np.inf, dtype=W.dtype)
    G[0, T, :] = 0.0
    later = np.arange(T + 1)[None, :] > np.arange(1, T)[:, None]           # (b, e): e > b
    for m in range(1, K):
        if T < 2:
            break
        for s in range(S):
            succ = np.nonzero(transitions[s])[0]
            if not len(succ):
                continue
            w = W[succ][:, :T - 1, :]               # (q, b - 1, e)
            terms = np.where(later[None] & ~np.isnan(w), w + G[m - 1][:, succ].T[:, None, :], -np.inf)
            G[m, 1:T, s] = _lse_over(terms, (0, 2))
    return G


def marginals_fast(W, F, transitions, A, G, k):
    """ `marginals` in the dtype of W """
    S, T = F.shape[0], F.shape[1] - 1
    post = np.full((S, T), -np.inf, dtype=W.dtype)
    a_, b_ = np.arange(1, T), np.arange(T + 1)
    for s in range(S):
        logQ = np.full((T, T + 1), -np.inf, dtype=W.dtype)
        logQ[0, 1:] = np.where(np.isnan(F[s, 1:]), -np.inf, F[s, 1:] + G[k, 1:, s])
        preds = np.nonzero(transitions[:, s])[0]
        if k >= 1 and T >= 2 and len(preds):
            w = W[s, :T - 1, :]
            a_in = _lse_over(A[:k, 1:T][:, :, preds], 2)         # [j - 1, a]: over the states before
            g_out = G[k - 1::-1, :, s]                          # [j - 1, b] = G[k - j, b, s]
            both = _lse_over(a_in[:, :, None] + g_out[:, None, :], 0)
            logQ[1:] = np.where((a_[:, None] < b_[None, :]) & ~np.isnan(w), both + w, -np.inf)
        # post[t] = log sum over a <= t < b: the tail sums over b by a running logaddexp, then the column over a
        tail = np.logaddexp.accumulate(logQ[:, ::-1], axis=1)[:, ::-1][:, 1:]       # [a, t] = lse over b > t
        post[s] = _lse_over(np.where(np.arange(T)[:, None] <= np.arange(T)[None, :], tail, -np.inf), 0)
    return post


def solve_fast(W, F, transitions, k_max, nan='propagate', with_marginals=True, dtype=np.float64, kept=None):
    """ `solve` by the vectorised recursions: the same dictionary, its arrays in `dtype`; a dict `kept` receives the tables """
    transitions = np.asarray(transitions, dtype=bool)
    W, F = np.asarray(W, dtype=dtype), np.asarray(F, dtype=dtype)
    S, T = F.shape[0], F.shape[1] - 1
    K = k_max + 1
    A, V, R, ok, bad, ptr_c, ptr_q = forward_fast(W, F, transitions, k_max)
    G = backward_fast(W, transitions, k_max) if with_marginals else None
    if kept is not None:
        kept.update(A=A, V=V, R=R, ok=ok, bad=bad, ptr_c=ptr_c, ptr_q=ptr_q, G=G)
    cfc = CFC(transitions)
    out = {'logev': np.full(K, -np.inf, dtype=dtype), 'KL': np.full(K, np.nan, dtype=dtype), 'map_logL': np.full(K, np.nan, dtype=dtype),
           'map_states': [None] * K, 'n_profiles': [0] * K, 'n_omitted': [0] * K, 'log_post': np.full((K, S, T), np.nan, dtype=dtype)}
    for k in range(K):
        n_all = math.comb(T - 1, k) * int(cfc.N_total(k)) if k <= T - 1 else 0
        n_ok, n_bad = int(sum(ok[k, T])), int(sum(bad[k, T]))
        assert n_ok + n_bad == n_all
        if n_all == 0:
            continue
        cand = [s for s in range(S) if ptr_c[k, T, s] >= 0]
        if cand:
            s = max(cand, key=lambda q: (V[k, T, q], -q))
            out['map_logL'][k] = V[k, T, s]
            states = np.empty(T, dtype=int)
            b = T
            for j in range(k, -1, -1):
                c, q = int(ptr_c[j, b, s]), int(ptr_q[j, b, s])
                states[c:b] = s
                b, s = c, q
            out['map_states'][k] = states
        if nan == 'propagate':
            out['n_profiles'][k] = n_all
            if n_bad:
                out['logev'][k] = np.nan
                continue
            count = n_all
        else:
            out['n_profiles'][k], out['n_omitted'][k] = n_ok, n_bad
            count = n_ok
        tot = _lse_over(A[k, T], 0)
        if count == 0 or tot == -np.inf:
            continue
        out['logev'][k] = tot - np.log(dtype(count))
        p = np.exp(A[k, T] - tot)
        out['KL'][k] = np.sum(np.where(p > 0, p * R[k, T], 0.0)) - out['logev'][k]
        if with_marginals:
            post = marginals_fast(W, F, transitions, A, G, k)
            with np.errstate(divide='ignore', invalid='ignore'):
                out['log_post'][k] = post - _lse_over(post, 0)
    return out
