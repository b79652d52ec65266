"""
NumPy statement of the dwell-time recursion (bild_amd.exact.exact_dwell) on the tables (W, F) that
`gauss_oracle.tables` returns, and the same answers by enumeration of every profile.  Straight loops and `logsumexp`.

With omega_s(a, b) = log_dwell[s][b - a] for b < T and log_surv[s][T - a] for b = T:

    A(b, s) = log( init_s e^omega_s(0, b) e^F[s][b] + sum_{c=1}^{b-1} e^alpha(c, s) e^omega_s(c, b) e^W[s][c-1][b] )
    alpha(c, s) = log sum_s' e^A(c, s') jump[s'][s],    evidence = sum_s e^A(T, s)
    gamma(T, s) = 0,  beta(a, s) = log sum_{b>a} e^omega_s(a, b) e^W[s][a-1][b] e^gamma(b, s),
    gamma(b, s) = log sum_s'' jump[s][s''] e^beta(b, s'')
    Q(a, b, s) = e^alpha(a, s) e^omega e^W e^gamma(b, s) / evidence

A NaN window never enters a sum or a maximum; it is counted where its prior weight is finite and a partial profile of
finite prior weight without a NaN window reaches its start.
"""
import numpy as np
from scipy.special import logsumexp

import exact_oracle as X
import segment_cases as C
from bild_amd.profiles import states_from_segments


def _lse(terms):
    terms = [t for t in terms if t > -np.inf]
    return float(logsumexp(terms)) if terms else -np.inf


def solve(W, F, prior, nan='propagate'):
    """
    dict: logev, map_logjoint, map_states (expanded profile or None), n_nan_windows, log_post (S, T), exp_jumps (S, S),
    exp_stay (S,); under nan='propagate' with n_nan_windows > 0 the evidence, the marginals and the counts are NaN
    """
    S, T = F.shape[0], F.shape[1] - 1
    init, jump = prior.log_init, prior.log_jump

    def om(s, a, b):
        return prior.log_surv[s, T - a - 1] if b == T else prior.log_dwell[s, b - a - 1]

    A = np.full((T + 1, S), -np.inf)
    V = np.full((T + 1, S), -np.inf)
    ptr = [[None] * S for _ in range(T + 1)]        # the start c of the last segment
    al = np.full((T + 1, S), -np.inf)
    alV = np.full((T + 1, S), -np.inf)
    alptr = [[None] * S for _ in range(T + 1)]      # the preceding state
    n_nan = 0
    for b in range(1, T + 1):
        for s in range(S):
            terms = []
            pr = init[s] + om(s, 0, b)
            if pr > -np.inf:
                if np.isnan(F[s, b]):
                    n_nan += 1
                else:
                    terms.append(pr + F[s, b])
                    V[b, s], ptr[b][s] = pr + F[s, b], 0
            for c in range(1, b):
                if alptr[c][s] is None:
                    continue
                o = om(s, c, b)
                if o == -np.inf:
                    continue
                w = W[s, c - 1, b]
                if np.isnan(w):
                    n_nan += 1
                    continue
                terms.append(al[c, s] + o + w)
                tv = alV[c, s] + o + w
                if ptr[b][s] is None or tv > V[b, s]:
                    V[b, s], ptr[b][s] = tv, c
            A[b, s] = _lse(terms)
        if b == T:
            break
        for s in range(S):
            al[b, s] = _lse([A[b, q] + jump[q, s] for q in range(S)])
            for q in range(S):
                if ptr[b][q] is None or jump[q, s] == -np.inf:
                    continue
                tv = V[b, q] + jump[q, s]
                if alptr[b][s] is None or tv > alV[b, s]:
                    alV[b, s], alptr[b][s] = tv, q

    out = {'logev': _lse(list(A[T])), 'map_logjoint': np.nan, 'map_states': None, 'n_nan_windows': n_nan,
           'log_post': np.full((S, T), np.nan), 'exp_jumps': np.full((S, S), np.nan), 'exp_stay': np.full(S, np.nan)}
    cand = [s for s in range(S) if ptr[T][s] is not None]
    if cand:
        s = max(cand, key=lambda q: (V[T, q], -q))
        out['map_logjoint'] = V[T, s]
        states = np.empty(T, dtype=int)
        b = T
        while True:
            c = ptr[b][s]
            states[c:b] = s
            if c == 0:
                break
            b, s = c, alptr[c][s]
        out['map_states'] = states
    logev = out['logev']
    if nan == 'propagate' and n_nan:
        out['logev'] = np.nan
        return out
    if logev == -np.inf:
        return out

    G = np.full((T + 1, S), -np.inf)
    B = np.full((T + 1, S), -np.inf)
    G[T] = 0.0
    for a in range(T - 1, 0, -1):
        for s in range(S):
            terms = []
            for b in range(a + 1, T + 1):
                w = W[s, a - 1, b]
                if not np.isnan(w):
                    terms.append(om(s, a, b) + w + G[b, s])
            B[a, s] = _lse(terms)
        for s in range(S):
            G[a, s] = _lse([jump[s, q] + B[a, q] for q in range(S)])

    post = np.zeros((S, T))
    stay = np.zeros(S)
    for s in range(S):
        Q = np.zeros((T, T + 1))
        for b in range(1, T + 1):
            if not np.isnan(F[s, b]):
                Q[0, b] = np.exp(init[s] + om(s, 0, b) + F[s, b] + G[b, s] - logev)
            for a in range(1, b):
                w = W[s, a - 1, b]
                if not np.isnan(w):
                    Q[a, b] = np.exp(al[a, s] + om(s, a, b) + w + G[b, s] - logev)
        for t in range(T):
            post[s, t] = np.sum(Q[:t + 1, t + 1:])
        length = np.arange(T + 1)[None, :] - np.arange(T)[:, None]
        stay[s] = np.sum(Q * np.maximum(length - 1, 0))
    jumps = np.zeros((S, S))
    for q in range(S):
        for s in range(S):
            if jump[q, s] > -np.inf:
                jumps[q, s] = sum(np.exp(A[c, q] + jump[q, s] + B[c, s] - logev) for c in range(1, T))
    with np.errstate(divide='ignore'):
        out['log_post'] = np.log(post)
    out['exp_jumps'], out['exp_stay'] = jumps, stay
    return out


def all_profiles(T, S):
    """ (states (n, T), seg_start, seg_state lists per k) of every profile of every k = 0 ... T - 1, no jump forbidden """
    full = ~np.eye(S, dtype=bool)
    rows = []
    for k in range(T):
        if S == 1 and k > 0:
            break
        seg_start, seg_state = X.enumerate_profiles(T, k, full)
        if len(seg_start):
            rows.append((k, seg_start, seg_state, states_from_segments(seg_start, seg_state, T)))
    return rows


def enumerate_all(W, F, prior, nan='propagate'):
    """
    the answers of `solve` from the log joint of every profile: dict with logev, map_logjoint, map_states, n_max (profiles
    within 1e-9 of the maximum), log_post, exp_jumps, exp_stay, and n_nan (profiles of finite prior weight whose logL is NaN)
    """
    S, T = F.shape[0], F.shape[1] - 1
    states, joint = [], []
    for k, seg_start, seg_state, st in all_profiles(T, S):
        logl = C.table_logl(W, F, seg_start, seg_state, T)
        prior_lp = np.array([prior.log_prob(row) for row in st])
        states.append(st)
        with np.errstate(invalid='ignore'):
            joint.append(np.where(prior_lp == -np.inf, -np.inf, prior_lp + logl))   # (a profile the prior excludes weighs 0)
    states, joint = np.concatenate(states), np.concatenate(joint)
    bad = np.isnan(joint)
    out = {'n_nan': int(bad.sum()), 'logev': np.nan, 'log_post': np.full((S, T), np.nan), 'exp_jumps': np.full((S, S), np.nan),
           'exp_stay': np.full(S, np.nan), 'map_logjoint': np.nan, 'map_states': None, 'n_max': 0}
    states, joint = states[~bad], joint[~bad]
    live = joint > -np.inf
    if live.any():
        top = np.max(joint)
        out['map_logjoint'], out['n_max'] = top, int(np.sum(joint >= top - 1e-9))
        out['map_states'] = states[np.argmax(joint)]
    if (nan == 'propagate' and out['n_nan']) or not live.any():
        return out
    out['logev'] = float(logsumexp(joint))
    w = np.exp(joint - out['logev'])
    post = np.array([w @ (states == s) for s in range(S)])
    with np.errstate(divide='ignore'):
        out['log_post'] = np.log(post)
    for q in range(S):
        out['exp_stay'][q] = w @ np.sum((states[:, :-1] == q) & (states[:, 1:] == q), axis=1)
        for s in range(S):
            out['exp_jumps'][q, s] = 0.0 if q == s else w @ np.sum((states[:, :-1] == q) & (states[:, 1:] == s), axis=1)
    return out
