"""
NumPy statement of the exact switch counts and first-contact times under a dwell-time prior
(bild_amd.exact.exact_dwell_switch_counts, exact_dwell_first_contact) on the tables (W, F) that
`gauss_oracle.tables` returns, and the same answers from the list of every profile.  Loops over the levels, the end frames
and the states; the switch frames of one sum are one array.

With omega_s(a, b) = log_dwell[s][b - a] for b < T and log_surv[s][T - a] for b = T:

    A_0(b, s) = log_init[s] + omega_s(0, b) + F[s][b]
    A_n(b, s) = log sum_{c=n}^{b-1} e^alpha_{n-1}(c, s) e^omega_s(c, b) e^W[s][c-1][b]        n >= 1, n < b <= T
    alpha_n(c, s) = log sum_s' e^A_n(c, s') jump[s'][s]
    log_count[n][s] = A_n(T, s) - logev

    first[0] = log sum_{s in G} init_s sum_b e^omega_s(0, b) e^F[s][b] e^gamma(b, s) - logev
    first[t] = log sum_{s in G} sum_{s' not in G} e^Ax(t, s') jump[s'][s] e^beta(t, s) - logev
    never    = log sum_{s' not in G} e^Ax(T, s') - logev

Ax is the forward table under the prior that lets nothing start in G or jump into it; logev, beta and gamma are those of the
full prior.  A NaN window enters no sum; it is counted (by the full forward pass) where its prior weight is finite and a
partial profile of positive weight without a NaN window reaches its start.
"""
import numpy as np

import dwell_oracle as DO
import segment_cases as C


def _lse(terms):
    terms = np.asarray(terms, dtype=float)
    terms = terms[terms > -np.inf]
    if not len(terms):
        return -np.inf
    top = terms.max()
    return float(top + np.log(np.sum(np.exp(terms - top))))


def _omega(prior, s, c, b, T):
    """ omega_s(c, b) for an array of starts c < b """
    return prior.log_surv[s, T - c - 1] if b == T else prior.log_dwell[s, b - c - 1]


def _mix(row, jump):
    """ alpha(c, .) from A(c, .) """
    return np.array([_lse(row + jump[:, s]) for s in range(len(row))])


def forward(W, F, prior, init, jump):
    """ (A (T + 1, S), n_nan): the ordinary forward table under (init, jump) and the NaN windows it skips, as `dwell_oracle.solve` """
    S, T = F.shape[0], F.shape[1] - 1
    A = np.full((T + 1, S), -np.inf)
    al = np.full((T + 1, S), -np.inf)
    n_nan = 0
    for b in range(1, T + 1):
        for s in range(S):
            terms = []
            pr = init[s] + _omega(prior, s, 0, b, T)
            if pr > -np.inf:
                if np.isnan(F[s, b]):
                    n_nan += 1
                else:
                    terms.append(pr + F[s, b])
            c = np.arange(1, b)
            o = _omega(prior, s, c, b, T)
            w = W[s, c - 1, b]
            live = (al[c, s] > -np.inf) & (o > -np.inf)
            n_nan += int(np.sum(live & np.isnan(w)))
            use = live & ~np.isnan(w)
            terms.extend(al[c[use], s] + o[use] + w[use])
            A[b, s] = _lse(terms)
        if b < T:
            al[b] = _mix(A[b], jump)
    return A, n_nan


def backward(W, prior):
    """ (beta, gamma), each (T + 1, S), of the full prior """
    S, T = W.shape[0], W.shape[2] - 1
    G = np.full((T + 1, S), -np.inf)
    B = np.full((T + 1, S), -np.inf)
    G[T] = 0.0
    for a in range(T - 1, 0, -1):
        for s in range(S):
            b = np.arange(a + 1, T + 1)
            o = np.append(prior.log_dwell[s, :T - a - 1], prior.log_surv[s, T - a - 1])
            w = W[s, a - 1, b]
            B[a, s] = _lse((o + w + G[b, s])[~np.isnan(w)])
        G[a] = np.array([_lse(prior.log_jump[s] + B[a]) for s in range(S)])
    return B, G


def solve(W, F, prior, target=None, k_max=None, nan='propagate'):
    """
    dict: logev, n_nan_windows, log_count (k_max + 1, S), log_tail and, with a target (a collection of states), log_first (T,)
    and log_never.  k_max None: T - 1.  NaN where the NaN rule refuses and where no profile has positive weight.
    """
    S, T = F.shape[0], F.shape[1] - 1
    k_max = T - 1 if k_max is None else k_max
    init, jump = prior.log_init, prior.log_jump
    A, n_nan = forward(W, F, prior, init, jump)
    logev = _lse(A[T])
    out = {'logev': logev, 'n_nan_windows': n_nan, 'log_count': np.full((k_max + 1, S), np.nan), 'log_tail': np.nan,
           'log_first': np.full(T, np.nan), 'log_never': np.nan}
    if nan == 'propagate' and n_nan:
        out['logev'] = np.nan
        return out
    if logev == -np.inf:
        return out

    count = np.full((k_max + 1, S), -np.inf)
    al = np.full((T + 1, S), -np.inf)
    for n in range(min(k_max, T - 1) + 1):
        An = np.full((T + 1, S), -np.inf)
        for b in range(n + 1, T + 1):
            for s in range(S):
                if n == 0:
                    An[b, s] = -np.inf if np.isnan(F[s, b]) else init[s] + _omega(prior, s, 0, b, T) + F[s, b]
                else:
                    c = np.arange(n, b)
                    w = W[s, c - 1, b]
                    An[b, s] = _lse((al[c, s] + _omega(prior, s, c, b, T) + w)[~np.isnan(w)])
        count[n] = An[T] - logev
        al = np.full((T + 1, S), -np.inf)
        for c in range(1, T):
            al[c] = _mix(An[c], jump)
    out['log_count'] = count
    with np.errstate(divide='ignore'):
        out['log_tail'] = -np.inf if k_max >= T - 1 else float(np.log(max(0.0, 1.0 - np.sum(np.exp(count)))))

    if target is not None:
        inside = np.isin(np.arange(S), list(target))
        init2, jump2 = np.where(inside, -np.inf, init), np.where(inside[None, :], -np.inf, jump)
        Ax, _ = forward(W, F, prior, init2, jump2)
        B, G = backward(W, prior)
        first = np.full(T, -np.inf)
        heads = []
        for s in np.flatnonzero(inside):
            b = np.arange(1, T + 1)
            terms = np.append(prior.log_dwell[s, :T - 1], prior.log_surv[s, T - 1]) + F[s, b] + G[b, s]
            heads.append(init[s] + _lse(terms[~np.isnan(F[s, b])]))
        first[0] = _lse(heads) - logev
        for t in range(1, T):
            first[t] = _lse([Ax[t, r] + jump[r, s] + B[t, s] for r in np.flatnonzero(~inside) for s in np.flatnonzero(inside)]) - logev
        out['log_first'], out['log_never'] = first, _lse(Ax[T, ~inside]) - logev
    return out


def enumerate_all(W, F, prior, target=None, nan='propagate'):
    """
    the answers of `solve` at complete k_max from every profile of every k, weighted by exp(`DwellPrior.log_prob` +
    `segment_cases.table_logl` - logev): dict with logev, n_nan (profiles of finite prior weight whose logL is NaN: they weigh 0
    under 'omit'), log_count (T, S), log_first (T,), log_never and, for two states, segments (2, (T + 1) // 2 + 1): the probability
    that state q has j segments at [q, j]
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
    out = {'n_nan': int(bad.sum()), 'logev': np.nan, 'log_count': np.full((T, S), np.nan), 'log_first': np.full(T, np.nan),
           'log_never': np.nan, 'segments': None}
    states, joint = states[~bad], joint[~bad]
    if (nan == 'propagate' and out['n_nan']) or not np.any(joint > -np.inf):
        return out
    out['logev'] = _lse(joint)
    weight = np.exp(joint - out['logev'])
    count, first, never, segments = np.zeros((T, S)), np.zeros(T), 0.0, np.zeros((2, (T + 1) // 2 + 1))
    inside = np.isin(np.arange(S), [] if target is None else list(target))
    for row, w in zip(states, weight):
        count[np.count_nonzero(np.diff(row) != 0), row[-1]] += w
        hit = np.flatnonzero(inside[row])
        if len(hit):
            first[hit[0]] += w
        else:
            never += w
        if S == 2:
            starts = np.concatenate(([True], np.diff(row) != 0))
            for q in range(2):
                segments[q, np.count_nonzero(starts & (row == q))] += w
    with np.errstate(divide='ignore'):
        out['log_count'] = np.log(count)
        if target is not None:
            out['log_first'], out['log_never'] = np.log(first), float(np.log(never))
    out['segments'] = segments if S == 2 else None
    return out
