"""
NumPy statement of the exact window support under a dwell-time prior (bild_amd.exact.exact_dwell_windows, DESIGN.md section
29) on the tables (W, F) that `gauss_oracle.tables` returns, in two formulations, and the same answer from the list of every
profile.  A window is (u, v, target): 0 <= u < v <= T and a collection of states G.

With omega_s(a, b) = log_dwell[s][b - a] for b < T and log_surv[s][T - a] for b = T, head(0, s) = log_init[s] and head(a, s) =
alpha(a, s), w(0, b, s) = F[s][b] and w(a, b, s) = W[s][a - 1][b], seg(a, b, s) = omega_s(a, b) + w(a, b, s):

    C(b, s)     = log[ sum_{a=0}^{u} e^head(a, s) e^seg(a, b, s) + sum_{c=u+1}^{b-1} e^kappa(c, s) e^seg(c, b, s) ]    u < b < v, s in G
    kappa(c, s) = log sum_{s' in G} e^C(c, s') jump[s'][s]                                                   u < c < v, s in G
    num         = log sum_{s in G} sum_{b=v}^{T} [ sum_{a<=u} e^head(a, s) e^seg(a, b, s) e^gamma(b, s)
                                                   + sum_{u<c<v} e^kappa(c, s) e^seg(c, b, s) e^gamma(b, s) ]
    log_all     = num - logev

`solve` is this split formulation: per state one matrix of terms, row = start frame, filled row after row, each row for all its
end frames at once.  `solve_masked` is the full forward pass that drops every segment (c, b, s) with s outside G that touches
the window (c < v and b > u).  logev, alpha, gamma and the count of NaN windows are those of the ordinary passes
(`dwell_event_oracle.forward`, `.backward`).  A NaN window enters no sum.
"""
import numpy as np

import dwell_event_oracle as DE
import dwell_oracle as DO
import segment_cases as C


def _lse(a, axis=None):
    """ log sum exp of an array along an axis; -inf where nothing is finite """
    a = np.asarray(a, dtype=float)
    top = np.max(a, axis=axis, keepdims=True, initial=-np.inf)
    safe = np.where(top > -np.inf, top, 0.0)
    with np.errstate(divide='ignore'):
        out = safe + np.log(np.sum(np.exp(a - safe), axis=axis, keepdims=True))
    out = np.where(top > -np.inf, out, -np.inf)
    return float(out.reshape(())) if axis is None else np.squeeze(out, axis=axis)


def _seg_row(W, F, prior, s, c, T):
    """ seg(c, b, s) for b = c + 1 .. T; -inf where the table entry is NaN """
    om = np.append(prior.log_dwell[s, :T - c - 1], prior.log_surv[s, T - c - 1])
    w = F[s, c + 1:] if c == 0 else W[s, c - 1, c + 1:]
    with np.errstate(invalid='ignore'):
        return np.where(np.isnan(w), -np.inf, om + w)


def _start(W, F, prior, nan, n):
    """ what every formulation shares: (out, A, logev, usable) """
    T = F.shape[1] - 1
    A, n_nan = DE.forward(W, F, prior, prior.log_init, prior.log_jump)
    logev = DE._lse(A[T])
    out = {'logev': logev, 'n_nan_windows': n_nan, 'log_all': np.full(n, np.nan)}
    if nan == 'propagate' and n_nan:
        out['logev'] = np.nan
        return out, A, logev, False
    return out, A, logev, logev > -np.inf


def solve(W, F, prior, windows, nan='propagate'):
    """
    dict: logev, n_nan_windows, log_all (n,) for the windows (u, v, target).  NaN where the NaN rule refuses and where no
    profile has positive weight.
    """
    S, T = F.shape[0], F.shape[1] - 1
    init, jump = prior.log_init, prior.log_jump
    out, A, logev, usable = _start(W, F, prior, nan, len(windows))
    if not usable:
        return out
    al = np.full((T + 1, S), -np.inf)
    for c in range(1, T):
        al[c] = DE._mix(A[c], jump)
    _, gamma = DE.backward(W, prior)
    for i, (u, v, target) in enumerate(windows):
        G = sorted(target)
        M = {s: np.full((v, T + 1), -np.inf) for s in G}       # M[s][c, b] = head(c, s) + seg(c, b, s)
        for c in range(v):
            if c == 0:
                head = {s: init[s] for s in G}
            elif c <= u:
                head = {s: al[c, s] for s in G}
            else:
                Cc = {s: _lse(M[s][:c, c]) for s in G}
                head = {s: DE._lse([Cc[r] + jump[r, s] for r in G]) for s in G}
            for s in G:
                if head[s] > -np.inf:
                    M[s][c, c + 1:] = head[s] + _seg_row(W, F, prior, s, c, T)
        out['log_all'][i] = DE._lse(np.concatenate([(M[s][:, v:] + gamma[v:, s]).ravel() for s in G])) - logev
    return out


def solve_masked(W, F, prior, windows, nan='propagate'):
    """ the answer of `solve` from one full forward pass a window, without the segments outside G that touch the window """
    S, T = F.shape[0], F.shape[1] - 1
    init, jump = prior.log_init, prior.log_jump
    out, _, logev, usable = _start(W, F, prior, nan, len(windows))
    if not usable:
        return out
    for i, (u, v, target) in enumerate(windows):
        inside = np.isin(np.arange(S), list(target))
        A = np.full((T + 1, S), -np.inf)
        al = np.full((T + 1, S), -np.inf)
        for b in range(1, T + 1):
            for s in range(S):
                c = np.arange(0, b)
                head = np.append(init[s], al[1:b, s])
                seg = np.array([_seg_row(W, F, prior, s, a, T)[b - a - 1] for a in c])
                keep = np.ones(b, dtype=bool) if inside[s] else ~((c < v) & (b > u))
                A[b, s] = DE._lse((head + seg)[keep & (head > -np.inf)])
            if b < T:
                al[b] = DE._mix(A[b], jump)
        out['log_all'][i] = DE._lse(A[T]) - logev
    return out


def enumerate_all(W, F, prior, windows, nan='propagate'):
    """
    the answer of `solve` from every profile of every k, weighted by exp(`DwellPrior.log_prob` + `segment_cases.table_logl` -
    logev): dict with logev, n_nan (profiles of finite prior weight whose logL is NaN: they weigh 0 under 'omit') and log_all
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
    out = {'n_nan': int(bad.sum()), 'logev': np.nan, 'log_all': np.full(len(windows), np.nan)}
    states, joint = states[~bad], joint[~bad]
    if (nan == 'propagate' and out['n_nan']) or not np.any(joint > -np.inf):
        return out
    out['logev'] = DE._lse(joint)
    for i, (u, v, target) in enumerate(windows):
        hit = np.isin(states[:, u:v], list(target)).all(axis=1)
        out['log_all'][i] = DE._lse(joint[hit]) - out['logev']
    return out
