"""
NumPy statement of the exact posterior draws under a dwell-time prior (bild_amd.exact.exact_dwell_draw)
on the tables (W, F) of `gauss_oracle.tables`, with its own backward tables.  Straight loops.

With omega_s(a, b) = log_dwell[s][b - a] for b < T and log_surv[s][T - a] for b = T, all tables in logs:

    gamma(T, s) = 0,  beta(a, s) = log sum_{b>a} exp(omega_s(a, b) + W[s][a-1][b] + gamma(b, s)),
    gamma(b, s) = log sum_q exp(log_jump[s][q] + beta(b, q))

A draw consumes a row u of uniforms.  u[0] picks (s_0, t_1) jointly over the list ordered by state, then by b = 1 ... T, with
log weight log_init[s] + omega_s(0, b) + F[s, b] + gamma(b, s).  For i = 1, 2, ..., starting at t_i < T: u[2i - 1] picks s_i among
q = 0 ... S - 1 with log weight log_jump[s_{i-1}][q] + beta(t_i, q), and u[2i] picks t_{i+1} among b = t_i + 1 ... T with log weight
omega_{s_i}(t_i, b) + W[s_i, t_i - 1, b] + gamma(b, s_i).  The draw ends when a pick returns b = T: k switches consume 1 + 2k
uniforms.  The pick and its *fragile* flag are `segment_draw_oracle.pick`, DELTA = 1e-9 for the reason that file gives: here
as there a device weight differs from the oracle's by the rounding of an exponent of size <~ 1e4 and of a sum of up to
2048 terms.
"""
import numpy as np
from scipy.special import logsumexp

import dwell_oracle as DO
import segment_cases as C
from segment_draw_oracle import DELTA, pick


def _lse(terms):
    terms = [t for t in terms if not np.isnan(t) and t > -np.inf]
    return float(logsumexp(terms)) if terms else -np.inf


def omega(prior, s, a, b, T):
    return prior.log_surv[s, T - a - 1] if b == T else prior.log_dwell[s, b - a - 1]


def backward(W, F, prior):
    """ (beta, gamma), each (T + 1, S); rows 1 ... T - 1 of beta and 1 ... T of gamma are defined, the rest is -inf """
    S, T = F.shape[0], F.shape[1] - 1
    B = np.full((T + 1, S), -np.inf)
    G = np.full((T + 1, S), -np.inf)
    G[T] = 0.0
    for a in range(T - 1, 0, -1):
        for s in range(S):
            B[a, s] = _lse([omega(prior, s, a, b, T) + W[s, a - 1, b] + G[b, s] for b in range(a + 1, T + 1)])
        for s in range(S):
            G[a, s] = _lse([prior.log_jump[s, q] + B[a, q] for q in range(S)])
    return B, G


class Lists:
    """ the log weights of every list of a trajectory: they belong to the tables, not to a draw """

    def __init__(self, W, F, prior):
        self.W, self.F, self.prior = W, F, prior
        self.S, self.T = F.shape[0], F.shape[1] - 1
        self.B, self.G = backward(W, F, prior)
        S, T = self.S, self.T
        self.head = np.array([prior.log_init[s] + omega(prior, s, 0, b, T) + F[s, b] + self.G[b, s]
                              for s in range(S) for b in range(1, T + 1)])
        self._ends = {}

    def states(self, s, t):
        return self.prior.log_jump[s] + self.B[t]

    def ends(self, s, t):
        if (s, t) not in self._ends:
            T = self.T
            self._ends[s, t] = np.array([omega(self.prior, s, t, b, T) + self.W[s, t - 1, b] + self.G[b, s] for b in range(t + 1, T + 1)])
        return self._ends[s, t]


def draw(lists, u, delta=DELTA):
    """
    One draw from the row u of uniforms: (states (T,), k, logl, log_prior, fragile, used).  states is None without a profile
    of positive weight (used = 0) and where the row is too short (used = -1).
    """
    S, T, prior, W, F = lists.S, lists.T, lists.prior, lists.W, lists.F
    if len(u) < 1:
        return None, -1, np.nan, np.nan, False, -1
    j, fragile = pick(lists.head, u[0], delta)
    if j < 0:
        return None, -1, np.nan, np.nan, False, 0
    used = 1
    s, t, b = j // T, 0, j % T + 1
    states = np.empty(T, dtype=np.uint8)
    states[:b] = s
    logl = 0.0 + F[s, b]
    lp = prior.log_init[s]
    k = 0
    while b < T:
        lp = lp + prior.log_dwell[s, b - t - 1]
        t = b
        if used + 2 > len(u):
            return None, -1, np.nan, np.nan, fragile, -1
        q, f = pick(lists.states(s, t), u[used], delta)
        assert q >= 0       # the pick before had positive weight: a completion exists
        fragile |= f
        lp = lp + prior.log_jump[s, q]
        s = q
        k += 1
        j, f = pick(lists.ends(s, t), u[used + 1], delta)
        assert j >= 0
        fragile |= f
        used += 2
        b = t + 1 + j
        logl += W[s, t - 1, b]
        states[t:b] = s
    lp = lp + prior.log_surv[s, T - t - 1]
    return states, k, logl, lp, fragile, used


def draws(W, F, prior, uniforms, delta=DELTA):
    """
    The draws of a batch in the device's layout: dict of states (n, T) uint8 (a row of 255 without a profile), n_switches (-1),
    logl, log_prior (NaN), n_uniforms (0 without a profile of positive weight, -1 where the row was too short), fragile (n,)
    """
    lists = Lists(W, F, prior)
    n, T = len(uniforms), lists.T
    out = {'states': np.full((n, T), 255, dtype=np.uint8), 'n_switches': np.full(n, -1, dtype=np.int64), 'logl': np.full(n, np.nan),
           'log_prior': np.full(n, np.nan), 'n_uniforms': np.zeros(n, dtype=np.int64), 'fragile': np.zeros(n, dtype=bool)}
    for r in range(n):
        states, k, logl, lp, out['fragile'][r], out['n_uniforms'][r] = draw(lists, uniforms[r], delta)
        if states is not None:
            out['states'][r], out['n_switches'][r], out['logl'][r], out['log_prior'][r] = states, k, logl, lp
    return out


def profile_posterior(W, F, prior):
    """
    (states (n, T), log joint (n,), p (n,), bad (n,)) of every profile of every k, from the profiles and the log joints that
    `dwell_oracle.enumerate_all` sums: p is the posterior under nan='omit' (0 for a profile with a NaN window or of prior
    weight 0), bad marks the profiles whose log-likelihood is NaN
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
    live = np.where(bad, -np.inf, joint)
    with np.errstate(under='ignore'):
        p = np.exp(live - logsumexp(live))
    return states, joint, p, bad
