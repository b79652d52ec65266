"""
NumPy statement of the exact posterior draws (bild_amd.exact.exact_draw) on the tables (W, F) of
`gauss_oracle.tables` and the backward table G of `segment_oracle.backward`.  Straight loops.

A draw of k switches consumes a row u of uniforms.  u[0] picks (s_0, t_1) jointly over the list ordered by state, then by
b = 1 ... T, with weight exp(F[s, b] + G[k, b, s]).  For i = 1 ... k and m = k - i, u[2i - 1] picks s_i among the allowed q in
ascending order with weight beta_m(t_i, q) = sum_{b > t_i} exp(W[q, t_i - 1, b] + G[m, b, q]), and, for i < k, u[2i] picks
t_{i+1} among b = t_i + 1 ... T with weight exp(W[s_i, t_i - 1, b] + G[m, b, s_i]); the last segment ends at T.  A pick returns
the smallest index of positive weight whose inclusive cumulative weight exceeds u times the total, and the last index of
positive weight when rounding carries that product past it.  NaN and -inf terms weigh 0.

A draw is *fragile* when one of its uniforms lies within DELTA = 1e-9 of an interior boundary of the normalised CDF it is
applied to: an implementation that sums in another order may then pick the neighbour.  A device weight differs from the
oracle's by the rounding of an exponent of size <~ 1e4 (about 1e-12 relative) and of a sum of up to 2048 terms (2e-13);
DELTA leaves about three orders of magnitude over that.
"""
import numpy as np

DELTA = 1e-9


def pick(logw, u, delta=DELTA):
    """ (index, fragile) of the inverse-CDF pick of u over exp(logw); index -1 when no weight is positive """
    logw = np.asarray(logw, dtype=np.float64)
    live = ~np.isnan(logw) & (logw > -np.inf)
    if not live.any():
        return -1, False
    top = np.max(logw[live])
    w = np.zeros(len(logw))
    with np.errstate(under='ignore'):
        w[live] = np.exp(logw[live] - top)
    cdf = np.cumsum(w)              # one fixed order: ascending
    cum = cdf[-1]
    hit = np.flatnonzero((w > 0) & (cdf > u * cum))
    index = int(hit[0]) if len(hit) else int(np.flatnonzero(w > 0)[-1])
    edges = cdf / cum
    edges = edges[(edges > 0) & (edges < 1)]
    fragile = bool(len(edges) and np.min(np.abs(edges - u)) < delta)
    return index, fragile


def beta(W, G, m, a, q, memo=None):
    """ log beta_m(a, q): the completions that start with a segment [a, .) in state q, m switches to come after it """
    if memo is not None:
        if (m, a, q) not in memo:
            memo[m, a, q] = beta(W, G, m, a, q)
        return memo[m, a, q]
    T = W.shape[1]
    terms = [W[q, a - 1, b] + G[m, b, q] for b in range(a + 1, T + 1)]
    terms = [t for t in terms if not np.isnan(t) and t > -np.inf]
    if not terms:
        return -np.inf
    top = max(terms)
    return top + np.log(sum(np.exp(t - top) for t in terms))


def draw(W, F, G, transitions, k, u, delta=DELTA, memo=None):
    """
    One draw of k switches from the row u of uniforms: (seg_start, seg_state, fragile, used) with k + 1 segments and the
    number of uniforms consumed, or (None, None, False, 0) when no profile of k switches has positive weight
    """
    S, T = F.shape[0], F.shape[1] - 1
    if k > T - 1:
        return None, None, False, 0
    head = (F[:, 1:] + G[k, 1:, :].T).ravel()       # state-major, b = 1 ... T
    j, fragile = pick(head, u[0], delta)
    if j < 0:
        return None, None, False, 0
    used = 1
    s, t = j // T, j % T + 1
    starts, states = [0], [s]
    for i in range(1, k + 1):
        m = k - i
        allowed = [q for q in range(S) if transitions[s, q]]
        j, f = pick([beta(W, G, m, t, q, memo) for q in allowed], u[2 * i - 1], delta)
        assert j >= 0       # the pick before had positive weight: a completion exists
        fragile |= f
        used += 1
        s = allowed[j]
        starts.append(t)
        states.append(s)
        if i < k:
            j, f = pick(W[s, t - 1, t + 1:] + G[m, t + 1:, s], u[2 * i], delta)     # b = t + 1 ... T
            assert j >= 0
            fragile |= f
            used += 1
            t = t + 1 + j
    return starts, states, fragile, used


def draws(W, F, G, transitions, ks, uniforms, delta=DELTA):
    """
    The draws of a batch: seg_start, seg_state (n, K) in the device's layout (k + 1 segments, then empty segments at T in
    state 0; -1 everywhere without a profile), fragile (n,) and the consumed uniforms (n, U), 0 where none was; K from G
    """
    K = G.shape[0]
    T = F.shape[1] - 1
    n = len(ks)
    seg_start = np.full((n, K), T, dtype=np.int32)
    seg_state = np.zeros((n, K), dtype=np.int32)
    fragile = np.zeros(n, dtype=bool)
    consumed = np.zeros_like(np.asarray(uniforms, dtype=np.float64))
    memo = {}       # beta belongs to the tables, not to a draw
    for r in range(n):
        a, b, fragile[r], used = draw(W, F, G, transitions, int(ks[r]), uniforms[r], delta, memo)
        if a is None:
            seg_start[r], seg_state[r] = -1, -1
            continue
        seg_start[r, :len(a)], seg_state[r, :len(a)] = a, b
        consumed[r, :used] = uniforms[r][:used]
    return seg_start, seg_state, fragile, consumed
