"""
The random streams of the device-side draws, stated in NumPy (no GPU): Philox-4x32-10 as Salmon, Moraes, Dror and Shaw
publish it (SC'11; the Random123 known answers are in tests/test_philox_oracle.py), the 53-bit uniform and the Box-Muller
pair as include/bild_amd.h documents them, and the counter layout of each of the five consumers -- what the consumer of
every draw should have seen.  Written from the paper and the header, not from csrc/philox.h.

`normal_pair` works in np.longdouble where that is wider than double (64-bit significand on x86), with pi from a decimal
string and the quadrant taken off the exact u2 before the multiplication, and rounds once to double: the host's rounding
adds nothing to the bars of tests/test_gpu_device_streams.py.  Where np.longdouble is double, the reduction to the
quadrant is still exact and the rest is double arithmetic.
"""
import math

import numpy as np

MASK = np.uint64(0xFFFFFFFF)
MUL0, MUL1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
WEYL0, WEYL1 = 0x9E3779B9, 0xBB67AE85
ROUNDS = 10
NOISE_BASE = 2 ** 31      # stream word of the Rouse localization noise
FRAGILE = 1e-9            # a comparison decided by less than this, relative: the sample is excused (a condition on the inputs)

LD = np.longdouble
WIDE = np.finfo(LD).nmant > np.finfo(np.float64).nmant
PI = LD('3.14159265358979323846264338327950288419716939937510')


def _words(c):
    c = np.asarray(c)
    if c.dtype == object or c.dtype.kind not in 'ui':
        c = np.array([int(v) for v in np.ravel(c)], dtype=np.uint64).reshape(np.shape(c))
    return c.astype(np.uint64) & MASK


def block(c0, c1, c2, c3, seed):
    """ philox4x32-10 of the counters (c0, c1, c2, c3), broadcast together, under key (seed low, seed high) -> (..., 4) uint32 """
    seed = int(seed)
    assert 0 <= seed < 2 ** 64
    x0, x1, x2, x3 = (a.copy() for a in np.broadcast_arrays(_words(c0), _words(c1), _words(c2), _words(c3)))
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    for _ in range(ROUNDS):
        p0, p1 = MUL0 * x0, MUL1 * x2         # 32 x 32 -> 64 bits: no overflow in uint64
        x0, x1, x2, x3 = (p1 >> np.uint64(32)) ^ x1 ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ x3 ^ np.uint64(k1), p0 & MASK
        k0, k1 = (k0 + WEYL0) & 0xFFFFFFFF, (k1 + WEYL1) & 0xFFFFFFFF
    return np.stack([x0, x1, x2, x3], axis=-1).astype(np.uint32)


def uniform(hi, lo):
    """ ((hi << 32 | lo) >> 11) 2^-53: in [0, 1), exact in double """
    bits = (np.asarray(hi).astype(np.uint64) << np.uint64(32)) | np.asarray(lo).astype(np.uint64)
    return (bits >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def stream_uniforms(seed, c0, c1, c2, n):
    """
    The first n uniforms of the stream (c0, c1, c2) of `seed`, in the order of Philox::uniform(): the block counter is word 3
    and starts at 0; a block gives the uniform of its words (2, 3), then that of its words (0, 1).  c0, c1, c2 broadcast
    -> (..., n)
    """
    nb = (n + 1) // 2
    c0, c1, c2 = np.broadcast_arrays(_words(c0), _words(c1), _words(c2))
    w = block(c0[..., None], c1[..., None], c2[..., None], np.arange(nb, dtype=np.uint64), seed)        # (..., nb, 4)
    u = np.stack([uniform(w[..., 2], w[..., 3]), uniform(w[..., 0], w[..., 1])], axis=-1)
    return u.reshape(u.shape[:-2] + (2 * nb,))[..., :n]


def normal_pair(words):
    """
    Box-Muller on one block (..., 4): u1 = 1 - uniform(w0, w1) in (0, 1], u2 = uniform(w2, w3), r = sqrt(-2 log u1)
    -> (r cos 2 pi u2, r sin 2 pi u2), float64, each rounded once
    """
    words = np.asarray(words)
    u1 = 1.0 - uniform(words[..., 0], words[..., 1])       # exact
    u2 = uniform(words[..., 2], words[..., 3])
    return normal_pair_of(u1, u2)


def normal_pair_of(u1, u2):
    """ the same from u1 in (0, 1] and u2 in [0, 1) """
    u1, u2 = np.asarray(u1, dtype=np.float64), np.asarray(u2, dtype=np.float64)
    q = np.floor(4.0 * u2)                                  # the quadrant: 4 u2 and the rest are exact
    f = (4.0 * u2 - q).astype(LD)
    r = np.sqrt(LD(-2) * np.log(u1.astype(LD)))
    ang = (PI / LD(2)) * f                                  # in [0, pi / 2)
    c, s = np.cos(ang), np.sin(ang)
    q = q.astype(np.int64)
    cq = np.choose(q, [c, -s, -c, s])
    sq = np.choose(q, [s, c, -s, -c])
    return (r * cq).astype(np.float64), (r * sq).astype(np.float64)


def _pair_table(seed, i, T, c2, c3, swap):
    """ the normal of frame t = 0 .. T - 1 and every stream word of c2 (any shape): counter (i, t / 2, c2, c3) -> (T,) + c2.shape """
    c2 = np.asarray(c2, dtype=np.uint64)
    nq = (T + 1) // 2
    q = np.arange(nq, dtype=np.uint64).reshape((nq,) + (1,) * c2.ndim)
    n0, n1 = normal_pair(block(np.uint64(int(i) & 0xFFFFFFFF), q, c2[None], c3, seed))
    if swap:
        n0, n1 = n1, n0
    out = np.empty((2 * nq,) + c2.shape)
    out[0::2] = n0      # even frames the cosine
    out[1::2] = n1      # odd frames the sine
    return out[:T]


def rouse_normals(seed, i, T, N, d, swap=False, mode_stride=16, noise_base=NOISE_BASE):
    """
    What bild_rouse_simulate's device mode uses for trajectory i of a call, in the layout of models._replay_draws: T N d
    normals of the dynamics (frame 0 the steady state; mode-major, dimension-minor), then T d of the localization noise.
    Counters (i, t / 2, 16 j + k, 0) and (i, t / 2, 2^31 + k, 0); even t takes the cosine.  The keyword arguments state
    the layouts that the contract rules out (the mutation checks of the GPU test).
    """
    j, k = np.arange(N, dtype=np.uint64)[:, None], np.arange(d, dtype=np.uint64)[None, :]
    dyn = _pair_table(seed, i, T, np.uint64(mode_stride) * j + k, 0, swap)                  # (T, N, d)
    noise = _pair_table(seed, i, T, np.uint64(noise_base) + k[0], 0, swap)                  # (T, d)
    return np.concatenate([dyn.ravel(), noise.ravel()])


def gauss_normals(seed, i, intervals, ss_order, swap=False):
    """
    What bild_gauss_simulate's device mode uses for trajectory i of a call, in its replay layout: interval (t0, t1, state)
    after interval, dimension after dimension; a first interval skips frame 0 in a dimension of ss_order 1.  The normal of
    (frame t, dimension k) comes from counter (i, t / 2, k, 1); even t takes the cosine.
    """
    ss_order = np.asarray(ss_order)
    d = ss_order.shape[1]
    T = intervals[-1][1]
    Z = _pair_table(seed, i, T, np.arange(d, dtype=np.uint64), 1, swap)                     # (T, d)
    out = []
    for t0, t1, s in intervals:
        for k in range(d):
            f0 = int(ss_order[s, k]) if t0 == 0 else t0
            out.append(Z[f0:t1, k])
    return np.concatenate(out) if out else np.zeros(0)


def segdraw_uniforms(seed, r, n):
    """ the first n uniforms of draw r (the index of the draw in the call; broadcasts) of bild_gauss_segment_draw: counter (r, 0, 0, block) """
    return stream_uniforms(seed, r, 0, 0, n)


def dwelldraw_uniforms(seed, stream, n):
    """ the first n uniforms of stream index `stream` (64 bits; broadcasts) of bild_gauss_dwell_draw: counter (low, high, 0, block) """
    s = np.array([int(v) for v in np.ravel(stream)], dtype=np.uint64).reshape(np.shape(stream))
    return stream_uniforms(seed, s & MASK, s >> np.uint64(32), 0, n)


# ---------------------------------------------------------------- the AMIS draws (amis_device.hip: draw_kernel)

def _near(x, y, scale):
    """ x and y compare within FRAGILE of `scale` (the magnitude of the terms that form them) """
    return not abs(x - y) > FRAGILE * scale


class _Stream:
    """ one sample's uniforms in order, and whether a comparison on them was close """

    def __init__(self, seed, k1, sample):
        self.key = (seed, sample & 0xFFFFFFFF, sample >> 32, k1)
        self.u = np.zeros(0)
        self.used = 0
        self.fragile = False

    def uniform(self):
        if self.used >= len(self.u):
            seed, c0, c1, c2 = self.key
            self.u = stream_uniforms(seed, c0, c1, c2, max(32, 2 * len(self.u)))
        self.used += 1
        return float(self.u[self.used - 1])

    def normal(self):
        """ one Box-Muller value per two uniforms: the cosine """
        u1 = 1.0 - self.uniform()
        u2 = self.uniform()
        return float(normal_pair_of(u1, u2)[0])

    def gamma(self, a):
        """ Marsaglia-Tsang, with gamma(a) = gamma(a + 1) U^(1/a) below one; at most 64 trials, then the mode d """
        if not a > 0:
            return 0.0
        boost = 1.0
        if a < 1.0:
            with np.errstate(over='ignore', divide='ignore'):
                e = float(np.float64(1.0) / np.float64(a))
            boost = float(np.power(np.float64(1.0 - self.uniform()), np.float64(e)))
            a += 1.0
        d = a - 1.0 / 3.0
        cc = 1.0 / math.sqrt(9.0 * d)
        for _ in range(64):
            x = self.normal()
            t = 1.0 + cc * x
            self.fragile |= _near(t, 0.0, 1.0 + abs(cc * x))
            if t <= 0:
                continue
            v = t * t * t
            u = 1.0 - self.uniform()
            x4 = (x * x) * (x * x)
            squeeze = 1.0 - 0.0331 * x4
            self.fragile |= _near(u, squeeze, 1.0 + 0.0331 * x4)
            if u < squeeze:
                return boost * d * v
            lu, lv = math.log(u), math.log(v)
            rhs = 0.5 * x * x + d * (1.0 - v + lv)
            self.fragile |= _near(lu, rhs, abs(lu) + 0.5 * x * x + d * (1.0 + v + abs(lv)))
            if lu < rhs:
                return boost * d * v
        return boost * d

    def crossing(self, weights, default):
        """ the first s with (w_0 + ... + w_s) / sum(w) > u, `default` if there is none """
        last = 0.0
        for w in weights:
            last += w
        u = self.uniform()
        c = 0.0
        for s, w in enumerate(weights):
            c += w
            if last > 0:
                ratio = c / last
                self.fragile |= _near(ratio, u, max(ratio, u))
                if ratio > u:
                    return s
        return default


def amis_draw(seed, k1, first, n, a, prob, trans):
    """
    The whole of draw_kernel for the samples r = 0 .. n - 1 of a step, stream (seed, k1, first + r): the k1 gamma variates
    of concentrations `a` and their normalised vector (or, where their sum is 0 or infinite, the corner j with probability
    a_j / sum(a) from one more uniform); then the trace, slot by slot, from prob (states, k1) -- slot 0 over all states with
    the last state as default, later slots over the successors that `trans` allows with state 0 as default.
    -> ss (n, k1), thetas (n, k1) int64, the uniforms consumed (n,), fragile (n,) bool
    """
    a = np.asarray(a, dtype=np.float64)
    prob = np.asarray(prob, dtype=np.float64)
    trans = np.asarray(trans) != 0
    S = prob.shape[0]
    assert a.shape == (k1,) and prob.shape == (S, k1) and trans.shape == (S, S)
    ss, thetas = np.empty((n, k1)), np.empty((n, k1), dtype=np.int64)
    used, fragile = np.empty(n, dtype=np.int64), np.zeros(n, dtype=bool)
    for r in range(n):
        rng = _Stream(int(seed), int(k1), int(first) + r)
        g = np.array([rng.gamma(float(a[j])) for j in range(k1)])
        tot = asum = 0.0
        for j in range(k1):
            tot += float(g[j])
            asum += float(a[j])
        if tot > 0 and tot < math.inf:
            ss[r] = g / tot
        else:
            u = float(np.float64(rng.uniform()) * np.float64(asum))
            c, corner = 0.0, k1 - 1
            for j in range(k1):
                c += float(a[j])
                rng.fragile |= _near(u, c, max(u, c))
                if u < c:
                    corner = j
                    break
            ss[r] = 0.0
            ss[r, corner] = 1.0
        prev = rng.crossing([float(prob[s, 0]) for s in range(S)], S - 1)
        thetas[r, 0] = prev
        for i in range(1, k1):
            prev = rng.crossing([float(prob[s, i]) * (1.0 if trans[prev, s] else 0.0) for s in range(S)], 0)
            thetas[r, i] = prev
        used[r], fragile[r] = rng.used, rng.fragile
    return ss, thetas, used, fragile


def amis_prob(logp):
    """ the slot weights as the host hands them to draw_kernel: exp(logp - logsumexp over the states of a slot), (states, k1) """
    logp = np.asarray(logp, dtype=np.float64)
    out = np.empty_like(logp)
    for i in range(logp.shape[1]):
        col = logp[:, i]
        top = np.max(col)
        top = top if np.isfinite(top) else 0.0
        s = 0.0
        for v in col:
            s += math.exp(v - top) if v > -math.inf else 0.0
        out[:, i] = np.exp(col - (math.log(s) + top))
    return out
