"""
Shared by tests/test_gauss_tables.py (CPU) and tests/test_gpu_gauss_tables.py: the read-out of every entry of
GenericGaussianModel's interval tables through `logL_segments`, a fast float64 oracle of the tables, and the cases.

* Rows.  The table of one trajectory holds W[s][a'][b] (window [a', b) of a later interval in state s) and F[s][b] (first
  interval [0, b)).  An interval [a, b) with a >= 1 reads W[s][a - 1][b].  The rows

      K1 = 1, state s:                                       F[s][T]
      K1 = 2, starts (0, a), states (s0, s):                 F[s0][a] + W[s][a - 1][T]
      K1 = 3, starts (0, a, b), states (s0, s, s2):          F[s0][a] + W[s][a - 1][b] + W[s2][b - 1][T]

  over every 1 <= a < b < T and every s, with s0 = s + 1 and s2 = s - 1 (mod S), contain every entry a profile can read,
  each row summing at most three of them.  All rows are padded to K1 = 3 with empty segments at T (starts (0, T, T) and
  (0, a, T)), which the walk skips, so that one call evaluates them all.
* `tables_fast`: W and F as `gauss_oracle.tables` defines them, with one Cholesky factor per (state, dimension) for all
  starts inside the dimension's trailing gap-free run, and one factor per distinct set of valid frames before it.
* Missing patterns per dimension, the designed cases and the seeded sweep of the GPU file.
"""
import numpy as np
from scipy.linalg import solve_triangular

import gauss_oracle as G
from bild_amd.gauss import covariance

HALF_LOG2PI = 0.5 * G.LOG2PI


# ------------------------------------------------------------------------------------------------------------ rows
class Rows:
    """ rows of one (T, S): kind (n,) in {1, 2, 3}, states (n, 3) = (s0, s, s2), a and b (n,) (T where the row has none) """

    def __init__(self, T, S, kind, states, a, b):
        self.T, self.S = T, S
        self.kind, self.states, self.a, self.b = kind, states, a, b

    def __len__(self):
        return len(self.kind)

    def segments(self):
        """ (seg_start, seg_state), both (n, 3) int32, for `logL_segments` """
        start = np.stack([np.zeros_like(self.a), self.a, self.b], axis=1).astype(np.int32)
        return np.ascontiguousarray(start), np.ascontiguousarray(self.states.astype(np.int32))

    def expanded(self, r):
        """ row r as an expanded profile (T,) """
        a, b = int(self.a[r]), int(self.b[r])
        return np.repeat(self.states[r], [a, b - a, self.T - b])

    def name(self, r):
        s0, s, s2 = (int(v) for v in self.states[r])
        a, b, T = int(self.a[r]), int(self.b[r]), self.T
        if self.kind[r] == 1:
            return f"K1=1 state {s0}: F[{s0}][{T}]"
        if self.kind[r] == 2:
            return f"K1=2 starts (0, {a}) states ({s0}, {s}): F[{s0}][{a}] + W[{s}][{a - 1}][{T}]"
        return (f"K1=3 starts (0, {a}, {b}) states ({s0}, {s}, {s2}): "
                f"F[{s0}][{a}] + W[{s}][{a - 1}][{b}] + W[{s2}][{b - 1}][{T}]")

    def entries(self):
        """ the table entries the rows read: (state, b) of F and (state, a', b) of W, one array of indices each """
        k1, k2, k3 = self.kind == 1, self.kind >= 2, self.kind == 3
        T = self.T
        f = np.concatenate([np.stack([self.states[k1, 0], np.full(k1.sum(), T)]),
                            np.stack([self.states[k2, 0], self.a[k2]])], axis=1)
        w = np.concatenate([np.stack([self.states[k2, 1], self.a[k2] - 1, self.b[k2]]),
                            np.stack([self.states[k3, 2], self.b[k3] - 1, np.full(k3.sum(), T)])], axis=1)
        return f, w

    def evaluate(self, W, F):
        """ the rows' sums on tables W (S, T, T + 1), F (S, T + 1) by fancy indexing """
        T = self.T
        s0, s, s2 = self.states.T
        out = F[s0, self.a].copy()               # kind 1: a == T
        k2, k3 = self.kind >= 2, self.kind == 3
        out[k2] += W[s[k2], self.a[k2] - 1, self.b[k2]]      # kind 2: b == T
        out[k3] += W[s2[k3], self.b[k3] - 1, T]
        return out


def rows(T, S, a_sel=None, b_sel=None):
    """
    The rows of (T, S); full, or (a_sel / b_sel given) with the K1 = 3 rows restricted to the chosen a with every b and
    the chosen b with every a.  The K1 = 1 and K1 = 2 rows are always complete.  S = 1 has the K1 = 1 row only: a
    boundary between equal states switches nothing.
    """
    kind, states, aa, bb = [], [], [], []
    for s in range(S):
        kind.append(np.array([1]))
        states.append(np.array([[s, s, s]]))
        aa.append(np.array([T]))
        bb.append(np.array([T]))
    if S > 1:
        a2 = np.arange(1, T)
        i, j = np.triu_indices(max(T - 1, 0), k=1)
        a3, b3 = i + 1, j + 1                   # 1 <= a < b < T
        if a_sel is not None or b_sel is not None:
            keep = np.isin(a3, np.asarray(a_sel if a_sel is not None else [], dtype=int)) | \
                np.isin(b3, np.asarray(b_sel if b_sel is not None else [], dtype=int))
            a3, b3 = a3[keep], b3[keep]
        for s in range(S):
            s0, s2 = (s + 1) % S, (s - 1) % S
            kind += [np.full(len(a2), 2), np.full(len(a3), 3)]
            states += [np.tile([s0, s, s], (len(a2), 1)), np.tile([s0, s, s2], (len(a3), 1))]
            aa += [a2, a3]
            bb += [np.full(len(a2), T), b3]
    return Rows(T, S, np.concatenate(kind), np.concatenate(states).astype(np.int64), np.concatenate(aa).astype(np.int64),
                np.concatenate(bb).astype(np.int64))


def touched(rw):
    """ how often the rows read each entry: counts of W (S, T, T + 1) and of F (S, T + 1) """
    cW = np.zeros((rw.S, rw.T, rw.T + 1), dtype=np.int64)
    cF = np.zeros((rw.S, rw.T + 1), dtype=np.int64)
    f, w = rw.entries()
    np.add.at(cF, tuple(f), 1)
    np.add.at(cW, tuple(w), 1)
    return cW, cF


# ------------------------------------------------------------------------------------------------------- fast oracle
def _tau(C, y):
    L = np.linalg.cholesky(C)
    z = solve_triangular(L, y, lower=True, check_finite=False)
    return np.log(np.diag(L)) + 0.5 * z ** 2 + HALF_LOG2PI


def _shifted(src, rows_, cols):
    """ M[i, q] = src[i + q] where that exists, 0 elsewhere """
    idx = np.add.outer(np.arange(rows_), np.arange(cols))
    return np.where(idx < len(src), src[np.minimum(idx, len(src) - 1)], 0.0) if len(src) else np.zeros((rows_, cols))


def tables_fast(msd, msd_inf, mean, order, x):
    """
    W (S, T, T + 1) and F (S, T + 1) as `gauss_oracle.tables` returns them.  Per state and dimension, with the valid
    frames v_0 < ... < v_{V-1} and c the length of the gap-free run that ends at the last frame:

    * a start whose valid frames all lie in that run (rank r >= V - c) has the covariance of n consecutive frames, a
      leading block of the run's Toeplitz matrix; the Cholesky factor of a leading block is the leading block of the
      factor, and forward substitution never looks beyond its row, so one factor L and one triangular solve L Z = Y with
      the starts' vectors as zero-padded columns give every z;
    * the other starts are factored on their own, once per rank (starts inside one gap share their valid frames).
    """
    x = np.asarray(x, dtype=np.float64)
    T, d = x.shape
    S = msd.shape[0]
    W = np.zeros((S, T, T + 1))
    F = np.zeros((S, T + 1))
    for k in range(d):
        valid = np.nonzero(~np.isnan(x[:, k]))[0]
        V = len(valid)
        c = 0
        while c < V and valid[V - 1 - c] == T - 1 - c:
            c += 1
        xc = x[T - c:T, k]
        rank = np.searchsorted(valid, np.arange(T), side='left')
        for n in range(S):
            m, o = mean[n, k], order[n, k]
            nS = c if o == 0 else c - 1           # size of the run's matrix
            logd = Z = None
            if nS > 0:
                L = np.linalg.cholesky(covariance(msd[n, k], msd_inf[n, k], np.arange(T - c, T), o))
                logd = np.log(np.diag(L))
                if o == 0:
                    Y = _shifted(xc - m, nS, c + 1)
                    Y[0, :c] = xc                          # the raw conditioning value
                    Y[:, c] = xc - m                       # the first interval: centred throughout
                else:
                    Y = _shifted(np.diff(xc) - m, nS, c)
                Z = solve_triangular(L, Y, lower=True, check_finite=False)
            own = {}

            def tau_of(r, centred):
                cnt = V - r if o == 0 else V - r - 1
                if cnt <= 0:
                    return np.zeros(0)
                if r >= V - c:
                    col = c if centred else r - (V - c)
                    return logd[:cnt] + 0.5 * Z[:cnt, col] ** 2 + HALF_LOG2PI
                if (r, centred) not in own:
                    u = valid[r:]
                    if o == 0:
                        y = x[u, k] - m
                        if not centred:
                            y[0] = x[u[0], k]
                    else:
                        y = np.diff(x[u, k]) - m
                    own[r, centred] = _tau(covariance(msd[n, k], msd_inf[n, k], u, o), y)
                return own[r, centred]

            for a in range(T + 1):          # a == T: the first interval
                first = a == T
                r = 0 if first else rank[a]
                u = valid[r:]
                tau = tau_of(r, first and o == 0)
                if o == 0:
                    ends, skip = u, 0 if first else 1
                else:
                    ends, skip = u[1:], 0
                lo = 0 if first else a
                b = np.arange(lo + 1, T + 1)
                part = np.concatenate(([0.0], np.cumsum(np.where(np.arange(len(tau)) >= skip, tau, 0.0))))
                val = -part[np.searchsorted(ends, b, side='left')]
                if o == 0 and not first:
                    val = np.where(np.searchsorted(u, b, side='left') == 0, np.nan, val)
                if first:
                    F[n, b] += val
                else:
                    W[n, a, b] += val
    return W, F


# ----------------------------------------------------------------------------------------------------------- cases
PATTERNS = ('none', 'last', 'first', 'inner20', 'iid10', 'two_valid', 'one_valid', 'all_nan', 'bursty')
SPARSE = ('two_valid', 'one_valid', 'all_nan')      # V <= 2: most later ss_order-0 windows have no valid frame


def missing_mask(name, rng, T):
    """ the missing frames (T,) bool of one dimension """
    m = np.zeros(T, dtype=bool)
    if name == 'last':
        m[T - 1] = True
    elif name == 'first':
        m[0] = True
    elif name == 'inner20':                     # one inner gap: 20 frames, fewer on a short trajectory
        g = min(20, T // 3)
        m[T // 3:T // 3 + g] = True
    elif name == 'iid10':
        m = rng.random(T) < 0.1
    elif name == 'two_valid':
        m[:] = True
        m[[5, 200] if T > 200 else [T // 4, (3 * T) // 4]] = False
    elif name == 'one_valid':
        m[:] = True
        m[T // 2] = False
    elif name == 'all_nan':
        m[:] = True
    elif name == 'bursty':                      # a few short bursts; from T = 16 on they end before the last frame
        for _ in range(1 + T // 64):
            t0 = int(rng.integers(0, T - 7 if T >= 16 else T))
            m[t0:t0 + int(rng.integers(2, 7))] = True
    elif name != 'none':
        raise ValueError(name)
    return m


# the designed patterns of the full read-out (S = 2, d = 2): name -> per-dimension patterns
DESIGNED = {
    'no_gaps': ('none', 'none'),
    'last_frame_missing_dim0': ('last', 'none'),        # c = 0 in dimension 0, the shared factor in dimension 1
    'first_frame_missing': ('first', 'first'),
    'inner_gap_20_dim0': ('inner20', 'none'),
    'iid_10_percent': ('iid10', 'iid10'),
    'two_valid_dim1': ('none', 'two_valid'),            # V = 2
    'one_valid_dim1': ('none', 'one_valid'),            # V = 1
    'all_nan_dim1': ('none', 'all_nan'),                # V = 0
}
DESIGNED_ORDERS = np.array([[0, 1], [1, 0]])            # both orders in both dimensions


def model_from(msd, msd_inf, mean, order):
    """ the GenericGaussianModel of the arrays """
    import bild_amd
    S, d = order.shape
    return bild_amd.GenericGaussianModel(
        [[(msd[n, k] if order[n, k] == 1 else np.append(msd[n, k], msd_inf[n, k]), mean[n, k], int(order[n, k]))
          for k in range(d)] for n in range(S)])


def random_case(rng, S, d, T, p_missing):
    """ random power-law MSDs with noise, means and ss_orders, a random walk with independent missing frames """
    lags = np.arange(T, dtype=float)
    msd = np.zeros((S, d, T))
    inf = np.zeros((S, d))
    for n in range(S):
        for k in range(d):
            G_, a, s2 = rng.uniform(0.3, 2), rng.uniform(0.4, 1.2), rng.uniform(0.05, 0.3)
            msd[n, k] = np.where(lags > 0, G_ * lags ** a + 2 * s2, 0)
            inf[n, k] = 2 * G_ * T ** a + 4 + 2 * s2
    order = rng.integers(0, 2, size=(S, d))
    mean = rng.normal(scale=0.3, size=(S, d))
    x = np.cumsum(rng.normal(size=(T, d)), axis=0)
    if p_missing:
        x[rng.random((T, d)) < p_missing] = np.nan
    return msd, inf, mean, order, x


def model_arrays(rng, S, d, T, order=None):
    """ means and power-law MSDs as `random_case` draws them, gap-free data: msd, inf, mean, order, x """
    msd, inf, mean, o, x = random_case(rng, S, d, T, 0.0)
    if order is not None:
        o = np.broadcast_to(np.asarray(order), (S, d)).copy()
    return msd, inf, mean, o, x


def apply_patterns(rng, x, patterns):
    x = x.copy()
    for k, name in enumerate(patterns):
        x[missing_mask(name, rng, len(x)), k] = np.nan
    return x


def expected_nan(rw, order, x):
    """
    Which rows the reference cannot evaluate, from the missing frames alone: a later interval [a, b) in a state with an
    ss_order-0 dimension that has no valid frame in the window [a - 1, b).  The first interval is always finite.
    """
    T = rw.T
    valid = np.concatenate([np.zeros((1, x.shape[1]), dtype=np.int64), np.cumsum(~np.isnan(x), axis=0)])    # valid frames before t
    out = np.zeros(len(rw), dtype=bool)
    k2, k3 = rw.kind >= 2, rw.kind == 3
    for k in range(x.shape[1]):
        empty = lambda lo, hi: valid[hi, k] == valid[lo, k]
        zero = order[:, k] == 0
        out[k2] |= zero[rw.states[k2, 1]] & empty(rw.a[k2] - 1, rw.b[k2])
        out[k3] |= zero[rw.states[k3, 2]] & empty(rw.b[k3] - 1, np.full(k3.sum(), T))
    return out


def expected_nan_profile(states, order, x):
    """ the same for one expanded profile """
    for i, (t0, t1, n) in enumerate(G.intervals(states)):
        if i > 0 and np.any((order[n] == 0) & np.all(np.isnan(x[t0 - 1:t1]), axis=0)):
            return True
    return False


def forces_nan(T, patterns, order):
    """
    Whether the missing patterns force many NaN rows: a dimension in which some state has ss_order 0 and which is
    sparse (V <= 2), or has gaps on a trajectory so short (T < 127) that a few all-missing windows are a large share
    """
    return any(np.any(order[:, k] == 0) and (p in SPARSE or (T < 127 and p != 'none')) for k, p in enumerate(patterns))


def designed_case(name, T, seed=0):
    """ a designed case of the full read-out: msd, inf, mean, order, x """
    rng = np.random.default_rng(1000 * T + seed)
    msd, inf, mean, order, x = model_arrays(rng, 2, 2, T, DESIGNED_ORDERS)
    return msd, inf, mean, order, apply_patterns(rng, x, DESIGNED[name])


SWEEP_T = (1, 2, 3, 4, 17, 63, 64, 65, 127, 129, 200, 255, 257)


def sweep_case(seed):
    """
    One seed of the sweep: S, d in 1 ... 4, T from SWEEP_T (in turn, so that 13 seeds see every length), ss_orders all 0,
    all 1 or random (in turn every 13 seeds), one missing pattern per dimension.  -> dict
    """
    rng = np.random.default_rng(90000 + seed)
    S, d = int(rng.integers(1, 5)), int(rng.integers(1, 5))
    T = SWEEP_T[seed % len(SWEEP_T)]
    mode = ('zero', 'one', 'random')[(seed // len(SWEEP_T)) % 3]
    msd, inf, mean, order, x = model_arrays(rng, S, d, T, {'zero': 0, 'one': 1, 'random': None}[mode])
    weight = np.array([1.0 if p in SPARSE else 3.0 for p in PATTERNS])      # (a sparse ss_order-0 dimension leaves few finite rows)
    patterns = tuple(str(rng.choice(PATTERNS, p=weight / weight.sum())) for _ in range(d))
    x = apply_patterns(rng, x, patterns)
    return dict(seed=seed, S=S, d=d, T=T, mode=mode, patterns=patterns, msd=msd, inf=inf, mean=mean, order=order, x=x, rng=rng)


def sweep_profiles(rng, T, S, x):
    """
    The candidates of a sweep seed, expanded: no switch, a switch at frame 1, one at T - 1, two adjacent switches, a
    switch inside a gap (a missing frame of some dimension; a random frame without one), one random profile.  Those a
    short trajectory or S = 1 cannot hold are left out.
    """
    def build(cuts):
        st = np.zeros(T, dtype=np.int64)
        cur = int(rng.integers(S))
        st[:] = cur
        for t in cuts:
            cur = (cur + 1 + int(rng.integers(S - 1))) % S
            st[t:] = cur
        return st

    out = [build([])]
    if S > 1 and T > 1:
        out.append(build([1]))
        out.append(build([T - 1]))
        if T > 2:
            t = int(rng.integers(1, T - 1))
            out.append(build([t, t + 1]))
        gaps = np.nonzero(np.any(np.isnan(x[1:]), axis=1))[0] + 1
        out.append(build([int(rng.choice(gaps)) if len(gaps) else int(rng.integers(1, T))]))
        k = int(rng.integers(0, min(6, T - 1) + 1))
        out.append(build(sorted(rng.choice(np.arange(1, T), size=k, replace=False))))
    return out
