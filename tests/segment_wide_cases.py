"""
Cases shared by tests/test_segment_wide.py (no GPU) and tests/test_gpu_segment_wide.py: the fixed-k exact paths
(`exact_sample`, `exact_draw`, `exact_evidence`) beyond S = 3 and T = 256.  Models and data come from
`segment_cases.random_model` / `random_traj` with seeds derived from (S, T); the transition matrix of every case is set by
name (`transitions_of`), so that `random_model`'s S = 3 rule does not reach it.  The tables come from
`gauss_table_cases.tables_fast`, the oracle answers from `segment_oracle.solve_fast`; an answer is computed once a session
and shared, its arrays read-only, the seconds it took in ORACLE_SECONDS.
"""
import functools
import time

import numpy as np

import bild_amd
import gauss_table_cases as TC
import segment_cases as C
import segment_draw_oracle as DO
import segment_oracle as SO

ORACLE_LIMIT = 20.0     # seconds an oracle answer may take (as tests/segment_sensitivity_cases.py)
ORACLE_SECONDS = {}


def transitions_of(name, S):
    """
    'full': every off-diagonal pair; 'ring': s -> s + 1 mod S only; 'sink' (S = 4): state 3 is never left and 0 -> 3 is
    forbidden; 'source' (S = 5): state 0 is never entered; 'no02' (S = 3): 0 -> 2 forbidden
    """
    M = ~np.eye(S, dtype=bool)
    if name == 'ring':
        M = np.zeros((S, S), dtype=bool)
        M[np.arange(S), (np.arange(S) + 1) % S] = S > 1
    elif name == 'sink':
        assert S == 4
        M[3, :] = False
        M[0, 3] = False
    elif name == 'source':
        assert S == 5
        M[:, 0] = False
    elif name == 'no02':
        assert S == 3
        M[0, 2] = False
    elif name != 'full':
        raise ValueError(name)
    return M


def fast_tables(model, x):
    W, F = TC.tables_fast(model.msd, model.msd_inf, model.mean, model.ss_order, np.asarray(x, dtype=np.float64))
    W.setflags(write=False)
    F.setflags(write=False)
    return W, F


def make(S, T, missing, trans, seed=None, d=2):
    """ (model, x): gap-free data get random ss_orders, data with missing frames ss_order 1 throughout (nothing is NaN) """
    rng = np.random.default_rng(7000 * S + T if seed is None else seed)
    model = C.random_model(rng, S, T + 8, orders=np.ones((S, d), dtype=int) if len(missing) else None, d=d)
    model.transitions = transitions_of(trans, S)
    x = C.random_traj(rng, T, missing, d=d)
    x.setflags(write=False)
    return model, x


def gap_case(T, lo, hi):
    """ `test_gpu_segment_dp.order0_gap_case` with its gap at frames lo ... hi - 1 of dimension 0 """
    rng = np.random.default_rng(33)
    model = bild_amd.GenericGaussianModel([[(np.append(np.arange(T + 8) * 0.5 + 0.1, 50.0), 0.3 * s, 0),
                                            (np.arange(T + 8) * (0.5 + s), 0.0, 1)] for s in range(2)])
    x = C.random_traj(rng, T)
    x[lo:hi, 0] = np.nan
    x.setflags(write=False)
    return model, x


# name -> (S, T, missing frames, transitions, k_max, nan mode)
SEGMENT_CASES = {
    's1_T1': (1, 1, (), 'full', 3, 'propagate'),
    's1_T65': (1, 65, (7,), 'full', 3, 'propagate'),
    's4_T3': (4, 3, (), 'full', 4, 'propagate'),
    's4_T64': (4, 64, (), 'full', 6, 'propagate'),
    's4_T65': (4, 65, (), 'full', 6, 'propagate'),
    's4_T130': (4, 130, (64,), 'full', 4, 'propagate'),
    's4_T65_ring': (4, 65, (), 'ring', 6, 'propagate'),
    's4_T70_sink': (4, 70, (), 'sink', 5, 'propagate'),
    's5_T70_source': (5, 70, (), 'source', 4, 'propagate'),
    's2_T257': (2, 257, (255,), 'full', 6, 'propagate'),
    's3_T321': (3, 321, (128,), 'no02', 4, 'propagate'),
    's4_T257': (4, 257, (100,), 'full', 3, 'propagate'),
    'gap_T130_propagate': (2, 130, 'gap', 'full', 4, 'propagate'),
    'gap_T130_omit': (2, 130, 'gap', 'full', 4, 'omit'),
}
GAP = (61, 67)      # frames 61 ... 66 of dimension 0: across the first tile edge
# the cases whose MAP profile is compared state by state: gap-free data, unique by 1e-9 at every k (test_segment_wide.py)
SAME_MAP = ('s4_T64', 's4_T65', 's4_T65_ring', 's4_T70_sink', 's5_T70_source')


@functools.lru_cache(maxsize=None)
def segment_case(name):
    """ (model, x, W, F, k_max, nan) """
    S, T, missing, trans, k_max, nan = SEGMENT_CASES[name]
    model, x = gap_case(T, *GAP) if missing == 'gap' else make(S, T, missing, trans)
    return (model, x) + fast_tables(model, x) + (k_max, nan)


def _freeze(out):
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def map_unique(W, F, transitions, kept, k, tol=1e-9):
    """
    Whether the MAP of k switches is the only profile within `tol` of the maximum, from the oracle's own V: one final
    state and, at every node of the MAP's path, one (c, s') within tol.  Another profile that close either ends in another
    state or leaves the path at some node through a second pointer that close, so the test is sufficient.
    """
    V, ptr_c, ptr_q, ok = kept['V'], kept['ptr_c'], kept['ptr_q'], kept['ok']
    S, T = F.shape[0], F.shape[1] - 1
    cand = [s for s in range(S) if ptr_c[k, T, s] >= 0]
    if not cand:
        return True
    s = max(cand, key=lambda q: (V[k, T, q], -q))
    if sum(V[k, T, q] >= V[k, T, s] - tol for q in cand) != 1:
        return False
    b = T
    for j in range(k, 0, -1):
        near = 0
        for q in np.nonzero(transitions[:, s])[0]:
            c = np.arange(j, b)
            t = V[j - 1, c, q] + W[s, c - 1, b]
            near += int(np.sum((t >= V[j, b, s] - tol) & (ok[j - 1, c, q] > 0).astype(bool)))
        if near != 1:
            return False
        b, s = int(ptr_c[j, b, s]), int(ptr_q[j, b, s])
    return True


def _answer(key, model, W, F, k_max, nan):
    kept = {}
    start = time.perf_counter()
    out = SO.solve_fast(W, F, model.transitions, k_max, nan=nan, kept=kept)
    ORACLE_SECONDS[key] = time.perf_counter() - start
    out['map_unique'] = [map_unique(W, F, model.transitions, kept, k) for k in range(k_max + 1)]
    return _freeze(out)


@functools.lru_cache(maxsize=None)
def segment_answer(name):
    model, x, W, F, k_max, nan = segment_case(name)
    return _answer(name, model, W, F, k_max, nan)


def oracle_noise(name):
    """ the oracle's own rounding: `solve_fast` in np.longdouble against the double answer, worst |difference| per output """
    model, x, W, F, k_max, nan = segment_case(name)
    d = segment_answer(name)
    e = SO.solve_fast(W, F, model.transitions, k_max, nan=nan, dtype=np.longdouble)
    worst = {}
    for key in ('logev', 'KL', 'map_logL', 'log_post'):
        fin = np.isfinite(d[key])
        worst[key] = float(np.max(np.abs(d[key][fin] - e[key][fin]))) if fin.any() else 0.0
    return worst


# --------------------------------------------------------------------------------------------------------- ragged set
RAGGED = ((1, ()), (257, (100,)), (64, ()), (130, (63,)), (2, ()), (65, (9,)))
RAGGED_K_MAX = 3
RAGGED_SAME_MAP = (2,)      # T = 64, gap-free; the one-frame trajectory ties in every state (ss_order 1: F[s][1] = 0)


def _ragged(seed):
    rng = np.random.default_rng(seed)
    model = C.random_model(rng, 4, 270, orders=np.ones((4, 2), dtype=int))
    model.transitions = transitions_of('full', 4)
    xs = [C.random_traj(rng, T, missing) for T, missing in RAGGED]
    for x in xs:
        x.setflags(write=False)
    return model, xs


@functools.lru_cache(maxsize=None)
def ragged_case():
    """ (model, trajectories, their (W, F)): four states, `full`, ss_order 1, six lengths for one call """
    model, xs = _ragged(7000 * 4 + sum(T for T, _ in RAGGED))
    return model, xs, [fast_tables(model, x) for x in xs]


# ---------------------------------------------------------------------- marginals below the range of linear weights
SHARP_K_MAX = 3
SHARP_FIRM, SHARP_FLOOR = -600.0, -700.0


@functools.lru_cache(maxsize=None)
def sharp_case():
    """
    (model, x, W, F): the T = 257 trajectory (frame 100 missing) of a ragged set of another seed, whose model tells the four
    states far apart: the oracle's log marginals go down to -2960 at k = 0 and -955 at k = 1, where `segdp_cover_kernel`'s
    linear weights exp(. - map_logL_k) have underflowed ("Range")
    """
    model, xs = _ragged(28999)
    return (model, xs[1]) + fast_tables(model, xs[1])


@functools.lru_cache(maxsize=None)
def sharp_answer():
    model, x, W, F = sharp_case()
    return _answer('sharp', model, W, F, SHARP_K_MAX, 'propagate')


def sharp_bar(want, k, T, n_profiles):
    """
    The error allowed to a finite device log marginal whose oracle value is `want`: 1e-10, plus what the subnormal range
    takes.  An entry is a sum of at most k T^2 terms Z_alpha Z_gamma exp(x) with 1 <= Z_alpha Z_gamma <= n_k (each Z sums
    exp(. - max) over partial profiles), scaled so that the entry is exp(want + D), D = logev + log n - map_logL >= 0.  An
    `exp` below 2^-1022 is off by up to one unit of 2^-1074, so the entry by up to k T^2 n_k 2^-1074, relative to at least
    exp(want).  The same count shows an entry above -700 finite: its largest `exp` is above exp(-700) / (k T^2 n_k) > 2^-1074.
    """
    slack = np.log(max(1, k) * T * T * float(max(1, n_profiles)))
    with np.errstate(over='ignore'):
        return 1e-10 + np.exp(slack - 1074 * np.log(2.0) - want)


@functools.lru_cache(maxsize=None)
def ragged_answers():
    model, xs, tabs = ragged_case()
    return [_answer(('ragged', j), model, W, F, RAGGED_K_MAX, 'propagate') for j, (W, F) in enumerate(tabs)]


# ------------------------------------------------------------------------------------------------------ backtrack set
BACKTRACK_T = tuple(range(5, 49))
BACKTRACK_K_MAX = 5
BACKTRACK_ORACLE = (0, 42, 43)      # the first trajectory and the two whose rows lie in the second workgroup


@functools.lru_cache(maxsize=None)
def backtrack_case():
    """ (model, trajectories): 44 trajectories of two states, 44 x 6 = 264 (trajectory, k) rows for 256 lanes a workgroup """
    rng = np.random.default_rng(7000 * 2 + 44)
    model = C.random_model(rng, 2, 56)
    model.transitions = transitions_of('full', 2)
    xs = [C.random_traj(rng, T) for T in BACKTRACK_T]
    for x in xs:
        x.setflags(write=False)
    return model, xs


@functools.lru_cache(maxsize=None)
def backtrack_answer(j):
    """ `segment_oracle.solve`, the loops, of trajectory j """
    model, xs = backtrack_case()
    W, F = fast_tables(model, xs[j])
    start = time.perf_counter()
    out = SO.solve(W, F, model.transitions, BACKTRACK_K_MAX)
    ORACLE_SECONDS['backtrack', j] = time.perf_counter() - start
    return W, F, _freeze(out)


# -------------------------------------------------------------------------------------------------------------- draws
N_UNIFORM_ROWS = 4096
N_REPLAY = 1024
N_RAGGED_DRAWS = 200
RAGGED_DRAWN = (1, 5)
REPLAY_CASES = ('s1_T65', 's4_T65', 's4_T130', 's4_T70_sink', 's5_T70_source', 's2_T257', 's3_T321', 's4_T257')


def replay_inputs(name, k_max, T, S, n=N_REPLAY):
    """ (uniforms, ks): the first n rows of a seeded (4096, 2 k_max) array; k cycles over the k that have profiles """
    u = np.random.default_rng(sum(map(ord, name))).random((N_UNIFORM_ROWS, 2 * k_max))[:n]
    top = 0 if S == 1 else min(k_max, T - 1)
    return u, np.arange(n) % (top + 1)


def _replay(key, model, W, F, k_max, u, ks):
    start = time.perf_counter()
    G = SO.backward(W, model.transitions, k_max)
    out = DO.draws(W, F, G, model.transitions, ks, u)
    ORACLE_SECONDS[key] = time.perf_counter() - start
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def replay_answer(name):
    """ (uniforms, ks, want_start, want_state, fragile, consumed) of a case of REPLAY_CASES """
    model, x, W, F, k_max, nan = segment_case(name)
    u, ks = replay_inputs(name, k_max, len(x), model.nStates)
    return (u, ks) + _replay(('replay', name), model, W, F, k_max, u, ks)


@functools.lru_cache(maxsize=None)
def ragged_replay_inputs():
    """ uniforms (6, 200, 2 k_max) and ks (6, 200) of the ragged set: every trajectory is drawn in the one call """
    model, xs, tabs = ragged_case()
    pairs = [replay_inputs(f'ragged{j}', RAGGED_K_MAX, len(x), 4, N_RAGGED_DRAWS) for j, x in enumerate(xs)]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


@functools.lru_cache(maxsize=None)
def ragged_replay_answer(j):
    model, xs, tabs = ragged_case()
    u, ks = ragged_replay_inputs()
    return _replay(('ragged_replay', j), model, *tabs[j], RAGGED_K_MAX, u[j], ks[j])


# -------------------------------------------------------------------------------------------------------- enumeration
# name -> (S, T, transitions, k, marginals, companion length of the batch call or None)
ENUM_CASES = {
    's2_T18_k4': (2, 18, 'full', 4, True, 11),
    's2_T18_k8': (2, 18, 'full', 8, True, 11),
    's2_T18_k15': (2, 18, 'full', 15, True, 17),       # 2 C(17, 15) = 272 profiles, K1 = 16
    's2_T17_k15': (2, 17, 'full', 15, True, 15),      # 2 C(16, 15) = 32 profiles; the companion has none
    's4_T12_k5': (4, 12, 'full', 5, True, 9),          # 449 064 profiles
    's5_T30_k3_source': (5, 30, 'source', 3, True, 12),
    's4_T40_k4_ring': (4, 40, 'ring', 4, True, 13),
    's1_T20_k0': (1, 20, 'full', 0, True, 7),          # one profile
    's1_T20_k1': (1, 20, 'full', 1, True, 7),          # no profile: the empty result
    's4_T1025_k1': (4, 1025, 'full', 1, True, None),   # 12 288 profiles: three whole blocks of 4096
    's4_T1026_k1': (4, 1026, 'full', 1, True, None),   # the last block has 12
    's4_T1800_k1': (4, 1800, 'full', 1, True, None),   # 63 744 B of dynamic LDS under 64 KiB, 10 240 B static on top
    's4_T2048_k1': (4, 2048, 'full', 1, True, None),   # S T = 8192, the limit: 71 680 B of dynamic LDS
}
ENUM_LONG = ('s4_T1025_k1', 's4_T1026_k1', 's4_T1800_k1', 's4_T2048_k1')


@functools.lru_cache(maxsize=None)
def enum_case(name):
    """
    (model, x, companion or None, k).  The long cases have one dimension: their time is the set's table build, one
    factorisation of T rows per state and dimension (13 s at S = 4, T = 2048, d = 2 on an MI355X; the enumeration itself 0.03 s)
    """
    S, T, trans, k, marg, T2 = ENUM_CASES[name]
    model, x = make(S, T, (), trans, seed=9000 * S + T, d=1 if name in ENUM_LONG else 2)
    other = None
    if T2 is not None:
        other = C.random_traj(np.random.default_rng(9000 * S + T + 1), T2)
        other.setflags(write=False)
    return model, x, other, k


def enum_reference(model, x, k, logL_segments, key=None):
    """
    (`exact_oracle.reduce` of the model's own segment logLs, seg_start, seg_state, logL); the seconds of the whole answer,
    the enumeration, the logLs and the reduction, go to ORACLE_SECONDS[key]
    """
    import exact_oracle as X
    T = len(x)
    start = time.perf_counter()
    seg_start, seg_state = X.enumerate_profiles(T, k, model.transitions)
    step = 1 << 17
    logL = np.concatenate([logL_segments(seg_start[lo:lo + step], seg_state[lo:lo + step], x) for lo in range(0, len(seg_start), step)]) \
        if len(seg_start) else np.zeros(0)
    want = X.reduce(logL, seg_start, seg_state, T, model.nStates)
    if key is not None:
        ORACLE_SECONDS[key] = time.perf_counter() - start
    return want, seg_start, seg_state, logL
