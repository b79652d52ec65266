"""
Cases shared by the tests of `kalman_kernel<L>` (csrc/kalman.hip) and `sens_kernel<L, P>` (csrc/sens.hip) at every lane width
and every number of tangents (tests/test_modal_cases.py, tests/test_gpu_modal_configs.py): models of exactly n effective modes,
one ragged batch of five trajectories whose covariance chains differ, the candidates on it, and the answers of the NumPy
oracles tests/kalman_oracle.py and tests/sensitivity_oracle.py.  An oracle answer is computed once a session and shared
(`kalman_answer`, `sens_answer`); its arrays are read-only.  tests/test_modal_cases.py asserts the conditions on these inputs
without a GPU.
"""
import functools
import time

import numpy as np

import bild_amd
import kalman_oracle as KO
import sensitivity_oracle as SO
from bild_amd.profiles import segments_from_states

D0, K0, F0 = 1.3, 2.0, 1.0      # the point of the family: Rouse D and k, the scale f of the added force
LOOPS = [None, (0, -1), (1, -2)]
MODES = (2, 8, 9, 16, 17, 32)   # each lane width at its emptiest and at its fullest (n = 1 is left out: the oracle's smoothed
                                # variance of a one-bead chain is exactly 0)
# At n = 2 and 3 the B of the three states commute (a ring and a chain of three beads share their eigenvectors, and at n = 2
# both loops are the one bond there is): every basis change is the identity up to order and sign, and the emptiest 8-lane
# case cannot see a wrong one.  n = 4 is the smallest chain whose three states have three different bases; it runs beside n = 2.
MODES_EXTRA = (4,)
P_MAX = 4


def lanes(n):
    """ lanes of a task: the smallest of 8, 16, 32 that holds the n effective modes (kalman.cpp, sens.cpp) """
    return 8 if n <= 8 else 16 if n <= 16 else 32


# (T, missing frames) of trajectories A ... E, and their localization errors by dimension count.  d = 3 is the batch of every
# configuration: one, two and three chains in one call, so that the `e >= td.dstar` tasks of A, B, D and E leave the wavefront
# beside live ones.  d = 5: four equal errors split into chains of three and one, plus a third chain (B, E); five equal ones
# into three and two (A, D); C has five dimensions on three variances.
TRAJS = ((40, ()), (40, (0,) + tuple(range(17, 23)) + (39,)), (23, (5,)), (1, ()), (2, (1,)))
ERRORS = {
    1: ((0.3,), (0.5,), (0.2,), (0.3,), (0.5,)),
    2: ((0.3, 0.3), (0.3, 0.5), (0.2, 0.4), (0.3, 0.3), (0.3, 0.5)),
    3: ((0.3, 0.3, 0.3), (0.3, 0.5, 0.3), (0.2, 0.4, 0.6), (0.3, 0.3, 0.3), (0.3, 0.5, 0.3)),
    5: ((0.3,) * 5, (0.3, 0.3, 0.3, 0.3, 0.5), (0.2, 0.4, 0.6, 0.2, 0.4), (0.3,) * 5, (0.3, 0.3, 0.3, 0.3, 0.5)),
}
N_CHAINS = {1: (1, 1, 1, 1, 1), 2: (1, 2, 2, 1, 2), 3: (1, 2, 3, 1, 2), 5: (2, 3, 3, 2, 3)}   # dstar of A ... E

SIX = (0, 1, 2, 0, 2, 1, 0)     # all six ordered changes of three states
SIX_AT = {40: (4, 9, 19, 26, 31, 36), 23: (2, 5, 9, 13, 17, 21)}   # frame 19 lies inside B's gap, frame 5 is C's missing frame


def profiles_of(T, S):
    """ the candidate profiles of a trajectory of T frames, where its length allows them """
    if S == 1:
        return [np.zeros(T, dtype=np.int32)]
    out = []
    if T in SIX_AT:
        st = np.zeros(T, dtype=np.int32)
        for at, s in zip(SIX_AT[T], SIX[1:]):
            st[at:] = s
        out.append(st)
    if T >= 6:      # the adjacent switches of test_gpu_sensitivity.test_generated_against_oracle
        st = np.zeros(T, dtype=np.int32)
        st[3], st[4], st[5:] = 1, 2, 1
        out.append(st)
    if T >= 2:      # a switch at frame 1 and one at frame T - 1 (T = 2: they are one)
        st = np.zeros(T, dtype=np.int32)
        st[1:] = 1
        st[T - 1] = 2 if T > 2 else 1
        out.append(st)
    out.append(np.full(T, S - 1, dtype=np.int32))
    return out


def candidates(S):
    """ (profiles, traj_id), interleaved by trajectory: neighbours in a wavefront differ in T, chains and state """
    per = [profiles_of(T, S) for T, _ in TRAJS]
    cands, tid = [], []
    for c in range(max(len(p) for p in per)):
        for j, p in enumerate(per):
            if c < len(p):
                cands.append(p[c])
                tid.append(j)
    return cands, np.array(tid, dtype=np.int32)


def segments(cands):
    """ run-length encoded (seg_start, seg_state) of profiles of different lengths: the padding repeats the last segment """
    T = max(len(c) for c in cands)
    full = np.stack([np.concatenate([c, np.full(T - len(c), c[-1], dtype=np.int32)]) for c in cands])
    return segments_from_states(full)


class Config:
    """ the arrays, derivatives, data and candidates of one (n, S, d); everything read-only """

    def __init__(self, n, S, d):
        self.n, self.S, self.d = n, S, d
        rng = np.random.default_rng(10000 * S + 100 * d + n)
        self.family = SO.rouse_family(n, LOOPS[:S], d)
        self.force = {'G': 0.2 * rng.standard_normal((S, n, d)), 'M0': 0.3 * rng.standard_normal((S, n, d))}
        self.w = rng.standard_normal(n)
        self.errs = np.array(ERRORS[d])
        self.trajs = []
        for T, missing in TRAJS:
            x = 2.0 * rng.standard_normal((T, d))
            x[list(missing)] = np.nan
            self.trajs.append(x)
        self.cands, self.tid = candidates(S)
        self.seg_start, self.seg_state = segments(self.cands)
        self.arrays = self.arrays_at(D0, K0, F0)
        # the four directions: D, k, f, and the localization error (ds2 = 2 sigma per trajectory and dimension, nothing else)
        rouse = self.family[1](D0, K0)
        z = {key: np.zeros((P_MAX,) + v.shape[1:]) for key, v in rouse.items()}
        for key, v in rouse.items():
            z[key][:2] = v
        z['dG'][2] += self.force['G']
        z['dM0'][2] += self.force['M0']
        self.derivs = z
        self.ds2 = np.zeros((P_MAX, len(self.trajs), d))
        self.ds2[3] = 2 * self.errs
        for a in [self.w, self.errs, self.tid, self.seg_start, self.seg_state, self.ds2] + self.trajs + self.cands \
                + list(self.arrays.values()) + list(self.derivs.values()) + list(self.force.values()):
            a.setflags(write=False)

    def arrays_at(self, D, k, f):
        a = {key: np.array(v, dtype=np.float64) for key, v in self.family[0](D, k).items()}
        a['G'] = a['G'] + f * self.force['G']
        a['M0'] = a['M0'] + f * self.force['M0']
        return a

    def derivatives(self, P):
        """ the `derivatives=` argument of logL_sensitivities for the first P directions """
        out = {key: v[:P] for key, v in self.derivs.items()}
        out['ds2'] = self.ds2[:P]
        return out

    def model(self):
        """ a fresh model: the errors sit on the trajectories (`trajectories`), so that dstar differs inside one set """
        return bild_amd.MultiStateRouse.from_arrays(**self.arrays, measurement=self.w, localization_error=None)

    def trajectories(self):
        return [bild_amd.Trajectory(x, localization_error=err) for x, err in zip(self.trajs, self.errs)]

    def var_scale(self):
        """ `test_gpu_kalman._var_scale` with the largest error of the set """
        return max(float(self.w @ C0 @ self.w) for C0 in self.arrays['C0']) + float(np.max(self.errs) ** 2)

    def data(self):
        """ every value of the set in one array: the scale of the means' bar """
        return np.concatenate([x.reshape(-1) for x in self.trajs])


@functools.lru_cache(maxsize=None)
def config(n, S=3, d=3):
    return Config(n, S, d)


# what the GPU file runs: (n, S, d) for the smoother and (n, S, d, P) for the sensitivities
KALMAN_CONFIGS = [(n, 3, 3) for n in MODES + MODES_EXTRA] + [(2, 1, 3), (9, 3, 1), (9, 3, 2), (9, 3, 5)]
SENS_CONFIGS = ([(n, 3, 3, P) for n in (2, 8, 9, 16) + MODES_EXTRA for P in range(P_MAX + 1)] + [(17, 3, 3, 0), (32, 3, 3, 0)]
                + [(2, 1, 3, P) for P in (0, P_MAX)] + [(9, 3, 1, 2), (9, 3, 2, 2), (9, 3, 5, 2)])
BIT_CONFIGS = [(17, 3, 3, 0), (16, 3, 3, 4)]

ORACLE_SECONDS = {}     # what each oracle answer of this session took


def _freeze(arrs):
    for a in arrs:
        a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def kalman_answer(n, S=3, d=3):
    """ `kalman_oracle.filter_smoother` of every candidate with its own trajectory's errors: dict of (n_cand, T_max, d) """
    c = config(n, S, d)
    start = time.perf_counter()
    T_max = max(len(x) for x in c.trajs)
    res = {k: np.full((len(c.cands), T_max, d), np.nan) for k in KO.OUTPUTS}
    for r, (st, j) in enumerate(zip(c.cands, c.tid)):
        o = KO.filter_smoother(c.arrays, c.w, c.errs[j], c.trajs[j], st)
        for k in KO.OUTPUTS:
            res[k][r, :len(st)] = o[k]
    ORACLE_SECONDS[('kalman', n, S, d)] = time.perf_counter() - start
    _freeze(res.values())
    return res


@functools.lru_cache(maxsize=None)
def sens_answer(n, S=3, d=3, P=0):
    """ `sensitivity_oracle.batch` of the first P directions: (logL (n_cand,), grad (n_cand, P), fisher (n_cand, P, P)) """
    c = config(n, S, d)
    start = time.perf_counter()
    derivs = {k: v[:P] for k, v in c.derivs.items()} if P else None
    out = SO.batch(c.arrays, c.w, c.errs, c.trajs, c.cands, traj_id=c.tid, derivs=derivs, ds2=c.ds2[:P] if P else None)
    ORACLE_SECONDS[('sens', n, S, d, P)] = time.perf_counter() - start
    _freeze(out)
    return out


def expected_nan(c):
    """ per output of the smoother: where the oracle's answer must be NaN (behind a trajectory's end; `innov` on missing frames) """
    T_max = max(len(x) for x in c.trajs)
    tail = np.zeros((len(c.cands), T_max, c.d), dtype=bool)
    gone = np.zeros_like(tail)
    for r, j in enumerate(c.tid):
        T = len(c.trajs[j])
        tail[r, T:] = True
        gone[r, :T] = np.any(np.isnan(c.trajs[j]), axis=1)[:, None]
    return {k: (tail | gone) if k == 'innov' else tail for k in KO.OUTPUTS}
