"""
Cases shared by the tests of exact fixed-lag smoothing under a dwell-time prior (tests/test_dwell_lag.py,
tests/test_gpu_dwell_lag.py): (entry of `dwell_cases.ORACLE_CASES`, lag) pairs that the GPU test holds to the oracle
tests/dwell_lag_oracle.py, the ragged batch, the ss_order-0 gap case and the oracle's answers.  An answer is computed once a
session and shared; its arrays are read-only.  tests/test_dwell_lag.py asserts the conditions on these inputs without a GPU.
"""
import functools
import time

import numpy as np

import dwell_cases as DC
import dwell_filter_cases as FC
import dwell_lag_oracle as LO

LAG_MAX = 63

# T = 1, 2, 3: the windows are clipped at frame 0 and lag >= T
GPU_CASES = [(case, lag) for case in ((2, 1, (), 'markov'), (2, 2, (), 'minlength'), (2, 3, (), 'markov')) for lag in (0, 1, 5)]
# the window is exactly one wavefront, and its left edge crosses frame 0 at u = 64
GPU_CASES += [((2, 63, (5,), 'markov'), 63), ((2, 64, (), 'minlength'), 63), ((2, 65, (10, 40), 'markov'), 63)]
# the shortest window with a chain, and one lane short of a wavefront; three states
GPU_CASES += [((2, 65, (10, 40), 'markov'), 1), ((2, 65, (10, 40), 'markov'), 62), ((3, 65, (7,), 'minlength'), 8)]
# BOUND = 70 exceeds the window, so the bases carry weight; two tiles of bases
GPU_CASES += [((2, 130, (), 'bounded'), 63), ((2, 130, (), 'bounded'), 6), ((2, 130, (64,), 'minlength'), 63)]
# S = 1 and 4, non-geometric tables, the bases over several tiles
GPU_CASES += [((1, 65, (3,), 'markov'), 10), ((4, 64, (), 'minlength'), 63), ((4, 129, (64, 100), 'markov'), 63),
              ((4, 257, (100,), 'nongeometric'), 63), ((3, 321, (128,), 'markov'), 20)]
# the hard priors
GPU_CASES += [((2, 65, (), 'one_start'), 5), ((3, 130, (20,), 'absorbing'), 5), ((2, 70, (), 'flip'), 5), ((2, 70, (), 'impossible'), 5)]
assert all(case in DC.ORACLE_CASES and 0 <= lag <= LAG_MAX for case, lag in GPU_CASES)

# the truncation cases of the GPU test: the parent's own device code on every x[:u]
TRUNCATION_CASES = [((3, 65, (7,), 'minlength'), 63), ((2, 130, (), 'bounded'), 40)]

RAGGED_LAG = 30
GAP_LAG = 12

ORACLE_SECONDS = {}


def _solve(key, W, F, prior, lag, **kw):
    start = time.perf_counter()
    out = LO.solve(W, F, prior, lag, **kw)
    ORACLE_SECONDS[key] = time.perf_counter() - start
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle_answer(case, lag):
    """ `dwell_lag_oracle.solve` of an entry of `dwell_cases.ORACLE_CASES` """
    _, _, prior, W, F = DC.oracle_case(case)
    return _solve((case, lag), W, F, prior, lag)


@functools.lru_cache(maxsize=None)
def ragged_answers():
    _, prior, _, tabs = DC.ragged_case()
    return [_solve(('ragged', j), W, F, prior, RAGGED_LAG) for j, (W, F) in enumerate(tabs)]


@functools.lru_cache(maxsize=None)
def gap_answer(nan):
    """ the ss_order-0 gap case of `dwell_filter_cases.gap_case` at lag GAP_LAG """
    _, _, prior, W, F = FC.gap_case()
    return _solve(('gap', nan), W, F, prior, GAP_LAG, nan=nan)


def cut_of(T, t, lag):
    """ the truncation that column `lag` of frame t speaks of """
    return min(t + lag + 1, T)


def column_steps(log_lagged, lag):
    """
    The largest, over the frames, of the smallest pairwise distance (in probability, maximum over the states) between the
    columns 0, 1 and `lag` of a frame, among the frames where these columns speak of as many different truncations as any
    frame of the trajectory has; and that number of truncations.  A shifted or repeated column cannot pass where it is > 0.
    """
    S, T, n = log_lagged.shape
    cols = sorted({0, min(1, lag), lag})
    n_cuts = [len({cut_of(T, t, l) for l in cols}) for t in range(T)]
    most = max(n_cuts)
    p = np.exp(log_lagged)
    best = 0.0
    for t in range(T):
        if n_cuts[t] < most or most < 2 or np.isnan(p[:, t, cols]).any():
            continue
        reps = {cut_of(T, t, l): l for l in cols}       # one column per truncation
        ls = sorted(reps.values())
        gaps = [np.max(np.abs(p[:, t, i] - p[:, t, j])) for k, i in enumerate(ls) for j in ls[k + 1:]]
        best = max(best, min(gaps))
    return best, most
