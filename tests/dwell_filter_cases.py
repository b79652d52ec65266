"""
Cases shared by the tests of the exact online filter under a dwell-time prior (tests/test_dwell_filter.py,
tests/test_gpu_dwell_filter.py): the entries of `dwell_cases.ORACLE_CASES` that the GPU test holds to the oracle
tests/dwell_filter_oracle.py, the ragged batch, the ss_order-0 gap case and the oracle's answers.  An answer is computed once a
session and shared; its arrays are read-only.  tests/test_dwell_filter.py asserts the conditions on these inputs without a GPU.
"""
import functools
import time

import numpy as np

import bild_amd
import dwell_cases as DC
import dwell_filter_oracle as FO
import segment_cases as C

# the smallest shapes at the tile seams: one, two and three tiles, the last lane of a tile, the 8-wave stride with fewer than 8
# switches, the sixth tile; then S = 1 and 4 and non-geometric tables, then the hard priors
GPU_CASES = [(2, 1, (), 'markov'), (2, 2, (), 'minlength'), (2, 3, (), 'markov'), (2, 63, (5,), 'markov'),
             (2, 64, (), 'minlength'), (2, 65, (10, 40), 'markov'), (3, 65, (7,), 'minlength'), (2, 130, (64,), 'minlength'),
             (3, 193, (), 'markov'),
             (1, 65, (3,), 'markov'), (4, 64, (), 'minlength'), (4, 129, (64, 100), 'markov'), (4, 257, (100,), 'nongeometric'),
             (3, 321, (128,), 'markov'),
             (2, 130, (), 'bounded'), (2, 65, (), 'one_start'), (3, 130, (20,), 'absorbing'), (2, 70, (), 'flip'),
             (2, 70, (), 'impossible')]
assert all(case in DC.ORACLE_CASES for case in GPU_CASES)

# the truncation cases of the GPU test: the parent's own device code on every x[:b]
TRUNCATION_CASES = [(3, 65, (7,), 'minlength'), (2, 130, (), 'bounded')]

RAGGED_RUN_MAX = 40

ORACLE_SECONDS = {}


def run_max_of(T):
    """ every run length below T = 200; above, 70 cuts inside a tile and across a seam """
    return T if T < 200 else 70


def _solve(key, W, F, prior, **kw):
    start = time.perf_counter()
    out = FO.solve(W, F, prior, **kw)
    ORACLE_SECONDS[key] = time.perf_counter() - start
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle_answer(case):
    """ `dwell_filter_oracle.solve` of an entry of GPU_CASES, run_max = run_max_of(T) """
    _, _, prior, W, F = DC.oracle_case(case)
    return _solve(case, W, F, prior, run_max=run_max_of(case[1]))


@functools.lru_cache(maxsize=None)
def ragged_answers():
    _, prior, _, tabs = DC.ragged_case()
    return [_solve(('ragged', j), W, F, prior, run_max=RAGGED_RUN_MAX) for j, (W, F) in enumerate(tabs)]


@functools.lru_cache(maxsize=None)
def gap_case():
    """
    (model, x, prior, W, F): the ss_order-0 gap case of tests/test_gpu_dwell.py::test_order0_gap_against_oracle, T = 70, frames
    60 ... 67 missing in dimension 0: a later ss_order-0 segment inside them has no valid value
    """
    T = 70
    rng = np.random.default_rng(7)
    model = bild_amd.GenericGaussianModel([[(np.append(np.arange(T + 8) * 0.5 + 0.1, 50.0), 0.3 * s, 0),
                                            (np.arange(T + 8) * (0.5 + s), 0.0, 1)] for s in range(2)])
    x = C.random_traj(rng, T)
    x[60:68, 0] = np.nan
    prior = DC.make_prior('markov', rng, 2, T)
    W, F = C.tables(model, x)
    for a in (x, W, F):
        a.setflags(write=False)
    return model, x, prior, W, F


@functools.lru_cache(maxsize=None)
def gap_answer(nan):
    _, _, prior, W, F = gap_case()
    return _solve(('gap', nan), W, F, prior, nan=nan, run_max=70)
