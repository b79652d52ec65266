"""
Cases shared by the tests of the exact visit counts under a dwell-time prior (tests/test_dwell_visits.py,
tests/test_gpu_dwell_visits.py): the entries of `dwell_event_cases.ORACLE_CASES` that have a target, the wide cases, the ragged
batch and the cases at the seam between two tiles of n, with the answers of the oracle tests/dwell_visit_oracle.py (computed
once a session and shared; their arrays are read-only).
"""
import functools
import time

import numpy as np

import dwell_cases as DC
import dwell_event_cases as DEC
import dwell_visit_oracle as DV
import segment_cases as C

ORACLE_CASES = [case for case in DEC.ORACLE_CASES if case[5]]

ORACLE_SECONDS = {}     # what each oracle answer of this session took

case_id = DEC.case_id
oracle_case = DEC.oracle_case

# (case, target): every wide case of `dwell_event_cases.WIDE` that has a proper subset, with every target of its S.  T = 257 and
# 321 reach the third tile of n
WIDE_CASES = [(case, target) for case in DEC.WIDE for target in DEC.WIDE_TARGETS[case[0]]]

# (case, n_max) of the cuts on soft priors: around the kernel's seam of n (rows 62 | 63) and the seam of a 64-row tiling, and in
# the third tile
CUT_CASES = [((2, 130, (), 'bounded'), n) for n in (5, 62, 63, 64, 65)] + [((3, 321, (128,), 'markov'), 128)]
CUT_TARGETS = {2: (1,), 3: (0, 2)}

# the seam: all the posterior mass in the rows around n = 63 and 64 under the `flip` prior, G = {1}
SEAM_T = (125, 126, 127, 128, 129)
SEAM_N_MAX = (None, 62, 63, 64)
# the (n, last state) entries that hold the mass: a profile that starts in state 0 has T // 2 visits, one that starts in 1 has
# (T + 1) // 2, and the last state follows from the first and the parity of T
SEAM_MASS = {125: ((62, 0), (63, 1)), 126: ((63, 0), (63, 1)), 127: ((63, 0), (64, 1)), 128: ((64, 0), (64, 1)), 129: ((64, 0), (65, 1))}


def wide_id(item):
    case, target = item
    return DEC.wide_id(case) + '_G' + ''.join(map(str, target))


def _frozen(out):
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def _timed(key, solve):
    start = time.perf_counter()
    out = _frozen(solve())
    ORACLE_SECONDS[key] = time.perf_counter() - start
    return out


@functools.lru_cache(maxsize=None)
def wide_answer(case, target, n_max=None):
    """ `dwell_visit_oracle.solve` of an entry of WIDE_CASES; timed under (case, target, n_max) """
    _, _, prior, W, F = DC.oracle_case(case)
    return _timed((case, target, n_max), lambda: DV.solve(W, F, prior, target, n_max=n_max))


@functools.lru_cache(maxsize=None)
def ragged_answer(j, target):
    """ the answer on trajectory j of `dwell_cases.ragged_case` """
    _, prior, _, tabs = DC.ragged_case()
    return _timed(('ragged', j, target), lambda: DV.solve(*tabs[j], prior, target))


@functools.lru_cache(maxsize=None)
def oracle_answer(case):
    """ `dwell_visit_oracle.solve` of an entry of ORACLE_CASES: a dict per target """
    _, _, prior, W, F = oracle_case(*case[:4])
    start = time.perf_counter()
    out = {target: _frozen(DV.solve(W, F, prior, target, nan=case[4])) for target in case[5]}
    ORACLE_SECONDS[case] = time.perf_counter() - start
    return out


@functools.lru_cache(maxsize=None)
def seam_case(T):
    """ (model, x, prior, W, F): two states that alternate every frame, so that a profile of T frames has T // 2 or (T + 1) // 2 visits to state 1 """
    rng = np.random.default_rng(900 + T)
    model = C.random_model(rng, 2, T + 8)
    x = C.random_traj(rng, T, ())
    prior = DC.prior_of('flip', rng, 2, T + 5, T)
    W, F = C.tables(model, x)
    for a in (x, W, F):
        a.setflags(write=False)
    return model, x, prior, W, F


@functools.lru_cache(maxsize=None)
def seam_answer(T, n_max=None):
    _, _, prior, W, F = seam_case(T)
    return _timed(('seam', T, n_max), lambda: DV.solve(W, F, prior, (1,), n_max=n_max))
