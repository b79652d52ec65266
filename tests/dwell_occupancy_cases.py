"""
Cases shared by the tests of the exact posterior of the looped time under a dwell-time prior (tests/test_dwell_occupancy.py,
tests/test_gpu_dwell_occupancy.py): the entries of `dwell_event_cases.ORACLE_CASES` that have a target, with the answers of the
oracle tests/dwell_occupancy_oracle.py (computed once a session and shared; their arrays are read-only).  T = 63, 64 and 65 sit
around the second tile of n, which opens at end frame b = 64: n = 0 .. b is b + 1 values.
"""
import functools
import time

import numpy as np

import dwell_cases as DC
import dwell_event_cases as DEC
import dwell_occupancy_oracle as DQ

ORACLE_CASES = [case for case in DEC.ORACLE_CASES if case[5]]

ORACLE_SECONDS = {}     # what each oracle answer of this session took

case_id = DEC.case_id
oracle_case = DEC.oracle_case


# (case, target): every wide case of `dwell_event_cases.WIDE` that has a proper subset, with every target of its S
WIDE_CASES = [(case, target) for case in DEC.WIDE for target in DEC.WIDE_TARGETS[case[0]]]


def wide_id(item):
    case, target = item
    return DEC.wide_id(case) + '_G' + ''.join(map(str, target))


@functools.lru_cache(maxsize=None)
def wide_answer(case, target):
    """ `dwell_occupancy_oracle.solve` of an entry of WIDE_CASES; timed under (case, target) """
    _, _, prior, W, F = DC.oracle_case(case)
    start = time.perf_counter()
    out = DQ.solve(W, F, prior, target)
    ORACLE_SECONDS[case, target] = time.perf_counter() - start
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def ragged_answer(j, target):
    """ the answer on trajectory j of `dwell_cases.ragged_case` """
    _, prior, _, tabs = DC.ragged_case()
    start = time.perf_counter()
    out = DQ.solve(*tabs[j], prior, target)
    ORACLE_SECONDS['ragged', j, target] = time.perf_counter() - start
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle_answer(case):
    """ `dwell_occupancy_oracle.solve` of an entry of ORACLE_CASES: a dict per target """
    _, _, prior, W, F = oracle_case(*case[:4])
    start = time.perf_counter()
    out = {target: DQ.solve(W, F, prior, target, nan=case[4]) for target in case[5]}
    ORACLE_SECONDS[case] = time.perf_counter() - start
    for answer in out.values():
        for a in answer.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return out
