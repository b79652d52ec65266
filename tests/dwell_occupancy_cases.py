"""
Cases shared by the tests of the exact posterior of the looped time under a dwell-time prior (tests/test_dwell_occupancy.py,
tests/test_gpu_dwell_occupancy.py): the entries of `dwell_event_cases.ORACLE_CASES` that have a target, with the answers of the
oracle tests/dwell_occupancy_oracle.py (computed once a session and shared; their arrays are read-only).  T = 63, 64 and 65 sit
around the second tile of n, which opens at end frame b = 64: n = 0 .. b is b + 1 values.
"""
import functools
import time

import numpy as np

import dwell_event_cases as DEC
import dwell_occupancy_oracle as DQ

ORACLE_CASES = [case for case in DEC.ORACLE_CASES if case[5]]

ORACLE_SECONDS = {}     # what each oracle answer of this session took

case_id = DEC.case_id
oracle_case = DEC.oracle_case


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
