"""
Cases shared by the tests of the exact window support under a dwell-time prior (tests/test_dwell_windows.py,
tests/test_gpu_dwell_windows.py): trajectories of `dwell_event_cases.oracle_case` with windows that place the edges of the
kernel of csrc/gauss_dwellwin.hip, and the answers of the oracle tests/dwell_window_oracle.py (computed once a session and
shared; their arrays are read-only).  A case holds at most 16 windows, so a trajectory's windows come in parts.
"""
import functools
import time

import numpy as np

import dwell_event_cases as DEC
import dwell_window_oracle as DW

TARGETS = {2: ((1,), (0,)), 3: ((1,), (0, 2))}
MAX_WINDOWS = 16

# (S, T, missing frames, prior kind, nan mode): T around the 64-frame tiles of the window chain; S = 3 (the jump 0 -> 2
# forbidden) at 65 and 193; isolated missing frames; Markov and minimum-length priors; 'order0_gap':
# `segment_sensitivity_cases.order0_gap_case` with the gap across the first tile's edge, in both NaN modes
TRAJECTORIES = [(2, 1, (), 'markov', 'propagate'), (2, 2, (), 'minlength', 'propagate'), (2, 3, (), 'markov', 'propagate'),
                (2, 64, (), 'minlength', 'propagate'), (2, 65, (10, 40), 'markov', 'propagate'), (3, 65, (7,), 'minlength', 'propagate'),
                (2, 130, (64,), 'minlength', 'propagate'), (2, 193, (3, 100), 'markov', 'propagate'),
                (3, 193, (64,), 'markov', 'propagate'),
                (2, 130, 'order0_gap', 'markov', 'propagate'), (2, 130, 'order0_gap', 'markov', 'omit')]


def spans(T):
    """
    the windows [u, v) of a trajectory of T frames, as far as they fit: one frame at either end and the whole trajectory;
    chains of 63, 64 and 65 frames (v - u - 1: the last tile of the chain full but for one lane, full, and one frame into the
    next tile) from u = 0 (no alpha in the chain's head) and from u = 1, 63, 64; a chain of 129 frames (three tiles) that ends
    inside the trajectory and one that ends at T (the closure sees gamma = 0 alone); short windows, two of which overlap
    """
    out = [(0, 1), (T - 1, T), (0, T)]
    out += [(u, u + n + 1) for n in (63, 64, 65) for u in (0, 1, 63, 64)]
    out += [(0, 130), (T - 130, T), (10, 40), (30, 50), (1, 2), (T - 2, T - 1)]
    seen = []
    for u, v in out:
        if 0 <= u < v <= T and (u, v) not in seen:
            seen.append((u, v))
    return seen


def windows_of(S, T):
    """ every span with every target of TARGETS[S], as (u, v, target) """
    return [(u, v, target) for u, v in spans(T) for target in TARGETS[S]]


# (S, T, missing, kind, nan, part)
ORACLE_CASES = [traj + (part,) for traj in TRAJECTORIES for part in range(-(-len(windows_of(traj[0], traj[1])) // MAX_WINDOWS))]

ORACLE_SECONDS = {}     # what each oracle answer of this session took

oracle_case = DEC.oracle_case


def case_id(case):
    S, T, missing, kind, nan, part = case
    return f"S{S}_T{T}_{kind}_{nan}" + ('_order0_gap' if missing == 'order0_gap' else '') + f"_part{part}"


def case_windows(case):
    S, T, part = case[0], case[1], case[5]
    return windows_of(S, T)[part * MAX_WINDOWS:(part + 1) * MAX_WINDOWS]


@functools.lru_cache(maxsize=None)
def oracle_answer(case):
    """ `dwell_window_oracle.solve` of an entry of ORACLE_CASES on its windows """
    _, _, prior, W, F = oracle_case(*case[:4])
    start = time.perf_counter()
    out = DW.solve(W, F, prior, case_windows(case), nan=case[4])
    ORACLE_SECONDS[case] = time.perf_counter() - start
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out
