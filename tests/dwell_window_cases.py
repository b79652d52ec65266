"""
Cases shared by the tests of the exact window support under a dwell-time prior (tests/test_dwell_windows.py,
tests/test_gpu_dwell_windows.py): trajectories of `dwell_event_cases.oracle_case` with windows that place the edges of the
kernel of csrc/gauss_dwellwin.hip, and the answers of the oracle tests/dwell_window_oracle.py (computed once a session and
shared; their arrays are read-only).  A case holds at most 16 windows, so a trajectory's windows come in parts.
"""
import functools
import time

import numpy as np

import dwell_cases as DC
import dwell_event_cases as DEC
import dwell_window_oracle as DW

TARGETS = {2: ((1,), (0,)), 3: ((1,), (0, 2)), 4: ((0,), (1, 3), (0, 1, 2))}
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


def wide_spans(T):
    """
    `spans(T)` and, from T = 257 on: chains whose head alpha(c <= u) lies in tile 3 or 4 and whose closure has the one end
    frame T, (192, T), (255, T) and (256, T); a chain of 64 frames that ends one frame before T, so that the closure has two end
    frames; and (191, 257), (192, 258), clipped to the trajectory: closures with 65 and 64 end frames at T = 321.  (0, T), a
    chain of five or six tiles, is `spans`' own
    """
    out = spans(T)
    if T >= 257:
        for u, v in ((0, T), (192, T), (255, T), (256, T), (T - 66, T - 1), (191, min(257, T)), (192, min(258, T))):
            if 0 <= u < v <= T and (u, v) not in out:
                out.append((u, v))
    return out


def wide_windows_of(case):
    """ every span of `wide_spans` with every target of the case's S, as (u, v, target) """
    return [(u, v, target) for u, v in wide_spans(case[1]) for target in DEC.WIDE_TARGETS[case[0]]]


# (case, part): the wide cases of `dwell_event_cases.WIDE` that have a proper subset, their windows in parts of MAX_WINDOWS
WIDE_CASES = [(case, part) for case in DEC.WIDE if case[0] > 1 for part in range(-(-len(wide_windows_of(case)) // MAX_WINDOWS))]


def wide_id(item):
    case, part = item
    return DEC.wide_id(case) + f"_part{part}"


def wide_windows(item):
    case, part = item
    return wide_windows_of(case)[part * MAX_WINDOWS:(part + 1) * MAX_WINDOWS]


def _solve(key, W, F, prior, windows):
    start = time.perf_counter()
    out = DW.solve(W, F, prior, windows)
    ORACLE_SECONDS[key] = time.perf_counter() - start
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def wide_answer(item):
    """ `dwell_window_oracle.solve` of an entry of WIDE_CASES on its windows """
    _, _, prior, W, F = DC.oracle_case(item[0])
    return _solve(item, W, F, prior, wide_windows(item))


def ragged_windows(T):
    """ the windows of a trajectory of `dwell_cases.ragged_case`: `spans(T)`, which keeps what fits, with both ragged targets """
    return [(u, v, target) for u, v in spans(T) for target in DEC.RAGGED_TARGETS]


@functools.lru_cache(maxsize=None)
def ragged_answer(j):
    _, prior, xs, tabs = DC.ragged_case()
    return _solve(('ragged', j), *tabs[j], prior, ragged_windows(len(xs[j])))


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
