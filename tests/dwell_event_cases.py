"""
Cases shared by the tests of the exact switch counts and first-contact times under a dwell-time prior
(tests/test_dwell_events.py, tests/test_gpu_dwell_events.py): the cases that the GPU test holds to the oracle
tests/dwell_event_oracle.py with the oracle's answers (computed once a session and shared; their arrays are read-only).
"""
import functools
import time

import numpy as np

import dwell_cases as DC
import dwell_event_oracle as DE
import segment_cases as C
import segment_sensitivity_cases as SC

# (S, T, missing frames, prior kind, nan mode, targets, k_max) of the cases that tests/test_gpu_dwell_events.py holds to the
# oracle.  T around the 64-frame tiles of the level kernel and of the 8-wave forward pass; S = 2 throughout, S = 1 (the counts
# alone: no proper subset of one state), 3 and 4 at 65, S = 3 at 193; isolated missing frames; Markov and minimum-length
# priors.  'order0_gap': `segment_sensitivity_cases.order0_gap_case` with the gap across the first tile's edge, in both NaN
# modes.  k_max None: complete; at T = 130 also k_max = 5, for log_tail.
ORACLE_CASES = [(2, 1, (), 'markov', 'propagate', ((1,),), None), (2, 2, (), 'minlength', 'propagate', ((1,),), None),
                (2, 3, (), 'markov', 'propagate', ((1,),), None), (2, 63, (5,), 'markov', 'propagate', ((1,),), None),
                (2, 64, (), 'minlength', 'propagate', ((1,),), None), (2, 65, (10, 40), 'markov', 'propagate', ((1,),), None),
                (1, 65, (20,), 'markov', 'propagate', (), None), (3, 65, (7,), 'minlength', 'propagate', ((2,), (0, 2)), None),
                (4, 65, (3,), 'markov', 'propagate', ((1, 3),), None),
                (2, 130, (64,), 'minlength', 'propagate', ((1,),), None), (2, 130, (64,), 'minlength', 'propagate', (), 5),
                (2, 193, (3, 100), 'markov', 'propagate', ((1,),), None), (3, 193, (64,), 'markov', 'propagate', ((2,), (0, 2)), None),
                (2, 130, 'order0_gap', 'markov', 'propagate', ((1,),), None), (2, 130, 'order0_gap', 'markov', 'omit', ((1,),), None)]

ORACLE_SECONDS = {}     # what each oracle answer of this session took

# The wide cases, shared by the three calls (switch counts and first contact, occupancy, windows): entries of
# `dwell_cases.ORACLE_CASES`, so that model, data and prior are `dwell_cases.oracle_case`'s.  Each is the smallest shape at
# which its edge exists: S = 4 on one tile, across two seams and on a fifth tile (level launches from tile0 = 4, the fifth tile
# of n) under non-monotone tables; exactly four tiles against four and one frame, with a missing frame at the seam; six tiles;
# non-geometric tables at the shapes that stood; S = 1 over two seams (the counts alone); and the hard priors: a switch forced
# across every seam ('bounded'), log_init, log_jump and log_dwell at -inf ('one_start', 'absorbing', 'flip').
WIDE = [(4, 64, (), 'minlength'), (4, 129, (64, 100), 'markov'), (4, 257, (100,), 'nongeometric'),
        (2, 256, (), 'markov'), (2, 257, (255,), 'minlength'), (3, 321, (128,), 'markov'),
        (2, 65, (), 'nongeometric'), (3, 193, (3,), 'nongeometric'), (1, 130, (), 'nongeometric'),
        (2, 130, (), 'bounded'), (3, 193, (), 'bounded'),
        (2, 65, (), 'one_start'), (3, 130, (20,), 'absorbing'), (2, 70, (), 'flip')]
assert all(case in DC.ORACLE_CASES for case in WIDE)
WIDE_TARGETS = {1: (), 2: ((1,), (0,)), 3: ((2,), (0, 2), (1,)), 4: ((0,), (1, 3), (0, 1, 2))}

# (case, k_max) of the switch counts: complete on every case; cut at the last level of tile 0, the first of tile 1 and the
# first of tile 4, for log_tail
WIDE_CASES = [(case, None) for case in WIDE] + [((2, 130, (), 'bounded'), k) for k in (63, 64, 65)] + [((3, 321, (128,), 'markov'), 256)]

# what a case is there for: its -inf entries are compared as well as its finite ones
HARD = ('minlength', 'bounded', 'one_start', 'absorbing', 'flip')


def case_id(case):
    S, T, missing, kind, nan, _, k_max = case
    return f"S{S}_T{T}_{kind}_{nan}" + ('_order0_gap' if missing == 'order0_gap' else '') + ('' if k_max is None else f"_k{k_max}")


def wide_id(case):
    """ of an entry of WIDE or of WIDE_CASES """
    (S, T, _, kind), k_max = case if len(case) == 2 else (case, None)
    return f"S{S}_T{T}_{kind}" + ('' if k_max is None else f"_k{k_max}")


@functools.lru_cache(maxsize=None)
def oracle_case(S, T, missing, kind):
    """ (model, x, prior, W, F) of an entry of ORACLE_CASES (the NaN mode, the targets and k_max do not change them) """
    rng = np.random.default_rng(2700 + 1000 * S + T)
    if missing == 'order0_gap':
        model, x = SC.order0_gap_case(rng, T, gap=(61, 67))
    else:
        model = C.random_model(rng, S, T + 8)
        x = C.random_traj(rng, T, missing)
    prior = DC.make_prior(kind, rng, S, T + 5)
    W, F = C.tables(model, x)
    for a in (x, W, F):
        a.setflags(write=False)
    return model, x, prior, W, F


@functools.lru_cache(maxsize=None)
def oracle_answer(case):
    """ `dwell_event_oracle.solve` of an entry of ORACLE_CASES: a dict per target ('counts' where the case has none) """
    _, _, prior, W, F = oracle_case(*case[:4])
    start = time.perf_counter()
    out = {target: DE.solve(W, F, prior, target=target, k_max=case[6], nan=case[4]) for target in case[5]}
    if not out:
        out['counts'] = DE.solve(W, F, prior, k_max=case[6], nan=case[4])
    ORACLE_SECONDS[case] = time.perf_counter() - start
    for answer in out.values():
        for a in answer.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return out


def _frozen(answer):
    for a in answer.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return answer


def _timed(key, solve):
    start = time.perf_counter()
    out = _frozen(solve())
    ORACLE_SECONDS[key] = time.perf_counter() - start
    return out


@functools.lru_cache(maxsize=None)
def wide_counts(case, k_max=None):
    """ `dwell_event_oracle.solve`'s counts of an entry of WIDE; timed under (case, 'counts', k_max) """
    _, _, prior, W, F = DC.oracle_case(case)
    return _timed((case, 'counts', k_max), lambda: DE.solve(W, F, prior, k_max=k_max))


@functools.lru_cache(maxsize=None)
def wide_contact(case, target):
    """ `dwell_event_oracle.solve`'s log_first and log_never of an entry of WIDE (level 0 of the counts alone); timed under (case, target) """
    _, _, prior, W, F = DC.oracle_case(case)
    return _timed((case, target), lambda: DE.solve(W, F, prior, target=target, k_max=0))


RAGGED_TARGETS = ((1, 3), (0,))


@functools.lru_cache(maxsize=None)
def ragged_counts(j):
    """ the counts of trajectory j of `dwell_cases.ragged_case`, at its own complete k_max """
    _, prior, _, tabs = DC.ragged_case()
    return _timed(('ragged', j, 'counts'), lambda: DE.solve(*tabs[j], prior))


@functools.lru_cache(maxsize=None)
def ragged_contact(j, target):
    _, prior, _, tabs = DC.ragged_case()
    return _timed(('ragged', j, target), lambda: DE.solve(*tabs[j], prior, target=target, k_max=0))


NINE_MORE = (65, 130, 3)


@functools.lru_cache(maxsize=None)
def nine_trajectories():
    """
    (model, prior, trajectories): the six of `dwell_cases.ragged_case` and three more from the same generator.  Nine is three
    workgroups of the first-contact kernel (a wave per trajectory, four waves), the last one with a single wave
    """
    model, prior, xs, _ = DC.ragged_case()
    rng = np.random.default_rng(4002)
    more = [C.random_traj(rng, T) for T in NINE_MORE]
    for a in more:
        a.setflags(write=False)
    return model, prior, list(xs) + more


# name: (S, T, the missing frame, prior kind) of the cases at which the three oracles are held to the enumeration of every
# profile beyond S = 2 and 3 under the soft priors: four states, one state (the counts alone: no proper subset), and the hard
# priors.  'bounded3': non-geometric tables cut to -inf beyond 3 frames (`dwell_cases.BOUND` does not bind at these lengths).
SMALL = {'s4_nongeometric': (4, 6, 2, 'nongeometric'), 's4_minlength': (4, 6, 3, 'minlength'), 's1': (1, 6, 2, 'nongeometric'),
         's2_bounded3': (2, 9, 4, 'bounded3'), 'flip': (2, 8, 3, 'flip'), 'absorbing': (3, 7, 2, 'absorbing'), 'one_start': (3, 7, 4, 'one_start')}
SMALL_TARGETS = {1: (), 2: ((1,), (0,)), 3: ((2,), (0, 2), (1,)), 4: ((0,), (1, 3), (0, 1, 2))}


@functools.lru_cache(maxsize=None)
def small_case(name):
    """ (model, x, prior, W, F) of an entry of SMALL: one frame missing, ss_order 1 throughout, so that no window is NaN """
    S, T, gap, kind = SMALL[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    model = C.random_model(rng, S, T + 4, orders=np.ones((S, 2), dtype=int))
    x = C.random_traj(rng, T, (gap,))
    if kind == 'bounded3':
        prior = DC.make_prior('nongeometric', rng, S, T + 3)
        dwell, surv = prior.log_dwell.copy(), prior.log_surv.copy()
        dwell[:, 3:] = surv[:, 3:] = -np.inf
        prior = type(prior)(prior.log_init, prior.log_jump, dwell, surv)
    else:
        prior = DC.prior_of(kind, rng, S, T + 3, T)
    W, F = C.tables(model, x)
    for a in (x, W, F):
        a.setflags(write=False)
    return model, x, prior, W, F
