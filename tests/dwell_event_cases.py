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


def case_id(case):
    S, T, missing, kind, nan, _, k_max = case
    return f"S{S}_T{T}_{kind}_{nan}" + ('_order0_gap' if missing == 'order0_gap' else '') + ('' if k_max is None else f"_k{k_max}")


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
