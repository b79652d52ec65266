"""
Cases shared by the tests of the expected segment-length counts and of the fit of the dwell-time prior
(tests/test_dwell_lengths.py, tests/test_gpu_dwell_lengths.py): the cases that the GPU test holds to the oracle
tests/dwell_length_oracle.py with the oracle's answers (computed once a session and shared; their arrays are read-only), the
generator of semi-Markov profiles from a piecewise-constant hazard, and the two data sets of the fits.
"""
import functools
import time

import numpy as np

import bild_amd
import dwell_cases as DC
import dwell_length_oracle as DL
import dwell_oracle as DO
import segment_cases as C
import segment_sensitivity_cases as SC

# (S, T, missing frames, prior kind, nan mode) of the cases that tests/test_gpu_dwell_lengths.py holds to the oracle.  T around
# the 64-length tiles of the length kernel; S = 2 throughout, S = 3 at 65 and 193, S = 1 and S = 4 at 65; T = 321 = 257 + 64
# has six blocks of 64 start frames and six tiles of lengths, past every boundary of either; isolated missing frames; the three prior
# kinds of `dwell_cases.make_prior`.  'order0_gap': `segment_sensitivity_cases.order0_gap_case` with the gap across the first
# tile's edge, in both NaN modes.
ORACLE_CASES = [(2, 1, (), 'markov', 'propagate'), (2, 2, (), 'minlength', 'propagate'), (2, 3, (), 'nongeometric', 'propagate'),
                (2, 63, (5,), 'markov', 'propagate'), (2, 64, (), 'minlength', 'propagate'),
                (2, 65, (10, 40), 'nongeometric', 'propagate'), (3, 65, (7,), 'minlength', 'propagate'),
                (1, 65, (20,), 'markov', 'propagate'), (4, 65, (3,), 'nongeometric', 'propagate'),
                (2, 130, (64,), 'minlength', 'propagate'), (2, 193, (3, 100), 'markov', 'propagate'),
                (3, 193, (64,), 'nongeometric', 'propagate'), (2, 321, (128,), 'markov', 'propagate'),
                (2, 130, 'order0_gap', 'markov', 'propagate'), (2, 130, 'order0_gap', 'markov', 'omit')]

ORACLE_SECONDS = {}     # what each oracle answer of this session took


@functools.lru_cache(maxsize=None)
def oracle_case(S, T, missing, kind):
    """ (model, x, prior, W, F) of an entry of ORACLE_CASES (the NaN mode does not change them) """
    rng = np.random.default_rng(2400 + 1000 * S + T)
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
    """ `dwell_length_oracle.solve` of an entry of ORACLE_CASES, and 'jumps': `dwell_oracle.solve`'s expected jumps """
    _, _, prior, W, F = oracle_case(*case[:4])
    start = time.perf_counter()
    out = DL.solve(W, F, prior, nan=case[4])
    out['jumps'] = DO.solve(W, F, prior, nan=case[4])['exp_jumps']
    ORACLE_SECONDS[case] = time.perf_counter() - start
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


# ---------------------------------------------------------------- data for the fits

def power_law_model(T):
    """ the two-state model of tests/test_gpu_dwell.py's `test_fit_markov_prior` """
    lags = np.arange(T + 8, dtype=float)
    return bild_amd.GenericGaussianModel([[(np.where(lags > 0, g * lags ** a + 0.1, 0), 0.0, 1)] * 2 for g, a in ((0.3, 0.6), (2.0, 0.9))])


MARKOV_P, MARKOV_START = np.array([[0.95, 0.05], [0.1, 0.9]]), np.array([[0.9, 0.1], [0.2, 0.8]])


def markov_data(n=64, T=200):
    """ (model, trajectories): the 64 x T = 200 data of tests/test_gpu_dwell.py's `test_fit_markov_prior`, drawn the same way """
    model = power_law_model(T)
    rng = np.random.default_rng(61)
    profiles = []
    for _ in range(n):
        st = np.empty(T, dtype=int)
        st[0] = rng.choice(2, p=[0.5, 0.5])
        for t in range(1, T):
            st[t] = rng.choice(2, p=MARKOV_P[st[t - 1]])
        profiles.append(st)
    return model, model.trajectories_from_loopingprofiles(profiles, seed=62)


HAZARD_EDGES = np.array([1, 4, 16])
HAZARD_TRUE = np.array([[0.0, 0.02, 0.15], [0.0, 0.1, 0.05]])     # per bin: no segment shorter than 4 frames


def hazard_profiles(rng, n, T, edges, hazard, init=(0.5, 0.5)):
    """
    n state sequences of T frames of a two-state semi-Markov chain: a segment in state s that has reached l frames ends there
    with probability hazard[s][bin of l], bin j covering [edges[j], edges[j + 1]), the last one open; the states alternate
    """
    out = []
    for _ in range(n):
        st, t, s = np.empty(T, dtype=int), 0, int(rng.choice(2, p=init))
        while t < T:
            length = 1
            while rng.random() >= hazard[s][np.searchsorted(edges, length, side='right') - 1]:
                length += 1
            st[t:t + length] = s
            t, s = t + length, 1 - s
        out.append(st)
    return out


def hazard_data(n=64, T=200):
    """ (model, trajectories, profiles): non-geometric data, drawn from HAZARD_TRUE on HAZARD_EDGES under `power_law_model` """
    model = power_law_model(T)
    profiles = hazard_profiles(np.random.default_rng(71), n, T, HAZARD_EDGES, HAZARD_TRUE)
    return model, model.trajectories_from_loopingprofiles(profiles, seed=72), profiles


def hazard_prior(edges, hazard, n, init=(0.5, 0.5)):
    """ the two-state `DwellPrior` of a piecewise-constant hazard, tables for n frames """
    bins = np.searchsorted(edges, np.arange(1, n + 1), side='right') - 1
    return bild_amd.DwellPrior.from_hazard(np.asarray(hazard)[:, bins], [[0.0, 1.0], [1.0, 0.0]], init)
