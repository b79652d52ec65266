"""
Cases shared by the tests of the evidence gradient under a dwell-time prior (tests/test_dwell_sensitivity.py,
tests/test_gpu_dwell_sensitivity.py): the four-parameter family of tests/segment_sensitivity_cases.py for any number of states,
the cases that the GPU test holds to the oracle tests/dwell_sensitivity_oracle.py with the oracle's answers (computed once a
session at P = 4 and shared; their arrays are read-only), the prior that admits one profile, and the data set of the fit.
"""
import functools
import math
import time

import numpy as np

import bild_amd
import dwell_cases as DC
import dwell_sensitivity_oracle as DS
import segment_cases as C
import segment_sensitivity_cases as SC


def derivatives(model, P=4):
    """ `segment_sensitivity_cases.derivatives` for any number of states: with one state, parameter 1 scales nothing """
    S, d, n_lags = model.msd.shape
    dmsd, dinf, dmean = np.zeros((4, S, d, n_lags)), np.zeros((4, S, d)), np.zeros((4, S, d))
    for s in range(min(S, 2)):
        dmsd[s, s] = model.msd[s]
        dinf[s, s] = model.msd_inf[s]
    dmean[2] = model.mean
    dmsd[3, :, :, 1:] = 1.0
    dinf[3] = model.ss_order == 0
    return dmsd[:P], dinf[:P], dmean[:P]


def oracle(model, x, prior, P=4, nan='propagate'):
    return DS.solve(model.msd, model.msd_inf, model.mean, model.ss_order, np.asarray(x, dtype=np.float64), prior,
                    *derivatives(model, P), nan=nan)


# (S, T, missing frames, prior kind, nan mode) of the cases that tests/test_gpu_dwell_sensitivity.py holds to the oracle: T around
# the 64-frame tiles of the weight kernel; S = 2 throughout, S = 3 at 65 and 193, S = 1 at 64, S = 4 at 130; isolated missing
# frames; the three prior kinds of `dwell_cases.make_prior`.  'order0_gap': `segment_sensitivity_cases.order0_gap_case` with the
# gap across the first tile's edge, in both NaN modes.
ORACLE_CASES = [(2, 1, (), 'markov', 'propagate'), (2, 2, (), 'minlength', 'propagate'), (2, 3, (), 'nongeometric', 'propagate'),
                (2, 63, (5,), 'markov', 'propagate'), (2, 64, (), 'minlength', 'propagate'), (1, 64, (20,), 'markov', 'propagate'),
                (2, 65, (10, 40), 'nongeometric', 'propagate'), (3, 65, (7,), 'minlength', 'propagate'),
                (2, 130, (64,), 'minlength', 'propagate'), (4, 130, (3, 100), 'nongeometric', 'propagate'),
                (2, 193, (3, 100), 'markov', 'propagate'), (3, 193, (64,), 'nongeometric', 'propagate'),
                (2, 130, 'order0_gap', 'markov', 'propagate'), (2, 130, 'order0_gap', 'markov', 'omit')]

ORACLE_SECONDS = {}     # what each oracle answer of this session took


@functools.lru_cache(maxsize=None)
def oracle_case(S, T, missing, kind):
    """ (model, x, prior) of an entry of ORACLE_CASES (the NaN mode does not change them) """
    rng = np.random.default_rng(2300 + 1000 * S + T)
    if missing == 'order0_gap':
        model, x = SC.order0_gap_case(rng, T, gap=(61, 67))
    else:
        model = C.random_model(rng, S, T + 8)
        x = C.random_traj(rng, T, missing)
    prior = DC.make_prior(kind, rng, S, T + 5)
    x.setflags(write=False)
    return model, x, prior


@functools.lru_cache(maxsize=None)
def oracle_answer(case):
    """ `dwell_sensitivity_oracle.solve` at P = 4 of an entry of ORACLE_CASES """
    model, x, prior = oracle_case(*case[:4])
    start = time.perf_counter()
    out = oracle(model, x, prior, P=4, nan=case[4])
    ORACLE_SECONDS[case] = time.perf_counter() - start
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def one_profile_prior(T, lengths, L):
    """
    two states; the dwell tables are -inf except `lengths[s]` in state s, log_init is on state 0, and log_surv is -inf except at the
    censored last segment: the one profile of positive weight alternates 0, 1, 0, ... in segments of those lengths.
    -> (prior, its states (T,))
    """
    dwell, surv = np.full((2, L), -np.inf), np.full((2, L), -np.inf)
    for s in (0, 1):
        dwell[s, lengths[s] - 1] = 0.0
    jump = np.array([[-np.inf, 0.0], [0.0, -np.inf]])
    states, s, t = np.zeros(T, dtype=int), 0, 0
    while t + lengths[s] < T:
        states[t:t + lengths[s]] = s
        t, s = t + lengths[s], 1 - s
    states[t:] = s
    surv[s, T - t - 1] = 0.0
    return bild_amd.DwellPrior([0.0, -np.inf], jump, dwell, surv), states


def flat_prior(L):
    """ two states, log_init on state 0 and every jump at -inf: the flat profile of state 0 alone has weight """
    return bild_amd.DwellPrior([0.0, -np.inf], np.full((2, 2), -np.inf), np.zeros((2, L)), np.zeros((2, L)))


def k_weights_of_symmetric_chain(p, T):
    """ proportional to the symmetric two-state chain's prior summed over the 2 C(T - 1, k) profiles of k switches, k = 0 ... T - 1 """
    return np.array([p ** k * (1 - p) ** (T - 1 - k) * 2 * math.comb(T - 1, k) for k in range(T)])


# ---------------------------------------------------------------- a family with a known truth and a data set for the fit

BASE, TAU, NOISE = (0.5, 4.0), (3.0, 6.0), 0.02
FIT_P = np.array([[0.95, 0.05], [0.1, 0.9]])


def exp_family(L, d=2, with_noise=True):
    """ tests/test_gpu_segment_sensitivity.py's family: two ss_order-0 states with saturating MSDs a factor 8 apart, truth (1, 1[, NOISE]) """
    lags = np.arange(L, dtype=np.float64)

    def family(t0, t1, n=NOISE):
        return [[(np.append(t * b * (1 - np.exp(-lags / tau)) + n * (lags > 0), t * b + n), 0.0, 0)] * d
                for t, b, tau in zip((t0, t1), BASE, TAU)]

    def derivs(t0, t1, n=NOISE):
        P = 3 if with_noise else 2
        dmsd, dinf = np.zeros((P, 2, d, L)), np.zeros((P, 2, d))
        for s in range(2):
            dmsd[s, s] = BASE[s] * (1 - np.exp(-lags / TAU[s]))
            dinf[s, s] = BASE[s]
        if with_noise:
            dmsd[2, :, :, 1:] = 1.0
            dinf[2] = 1.0
        return dmsd, dinf, None

    return family, derivs


def markov_profiles(rng, n, T, P, init=(0.5, 0.5)):
    """ n state sequences of T frames from the Markov chain (P, init) """
    out = []
    for _ in range(n):
        st = np.empty(T, dtype=int)
        st[0] = rng.choice(len(init), p=init)
        for t in range(1, T):
            st[t] = rng.choice(len(init), p=P[st[t - 1]])
        out.append(st)
    return out
