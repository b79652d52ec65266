"""
What the tests of the evidence gradient share (tests/test_segment_sensitivity.py, tests/test_gpu_segment_sensitivity.py): a
four-parameter family through any `GenericGaussianModel` of at least two states, the oracle's answer for a model, and the
designed cases beyond one 64-frame tile of the weight kernel with their cached oracle answers.

theta = (scale of state 0's MSD, scale of state 1's MSD, scale of every mean, a noise term added to every MSD at positive
lags and at infinity); the model itself sits at theta = (1, 1, 1, 0).  The family is linear in theta.
"""
import functools
import time

import numpy as np
from scipy.special import logsumexp

import bild_amd
from bild_amd.gauss import covariance

import gauss_sensitivity_oracle as GS
import segment_cases as C
import segment_oracle as SO
import segment_sensitivity_oracle as SS

BASE = np.array([1.0, 1.0, 1.0, 0.0])


def family_arrays(model, theta):
    """ msd, msd_inf, mean of the family's member theta (4,) """
    msd, msd_inf, mean = model.msd.copy(), model.msd_inf.copy(), model.mean * theta[2]
    for s in (0, 1):
        msd[s] *= theta[s]
        msd_inf[s] *= theta[s]
    msd[:, :, 1:] += theta[3]
    msd_inf = msd_inf + theta[3] * (model.ss_order == 0)
    return msd, msd_inf, mean


def derivatives(model, P=4):
    """ dmsd (P, S, d, n_lags), dmsd_inf, dmean (P, S, d) of the first P parameters at the model itself """
    S, d, n_lags = model.msd.shape
    dmsd, dinf, dmean = np.zeros((4, S, d, n_lags)), np.zeros((4, S, d)), np.zeros((4, S, d))
    for s in (0, 1):
        dmsd[s, s] = model.msd[s]
        dinf[s, s] = model.msd_inf[s]
    dmean[2] = model.mean
    dmsd[3, :, :, 1:] = 1.0
    dinf[3] = model.ss_order == 0
    return dmsd[:P], dinf[:P], dmean[:P]


def oracle(model, x, k_max, P=4, log_k_prior=None, nan='propagate'):
    return SS.solve(model.msd, model.msd_inf, model.mean, model.ss_order, np.asarray(x, dtype=np.float64), model.transitions, k_max,
                    *derivatives(model, P), log_k_prior=log_k_prior, nan=nan)


# ---------------------------------------------------------------- designed cases beyond one 64-frame tile

def order0_gap_case(rng, T, gap=(20, 26)):
    """ two states, dimension 0 of ss_order 0 and missing on the frames gap[0] ... gap[1] - 1: a later segment inside has no value """
    model = bild_amd.GenericGaussianModel([[(np.append(np.arange(T + 8) * 0.5 + 0.1, 50.0), 0.3 * s, 0),
                                            (np.arange(T + 8) * (0.5 + s), 0.0, 1)] for s in range(2)])
    x = C.random_traj(rng, T)
    x[gap[0]:gap[1], 0] = np.nan
    return model, x


# the models of the designed cases: name -> (seed, S, n_lags, orders (None: random), d).  Cases of one name share one model
# object, so that they can form a batch.
MODELS = {
    'edge': (640, 2, 136, [[0, 1], [1, 0]], 2),
    'straddle': (1280, 3, 136, [[1, 1]] * 3, 2),
    'd3': (131, 2, 136, None, 3),
    'd1_S4': (100, 4, 104, None, 1),
    'stride_o0': (2600, 2, 264, [[0], [0]], 1),
    'stride_o1': (2601, 2, 264, [[1], [1]], 1),
}

STRADDLE_MISSING = (0, 1, 62, 63, 64, 65, 127)
ORDER0_GAP_PRIOR = (1, 1, 0, 0, 0, 0, 0)

# name: (model, T, missing frames, k_max, runs), a run = (nan mode, prior weights or None).  `order0_gap_T130` builds its own
# model; under 'propagate' with the uniform prior its evidence is NaN from k = 2 on, and it is the only case with a NaN.
DESIGNED = {
    'edge_T64': ('edge', 64, (), 6, (('propagate', None),)),
    'edge_T65': ('edge', 65, (), 6, (('propagate', None),)),
    'edge_T127': ('edge', 127, (), 4, (('propagate', None),)),
    'edge_T128': ('edge', 128, (), 4, (('propagate', None),)),
    'edge_T129': ('edge', 129, (), 4, (('propagate', None),)),
    'straddle_T128': ('straddle', 128, STRADDLE_MISSING, 6, (('propagate', None), ('omit', None))),
    'straddle_T129': ('straddle', 129, STRADDLE_MISSING, 6, (('propagate', None), ('omit', None))),
    'order0_gap_T130': (None, 130, (), 6, (('propagate', None), ('propagate', ORDER0_GAP_PRIOR), ('omit', None))),
    'd3_T131': ('d3', 131, (5, 70), 4, (('omit', None),)),
    'd1_S4_T100': ('d1_S4', 100, (), 4, (('propagate', None),)),
    'stride_T260_o0': ('stride_o0', 260, (), 3, (('propagate', None),)),
    'stride_T260_o1': ('stride_o1', 260, (), 3, (('propagate', None),)),
    'stride_gap_T260_o0': ('stride_o0', 260, (258,), 3, (('omit', None),)),
    'stride_gap_T260_o1': ('stride_o1', 260, (258,), 3, (('omit', None),)),
}
NAN_RUNS = {('order0_gap_T130', 'propagate', None)}     # the runs whose oracle answer is NaN, named


@functools.lru_cache(maxsize=None)
def designed_model(name):
    seed, S, n_lags, orders, d = MODELS[name]
    return C.random_model(np.random.default_rng(seed), S, n_lags, orders=orders, d=d)


@functools.lru_cache(maxsize=None)
def _designed(name):
    mname, T, missing, k_max, _ = DESIGNED[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    if mname is None:
        model, x = order0_gap_case(rng, T, gap=(61, 67))
    else:
        model = designed_model(mname)
        x = C.random_traj(rng, T, missing, d=model.d)
    x.setflags(write=False)
    return model, x, k_max


def designed(name):
    """ (model, trajectory (read-only), k_max) of a designed case """
    return _designed(name)


def designed_runs(names=None):
    """ (name, nan mode, prior) of every run of the designed cases """
    return [(name, nan, prior) for name in (names or DESIGNED) for nan, prior in DESIGNED[name][4]]


def log_prior(k_prior, K):
    """ the log weights (K,) of `exact_sensitivities`' k_prior: None, an integer (that k alone) or K weights """
    if k_prior is None:
        return None
    with np.errstate(divide='ignore'):
        return np.log(np.arange(K) == k_prior if isinstance(k_prior, (int, np.integer)) else np.asarray(k_prior, dtype=float))


ORACLE_SECONDS = {}     # (name, nan, prior) -> the wall time of the oracle's answer


@functools.lru_cache(maxsize=None)
def designed_oracle(name, nan, k_prior=None):
    """
    The oracle's answer at P = 4 for a designed case, computed once per (case, nan mode, prior) and shared by whoever asks: treat
    it as read-only.  k_prior: None, an integer or a tuple of weights.
    """
    model, x, k_max = designed(name)
    t0 = time.perf_counter()
    out = oracle(model, x, k_max, P=4, log_k_prior=log_prior(k_prior, k_max + 1), nan=nan)
    ORACLE_SECONDS[name, nan, k_prior] = time.perf_counter() - t0
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def designed_logev(name, nan):
    """ the oracle's logev of a designed case alone: what `segment_sensitivity_oracle.solve` returns as 'logev', without the tangents """
    model, x, k_max = designed(name)
    W, F = C.tables(model, x)
    return SO.solve(W, F, model.transitions, k_max, nan=nan, with_marginals=False)['logev']


def flat_long_case(T):
    """
    Two ss_order-0 states in one dimension whose MSDs are 2 % and whose means 0.3 apart, and a gap-free trajectory drawn between
    them, so that both flat profiles keep weight: the k = 0 case at lengths the segment oracle cannot reach
    """
    lags = np.arange(T + 1, dtype=float)
    msd = 0.8 * lags ** 0.6 + np.where(lags > 0, 0.2, 0.0)
    msd_inf = 2 * msd[-1] + 4
    model = bild_amd.GenericGaussianModel([[(np.append(c * msd, c * msd_inf), m, 0)] for c, m in ((1.0, 0.2), (1.02, 0.5))])
    rng = np.random.default_rng(T)
    cov = covariance(1.01 * msd, 1.01 * msd_inf, np.arange(T), 0)
    x = 0.35 + np.linalg.cholesky(cov) @ rng.normal(size=T)
    return model, x[:, None]


def flat_profile_reference(model, x, P=4):
    """
    All prior weight on k = 0: the posterior is over the S flat profiles, so log_marginal = logsumexp_s logL_s - log S, and grad,
    fisher and expected_logL are the softmax-weighted sums of `gauss_sensitivity_oracle.sensitivities` of the flat profiles.
    """
    S, T = model.nStates, len(x)
    dmsd, dinf, dmean = derivatives(model, P)
    terms = [GS.sensitivities(model.msd, model.msd_inf, model.mean, model.ss_order, x, np.full(T, s), dmsd=dmsd, dmsd_inf=dinf,
                              dmean=dmean) for s in range(S)]
    logL = np.array([t[0] for t in terms])
    lm = logsumexp(logL)
    p = np.exp(logL - lm)
    return {'weights': p, 'log_marginal': lm - np.log(S), 'exp_logl': p @ logL, 'grad': p @ np.array([t[1] for t in terms]),
            'fisher': np.tensordot(p, np.array([t[2] for t in terms]), axes=1)}
