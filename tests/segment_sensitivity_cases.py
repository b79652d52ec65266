"""
What the tests of the evidence gradient share (tests/test_segment_sensitivity.py, tests/test_gpu_segment_sensitivity.py): a
four-parameter family through any `GenericGaussianModel` of at least two states, and the oracle's answer for a model.

theta = (scale of state 0's MSD, scale of state 1's MSD, scale of every mean, a noise term added to every MSD at positive
lags and at infinity); the model itself sits at theta = (1, 1, 1, 0).  The family is linear in theta.
"""
import numpy as np

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
