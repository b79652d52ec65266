"""
Cases shared by the tests of the dwell-time recursion (tests/test_dwell.py, tests/test_gpu_dwell.py): priors, and the
identity that ties the symmetric two-state chain to the segment recursion of section 18.
"""
import math

import numpy as np
from scipy.special import logsumexp

import bild_amd


def markov_matrix(rng, S):
    """ a random row-stochastic P with a stay probability of 0.6 ... 0.9; S = 3 forbids 0 -> 2 as `segment_cases.random_model` """
    P = rng.uniform(0.2, 1.0, size=(S, S))
    np.fill_diagonal(P, 0.0)
    if S == 3:
        P[0, 2] = 0.0
    if S > 1:
        P *= (rng.uniform(0.1, 0.4, size=S) / P.sum(axis=1))[:, None]
    P[np.arange(S), np.arange(S)] = 1.0 - P.sum(axis=1)
    return P


def make_prior(kind, rng, S, L):
    """ 'markov'; 'nongeometric': unnormalised random tables; 'minlength': Markov whose completed segments have >= 2 frames """
    P = markov_matrix(rng, S)
    init = rng.dirichlet(np.ones(S))
    prior = bild_amd.DwellPrior.markov(P, init, n=L)
    if kind == 'markov':
        return prior
    if kind == 'minlength':
        dwell = prior.log_dwell.copy()
        dwell[:, 0] = -np.inf
        return bild_amd.DwellPrior(prior.log_init, prior.log_jump, dwell, prior.log_surv)
    assert kind == 'nongeometric'
    lengths = np.arange(1, L + 1)
    dwell = np.stack([np.log(lengths) * rng.uniform(0.5, 2) - lengths * rng.uniform(0.1, 0.6) + rng.normal(scale=0.3, size=L)
                      for _ in range(S)])
    surv = np.stack([-lengths * rng.uniform(0.05, 0.4) + rng.normal(scale=0.3, size=L) for _ in range(S)])
    return bild_amd.DwellPrior(prior.log_init, prior.log_jump, dwell, surv)


def symmetric_chain(p, L):
    """ two states, switching probability p either way, uniform start: the prior of a profile depends on its k alone """
    return bild_amd.DwellPrior.markov([[1 - p, p], [p, 1 - p]], [0.5, 0.5], n=L)


def symmetric_mixture(p, T, logev_k, log_post_k):
    """
    log evidence and (2, T) marginals (linear scale) of the symmetric chain from section 18's evidences per k (the log MEAN
    likelihood over the n_k = 2 C(T - 1, k) profiles of k switches) and marginals per k, k = 0 ... len(logev_k) - 1
    """
    terms = np.array([math.log(0.5) + k * math.log(p) + (T - 1 - k) * math.log1p(-p) + math.log(2 * math.comb(T - 1, k)) + ev
                      for k, ev in enumerate(logev_k)])
    total = float(logsumexp(terms))
    w = np.exp(terms - total)
    return total, np.tensordot(w, np.exp(np.asarray(log_post_k)), axes=1)
