"""
Cases shared by the tests of the dwell-time recursion (tests/test_dwell.py, tests/test_gpu_dwell.py) and of its draws: priors,
the cases that the GPU test holds to the oracle tests/dwell_oracle.py with the oracle's answers, and the identity that ties
the symmetric two-state chain to the segment recursion of section 18.  An oracle answer is computed once a session and shared
(`oracle_answer`, `ragged_answers`, `sharp_answer`); its arrays are read-only.  tests/test_dwell.py asserts the conditions on
these inputs without a GPU.
"""
import functools
import math
import time

import numpy as np
from scipy.special import logsumexp

import bild_amd
import dwell_oracle as DO
import segment_cases as C


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


def absorbing_prior(rng, L):
    """ three states, 0 -> 2 forbidden, state 2 absorbing: its jumps and dwells are -inf, gamma behind it is -inf before T """
    P = np.array([[0.85, 0.15, 0.0], [0.1, 0.8, 0.1], [0.0, 0.0, 1.0]])
    return bild_amd.DwellPrior.markov(P, rng.dirichlet(np.ones(3)), n=L)


BOUND = 70      # the longest segment of the 'bounded' prior: longer than a 64-frame tile, shorter than two


def prior_of(kind, rng, S, L, T):
    """
    `make_prior`'s kinds, and the hard priors: 'bounded' -- non-geometric tables that end at BOUND frames, so that a switch is
    forced across every tile seam; 'one_start' -- Markov, every profile starts in state S - 1; 'absorbing' -- `absorbing_prior`;
    'flip' -- every segment has one frame; 'impossible' -- no profile of a trajectory of T frames has positive weight: state 0
    alone starts, nothing jumps, and the one segment of T frames does not survive
    """
    if kind in ('markov', 'minlength', 'nongeometric'):
        return make_prior(kind, rng, S, L)
    if kind == 'bounded':
        prior = make_prior('nongeometric', rng, S, L)
        dwell, surv = prior.log_dwell.copy(), prior.log_surv.copy()
        dwell[:, BOUND:] = surv[:, BOUND:] = -np.inf
        return bild_amd.DwellPrior(prior.log_init, prior.log_jump, dwell, surv)
    if kind == 'one_start':
        prior = make_prior('markov', rng, S, L)
        init = np.full(S, -np.inf)
        init[S - 1] = 0.0
        return bild_amd.DwellPrior(init, prior.log_jump, prior.log_dwell, prior.log_surv)
    if kind == 'absorbing':
        assert S == 3
        return absorbing_prior(rng, L)
    if kind == 'flip':
        assert S == 2
        return bild_amd.DwellPrior.markov([[0, 1], [1, 0]], [0.3, 0.7], n=L)
    assert kind == 'impossible' and S == 2
    prior = make_prior('markov', rng, S, L)
    surv = prior.log_surv.copy()
    surv[0, T - 1] = -np.inf
    return bild_amd.DwellPrior([0.0, -np.inf], np.full((2, 2), -np.inf), prior.log_dwell, surv)


# (S, T, missing frames, prior kind) of the cases that tests/test_gpu_dwell.py holds to the oracle.  The first ten stood before
# the others: S = 2 and 3, geometric tables, at most four tiles.  The others: S = 1 (no switch ever) and S = 4 (the largest
# instantiation) around the tiles; non-geometric tables; T > 256, where the statistics kernels need a second workgroup;
# and the hard priors of `prior_of`.
ORACLE_CASES = [(2, 1, (), 'markov'), (2, 2, (), 'minlength'), (2, 3, (), 'markov'), (2, 63, (5,), 'markov'),
                (2, 64, (), 'minlength'), (2, 65, (10, 40), 'markov'), (3, 65, (7,), 'minlength'), (2, 130, (64,), 'minlength'),
                (2, 193, (3, 100), 'markov'), (3, 193, (), 'markov'),
                (1, 1, (), 'markov'), (1, 65, (3,), 'markov'), (1, 130, (), 'nongeometric'),
                (4, 3, (), 'markov'), (4, 64, (), 'minlength'), (4, 65, (7,), 'nongeometric'),
                (4, 129, (64, 100), 'markov'), (4, 257, (100,), 'nongeometric'),
                (2, 65, (), 'nongeometric'), (3, 193, (3,), 'nongeometric'),
                (2, 256, (), 'markov'), (2, 257, (255,), 'minlength'), (3, 321, (128,), 'markov'),
                (2, 130, (), 'bounded'), (3, 193, (), 'bounded'), (2, 65, (), 'one_start'),
                (3, 130, (20,), 'absorbing'), (2, 70, (), 'flip'), (2, 70, (), 'impossible')]
N_ORACLE_CASES_BEFORE = 10

ORACLE_SECONDS = {}     # what each oracle answer of this session took: tests/README.md allows a designed case 20 s


def _solve(key, W, F, prior):
    start = time.perf_counter()
    out = DO.solve(W, F, prior)
    ORACLE_SECONDS[key] = time.perf_counter() - start
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle_case(case):
    """ (model, x, prior, W, F) of an entry of ORACLE_CASES """
    S, T, missing, kind = case
    rng = np.random.default_rng(1000 * S + T)
    model = C.random_model(rng, S, T + 8)
    x = C.random_traj(rng, T, missing)
    prior = prior_of(kind, rng, S, T + 5, T)
    W, F = C.tables(model, x)
    for a in (x, W, F):
        a.setflags(write=False)
    return model, x, prior, W, F


@functools.lru_cache(maxsize=None)
def oracle_answer(case):
    """ `dwell_oracle.solve` of an entry of ORACLE_CASES """
    _, _, prior, W, F = oracle_case(case)
    return _solve(case, W, F, prior)


RAGGED = ((1, ()), (257, (100,)), (64, ()), (130, (63,)), (2, ()), (65, (9,)))


@functools.lru_cache(maxsize=None)
def ragged_case():
    """ (model, prior, trajectories, their (W, F)): six trajectories of four states for one call, most shorter than the longest """
    rng = np.random.default_rng(4001)
    model = C.random_model(rng, 4, 270)
    prior = make_prior('nongeometric', rng, 4, 262)
    xs = [C.random_traj(rng, T, missing) for T, missing in RAGGED]
    tabs = [C.tables(model, x) for x in xs]
    for a in xs + [t for pair in tabs for t in pair]:
        a.setflags(write=False)
    return model, prior, xs, tabs


@functools.lru_cache(maxsize=None)
def ragged_answers():
    _, prior, _, tabs = ragged_case()
    return [_solve(('ragged', j), W, F, prior) for j, (W, F) in enumerate(tabs)]


@functools.lru_cache(maxsize=None)
def sharp_case():
    """
    (model, x, prior, true states, W, F): the steps of state 1 are 50 times those of state 0, so W reaches -1.1e5 and the
    oracle's marginals underflow to 0 on an eighth of the entries
    """
    T = 130
    rng = np.random.default_rng(99)
    lags = np.arange(T + 8.)
    model = bild_amd.GenericGaussianModel([[(np.where(lags > 0, g * lags + 2e-4, 0), 0.0, 1)] * 2 for g in (0.01, 25.0)])
    st = np.zeros(T, dtype=int)
    st[30:70] = 1
    st[100:110] = 1
    x = np.cumsum(rng.normal(size=(T, 2)) * np.where(st == 1, 5.0, 0.1)[:, None], axis=0)
    prior = make_prior('markov', rng, 2, T + 5)
    W, F = C.tables(model, x)
    for a in (st, x, W, F):
        a.setflags(write=False)
    return model, x, prior, st, W, F


@functools.lru_cache(maxsize=None)
def sharp_answer():
    _, _, prior, _, W, F = sharp_case()
    return _solve('sharp', W, F, prior)


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
