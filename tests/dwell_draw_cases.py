"""
Cases and seeds shared by the tests of the draws under a dwell-time prior (tests/test_dwell_draw.py,
tests/test_gpu_dwell_draw.py).  The replay cases are what the GPU test runs against the oracle draw for draw;
tests/test_dwell_draw.py asserts that the oracle alone flags none of their draws as fragile, so the seeds below are part of
the cases.  The oracle's answer of a case is computed once a session and shared (`oracle_replay`); nobody writes to it.
"""
import functools

import numpy as np

import bild_amd
import dwell_cases as DC
import dwell_draw_oracle as DDO
import segment_cases as C

N_REPLAY = 4096

# name: (S, T, missing frames, prior kind of `dwell_cases.prior_of`, seed of the uniforms[, draws: the first rows of the
# (N_REPLAY, 2T - 1) uniforms of that seed, where the oracle would take a minute for all of them])
REPLAY_CASES = {
    's2_T1_markov': (2, 1, (), 'markov', 1),
    's2_T2_minlength': (2, 2, (), 'minlength', 2),
    's2_T3_markov': (2, 3, (), 'markov', 3),
    's2_T63_markov': (2, 63, (5,), 'markov', 4),
    's2_T64_minlength': (2, 64, (), 'minlength', 5),
    's2_T65_markov': (2, 65, (10, 40), 'markov', 6),
    's3_T65_minlength': (3, 65, (7,), 'minlength', 7),
    's2_T130_minlength': (2, 130, (64,), 'minlength', 8),
    's2_T193_markov': (2, 193, (3, 100), 'markov', 9),
    's3_T193_markov': (3, 193, (), 'markov', 10),
    's3_T65_absorbing': (3, 65, (20,), 'absorbing', 11),
    's2_T70_order0_gap': (2, 70, (), 'markov', 12),
    # S = 1 and S = 4, non-geometric and length-bounded tables, and more than 256 frames
    's1_T65_markov': (1, 65, (), 'markov', 21),
    's4_T65_nongeometric': (4, 65, (7,), 'nongeometric', 22),
    's4_T130_minlength': (4, 130, (64,), 'minlength', 23),
    's2_T257_markov': (2, 257, (255,), 'markov', 24, 1024),
    's3_T321_nongeometric': (3, 321, (128,), 'nongeometric', 25, 1024),
    's2_T130_bounded': (2, 130, (), 'bounded', 26),
}


def n_replay(name):
    """ the draws of a case """
    case = REPLAY_CASES[name]
    return case[5] if len(case) > 5 else N_REPLAY


def order0_gap_case(rng, T):
    """ a later ss_order-0 segment inside frames 60 .. 67 has no valid value: NaN windows across the first tile's edge """
    model = bild_amd.GenericGaussianModel([[(np.append(np.arange(T + 8) * 0.5 + 0.1, 50.0), 0.3 * s, 0),
                                            (np.arange(T + 8) * (0.5 + s), 0.0, 1)] for s in range(2)])
    x = C.random_traj(rng, T)
    x[60:68, 0] = np.nan
    return model, x


def replay_case(name):
    """ (model, x, prior, uniforms (n_replay(name), 2T - 1)) """
    S, T, missing, kind, seed = REPLAY_CASES[name][:5]
    rng = np.random.default_rng(1000 * S + T)
    if 'order0' in name:
        model, x = order0_gap_case(rng, T)
    else:
        model = C.random_model(rng, S, T + 8)
        x = C.random_traj(rng, T, missing)
    prior = DC.prior_of(kind, rng, S, T + 5, T)
    return model, x, prior, np.random.default_rng(seed).random((N_REPLAY, 2 * T - 1))[:n_replay(name)]


N_SIX = 200     # draws per trajectory of the six-trajectory call


def six_uniforms():
    """ the replayed uniforms (6, N_SIX, 2 * 257 - 1) of the call that draws on `dwell_cases.ragged_case`'s six trajectories """
    return np.random.default_rng(27).random((len(DC.RAGGED), N_SIX, 2 * 257 - 1))


@functools.lru_cache(maxsize=None)
def oracle_six(j):
    """ `dwell_draw_oracle.draws` of trajectory j of the six, arrays read-only """
    _, prior, _, tabs = DC.ragged_case()
    out = DDO.draws(*tabs[j], prior, six_uniforms()[j])
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle_replay(name):
    """ `dwell_draw_oracle.draws` of the case, arrays read-only """
    model, x, prior, u = replay_case(name)
    W, F = C.tables(model, x)
    out = DDO.draws(W, F, prior, u)
    for a in out.values():
        a.setflags(write=False)
    return out
