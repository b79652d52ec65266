"""
Cases of tests/test_gpu_device_streams.py (each device-side consumer of csrc/philox.h against tests/philox_oracle.py), and
the conditions on them that tests/test_philox_oracle.py asserts without a GPU.  tests/README_device_streams.md describes
them and holds what the MI355X gave.
"""
import functools

import numpy as np

import bild_amd
import dwell_cases as DC
import gauss_sim_cases as GS
import philox_oracle as PO
import segment_cases as C

SEEDS = (1, 2 ** 32, 0x9E3779B97F4A7C15, 2 ** 64 - 1)
MIXED = SEEDS[2]        # a high word that is neither 0 nor the low word


def swap_halves(seed):
    return ((seed & 0xFFFFFFFF) << 32) | (seed >> 32)


# ---------------------------------------------------------------- the Rouse generator

# (N, d, seed): every split of the dimensions over workgroups (dpb = d at N <= 128 for d = 8, 7 at 130, 4 at 256), one and
# several workgroups per trajectory.  The exchange of the seed's halves must change the stream, so 2^64 - 1 keys the
# sub-batch call instead.
ROUSE_CASES = ((1, 1, SEEDS[0]), (5, 3, SEEDS[1]), (20, 8, MIXED), (64, 3, SEEDS[0]), (130, 2, MIXED), (256, 8, SEEDS[1]))
ROUSE_LENGTHS = (3, 257, 1, 65, 2, 64, 3, 65, 2, 1)
ROUSE_SUB = 3           # the second call takes the trajectories from this one on, with seed 2^64 - 1
ROUSE_S = 3
CONDITION = 1e-3        # every modal weight and noise scale against its largest


def rouse_model(N, d):
    """ the three-state chain of tests/test_gpu_simulate.py's make_model """
    loops = [None, (0, -1), (1, max(N // 2, 1))]
    return bild_amd.MultiStateRouse(N, 1.0, 0.7, d=d, looppositions=loops, measurement=np.linspace(0.2, 1.0, N), localization_error=0.1)


def rouse_condition(arrays, w):
    """ the smallest of |V_s^T w|_j, sqrt_sig_j and sqrt_cinf_j, each against its largest value """
    V, _, ssig, scinf = arrays[:4]
    u = np.abs(np.einsum('snj,n->sj', V, w))
    return min(float(np.min(a) / np.max(a)) for a in (u, ssig, scinf))


@functools.lru_cache(maxsize=None)
def rouse_inputs(N, d):
    """
    (modal arrays, w) for `_lib.rouse_simulate`: the model's own V, b, sqrt_sig, V^T G and V^T M0.  Two of its inputs would let
    a wrong normal pass unseen, so they are replaced: the centre-of-mass weights linspace(0.2, 1, N) have no component
    along the even modes of the free chain (1e-17 of the largest) and 1e-5 of it along the fast ones, so w is the first
    standard-normal vector of seeds 0, 1, ... that meets CONDITION in all three bases; and the steady-state scale of the
    centre-of-mass mode, which the model sets to 0, is set to the largest of the others.
    """
    arrays = [a.copy() for a in rouse_model(N, d)._modal_arrays()]
    scinf = arrays[3]
    for s in range(len(scinf)):
        scinf[s][scinf[s] == 0] = np.max(scinf[s]) if np.max(scinf[s]) > 0 else 1.0
    for seed in range(2000):
        w = np.random.default_rng(seed).standard_normal(N)
        if rouse_condition(arrays, w) > CONDITION:
            break
    for a in arrays + [w]:
        a.setflags(write=False)
    return arrays, w


def rouse_profiles(N, d):
    """ states of S = 3 per trajectory: switches at odd frames (between a cosine and its sine), at even ones, at frame 1 and T - 1 """
    rng = np.random.default_rng(100 * N + d)
    out = []
    for i, T in enumerate(ROUSE_LENGTHS):
        st = np.full(T, (i + N) % ROUSE_S)
        cuts = {1: [], 2: [1], 3: [1, 2], 64: [33, 63], 65: [1, 2, 33, 64]}.get(T)
        if cuts is None:
            cuts = sorted({1, 2, 65, 129, 256} | set(rng.choice(np.arange(3, T), size=12, replace=False).tolist()))
        for t in cuts:
            st[t:] = (st[t - 1] + 1 + rng.integers(ROUSE_S - 1)) % ROUSE_S
        out.append(st)
    return out


def rouse_call(N, d, first=0):
    """ the arguments of `_lib.rouse_simulate` behind the model's: T, seg_start, seg_state, missing, loc_err; and w's data scale """
    from bild_amd import models as M
    arrays, w = rouse_inputs(N, d)
    states = rouse_profiles(N, d)[first:]
    T = np.array([len(s) for s in states], dtype=np.int64)
    seg_start, seg_state = M._ragged_segments(states, T)
    rng = np.random.default_rng(7 * N + d + first)
    missing = rng.random(int(T.sum())) < 0.1
    missing[0] = True
    u = np.einsum('snj,n->sj', arrays[0], w)
    scale = float(np.sqrt(np.sum((u[0] * arrays[3][0]) ** 2)))      # the steady-state deviation of the data in state 0
    loc_err = 0.05 * scale * (1.0 + 0.1 * np.arange(d))[None, :] * (1.0 + 0.01 * np.arange(len(T)))[:, None]
    return T, seg_start, seg_state, missing, loc_err


def rouse_oracle(N, d, seed, first=0, shift=0, **mutation):
    """ the normals of every trajectory of the call from trajectory `first` on, index in the call + shift, in the replay layout """
    lengths = ROUSE_LENGTHS[first:]
    return np.concatenate([PO.rouse_normals(seed, i + shift, T, N, d, **mutation) for i, T in enumerate(lengths)])


# ---------------------------------------------------------------- the GenericGaussianModel generator

GAUSS_CASES = ((11, SEEDS[0]), (12, SEEDS[1]), (13, MIXED))    # (seed of gauss_sim_cases.make_model(3, 3, .), seed of the stream)
GAUSS_PROFILES = (                                              # (T, [(switch frame, state), ...]) behind the first state
    (700, 0, [(33, 1), (400, 2)]),      # an interval from an odd frame, one from an even frame; eleven 64-lane strides
    (65, 1, [(1, 2), (64, 0)]),
    (64, 2, [(32, 0), (63, 1)]),
    (3, 0, [(1, 1)]),
    (3, 2, [(2, 0)]),
    (2, 1, [(1, 0)]),
    (2, 2, []),
    (1, 0, []), (1, 1, []), (1, 2, []),
    (65, 0, [(7, 2), (8, 1), (40, 0)]),
)
GAUSS_SCRATCH = 700 * 3 * 8 + 64        # the longest trajectory's normals: a chunk of its own


def gauss_model(model_seed):
    return GS.make_model(3, 3, model_seed)


def gauss_states():
    out = []
    for T, s0, cuts in GAUSS_PROFILES:
        st = np.full(T, s0)
        for t, s in cuts:
            st[t:] = s
        out.append(st)
    return out


def gauss_call():
    """ T, seg_start, seg_state, missing of `_lib.gauss_simulate` """
    from bild_amd import models as M
    states = gauss_states()
    T = np.array([len(s) for s in states], dtype=np.int64)
    seg_start, seg_state = M._ragged_segments(states, T)
    missing = np.random.default_rng(5).random(int(T.sum())) < 0.1
    return T, seg_start, seg_state, missing


def gauss_oracle(model, seed, shift=0, swap=False):
    return np.concatenate([PO.gauss_normals(seed, i + shift, GS.intervals(st), model.ss_order, swap=swap)
                           for i, st in enumerate(gauss_states())])


# ---------------------------------------------------------------- the profile draws

DRAW_LENGTHS = (3, 65, 130)
N_DRAWS = 200           # 50 waves: several workgroups and a partial last one
DRAW_K_MAX = 4
DRAW_CASES = ((2, SEEDS[3]), (4, MIXED))        # (S, seed)
DWELL_STREAMS = (0, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 5)


def draw_case(S):
    """ (model, three trajectories, dwell-time prior) """
    rng = np.random.default_rng(900 + S)
    model = C.random_model(rng, S, max(DRAW_LENGTHS) + 8)
    if S == 3:
        model.transitions[0, 2] = True
    xs = [C.random_traj(rng, T) for T in DRAW_LENGTHS]
    prior = DC.make_prior('markov', rng, S, max(DRAW_LENGTHS))
    return model, xs, prior


def draw_ks():
    """ (3, N_DRAWS): k cycles over 0 ... min(DRAW_K_MAX, T - 1) """
    return np.array([np.arange(N_DRAWS) % (min(DRAW_K_MAX, T - 1) + 1) for T in DRAW_LENGTHS])


# ---------------------------------------------------------------- the AMIS draws

AMIS_N = 1000
FRAGILE_CAP = 0.01

FORBID = np.array([[1, 1, 0], [1, 1, 1], [1, 1, 1]], dtype=bool)        # 0 -> 2 forbidden


def _logp(S, k1, seed):
    p = np.random.default_rng(seed).dirichlet(np.ones(S) * 2.0, size=k1).T
    return np.log(p)


# name -> (number of states, a0, seed of the slot weights, seed of the stream)
AMIS_CASES = {
    'regimes_s2': (2, (0.3, 2.5, 7.0, 40.0), 1, MIXED),
    'ones_s3_forbidden': (3, (1.0, 1.0, 1.0, 1.0), 2, SEEDS[3]),
    'corner_s2': (2, (1e-320,) * 3, 3, SEEDS[1]),
    'regimes_s3_forbidden': (3, (0.3, 2.5, 7.0, 40.0), 4, SEEDS[0]),
    'k1_5_s2': (2, (0.3, 2.5, 7.0, 40.0, 1.0), 1, MIXED),              # regimes_s2's seed with k1 one larger
}


def amis_case(name):
    """ (transitions, a0, logp0, seed) """
    S, a0, wseed, seed = AMIS_CASES[name]
    trans = FORBID if S == 3 else np.ones((2, 2), dtype=bool)
    return trans, np.array(a0), _logp(S, len(a0), wseed), seed


def amis_target(S):
    """ (model, trajectory) whose likelihood the step evaluates: nothing of it enters the draws of the first step """
    rng = np.random.default_rng(40 + S)
    model = bild_amd.MultiStateRouse(5, 1.0, 0.7, d=2, looppositions=[None, (0, -1), (1, 3)][:S], localization_error=0.1)
    st = np.repeat(np.arange(8) % S, 5)
    return model, model.trajectory_from_loopingprofile(st, rng=rng)


@functools.lru_cache(maxsize=None)
def amis_oracle(name):
    """ `philox_oracle.amis_draw` of the first step: ss, thetas, uniforms consumed, fragile """
    trans, a0, logp0, seed = amis_case(name)
    out = PO.amis_draw(seed, len(a0), 0, AMIS_N, a0, PO.amis_prob(logp0), trans)
    for a in out:
        a.setflags(write=False)
    return out
