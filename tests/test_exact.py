"""
Exact evidence by enumeration (bild_amd.exact), the parts that need no GPU: the profile count of the C ABI, the NumPy
oracle (tests/exact_oracle.py) against FixedkSampler's exhaustive path on the CPU likelihood double, and the refusals of
`exact_evidence` that come before any device work.
"""
import math

import numpy as np
import pytest
from scipy import stats

import bild_amd
import exact_oracle as X
from bild_amd import _lib
from bild_amd.amis import CFC
from bild_amd.profiles import states_from_segments


def masks(S):
    full = np.ones((S, S), dtype=bool)
    switch = ~np.eye(S, dtype=bool)
    restricted = switch.copy()
    restricted[0, S - 1] = False
    return [full, switch, restricted]


@pytest.mark.parametrize('S', [2, 3])
def test_count_matches_combinatorics(built_lib, S):
    for tr in masks(S):
        for k in range(7):
            for T in (1, 2, 3, 4, 7, 40, 200):
                want = math.comb(T - 1, k) * CFC(tr).N_total(k)
                assert _lib.exact_count(T, k, tr) == want, (tr.tolist(), k, T)
                assert bild_amd.exact.profile_count(T, k, tr) == want


def test_count_refusals(built_lib):
    tr = ~np.eye(2, dtype=bool)
    with pytest.raises(_lib.BildAmdError):
        _lib.exact_count(10, 16, tr)
    with pytest.raises(_lib.BildAmdError):
        _lib.exact_count(0, 1, tr)
    with pytest.raises(ValueError):
        _lib.exact_count(10, 1, np.ones((2, 3), dtype=bool))


def test_enumeration_order(built_lib):
    tr = masks(3)[2]
    seg_start, seg_state = X.enumerate_profiles(6, 2, tr)
    traces = CFC(tr).full_sample(2, Nmax=np.inf)
    assert len(seg_start) == math.comb(5, 2) * len(traces) == _lib.exact_count(6, 2, tr)
    assert np.array_equal(seg_start[:3], [[0, 1, 2], [0, 1, 3], [0, 1, 4]])
    assert np.array_equal(seg_state[:10], np.repeat(traces[:1], 10, axis=0))
    assert np.array_equal(seg_state[10], traces[1])
    for T, k in ((1, 0), (2, 2), (3, 3)):
        s, v = X.enumerate_profiles(T, k, tr)
        assert len(s) == _lib.exact_count(T, k, tr)


def factorized_case(seed, T, S, missing=()):
    rng = np.random.default_rng(seed)
    np.random.seed(seed)
    model = bild_amd.FactorizedModel([stats.maxwell(scale=s) for s in (0.3, 1.0, 2.5)[:S]])
    truth = bild_amd.Loopingprofile(np.repeat(rng.integers(0, S, 3), [T // 3, T // 3, T - 2 * (T // 3)]))
    traj = model.trajectory_from_loopingprofile(truth, missing_frames=np.asarray(missing, dtype=int))
    return model, traj


@pytest.mark.parametrize('S,T,k,restrict,missing', [
    (2, 12, 0, False, ()),
    (2, 12, 1, False, (0, 1, 5)),
    (2, 10, 2, False, ()),
    (3, 9, 2, True, (0, 4)),
    (3, 8, 3, True, ()),
    (2, 3, 3, False, ()),
])
def test_oracle_matches_fix_exhaustive(built_lib, S, T, k, restrict, missing):
    model, traj = factorized_case(S * 100 + T * 10 + k, T, S, missing)
    if restrict:
        model.transitions[0, S - 1] = False
    sampler = bild_amd.FixedkSampler(traj, model, k=k, max_fcomplete=10 ** 7, max_fev=10 ** 7)
    seg_start, seg_state = X.enumerate_profiles(T, k, model.transitions)
    logL = model.logL_batch(states_from_segments(seg_start, seg_state, T), traj) if len(seg_start) else np.zeros(0)
    got = X.reduce(logL, seg_start, seg_state, T, S)
    assert got['n_profiles'] == _lib.exact_count(T, k, model.transitions)
    if T - 1 < k:
        assert got['logev'] == -np.inf and np.isnan(got['KL']) and got['map_index'] == -1
        assert sampler.evidences[-1][0] == -np.inf
        return
    assert sampler.exhausted
    logev, _, KL = sampler.evidences[-1]
    assert abs(got['logev'] - logev) < 1e-12
    assert abs(got['KL'] - KL) < 1e-10
    assert np.array_equal(states_from_segments(seg_start[got['map_index']:got['map_index'] + 1],
                                               seg_state[got['map_index']:got['map_index'] + 1], T)[0],
                          sampler.MAP_profile()[:])
    want = sampler.log_marginal_posterior()
    fin = np.isfinite(want)
    assert np.array_equal(fin, np.isfinite(got['log_post']))
    assert np.max(np.abs(got['log_post'][fin] - want[fin])) < 1e-10


def test_oracle_edge_cases():
    seg_start, seg_state = X.enumerate_profiles(4, 1, ~np.eye(2, dtype=bool))
    logL = np.array([-3.0, -np.inf, -1.0, -1.0, -2.0, -5.0])
    got = X.reduce(logL, seg_start, seg_state, 4, 2)
    assert got['map_index'] == 2 and got['map_logL'] == -1.0
    assert np.isfinite(got['KL'])                   # -inf weighs 0 and adds 0 (the host's formula gives NaN)
    logL[4] = np.nan
    got = X.reduce(logL, seg_start, seg_state, 4, 2)
    assert got['n_nan'] == 1 and np.isnan(got['logev']) and np.isnan(got['KL']) and got['map_index'] == 2


def rouse_model():
    return bild_amd.MultiStateRouse(20, 1, 5, d=3, localization_error=0.1)


def test_refusals_before_device(built_lib):
    # none of these may reach a trajectory set: they raise the same on a machine without a GPU
    model = rouse_model()
    traj = bild_amd.Trajectory(np.zeros((50, 3)), localization_error=[0.1] * 3)
    with pytest.raises(ValueError, match='k = 16'):
        bild_amd.exact_evidence(traj, model, 16)
    with pytest.raises(ValueError, match='k = -1'):
        bild_amd.exact_evidence(traj, model, -1)
    with pytest.raises(ValueError, match='36848 profiles'):
        bild_amd.exact_evidence(traj, model, 3, max_profiles=1000)
    with pytest.raises(ValueError, match='exceed max_profiles'):
        bild_amd.exact_evidence([traj, traj], model, 2, max_profiles=2 * 1176 * 2 - 1)
    with pytest.raises(TypeError):
        bild_amd.exact_evidence(traj, bild_amd.FactorizedModel([stats.maxwell(), stats.maxwell()]), 1)
    with pytest.raises(ValueError, match='marginals'):
        bild_amd.exact_evidence(bild_amd.Trajectory(np.zeros((5000, 3)), localization_error=[0.1] * 3), model, 1)
    assert model._trajsets == {} or len(model._trajsets) == 0
