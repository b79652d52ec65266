"""
CPU tests of the batched GenericGaussianModel generator (GenericGaussianModel.trajectories_from_loopingprofiles): the
loop's normals scattered to their (frame, dimension) and run through the generator's algebra (one Toeplitz factor per
state and dimension, restated in NumPy in gauss_sim_cases.py) against the loop of trajectory_from_loopingprofile; the
replay mode's host side -- draws, packing, grouping, the Generator's end state -- with the library call replaced by that
restatement; and the argument errors, which come before any library call.
"""
import copy

import numpy as np
import pytest

import bild_amd
from bild_amd import _lib
from bild_amd import gauss as GM

import gauss_sim_cases as C

MISSING = [None, 0, 0.3, 1, np.array([0, -1]), 'per-trajectory']


def cases(S, d, seed, lengths=(1, 2, 37, 700)):
    rng = np.random.default_rng(seed)
    return [bild_amd.Loopingprofile(C.profile(rng, T, S, sw)) for T in lengths for sw in (0, 1, 7)]


def per_trajectory(n):
    return [[None, 0.2, 1, np.array([0]), 0][i % 5] for i in range(n)]


def loop(model, profiles, missing, rng):
    specs = missing if isinstance(missing, list) else [missing] * len(profiles)
    return [model.trajectory_from_loopingprofile(p, m, rng=rng) for p, m in zip(profiles, specs)]


@pytest.mark.parametrize('S,d', [(2, 1), (2, 3), (3, 1), (3, 3)])
def test_scattered_normals_through_the_factors_equal_the_loop(S, d):
    model = C.make_model(S, d, seed=10 * S + d, L=800)
    profiles = cases(S, d, seed=S + d)
    L = C.factors(model, 700)
    rng = np.random.default_rng(5)
    for p in profiles:
        states = np.asarray(p[:])
        T = len(states)
        clone = copy.deepcopy(rng)
        want = model.trajectory_from_loopingprofile(p, rng=rng)[:]
        per = GM.normals_per_trajectory(model.ss_order, [states[0]], [T])
        _, z = bild_amd.models._draw_normals([None], [T], per, clone)
        assert clone.random() == copy.deepcopy(rng).random()        # the loop drew exactly these
        got = C.restate(model, states, z, L)
        scale = np.max(np.abs(want))
        assert np.max(np.abs(got - want)) <= 1e-12 * scale


def test_every_normal_has_one_slot():
    """ the scatter fills every (frame, dimension) but frame 0 of a dimension whose first state has ss_order 1 """
    model = C.make_model(3, 3, seed=4, L=100)
    rng = np.random.default_rng(0)
    for T in (1, 2, 50):
        for sw in (0, 1, 10):
            states = C.profile(rng, T, 3, sw)
            n = int(GM.normals_per_trajectory(model.ss_order, [states[0]], [T])[0])
            Z = C.scatter_normals(model, states, np.arange(n, dtype=np.float64))
            assert np.array_equal(np.isnan(Z[0]), model.ss_order[states[0]] == 1)
            assert not np.isnan(Z[1:]).any()
            assert sorted(Z[~np.isnan(Z)].tolist()) == list(range(n))


def fake_simulate(model, calls):
    """ bild_gauss_simulate's replay mode restated: the library call of the method, replaced """
    def run(handle, T, seg_start, seg_state, missing, normals=None, seed=0, scratch_bytes=0):
        assert normals is not None
        calls.append(len(T))
        out, zo, ro = [], 0, 0
        for i, Ti in enumerate(T):
            states = np.empty(Ti, dtype=np.int64)
            starts = [min(a, Ti) for a in seg_start[i]] + [Ti]
            for q in range(len(seg_state[i])):
                states[starts[q]:starts[q + 1]] = seg_state[i][q]
            n = int(GM.normals_per_trajectory(model.ss_order, [states[0]], [Ti])[0])
            x = C.restate(model, states, normals[zo:zo + n])
            x[missing[ro:ro + Ti]] = np.nan
            out.append(x)
            zo, ro = zo + n, ro + Ti
        assert zo == len(normals)
        return np.concatenate(out)
    return run


@pytest.mark.parametrize('missing', MISSING)
@pytest.mark.parametrize('S,d', [(2, 3), (3, 1)])
def test_replay_host_side_follows_the_loop(monkeypatch, missing, S, d):
    model = C.make_model(S, d, seed=S * d, L=800)
    profiles = cases(S, d, seed=7, lengths=(1, 2, 37, 120))
    if isinstance(missing, str):
        missing = per_trajectory(len(profiles))
    calls = []
    monkeypatch.setattr(_lib, 'gauss_simulate', fake_simulate(model, calls))
    rng = np.random.default_rng(99)
    clone = copy.deepcopy(rng)
    want = loop(model, profiles, missing, rng)
    got = model.trajectories_from_loopingprofiles(profiles, missing_frames=missing, rng=clone)
    C.compare(got, want, 1e-12)
    assert clone.random() == rng.random()       # the Generator is left where the loop leaves it
    assert calls == [len(profiles)]


def test_replay_groups_and_int_profiles(monkeypatch):
    """ several host groups of normals (a small group size), integer arrays and an (n, T) array as profiles """
    model = C.make_model(2, 3, seed=1, L=300)
    rng0 = np.random.default_rng(3)
    arr = np.stack([C.profile(rng0, 200, 2, 3) for _ in range(6)])
    calls = []
    monkeypatch.setattr(_lib, 'gauss_simulate', fake_simulate(model, calls))
    monkeypatch.setattr(GM, '_REPLAY_GROUP_BYTES', 2 * 600 * 8)
    rng = np.random.default_rng(4)
    clone = copy.deepcopy(rng)
    want = loop(model, [bild_amd.Loopingprofile(p) for p in arr], 0.1, rng)
    got = model.trajectories_from_loopingprofiles(arr, missing_frames=0.1, rng=clone)
    assert len(calls) == 3 and sum(calls) == 6
    for g, w in zip(got, want):
        assert np.array_equal(np.isnan(g[:]), np.isnan(w[:]))
        ok = ~np.isnan(w[:])
        assert np.max(np.abs(g[:][ok] - w[:][ok])) <= 1e-12 * np.max(np.abs(w[:][ok]))
    assert clone.random() == rng.random()


def test_normals_per_trajectory():
    order = np.array([[0, 1, 1], [1, 0, 0]])
    assert GM.normals_per_trajectory(order, [0, 1, 1], [5, 5, 1]).tolist() == [13, 14, 2]


@pytest.mark.parametrize('bad', ['state', 'negative', 'long', 'lags', 'empty', 'float', 'both', 'list', 'seed'])
def test_argument_errors_before_the_library(monkeypatch, bad):
    model = C.make_model(2, 2, seed=3, L=100)

    def touched(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, 'gauss_simulate', touched)
    monkeypatch.setattr(model, 'handle', touched)
    profiles = [np.zeros(10, dtype=int), np.ones(20, dtype=int)]
    kw = {}
    if bad == 'state':
        profiles[1][5] = 2
    elif bad == 'negative':
        profiles[0][0] = -1
    elif bad == 'long':
        big = C.make_model(2, 2, seed=3, L=2100)
        monkeypatch.setattr(big, 'handle', touched)
        with pytest.raises(ValueError, match='at most 2048'):
            big.trajectories_from_loopingprofiles([np.zeros(2049, dtype=int)], seed=1)
        return
    elif bad == 'lags':
        profiles[1] = np.zeros(101, dtype=int)
    elif bad == 'empty':
        profiles[0] = np.zeros(0, dtype=int)
    elif bad == 'float':
        profiles[0] = np.zeros(10)
    elif bad == 'both':
        kw = dict(rng=np.random.default_rng(0), seed=1)
    elif bad == 'list':
        kw = dict(missing_frames=[None, None, None])
    elif bad == 'seed':
        kw = dict(seed=2 ** 64)
    with pytest.raises(ValueError):
        model.trajectories_from_loopingprofiles(profiles, **kw)


def test_no_profiles():
    model = C.make_model(2, 1, seed=0, L=10)
    assert model.trajectories_from_loopingprofiles([], seed=1) == []
