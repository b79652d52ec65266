"""
CPU tests of the batched Rouse generator (MultiStateRouse.trajectories_from_loopingprofiles): the modal form of each
state's dynamics, the host packing of the replay draws against the order in which trajectory_from_loopingprofile draws
them, the modal recurrences the kernel runs (restated in NumPy) against that loop, and the argument errors, which come
before any device work.
"""
import copy

import numpy as np
import pytest

import bild_amd
from bild_amd import models as M
from bild_amd import rouse


def make_model(S, N, d=3, **kw):
    loops = [None, (0, -1), (1, N // 2)][:S]
    return bild_amd.MultiStateRouse(N, 1.0, 1.0, d=d, looppositions=loops, **kw)


@pytest.mark.parametrize('S', [2, 3])
@pytest.mark.parametrize('N', [1, 2, 20, 64])
def test_modal_dynamics_reproduce_the_dense_ones(S, N):
    model = make_model(S, N)
    for m in model.models:
        m.check_dynamics()
        keys = sorted(m._dynamics)
        V, b, sig, cinf = m.modal_dynamics()
        dyn = m._dynamics
        assert sorted(dyn) == keys      # nothing added
        assert np.allclose(V.T @ V, np.eye(N), rtol=0, atol=1e-14)
        assert np.allclose((V * b) @ V.T, dyn['B'], rtol=0, atol=1e-14)
        assert np.allclose(V * np.sqrt(np.maximum(sig, 0)), dyn['LSig'], rtol=0, atol=1e-14)
        assert np.allclose(V * np.sqrt(np.maximum(cinf, 0)), dyn['LC0'], rtol=0, atol=1e-14)


def loop_draws(model, profiles, localization_error, missing_frames, rng):
    """ what the single method's loop takes from rng, restated in NumPy: per trajectory (missing, normals) """
    out = []
    for i, p in enumerate(profiles):
        spec = missing_frames[i] if isinstance(missing_frames, list) else missing_frames
        T, N, d = len(p), model.measurement.shape[0], model.d
        if spec is None or (np.isscalar(spec) and spec == 0):
            miss = np.array([], dtype=int)
        elif np.isscalar(spec) and 0 < spec < 1:
            miss = np.nonzero(rng.random(T) < spec)[0]
        elif np.isscalar(spec):
            miss = rng.choice(T, size=int(spec), replace=False)
        else:
            miss = np.asarray(spec)
        z = [rng.standard_normal((N, d)).ravel()]
        z += [rng.standard_normal((N, d)).ravel() for _ in range(1, T)]
        z.append(rng.standard_normal((T, d)).ravel())
        mask = np.zeros(T, dtype=bool)
        mask[miss] = True
        out.append((mask, np.concatenate(z)))
    return out


@pytest.mark.parametrize('missing', [None, 0.3, 4, np.array([0, 2, -1]), 'per-trajectory'])
def test_replay_packing_follows_the_loop(missing):
    model = make_model(2, 5, d=2, localization_error=0.1)
    prof_rng = np.random.default_rng(1)
    profiles = [prof_rng.integers(0, 2, size=T) for T in (5, 7, 12, 30)]
    if isinstance(missing, str):
        missing = [None, 0.5, 3, np.array([1, 5])]
    specs = missing if isinstance(missing, list) else [missing] * len(profiles)
    rng = np.random.default_rng(123)
    clone = copy.deepcopy(rng)
    mask, z = M._replay_draws(specs, [len(p) for p in profiles], 5, 2, rng)
    want = loop_draws(model, profiles, None, missing, clone)
    assert np.array_equal(mask, np.concatenate([w[0] for w in want]))
    assert np.array_equal(z, np.concatenate([w[1] for w in want]))
    assert rng.random() == clone.random()


def test_replay_draws_match_the_single_method():
    # the same number of draws as the single method itself (not only its restatement above)
    model = make_model(3, 4, d=3, localization_error=0.2)
    profiles = [np.array([0, 1, 1, 2, 0]), np.array([2] * 9)]
    a, b = np.random.default_rng(9), np.random.default_rng(9)
    for p in profiles:
        model.trajectory_from_loopingprofile(p, missing_frames=0.4, rng=a)
    M._replay_draws([0.4, 0.4], [5, 9], 4, 3, b)
    assert a.standard_normal() == b.standard_normal()


def modal_restatement(model, profile, err, mask, z):
    """ the kernel's arithmetic in NumPy: modal recurrences, basis change at a switch, measurement u . x' """
    arrs = model._modal_arrays()
    V, b, ssig, scinf, g, m0 = arrs
    w = model.measurement
    T, N, d = len(profile), w.shape[0], model.d
    zd = z[:T * N * d].reshape(T, N, d)
    zn = z[T * N * d:].reshape(T, d)
    s = profile[0]
    x = m0[s] + scinf[s][:, None] * zd[0]
    y = np.empty((T, d))
    y[0] = (V[s].T @ w) @ x
    for t in range(1, T):
        if profile[t] != s:
            x = V[profile[t]].T @ (V[s] @ x)
            s = profile[t]
        x = b[s][:, None] * x + g[s] + ssig[s][:, None] * zd[t]
        y[t] = (V[s].T @ w) @ x
    y[mask] = np.nan
    return y + err[None, :] * zn


@pytest.mark.parametrize('N,d,measurement', [(1, 1, 'end2end'), (6, 3, 'end2end'), (20, 2, 'com')])
def test_modal_recurrences_equal_the_loop(N, d, measurement):
    w = 'end2end' if measurement == 'end2end' else np.linspace(0.1, 1.0, N)     # sum(w) != 0: the free mode is seen
    model = bild_amd.MultiStateRouse(N, 1.0, 1.0, d=d, looppositions=[None, (0, -1), (1, N // 2)], measurement=w,
                                     localization_error=0.05)
    profile = np.array([0] * 40 + [1] * 30 + [2] * 10 + [0] * 20)
    err = np.full(d, 0.05)
    rng = np.random.default_rng(3)
    clone = copy.deepcopy(rng)
    traj = model.trajectory_from_loopingprofile(profile, missing_frames=0.1, rng=rng)
    mask, z = M._replay_draws([0.1], [len(profile)], N, d, clone)
    got = modal_restatement(model, profile, err, mask, z)
    assert np.array_equal(np.isnan(got), np.isnan(traj[:]))
    ok = ~np.isnan(got)
    assert np.max(np.abs(got[ok] - traj[:][ok])) <= 1e-11 * np.max(np.abs(traj[:][ok]))


def test_ragged_segments_round_trip():
    from bild_amd.profiles import states_from_segments
    rng = np.random.default_rng(0)
    states = [rng.integers(0, 3, size=T) for T in (1, 2, 17, 5)] + [np.zeros(9, dtype=int)]
    T = np.array([len(s) for s in states])
    seg_start, seg_state = M._ragged_segments(states, T)
    for i, st in enumerate(states):
        assert np.array_equal(states_from_segments(seg_start[i:i + 1], seg_state[i:i + 1], T[i])[0], st)
        assert np.all(seg_start[i, 1:] >= 1)


class _NoDevice(Exception):
    pass


@pytest.fixture
def no_device(monkeypatch):
    """ any call into the library's generator fails the test: the errors must come first """
    def boom(*a, **k):
        raise _NoDevice
    monkeypatch.setattr(bild_amd._lib, 'rouse_simulate', boom)


def test_argument_errors_come_before_device_work(no_device):
    model = make_model(2, 5, localization_error=0.1)
    good = [np.array([0, 1, 1])]
    with pytest.raises(ValueError, match='not both'):
        model.trajectories_from_loopingprofiles(good, rng=np.random.default_rng(0), seed=1)
    with pytest.raises(ValueError, match='outside'):
        model.trajectories_from_loopingprofiles([np.array([0, 2, 1])], seed=1)
    with pytest.raises(ValueError, match='outside'):
        model.trajectories_from_loopingprofiles(np.array([[0, 1], [1, -1]]), seed=1)
    with pytest.raises(ValueError, match='entries'):
        model.trajectories_from_loopingprofiles(good, missing_frames=[None, None], seed=1)
    with pytest.raises(ValueError, match='seed'):
        model.trajectories_from_loopingprofiles(good, seed=-1)
    with pytest.raises(ValueError, match='localization_error'):
        model.trajectories_from_loopingprofiles(good, localization_error=[0.1, 0.2], seed=1)
    bare = make_model(2, 5)
    with pytest.raises(ValueError, match='localization_error'):
        bare.trajectories_from_loopingprofiles(good, seed=1)
    a = model.arrays()
    from_arrays = bild_amd.MultiStateRouse.from_arrays(a['B'], a['G'], a['Sig'], a['M0'], a['C0'], model.measurement,
                                                       localization_error=0.1)
    with pytest.raises(ValueError, match='eigenbasis'):
        from_arrays.trajectories_from_loopingprofiles(good, seed=1)
    assert model.trajectories_from_loopingprofiles([], seed=1) == []
    with pytest.raises(_NoDevice):      # and a good call does reach the library
        model.trajectories_from_loopingprofiles(good, seed=1)


def test_replay_error_leaves_the_generator_untouched(no_device):
    model = make_model(2, 5, localization_error=0.1)
    rng = np.random.default_rng(4)
    state = copy.deepcopy(rng.bit_generator.state)
    with pytest.raises(ValueError):
        model.trajectories_from_loopingprofiles([np.array([0, 1]), np.array([3])], rng=rng)
    assert rng.bit_generator.state == state


def test_modal_dynamics_rebuilds_after_a_change():
    m = rouse.Model(6, 1.0, 1.0, d=2)
    V0 = m.modal_dynamics()[0]
    m.add_bond(0, -1)
    V, b, _, _ = m.modal_dynamics()
    assert not np.allclose(V0, V)
    assert np.allclose((V * b) @ V.T, m._dynamics['B'], rtol=0, atol=1e-14)


def test_library_refuses_bad_input_before_the_device():
    from bild_amd import _lib

    def call(S=2, N=4, d=2, T=(3,), seg=((0, 1),), states=((0, 1),), err=0.1, **kw):
        n = len(T)
        V = np.tile(np.eye(N), (S, 1, 1))
        v = np.ones((S, N))
        g = np.zeros((S, N, d))
        return _lib.rouse_simulate(V, v, v, v, g, g, np.ones(N), np.array(T), np.array(seg), np.array(states), None,
                                   np.full((n, d), err), **kw)

    def code(**kw):
        with pytest.raises(_lib.BildAmdError) as e:
            call(**kw)
        return e.value.code

    assert code(N=257) == _lib.ERR_UNSUPPORTED
    assert code(d=9) == _lib.ERR_UNSUPPORTED
    assert code(seg=((1, 2),)) == _lib.ERR_INVALID           # the first segment must start at 0
    assert code(seg=((0, 0),)) == _lib.ERR_INVALID           # later starts >= 1
    assert code(states=((0, 2),)) == _lib.ERR_INVALID        # state out of range
    assert code(T=(0,)) == _lib.ERR_INVALID
    assert code(err=np.nan) == _lib.ERR_INVALID
