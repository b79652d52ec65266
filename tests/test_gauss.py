"""
CPU tests of GenericGaussianModel: the NumPy oracle (tests/gauss_oracle.py) against the reference's own logL values
(tests/golden/gauss/*.npz, tests/golden/make_gauss_golden.py), the decomposition into window tables, and the model's
host side -- construction, MSD evaluation, argument errors, the trajectory-length limit and the generator.
"""
import glob
import os

import numpy as np
import pytest

import gauss_oracle as G

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDENS = sorted(glob.glob(os.path.join(HERE, 'golden', 'gauss', '*.npz')))


def load(path):
    z = np.load(path)
    return {k: z[k] for k in z.files}


def test_goldens_present():
    assert len(GOLDENS) == 4


@pytest.mark.parametrize('path', GOLDENS, ids=os.path.basename)
def test_oracle_reproduces_reference(path):
    g = load(path)
    args = (g['msd'], g['msd_inf'], g['mean'], g['order'], g['x'])
    W, F = G.tables(*args)
    for p, want in zip(g['profiles'], g['logL']):
        assert abs(G.logl_reference(*args, p) - want) <= 1e-10 * max(1.0, abs(want))
        assert abs(G.logl_tables(W, F, p) - want) <= 1e-10 * max(1.0, abs(want))


def test_goldens_cover_the_cases():
    seen = {'d1': False, 'd3': False, 's2': False, 's3': False, 'mixed': False, 'mean': False, 'frame0': False,
            'one_frame': False, 'switch1': False, 'switchT1': False}
    for path in GOLDENS:
        g = load(path)
        S, d = g['order'].shape
        seen['d%d' % d] = seen['s%d' % S] = True
        seen['mixed'] |= len(np.unique(g['order'])) == 2
        seen['mean'] |= bool(np.any(g['mean'] != 0))
        seen['frame0'] |= bool(np.any(np.isnan(g['x'][0])))
        T = g['x'].shape[0]
        for p in g['profiles']:
            ivs = G.intervals(p)
            seen['one_frame'] |= any(t1 - t0 == 1 for t0, t1, _ in ivs)
            seen['switch1'] |= len(ivs) > 1 and ivs[1][0] == 1
            seen['switchT1'] |= len(ivs) > 1 and ivs[-1][0] == T - 1
    assert all(seen.values()), seen


def spec_from(g, callables=True):
    S, d = g['order'].shape
    out = []
    for n in range(S):
        row = []
        for k in range(d):
            o = int(g['order'][n, k])
            arr = g['msd'][n, k] if o == 1 else np.append(g['msd'][n, k], g['msd_inf'][n, k])
            row.append((arr, g['mean'][n, k], o))
        out.append(row)
    return out


def test_model_construction_from_arrays_and_callables():
    import bild_amd
    g = load(GOLDENS[-1])
    m = bild_amd.GenericGaussianModel(spec_from(g))
    S, d = g['order'].shape
    assert (m.nStates, m.d) == (S, d)
    assert m.transitions.shape == (S, S) and not m.transitions.diagonal().any()
    np.testing.assert_array_equal(m.msd, g['msd'])
    np.testing.assert_array_equal(m.msd_inf[g['order'] == 0], g['msd_inf'][g['order'] == 0])
    assert m.max_T == g['msd'].shape[2]

    calls = []
    def powerlaw(dt):
        calls.append(np.shape(dt))
        return np.where(np.isinf(dt), 1e6, 2.0 * np.asarray(dt, dtype=float) ** 0.7)
    m2 = bild_amd.GenericGaussianModel([[(powerlaw, 0.0, 0)], [(powerlaw, 0.1, 1)]])
    assert m2.msd.shape == (2, 1, 2048) and m2.max_T == 2048
    np.testing.assert_allclose(m2.msd[0, 0, :5], 2.0 * np.arange(5.0) ** 0.7)
    assert m2.msd_inf[0, 0] == 1e6
    assert len(calls) == 3      # lags of both states, inf of the ss_order-0 state: evaluated once each

    scalar_only = lambda t: float(t) ** 0.5 if np.isfinite(t) else 1e3     # not vectorised
    m3 = bild_amd.GenericGaussianModel([[(scalar_only, 0, 0)], [(scalar_only, 0, 0)]])
    np.testing.assert_allclose(m3.msd[0, 0, :4], np.sqrt(np.arange(4.0)))
    with pytest.raises(NotImplementedError):
        m3.initial_loopingprofile(None)


def test_argument_errors():
    import bild_amd
    ok = np.r_[np.arange(10.0), 100.0]
    with pytest.raises(ValueError):
        bild_amd.GenericGaussianModel([[(ok, 0, 2)]])                   # ss_order
    with pytest.raises(ValueError):
        bild_amd.GenericGaussianModel([[(ok, 0, 0)], [(ok, 0)]])        # not (S, d, 3)
    with pytest.raises(ValueError):
        bild_amd.GenericGaussianModel([[(ok, 0, 0)], [(ok, 0, 0), (ok, 0, 0)]])
    with pytest.raises(ValueError):
        bild_amd.GenericGaussianModel([[(ok, np.nan, 0)]])              # mean
    with pytest.raises(ValueError):
        bild_amd.GenericGaussianModel([[(np.r_[0.0, np.inf, 1.0], 0, 0)]])
    with pytest.raises(ValueError):
        bild_amd.GenericGaussianModel([[(lambda t: np.asarray(t) * 1.0, 0, 0)]])     # msd(inf) = inf
    m = bild_amd.GenericGaussianModel([[(ok, 0, 0)], [(ok, 0, 1)]])
    assert m.max_T == 10
    with pytest.raises(ValueError, match='10'):                         # beyond the MSD lags: before any device work
        m.logL(bild_amd.Loopingprofile(np.zeros(11, dtype=int)), np.zeros((11, 1)))
    with pytest.raises(ValueError):
        m.trajset(np.zeros((5, 2)))                                     # d mismatch


def test_trajectory_limit():
    import bild_amd
    f = lambda t: np.where(np.isinf(t), 1e9, np.asarray(t, dtype=float))
    m = bild_amd.GenericGaussianModel([[(f, 0, 0)], [(f, 0, 0)]])
    with pytest.raises(ValueError, match='2048'):
        m.trajset(np.zeros((2049, 1)))


def test_native_refuses_long_trajectories(built_lib):
    # the C ABI names the limit too, before it touches a device
    from bild_amd import _lib
    L = 2100
    msd = np.tile(np.arange(L + 1.0), (2, 1, 1))
    h = _lib.GaussModelHandle(np.zeros((2, 1)), np.zeros((2, 1)), msd, np.full((2, 1), 1e5))
    with pytest.raises(_lib.BildAmdError, match='2048'):
        _lib.GaussTrajSetHandle(h, [np.zeros((2049, 1))])
    with pytest.raises(_lib.BildAmdError, match='ss_order'):
        _lib.GaussModelHandle(np.full((2, 1), 3), np.zeros((2, 1)), msd, np.full((2, 1), 1e5))


def test_trajectory_from_loopingprofile():
    import bild_amd
    g = load(GOLDENS[2])
    m = bild_amd.GenericGaussianModel(spec_from(g))
    T = 100
    prof = bild_amd.Loopingprofile(np.repeat([0, 1, 0], [30, 40, 30]))
    t = m.trajectory_from_loopingprofile(prof, rng=np.random.default_rng(0))
    assert t[:].shape == (T, m.d) and np.all(np.isfinite(t[:]))
    assert t.meta['loopingprofile'] is prof
    t2 = m.trajectory_from_loopingprofile(prof, rng=np.random.default_rng(0))
    np.testing.assert_array_equal(t[:], t2[:])
    # ss_order 1, first interval: the trajectory starts at 0
    assert t[0][g['order'][0] == 1].tolist() == [0.0] * int(np.sum(g['order'][0] == 1))
    t = m.trajectory_from_loopingprofile(prof, missing_frames=[0, 5, 99], rng=np.random.default_rng(1))
    assert np.all(np.isnan(t[:][[0, 5, 99]])) and np.sum(np.isnan(t[:])) == 3 * m.d
    t = m.trajectory_from_loopingprofile(prof, missing_frames=7, rng=np.random.default_rng(2))
    assert np.sum(np.all(np.isnan(t[:]), axis=1)) == 7
    t = m.trajectory_from_loopingprofile(prof, missing_frames=0.3, rng=np.random.default_rng(3))
    assert 0 < np.sum(np.all(np.isnan(t[:]), axis=1)) < T


def test_generator_matches_the_model_statistics():
    # ss_order 0 in the first interval: frames are N(m, C); a cheap check of the sampled variance at one frame
    import bild_amd
    lags = np.arange(60.0)
    arr = np.append(np.where(lags > 0, lags ** 0.5 + 0.2, 0), 40.0)
    m = bild_amd.GenericGaussianModel([[(arr, 1.5, 0)], [(arr, 0, 0)]])
    rng = np.random.default_rng(5)
    prof = bild_amd.Loopingprofile(np.zeros(20, dtype=int))
    xs = np.array([m.trajectory_from_loopingprofile(prof, rng=rng)[:][10, 0] for _ in range(4000)])
    assert abs(xs.mean() - 1.5) < 0.25 and abs(xs.var() / 20.0 - 1) < 0.1
