"""
GenericGaussianModel on the GPU: the interval tables and the walk (bild_amd/csrc/gauss.hip) against the reference's own
values (tests/golden/gauss/*.npz) and the NumPy oracle (tests/gauss_oracle.py), the entry points against each other,
and the samplers driven by it.
"""
import glob
import os

import numpy as np
import pytest

import gauss_oracle as G
from gauss_table_cases import model_from, random_case

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDENS = sorted(glob.glob(os.path.join(HERE, 'golden', 'gauss', '*.npz')))


def load(path):
    z = np.load(path)
    return {k: z[k] for k in z.files}


def random_states(rng, n, T, S, kmax=6):
    out = np.zeros((n, T), dtype=int)
    for r in range(n):
        k = rng.integers(0, min(kmax, T - 1) + 1)
        cuts = np.sort(rng.choice(np.arange(1, T), size=k, replace=False))
        st = rng.integers(0, S, size=k + 1)
        out[r] = np.repeat(st, np.diff(np.r_[0, cuts, T]))
    return out


@pytest.mark.parametrize('path', GOLDENS, ids=os.path.basename)
def test_goldens(path):
    g = load(path)
    m = model_from(g['msd'], g['msd_inf'], g['mean'], g['order'])
    got = m.logL_batch(g['profiles'], g['x'])
    np.testing.assert_allclose(got, g['logL'], rtol=0, atol=1e-8)


@pytest.mark.parametrize('p_missing', [0.0, 0.1])
def test_random_T1000_against_oracle(p_missing):
    rng = np.random.default_rng(7 + int(100 * p_missing))
    S, d, T = 2, 3, 1000
    msd, inf, mean, order, x = random_case(rng, S, d, T, p_missing)
    if p_missing:
        x[0, 1] = np.nan
    m = model_from(msd, inf, mean, order)
    states = random_states(rng, 24, T, S)
    got = m.logL_batch(states, x)
    want = np.array([G.logl_reference(msd, inf, mean, order, x, s) for s in states])
    assert np.all(np.isfinite(want))
    np.testing.assert_allclose(got, want, rtol=1e-11, atol=1e-8)


def test_window_without_valid_frame_is_nan_for_that_candidate_only():
    rng = np.random.default_rng(3)
    S, d, T = 2, 2, 60
    msd, inf, mean, order, x = random_case(rng, S, d, T, 0.0)
    order[:] = 0
    x[20:30, 1] = np.nan      # dimension 1: a 10-frame gap
    m = model_from(msd, inf, mean, order)
    bad = np.zeros(T, dtype=int); bad[22:27] = 1           # window [21, 27) has no valid frame in dimension 1
    good = np.zeros(T, dtype=int); good[15:40] = 1
    got = m.logL_batch(np.stack([good, bad, good]), x)
    assert np.isnan(got[1]) and np.all(np.isfinite(got[[0, 2]]))
    assert np.isnan(G.logl_reference(msd, inf, mean, order, x, bad))
    np.testing.assert_allclose(got[0], G.logl_reference(msd, inf, mean, order, x, good), rtol=1e-11, atol=1e-9)


def st_batch(rng, n, k, S):
    ss = rng.dirichlet(np.ones(k + 1), size=n)
    thetas = np.zeros((n, k + 1), dtype=np.int64)
    thetas[:, 0] = rng.integers(S, size=n)
    for i in range(1, k + 1):
        thetas[:, i] = (thetas[:, i - 1] + rng.integers(1, S, size=n)) % S
    return ss, thetas


def test_entry_points_agree_bit_for_bit():
    import bild_amd
    from bild_amd.amis import FixedkSampler
    rng = np.random.default_rng(11)
    S, d, T = 3, 2, 300
    msd, inf, mean, order, x = random_case(rng, S, d, T, 0.05)
    m = model_from(msd, inf, mean, order)
    traj = bild_amd.Trajectory(x)
    ss, thetas = st_batch(rng, 200, 3, S)
    sampler = FixedkSampler(traj, m, k=3, N=10)
    profiles = [sampler.st2profile(s, th) for s, th in zip(ss, thetas)]
    states = np.stack([np.asarray(p[:]) for p in profiles])
    a = m.logL_st_batch(ss, thetas, traj)
    b = m.logL_batch(states, traj)
    from bild_amd.profiles import segments_from_states
    c = m.logL_segments(*segments_from_states(states), traj)
    e = np.array([m.logL(p, traj) for p in profiles[:20]])
    f = np.array([m.logL_st(s, th, traj) for s, th in zip(ss[:20], thetas[:20])])
    assert a.tobytes() == b.tobytes() == c.tobytes()
    assert e.tobytes() == a[:20].tobytes() == f.tobytes()
    want = np.array([G.logl_reference(msd, inf, mean, order, x, s) for s in states[:30]])
    np.testing.assert_allclose(a[:30], want, rtol=1e-11, atol=1e-8)


def test_st_conversion_pinned_to_golden():
    # the device conversion of (s, theta) rows against the reference's st2profile (tests/golden/st2profile.npz): the
    # (s, theta) entry gives bit for bit what the reference's expanded profiles give
    z = np.load(os.path.join(HERE, 'golden', 'st2profile.npz'))
    rng = np.random.default_rng(2)
    models = {}
    checked = 0
    i = 0
    while f'ss_{i}' in z.files:
        ss, thetas, states = z[f'ss_{i}'], z[f'thetas_{i}'], z[f'states_{i}'].astype(int)
        T, S = int(z[f'T_{i}']), max(int(z[f'S_{i}']), 2)
        i += 1
        if T < 2:
            continue
        if (T, S) not in models:
            msd, inf, mean, order, x = random_case(rng, S, 1, T, 0.0)
            models[T, S] = (model_from(msd, inf, mean, order), x)
        m, x = models[T, S]
        got = m.logL_st_batch(ss, thetas, x)
        assert got.tobytes() == m.logL_batch(states, x).tobytes()
        checked += 1
    assert checked > 0


def test_batch_invariance():
    rng = np.random.default_rng(5)
    S, d, T = 2, 3, 400
    msd, inf, mean, order, x = random_case(rng, S, d, T, 0.1)
    m = model_from(msd, inf, mean, order)
    ss, thetas = st_batch(rng, 3000, 4, S)
    full = m.logL_st_batch(ss, thetas, x)
    perm = rng.permutation(len(ss))
    assert m.logL_st_batch(ss[perm], thetas[perm], x).tobytes() == full[perm].tobytes()
    assert m.logL_st_batch(ss[:7], thetas[:7], x).tobytes() == full[:7].tobytes()
    assert m.logL_st_batch(ss[1234:1235], thetas[1234:1235], x).tobytes() == full[1234:1235].tobytes()


def test_multi_trajectory_set():
    rng = np.random.default_rng(9)
    S, d = 2, 2
    msd, inf, mean, order, _ = random_case(rng, S, d, 250, 0.0)
    m = model_from(msd, inf, mean, order)
    trajs = [random_case(rng, S, d, T, 0.1)[4] for T in (50, 250, 1, 120)]
    n = 60
    tid = rng.integers(0, len(trajs), size=n).astype(np.int32)
    from bild_amd.profiles import segments_from_states
    rows = [random_states(rng, 1, len(trajs[j]), S)[0] for j in tid]
    K1 = 8
    seg_start = np.zeros((n, K1), dtype=np.int32)
    seg_state = np.zeros((n, K1), dtype=np.int32)
    for r, st in enumerate(rows):
        a, b = segments_from_states(st[None, :])
        seg_start[r, :] = len(st)
        seg_start[r, :a.shape[1]], seg_state[r, :a.shape[1]] = a[0], b[0]
        seg_state[r, a.shape[1]:] = b[0, -1]
    got = m.logL_segments(seg_start, seg_state, trajs, tid)
    alone = np.array([m.logL_batch(st[None, :], trajs[j])[0] for st, j in zip(rows, tid)])
    want = np.array([G.logl_reference(msd, inf, mean, order, trajs[j], st) for st, j in zip(rows, tid)])
    np.testing.assert_allclose(got, want, rtol=1e-11, atol=1e-8)
    np.testing.assert_allclose(got, alone, rtol=1e-13, atol=1e-10)
    from bild_amd import _lib
    with pytest.raises(_lib.BildAmdError):
        m.logL_segments(seg_start, seg_state, trajs, np.full(n, 4, dtype=np.int32))


def test_table_info():
    rng = np.random.default_rng(1)
    msd, inf, mean, order, x = random_case(rng, 2, 3, 200, 0.1)
    m = model_from(msd, inf, mean, order)
    b, ms = m.trajset(x).info()
    assert b == 8 * 2 * (200 * 201 // 2 + 201) and ms > 0


class OracleModel:
    """ the same model on the CPU, through the NumPy decomposition: what the samplers see of the GPU model """

    def __init__(self, gm, x):
        self.transitions = gm.transitions
        self.nStates, self.d = gm.nStates, gm.d
        self.W, self.F = G.tables(gm.msd, gm.msd_inf, gm.mean, gm.ss_order, x)

    def logL(self, profile, traj):
        return G.logl_tables(self.W, self.F, np.asarray(profile[:]))


def test_fixedk_sampler_steps_equal_oracle():
    import bild_amd
    from bild_amd.amis import FixedkSampler
    rng = np.random.default_rng(4)
    S, d, T = 2, 2, 80
    msd, inf, mean, order, x = random_case(rng, S, d, T, 0.05)
    gm = model_from(msd, inf, mean, order)
    traj = bild_amd.Trajectory(x)
    om = OracleModel(gm, x)
    out = []
    for model in (gm, om):
        np.random.seed(17)
        s = FixedkSampler(traj, model, k=2, N=40)
        for _ in range(4):
            s.step()
        out.append((np.array(s.evidences), s._arr['logLs'].copy()))
    np.testing.assert_allclose(out[0][1], out[1][1], rtol=1e-11, atol=1e-9)
    np.testing.assert_allclose(out[0][0], out[1][0], rtol=1e-9, atol=1e-9)


def test_core_sample_native_segments_driver_equals_python_driver():
    import bild_amd
    rng = np.random.default_rng(8)
    S, d, T = 2, 1, 60
    msd, inf, mean, order, _ = random_case(rng, S, d, T, 0.0)
    gm = model_from(msd, inf, mean, order)
    prof = bild_amd.Loopingprofile(np.repeat([0, 1, 0], [20, 20, 20]))
    traj = gm.trajectory_from_loopingprofile(prof, rng=rng)
    res = []
    for driver in ('native', 'python'):
        np.random.seed(3)
        r = bild_amd.sample(traj, gm, driver=driver, k_max=3, init_runs=3, sampler_kw=dict(N=30, max_fev=600))
        res.append(r)
    assert [s.k for s in res[0].samplers] == [s.k for s in res[1].samplers]
    np.testing.assert_allclose(res[0].evidence, res[1].evidence, rtol=1e-12, atol=1e-12)
