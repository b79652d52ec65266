"""
GenericGaussianModel.kalman and kalman_mixture on the GPU (csrc/gauss_kalman.hip), against the NumPy oracle
(tests/gauss_kalman_oracle.py), the device's own likelihood, the reference goldens and the statistics of the innovations
and of the gap filling; bit-identity across batches and chunking; the posterior tracks of sampling results.  `-s` prints
the worst deviations observed.
"""
import glob
import os

import numpy as np
import pytest

import gauss_kalman_oracle as GK

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDENS = sorted(glob.glob(os.path.join(HERE, 'golden', 'gauss', '*.npz')))
ALL = ('terms', 'pred', 'smooth', 'innov')


def load(path):
    z = np.load(path)
    return {k: z[k] for k in z.files}


def model_from(msd, msd_inf, mean, order):
    import bild_amd
    S, d = order.shape
    return bild_amd.GenericGaussianModel(
        [[(msd[n, k] if order[n, k] == 1 else np.append(msd[n, k], msd_inf[n, k]), mean[n, k], int(order[n, k]))
          for k in range(d)] for n in range(S)])


def arrays(model):
    return model.msd, model.msd_inf, model.mean, model.ss_order


def segments(states_list):
    from bild_amd.models import _ragged_segments
    return _ragged_segments([np.asarray(s) for s in states_list], np.array([len(s) for s in states_list]))


def _bits_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def compare(res, want, xscale, label):
    """ every output against the oracle: NaN patterns equal; terms 1e-10 max|term|, means 1e-9 max|x|, variances 1e-9 """
    worst = {}
    for name in GK.OUTPUTS:
        got, ref = getattr(res, name), want[name]
        assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{label}: NaN pattern of {name}"
        ok = ~np.isnan(ref)
        if not ok.any():
            continue
        diff = np.abs(got[ok] - ref[ok])
        if name == 'terms':
            err = float(np.max(diff)) / max(1.0, float(np.max(np.abs(ref[ok]))))
            bar = 1e-10
        elif name.endswith('_var'):
            err = float(np.max(diff / np.maximum(np.abs(ref[ok]), 1e-300) * (ref[ok] != 0) + diff * (ref[ok] == 0)))
            bar = 1e-9
        elif name == 'innov':
            err = float(np.max(diff)) / max(1.0, float(np.max(np.abs(ref[ok]))))
            bar = 1e-9
        else:
            err = float(np.max(diff)) / max(1.0, xscale)
            bar = 1e-9
        worst[name] = err
        assert err < bar, f"{label}: {name} off by {err:.3g}"
    print(f"\n{label}: " + ', '.join(f"{k} {v:.2g}" for k, v in worst.items()))


@pytest.mark.parametrize('path', GOLDENS, ids=os.path.basename)
def test_goldens(built_lib, path):
    g = load(path)
    model = model_from(g['msd'], g['msd_inf'], g['mean'], g['order'])
    states = g['profiles'][:16]
    res = model.kalman(states, g['x'], outputs=ALL)
    want = GK.batch(*arrays(model), [g['x']], list(states))
    compare(res, want, float(np.nanmax(np.abs(g['x']))), os.path.basename(path))
    total = res.terms.sum(axis=(1, 2))
    ok = np.isfinite(g['logL'][:16])
    assert np.array_equal(np.isnan(total), ~ok)
    ll = model.logL_batch(states, g['x'])
    assert np.max(np.abs(total[ok] - ll[ok]) / np.maximum(1.0, np.abs(ll[ok]))) < 1e-10
    assert np.max(np.abs(total[ok] - g['logL'][:16][ok]) / np.maximum(1.0, np.abs(g['logL'][:16][ok]))) < 1e-8


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_cases_against_oracle(built_lib, seed):
    model, cases = GK.cases(seed)
    trajs = [x for x, _ in cases]
    states, tid = [], []
    for j, (x, sl) in enumerate(cases):
        states += list(sl)
        tid += [j] * len(sl)
    tid = np.array(tid, dtype=np.int32)
    seg_start, seg_state = segments(states)
    res = model.kalman((seg_start, seg_state), trajs, traj_id=tid, outputs=ALL)
    want = GK.batch(*arrays(model), trajs, states, traj_id=tid)
    compare(res, want, max(float(np.nanmax(np.abs(x))) for x in trajs), f"cases seed {seed}")
    ll = model.logL_segments(seg_start, seg_state, trajs, tid)
    total = res.terms.reshape(len(states), -1)
    total = np.array([np.sum(r[~np.isnan(r)]) if not np.isnan(l) else np.nan for r, l in zip(total, ll)])
    ok = ~np.isnan(ll)
    assert np.any(~ok)
    assert np.max(np.abs(total[ok] - ll[ok]) / np.maximum(1.0, np.abs(ll[ok]))) < 1e-10
    # the NaN tail behind a shorter trajectory, and the T = 1 trajectory
    short = tid == 1
    assert np.all(np.isnan(res.smooth_mean[short, len(trajs[1]):]))
    assert np.all(np.isnan(res.terms[short, len(trajs[1]):]))


def test_bit_identity(built_lib):
    from gauss_sim_cases import make_model, profile
    rng = np.random.default_rng(5)
    model = make_model(2, 3, 7, L=300)
    T = 250
    truth = [np.full(T, s) for s in (0, 1)]
    trajs = [t[:] for t in model.trajectories_from_loopingprofiles(truth, missing_frames=0.1, seed=3)]
    trajs.append(model.trajectories_from_loopingprofiles([np.zeros(T, dtype=int)], seed=4)[0][:])    # gap-free
    states = [profile(rng, T, 2, sw) for sw in (0, 1, 2, 4, 8) for _ in range(6)]
    tid = (np.arange(len(states)) % 3).astype(np.int32)
    seg = segments(states)
    ref = model.kalman(seg, trajs, traj_id=tid, outputs=ALL)
    perm = rng.permutation(len(states))
    dup = np.concatenate([perm, perm[:7]])
    runs = [
        (model.kalman((seg[0][perm], seg[1][perm]), trajs, traj_id=tid[perm], outputs=ALL), perm),
        (model.kalman((seg[0][dup], seg[1][dup]), trajs, traj_id=tid[dup], outputs=ALL), dup),
        (model.kalman(seg, trajs, traj_id=tid, outputs=ALL, scratch_bytes=1 << 16), np.arange(len(states))),
        (model.kalman(seg, trajs, traj_id=tid, outputs=ALL), np.arange(len(states))),
    ]
    for res, idx in runs:
        for name in GK.OUTPUTS:
            assert _bits_equal(getattr(res, name), getattr(ref, name)[idx]), name
    # one candidate alone
    one = model.kalman((seg[0][3:4], seg[1][3:4]), [trajs[tid[3]]], outputs=ALL)
    for name in GK.OUTPUTS:
        assert _bits_equal(getattr(one, name)[0], getattr(ref, name)[3][:T]), name


def _ks(z):
    from scipy import stats
    z = np.asarray(z)
    p = stats.kstest(z, 'norm').pvalue
    se = 1.0 / np.sqrt(len(z))
    return p, abs(np.mean(z)) / se


def calibration_model():
    """
    A model whose likelihood describes its own generator exactly: each dimension keeps its ss_order across the states, and
    the ss_order-0 dimension has one MSD and mean 0 in both, so that the value a later interval conditions on (raw, as
    in the reference) has the marginal of the new state (its MSDs, means and orders otherwise differ by state)
    """
    import bild_amd
    from gauss_sim_cases import msd_exp, msd_pow
    L = 256
    return bild_amd.GenericGaussianModel([[(msd_exp(1.0, 8.0, 0.3, L), 0.0, 0), (msd_pow(0.5, 0.8, 0.3, L), 0.1, 1)],
                                          [(msd_exp(1.0, 8.0, 0.3, L), 0.0, 0), (msd_pow(1.0, 1.2, 0.4, L), -0.2, 1)]])


def test_calibration_of_innovations(built_lib):
    from gauss_sim_cases import profile
    rng = np.random.default_rng(21)
    model = calibration_model()
    T, n = 200, 2000
    truth = [profile(rng, T, 2, 3) for _ in range(n)]
    trajs = [t[:] for t in model.trajectories_from_loopingprofiles(truth, missing_frames=0.1, seed=5)]
    seg = segments(truth)
    res = model.kalman(seg, trajs, traj_id=np.arange(n, dtype=np.int32), outputs='innov')
    z = res.innov[~np.isnan(res.innov)]
    p, dev = _ks(z)
    print(f"\ninnovations: {len(z)} values, KS p = {p:.3g}, |mean| = {dev:.2f} SE, var = {np.var(z):.4f}")
    assert p > 0.01 and dev < 4


def test_calibration_of_gap_filling(built_lib):
    from gauss_sim_cases import profile
    rng = np.random.default_rng(22)
    model = calibration_model()
    T, n = 200, 2000
    truth = [profile(rng, T, 2, 3) for _ in range(n)]
    full = [t[:] for t in model.trajectories_from_loopingprofiles(truth, seed=6)]
    masked = []
    for x in full:
        m = x.copy()
        m[rng.random(T) < 0.1] = np.nan
        masked.append(m)
    res = model.kalman(segments(truth), masked, traj_id=np.arange(n, dtype=np.int32))
    xs = np.stack(full)
    gap = np.isnan(np.stack(masked)) & ~np.isnan(res.smooth_mean)
    z = (xs[gap] - res.smooth_mean[gap]) / np.sqrt(res.smooth_var[gap])
    p, dev = _ks(z)
    print(f"\ngap filling: {len(z)} values, KS p = {p:.3g}, |mean| = {dev:.2f} SE, var = {np.var(z):.4f}")
    assert p > 0.01 and dev < 4


def _np_mixture(model, seg, trajs, tid, lw):
    """ NumPy weighted average of the per-candidate smoothed tracks, per trajectory """
    res = model.kalman(seg, trajs, traj_id=tid)
    nt, Tm, d = len(trajs), res.smooth_mean.shape[1], model.d
    mean, var = np.full((nt, Tm, d), np.nan), np.full((nt, Tm, d), np.nan)
    for j in range(nt):
        sel = (tid == j) & (lw > -np.inf)
        w = np.exp(lw[sel] - lw[sel].max())
        w /= w.sum()
        m, v = res.smooth_mean[sel], res.smooth_var[sel]
        mean[j] = np.tensordot(w, m, 1)
        var[j] = np.tensordot(w, v + m * m, 1) - mean[j] ** 2
    return mean, var


def test_mixture(built_lib):
    from gauss_sim_cases import make_model, profile
    rng = np.random.default_rng(31)
    model = make_model(2, 3, 9, L=200)
    T = 150
    trajs = [t[:] for t in model.trajectories_from_loopingprofiles([profile(rng, T, 2, 2), profile(rng, 120, 2, 1)],
                                                                  missing_frames=0.1, seed=8)]
    states = [profile(rng, T, 2, sw) for sw in (1, 2, 3) for _ in range(50)]
    states += [profile(rng, 120, 2, sw) for sw in (1, 2) for _ in range(40)]
    tid = np.array([0] * 150 + [1] * 80, dtype=np.int32)
    seg = segments(states)
    lw = rng.normal(scale=3.0, size=len(states))
    lw[[3, 7, 160]] = -np.inf
    mean, var = model.kalman_mixture(seg, trajs, lw, traj_id=tid)
    wm, wv = _np_mixture(model, seg, trajs, tid, lw)
    ok = ~np.isnan(wm)
    assert np.array_equal(np.isnan(mean), ~ok)
    em = float(np.max(np.abs(mean[ok] - wm[ok]) / np.maximum(np.abs(wm[ok]), 1.0)))
    gap = ok & (var > 0)        # (valid frames: variance exactly 0, checked below; NumPy leaves rounding there)
    ev = float(np.max(np.abs(var[gap] - wv[gap]) / wv[gap]))
    print(f"\nmixture: mean {em:.2g}, var {ev:.2g}")
    assert em < 1e-12 and ev < 1e-12
    # at valid frames: the data bit for bit, variance 0
    for j, x in enumerate(trajs):
        valid = ~np.isnan(x)
        assert np.array_equal(mean[j, :len(x)][valid], x[valid]) and np.all(var[j, :len(x)][valid] == 0)
    # chunking does not change a bit; -inf weights are skipped
    big = np.repeat(seg[0], 4, axis=0), np.repeat(seg[1], 4, axis=0)
    lwb = np.repeat(lw, 4) + rng.normal(size=4 * len(lw))
    ma, va = model.kalman_mixture(big, trajs, lwb, traj_id=np.repeat(tid, 4))
    mb, vb = model.kalman_mixture(big, trajs, lwb, traj_id=np.repeat(tid, 4), scratch_bytes=1 << 16)
    assert _bits_equal(ma, mb) and _bits_equal(va, vb)
    one = np.full(len(lw), -np.inf)
    one[5] = 0.0
    m1, v1 = model.kalman_mixture(seg, trajs, one, traj_id=tid)
    r1 = model.kalman((seg[0][5:6], seg[1][5:6]), [trajs[0]])
    assert _bits_equal(m1[0], r1.smooth_mean[0]) and _bits_equal(v1[0], r1.smooth_var[0])
    assert np.all(np.isnan(m1[1]))


def test_posterior_distances_of_sample_many(built_lib):
    import bild_amd
    model = calibration_model()
    rng = np.random.default_rng(9)
    prof = [np.repeat([0, 1, 0], [20, 25, 15]), np.repeat([1, 0], [30, 40])]
    trajs = []
    for x in model.trajectories_from_loopingprofiles(prof, seed=9):
        x = x[:].copy()
        x[rng.random(len(x)) < 0.1, 1] = np.nan        # gaps in the ss_order-1 dimension: every logL stays finite
        trajs.append(bild_amd.Trajectory(x))
    results = bild_amd.sample_many(trajs, model, k_max=3, init_runs=2, rng=np.random.default_rng(2))
    many = bild_amd.posterior_distances(results)
    for r, (m, v) in zip(results, many):
        m1, v1 = r.posterior_distance()
        assert _bits_equal(m, m1) and _bits_equal(v, v1)
        x = r.traj[:]
        valid = ~np.isnan(x)
        assert np.array_equal(m[valid], x[valid]) and np.all(v[valid] == 0)
    ma, va = results[0].posterior_distance(dE='average')
    assert ma.shape == (len(results[0].traj), model.d) and np.all(va[~np.isnan(va)] >= 0)
    avg = bild_amd.posterior_distances(results, dE='average')
    assert _bits_equal(avg[0][0], ma) and _bits_equal(avg[0][1], va)
