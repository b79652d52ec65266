"""
MultiStateRouse.kalman and the posterior distance tracks on the GPU (csrc/kalman.hip), against the NumPy oracle
(tests/kalman_oracle.py: dense filter, classical RTS smoother) and the reference's log-likelihoods.  `-s` prints the
worst deviations observed.
"""
import numpy as np
import pytest
from scipy import stats

import goldens
import helpers as H
import kalman_oracle as KO

pytestmark = pytest.mark.gpu

ALL = ('terms', 'pred', 'filt', 'smooth', 'innov')


def _synth(model, states, err, rng):
    return np.array(H.synth_trajectory(model, states, err, rng)[:])


def _result_dict(res):
    return {k: getattr(res, k) for k in KO.OUTPUTS}


def _compare(got, want, x, var_scale, var_rel=1e-9, terms_rel=False, label=''):
    """
    the bars of the goldens: means 1e-9 max|x|, variances var_rel * var_scale, terms 1e-10 per frame (terms_rel: times the
    largest |term|, for data whose innovations are many standard deviations)
    """
    xs = max(1.0, float(np.nanmax(np.abs(x)))) if np.any(np.isfinite(x)) else 1.0
    worst = {}
    for k in KO.OUTPUTS:
        g, w = got[k], want[k]
        assert np.array_equal(np.isnan(g), np.isnan(w)), (label, k)
        ok = ~np.isnan(w)
        dev = float(np.max(np.abs(g[ok] - w[ok]), initial=0.0))
        if k == 'terms':
            bar = 1e-10 * (max(1.0, float(np.max(np.abs(w[ok]), initial=0.0))) if terms_rel else 1.0)
        elif k.endswith('mean'):
            bar = 1e-9 * xs
        elif k == 'innov':
            bar = 1e-8
        else:
            bar = var_rel * var_scale
        worst[k] = dev / bar
        assert dev <= bar, (label, k, dev, bar)
    return worst


def _var_scale(model):
    a = model.arrays()
    w = model.measurement
    err = np.asarray(model.localization_error if model.localization_error is not None else 0.0)
    return max(float(w @ C0 @ w) for C0 in a['C0']) + float(np.max(err) ** 2)


@pytest.mark.parametrize('name', goldens.names())
def test_goldens(built_lib, name):
    import bild_amd
    g = goldens.load(name)
    model = bild_amd.MultiStateRouse.from_arrays(**g['arrays'], measurement=g['w'], localization_error=g['localization_error'])
    res = model.kalman(g['states'], g['x'], outputs=ALL)
    assert np.max(np.abs(res.terms.sum(axis=(1, 2)) - g['logL_ref_numpy'])) < 1e-8
    want = KO.batch(g['arrays'], g['w'], g['localization_error'], [g['x']], list(g['states']))
    worst = _compare(_result_dict(res), want, g['x'], _var_scale(model), label=name)
    print(f"\n{name}: worst deviation / bar: " + ', '.join(f"{k} {v:.2g}" for k, v in worst.items()))


ADVERSARIAL = {
    'sigma_1e-3': dict(err=1e-3),
    'long_gaps': dict(gaps=True),
    'stiff_chain': dict(k=50.0),
    'soft_chain': dict(k=0.05),
    'N32': dict(N=32),
    'N64': dict(N=64),
}


@pytest.mark.parametrize('case', sorted(ADVERSARIAL))
def test_data_the_model_did_not_produce(built_lib, case):
    import bild_amd
    c = ADVERSARIAL[case]
    rng = np.random.default_rng(sorted(ADVERSARIAL).index(case) + 70)
    T, n = 300, 6
    err = c.get('err', 0.1)
    model = bild_amd.MultiStateRouse(c.get('N', 20), 1.0, c.get('k', 5.0), d=3, localization_error=err)
    truth = H.random_profile(rng, T, 2, 60)
    x = _synth(model, truth, err, rng)
    x = x + rng.normal(scale=3.0, size=x.shape)        # not what the model produces
    if c.get('gaps'):
        x[40:110] = np.nan
        x[200:260] = np.nan
    states = np.array([H.random_profile(rng, T, 2, 50) for _ in range(n)])
    res = model.kalman(states, x, outputs=ALL)
    want = KO.batch(model.arrays(), model.measurement, model.localization_error, [x], list(states))
    worst = _compare(_result_dict(res), want, x, _var_scale(model), var_rel=1e-7, terms_rel=True, label=case)
    print(f"\n{case}: worst deviation / bar: " + ', '.join(f"{k} {v:.2g}" for k, v in worst.items()))


def test_calibration(built_lib):
    import bild_amd
    rng = np.random.default_rng(5)
    n, T, sigma = 2000, 200, 0.1
    model = bild_amd.MultiStateRouse(20, 1.0, 5.0, d=3, localization_error=sigma)
    profiles = [bild_amd.Loopingprofile(H.random_profile(rng, T, 2, 40)) for _ in range(n)]
    clean = model.trajectories_from_loopingprofiles(profiles, localization_error=0, seed=11)
    ys = [np.array(t[:]) for t in clean]
    xs = []
    for y in ys:
        x = y + rng.normal(scale=sigma, size=y.shape)
        x[rng.random(T) < 0.1] = np.nan
        xs.append(x)
    from bild_amd.profiles import segments_from_states
    seg_start, seg_state = segments_from_states(np.array([p[:] for p in profiles], dtype=np.int32))
    res = model.kalman((seg_start, seg_state), xs, traj_id=np.arange(n), outputs=('filt', 'smooth', 'innov'))
    k = rng.integers(3, size=n)
    t = rng.integers(T, size=n)
    y = np.array([ys[i][t[i], k[i]] for i in range(n)])
    r = np.arange(n)
    z_s = (y - res.smooth_mean[r, t, k]) / np.sqrt(res.smooth_var[r, t, k])
    z_f = (y - res.filt_mean[r, t, k]) / np.sqrt(res.filt_var[r, t, k])
    t_obs = np.array([rng.choice(np.flatnonzero(~np.isnan(xs[i][:, 0]))) for i in range(n)])
    z_i = res.innov[r, t_obs, k]
    for label, z in (('smoothed', z_s), ('filtered', z_f), ('innovations', z_i)):
        p = stats.kstest(z, 'norm').pvalue
        print(f"\ncalibration {label}: mean {z.mean():+.3f} sd {z.std():.3f} KS p = {p:.3g}")
        assert p > 1e-3, label
        assert abs(z.mean()) < 5 / np.sqrt(n), label


def test_structure(built_lib):
    import bild_amd
    rng = np.random.default_rng(8)
    T = 150
    model = bild_amd.MultiStateRouse(20, 1.0, 5.0, d=3, localization_error=0.1)
    truth = H.random_profile(rng, T, 2, 40)
    x = _synth(model, truth, 0.1, rng)
    x[120:] = np.nan
    res = model.kalman(truth[None, :], x, outputs=ALL)
    assert np.array_equal(res.smooth_mean[0, -1], res.filt_mean[0, -1])
    assert np.array_equal(res.smooth_var[0, -1], res.filt_var[0, -1])
    # missing to the end: from the last observed frame on, the smoother is the filter
    assert np.allclose(res.smooth_mean[0, 119:], res.filt_mean[0, 119:], rtol=1e-12, atol=1e-12)
    assert np.allclose(res.smooth_var[0, 119:], res.filt_var[0, 119:], rtol=1e-12, atol=1e-14)
    # almost no localization error: the smoothed mean of an observed frame is the data
    tiny = bild_amd.MultiStateRouse(20, 1.0, 5.0, d=3, localization_error=1e-6)
    xt = _synth(tiny, truth, 1e-6, rng)
    xt[50:60] = np.nan
    r2 = tiny.kalman(truth[None, :], xt, outputs=('smooth',))
    ok = ~np.isnan(xt)
    assert np.max(np.abs(r2.smooth_mean[0][ok] - xt[ok]) / np.max(np.abs(xt[ok]))) < 1e-5
    # T = 1 and an all-missing trajectory
    one = model.kalman(np.zeros((1, 1), dtype=int), x[:1], outputs=ALL)
    assert np.array_equal(one.smooth_mean, one.filt_mean)
    gone = model.kalman(truth[None, :20], np.full((20, 3), np.nan), outputs=ALL)
    assert np.all(gone.terms == 0.0)
    assert np.array_equal(gone.filt_mean, gone.pred_mean) and np.array_equal(gone.smooth_mean, gone.pred_mean)


def test_reproducibility(built_lib):
    import bild_amd
    from bild_amd import _lib
    rng = np.random.default_rng(9)
    model = bild_amd.MultiStateRouse(20, 1.0, 5.0, d=3, localization_error=[0.1, 0.1, 0.2])
    Ts = rng.integers(50, 250, size=50)
    trajs = [_synth(model, H.random_profile(rng, int(T), 2, 40), np.array([0.1, 0.1, 0.2]), rng) for T in Ts]
    for x in trajs[::7]:
        x[rng.random(len(x)) < 0.1] = np.nan
    n = 4096
    tid = rng.integers(50, size=n).astype(np.int32)
    K1 = 4
    seg_start = np.zeros((n, K1), dtype=np.int32)
    seg_state = rng.integers(2, size=(n, K1)).astype(np.int32)
    for r in range(n):
        seg_start[r, 1:] = np.sort(rng.integers(1, Ts[tid[r]], size=K1 - 1))
    full = model.kalman((seg_start, seg_state), trajs, traj_id=tid, outputs=ALL)
    perm = rng.permutation(n)
    shuf = model.kalman((seg_start[perm], seg_state[perm]), trajs, traj_id=tid[perm], outputs=ALL)
    small = model.kalman((seg_start, seg_state), trajs, traj_id=tid, outputs=ALL, scratch_bytes=3 << 20)
    again = model.kalman((seg_start, seg_state), trajs, traj_id=tid, outputs=ALL)
    for name in KO.OUTPUTS:
        a = getattr(full, name)
        assert np.array_equal(a[perm], getattr(shuf, name), equal_nan=True), name
        assert np.array_equal(a, getattr(small, name), equal_nan=True), name
        assert np.array_equal(a, getattr(again, name), equal_nan=True), name
    r = int(np.flatnonzero(tid == 3)[0])
    alone = model.kalman((seg_start[r:r + 1], seg_state[r:r + 1]), trajs[3], outputs=ALL)
    T3 = len(trajs[3])
    for name in KO.OUTPUTS:
        assert np.array_equal(getattr(full, name)[r, :T3], getattr(alone, name)[0], equal_nan=True), name
    # no likelihood table was built for either set
    assert _lib.prefix_info(model.trajset(trajs)) == (0, 0.0)
    assert _lib.prefix_info(model.trajset(trajs[3])) == (0, 0.0)


def _np_mixture(model, seg_start, seg_state, traj, lw):
    res = model.kalman((seg_start, seg_state), [traj], outputs=('smooth',))
    keep = np.exp(lw - lw.max()) > 0
    return KO.mixture(res.smooth_mean[keep, :, :], res.smooth_var[keep], lw[keep])


def test_mixture(built_lib):
    import bild_amd
    from bild_amd import _lib
    rng = np.random.default_rng(12)
    T = 120
    model = bild_amd.MultiStateRouse(20, 1.0, 5.0, d=3, localization_error=0.1)
    truth = H.random_profile(rng, T, 2, 30)
    x = _synth(model, truth, 0.1, rng)
    sampler = bild_amd.FixedkSampler(bild_amd.Trajectory(x, localization_error=0.1), model, k=2, N=100)
    for _ in range(3):
        sampler.step()
    mean, var = sampler.posterior_distance()
    seg_start, seg_state, lw = sampler._posterior_segments()
    wm, wv = _np_mixture(model, seg_start, seg_state, x, lw)
    assert np.max(np.abs(mean - wm) / np.maximum(np.abs(wm), 1.0)) < 1e-12
    assert np.max(np.abs(var - wv) / wv) < 1e-12
    # all weight on one candidate: its own track
    one = np.full(len(lw), -np.inf)
    one[5] = 0.0
    m1, v1 = model.kalman_mixture((seg_start, seg_state), [x], one)
    r1 = model.kalman((seg_start[5:6], seg_state[5:6]), [x])
    assert np.array_equal(m1[0], r1.smooth_mean[0]) and np.array_equal(v1[0], r1.smooth_var[0])
    # chunking does not change a bit
    big = np.repeat(seg_start, 8, axis=0), np.repeat(seg_state, 8, axis=0)
    lwb = np.repeat(lw, 8) + rng.normal(size=8 * len(lw))
    ma, va = model.kalman_mixture(big, [x], lwb)
    mb, vb = model.kalman_mixture(big, [x], lwb, scratch_bytes=1 << 20)
    assert np.array_equal(ma, mb) and np.array_equal(va, vb)
    # the device entry refuses what would be garbage
    ts = model.trajset(x)
    bad = lw.copy()
    bad[1] = np.nan
    with pytest.raises(_lib.BildAmdError):
        _lib.kalman_mixture(model.handle(), ts, seg_start, seg_state, bad)
    wrong = seg_start.copy()
    wrong[0, 0] = 1
    with pytest.raises(_lib.BildAmdError):
        _lib.kalman_segments(model.handle(), ts, wrong, seg_state)


def test_results_and_many(built_lib):
    import bild_amd
    rng = np.random.default_rng(13)
    model = bild_amd.MultiStateRouse(20, 1.0, 5.0, d=3, localization_error=0.1)
    trajs = [_synth(model, H.random_profile(rng, T, 2, 20), 0.1, rng) for T in (50, 70)]
    results = bild_amd.sample_many([bild_amd.Trajectory(t, localization_error=0.1) for t in trajs], model, k_max=3, init_runs=2, rng=np.random.default_rng(1))
    res = results[0]
    mean, var = res.posterior_distance(dE='average')
    parts = []
    for s, logev in zip(res.samplers, res.evidence):
        if s.evidences[-1][0] > -np.inf:
            a, b, lw = s._posterior_segments()
            r = model.kalman((a, b), [res.traj])
            keep = np.exp(lw - lw.max()) > 0
            parts.append((r.smooth_mean[keep], r.smooth_var[keep], lw[keep] - np.log(np.sum(np.exp(lw - lw.max()))) - lw.max() + logev))
    wm, wv = KO.mixture(np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]),
                        np.concatenate([p[2] for p in parts]))
    assert np.max(np.abs(mean - wm[0] if wm.ndim == 3 else mean - wm) / np.maximum(np.abs(wm), 1.0)) < 1e-10
    assert np.max(np.abs(var - wv) / wv) < 1e-10
    many = bild_amd.posterior_distances(results)
    for r, (m, v) in zip(results, many):
        m1, v1 = r.posterior_distance()
        assert np.array_equal(m, m1) and np.array_equal(v, v1)
