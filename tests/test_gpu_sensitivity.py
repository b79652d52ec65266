"""
MultiStateRouse.logL_sensitivities and MultiStateRouse.fit on the GPU (csrc/sens.hip), against the NumPy tangent filter
(tests/sensitivity_oracle.py), the device's own likelihood, the reference goldens, finite differences and the statistics
of the score.  `-s` prints the worst deviations observed.
"""
import numpy as np
import pytest

import goldens
import helpers as H
import sensitivity_oracle as SO

pytestmark = pytest.mark.gpu

REL = 1e-8


def _rel(got, want):
    scale = max(1.0, float(np.max(np.abs(want)))) if np.size(want) else 1.0
    return float(np.max(np.abs(np.asarray(got) - np.asarray(want)), initial=0.0)) / scale


def _golden_derivs(g):
    """ three parameters the arrays of any golden admit: a scale of (Sig, C0), of the variances s2, of (G, M0) """
    a = g['arrays']
    z = {k: np.zeros((3,) + a[k[1:]].shape) for k in SO.KEYS}
    z['dSig'][0], z['dC0'][0] = a['Sig'], a['C0']
    z['dG'][2], z['dM0'][2] = a['G'], a['M0']
    ds2 = np.zeros((3, 1, a['G'].shape[2]))
    ds2[1, 0] = np.asarray(g['localization_error'], dtype=np.float64) ** 2
    return z, ds2


@pytest.mark.parametrize('name', goldens.names())
def test_goldens(built_lib, name):
    import bild_amd
    from bild_amd import _lib
    g = goldens.load(name)
    model = bild_amd.MultiStateRouse.from_arrays(**g['arrays'], measurement=g['w'], localization_error=g['localization_error'])
    states = np.asarray(g['states'])
    derivs, ds2 = _golden_derivs(g)
    if model.handle().query(_lib.Q_NEFF) > 16:   # 17..32 modes: logL only
        with pytest.raises(_lib.BildAmdError, match='17 to 32'):
            model.logL_sensitivities(states, g['x'], derivatives={**derivs, 'ds2': ds2}, log=False)
        derivs, ds2 = {}, None
    ll, grad, F = model.logL_sensitivities(states, g['x'], log=False,
                                           derivatives={**derivs, 'ds2': ds2} if ds2 is not None else {})
    assert _rel(ll, g['logL_ref_numpy']) < REL
    assert _rel(ll, model.logL_batch(states, g["x"])) < REL
    err = np.broadcast_to(np.asarray(g['localization_error'], dtype=np.float64), (1, g['x'].shape[1]))
    oll, og, oF = SO.batch(g['arrays'], g['w'], err, [g['x']], list(states), derivs=derivs or None,
                           ds2=None if ds2 is None else ds2)
    assert _rel(ll, oll) < REL
    if derivs:
        assert _rel(grad, og) < REL and _rel(F, oF) < REL
        print(f"\n{name}: logL {_rel(ll, oll):.2g}, grad {_rel(grad, og):.2g}, fisher {_rel(F, oF):.2g}")


def _rouse_case(rng, N=8, S=3, d=3, T=120, n_traj=3, missing=True):
    import bild_amd
    loops = [None, (0, -1), (1, -2)][:S]
    model = bild_amd.MultiStateRouse(N, 1.3, 2.0, d=d, looppositions=loops, localization_error=0.3)
    trajs, profiles = [], []
    for j in range(n_traj):
        st = H.random_profile(rng, T, S, 25)
        x = model.trajectory_from_loopingprofile(st, rng=rng)[:].copy()
        if missing:
            x[rng.random(T) < 0.15] = np.nan
            if j == 0:
                x[0] = np.nan
        trajs.append(x)
        profiles.append(np.asarray(st[:]))
    return model, trajs, profiles


def test_generated_against_oracle(built_lib):
    from bild_amd.profiles import segments_from_states
    rng = np.random.default_rng(7)
    model, trajs, profiles = _rouse_case(rng)
    # candidates: the true profiles, constant ones, and adjacent switches
    cands, tids = [], []
    for j, st in enumerate(profiles):
        T = len(st)
        adj = np.zeros(T, dtype=int)
        adj[3], adj[4], adj[5:] = 1, 2, 1
        for c in (st, np.zeros(T, dtype=int), np.full(T, 2), adj):
            cands.append(c)
            tids.append(j)
    seg_start, seg_state = segments_from_states(np.stack(cands).astype(np.int32))
    ll, g, F = model.logL_sensitivities((seg_start, seg_state), trajs, traj_id=np.array(tids), log=False)
    arrays = model.arrays()
    D_k = SO.rouse_family(8, [None, (0, -1), (1, -2)], d=3)[1](1.3, 2.0)
    derivs = {k: np.concatenate([v, np.zeros((1,) + v.shape[1:])]) for k, v in D_k.items()}
    ds2 = np.zeros((3, len(trajs), 3))
    ds2[2] = 2 * 0.3
    errs = np.full((len(trajs), 3), 0.3)
    oll, og, oF = SO.batch(arrays, model.measurement, errs, trajs, cands, traj_id=tids, derivs=derivs, ds2=ds2)
    print(f"\ngenerated: logL {_rel(ll, oll):.2g}, grad {_rel(g, og):.2g}, fisher {_rel(F, oF):.2g}")
    assert _rel(ll, oll) < REL and _rel(g, og) < REL and _rel(F, oF) < REL
    assert _rel(ll, model.logL_segments(seg_start, seg_state, trajs, np.array(tids, dtype=np.int32))) < REL
    # log parameters: times theta
    _, gl, Fl = model.logL_sensitivities((seg_start, seg_state), trajs, traj_id=np.array(tids), log=True)
    th = np.array([1.3, 2.0, 0.3])
    assert np.allclose(gl, g * th, rtol=1e-14, atol=0) and np.allclose(Fl, F * np.outer(th, th), rtol=1e-14, atol=0)


def test_gradient_against_device_differences(built_lib):
    import bild_amd
    rng = np.random.default_rng(2)
    model = bild_amd.MultiStateRouse(20, 1.0, 5.0, d=3, localization_error=0.1)
    st = H.random_profile(rng, 300, 2, 60)
    traj = model.trajectory_from_loopingprofile(st, rng=rng)
    prof = np.asarray(st[:])[None, :]
    ll, g, _ = model.logL_sensitivities(prof, traj, log=False, fisher=False)
    worst = 0.0
    for p, name in enumerate(('D', 'k', 'localization_error')):
        x = {'D': 1.0, 'k': 5.0, 'localization_error': 0.1}[name]
        h = 1e-5 * x
        lp = model.with_parameters(**{name: x + h}).logL_batch(prof, traj)[0]
        lm = model.with_parameters(**{name: x - h}).logL_batch(prof, traj)[0]
        fd = (lp - lm) / (2 * h)
        worst = max(worst, abs(g[0, p] - fd) / max(1.0, abs(fd)))
        assert abs(g[0, p] - fd) <= 1e-6 * max(1.0, abs(fd)), (name, g[0, p], fd)
    print(f"\ndevice differences: worst relative {worst:.2g}")


def test_bit_identity(built_lib):
    import bild_amd
    from bild_amd import _lib
    from bild_amd.profiles import segments_from_states
    rng = np.random.default_rng(4)
    model = bild_amd.MultiStateRouse(20, 1.0, 5.0, d=3, localization_error=0.1)
    trajs = [model.trajectory_from_loopingprofile(H.random_profile(rng, T, 2, 40), rng=rng)[:] for T in (150, 90, 200)]
    cands = [H.random_profile(rng, 150, 2, 30) for _ in range(40)]
    ss, st = segments_from_states(np.stack([np.asarray(c[:]) for c in cands]).astype(np.int32))
    tid = np.zeros(len(cands), dtype=np.int32)
    ref = model.logL_sensitivities((ss, st), trajs, traj_id=tid)
    again = model.logL_sensitivities((ss, st), trajs, traj_id=tid)
    perm = rng.permutation(len(cands))
    shuffled = model.logL_sensitivities((ss[perm], st[perm]), trajs, traj_id=tid)
    chunked = model.logL_sensitivities((ss, st), trajs, traj_id=tid, scratch_bytes=1)
    alone = model.logL_sensitivities((ss[5:6], st[5:6]), trajs[0])
    other_set = model.logL_sensitivities((ss[:7], st[:7]), [trajs[2], trajs[0]], traj_id=np.ones(7, dtype=np.int32))
    for a, b in zip(ref, again):
        assert np.array_equal(a, b)
    for a, b in zip(ref, shuffled):
        assert np.array_equal(a[perm], b)
    for a, b in zip(ref, chunked):
        assert np.array_equal(a, b)
    for a, b in zip(ref, alone):
        assert np.array_equal(a[5:6], b)
    for a, b in zip(ref, other_set):
        assert np.array_equal(a[:7], b)
    assert _lib.prefix_info(model.trajset(trajs)) == (0, 0.0)


def test_refusals(built_lib):
    import bild_amd
    from bild_amd import _lib
    rng = np.random.default_rng(9)
    model = bild_amd.MultiStateRouse(10, 1.0, 5.0, d=3, localization_error=0.1)
    traj = np.asarray(model.trajectory_from_loopingprofile(np.zeros(50, dtype=int), rng=rng)[:])
    prof = np.zeros((1, 50), dtype=int)
    a = model.arrays()
    S, N = a['B'].shape[:2]
    V = model.handle().export(_lib.X_V)   # the reduced subspace
    X = rng.standard_normal((N, N))
    inside = V @ (X[:V.shape[1], :V.shape[1]] + X[:V.shape[1], :V.shape[1]].T) @ V.T   # not diagonal in Q_s
    outside = X + X.T
    for key, arr, msg in (('dB', inside, 'not diagonal'), ('dSig', inside, 'not diagonal'), ('dB', outside, 'reduced subspace'),
                          ('dC0', outside, 'reduced subspace')):
        d = np.zeros((1, S, N, N))
        d[0, 1] = arr
        with pytest.raises(_lib.BildAmdError, match=msg):
            model.logL_sensitivities(prof, traj, derivatives={key: d}, log=False)
    dM0 = np.zeros((1, S, N, 3))
    dM0[0, 0, :, 0] = np.ones(N)      # the uniform vector: outside the end-to-end subspace
    with pytest.raises(_lib.BildAmdError, match='reduced subspace'):
        model.logL_sensitivities(prof, traj, derivatives={'dM0': dM0}, log=False)
    with pytest.raises(_lib.BildAmdError, match='at most 4'):
        model.logL_sensitivities(prof, traj, derivatives={'dB': np.zeros((5, S, N, N))}, log=False)
    ds2 = np.zeros((1, 1, 3))
    ds2[0, 0] = [0.1, 0.1, 0.2]     # one chain (equal localization errors), different derivatives
    with pytest.raises(_lib.BildAmdError, match='share'):
        model.logL_sensitivities(prof, traj, derivatives={'ds2': ds2}, log=False)
    big = bild_amd.MultiStateRouse(80, 1.0, 5.0, d=3, localization_error=0.1)   # 40 effective modes
    with pytest.raises(_lib.BildAmdError, match='32 effective modes'):
        big.logL_sensitivities(np.zeros((1, 20), dtype=int), np.zeros((20, 3)), params=('D',))
    mid = bild_amd.MultiStateRouse(40, 1.0, 5.0, d=3, localization_error=0.1)   # 20 effective modes
    with pytest.raises(_lib.BildAmdError, match='17 to 32'):
        mid.logL_sensitivities(np.zeros((1, 20), dtype=int), np.zeros((20, 3)), params=('D',))
    # P = 0 there is the log-likelihood alone
    ll, g, F = mid.logL_sensitivities(np.zeros((1, 20), dtype=int), np.ones((20, 3)), params=())
    assert g.shape == (1, 0) and abs(ll[0] - mid.logL_batch(np.zeros((1, 20), dtype=int), np.ones((20, 3)))[0]) < 1e-9


def test_score_statistics(built_lib):
    """
    At the true parameters the score has mean 0 and covariance equal to the Fisher information (information equality).
    Bars: the mean score within 4 standard errors (sample sd / sqrt(n)) per component; each entry of the sample covariance
    of the scores within 5 standard errors of the mean Fisher matrix, the standard error of an entry estimated from the
    sample of products g_a g_b (sd / sqrt(n)), plus that of the mean Fisher entry itself.
    """
    import bild_amd
    rng = np.random.default_rng(12)
    n, T = 2000, 100
    model = bild_amd.MultiStateRouse(10, 1.0, 5.0, d=3, localization_error=0.2)
    profiles = [H.random_profile(rng, T, 2, 30) for _ in range(n)]
    trajs = model.trajectories_from_loopingprofiles(profiles, seed=2024)
    from bild_amd.models import _fit_profiles
    seg = _fit_profiles(profiles, [T] * n, 2)
    _, g, F = model.logL_sensitivities(seg, trajs, traj_id=np.arange(n, dtype=np.int32))
    mean, se = g.mean(axis=0), g.std(axis=0, ddof=1) / np.sqrt(n)
    print(f"\nscore mean / se: {mean / se}")
    assert np.all(np.abs(mean) < 4 * se)
    cov = np.cov(g.T)
    Fm = F.mean(axis=0)
    prod = g[:, :, None] * g[:, None, :]
    bar = 5 * (prod.std(axis=0, ddof=1) / np.sqrt(n) + F.std(axis=0, ddof=1) / np.sqrt(n))
    print(f"cov - Fisher over bar:\n{(cov - Fm) / bar}")
    assert np.all(np.abs(cov - Fm) < bar)


@pytest.mark.parametrize('kind', ['switching', 'constant'])
def test_fit_recovers_truth(built_lib, kind):
    import bild_amd
    rng = np.random.default_rng(21 if kind == 'switching' else 22)
    n, T = 128, 400
    truth = bild_amd.MultiStateRouse(20, 1.0, 5.0, d=3, localization_error=0.1)
    if kind == 'switching':
        profiles = [H.random_profile(rng, T, 2, 50) for _ in range(n)]
    else:
        profiles = [np.zeros(T, dtype=int) for _ in range(n)]
    trajs = truth.trajectories_from_loopingprofiles(profiles, seed=77 if kind == 'switching' else 78)
    start = {'D': 2.0, 'k': 10.0, 'localization_error': 0.2}
    res = truth.fit(trajs, profiles if kind == 'switching' else 0, start=start, tol=1e-8, max_iter=50)
    print(f"\n{kind}: {res}")
    assert res.converged and res.n_iter <= 50
    for name, x in (('D', 1.0), ('k', 5.0), ('localization_error', 0.1)):
        assert abs(res.params[name] - x) < 4 * res.se[name], (name, res.params[name], res.se[name])
    from bild_amd.models import _fit_profiles
    seg = _fit_profiles(profiles if kind == 'switching' else 0, [T] * n, 2)
    tid = np.arange(n, dtype=np.int32)
    l_truth = truth.logL_sensitivities(seg, trajs, traj_id=tid, fisher=False)[0].sum()
    assert res.logL >= l_truth
    _, g, F = res.model.logL_sensitivities(seg, trajs, traj_id=tid)
    from bild_amd.models import _newton_decrement
    assert _newton_decrement(g.sum(axis=0), F.sum(axis=0)) < 1e-8
    assert np.all(np.diff([h[1] for h in res.history]) > 0)
