"""
GenericGaussianModel.logL_sensitivities and GenericGaussianModel.fit on the GPU (csrc/gauss_sens.hip), against the NumPy
tangent oracle (tests/gauss_sensitivity_oracle.py), the device's own likelihood, the reference goldens, the statistics
of the score and parameter recovery.  `-s` prints the worst deviations observed.
"""
import glob
import os

import numpy as np
import pytest

import gauss_sensitivity_oracle as GS
from gauss_sim_cases import make_model, msd_exp, msd_pow, profile

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDENS = sorted(glob.glob(os.path.join(HERE, 'golden', 'gauss', '*.npz')))


def _rel(got, want):
    want = np.asarray(want)
    scale = max(1.0, float(np.max(np.abs(want)))) if want.size else 1.0
    return float(np.max(np.abs(np.asarray(got) - want), initial=0.0)) / scale


def _bits_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


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


def random_derivs(rng, model, P):
    """ P parameters: a random scale of every (state, dimension)'s MSD and msd(inf), and a random shift of the means """
    S, d, L = model.msd.shape
    c = rng.uniform(-1, 1, size=(P, S, d))
    return dict(dmsd=c[..., None] * model.msd[None], dmsd_inf=c * model.msd_inf[None], dmean=rng.uniform(-1, 1, size=(P, S, d)))


def segments(states_list):
    from bild_amd.models import _ragged_segments
    return _ragged_segments([np.asarray(s) for s in states_list], np.array([len(s) for s in states_list]))


@pytest.mark.parametrize('path', GOLDENS, ids=os.path.basename)
def test_goldens(built_lib, path):
    g = load(path)
    model = model_from(g['msd'], g['msd_inf'], g['mean'], g['order'])
    S, d, L = g['msd'].shape
    dm = dict(dmsd=np.zeros((S + 1, S, d, L)), dmsd_inf=np.zeros((S + 1, S, d)), dmean=np.zeros((S + 1, S, d)))
    for s in range(S):
        dm['dmsd'][s, s], dm['dmsd_inf'][s, s] = g['msd'][s], g['msd_inf'][s]
    dm['dmean'][S] = 1.0
    states = g['profiles'][:16]
    ll, grad, F = model.logL_sensitivities(states, g['x'], **dm)
    oll, og, oF = GS.batch(*arrays(model), [g['x']], list(states), **dm)
    ok = np.isfinite(g['logL'][:16])
    assert np.array_equal(np.isnan(ll), ~ok)
    assert _rel(ll[ok], g['logL'][:16][ok]) < 1e-10
    assert _rel(ll[ok], oll[ok]) < 1e-10
    assert _rel(ll[ok], model.logL_batch(states, g['x'])[ok]) < 1e-10
    assert _rel(grad[ok], og[ok]) < 1e-8 and _rel(F[ok], oF[ok]) < 1e-8
    print(f"\n{os.path.basename(path)}: logL {_rel(ll[ok], oll[ok]):.2g}, grad {_rel(grad[ok], og[ok]):.2g}, "
          f"fisher {_rel(F[ok], oF[ok]):.2g}")


def _case(seed, S, d, T, p_missing, n_traj=2, n_cand=10):
    rng = np.random.default_rng(seed)
    model = make_model(S, d, seed, L=max(T, 64))
    truth = [profile(rng, T, S, 3) for _ in range(n_traj)]
    trajs = [t[:] for t in model.trajectories_from_loopingprofiles(truth, missing_frames=p_missing or None, seed=seed)]
    cands = [profile(rng, T, S, int(rng.integers(0, 6))) for _ in range(n_cand)]
    tid = rng.integers(0, n_traj, size=n_cand).astype(np.int32)
    return rng, model, trajs, cands, tid


CASES = [(2, 1, 0.0, 1), (2, 2, 0.1, 0), (3, 3, 0.1, 4), (3, 2, 0.0, 2), (2, 3, 0.1, 3), (3, 1, 0.1, 4)]


@pytest.mark.parametrize('S,d,p_missing,P', CASES)
def test_against_the_oracle(built_lib, S, d, p_missing, P):
    rng, model, trajs, cands, tid = _case(10 * S + d + P, S, d, 90, p_missing)
    dm = random_derivs(rng, model, P)
    seg = segments(cands)
    ll, grad, F = model.logL_sensitivities(seg, trajs, traj_id=tid, **dm)
    oll, og, oF = GS.batch(*arrays(model), trajs, cands, traj_id=tid, **dm)
    assert grad.shape == (len(cands), P) and F.shape == (len(cands), P, P)
    assert _rel(ll, oll) < 1e-10
    assert _rel(ll, model.logL_segments(*seg, trajs, traj_id=tid)) < 1e-10
    assert _rel(grad, og) < 1e-8 and _rel(F, oF) < 1e-8
    print(f"\nS={S} d={d} missing={p_missing} P={P}: logL {_rel(ll, oll):.2g}, grad {_rel(grad, og):.2g}, fisher {_rel(F, oF):.2g}")


def test_longest_trajectory(built_lib):
    rng = np.random.default_rng(5)
    model = make_model(2, 1, 1, L=2048)
    st = profile(rng, 2048, 2, 1)
    x = model.trajectories_from_loopingprofiles([st], seed=3)[0][:]
    dm = random_derivs(rng, model, 1)
    ll, grad, F = model.logL_sensitivities(st[None], x, **dm)
    oll, og, oF = GS.batch(*arrays(model), [x], [st], **dm)
    assert _rel(ll, oll) < 1e-10 and _rel(ll, model.logL_batch(st[None], x)) < 1e-10
    assert _rel(grad, og) < 1e-8 and _rel(F, oF) < 1e-8


@pytest.mark.parametrize('p_missing', [0.0, 0.1])
def test_bit_identity(built_lib, p_missing):
    rng, model, trajs, cands, tid = _case(77, 3, 2, 150, p_missing, n_traj=3, n_cand=24)
    dm = random_derivs(rng, model, 3)
    seg = segments(cands)
    ll, grad, F = model.logL_sensitivities(seg, trajs, traj_id=tid, **dm)
    # another order, duplicates, a subset
    idx = np.concatenate([np.arange(len(cands))[::-1], [3, 3, 5]])
    l2, g2, F2 = model.logL_sensitivities((seg[0][idx], seg[1][idx]), trajs, traj_id=tid[idx], **dm)
    assert _bits_equal(l2, ll[idx]) and _bits_equal(g2, grad[idx]) and _bits_equal(F2, F[idx])
    one = model.logL_sensitivities((seg[0][7:8], seg[1][7:8]), trajs, traj_id=tid[7:8], **dm)
    assert _bits_equal(one[0], ll[7:8]) and _bits_equal(one[1], grad[7:8]) and _bits_equal(one[2], F[7:8])
    # small chunks of the factorisations
    l3, g3, F3 = model.logL_sensitivities(seg, trajs, traj_id=tid, scratch_bytes=1 << 16, **dm)
    assert _bits_equal(l3, ll) and _bits_equal(g3, grad) and _bits_equal(F3, F)
    # fisher=False, and logL whatever P
    l4, g4, F4 = model.logL_sensitivities(seg, trajs, traj_id=tid, fisher=False, **dm)
    assert F4 is None and _bits_equal(l4, ll) and _bits_equal(g4, grad)
    for P in (0, 1, 4):
        dP = random_derivs(np.random.default_rng(P), model, P)
        lP = model.logL_sensitivities(seg, trajs, traj_id=tid, **dP)[0]
        assert _bits_equal(lP, ll), P


def test_nan_candidate_leaves_its_neighbours_alone(built_lib):
    import bild_amd
    L = 80
    model = bild_amd.GenericGaussianModel([[(msd_exp(1.0, 5.0, 0.3, L), 0.1, 0)], [(msd_exp(2.0, 9.0, 0.3, L), -0.1, 0)]])
    rng = np.random.default_rng(2)
    x = model.trajectories_from_loopingprofiles([np.zeros(60, dtype=int)], seed=1)[0][:]
    x[19:31] = np.nan
    bad = np.zeros(60, dtype=int)
    bad[21:30] = 1                  # a later interval whose window [20, 30) has no valid frame
    good = [profile(rng, 60, 2, 2) for _ in range(12)]
    good = [g for g in good if np.isfinite(GS.sensitivities(*arrays(model), x, g)[0])][:4]
    assert len(good) >= 2
    states = np.stack(good[:1] + [bad] + good[1:])
    dm = random_derivs(rng, model, 2)
    ll, grad, F = model.logL_sensitivities(states, x, **dm)
    assert np.isnan(ll[1]) and np.all(np.isnan(grad[1])) and np.all(np.isnan(F[1]))
    assert np.all(np.isfinite(np.delete(ll, 1)))
    assert np.isnan(model.logL_batch(bad[None], x)[0])
    rest = np.delete(np.arange(len(states)), 1)
    l2, g2, F2 = model.logL_sensitivities(states[rest], x, **dm)
    assert _bits_equal(l2, ll[rest]) and _bits_equal(g2, grad[rest]) and _bits_equal(F2, F[rest])


def test_refusals(built_lib):
    import bild_amd
    from bild_amd import _lib
    L = 2100
    model = bild_amd.GenericGaussianModel([[(msd_pow(0.5, 1.0, 0.3, L), 0.0, 1)], [(msd_pow(1.0, 1.0, 0.3, L), 0.0, 1)]])
    h = model.handle()
    seg = (np.zeros((1, 1), dtype=np.int32), np.zeros((1, 1), dtype=np.int32))
    x = np.zeros((40, 1))
    with pytest.raises(_lib.BildAmdError, match='at most 2048'):
        _lib.gauss_logl_sensitivities(h, [np.zeros((2049, 1))], *seg)
    with pytest.raises(_lib.BildAmdError, match='at most 4'):
        _lib.gauss_logl_sensitivities(h, [x], *seg, dmean=np.zeros((5, 2, 1)), P=5)
    with pytest.raises(_lib.BildAmdError, match='not finite'):
        _lib.gauss_logl_sensitivities(h, [x], *seg, dmsd=np.full((1, 2, 1, L), np.nan), P=1)
    with pytest.raises(_lib.BildAmdError, match='first segment'):
        _lib.gauss_logl_sensitivities(h, [x], np.ones((1, 1), dtype=np.int32), seg[1])
    with pytest.raises(ValueError, match='at most'):
        model.logL_sensitivities(np.zeros((1, 2049), dtype=np.int64), np.zeros((2049, 1)))


def test_score_calibration(built_lib):
    """ at the true parameters the score has mean 0 and covariance equal to the mean Fisher information """
    rng = np.random.default_rng(11)
    model = make_model(2, 2, 4, L=64)
    n, T = 2000, 40
    truth = [profile(rng, T, 2, int(rng.integers(0, 3))) for _ in range(n)]
    trajs = [t[:] for t in model.trajectories_from_loopingprofiles(truth, seed=99)]
    S, d, L = model.msd.shape
    dm = dict(dmsd=np.zeros((2, S, d, L)), dmsd_inf=np.zeros((2, S, d)), dmean=np.zeros((2, S, d)))
    dm['dmsd'][0, 0], dm['dmsd_inf'][0, 0] = model.msd[0], model.msd_inf[0]
    dm['dmean'][1] = 1.0
    seg = segments(truth)
    ll, grad, F = model.logL_sensitivities(seg, trajs, traj_id=np.arange(n, dtype=np.int32), **dm)
    mean_score = grad.mean(axis=0)
    se = grad.std(axis=0) / np.sqrt(n)
    assert np.all(np.abs(mean_score) < 4 * se), (mean_score, se)
    cov = np.cov(grad.T)
    Fm = F.mean(axis=0)
    rel = np.abs(cov - Fm) / np.sqrt(np.outer(np.diag(Fm), np.diag(Fm)))
    print(f"\nscore mean {mean_score} (se {se}); cov {cov.ravel()} vs Fisher {Fm.ravel()}")
    assert np.all(rel < 0.15), rel


def _fit_family(L):
    def family(A, G):
        return [[(msd_exp(A, 10.0, 0.3, L), 0.1, 0), (msd_pow(G, 0.8, 0.3, L), 0.05, 1)],
                [(msd_exp(2 * A, 4.0, 0.3, L), -0.1, 0), (msd_pow(0.5 * G, 1.2, 0.3, L), 0.0, 1)]]

    def derivatives(A, G):
        t = np.arange(L, dtype=np.float64)
        dmsd = np.zeros((2, 2, 2, L))
        dinf = np.zeros((2, 2, 2))
        dmsd[0, 0, 0] = 2 * (1 - np.exp(-t / 10.0))
        dmsd[0, 1, 0] = 4 * (1 - np.exp(-t / 4.0))
        dinf[0, 0, 0], dinf[0, 1, 0] = 2.0, 4.0
        dmsd[1, 0, 1] = t ** 0.8
        dmsd[1, 1, 1] = 0.5 * t ** 1.2
        dmsd[..., 0] = 0.0
        return dmsd, dinf, None

    return family, derivatives


@pytest.mark.parametrize('switching', [False, True])
def test_fit_recovers_the_truth(built_lib, switching):
    import bild_amd
    L, T, n = 1000, 1000, 256
    family, derivatives = _fit_family(L)
    truth = {'A': 1.2, 'G': 0.6}
    model = bild_amd.GenericGaussianModel(family(**truth))
    rng = np.random.default_rng(21 + switching)
    profiles = [profile(rng, T, 2, 3 if switching else 0) for _ in range(n)]
    trajs = model.trajectories_from_loopingprofiles(profiles, seed=5 + switching)
    start = {k: 2 * v for k, v in truth.items()}
    fd = bild_amd.GenericGaussianModel.fit(trajs, profiles, family, start)
    an = bild_amd.GenericGaussianModel.fit(trajs, profiles, family, start, derivatives=derivatives)
    print(f"\n{fd}\n{an}")
    for res in (fd, an):
        assert res.converged
        for k, v in truth.items():
            assert abs(res.params[k] - v) < 4 * res.se[k], (k, res.params[k], res.se[k])
    for k in truth:
        assert abs(fd.params[k] - an.params[k]) <= 1e-5 * abs(an.params[k])
