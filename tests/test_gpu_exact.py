"""
Exact evidence by enumeration on the GPU (bild_amd.exact, csrc/exact.hip), for MultiStateRouse and
GenericGaussianModel: parity with FixedkSampler's exhaustive path, k = 0, a million profiles against the NumPy oracle
(tests/exact_oracle.py) on the public likelihood, reproducibility, and the NaN and empty cases.
"""
import numpy as np
import pytest

import bild_amd
import exact_oracle as X
from bild_amd.amis import logsumexp

pytestmark = pytest.mark.gpu


def rouse_model(S):
    if S == 2:
        return bild_amd.MultiStateRouse(20, 1, 5, d=3, localization_error=0.1)
    model = bild_amd.MultiStateRouse(20, 1, 5, d=3, looppositions=(None, (0, -1), (0, 10)), localization_error=0.1)
    model.transitions[0, 2] = False
    return model


def rouse_traj(model, T, rng, missing=(), cuts=None):
    S = model.nStates
    cuts = sorted(rng.choice(np.arange(1, T), size=2, replace=False)) if cuts is None else cuts
    states = np.repeat([0, 1, S - 1], np.diff(np.r_[0, cuts, T]))
    return model.trajectory_from_loopingprofile(bild_amd.Loopingprofile(states), missing_frames=np.asarray(missing, dtype=int),
                                                rng=rng)


def gauss_model(rng, S, T, scale=1.0):
    # (tests/test_gpu_gauss.py: random_case, model_from)
    d = 2
    lags = np.arange(T, dtype=float)
    spec = []
    for n in range(S):
        row = []
        for k in range(d):
            G_, a, s2 = rng.uniform(0.3, 2), rng.uniform(0.4, 1.2), rng.uniform(0.05, 0.3)
            msd = np.where(lags > 0, G_ * lags ** a + 2 * s2, 0)
            order = int(rng.integers(0, 2))
            mean = scale * rng.normal(scale=0.3)
            row.append((msd if order == 1 else np.append(msd, 2 * G_ * T ** a + 4 + 2 * s2), mean, order))
        spec.append(row)
    model = bild_amd.GenericGaussianModel(spec)
    if S == 3:
        model.transitions[0, 2] = False
    return model


def gauss_traj(rng, T, missing=()):
    x = np.cumsum(rng.normal(size=(T, 2)), axis=0)
    x[np.asarray(missing, dtype=int)] = np.nan
    return x


def make(kind, S, T, seed, missing=()):
    rng = np.random.default_rng(seed)
    if kind == 'rouse':
        model = rouse_model(S)
        return model, rouse_traj(model, T, rng, missing)
    # (isolated missing frames: a later ss_order-0 window without a valid frame gives NaN, test_nan_candidates_gauss)
    return gauss_model(rng, S, T + 8), gauss_traj(rng, T, [t for t in missing if t - 1 not in missing])


def check_parity(model, traj, k):
    got = bild_amd.exact_evidence(traj, model, k)
    sampler = bild_amd.FixedkSampler(traj, model, k=k, max_fcomplete=10 ** 7, max_fev=10 ** 7)
    assert sampler.exhausted
    logev, _, KL = sampler.evidences[-1]
    assert got.n_profiles == len(sampler._arr['logLs']) and got.n_nan == 0
    assert abs(got.logev - logev) < 1e-10, (got.logev, logev)
    assert abs(got.KL - KL) < 1e-9, (got.KL, KL)
    assert np.array_equal(got.map_profile[:], sampler.MAP_profile()[:])
    assert got.map_logL == model.logL(got.map_profile, traj)
    want = sampler.log_marginal_posterior()
    fin = np.isfinite(want)
    assert np.array_equal(fin, np.isfinite(got.log_marginal_posterior))
    assert np.max(np.abs(got.log_marginal_posterior[fin] - want[fin])) < 1e-10
    return got


@pytest.mark.parametrize('kind', ['rouse', 'gauss'])
@pytest.mark.parametrize('S,T', [(2, 64), (3, 44)])
@pytest.mark.parametrize('k', [0, 1, 2, 3])
def test_parity_with_fix_exhaustive(kind, S, T, k):
    model, traj = make(kind, S, T, 1000 * S + 10 * k + (kind == 'gauss'), missing=(0, 1, 9, 30))
    check_parity(model, traj, k)


def test_parity_peaked():
    # a posterior so sharp that the marginals span more than 100 orders of magnitude (and stay clear of underflow: ~16 nats
    # per frame in the wrong state, 80 frames)
    rng = np.random.default_rng(7)
    T = 80
    model = bild_amd.GenericGaussianModel([[(np.arange(T + 8, dtype=float), m, 1)] * 2 for m in (-2.0, 2.0)])
    steps = np.where(np.arange(T)[:, None] < 40, -2.0, 2.0) + rng.normal(size=(T, 2))
    traj = np.cumsum(steps, axis=0)
    traj[[0, 17]] = np.nan
    got = check_parity(model, traj, 2)
    lp = got.log_marginal_posterior
    assert np.all(np.isfinite(lp))
    assert np.max(lp) - np.min(lp) > 100 * np.log(10)


@pytest.mark.parametrize('kind', ['rouse', 'gauss'])
def test_k0_is_mean_over_constant_profiles(kind):
    model, traj = make(kind, 3, 50, 5, missing=(0, 3))
    got = bild_amd.exact_evidence(traj, model, 0)
    ls = [model.logL(bild_amd.Loopingprofile(np.full(50, s)), traj) for s in range(3)]
    assert got.n_profiles == 3
    assert abs(got.logev - (logsumexp(ls) - np.log(3))) < 1e-10
    assert got.map_logL == max(ls)


@pytest.mark.parametrize('kind', ['rouse', 'gauss'])
def test_million_profiles_against_oracle(kind):
    T, k = 1000, 2
    model, traj = make(kind, 2, T, 11, missing=(0, 500, 501))
    got = bild_amd.exact_evidence(traj, model, k)
    seg_start, seg_state = X.enumerate_profiles(T, k, model.transitions)
    assert got.n_profiles == len(seg_start) == 2 * 999 * 998 // 2
    logL = np.concatenate([model.logL_segments(seg_start[lo:lo + (1 << 17)], seg_state[lo:lo + (1 << 17)], traj)
                           for lo in range(0, len(seg_start), 1 << 17)])
    want = X.reduce(logL, seg_start, seg_state, T, 2)
    assert abs(got.logev - want['logev']) <= 1e-11 * abs(want['logev'])
    assert abs(got.KL - want['KL']) <= 1e-11 * max(1.0, abs(want['KL']))
    j = want['map_index']
    assert got.map_logL == want['map_logL']
    assert np.array_equal(got.map_profile[:], X.states_from_segments(seg_start[j:j + 1], seg_state[j:j + 1], T)[0])
    fin = np.isfinite(want['log_post'])
    assert np.array_equal(fin, np.isfinite(got.log_marginal_posterior))
    # below exp(-600) of the largest weight the oracle's own weights exp(logL - top) approach the subnormal range and
    # carry few digits: compared there to the digits they have
    lp, wp = got.log_marginal_posterior[fin], want['log_post'][fin]
    normal = wp > -600
    err = np.abs(lp - wp)
    assert np.max(err[normal]) < 1e-11, (np.argmax(err[normal]), wp[normal][np.argmax(err[normal])], np.max(err[normal]))
    assert np.all(err[~normal] < 0.1), (wp[~normal][np.argmax(err[~normal])], np.max(err[~normal]))


def same(a, b):
    for name in ('n_profiles', 'n_nan'):
        assert getattr(a, name) == getattr(b, name)
    for name in ('logev', 'KL', 'map_logL'):
        assert np.array_equal(getattr(a, name), getattr(b, name), equal_nan=True), name
    assert (a.map_profile is None) == (b.map_profile is None)
    if a.map_profile is not None:
        assert np.array_equal(a.map_profile[:], b.map_profile[:])
    assert np.array_equal(a.log_marginal_posterior, b.log_marginal_posterior, equal_nan=True)


def close(a, b, tol):
    assert a.n_profiles == b.n_profiles and np.array_equal(a.map_profile[:], b.map_profile[:])
    assert abs(a.logev - b.logev) <= tol * abs(b.logev) and abs(a.KL - b.KL) <= tol * max(1, abs(b.KL))
    fin = np.isfinite(b.log_marginal_posterior)
    assert np.max(np.abs(a.log_marginal_posterior[fin] - b.log_marginal_posterior[fin])) <= tol * 1e3


@pytest.mark.parametrize('kind', ['rouse', 'gauss'])
def test_reproducible(kind):
    rng = np.random.default_rng(3)
    lengths = [60, 45, 72, 50]
    if kind == 'rouse':
        model = rouse_model(2)
        trajs = [rouse_traj(model, T, rng, missing=(0, 5)) for T in lengths]
    else:
        model = gauss_model(rng, 2, 80)
        trajs = [gauss_traj(rng, T, missing=(0, 5)) for T in lengths]
    first = bild_amd.exact_evidence(trajs, model, 2)
    for a, b in zip(first, bild_amd.exact_evidence(trajs, model, 2)):
        same(a, b)
    perm = [2, 0, 3, 1]
    for j, b in zip(perm, bild_amd.exact_evidence([trajs[j] for j in perm], model, 2)):
        same(first[j], b)
    for a, b in zip(first, bild_amd.exact_evidence(trajs, model, 2, scratch_bytes=1)):     # one block per chunk
        same(a, b)
    alone = bild_amd.exact_evidence(trajs[2], model, 2)
    if kind == 'gauss':
        same(first[2], alone)
    else:
        # the likelihood of one trajectory on two different sets agrees to rounding (include/bild_amd.h, REPRODUCIBILITY
        # CONTRACT); the reduction adds nothing of its own
        close(first[2], alone, 1e-12)


def test_nan_candidates_gauss():
    rng = np.random.default_rng(21)
    T = 40
    model = bild_amd.GenericGaussianModel([[(np.append(np.arange(T + 8) * 0.5 + 0.1, 50.0), 0.0, 0),
                                            (np.arange(T + 8) * 0.5, 0.0, 1)] for _ in range(2)])
    x = gauss_traj(rng, T)
    x[10:15, 0] = np.nan            # a later ss_order-0 interval inside frames 10 .. 14 has no valid value in dimension 0
    got = bild_amd.exact_evidence(x, model, 2)
    assert got.n_nan > 0 and np.isnan(got.logev) and np.isnan(got.KL)
    assert got.map_profile is not None and np.isfinite(got.map_logL)
    assert got.map_logL == model.logL(got.map_profile, x)


@pytest.mark.parametrize('kind', ['rouse', 'gauss'])
def test_empty_trajectory_in_batch(kind):
    rng = np.random.default_rng(9)
    if kind == 'rouse':
        model = rouse_model(2)
        trajs = [rouse_traj(model, 50, rng), rouse_traj(model, 2, rng, cuts=[1, 1])]
    else:
        model = gauss_model(rng, 2, 60)
        trajs = [gauss_traj(rng, 50), gauss_traj(rng, 2)]
    full, empty = bild_amd.exact_evidence(trajs, model, 2)
    assert empty.n_profiles == 0 and empty.logev == -np.inf and np.isnan(empty.KL)
    assert empty.map_profile is None and np.isnan(empty.map_logL) and empty.n_nan == 0
    assert empty.log_marginal_posterior.shape == (2, 2) and np.all(np.isnan(empty.log_marginal_posterior))
    alone = check_parity(model, trajs[0], 2)
    if kind == 'gauss':
        same(full, alone)
    else:
        close(full, alone, 1e-12)
