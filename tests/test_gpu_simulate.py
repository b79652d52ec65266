"""
The batched Rouse generator on the GPU (bild_amd/csrc/sim.hip through MultiStateRouse.trajectories_from_loopingprofiles):
replay mode against the loop of trajectory_from_loopingprofile on the same Generator, the law of the device mode
against the Gaussian its profile defines, the device mode's independence of batch and launch, and the chunked upload of
the replay normals.  `-s` prints the worst relative deviation from the loop.
"""

import numpy as np
import pytest

import bild_amd
from bild_amd import _lib
from bild_amd import models as M

pytestmark = pytest.mark.gpu


def make_model(S, N, d, com=False, err=0.1):
    loops = [None, (0, -1), (1, max(N // 2, 1))][:S]
    w = np.linspace(0.2, 1.0, N) if com else 'end2end'     # sum(w) != 0: the centre-of-mass random walk is measured
    return bild_amd.MultiStateRouse(N, 1.0, 0.7, d=d, looppositions=loops, measurement=w, localization_error=err)


def profile(rng, T, S, switches):
    st = np.full(T, rng.integers(S))
    if T > 1 and switches:
        for t in np.sort(rng.choice(np.arange(1, T), size=min(switches, T - 1), replace=False)):
            st[t:] = (st[t - 1] + 1 + rng.integers(S - 1)) % S
    return st


def compare(got, want):
    assert len(got) == len(want)
    worst = 0.0
    for g, w in zip(got, want):
        assert g[:].shape == w[:].shape
        assert np.array_equal(np.isnan(g[:]), np.isnan(w[:]))
        ok = ~np.isnan(w[:])
        if ok.any():
            scale = np.max(np.abs(w[:][ok]))
            dev = np.max(np.abs(g[:][ok] - w[:][ok]))
            assert dev <= 1e-9 * scale, (dev, scale)
            worst = max(worst, dev / scale)
        assert np.array_equal(g.localization_error, w.localization_error)
        assert g.meta['loopingprofile'] is w.meta['loopingprofile']
    return worst


CASES = [(S, N, d) for S in (2, 3) for N in (1, 5, 20, 64, 130) for d in (1, 3)]


@pytest.mark.parametrize('S,N,d', CASES)
def test_replay_equals_the_loop(S, N, d):
    rng = np.random.default_rng(1000 * S + 10 * N + d)
    com = (N + d) % 2 == 0
    model = make_model(S, N, d, com=com)
    lengths = [1, 2, 37, 300, 1500] if N <= 20 else [1, 64, 257, 1500]
    profiles = [profile(rng, T, S, sw) for T in lengths for sw in (0, 1, 40)][::2]
    if N <= 20:
        profiles[0] = bild_amd.Loopingprofile(profiles[0])
    worst = 0.0
    for missing in (None, 0.2, 3, np.array([0, -1]),
                    [None if T < 4 else (0.5 if i % 2 else 2) for i, T in enumerate(map(len, profiles))]):
        if isinstance(missing, int) or isinstance(missing, np.ndarray):
            use = [p for p in profiles if len(p) >= 3]
        else:
            use = profiles
        seed = int(rng.integers(2 ** 32))
        a, b = np.random.default_rng(seed), np.random.default_rng(seed)
        if isinstance(missing, list):
            want = [model.trajectory_from_loopingprofile(p, missing_frames=m, rng=a) for p, m in zip(use, missing)]
        else:
            want = [model.trajectory_from_loopingprofile(p, missing_frames=missing, rng=a) for p in use]
        got = model.trajectories_from_loopingprofiles(use, missing_frames=missing, rng=b)
        worst = max(worst, compare(got, want))
        assert a.random() == b.random()     # the Generator is where the loop leaves it
    print(f"replay S={S} N={N} d={d} com={com}: worst |delta| / max|data| = {worst:.2e}")


def test_replay_with_an_array_of_profiles_and_a_per_call_error():
    model = make_model(2, 8, 2, err=None)
    rng = np.random.default_rng(5)
    profiles = np.stack([profile(rng, 50, 2, k) for k in range(6)])
    a, b = np.random.default_rng(2), np.random.default_rng(2)
    want = [model.trajectory_from_loopingprofile(p, localization_error=[0.1, 0.3], rng=a) for p in profiles]
    got = model.trajectories_from_loopingprofiles(profiles, localization_error=[0.1, 0.3], rng=b)
    for g, w in zip(got, want):
        assert np.array_equal(g.meta['loopingprofile'], w.meta['loopingprofile'])
        assert np.max(np.abs(g[:] - w[:])) <= 1e-9 * np.max(np.abs(w[:]))


def dense_law(model, states, missing, err):
    """ mean and covariance of the data vector (valid frames, dimension-major) from the dense per-state arrays """
    a = model.arrays()
    B, G, Sig, M0, C0 = a['B'], a['G'], a['Sig'], a['M0'], a['C0']
    w = model.measurement
    T, N, d = len(states), w.shape[0], model.d
    mean = np.empty((T, N, d))
    # x_t as a linear map of independent unit normals: A[t] (N, T*N)
    A = np.zeros((T, N, T * N))
    ev, U = np.linalg.eigh(C0[states[0]])
    L0 = U * np.sqrt(np.maximum(ev, 0))
    mean[0] = M0[states[0]]
    A[0][:, :N] = L0
    for t in range(1, T):
        s = states[t]
        ev, U = np.linalg.eigh(Sig[s])
        Ls = U * np.sqrt(np.maximum(ev, 0))
        mean[t] = B[s] @ mean[t - 1] + G[s]
        A[t] = B[s] @ A[t - 1]
        A[t][:, t * N:(t + 1) * N] += Ls
    Y = np.einsum('n,tnm->tm', w, A)            # (T, T*N): measurement as a map of the normals
    cov = Y @ Y.T
    valid = np.setdiff1d(np.arange(T), missing)
    mu = np.concatenate([(w @ mean[valid, :, k].T) for k in range(d)])
    C = np.zeros((d * len(valid),) * 2)
    for k in range(d):
        sl = slice(k * len(valid), (k + 1) * len(valid))
        C[sl, sl] = cov[np.ix_(valid, valid)] + err[k] ** 2 * np.eye(len(valid))
    return mu, C, valid


def test_device_mode_has_the_law_of_the_model():
    from scipy import stats
    model = make_model(3, 6, 2, com=True, err=0.2)
    force = np.random.default_rng(7).normal(size=(3, 6, 2))
    for m, F in zip(model.models, force):       # an external force: non-zero means G and M0
        m.F = F
        m._dynamics = {'needs_updating': True}
    states = np.array([0, 0, 0, 0, 2, 2, 2, 1, 1, 1, 1, 1])
    missing = [5]
    n = 20000
    trajs = model.trajectories_from_loopingprofiles([states] * n, localization_error=[0.2, 0.3], missing_frames=[np.array(missing)] * n,
                                                    seed=20240607)
    X = np.stack([t[:] for t in trajs])                 # (n, T, d)
    assert np.all(np.isnan(X[:, missing])) and not np.any(np.isnan(np.delete(X, missing, axis=1)))
    mu, C, valid = dense_law(model, states, missing, np.array([0.2, 0.3]))
    Y = np.concatenate([X[:, valid, k] for k in range(model.d)], axis=1)
    se = np.sqrt(np.diag(C) / n)
    z = (Y.mean(axis=0) - mu) / se
    assert np.max(np.abs(z)) < 5, z
    Lc = np.linalg.cholesky(C)
    r = np.linalg.solve(Lc, (Y - mu).T)
    m2 = np.sum(r ** 2, axis=0)
    p = stats.kstest(m2, stats.chi2(df=len(mu)).cdf).pvalue
    print(f"device law: max |mean z| = {np.max(np.abs(z)):.2f}, KS p = {p:.3f} (df = {len(mu)})")
    assert p > 1e-3


def test_device_mode_does_not_depend_on_the_batch():
    rng = np.random.default_rng(11)
    model = make_model(2, 20, 3)
    profiles = [profile(rng, int(T), 2, int(k)) for T, k in zip(rng.integers(1, 400, 200), rng.integers(0, 5, 200))]
    a = model.trajectories_from_loopingprofiles(profiles, missing_frames=0.1, seed=77)
    b = model.trajectories_from_loopingprofiles(profiles[:10], missing_frames=0.1, seed=77)
    other = [profile(rng, 50, 2, 3) for _ in range(200)]
    other[:10] = profiles[:10]
    c = model.trajectories_from_loopingprofiles(other, missing_frames=0.1, seed=77)
    again = model.trajectories_from_loopingprofiles(profiles, missing_frames=0.1, seed=77)
    for i in range(10):
        assert np.array_equal(a[i][:], b[i][:], equal_nan=True)
        assert np.array_equal(a[i][:], c[i][:], equal_nan=True)
    for x, y in zip(a, again):
        assert np.array_equal(x[:], y[:], equal_nan=True)
    diff = model.trajectories_from_loopingprofiles(profiles[:10], missing_frames=0.1, seed=78)
    assert all(not np.array_equal(x[:], y[:], equal_nan=True) for x, y in zip(b, diff))
    assert any(np.isnan(t[:]).any() for t in a)
    # different trajectories of one call are different, and the fresh-seed default gives new data each call
    assert not np.array_equal(a[0][:1], model.trajectories_from_loopingprofiles([profiles[0]] * 2, seed=77)[1][:1])
    f1 = model.trajectories_from_loopingprofiles(profiles[:2])
    f2 = model.trajectories_from_loopingprofiles(profiles[:2])
    assert not np.array_equal(f1[0][:], f2[0][:])


def test_replay_upload_in_chunks_is_bit_identical():
    rng = np.random.default_rng(3)
    model = make_model(2, 20, 3, com=True)
    profiles = [profile(rng, int(T), 2, 3) for T in rng.integers(50, 300, 40)]
    g = np.random.default_rng(99)
    small = []
    for i in range(0, 40, 5):
        small += model.trajectories_from_loopingprofiles(profiles[i:i + 5], missing_frames=0.05, rng=g)
    h = np.random.default_rng(99)
    T = np.array([len(p) for p in profiles])
    mask, z = M._replay_draws([0.05] * 40, T, 20, 3, h)
    assert g.random() == h.random()
    seg_start, seg_state = M._ragged_segments(profiles, T)
    budget = z.nbytes // 9
    big = _lib.rouse_simulate(*model._modal_arrays(), model.measurement, T, seg_start, seg_state, mask,
                              np.tile(model.localization_error, (40, 1)), normals=z, scratch_bytes=budget)
    assert z.nbytes > 8 * budget        # at least nine chunks
    offs = np.concatenate([[0], np.cumsum(T)])
    for i, t in enumerate(small):
        assert np.array_equal(big[offs[i]:offs[i + 1]], t[:], equal_nan=True)
    # a trajectory larger than the budget is refused
    with pytest.raises(_lib.BildAmdError) as e:
        _lib.rouse_simulate(*model._modal_arrays(), model.measurement, T, seg_start, seg_state, mask,
                            np.tile(model.localization_error, (40, 1)), normals=z, scratch_bytes=1024)
    assert e.value.code == _lib.ERR_UNSUPPORTED


def test_widest_supported_chain():
    # N = 256: the dimensions are split over several workgroups (at most 1024 lanes each)
    rng = np.random.default_rng(8)
    model = make_model(2, 256, 8)
    profiles = [profile(rng, 40, 2, 2), profile(rng, 3, 2, 1)]
    a, b = np.random.default_rng(4), np.random.default_rng(4)
    want = [model.trajectory_from_loopingprofile(p, rng=a) for p in profiles]
    print(f"N=256 d=8: worst {compare(model.trajectories_from_loopingprofiles(profiles, rng=b), want):.2e}")
