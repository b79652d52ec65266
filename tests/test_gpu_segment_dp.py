"""
The segment recursion on the GPU (bild_amd.exact.exact_sample, csrc/gauss_segdp.hip): against the
enumeration of `exact_evidence` for k <= 3, against the NumPy oracle tests/segment_oracle.py beyond, T = 1000 with
k_max = 20, a peaked posterior, the NaN modes, and bit-identity across calls, batch orders, batch sizes and chunking.
Tolerances as in tests/test_gpu_exact.py: logev 1e-10, KL 1e-9, finite log marginals 1e-10, map_logL 1e-10.
"""
import warnings

import numpy as np
import pytest

import bild_amd
import exact_oracle as X
import helpers as H
import segment_cases as C
from bild_amd.exact import results_from_arrays
from bild_amd.profiles import segments_from_st, segments_from_states

pytestmark = pytest.mark.gpu


def n_switches(profile):
    return int(np.count_nonzero(np.diff(np.asarray(profile[:]))))


def check_against_enumeration(r, k, e, same_map):
    """ `ExactSamplingResults` r at k against the `ExactResult` e of the same trajectory """
    assert r.n_profiles[k] == e.n_profiles and r.n_omitted[k] == 0 and e.n_nan == 0
    assert abs(r.evidence[k] - e.logev) < 1e-10, (k, r.evidence[k], e.logev)
    assert abs(r.KL[k] - e.KL) < 1e-9, (k, r.KL[k], e.KL)
    assert abs(r.map_logL[k] - e.map_logL) < 1e-10, (k, r.map_logL[k], e.map_logL)
    if same_map:
        assert np.array_equal(r.map_profile(k)[:], e.map_profile[:]), k
    got, want = r.log_marginal_posterior_k(k), e.log_marginal_posterior
    fin = np.isfinite(want)
    assert np.array_equal(fin, np.isfinite(got))
    # below exp(-600) of the largest weight the enumeration's own weights exp(logL - top) approach the subnormal range and
    # keep few digits (tests/test_gpu_exact.py, test_million_profiles_against_oracle): compared there to the digits they have
    normal = fin & (want > -600)
    with np.errstate(invalid='ignore'):     # (-inf in both)
        err = np.abs(got - want)
    assert np.max(err[normal]) < 1e-10, (k, np.max(err[normal]))
    assert np.all(err[fin & ~normal] < 0.1)


@pytest.mark.parametrize('S,T,missing', [(2, 200, ()), (2, 64, (0, 9, 30)), (3, 44, ()), (3, 40, (0, 1, 2))])
def test_against_exact_evidence(S, T, missing):
    rng = np.random.default_rng(100 * S + T)
    # (isolated missing frames with random ss_orders; a longer leading gap with ss_order 1 everywhere: a later ss_order-0
    # window without a valid frame is NaN, test_nan_windows_against_oracle_k12)
    model = C.random_model(rng, S, T + 8, orders=np.ones((S, 2), dtype=int) if len(missing) == 3 and missing[1] == 1 else None)
    x = C.random_traj(rng, T, missing)
    r = bild_amd.exact_sample(x, model, k_max=3)
    W = F = None
    if T <= 64:
        W, F = C.tables(model, x)
    for k in range(4):
        e = bild_amd.exact_evidence(x, model, k)
        unique = not missing
        if W is not None:
            # is the maximum attained once?  (from the oracle's logL of every profile; a first segment of one frame whose
            # dimensions are all ss_order 1 has no term, so even gap-free data can tie there)
            logL = C.table_logl(W, F, *X.enumerate_profiles(T, k, model.transitions), T)
            unique = int(np.sum(logL >= np.max(logL) - 1e-9)) == 1
            if not missing:
                assert unique
        check_against_enumeration(r, k, e, same_map=unique)
        assert n_switches(r.map_profile(k)) == k


def order0_gap_case(rng, T):
    model = bild_amd.GenericGaussianModel([[(np.append(np.arange(T + 8) * 0.5 + 0.1, 50.0), 0.3 * s, 0),
                                            (np.arange(T + 8) * (0.5 + s), 0.0, 1)] for s in range(2)])
    x = C.random_traj(rng, T)
    x[20:26, 0] = np.nan        # a later ss_order-0 segment inside frames 20 .. 25 has no valid value in dimension 0
    return model, x


def check_against_oracle(r, res, out, model, x, W, F, same_map, marginals=True):
    """ (marginals=False leaves the log marginals to the caller: tests/test_gpu_segment_wide.py, below the linear range) """
    K = len(r.k)
    T = len(x)
    for k in range(K):
        assert r.n_profiles[k] == out['n_profiles'][k] and r.n_omitted[k] == out['n_omitted'][k], k
        for name, got, want, tol in (('logev', r.evidence[k], out['logev'][k], 1e-10), ('KL', r.KL[k], out['KL'][k], 1e-9),
                                     ('map_logL', r.map_logL[k], out['map_logL'][k], 1e-10)):
            if np.isfinite(want):
                assert abs(got - want) < tol, (name, k, got, want)
            else:
                assert np.array_equal(got, want, equal_nan=True), (name, k, got, want)
        p = r.map_profile(k)
        assert (p is None) == (out['map_states'][k] is None)
        if p is not None:
            assert n_switches(p) == k
            a, b = segments_from_states(np.asarray(p[:]))
            assert abs(C.table_logl(W, F, a, b, T)[0] - out['map_logL'][k]) < 1e-10       # the profile attains the maximum
            if same_map:
                assert np.array_equal(p[:], out['map_states'][k]), k
        if not marginals:
            continue
        got, want = r.log_marginal_posterior_k(k), out['log_post'][k]
        fin = np.isfinite(want)
        assert np.array_equal(fin, np.isfinite(got)) and np.array_equal(np.isnan(got), np.isnan(want)), k
        if fin.any():
            assert np.max(np.abs(got[fin] - want[fin])) < 1e-10, (k, np.max(np.abs(got[fin] - want[fin])))


@pytest.mark.parametrize('case', ['s2_gapfree', 's3_gapfree', 's2_inner_gap', 's3_leading_and_inner_gap'])
def test_against_oracle_k12(case):
    S = int(case[1])
    rng = np.random.default_rng(sum(map(ord, case)))
    T = 60 if S == 2 else 52
    # ss_order 1 everywhere where there is a gap: nothing is NaN, and every switch frame inside the gap ties
    model = C.random_model(rng, S, T + 8, orders=None if 'gapfree' in case else np.ones((S, 2), dtype=int))
    missing = () if 'gapfree' in case else (24, 25, 26, 27) if 'leading' not in case else (0, 1, 30, 31, 32, 33)
    x = C.random_traj(rng, T, missing)
    r = bild_amd.exact_sample(x, model, k_max=12)
    res, out = C.oracle_arrays(model, x, 12)
    W, F = C.tables(model, x)
    check_against_oracle(r, res, out, model, x, W, F, same_map='gapfree' in case)
    assert np.all(np.isfinite(r.evidence))


@pytest.mark.parametrize('nan', ['propagate', 'omit'])
def test_nan_windows_against_oracle_k12(nan):
    rng = np.random.default_rng(33)
    T = 56
    model, x = order0_gap_case(rng, T)
    r = bild_amd.exact_sample(x, model, k_max=12, nan=nan)
    res, out = C.oracle_arrays(model, x, 12, nan=nan)
    W, F = C.tables(model, x)
    check_against_oracle(r, res, out, model, x, W, F, same_map=False)
    if nan == 'propagate':
        assert np.all(np.isfinite(r.evidence[:2])) and np.all(np.isnan(r.evidence[2:]))    # two switches inside the gap
        assert np.all(np.isfinite(r.map_logL))
        e = bild_amd.exact_evidence(x, model, 2)
        assert e.n_nan > 0 and abs(e.map_logL - r.map_logL[2]) < 1e-10
    else:
        assert np.all(np.isfinite(r.evidence)) and sum(r.n_omitted[2:]) > 0 and r.n_omitted[:2] == [0, 0]
        e = bild_amd.exact_evidence(x, model, 2)
        assert r.n_omitted[2] == e.n_nan and r.n_profiles[2] == e.n_profiles - e.n_nan


def test_T1000_kmax20():
    T, k_max = 1000, 20
    rng = np.random.default_rng(11)
    model = C.random_model(rng, 2, T + 8)
    x = C.random_traj(rng, T, (0, 500))      # (isolated missing frames: nothing is NaN)
    r = bild_amd.exact_sample(x, model, k_max=k_max)
    assert np.all(np.isfinite(r.evidence)) and np.all(np.isfinite(r.KL)) and np.all(r.KL >= 0)
    for k in range(3):      # k = 2: 997 002 profiles
        check_against_enumeration(r, k, bild_amd.exact_evidence(x, model, k), same_map=False)
    assert r.n_profiles[2] == 997002
    for k in range(k_max + 1):
        p = r.map_profile(k)
        assert n_switches(p) == k
        a, b = segments_from_states(np.asarray(p[:]))
        assert abs(model.logL_segments(a, b, x)[0] - r.map_logL[k]) < 1e-10, k
        # 200 random profiles of exactly k switches
        ss, thetas = H.candidate_profiles(rng, 400, k, 2)
        a, b = segments_from_st(ss, thetas, T)
        keep = np.all(np.diff(a, axis=1) > 0, axis=1) & (a[:, -1] < T) if k else np.ones(len(a), dtype=bool)
        a, b = a[keep][:200], b[keep][:200]
        assert len(a) == 200
        assert np.all(model.logL_segments(a, b, x) <= r.map_logL[k])
        lp = r.log_marginal_posterior_k(k)
        assert np.all(np.isfinite(np.max(lp, axis=0)))
        with np.errstate(under='ignore'):
            assert np.max(np.abs(np.sum(np.exp(lp), axis=0) - 1.0)) < 1e-12


def test_peaked_against_oracle():
    # tests/test_gpu_exact.py, test_parity_peaked: marginals spanning more than 100 orders of magnitude
    rng = np.random.default_rng(7)
    T = 80
    model = bild_amd.GenericGaussianModel([[(np.arange(T + 8, dtype=float), m, 1)] * 2 for m in (-2.0, 2.0)])
    steps = np.where(np.arange(T)[:, None] < 40, -2.0, 2.0) + rng.normal(size=(T, 2))
    x = np.cumsum(steps, axis=0)
    x[[0, 17]] = np.nan
    r = bild_amd.exact_sample(x, model, k_max=8)
    res, out = C.oracle_arrays(model, x, 8)
    W, F = C.tables(model, x)
    check_against_oracle(r, res, out, model, x, W, F, same_map=False)
    lp = np.array([r.log_marginal_posterior_k(k) for k in range(9)])
    assert np.all(np.isfinite(lp)) and np.all(np.isfinite(r.evidence)) and np.all(np.isfinite(r.KL))
    assert np.max(lp[2]) - np.min(lp[2]) > 100 * np.log(10)
    assert r.best_k() == 1


def same(a, b):
    assert a.n_profiles == b.n_profiles and a.n_omitted == b.n_omitted
    for name in ('evidence', 'KL', 'map_logL', '_seg_start', '_seg_state', '_log_post'):
        assert np.array_equal(getattr(a, name), getattr(b, name), equal_nan=name != '_seg_start'), name


def test_bit_identity():
    rng = np.random.default_rng(3)
    lengths = [60, 3, 131, 45, 72]
    model = C.random_model(rng, 2, 140)
    trajs = [C.random_traj(rng, T, (0, 5) if T > 10 else ()) for T in lengths]
    first = bild_amd.exact_sample(trajs, model, k_max=6)
    assert np.all(first[1].evidence[3:] == -np.inf) and np.all(np.isfinite(first[1].evidence[:3]))      # T = 3 < k_max
    for a, b in zip(first, bild_amd.exact_sample(trajs, model, k_max=6)):
        same(a, b)
    perm = [2, 0, 4, 1, 3]
    for j, b in zip(perm, bild_amd.exact_sample([trajs[j] for j in perm], model, k_max=6)):
        same(first[j], b)
    for a, b in zip(first, bild_amd.exact_sample(trajs, model, k_max=6, scratch_bytes=1)):      # one trajectory per chunk
        same(a, b)
    for j in (0, 1, 2):
        same(first[j], bild_amd.exact_sample(trajs[j], model, k_max=6))
    # without marginals: the same numbers
    for a, b in zip(first, bild_amd.exact_sample(trajs, model, k_max=6, marginals=False)):
        assert np.array_equal(a.evidence, b.evidence, equal_nan=True) and np.array_equal(a._seg_start, b._seg_start)
        with pytest.raises(ValueError, match='marginals'):
            b.log_marginal_posterior_k(0)


def test_list_equals_single_calls_and_methods_agree_with_oracle():
    rng = np.random.default_rng(17)
    model = C.random_model(rng, 2, 60)
    truth = np.repeat([0, 1, 0], [15, 17, 16])
    trajs = [model.trajectory_from_loopingprofile(bild_amd.Loopingprofile(truth), rng=rng)[:], C.random_traj(rng, 40)]
    batch = bild_amd.exact_sample(trajs, model, dE=1.0, k_max=6)
    assert isinstance(batch, list) and len(batch) == 2
    for x, r in zip(trajs, batch):
        same(r, bild_amd.exact_sample(x, model, dE=1.0, k_max=6))
        res, out = C.oracle_arrays(model, x, 6)
        o = results_from_arrays(x, model, 1.0, model.transitions, res)
        with warnings.catch_warnings():
            warnings.simplefilter('error')
            for dE in (None, 0, 3.0):
                assert r.best_k(dE) == o.best_k(dE)
                assert np.array_equal(r.best_profile(dE)[:], o.best_profile(dE)[:])
                assert np.max(np.abs(r.log_marginal_posterior(dE) - o.log_marginal_posterior(dE))) < 1e-10
            got, want = r.log_marginal_posterior('average'), o.log_marginal_posterior('average')
        assert np.max(np.abs(got - want)) < 1e-10


def test_kmax64_short_trajectory():
    # the largest k_max on T = 40: k = 0 ... 39 have profiles, the rest none
    rng = np.random.default_rng(64)
    T = 40
    model = C.random_model(rng, 2, T + 8)
    x = C.random_traj(rng, T, (0, 11))
    r = bild_amd.exact_sample(x, model, k_max=64)
    res, out = C.oracle_arrays(model, x, 64, with_marginals=False)
    assert r.n_profiles == out['n_profiles'] and r.n_profiles[39] == 2 and r.n_profiles[40:] == [0] * 25
    assert np.max(np.abs(r.evidence[:40] - out['logev'][:40])) < 1e-10 and np.all(r.evidence[40:] == -np.inf)
    assert np.max(np.abs(r.KL[:40] - out['KL'][:40])) < 1e-9 and np.all(np.isnan(r.KL[40:]))
    assert np.max(np.abs(r.map_logL[:40] - out['map_logL'][:40])) < 1e-10 and np.all(np.isnan(r.map_logL[40:]))
    assert all(n_switches(r.map_profile(k)) == k for k in range(40)) and r.map_profile(40) is None
    small = bild_amd.exact_sample(x, model, k_max=5)
    for k in range(6):      # the levels do not depend on k_max
        assert np.array_equal(r.log_marginal_posterior_k(k), small.log_marginal_posterior_k(k))
    _, out5 = C.oracle_arrays(model, x, 5)
    assert np.max(np.abs(np.array([small.log_marginal_posterior_k(k) for k in range(6)]) - out5['log_post'])) < 1e-10
    lp = np.array([r.log_marginal_posterior_k(k) for k in range(40)])
    with np.errstate(under='ignore'):
        assert np.max(np.abs(np.sum(np.exp(lp), axis=1) - 1.0)) < 1e-12
    assert np.all(np.isnan(r.log_marginal_posterior_k(40)))


def test_longest_trajectory():
    # T = 2048, the set's limit: k <= 2 against the enumeration (k = 2: 4 188 462 profiles)
    rng = np.random.default_rng(2048)
    T = 2048
    lags = np.arange(T + 1, dtype=float)
    model = bild_amd.GenericGaussianModel([[(0.8 * lags ** 0.6 + np.where(lags > 0, 0.2, 0.0), m, 1)] * 2 for m in (0.0, 0.3)])
    x = C.random_traj(rng, T)
    r = bild_amd.exact_sample(x, model, k_max=3)
    for k in range(3):
        check_against_enumeration(r, k, bild_amd.exact_evidence(x, model, k), same_map=True)
    p = r.map_profile(3)
    a, b = segments_from_states(np.asarray(p[:]))
    assert n_switches(p) == 3 and abs(model.logL_segments(a, b, x)[0] - r.map_logL[3]) < 1e-10
