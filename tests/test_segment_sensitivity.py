"""
The evidence gradient without a GPU (bild_amd.exact.exact_sensitivities): the NumPy oracle
tests/segment_sensitivity_oracle.py against central differences of the segment recursion's log evidence and against the
enumeration of every profile, its identities, the argument errors of `exact_sensitivities` and `fit_marginal`, and the designed
cases of tests/test_gpu_segment_sensitivity_tiles.py: that they build, where their evidence is NaN, and the k = 0 identity.
"""
import os

import numpy as np
import pytest
from scipy import stats
from scipy.special import logsumexp

import bild_amd
import exact_oracle as X
import gauss_oracle as G
import gauss_sensitivity_oracle as GS
import segment_cases as C
import segment_oracle as SO
import segment_sensitivity_cases as SC
from bild_amd.profiles import states_from_segments
from test_segment_dp import CASES, build

K_MAX = 4
FD_STEP, FD_TOL = 1e-5, 1e-6        # the project's figure for such checks; 1.3e-9 was seen
ENUM_TOL = 1e-10                    # relative to the largest entry
MODES = [(name, nan) for name in CASES for nan in (('propagate', 'omit') if 'order0' in name else ('propagate',))]
PRIOR = np.array([np.log(0.1), np.log(0.4), -np.inf, np.log(0.3), np.log(0.2)])


def logev_at(model, x, theta, nan):
    msd, msd_inf, mean = SC.family_arrays(model, theta)
    W, F = G.tables(msd, msd_inf, mean, model.ss_order, x)
    return SO.solve(W, F, model.transitions, K_MAX, nan=nan, with_marginals=False)['logev']


def log_marginal_of(logev, log_prior):
    use = log_prior > -np.inf
    return logsumexp((log_prior - logsumexp(log_prior[use]) + logev)[use])


@pytest.mark.parametrize('name,nan', MODES)
def test_oracle_gradient_against_central_differences(name, nan):
    model, x = build(name)
    prior = PRIOR.copy()
    if nan == 'propagate' and 'order0' in name:
        prior[2:] = -np.inf       # the k with a NaN evidence get no weight: the rest is still a marginal
    got = SC.oracle(model, x, K_MAX, log_k_prior=prior, nan=nan)
    fin = np.isfinite(got['logev'])
    assert fin.sum() >= 2 and np.all(np.isfinite(got['grad']))
    worst = 0.0
    for p in range(4):
        e = np.zeros(4)
        e[p] = FD_STEP
        hi, lo = logev_at(model, x, SC.BASE + e, nan), logev_at(model, x, SC.BASE - e, nan)
        fd = (hi - lo) / (2 * FD_STEP)
        err = np.max(np.abs(got['grad_k'][fin, p] - fd[fin]))
        fd_m = (log_marginal_of(hi, prior) - log_marginal_of(lo, prior)) / (2 * FD_STEP)
        worst = max(worst, err, abs(got['grad'][p] - fd_m))
        assert err < FD_TOL and abs(got['grad'][p] - fd_m) < FD_TOL, (p, err, got['grad'][p], fd_m)
    print(f"{name} {nan}: worst |grad - central difference| = {worst:.2e}")


def enumerated(model, x, k, nan):
    """ posterior means over every profile of k switches of logL, its gradient and its Fisher matrix, and the KL + logev """
    T = len(x)
    seg_start, seg_state = X.enumerate_profiles(T, k, model.transitions)
    states = states_from_segments(seg_start, seg_state, T)
    logL, g, F = GS.batch(model.msd, model.msd_inf, model.mean, model.ss_order, [x], states,
                          **dict(zip(('dmsd', 'dmsd_inf', 'dmean'), SC.derivatives(model))))
    bad = np.isnan(logL)
    if bad.any() and nan == 'propagate':
        return None
    logL, g, F = logL[~bad], g[~bad], F[~bad]
    p = np.exp(logL - logsumexp(logL))
    return p @ logL, p @ g, np.tensordot(p, F, axes=1)


def close(got, want):
    return np.max(np.abs(got - want)) <= ENUM_TOL * max(np.max(np.abs(want)), 1e-300)


@pytest.mark.parametrize('name,nan', MODES)
def test_oracle_against_enumeration(name, nan):
    model, x = build(name)
    got = SC.oracle(model, x, K_MAX, nan=nan)
    W, F = C.tables(model, x)
    ref = SO.solve(W, F, model.transitions, K_MAX, nan=nan, with_marginals=False)
    seen = 0
    for k in range(K_MAX + 1):
        want = enumerated(model, x, k, nan)
        if want is None:
            assert np.isnan(got['logev'][k]) and np.all(np.isnan(got['grad_k'][k]))
            continue
        seen += 1
        el, g, Fm = want
        assert close(got['exp_logl_k'][k], el), (k, got['exp_logl_k'][k], el)
        assert close(got['grad_k'][k], g), (k, got['grad_k'][k], g)
        assert close(got['fisher_k'][k], Fm), (k, got['fisher_k'][k], Fm)
        # the posterior mean of logL of a single k is KL + logev, and a profile of k switches has k + 1 segments
        assert close(got['exp_logl_k'][k], ref['KL'][k] + ref['logev'][k])
        assert abs(got['n_segments'][k] - (k + 1)) < 1e-12
        assert np.all(np.linalg.eigvalsh(got['fisher_k'][k]) > -1e-9)
    assert seen >= (2 if nan == 'propagate' and 'order0' in name else K_MAX + 1)


def test_oracle_prior_over_k():
    model, x = build('s2_inner_gap4')
    uni = SC.oracle(model, x, K_MAX)
    assert abs(uni['log_marginal'] - (logsumexp(uni['logev']) - np.log(K_MAX + 1))) < 1e-12
    assert abs(uni['k_post'].sum() - 1) < 1e-14
    assert np.allclose(uni['grad'], uni['k_post'] @ uni['grad_k'], rtol=0, atol=1e-13)
    one = SC.oracle(model, x, K_MAX, log_k_prior=np.where(np.arange(K_MAX + 1) == 2, 0.0, -np.inf))
    assert one['log_marginal'] == uni['logev'][2] and np.array_equal(one['grad'], uni['grad_k'][2])
    assert one['exp_logl'] == uni['exp_logl_k'][2] and np.array_equal(one['k_post'], [0, 0, 1, 0, 0])
    # a NaN evidence at a k of positive weight: NaN; at weight 0: skipped
    model, x = build('s2_order0_inner_gap')
    assert np.isnan(SC.oracle(model, x, K_MAX)['log_marginal'])
    ok = SC.oracle(model, x, K_MAX, log_k_prior=np.array([0.0, 0.0, -np.inf, -np.inf, -np.inf]))
    assert np.isfinite(ok['log_marginal']) and np.all(np.isfinite(ok['grad']))


def test_exact_sensitivities_refusals_before_device(built_lib):
    rng = np.random.default_rng(1)
    model = C.random_model(rng, 2, 40)
    x = C.random_traj(rng, 30)
    dmsd, dinf, dmean = SC.derivatives(model)
    with pytest.raises(TypeError):
        bild_amd.exact_sensitivities(bild_amd.Trajectory(np.zeros((30, 3)), localization_error=[0.1] * 3),
                                     bild_amd.MultiStateRouse(20, 1, 5, d=3, localization_error=0.1))
    with pytest.raises(TypeError):
        bild_amd.exact_sensitivities(x, bild_amd.FactorizedModel([stats.maxwell(), stats.maxwell()]))
    with pytest.raises(ValueError, match='k_max = 65'):
        bild_amd.exact_sensitivities(x, model, k_max=65)
    with pytest.raises(ValueError, match="nan = 'drop'"):
        bild_amd.exact_sensitivities(x, model, nan='drop')
    with pytest.raises(ValueError, match='40 frames'):
        bild_amd.exact_sensitivities([x, C.random_traj(rng, 41)], model)
    with pytest.raises(ValueError, match='dmsd has shape'):
        bild_amd.exact_sensitivities(x, model, dmsd=dmsd[:, :, :, :-1])
    with pytest.raises(ValueError, match='disagree'):
        bild_amd.exact_sensitivities(x, model, dmsd=dmsd, dmean=dmean[:2])
    with pytest.raises(ValueError, match='not finite'):
        bild_amd.exact_sensitivities(x, model, dmean=dmean * np.nan)
    with pytest.raises(bild_amd._lib.BildAmdError, match='at most 4'):
        bild_amd.exact_sensitivities(x, model, dmean=np.zeros((5, 2, 2)))
    for bad, match in ((5, 'single k'), (-1, 'single k'), (np.ones(3), 'shape'), (np.ones((2, 5)), 'shape'),
                       ([1, 1, -1, 1, 1], 'non-negative'), ([1, np.nan, 1, 1, 1], 'finite'), (np.zeros(5), 'zero everywhere')):
        with pytest.raises(ValueError, match=match):
            bild_amd.exact_sensitivities(x, model, k_max=4, k_prior=bad)
    assert len(model._trajsets) == 0


def test_fit_marginal_refusals_before_device(built_lib):
    rng = np.random.default_rng(2)
    x = C.random_traj(rng, 30, d=1)
    made = []

    def family(a, b=1.0):
        lags = np.arange(40.0)
        spec = [[(np.append(s * a * (1 - np.exp(-lags / 3)) + 0.02 * (lags > 0), s * a + 0.02), 0.0, 0)] for s in (0.5, 4.0 * b)]
        made.append(spec)
        return spec

    fit = bild_amd.GenericGaussianModel.fit_marginal
    with pytest.raises(ValueError, match='nothing to fit'):
        fit([x], family, {})
    with pytest.raises(ValueError, match='at most 4'):
        fit([x], family, dict(a=1, b=1, c=1, d=1, e=1))
    with pytest.raises(ValueError, match='positive and finite'):
        fit([x], family, dict(a=-1.0))
    with pytest.raises(ValueError, match='tol > 0'):
        fit([x], family, dict(a=1.0), tol=0)
    with pytest.raises(ValueError, match='at least one trajectory'):
        fit([], family, dict(a=1.0))
    with pytest.raises(ValueError, match='k_max = 65'):
        fit([x], family, dict(a=1.0), k_max=65)
    with pytest.raises(ValueError, match="nan = 'drop'"):
        fit([x], family, dict(a=1.0), nan='drop')
    with pytest.raises(ValueError, match='40 frames'):
        fit([x, C.random_traj(rng, 41, d=1)], family, dict(a=1.0))
    with pytest.raises(ValueError, match='single k'):
        fit([x], family, dict(a=1.0), k_max=3, k_prior=4)
    assert len(made) <= 9       # one probe model per call at the most: no trajectory set, no evaluation


# ---------------------------------------------------------------- the designed cases of the GPU tier (beyond one 64-frame tile)

def test_designed_cases_build():
    assert len(SC.DESIGNED) == 14
    for name, (mname, T, missing, k_max, runs) in SC.DESIGNED.items():
        model, x, k = SC.designed(name)
        d = model.msd.shape[1]
        assert x.shape == (T, d) and k == k_max and T > 63 and model.msd.shape[2] >= T and len(runs) >= 1
        assert SC.designed(name)[1] is x and not x.flags.writeable          # built once, shared, left unchanged
        if mname is not None:
            assert model is SC.designed_model(mname)                        # cases of one model can form a batch
            gone = np.zeros(T, dtype=bool)
            gone[list(missing)] = True
            assert np.array_equal(np.isnan(x), np.repeat(gone[:, None], d, axis=1))
        for p in range(5):
            assert [a.shape[0] for a in SC.derivatives(model, p)] == [p] * 3
    # what the cases aim at
    S, d = SC.designed_model('edge').ss_order.shape
    assert (S, d) == (2, 2) and SC.designed_model('edge').ss_order.tolist() == [[0, 1], [1, 0]]
    straddle = SC.designed_model('straddle')
    assert straddle.nStates == 3 and not straddle.transitions[0, 2] and np.all(straddle.ss_order == 1)
    assert set(SC.STRADDLE_MISSING) >= {0, 62, 63, 64, 65, 127} and np.isnan(SC.designed('straddle_T128')[1][-1]).all()
    model, x, _ = SC.designed('order0_gap_T130')
    assert model.ss_order.tolist() == [[0, 1], [0, 1]] and np.array_equal(np.nonzero(np.isnan(x[:, 0]))[0], np.arange(61, 67))
    assert not np.isnan(x[:, 1]).any()
    assert SC.designed_model('d3').msd.shape[1] == 3 and SC.designed_model('d1_S4').msd.shape[:2] == (4, 1)
    assert np.all(SC.designed_model('d1_S4').transitions == ~np.eye(4, dtype=bool))
    for o in (0, 1):        # solve jobs of 260 / 259 entries, factorisations of 260 / 259 rows: the 256-thread stride wraps
        model = SC.designed_model(f'stride_o{o}')
        assert np.all(model.ss_order == o) and model.msd.shape[:2] == (2, 1)
        assert 260 - o > 256 and (259 - o) + 1 > 256


@pytest.mark.parametrize('name', list(SC.DESIGNED))
def test_designed_cases_nan_condition(name):
    """ the oracle's logev is finite at every k, except `order0_gap_T130` under 'propagate': there exactly k >= 2 is NaN """
    k_max = SC.DESIGNED[name][3]
    for nan in sorted({nan for _, nan, _ in SC.designed_runs([name])}):
        logev = SC.designed_logev(name, nan)
        assert logev.shape == (k_max + 1,)
        if (name, nan, None) in SC.NAN_RUNS:
            assert np.all(np.isfinite(logev[:2])) and np.all(np.isnan(logev[2:]))
        else:
            assert np.all(np.isfinite(logev)), (name, nan, logev)
    assert {n for n, _, _ in SC.NAN_RUNS} == {'order0_gap_T130'}
    for n, nan, prior in SC.designed_runs([name]):      # a prior run of a NaN case puts no weight on the NaN ks
        if prior is not None and (n, nan, None) in SC.NAN_RUNS:
            assert np.all(np.isfinite(SC.designed_logev(n, nan)[np.asarray(prior) > 0]))


def test_k0_identity_with_the_flat_profiles():
    """ all prior weight on k = 0: the segment oracle against the softmax-weighted flat profiles of the tangent oracle """
    rng = np.random.default_rng(70)
    lags = np.arange(78, dtype=float)
    msd = np.where(lags > 0, 0.9 * lags ** 0.8 + 0.2, 0.0)
    # two states a little apart, so that both flat profiles keep weight; dimension 0 of ss_order 0, dimension 1 of ss_order 1
    model = bild_amd.GenericGaussianModel([[(np.append(c * msd, c * 80.0), m, 0), (c * msd, m, 1)] for c, m in ((1.0, 0.05), (1.15, -0.1))])
    x = C.random_traj(rng, 70, (33,))
    got = SC.oracle(model, x, 2, P=4, log_k_prior=SC.log_prior(0, 3), nan='omit')
    want = SC.flat_profile_reference(model, x)
    assert np.min(want['weights']) > 1e-3
    devs = {'log_marginal': abs(got['log_marginal'] - want['log_marginal']) / abs(want['log_marginal']),
            'exp_logl': abs(got['exp_logl'] - want['exp_logl']) / abs(want['exp_logl']),
            'grad': np.max(np.abs(got['grad'] - want['grad'])) / np.max(np.abs(want['grad'])),
            'fisher': np.max(np.abs(got['fisher'] - want['fisher'])) / np.max(np.abs(want['fisher']))}
    print(f"k = 0 identity at T = 70: {devs}, weights {want['weights']}")
    assert max(devs.values()) < 1e-12, devs
    assert np.array_equal(got['k_post'], [1.0, 0.0, 0.0])


@pytest.mark.skipif(not os.environ.get('BILD_DESIGNED_ORACLE'), reason="runs the oracle on every designed case (about 90 s): "
                    "set BILD_DESIGNED_ORACLE=1; the GPU tier asserts the same limit on every answer it uses")
@pytest.mark.parametrize('name,nan,prior', SC.designed_runs())
def test_designed_oracle_answers_take_under_20s(name, nan, prior):
    out = SC.designed_oracle(name, nan, prior)
    seconds = SC.ORACLE_SECONDS[name, nan, prior]
    print(f"{name} {nan} {prior}: {seconds:.1f} s")
    assert seconds < 20.0
    assert np.array_equal(out['logev'], SC.designed_logev(name, nan), equal_nan=True)
    assert np.isnan(out['log_marginal']) == ((name, nan, prior) in SC.NAN_RUNS)
