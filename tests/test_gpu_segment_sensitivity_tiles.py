"""
The evidence gradient on the GPU beyond one 64-frame tile of `segsens_weight_kernel` (csrc/gauss_segsens.hip and .cpp, DESIGN.md
section 20), against the NumPy oracle under the bar of tests/test_gpu_segment_sensitivity.py: the designed cases of
tests/segment_sensitivity_cases.py (tile seams, merged tau rows over a seam, d = 1 and 3, four states, jobs of more than 256
rows), priors over k with zeros and per trajectory, a ragged batch in one and in six chunks, and k = 0 alone at the length where
the solve kernel's dynamic LDS passes 64 KB, against the flat profiles of tests/gauss_sensitivity_oracle.py.  `-s` prints the
worst deviation per case and the oracle's and the device's wall times.
"""
import time

import numpy as np
import pytest

import bild_amd
import segment_cases as C
import segment_sensitivity_cases as SC
from test_gpu_segment_sensitivity import FIELDS, TOL, check_against_oracle, rel

pytestmark = pytest.mark.gpu

ORACLE_LIMIT = 20.0     # seconds: no designed case's oracle answer may take longer
ZEROS_PRIOR = (0.1, 0.4, 0.0, 0.3, 0.0, 0.0, 0.2)       # k_max = 6: non-uniform, with zeros in the middle


def run_designed(name, nan, prior):
    model, x, k_max = SC.designed(name)
    want = SC.designed_oracle(name, nan, prior)
    seconds = SC.ORACLE_SECONDS[name, nan, prior]
    assert seconds < ORACLE_LIMIT, (name, nan, prior, seconds)
    label = f"{name}{'' if prior is None else f' prior {prior}'}"
    t0 = time.perf_counter()
    worst = check_against_oracle(model, x, k_max, nan, k_prior=list(prior) if isinstance(prior, tuple) else prior, label=label, want=want)
    print(f"{label} nan={nan}: worst deviation {worst:.1e}; oracle {seconds:.1f} s, device side (P = 0 ... 4 and exact_sample) "
          f"{time.perf_counter() - t0:.1f} s")
    return want


@pytest.mark.parametrize('name', list(SC.DESIGNED))
def test_designed_case(name):
    for _, nan, prior in SC.designed_runs([name]):
        want = run_designed(name, nan, prior)
        assert np.isnan(want['log_marginal']) == ((name, nan, prior) in SC.NAN_RUNS)
    if name == 'order0_gap_T130':       # NaN from k = 2 on, and finite below, on the device as well
        model, x, k_max = SC.designed(name)
        r = bild_amd.exact_sensitivities(x, model, k_max=k_max)
        assert np.all(np.isfinite(r.logev[0, :2])) and np.all(np.isnan(r.logev[0, 2:]))


@pytest.mark.parametrize('name', ['edge_T65', 'straddle_T129'])
def test_designed_case_priors(name):
    assert SC.DESIGNED[name][3] + 1 == len(ZEROS_PRIOR)
    for nan in sorted({nan for _, nan, _ in SC.designed_runs([name])}):
        run_designed(name, nan, ZEROS_PRIOR)
        run_designed(name, nan, 1)


BATCH_K_MAX = 4
# one row per trajectory of `batch_case`: a zero in the middle, two short ones, a single k, all different
BATCH_PRIOR = np.array([[0.3, 0.0, 0.2, 0.1, 0.4],
                        [0.5, 0.5, 0.0, 0.0, 0.0],
                        [0.2, 0.8, 0.0, 0.0, 0.0],
                        [0.0, 0.0, 0.0, 1.0, 0.0],
                        [1.0, 2.0, 3.0, 4.0, 5.0],
                        [0.4, 0.0, 0.0, 0.6, 0.0]])


def batch_case():
    model = SC.designed_model('edge')
    rng = np.random.default_rng(12)
    short = [C.random_traj(rng, 1), C.random_traj(rng, 2)]
    xs = [SC.designed('edge_T65')[1], *short, SC.designed('edge_T129')[1], SC.designed('edge_T64')[1], SC.designed('edge_T128')[1]]
    return model, xs


def test_ragged_batch_with_a_prior_per_trajectory():
    model, xs = batch_case()
    K = BATCH_K_MAX + 1
    dmsd, dinf, dmean = SC.derivatives(model, 4)
    kw = dict(dmsd=dmsd, dmsd_inf=dinf, dmean=dmean, k_max=BATCH_K_MAX, k_prior=BATCH_PRIOR)
    a = bild_amd.exact_sensitivities(xs, model, **kw)
    # T = 129, K = 5, S = 2: a trajectory's tables take 293 KB (per_traj in gauss_segsens.cpp), so 256 KB hold one a chunk
    small = bild_amd.exact_sensitivities(xs, model, scratch_bytes=1 << 18, **kw)
    for f in FIELDS:
        assert np.array_equal(getattr(a, f), getattr(small, f), equal_nan=True), f
    for i, x in enumerate(xs):
        t0 = time.perf_counter()
        want = SC.oracle(model, x, BATCH_K_MAX, P=4, log_k_prior=SC.log_prior(BATCH_PRIOR[i], K))
        seconds = time.perf_counter() - t0
        devs = {'log_marginal': rel(a.log_marginal[i], want['log_marginal']), 'k_posterior': rel(a.k_posterior[i], want['k_post']),
                'expected_logL': rel(a.expected_logL[i], want['exp_logl']), 'grad': rel(a.grad[i], want['grad']),
                'fisher': rel(a.fisher[i], want['fisher'])}
        print(f"trajectory {i} (T = {len(x)}), prior {BATCH_PRIOR[i]}: " + ', '.join(f"{k} {v:.1e}" for k, v in devs.items())
              + f"; oracle {seconds:.1f} s")
        assert np.all(np.isfinite(a.grad[i])) and np.all(np.isfinite(a.fisher[i]))
        for name, v in devs.items():
            assert v < TOL, (i, name, v)
        assert np.all(a.k_posterior[i][BATCH_PRIOR[i] == 0] == 0)
        fin = np.isfinite(want['logev'])
        assert np.array_equal(np.isfinite(a.logev[i]), fin) and rel(a.logev[i][fin], want['logev'][fin]) < TOL


# ---------------------------------------------------------------- k = 0 alone, at length

def rel1(got, want):
    """ tests/test_gpu_gauss_sensitivity.py's measure: relative to the largest entry, or to 1 where that is smaller """
    want = np.asarray(want)
    return float(np.max(np.abs(np.asarray(got) - want), initial=0.0)) / max(1.0, float(np.max(np.abs(want))))


def check_flat_profiles(T):
    """
    All prior weight on k = 0 at length T, P = 4 with dmean: against the softmax-weighted flat profiles
    (`segment_sensitivity_cases.flat_profile_reference`), and k_max = 0 against k_max = 2.  Returns the deviations and the times.
    """
    model, x = SC.flat_long_case(T)
    dmsd, dinf, dmean = SC.derivatives(model, 4)
    assert np.any(dmean != 0)
    kw = dict(dmsd=dmsd, dmsd_inf=dinf, dmean=dmean, k_prior=0)
    t0 = time.perf_counter()
    r = bild_amd.exact_sensitivities(x, model, k_max=2, **kw)
    t1 = time.perf_counter()
    r0 = bild_amd.exact_sensitivities(x, model, k_max=0, **kw)
    t2 = time.perf_counter()
    want = SC.flat_profile_reference(model, x)
    t3 = time.perf_counter()
    devs = {'log_marginal': rel1(r.log_marginal[0], want['log_marginal']), 'expected_logL': rel1(r.expected_logL[0], want['exp_logl']),
            'grad': rel1(r.grad[0], want['grad']), 'fisher': rel1(r.fisher[0], want['fisher']),
            'grad k_max=0': rel1(r0.grad[0], r.grad[0]), 'fisher k_max=0': rel1(r0.fisher[0], r.fisher[0])}
    print(f"T = {T}: " + ', '.join(f"{k} {v:.1e}" for k, v in devs.items()) + f"; weights of the flat profiles {want['weights']}; "
          f"device k_max = 2 {t1 - t0:.1f} s, k_max = 0 {t2 - t1:.1f} s, flat oracle {t3 - t2:.1f} s")
    assert np.array_equal(r.k_posterior[0], [1.0, 0.0, 0.0]) and r.log_marginal[0] == r.logev[0, 0]
    assert np.min(want['weights']) > 1e-3       # both flat profiles count
    assert devs['log_marginal'] < 1e-10 and devs['expected_logL'] < 1e-10
    assert devs['grad'] < 1e-8 and devs['fisher'] < 1e-8
    assert devs['grad k_max=0'] < 1e-8 and devs['fisher k_max=0'] < 1e-8
    assert rel1(r0.log_marginal[0], want['log_marginal']) < 1e-10 and rel1(r0.expected_logL[0], want['exp_logl']) < 1e-10
    return devs


def test_flat_profiles_beyond_64_KB_of_LDS():
    """ T = 1376: the smallest round length at which the solve kernel's (2 + 4) n 8 bytes of dynamic LDS exceed 64 KB """
    assert (2 + 4) * 1376 * 8 > 64 * 1024 >= (2 + 4) * 1365 * 8
    check_flat_profiles(1376)
