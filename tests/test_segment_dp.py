"""
The segment recursion without a GPU (bild_amd.exact.exact_sample): the NumPy oracle
tests/segment_oracle.py against the enumeration of every profile (tests/exact_oracle.py on gauss_oracle.logl_tables), the
refusals, and `ExactSamplingResults` on arrays from the oracle.
"""
import warnings

import numpy as np
import pytest
from scipy import stats
from scipy.special import logsumexp

import bild_amd
import exact_oracle as X
import gauss_oracle as G
import segment_cases as C
import segment_oracle as SO
from bild_amd.exact import results_from_arrays
from bild_amd.profiles import states_from_segments

K_MAX = 5
# observed on these cases: logev <= 6e-15, KL <= 3e-14, map_logL <= 4e-15, finite log marginals <= 2e-13; the bound of all
# four is the issue's 1e-12
TOL = 1e-12

# name: (S, T, missing frames, orders (None: ss_order 1 everywhere))
CASES = {
    's2_gapfree': (2, 14, (), None),
    's3_gapfree': (3, 12, (), None),
    's2_leading_gap': (2, 14, (0, 1), None),
    's3_leading_gap': (3, 12, (0, 1), None),
    's2_inner_gap4': (2, 14, (5, 6, 7, 8), None),
    's3_inner_gap4': (3, 12, (4, 5, 6, 7), None),
    's2_order0_inner_gap': (2, 13, (5, 6, 7), [[0, 1], [1, 0]]),
}


def build(name):
    S, T, missing, orders = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    model = C.random_model(rng, S, T + 4, orders=np.ones((S, 2), dtype=int) if orders is None else orders)
    return model, C.random_traj(rng, T, missing)


def enumerated(model, x, k, drop_nan=False):
    """ `exact_oracle.reduce` on the logL of every profile of k switches, and those logLs """
    W, F = C.tables(model, x)
    T, S = len(x), model.nStates
    seg_start, seg_state = X.enumerate_profiles(T, k, model.transitions)
    states = states_from_segments(seg_start, seg_state, T) if len(seg_start) else np.zeros((0, T), dtype=int)
    logL = np.array([G.logl_tables(W, F, st) for st in states])
    n_nan = int(np.isnan(logL).sum())
    if drop_nan:
        keep = ~np.isnan(logL)
        seg_start, seg_state, logL = seg_start[keep], seg_state[keep], logL[keep]
    return X.reduce(logL, seg_start, seg_state, T, S), logL, n_nan


def compare(got, k, want, what=('logev', 'KL', 'map_logL', 'log_post')):
    for name, theirs in (('logev', 'logev'), ('KL', 'KL'), ('map_logL', 'map_logL')):
        if name not in what:
            continue
        a, b = got[name][k], want[theirs]
        if np.isfinite(b):
            assert abs(a - b) < TOL, (name, k, a, b)
        else:
            assert np.array_equal(a, b, equal_nan=True), (name, k, a, b)
    if 'log_post' in what:
        a, b = got['log_post'][k], want['log_post']
        fin = np.isfinite(b)
        assert np.array_equal(fin, np.isfinite(a)), k
        assert np.array_equal(np.isnan(a), np.isnan(b)), k
        if fin.any():
            assert np.max(np.abs(a[fin] - b[fin])) < TOL, (k, np.max(np.abs(a[fin] - b[fin])))


@pytest.mark.parametrize('name', [n for n in CASES if 'order0' not in n])
def test_oracle_against_enumeration(name):
    model, x = build(name)
    W, F = C.tables(model, x)
    got = SO.solve(W, F, model.transitions, K_MAX)
    ties = 0
    for k in range(K_MAX + 1):
        want, logL, n_nan = enumerated(model, x, k)
        assert n_nan == 0 and got['n_profiles'][k] == want['n_profiles'] and got['n_omitted'][k] == 0
        compare(got, k, want)
        # the returned profile attains the maximum and has k switches
        st = got['map_states'][k]
        assert np.count_nonzero(np.diff(st)) == k
        assert abs(G.logl_tables(W, F, st) - np.max(logL)) < TOL
        ties += int(np.sum(logL == np.max(logL)) > 1)
    if 'inner_gap' in name:
        assert ties >= K_MAX            # every switch frame inside the gap gives the same logL: ties at every k >= 1


def test_oracle_nan_windows_both_modes():
    model, x = build('s2_order0_inner_gap')
    W, F = C.tables(model, x)
    prop = SO.solve(W, F, model.transitions, K_MAX, nan='propagate')
    omit = SO.solve(W, F, model.transitions, K_MAX, nan='omit')
    seen = 0
    for k in range(K_MAX + 1):
        want, logL, n_nan = enumerated(model, x, k)
        assert prop['n_profiles'][k] == want['n_profiles'] and prop['n_omitted'][k] == 0
        compare(prop, k, want)          # NaN logev, KL and marginals exactly where the enumeration has a NaN profile
        assert np.isnan(prop['logev'][k]) == (n_nan > 0)
        left, _, _ = enumerated(model, x, k, drop_nan=True)
        assert omit['n_omitted'][k] == n_nan and omit['n_profiles'][k] == left['n_profiles'] == want['n_profiles'] - n_nan
        compare(omit, k, left)
        assert np.isfinite(omit['logev'][k])
        seen += n_nan > 0
    assert seen >= 3        # two switches inside the gap: NaN profiles at every k >= 2


def test_oracle_without_profiles():
    rng = np.random.default_rng(5)
    model = C.random_model(rng, 2, 12, orders=[[1, 1], [1, 1]])
    x = C.random_traj(rng, 4)
    got = SO.solve(*C.tables(model, x), model.transitions, K_MAX)
    for k in (4, 5):        # T - 1 < k
        assert got['logev'][k] == -np.inf and np.isnan(got['KL'][k]) and got['map_states'][k] is None
        assert got['n_profiles'][k] == 0 and np.all(np.isnan(got['log_post'][k]))
    assert np.all(np.isfinite(got['logev'][:4]))
    model.transitions[:] = [[False, True], [False, False]]      # only 0 -> 1: no trace of two switches
    x = C.random_traj(rng, 10)
    got = SO.solve(*C.tables(model, x), model.transitions, 3)
    want, _, _ = enumerated(model, x, 1)
    compare(got, 1, want)
    assert got['n_profiles'] == [2, 9, 0, 0]
    for k in (2, 3):
        assert got['logev'][k] == -np.inf and np.isnan(got['KL'][k]) and got['map_states'][k] is None


def test_refusals_before_device(built_lib):
    rng = np.random.default_rng(1)
    model = C.random_model(rng, 2, 40)
    x = C.random_traj(rng, 30)
    with pytest.raises(TypeError):
        bild_amd.exact_sample(bild_amd.Trajectory(np.zeros((30, 3)), localization_error=[0.1] * 3),
                              bild_amd.MultiStateRouse(20, 1, 5, d=3, localization_error=0.1))
    with pytest.raises(TypeError):
        bild_amd.exact_sample(x, bild_amd.FactorizedModel([stats.maxwell(), stats.maxwell()]))
    with pytest.raises(ValueError, match='k_max = 65'):
        bild_amd.exact_sample(x, model, k_max=65)
    with pytest.raises(ValueError, match='k_max = -1'):
        bild_amd.exact_sample(x, model, k_max=-1)
    with pytest.raises(ValueError, match='k_max = 2.0'):
        bild_amd.exact_sample(x, model, k_max=2.0)
    with pytest.raises(ValueError, match="nan = 'drop'"):
        bild_amd.exact_sample(x, model, nan='drop')
    with pytest.raises(ValueError, match='40 frames'):
        bild_amd.exact_sample([x, C.random_traj(rng, 41)], model)
    model.transitions = np.ones((3, 3), dtype=bool)
    with pytest.raises(ValueError, match='transitions'):
        bild_amd.exact_sample(x, model)
    assert len(model._trajsets) == 0


def oracle_results(name='s2_gapfree', k_max=K_MAX, nan='propagate', dE=0):
    model, x = build(name)
    res, out = C.oracle_arrays(model, x, k_max, nan=nan)
    return results_from_arrays(x, model, dE, model.transitions, res), out, model, x


def test_results_object_mirrors_sampling_results():
    r, out, model, x = oracle_results()
    assert np.array_equal(r.k, np.arange(K_MAX + 1)) and np.array_equal(r.evidence, out['logev'])
    assert np.array_equal(r.evidence_se, np.zeros(K_MAX + 1)) and np.array_equal(r.KL, out['KL'])
    assert r.n_profiles == out['n_profiles'] and r.n_omitted == [0] * (K_MAX + 1)
    assert all(isinstance(n, int) for n in r.n_profiles)
    for k in range(K_MAX + 1):
        assert np.array_equal(r.map_profile(k)[:], out['map_states'][k])
        assert np.array_equal(r.log_marginal_posterior_k(k), out['log_post'][k])
    # best_k: the smallest k within dE of the maximum
    ev = r.evidence
    assert r.best_k() == r.best_k(0) == int(np.argmax(ev))
    for dE in (0.5, 2.0, 10.0, 1e6):
        assert r.best_k(dE) == min(k for k in range(K_MAX + 1) if ev[k] >= ev.max() - dE)
    assert r.best_k(1e6) == 0
    r.dE = 1e6
    assert r.best_k() == 0 and np.array_equal(r.best_profile()[:], out['map_states'][0])
    assert np.array_equal(r.best_profile(0)[:], out['map_states'][int(np.argmax(ev))])
    assert np.array_equal(r.log_marginal_posterior(0), out['log_post'][int(np.argmax(ev))])
    # dE = 'average': SamplingResults' formula written out
    logpost = logsumexp([out['log_post'][k] + ev[k] for k in range(K_MAX + 1) if ev[k] > -np.inf], axis=0)
    want = logpost - logsumexp(logpost, axis=0)
    assert np.array_equal(r.log_marginal_posterior('average'), want)
    assert np.max(np.abs(logsumexp(want, axis=0))) < 1e-12


def test_results_object_nan_and_missing_k():
    r, out, model, x = oracle_results('s2_order0_inner_gap')
    bad = np.isnan(r.evidence)
    assert bad.any() and not bad.all()
    with pytest.warns(RuntimeWarning, match='NaN'):
        k = r.best_k()
    ev = np.where(bad, -np.inf, r.evidence)
    assert k == int(np.argmax(ev)) and not bad[k]
    with pytest.warns(RuntimeWarning):
        avg = r.log_marginal_posterior('average')
    logpost = logsumexp([out['log_post'][k] + ev[k] for k in range(K_MAX + 1) if ev[k] > -np.inf], axis=0)
    assert np.array_equal(avg, logpost - logsumexp(logpost, axis=0))
    r.evidence[:] = np.nan
    with pytest.raises(ValueError, match='NaN'):
        r.best_k()
    # nan='omit': nothing is NaN, no warning
    r, out, _, _ = oracle_results('s2_order0_inner_gap', nan='omit')
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        assert r.best_k() == int(np.argmax(out['logev']))
    assert r.n_omitted == out['n_omitted'] and sum(r.n_omitted) > 0
    assert [a + b for a, b in zip(r.n_profiles, r.n_omitted)] == [X.enumerate_profiles(len(x), k, model.transitions)[0].shape[0]
                                                                  for k in range(K_MAX + 1)]
    # k beyond T - 1: evidence -inf, no profile, never the best
    rng = np.random.default_rng(2)
    model = C.random_model(rng, 2, 12, orders=[[1, 1], [1, 1]])
    x = C.random_traj(rng, 3)
    res, out = C.oracle_arrays(model, x, 4)
    r = results_from_arrays(x, model, 0, model.transitions, res)
    assert np.all(r.evidence[3:] == -np.inf) and r.map_profile(3) is None and r.n_profiles[3:] == [0, 0]
    assert r.best_k(1e9) == 0 and r.best_k() <= 2
