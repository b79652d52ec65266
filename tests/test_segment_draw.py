"""
The exact posterior draws without a GPU (bild_amd.exact.exact_draw): the NumPy oracle
tests/segment_draw_oracle.py against the enumeration of every profile (tests/exact_oracle.py on gauss_oracle tables) on the
cases of tests/test_segment_dp.py, and the refusals of `exact_draw`, which are raised before any device work.

The count bound: of N independent draws, a profile of posterior p is drawn Binomial(N, p) times, and
|count - N p| <= 5.5 sqrt(N p (1 - p)) + 3 is asked of every profile.  5.5 standard deviations leave a two-sided normal tail of
4e-8 per comparison, and the + 3 covers the Poisson regime of small N p (P(Poisson(1) >= 10) ~ 1e-7); with under 2e4
comparisons a correct sampler fails with probability below 1e-3, and with fixed seeds not at all once it has passed.
"""
import numpy as np
import pytest
from scipy.special import logsumexp

import bild_amd
import exact_oracle as X
import segment_cases as C
import segment_draw_oracle as DO
import segment_oracle as SO
from bild_amd.exact import results_from_arrays
from test_segment_dp import CASES, build

N_DRAWS = 20000


def count_bound(N, p):
    return 5.5 * np.sqrt(N * p * (1 - p)) + 3


def enumeration_posterior(W, F, T, k, transitions):
    """ (seg_start, seg_state, p): every profile of k switches and its posterior (0 for a NaN profile) """
    seg_start, seg_state = X.enumerate_profiles(T, k, transitions)
    logL = C.table_logl(W, F, seg_start, seg_state, T)
    bad = np.isnan(logL)
    logL = np.where(bad, -np.inf, logL)
    with np.errstate(under='ignore'):
        p = np.exp(logL - logsumexp(logL))
    return seg_start, seg_state, p, bad


def profile_counts(seg_start, seg_state, got_start, got_state, k):
    """ how often each enumerated profile occurs among the drawn rows """
    index = {tuple(a) + tuple(b): i for i, (a, b) in enumerate(zip(seg_start.tolist(), seg_state.tolist()))}
    counts = np.zeros(len(seg_start), dtype=np.int64)
    for a, b in zip(got_start[:, :k + 1].tolist(), got_state[:, :k + 1].tolist()):
        counts[index[tuple(a) + tuple(b)]] += 1
    return counts


def check_counts(counts, p, N):
    assert counts.sum() == N
    excess = np.abs(counts - N * p) - count_bound(N, p)
    assert np.all(excess <= 0), (int(np.argmax(excess)), float(np.max(excess)))
    return float(np.max(np.abs(counts - N * p) / count_bound(N, p)))


@pytest.mark.parametrize('name', list(CASES))
def test_oracle_draws_against_enumeration(name):
    model, x = build(name)
    W, F = C.tables(model, x)
    T, k_max = len(x), 3
    G = SO.backward(W, model.transitions, k_max)
    rng = np.random.default_rng(sum(map(ord, name)) + 1)
    nan_profiles = 0
    for k in range(k_max + 1):
        seg_start, seg_state, p, bad = enumeration_posterior(W, F, T, k, model.transitions)
        u = rng.random((N_DRAWS, 2 * k_max))
        a, b, fragile, consumed = DO.draws(W, F, G, model.transitions, np.full(N_DRAWS, k), u)
        assert np.all(a[:, 0] == 0) and np.all(a[:, k + 1:] == T) and np.all(b[:, k + 1:] == 0)
        assert np.all(np.diff(a[:, :k + 1], axis=1) > 0) and np.all(a[:, :k + 1] < T)
        # every draw consumed max(1, 2k) uniforms, a pick with one candidate included
        assert np.array_equal(consumed[:, :max(1, 2 * k)], u[:, :max(1, 2 * k)]) and np.all(consumed[:, max(1, 2 * k):] == 0)
        counts = profile_counts(seg_start, seg_state, a, b, k)
        assert np.all(counts[bad] == 0)         # a NaN profile is never drawn
        check_counts(counts, p, N_DRAWS)
        nan_profiles += int(bad.sum())
    assert (nan_profiles > 0) == ('order0' in name)


def test_oracle_k_without_profile():
    rng = np.random.default_rng(5)
    model = C.random_model(rng, 2, 12, orders=[[1, 1], [1, 1]])
    x = C.random_traj(rng, 4)
    W, F = C.tables(model, x)
    G = SO.backward(W, model.transitions, 5)
    u = rng.random((6, 10))
    a, b, fragile, consumed = DO.draws(W, F, G, model.transitions, np.arange(6), u)
    for k in range(4):
        assert a[k, 0] == 0 and np.all(np.diff(a[k, :k + 1]) > 0) and np.all(a[k, k + 1:] == 4)
    assert np.all(a[4:] == -1) and np.all(b[4:] == -1) and np.all(consumed[4:] == 0)     # T - 1 < k
    assert np.array_equal(a[3, :4], [0, 1, 2, 3])
    model.transitions[:] = [[False, True], [False, False]]      # only 0 -> 1: no trace of two switches
    x = C.random_traj(rng, 10)
    W, F = C.tables(model, x)
    G = SO.backward(W, model.transitions, 3)
    a, b, _, _ = DO.draws(W, F, G, model.transitions, np.array([0, 1, 1, 2, 3]), rng.random((5, 6)))
    assert np.all(a[3:] == -1) and np.all(a[:3, 0] == 0)
    assert np.array_equal(b[1, :2], [0, 1]) and np.array_equal(b[2, :2], [0, 1])


def test_pick_rules():
    # zero weights are never returned, not even at u = 0 or when rounding carries u * total past the last positive weight
    logw = np.array([-np.inf, np.log(0.25), -np.inf, np.log(0.75), -np.inf])
    assert DO.pick(logw, 0.0) == (1, False)
    assert DO.pick(logw, 0.2499) == (1, False) and DO.pick(logw, 0.25) == (3, True) and DO.pick(logw, 0.25 + 1e-10) == (3, True)
    assert DO.pick(logw, np.nextafter(1.0, 0)) == (3, False)
    assert DO.pick([np.nan, -np.inf], 0.5) == (-1, False)
    assert DO.pick([np.nan, 0.0, -np.inf], 0.999) == (1, False)


def oracle_results(name, k_max=5, nan='propagate'):
    model, x = build(name)
    res, out = C.oracle_arrays(model, x, k_max, nan=nan, with_marginals=False)
    return results_from_arrays(x, model, 0, model.transitions, res, nan=nan), model, x


def test_results_remember_nan_mode():
    r, model, x = oracle_results('s2_gapfree')
    assert r.nan == 'propagate'
    res, _ = C.oracle_arrays(model, x, 2, with_marginals=False)
    assert results_from_arrays(x, model, 0, model.transitions, res).nan == 'propagate'      # the keyword's default
    r, _, _ = oracle_results('s2_order0_inner_gap', nan='omit')
    assert r.nan == 'omit'


def test_exact_draw_refusals_before_device():
    r, model, x = oracle_results('s2_gapfree')
    for bad_k in (6, -1):
        with pytest.raises(ValueError, match=f'k = {bad_k}'):
            bild_amd.exact_draw(r, 10, k=bad_k)
    with pytest.raises(ValueError, match='k = 2.0'):
        bild_amd.exact_draw(r, 10, k=2.0)
    with pytest.raises(ValueError, match="k = 'mean'"):
        r.draw(10, k='mean')
    with pytest.raises(ValueError, match='shape'):
        r.draw(10, k=np.zeros(9, dtype=int))
    with pytest.raises(ValueError, match='k = 7'):
        r.draw(3, k=np.array([0, 7, 1]))
    for bad_n in (-1, 2.5, True):
        with pytest.raises(ValueError, match='n = '):
            r.draw(bad_n)
    with pytest.raises(ValueError, match='uniforms has shape'):
        r.draw(4, k=2, uniforms=np.zeros((4, 9)))
    u = np.full((4, 10), 0.5)
    for bad_u in (1.0, np.nan, -1e-9):
        u[2, 3] = bad_u
        with pytest.raises(ValueError, match=r'\[0, 1\)'):
            r.draw(4, k=2, uniforms=u)
    with pytest.raises(TypeError):
        bild_amd.exact_draw([r, 'x'], 4)
    other, _, _ = oracle_results('s2_leading_gap')
    with pytest.raises(ValueError, match='one model'):
        bild_amd.exact_draw([r, other], 4)
    short, _, _ = oracle_results('s2_gapfree', k_max=3)
    short.model = model
    with pytest.raises(ValueError, match='one k_max'):
        bild_amd.exact_draw([r, short], 4)
    assert bild_amd.exact_draw([], 4) == []
    # a k whose evidence is -inf (T - 1 < k) or NaN (nan='propagate' with a NaN profile)
    rng = np.random.default_rng(2)
    model3 = C.random_model(rng, 2, 12, orders=[[1, 1], [1, 1]])
    x3 = C.random_traj(rng, 3)
    res, _ = C.oracle_arrays(model3, x3, 4, with_marginals=False)
    r3 = results_from_arrays(x3, model3, 0, model3.transitions, res)
    with pytest.raises(ValueError, match='-inf'):
        r3.draw(5, k=3)
    rn, modeln, _ = oracle_results('s2_order0_inner_gap')
    assert np.isnan(rn.evidence[2])
    with pytest.raises(ValueError, match="nan='omit'"):
        rn.draw(5, k=2)
    with pytest.raises(ValueError, match="nan='omit'"):
        rn.draw(3, k=np.array([0, 1, 3]))
    # n = 0: empty draws, still no device work
    d = r.draw(0)
    assert isinstance(d, bild_amd.ExactDraws) and len(d) == 0 and d.seg_start.shape == (0, 6) and d.uniforms.shape == (0, 10)
    assert d.states().shape == (0, len(x)) and d.profiles() == [] and d.n_switches is d.k
    for m in (model, model3, modeln):
        assert len(m._trajsets) == 0
