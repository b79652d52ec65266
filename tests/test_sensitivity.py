"""
The NumPy tangent filter (tests/sensitivity_oracle.py) against the filter of tests/kalman_oracle.py, finite differences
and a direct evaluation of the innovations form of the Fisher information; the Rouse derivatives; the host side of
MultiStateRouse.fit.  No device needed.
"""
import numpy as np
import pytest

import kalman_oracle as KO
import sensitivity_oracle as SO

H_REL = 1e-5  # relative step of the central differences


def _logl(arrays, w, err, x, states):
    return float(KO.filter_smoother(arrays, w, err, x, states)['terms'].sum())


def _data(rng, T, d, missing='none'):
    x = rng.standard_normal((T, d)) * 2.0
    if missing == 'first':
        x[0] = np.nan
    elif missing == 'gaps':
        x[5:25] = np.nan
        x[-7:] = np.nan
    elif missing == 'scattered':
        x[rng.random(T) < 0.2] = np.nan
    return x


def _states(rng, T, S, kind):
    if kind == 'constant':
        return np.full(T, S - 1)
    if kind == 'adjacent':
        st = np.zeros(T, dtype=int)
        st[10], st[11], st[12] = 1, S - 1, 0
        st[30:] = 1
        return st
    st = np.zeros(T, dtype=int)
    for t0 in sorted(rng.choice(np.arange(1, T), size=4, replace=False)):
        st[t0:] = rng.integers(S)
    return st


CASES = [
    dict(S=2, d=3, dstar=1, missing='none', kind='switching'),
    dict(S=3, d=2, dstar=2, missing='first', kind='adjacent'),
    dict(S=2, d=3, dstar=2, missing='gaps', kind='constant'),
    dict(S=3, d=1, dstar=1, missing='scattered', kind='switching'),
]


@pytest.mark.parametrize('case', CASES, ids=lambda c: f"S{c['S']}_d{c['d']}_dstar{c['dstar']}_{c['missing']}_{c['kind']}")
def test_tangent_filter_against_kalman_oracle_and_differences(case):
    rng = np.random.default_rng(11)
    S, d, P, N, T = case['S'], case['d'], 3, 6, 60
    arrays_of, derivs = SO.affine_family(rng, N, S, d, P)
    theta = rng.uniform(-0.5, 0.5, P)
    w = rng.standard_normal(N)
    err = np.full(d, 0.4)
    if case['dstar'] == 2:
        err[0] = 0.7
    x = _data(rng, T, d, case['missing'])
    st = _states(rng, T, S, case['kind'])
    ll, g, F = SO.tangent_filter(arrays_of(theta), w, err, x, st, derivs)
    assert abs(ll - _logl(arrays_of(theta), w, err, x, st)) <= 1e-12 * max(1.0, abs(ll))
    # gradient: central differences of the kalman oracle's logL
    for p in range(P):
        h = H_REL
        tp, tm = theta.copy(), theta.copy()
        tp[p] += h
        tm[p] -= h
        fd = (_logl(arrays_of(tp), w, err, x, st) - _logl(arrays_of(tm), w, err, x, st)) / (2 * h)
        assert abs(g[p] - fd) <= 1e-6 * max(1.0, abs(fd)), (p, g[p], fd)
    # Fisher: the innovations form evaluated directly on differences of the oracle's (e, S)
    de, dS = [], []
    for p in range(P):
        tp, tm = theta.copy(), theta.copy()
        tp[p] += H_REL
        tm[p] -= H_REL
        ep, Sp = SO.innovations(arrays_of(tp), w, err, x, st)
        em, Sm = SO.innovations(arrays_of(tm), w, err, x, st)
        de.append((ep - em) / (2 * H_REL))
        dS.append((Sp - Sm) / (2 * H_REL))
    _, S_ = SO.innovations(arrays_of(theta), w, err, x, st)
    obs = ~np.isnan(de[0])
    want = np.array([[np.sum(dS[a][obs] * dS[b][obs] / (2 * S_[obs] ** 2) + de[a][obs] * de[b][obs] / S_[obs])
                      for b in range(P)] for a in range(P)])
    assert np.allclose(F, want, rtol=1e-6, atol=1e-9 * np.max(np.abs(want)))
    assert np.all(np.linalg.eigvalsh(F) >= -1e-10 * np.max(np.abs(F)))


def test_localization_error_derivative():
    rng = np.random.default_rng(3)
    arrays_of, _ = SO.affine_family(rng, 5, 2, 3, 1)
    a = arrays_of(np.zeros(1))
    w = rng.standard_normal(5)
    x = _data(rng, 50, 3, 'scattered')
    st = _states(rng, 50, 2, 'switching')
    sigma = 0.3
    ll, g, F = SO.tangent_filter(a, w, np.full(3, sigma), x, st, derivs=None, ds2=np.full((1, 3), 2 * sigma))
    fd = (_logl(a, w, np.full(3, sigma * (1 + H_REL)), x, st) - _logl(a, w, np.full(3, sigma * (1 - H_REL)), x, st)) \
        / (2 * sigma * H_REL)
    assert abs(g[0] - fd) <= 1e-6 * max(1.0, abs(fd))
    assert F[0, 0] > 0


def test_rouse_family_gradient():
    """ D and k of a two-state Rouse model (end-to-end measurement, loop between the ends) """
    from helpers import end2end
    rng = np.random.default_rng(5)
    N, d, T = 8, 2, 40
    arrays_of, derivs_of = SO.rouse_family(N, [None, (0, -1)], d=d)
    w = end2end(N)
    D, k, err = 1.3, 2.5, np.full(d, 0.2)
    x = rng.standard_normal((T, d))
    st = _states(rng, T, 2, 'switching')
    ll, g, F = SO.tangent_filter(arrays_of(D, k), w, err, x, st, derivs_of(D, k))
    for p, (dD, dk) in enumerate([(D * H_REL, 0), (0, k * H_REL)]):
        fd = (_logl(arrays_of(D + dD, k + dk), w, err, x, st) - _logl(arrays_of(D - dD, k - dk), w, err, x, st)) \
            / (2 * (dD + dk))
        assert abs(g[p] - fd) <= 1e-6 * max(1.0, abs(fd)), (p, g[p], fd)


@pytest.mark.parametrize('k', [1e-4, 0.3, 5.0, 500.0])
@pytest.mark.parametrize('param', ['D', 'k'])
def test_rouse_dynamics_derivatives(param, k):
    from bild_amd import rouse
    D, N, h = 1.7, 20, 1e-4

    def arrs(D, k):
        m = rouse.Model(N, D, k, 3, add_bonds=[(0, -1)])
        m.check_dynamics()
        M0, C0 = m.steady_state()
        return {'dB': m._dynamics['B'], 'dSig': m._dynamics['Sig'], 'dC0': C0, 'dG': m._dynamics['G'], 'dM0': M0}

    x = D if param == 'D' else k
    plus = arrs(D * (1 + h), k) if param == 'D' else arrs(D, k * (1 + h))
    minus = arrs(D * (1 - h), k) if param == 'D' else arrs(D, k * (1 - h))
    got = rouse.Model(N, D, k, 3, add_bonds=[(0, -1)]).dynamics_derivatives(param)
    for key in plus:
        fd = (plus[key] - minus[key]) / (2 * x * h)
        # relative 1e-7 of the derivative, with a floor at the rounding of the array itself over the step
        floor = 1e-14 * max(np.max(np.abs(plus[key])), 1e-300) / (x * h)
        assert np.max(np.abs(got[key] - fd)) <= 1e-7 * np.max(np.abs(got[key])) + floor, (key, param, k)


def test_rouse_derivative_series_branch():
    """ the small-a series of the k-derivatives meets the closed form at the switch point """
    from bild_amd.rouse import _two_exp_plus, _h_over_a
    u = np.array([0.5 - 1e-12, 0.5 + 1e-12])
    assert abs(_two_exp_plus(u)[0] - _two_exp_plus(u)[1]) < 1e-11
    assert abs(_h_over_a(u)[0] - _h_over_a(u)[1]) < 1e-11
    assert abs(_two_exp_plus(np.array([1e-8]))[0] + 1e-8) < 1e-15   # -u + O(u^2)


def test_log_chain_rule():
    from bild_amd.models import _log_chain_rule
    rng = np.random.default_rng(0)
    g = rng.standard_normal((4, 3))
    F = rng.standard_normal((4, 3, 3))
    th = rng.uniform(0.5, 2, (4, 3))
    g2, F2 = _log_chain_rule(g, F, th)
    assert np.allclose(g2, g * th)
    for r in range(4):
        assert np.allclose(F2[r], np.diag(th[r]) @ F[r] @ np.diag(th[r]))
    # and it is the derivative in log theta: d/d log sigma of the oracle's logL
    arrays_of, _ = SO.affine_family(rng, 4, 2, 1, 1)
    a = arrays_of(np.zeros(1))
    w = rng.standard_normal(4)
    x = rng.standard_normal((30, 1))
    st = np.zeros(30, dtype=int)
    sigma = 0.5
    _, g, _ = SO.tangent_filter(a, w, [sigma], x, st, ds2=[[2 * sigma]])
    gl, _ = _log_chain_rule(g[None, :], None, np.array([[sigma]]))
    fd = (_logl(a, w, [sigma * np.exp(1e-6)], x, st) - _logl(a, w, [sigma * np.exp(-1e-6)], x, st)) / 2e-6
    assert abs(gl[0, 0] - fd) <= 1e-6 * max(1.0, abs(fd))


def test_fit_argument_checks():
    import bild_amd
    from bild_amd.models import _fit_profiles, _newton_decrement, _damped_step
    m = bild_amd.MultiStateRouse(10, 1.0, 2.0, d=3, localization_error=0.1)
    trajs = [np.zeros((20, 3)), np.zeros((15, 3))]
    with pytest.raises(ValueError, match='unknown parameter'):
        m.fit(trajs, 0, params=('D', 'N'))
    with pytest.raises(ValueError, match='repeat'):
        m.fit(trajs, 0, params=('D', 'D'))
    with pytest.raises(ValueError, match='out of range'):
        m.fit(trajs, 5)
    with pytest.raises(ValueError, match='profiles for'):
        m.fit(trajs, [np.zeros(20, dtype=int)])
    with pytest.raises(ValueError, match='frames'):
        m.fit(trajs, [np.zeros(20, dtype=int), np.zeros(20, dtype=int)])
    with pytest.raises(ValueError, match='not fitted'):
        m.fit(trajs, 0, params=('D',), start={'k': 2.0})
    with pytest.raises(ValueError, match='positive'):
        m.fit(trajs, 0, params=('D',), start={'D': -1.0})
    with pytest.raises(ValueError, match='tol'):
        m.fit(trajs, 0, tol=0)
    a = m.arrays()
    ma = bild_amd.MultiStateRouse.from_arrays(**a, measurement=m.measurement, localization_error=0.1)
    with pytest.raises(ValueError, match='no D or k'):
        ma.fit(trajs, 0, params=('D',))
    with pytest.raises(ValueError, match='no D or k'):
        ma.logL_sensitivities((np.zeros((1, 1)), np.zeros((1, 1))), trajs[:1], params=('k',))
    with pytest.raises(ValueError, match='log=False'):
        ma.logL_sensitivities((np.zeros((1, 1)), np.zeros((1, 1))), trajs[:1], derivatives={'dB': np.zeros((1, 2, 10, 10))})
    with pytest.raises(ValueError, match='one sigma'):
        bild_amd.MultiStateRouse(10, 1.0, 2.0, d=3, localization_error=[0.1, 0.2, 0.1]).fit(trajs, 0)
    # profiles: constant, per trajectory, run-length encoded
    ss, st = _fit_profiles(1, [20, 15], 2)
    assert ss.tolist() == [[0], [0]] and st.tolist() == [[1], [1]]
    ss, st = _fit_profiles([np.r_[np.zeros(10, int), np.ones(10, int)], np.ones(15, int)], [20, 15], 2)
    assert ss.tolist() == [[0, 10], [0, 15]] and st.tolist() == [[0, 1], [1, 0]]
    # the scoring step and the decrement
    F = np.array([[2.0, 0.5], [0.5, 1.0]])
    g = np.array([1.0, -1.0])
    assert np.allclose(_damped_step(g, F, 0.0), np.linalg.solve(F, g))
    assert abs(_newton_decrement(g, F) - 0.5 * g @ np.linalg.solve(F, g)) < 1e-14


def test_with_parameters_keeps_structure():
    import bild_amd
    m = bild_amd.MultiStateRouse(12, 1.0, 2.0, d=2, looppositions=(None, (2, -3), [(0, -1), (3, 5)]), localization_error=0.2)
    m2 = m.with_parameters(D=2.0, k=3.0, localization_error=0.05)
    ref = bild_amd.MultiStateRouse(12, 2.0, 3.0, d=2, looppositions=(None, (2, -3), [(0, -1), (3, 5)]), localization_error=0.05)
    for key in ('B', 'Sig', 'C0'):
        assert np.array_equal(m2.arrays()[key], ref.arrays()[key])
    assert np.array_equal(m2.localization_error, [0.05, 0.05])
    assert np.array_equal(m.with_parameters(D=3.0).localization_error, m.localization_error)
    assert m2.nStates == 3 and m2.d == 2
