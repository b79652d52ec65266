"""
The exact switch counts and first-contact times under a dwell-time prior without a GPU
(bild_amd.exact.exact_dwell_switch_counts, exact_dwell_first_contact): the NumPy oracle
tests/dwell_event_oracle.py against the enumeration of every profile on the cases of tests/test_dwell.py, its identities
against `dwell_oracle.solve`, `DwellSwitchCounts`' derived distributions, `ExactDwellDraws.first_contact` on hand-made states,
and the argument errors.
"""
import numpy as np
import pytest

import bild_amd
import dwell_cases as DC
import dwell_event_oracle as DE
import dwell_oracle as DO
import segment_cases as C
import test_dwell as TD
from bild_amd import _lib

# the issue's bound against enumeration, the siblings' CPU bound
TOL = 1e-12

TARGETS = {2: ((1,),), 3: ((2,), (0, 2))}


def close_logs(got, want, what):
    """ every finite log within TOL, -inf exactly; returns the worst deviation """
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    assert got.shape == want.shape, what
    assert not np.any(np.isnan(got)) and not np.any(np.isnan(want)), what
    assert np.array_equal(got == -np.inf, want == -np.inf), what
    fin = want > -np.inf
    worst = float(np.max(np.abs(got[fin] - want[fin]), initial=0.0))
    assert worst < TOL, (what, worst)
    return worst


def compare(got, want):
    assert abs(got['logev'] - want['logev']) < TOL
    worst = {name: close_logs(got[name], want[name], name) for name in ('log_count', 'log_first', 'log_never')}
    assert got['log_tail'] == -np.inf
    print('worst deviation of a log from the enumeration: ' + ', '.join(f"{k} {v:.1e}" for k, v in worst.items()))


def result(answer, model, prior, x):
    """ the oracle's counts as the `DwellSwitchCounts` that the device call would return """
    return bild_amd.DwellSwitchCounts(traj=x, model=model, prior=prior, nan='propagate', log_evidence=answer['logev'],
                                      n_nan_windows=answer['n_nan_windows'], log_count=answer['log_count'], log_tail=answer['log_tail'])


def identities(got, ref, target, S, T, model, prior, x):
    """ the identities of section 27 against `dwell_oracle.solve`'s jumps and marginals """
    count, post = np.exp(got['log_count']), np.exp(ref['log_post'])
    inside = np.isin(np.arange(S), target)
    r = result(got, model, prior, x)
    devs = {'sum pmf = 1': abs(r.pmf().sum() - 1),
            'mean = sum exp_jumps': abs(r.mean() - ref['exp_jumps'].sum()),
            'sum_n count = last marginal': np.max(np.abs(count.sum(axis=0) - post[:, T - 1])),
            'sum first + never = 1': abs(np.exp(got['log_first']).sum() + np.exp(got['log_never']) - 1),
            'first[0] = first marginal in G': abs(np.exp(got['log_first'][0]) - post[inside, 0].sum())}
    if S == 2 and tuple(target) == (1,):
        devs['never = count[0][0]'] = abs(np.exp(got['log_never']) - count[0, 0])
    print(', '.join(f"{k}: {v:.1e}" for k, v in devs.items()))
    for name, v in devs.items():
        assert v < TOL, (name, v)


@pytest.mark.parametrize('kind', ['markov', 'nongeometric', 'minlength'])
@pytest.mark.parametrize('name', [n for n in TD.CASES if 'order0' not in n])
def test_oracle_against_enumeration_and_identities(name, kind):
    model, x, prior = TD.build(name, kind)
    S, T = TD.CASES[name][:2]
    W, F = C.tables(model, x)
    ref = DO.solve(W, F, prior)
    for target in TARGETS[S]:
        got, want = DE.solve(W, F, prior, target=target), DE.enumerate_all(W, F, prior, target=target)
        assert got['n_nan_windows'] == 0 and want['n_nan'] == 0 and got['log_count'].shape == (T, S)
        assert abs(got['logev'] - ref['logev']) < TOL
        compare(got, want)
        identities(got, ref, target, S, T, model, prior, x)
    if kind == 'minlength':
        assert np.all(got['log_count'][(T + 1) // 2:] == -np.inf)      # completed segments have two frames at least
    if S == 2:
        r = result(got, model, prior, x)
        for q in range(2):
            pmf = r.segment_count_pmf(q)
            assert pmf.shape == ((T + 1) // 2 + 1,) == want['segments'][q].shape
            assert np.max(np.abs(pmf - want['segments'][q])) < TOL
    else:
        with pytest.raises(NotImplementedError, match='exact_dwell_draw'):
            result(got, model, prior, x).segment_count_pmf(0)


@pytest.mark.parametrize('kind', ['markov', 'minlength'])
@pytest.mark.parametrize('nan', ['propagate', 'omit'])
def test_oracle_nan_windows_against_enumeration(nan, kind):
    model, x, prior = TD.build('s2_order0_inner_gap', kind)
    W, F = C.tables(model, x)
    got, want = DE.solve(W, F, prior, target=(1,), nan=nan), DE.enumerate_all(W, F, prior, target=(1,), nan=nan)
    ref = DO.solve(W, F, prior, nan=nan)
    assert got['n_nan_windows'] == ref['n_nan_windows'] > 0 and want['n_nan'] > 0
    if nan == 'propagate':
        assert np.isnan(got['logev']) and np.isnan(got['log_tail']) and np.isnan(got['log_never']) and np.isnan(want['log_never'])
        for name in ('log_count', 'log_first'):
            assert np.all(np.isnan(got[name])) and np.all(np.isnan(want[name]))
        return
    compare(got, want)
    identities(got, ref, (1,), 2, len(x), model, prior, x)


def test_truncated_k_max_and_tail():
    model, x, prior = TD.build('s2_inner_gap', 'markov')
    W, F = C.tables(model, x)
    full, cut = DE.solve(W, F, prior), DE.solve(W, F, prior, k_max=3)
    assert cut['log_count'].shape == (4, 2) and np.array_equal(cut['log_count'], full['log_count'][:4])
    # a difference from 1 of a sum of 8 terms, against a sum of 16: a few roundings of numbers below 1, 2e-16 each
    assert abs(np.exp(cut['log_tail']) - np.exp(full['log_count'][4:]).sum()) < 1e-14
    r = result(cut, model, prior, x)
    assert abs(r.pmf().sum() + np.exp(r.log_tail) - 1) < 1e-14 and r.segment_count_pmf(0).shape == (3,)
    assert abs(r.segment_count_pmf(0).sum() - r.pmf().sum()) < 1e-14
    with pytest.raises(ValueError):
        r.segment_count_pmf(2)


def test_first_contact_of_draws_on_hand_made_states():
    states = np.array([[0, 0, 1, 1, 0, 255], [1, 0, 0, 0, 0, 255], [0, 0, 0, 0, 0, 255], [0, 2, 2, 1, 0, 255], [2, 1, 1, 1, 1, 255]],
                      dtype=np.uint8)
    n = len(states)
    draws = bild_amd.ExactDwellDraws(5, states, np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n), None)
    for target, want in ((1, [2, 0, -1, 3, 1]), ([1], [2, 0, -1, 3, 1]), ((1, 2), [2, 0, -1, 1, 0]), ({2}, [-1, -1, -1, 1, 0]),
                         (0, [0, 1, 0, 0, -1]), (3, [-1] * 5), (255, [-1] * 5)):      # (the padding behind T is never a contact)
        got = draws.first_contact(target)
        assert got.dtype == np.int64 and got.tolist() == want, target
    empty = bild_amd.ExactDwellDraws(5, np.zeros((0, 5), dtype=np.uint8), np.zeros(0), np.zeros(0), np.zeros(0), np.zeros(0), None)
    assert empty.first_contact(1).shape == (0,)


def test_refusals_come_before_any_upload(monkeypatch):
    def no_upload(*a, **k):
        raise AssertionError("a trajectory set was made")
    monkeypatch.setattr(_lib, 'GaussTrajSetHandle', no_upload)
    rng = np.random.default_rng(3)
    model = C.random_model(rng, 2, 24)
    x = C.random_traj(rng, 20)
    prior = DC.symmetric_chain(0.1, 20)
    rouse = bild_amd.MultiStateRouse(8, 1, 5, d=2, localization_error=0.1)
    factorized = bild_amd.FactorizedModel([np.array([1.0, 2.0]), np.array([1.0, 4.0])], d=2)
    counts, contact = bild_amd.exact_dwell_switch_counts, bild_amd.exact_dwell_first_contact
    for other in (rouse, factorized):
        with pytest.raises(TypeError):
            counts(x, other, prior)
        with pytest.raises(TypeError):
            contact(x, other, prior, 1)
    for call in (lambda *a, **k: counts(*a, **k), lambda *a, **k: contact(*a, 1, **k)):
        with pytest.raises(TypeError):
            call(x, model, (prior.log_init, prior.log_jump))
        with pytest.raises(ValueError):
            call(x, model, prior, nan='drop')
        with pytest.raises(ValueError):         # the tables are shorter than the trajectory
            call(x, model, DC.symmetric_chain(0.1, 19))
        with pytest.raises(ValueError):         # the states do not match
            call(x, model, DC.make_prior('markov', rng, 3, 20))
        with pytest.raises(ValueError):         # beyond the model's lags
            call(C.random_traj(rng, 30), model, DC.symmetric_chain(0.1, 40))
        with pytest.raises(ValueError):         # more states than the recursion supports
            call(x, C.random_model(rng, 5, 24), DC.make_prior('markov', rng, 5, 20))
    for k_max in (-1, 20, 2.0, True):           # negative, beyond T - 1, not an integer
        with pytest.raises(ValueError):
            counts(x, model, prior, k_max=k_max)
    for target in ((), [], (0, 1), [1, 0, 1], 2, -1, (1, 2), 1.0, True, (0.5,)):     # empty, full, out of range, not a state
        with pytest.raises(ValueError):
            contact(x, model, prior, target)
    one = C.random_model(rng, 1, 24)            # one state has no proper subset
    with pytest.raises(ValueError):
        contact(x, one, DC.make_prior('markov', rng, 1, 20), 0)
    assert counts([], model, prior) == [] and contact([], model, prior, 1) == []
    with pytest.raises(ValueError):
        contact([], model, prior, 2)
