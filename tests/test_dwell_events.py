"""
The exact switch counts and first-contact times under a dwell-time prior without a GPU
(bild_amd.exact.exact_dwell_switch_counts, exact_dwell_first_contact): the NumPy oracle
tests/dwell_event_oracle.py against the enumeration of every profile on the cases of tests/test_dwell.py, its identities
against `dwell_oracle.solve`, `DwellSwitchCounts`' derived distributions, `ExactDwellDraws.first_contact` on hand-made states,
and the argument errors.
"""
import os
import re

import numpy as np
import pytest

import bild_amd
import dwell_cases as DC
import dwell_event_cases as DEC
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


@pytest.mark.parametrize('name', list(DEC.SMALL))
def test_oracle_against_enumeration_at_one_and_four_states_and_hard_priors(name):
    """ the oracle is the statement at these shapes too: `dwell_event_cases.SMALL`, every target of S, one frame missing """
    S, T, gap, kind = DEC.SMALL[name]
    model, x, prior, W, F = DEC.small_case(name)
    assert model.nStates == prior.nStates == S and np.array_equal(np.flatnonzero(np.isnan(x[:, 0])), [gap]) and F.shape == (S, T + 1)
    ref = DO.solve(W, F, prior)
    assert ref['n_nan_windows'] == 0 and np.isfinite(ref['logev'])
    if S == 1:      # the counts alone: one state has no proper subset, and the calls with a target refuse it (below)
        got, want = DE.solve(W, F, prior), DE.enumerate_all(W, F, prior)
        assert abs(got['logev'] - want['logev']) < TOL and got['log_tail'] == -np.inf
        close_logs(got['log_count'], want['log_count'], name)
        assert abs(got['log_count'][0, 0]) < TOL and np.all(got['log_count'][1:] == -np.inf)
        return
    n_inf = 0
    for target in DEC.SMALL_TARGETS[S]:
        got, want = DE.solve(W, F, prior, target=target), DE.enumerate_all(W, F, prior, target=target)
        assert got['n_nan_windows'] == 0 and want['n_nan'] == 0 and got['log_count'].shape == (T, S)
        assert abs(got['logev'] - ref['logev']) < TOL
        compare(got, want)
        identities(got, ref, target, S, T, model, prior, x)
        n_inf += int(np.sum(got['log_count'] == -np.inf)) + int(np.sum(got['log_first'] == -np.inf)) + int(got['log_never'] == -np.inf)
    print(f"{name}: {n_inf} entries at -inf")
    # ('absorbing' has its -inf in log_jump: every level and every contact frame keeps a profile)
    assert (n_inf > 0) == (kind not in ('nongeometric', 'absorbing'))
    if kind == 'absorbing':
        assert np.all(prior.log_jump[2] == -np.inf) and prior.log_jump[0, 2] == -np.inf
    if kind == 'flip':          # one profile per start state: T - 1 switches
        assert np.all(got['log_count'][:T - 1] == -np.inf) and np.all(np.isfinite(got['log_count'][T - 1]))
    if kind == 'bounded3':      # no segment longer than 3 frames: at least ceil(T / 3) - 1 switches, and a contact within 3 frames
        assert np.all(got['log_count'][:-(-T // 3) - 1] == -np.inf) and np.all(got['log_first'][4:] == -np.inf) and got['log_never'] == -np.inf


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


# ---------------------------------------------------------------- the conditions on the inputs of the wide GPU cases

# per wide case what the oracle gives: the finite entries of log_count, and per target (the finite entries of log_first, whether
# log_never is finite).  Listed, so that a change of a generator that empties a comparison is seen here.
WIDE_FINITE = {
    (4, 64, (), 'minlength'): (128, {(0,): (63, True), (1, 3): (63, True), (0, 1, 2): (63, True)}),
    (4, 129, (64, 100), 'markov'): (516, {(0,): (129, True), (1, 3): (129, True), (0, 1, 2): (129, True)}),
    (4, 257, (100,), 'nongeometric'): (1028, {(0,): (257, True), (1, 3): (257, True), (0, 1, 2): (257, True)}),
    (2, 256, (), 'markov'): (512, {(1,): (256, True), (0,): (256, True)}),
    (2, 257, (255,), 'minlength'): (258, {(1,): (256, True), (0,): (256, True)}),
    (3, 321, (128,), 'markov'): (963, {(2,): (321, True), (0, 2): (321, True), (1,): (321, True)}),
    (2, 65, (), 'nongeometric'): (130, {(1,): (65, True), (0,): (65, True)}),
    (3, 193, (3,), 'nongeometric'): (579, {(2,): (193, True), (0, 2): (193, True), (1,): (193, True)}),
    (1, 130, (), 'nongeometric'): (1, {}),
    (2, 130, (), 'bounded'): (258, {(1,): (71, False), (0,): (71, False)}),
    (3, 193, (), 'bounded'): (573, {(2,): (193, True), (0, 2): (71, False), (1,): (141, False)}),
    (2, 65, (), 'one_start'): (65, {(1,): (1, False), (0,): (64, True)}),
    (3, 130, (20,), 'absorbing'): (390, {(2,): (130, True), (0, 2): (130, True), (1,): (130, True)}),
    (2, 70, (), 'flip'): (2, {(1,): (2, False), (0,): (2, False)}),
}
# the finite entries of log_count under the cut k_max; log_tail is finite under each
WIDE_CUT_FINITE = {((2, 130, (), 'bounded'), 63): 126, ((2, 130, (), 'bounded'), 64): 128, ((2, 130, (), 'bounded'), 65): 130,
                   ((3, 321, (128,), 'markov'), 256): 771}


@pytest.mark.parametrize('case', DEC.WIDE, ids=DEC.wide_id)
def test_gpu_wide_cases_meet_their_conditions(case):
    """ what tests/test_gpu_dwell_events.py compares the device with is what it is meant to be, and no comparison is vacuous """
    S, T, missing, kind = case
    model, x, prior, W, F = DC.oracle_case(case)
    assert model.nStates == prior.nStates == S and x.shape == (T, 2) and prior.L == T + 5
    assert np.array_equal(np.flatnonzero(np.isnan(x[:, 0])), missing)
    if kind in ('nongeometric', 'bounded'):     # independent tables, neither of them monotone
        assert all(np.any(np.diff(t[:, :DC.BOUND], axis=1) > 0) and np.any(np.diff(t[:, :DC.BOUND], axis=1) < 0) for t in (prior.log_dwell, prior.log_surv))
    want = DEC.wide_counts(case)
    assert want['n_nan_windows'] == 0 and np.isfinite(want['logev']) and want['log_count'].shape == (T, S) and want['log_tail'] == -np.inf
    assert not np.any(np.isnan(want['log_count'])) and abs(np.exp(want['log_count']).sum() - 1) < 1e-10
    finite, contacts = WIDE_FINITE[case]
    assert int(np.sum(want['log_count'] > -np.inf)) == finite > 0
    seconds = [DEC.ORACLE_SECONDS[case, 'counts', None]]
    assert list(contacts) == list(DEC.WIDE_TARGETS[S])
    for target, (n_first, never) in contacts.items():
        c = DEC.wide_contact(case, target)
        seconds.append(DEC.ORACLE_SECONDS[case, target])
        assert c['log_first'].shape == (T,) and not np.any(np.isnan(c['log_first'])) and not np.isnan(c['log_never'])
        assert int(np.sum(c['log_first'] > -np.inf)) == n_first > 0 and bool(c['log_never'] > -np.inf) == never
        assert c['logev'] == want['logev'] and np.array_equal(c['log_count'][0], want['log_count'][0])
    print(f"{case}: slowest oracle answer {max(seconds):.1f} s, {finite} of {T * S} counts finite")
    assert max(seconds) < 20
    # where the case is there for its -inf entries, some are compared: every hard prior but 'absorbing' has levels without a
    # profile ('absorbing' has its -inf in log_jump, which the kernels read, and in the occupancy); 'bounded', 'one_start' and
    # 'flip' have frames without a first contact
    if kind in ('minlength', 'bounded', 'one_start', 'flip'):
        assert finite < T * S
    if kind in ('bounded', 'one_start', 'flip'):
        assert any(n_first < T and not never for n_first, never in contacts.values())
    if kind == 'absorbing':
        assert np.all(prior.log_jump[2] == -np.inf)


@pytest.mark.parametrize('item', [c for c in DEC.WIDE_CASES if c[1] is not None], ids=DEC.wide_id)
def test_gpu_wide_cuts_meet_their_conditions(item):
    case, k_max = item
    S, T = case[:2]
    cut, full = DEC.wide_counts(case, k_max), DEC.wide_counts(case)
    assert k_max % 64 in (63, 0, 1) and k_max < T - 1      # around the first level of a tile of the level kernel
    assert cut['log_count'].shape == (k_max + 1, S) and np.array_equal(cut['log_count'], full['log_count'][:k_max + 1])
    assert int(np.sum(cut['log_count'] > -np.inf)) == WIDE_CUT_FINITE[item]
    # the tail is a probability that the bar of 1e-12 can see, or the logs of the levels behind the cut add up to it
    assert np.isfinite(cut['log_tail']) and abs(np.exp(cut['log_tail']) - np.exp(full['log_count'][k_max + 1:]).sum()) < 1e-12
    assert DEC.ORACLE_SECONDS[case, 'counts', k_max] < 20


def test_gpu_ragged_batch_meets_its_conditions():
    model, prior, xs, _ = DC.ragged_case()
    assert [len(x) for x in xs] == [1, 257, 64, 130, 2, 65] and model.nStates == 4
    for j, x in enumerate(xs):
        T = len(x)
        want = DEC.ragged_counts(j)
        assert want['n_nan_windows'] == 0 and np.isfinite(want['logev']) and np.all(np.isfinite(want['log_count'])) and want['log_count'].shape == (T, 4)
        seconds = [DEC.ORACLE_SECONDS['ragged', j, 'counts']]
        for target in DEC.RAGGED_TARGETS:
            c = DEC.ragged_contact(j, target)
            seconds.append(DEC.ORACLE_SECONDS['ragged', j, target])
            assert c['log_first'].shape == (T,) and np.all(np.isfinite(c['log_first'])) and np.isfinite(c['log_never'])
        assert max(seconds) < 20


def dwell_constants():
    """ the constexpr ints of bild_amd/csrc/gauss_dwell.h """
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'bild_amd', 'csrc', 'gauss_dwell.h')).read()
    return {name: int(value) for name, value in re.findall(r'constexpr int (k\w+) = (\d+);', text)}


def test_nine_trajectories_are_more_than_two_workgroups():
    """ dwell_contact_kernel puts kDwellThreads / 64 trajectories in a workgroup, a wave each (csrc/gauss_dwellevent.hip) """
    k = dwell_constants()
    assert k['kDwellThreads'] == 256 and k['kDwellTile'] == 64 and k['kDwellMaxS'] == 4
    source = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'bild_amd', 'csrc', 'gauss_dwellevent.hip')).read()
    assert 'blockIdx.x * (kDwellThreads / 64) + (threadIdx.x >> 6)' in source
    per_group = k['kDwellThreads'] // 64
    model, prior, xs = DEC.nine_trajectories()
    assert len(xs) == 9 > 2 * per_group and len(xs) % per_group == 1        # three workgroups, the last with one wave
    assert per_group < len(DC.RAGGED) < 2 * per_group                       # the ragged batch: two, the second partial
    assert [len(x) for x in xs] == [T for T, _ in DC.RAGGED] + list(DEC.NINE_MORE) and max(len(x) for x in xs) == 257
    assert all(x.shape[1] == 2 and not np.any(np.isnan(x[len(x) - 1])) for x in xs)
