"""
The exact posterior of the number of visits to a set of states under a dwell-time prior without a GPU
(bild_amd.exact.exact_dwell_visits): the NumPy oracle tests/dwell_visit_oracle.py against the enumeration
of every profile on the cases of tests/test_dwell.py and on `dwell_event_cases.SMALL`, its identities against
`dwell_oracle.solve` and `dwell_event_oracle.solve`, the masses at the seam between two tiles of n, `DwellVisits`' derived
numbers, `ExactDwellDraws.visits` on hand-made states, `pooled_visits`, the argument errors and the binding against
include/bild_amd_visits.h.
"""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import bild_amd
import dwell_cases as DC
import dwell_event_cases as DEC
import dwell_event_oracle as DE
import dwell_oracle as DO
import dwell_visit_cases as DVC
import dwell_visit_oracle as DV
import segment_cases as C
import test_abi_header as AH
import test_dwell as TD
from bild_amd import _lib

# the issue's bound against enumeration and on the identities, the siblings' CPU bound
TOL = 1e-12

TARGETS = {2: ((1,), (0,)), 3: ((2,), (0, 2), (1,))}


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


def result(answer, model, prior, x, target):
    """ the oracle's answer as the `DwellVisits` that the device call would return """
    return bild_amd.DwellVisits(traj=x, model=model, prior=prior, nan='propagate', target=tuple(target), log_evidence=answer['logev'],
                                n_nan_windows=answer['n_nan_windows'], log_visits=answer['log_visits'], log_tail=answer['log_tail'])


def log_of(p):
    with np.errstate(divide='ignore'):
        return np.log(p)


def identities(W, F, prior, target, model, x, nan='propagate'):
    """ the identities of section 30 against `dwell_oracle.solve`'s marginals and jumps and `dwell_event_oracle.solve`, as deviations of logs """
    S, T = F.shape[0], F.shape[1] - 1
    inside = np.isin(np.arange(S), list(target))
    got = DV.solve(W, F, prior, target, nan=nan)
    ref = DO.solve(W, F, prior, nan=nan)
    events = DE.solve(W, F, prior, target=target, nan=nan)
    r = result(got, model, prior, x, target)
    pmf = r.pmf()
    assert pmf.shape == ((T + 1) // 2 + 1,) and got['log_tail'] == -np.inf
    post = np.exp(ref['log_post'])
    mean = post[inside, 0].sum() + ref['exp_jumps'][np.ix_(~inside, inside)].sum()
    devs = {'sum pmf = 1': abs(np.log(pmf.sum())),
            'pmf[0] = never in G': close_logs(log_of(pmf[0]), events['log_never'], 'never'),
            'sum_n visits = last marginal': close_logs(log_of(np.exp(got['log_visits']).sum(axis=0)), ref['log_post'][:, T - 1], 'columns'),
            'mean = starts in G + jumps into G': abs(np.log(r.mean()) - np.log(mean)) if mean > 0 else abs(r.mean())}
    if S == 2:
        counts = bild_amd.DwellSwitchCounts(traj=x, model=model, prior=prior, nan=nan, log_evidence=events['logev'],
                                            n_nan_windows=events['n_nan_windows'], log_count=events['log_count'], log_tail=events['log_tail'])
        seg = counts.segment_count_pmf(target[0])
        assert len(seg) >= len(pmf) and np.all(seg[len(pmf):] == 0)
        devs['pmf = segment_count_pmf'] = close_logs(log_of(pmf), log_of(seg[:len(pmf)]), 'segments')
    print(f"{target}: " + ', '.join(f"{k}: {v:.1e}" for k, v in devs.items()))
    for name, v in devs.items():
        assert v < TOL, (name, v)
    assert abs(got['logev'] - ref['logev']) < TOL
    return max(devs.values())


def cuts(W, F, prior, target, got):
    """ n_max = 0 and 1 reproduce the leading rows, and log_tail is the rest """
    pmf = np.exp(got['log_visits']).sum(axis=1)
    for n_max in (0, 1):
        cut = DV.solve(W, F, prior, target, n_max=n_max)
        rows = min(n_max + 1, len(got['log_visits']))
        assert cut['log_visits'].shape == (n_max + 1, F.shape[0])
        close_logs(cut['log_visits'][:rows], got['log_visits'][:rows], ('cut', n_max))
        assert np.all(cut['log_visits'][rows:] == -np.inf)
        rest = pmf[n_max + 1:].sum()
        if n_max >= len(pmf) - 1:
            assert cut['log_tail'] == -np.inf
        else:
            assert abs(np.exp(cut['log_tail']) - rest) < TOL, (n_max, cut['log_tail'], rest)


@pytest.mark.parametrize('kind', ['markov', 'nongeometric', 'minlength'])
@pytest.mark.parametrize('name', [n for n in TD.CASES if 'order0' not in n])
def test_oracle_against_enumeration_and_identities(name, kind):
    model, x, prior = TD.build(name, kind)
    S, T = TD.CASES[name][:2]
    W, F = C.tables(model, x)
    for target in TARGETS[S]:
        got, want = DV.solve(W, F, prior, target), DV.enumerate_all(W, F, prior, target)
        assert got['n_nan_windows'] == 0 and want['n_nan'] == 0 and got['log_visits'].shape == ((T + 1) // 2 + 1, S)
        assert abs(got['logev'] - want['logev']) < TOL
        worst = close_logs(got['log_visits'], want['log_visits'], (name, kind, target))
        print(f"{target}: worst deviation of a log from the enumeration {worst:.1e}")
        assert np.array_equal(got['log_visits'] > -np.inf, DV.prior_support(prior, target, S, T)), target
        identities(W, F, prior, target, model, x)
        cuts(W, F, prior, target, got)


@pytest.mark.parametrize('name', [n for n in DEC.SMALL if DEC.SMALL[n][0] > 1])
def test_oracle_against_enumeration_at_four_states_and_hard_priors(name):
    """ the oracle is the statement at these shapes too: `dwell_event_cases.SMALL`, every target of S, one frame missing """
    S, T, gap, kind = DEC.SMALL[name]
    model, x, prior, W, F = DEC.small_case(name)
    n_inf = 0
    for target in DEC.SMALL_TARGETS[S]:
        got, want = DV.solve(W, F, prior, target), DV.enumerate_all(W, F, prior, target)
        assert got['n_nan_windows'] == 0 and want['n_nan'] == 0 and got['log_visits'].shape == ((T + 1) // 2 + 1, S)
        assert np.isfinite(want['logev']) and abs(got['logev'] - want['logev']) < TOL
        worst = close_logs(got['log_visits'], want['log_visits'], (name, target))
        print(f"{target}: worst deviation of a log from the enumeration {worst:.1e}")
        identities(W, F, prior, target, model, x)
        cuts(W, F, prior, target, got)
        assert np.array_equal(got['log_visits'] > -np.inf, DV.prior_support(prior, target, S, T)), target
        n_inf += int(np.sum(got['log_visits'] == -np.inf))
    print(f"{name}: {n_inf} entries at -inf")
    assert n_inf > 0        # (n = 0 ends outside the target, under every prior)
    if kind == 'flip':      # the states alternate: T / 2 visits to either, T even
        assert T % 2 == 0 and np.all(np.isfinite(got['log_visits'][T // 2])) and np.all(np.delete(got['log_visits'], T // 2, axis=0) == -np.inf)


@pytest.mark.parametrize('kind', ['markov', 'nongeometric', 'minlength'])
@pytest.mark.parametrize('nan', ['propagate', 'omit'])
def test_oracle_nan_windows_against_enumeration(nan, kind):
    model, x, prior = TD.build('s2_order0_inner_gap', kind)
    W, F = C.tables(model, x)
    got, want = DV.solve(W, F, prior, (1,), nan=nan), DV.enumerate_all(W, F, prior, (1,), nan=nan)
    assert got['n_nan_windows'] == DO.solve(W, F, prior, nan=nan)['n_nan_windows'] > 0 and want['n_nan'] > 0
    if nan == 'propagate':
        assert np.isnan(got['logev']) and np.all(np.isnan(got['log_visits'])) and np.isnan(got['log_tail']) and np.all(np.isnan(want['log_visits']))
        return
    assert abs(got['logev'] - want['logev']) < TOL
    close_logs(got['log_visits'], want['log_visits'], (nan, kind))
    identities(W, F, prior, (1,), model, x, nan=nan)


@pytest.mark.parametrize('case', [c for c in DVC.ORACLE_CASES if c[4] == 'propagate' and c[2] != 'order0_gap'], ids=DVC.case_id)
def test_identities_on_the_gpu_cases(case):
    """ the identities that tests/test_gpu_dwell_visits.py holds the device to, on the oracle at the same cases """
    model, x, prior, W, F = DVC.oracle_case(*case[:4])
    worst = max(identities(W, F, prior, target, model, x) for target in case[5])
    print(f"{DVC.case_id(case)}: worst {worst:.1e}")


@pytest.mark.parametrize('T', DVC.SEAM_T)
def test_masses_at_the_tile_seam(T):
    """
    the `flip` prior alternates the states every frame: a profile that starts in 0 has T // 2 visits to state 1 and one that
    starts in 1 has (T + 1) // 2, so all the mass is in two entries, around the rows 62 | 63 (the kernel's seam) and 63 | 64
    """
    full = DVC.seam_answer(T)
    assert full['n_nan_windows'] == 0 and np.isfinite(full['logev']) and full['log_tail'] == -np.inf
    finite = tuple(map(tuple, np.argwhere(full['log_visits'] > -np.inf).tolist()))
    assert finite == DVC.SEAM_MASS[T]
    assert abs(np.exp(full['log_visits']).sum() - 1) < TOL
    for n_max in DVC.SEAM_N_MAX[1:]:
        cut = DVC.seam_answer(T, n_max)
        assert cut['log_visits'].shape == (n_max + 1, 2)
        rows = min(n_max + 1, len(full['log_visits']))
        assert np.array_equal(cut['log_visits'][:rows], full['log_visits'][:rows]) and np.all(cut['log_visits'][rows:] == -np.inf)
        kept = np.exp(cut['log_visits']).sum()
        if n_max >= (T + 1) // 2:
            assert cut['log_tail'] == -np.inf and abs(kept - 1) < TOL
        else:
            assert abs(np.exp(cut['log_tail']) - (1 - kept)) < TOL
    # the issue's numbers
    if T in (128, 129):
        cut = DVC.seam_answer(T, 63)
        assert np.all(cut['log_visits'] == -np.inf) and cut['log_tail'] == 0.0
    if T == 127:
        assert abs(np.exp(DVC.seam_answer(T, 63)['log_tail']) - 0.00131) < 1e-5
    if T == 129:
        assert abs(np.exp(DVC.seam_answer(T, 64)['log_tail']) - 0.9613) < 1e-4


def hand_made(vis, target=(1,), tail=0.0, T=None):
    with np.errstate(divide='ignore'):
        return bild_amd.DwellVisits(traj=np.zeros((2 * (len(vis) - 1) if T is None else T, 1)), model=None, prior=None, nan='propagate',
                                    target=target, log_evidence=0.0, n_nan_windows=0, log_visits=np.log(np.asarray(vis, dtype=float)),
                                    log_tail=float(np.log(tail)))


def test_derived_numbers_on_a_hand_made_pmf():
    # P(N = n) = 0.1, 0.2, 0.4, 0.25, 0.05, split over two last states
    r = hand_made([[0.1, 0.0], [0.05, 0.15], [0.3, 0.1], [0.0, 0.25], [0.0, 0.05]])
    assert np.allclose(r.pmf(), [0.1, 0.2, 0.4, 0.25, 0.05], atol=1e-15)
    assert np.allclose(r.cdf(), [0.1, 0.3, 0.7, 0.95, 1.0], atol=1e-15)
    mean = 0.2 + 0.8 + 0.75 + 0.2
    assert abs(r.mean() - mean) < 1e-15
    assert abs(r.var() - (0.2 + 1.6 + 2.25 + 0.8 - mean ** 2)) < 1e-14
    # the smallest n whose cdf reaches the tail's share: 0.025 -> 0 and 0.975 -> 4; 0.2 -> 1 and 0.8 -> 3; 0.35 -> 2 and 0.65 -> 2
    assert r.interval() == (0, 4) and r.interval(0.6) == (1, 3) and r.interval(0.3) == (2, 2)
    assert r.interval(0.8) == (0, 3)        # 0.1 is reached at n = 0 (cdf = 0.1), 0.9 at n = 3
    spike = hand_made([[0.0, 0.0], [0.0, 0.0], [1.0, 0.0]])
    assert spike.interval() == (2, 2) and spike.mean() == 2.0 and spike.var() == 0.0
    for level in (0, 1, -0.5, 1.5):
        with pytest.raises(ValueError):
            r.interval(level)
    with pytest.raises(ValueError):
        hand_made([[np.nan, np.nan], [np.nan, np.nan]]).interval()
    assert 'target=(1,)' in repr(r) and 'T=8' in repr(r) and 'n_max=4' in repr(r)
    # a cut table: 0.05 lies beyond n_max = 3.  (1 - level) / 2 = 0.1 leaves room for it, 0.025 does not
    cut = hand_made([[0.1, 0.0], [0.05, 0.15], [0.3, 0.1], [0.0, 0.25]], tail=0.05)
    assert np.allclose(cut.cdf(), [0.1, 0.3, 0.7, 0.95], atol=1e-15) and abs(cut.mean() - (0.2 + 0.8 + 0.75)) < 1e-15
    assert cut.interval(0.8) == (0, 3) and cut.interval(0.6) == (1, 3)
    with pytest.raises(ValueError, match='n_max'):
        cut.interval()


def test_visits_of_draws_on_hand_made_states():
    states = np.array([[0, 0, 1, 1, 0, 255], [1, 0, 0, 0, 0, 255], [0, 0, 0, 0, 1, 255], [0, 2, 2, 1, 0, 255], [2, 1, 0, 1, 2, 255],
                       [1, 0, 1, 0, 1, 255], [0, 0, 0, 0, 0, 255], [1, 2, 0, 2, 1, 255]], dtype=np.uint8)
    n = len(states)
    draws = bild_amd.ExactDwellDraws(5, states, np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n), None)
    # a run at frame 0 (rows 1, 4, 5, 7), a run that reaches frame T - 1 (rows 2, 4, 5, 7), adjacent states of the set as one
    # visit (rows 3, 4, 7 under (1, 2)), a state that never occurs, and the padding behind T
    for target, want in ((1, [1, 1, 1, 1, 2, 3, 0, 2]), ([1], [1, 1, 1, 1, 2, 3, 0, 2]), ((1, 2), [1, 1, 1, 1, 2, 3, 0, 2]),
                         ({2}, [0, 0, 0, 1, 2, 0, 0, 2]), (0, [2, 1, 1, 2, 1, 2, 1, 1]), ((0, 2), [2, 1, 1, 2, 3, 2, 1, 1]),
                         (3, [0] * 8), (255, [0] * 8)):
        got = draws.visits(target)
        assert got.dtype == np.int64 and got.tolist() == want, target
        inside = np.isin(np.arange(256), [target] if isinstance(target, int) else list(target))
        assert want == [DV.count_visits(row[:5], inside) for row in states] or target == 255
    empty = bild_amd.ExactDwellDraws(5, np.zeros((0, 5), dtype=np.uint8), np.zeros(0), np.zeros(0), np.zeros(0), np.zeros(0), None)
    assert empty.visits(1).shape == (0,)
    none = bild_amd.ExactDwellDraws(0, np.zeros((3, 0), dtype=np.uint8), np.zeros(3), np.zeros(3), np.zeros(3), np.zeros(3), None)
    assert none.visits(1).tolist() == [0, 0, 0]


def test_pooled_visits():
    a = hand_made([[0.1, 0.0], [0.05, 0.15], [0.3, 0.1], [0.0, 0.3]])
    b = hand_made([[0.2, 0.2], [0.0, 0.5], [0.1, 0.0]])
    want = np.zeros(3 + 2 + 1)
    for i, p in enumerate(a.pmf()):
        for j, q in enumerate(b.pmf()):
            want[i + j] += p * q
    got = bild_amd.pooled_visits([a, b])
    assert got.shape == (6,) and np.max(np.abs(got - want)) < 1e-15 and abs(got.sum() - 1) < 1e-15
    assert np.max(np.abs(bild_amd.pooled_visits([b, a]) - want)) < 1e-15
    assert np.array_equal(bild_amd.pooled_visits([a]), a.pmf())
    assert np.array_equal(bild_amd.pooled_visits(iter([a])), a.pmf())
    with pytest.raises(ValueError, match='no result'):
        bild_amd.pooled_visits([])
    with pytest.raises(ValueError, match='differing targets'):
        bild_amd.pooled_visits([a, hand_made([[0.5, 0.5], [0.0, 0.0]], target=(0,))])
    with pytest.raises(ValueError, match='NaN'):
        bild_amd.pooled_visits([a, hand_made([[np.nan, np.nan], [np.nan, np.nan]])])
    with pytest.raises(ValueError, match='log_tail'):
        bild_amd.pooled_visits([a, hand_made([[0.2, 0.2], [0.0, 0.5]], tail=0.1)])


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
    call = bild_amd.exact_dwell_visits
    for other in (rouse, factorized):
        with pytest.raises(TypeError):
            call(x, other, prior, 1)
    with pytest.raises(TypeError):
        call(x, model, (prior.log_init, prior.log_jump), 1)
    with pytest.raises(ValueError):
        call(x, model, prior, 1, nan='drop')
    with pytest.raises(ValueError):         # the tables are shorter than the trajectory
        call(x, model, DC.symmetric_chain(0.1, 19), 1)
    with pytest.raises(ValueError):         # the states do not match
        call(x, model, DC.make_prior('markov', rng, 3, 20), 1)
    with pytest.raises(ValueError):         # beyond the model's lags
        call(C.random_traj(rng, 30), model, DC.symmetric_chain(0.1, 40), 1)
    with pytest.raises(ValueError):         # more states than the recursion supports
        call(x, C.random_model(rng, 5, 24), DC.make_prior('markov', rng, 5, 20), 1)
    for target in ((), [], (0, 1), [1, 0, 1], 2, -1, (1, 2), 1.0, True, (0.5,)):     # empty, full, out of range, not a state
        with pytest.raises(ValueError):
            call(x, model, prior, target)
    for n_max in (-1, 1.0, True, '3', (2,)):        # negative, not an integer
        with pytest.raises(ValueError, match='n_max'):
            call(x, model, prior, 1, n_max=n_max)
    with pytest.raises(ValueError, match='target'):     # the target is checked before n_max
        call(x, model, prior, 2, n_max=-1)
    with pytest.raises(ValueError, match="nan ="):      # and `exact_dwell`'s checks before the target
        call(x, model, prior, 2, nan='drop')
    one = C.random_model(rng, 1, 24)            # one state has no proper subset
    with pytest.raises(ValueError):
        call(x, one, DC.make_prior('markov', rng, 1, 20), 0)
    assert call([], model, prior, 1) == [] and call([], model, prior, 1, n_max=3) == []
    with pytest.raises(ValueError):
        call([], model, prior, 2)
    with pytest.raises(ValueError):
        call([], model, prior, 1, n_max=-1)


# ---------------------------------------------------------------- the binding against include/bild_amd_visits.h

def visits_header():
    """ include/bild_amd_visits.h without its comments, as `test_dwell_windows.windows_header` reads its header: ({struct: fields}, {function: (return type, parameters)}) """
    text = open(os.path.join(AH.ROOT, 'include', 'bild_amd_visits.h')).read()
    text = re.sub(r'//[^\n]*', '', re.sub(r'/\*.*?\*/', '', text, flags=re.S))
    structs = {tag: [f for part in body.split(';') if part.strip() for f in AH._declarations(part)]
               for tag, body, name in re.findall(r'typedef\s+struct\s+(bild_\w+_out)\s*\{(.*?)\}\s*(\w+)\s*;', text, flags=re.S) if tag == name}
    text = re.sub(r'typedef\s+struct\s*\w*\s*\{.*?\}\s*\w+\s*;', '', text, flags=re.S)
    text = '\n'.join(line for line in text.splitlines() if not line.lstrip().startswith('#'))
    prototypes = {name: (' '.join(ret.split()), [AH._declarations(a)[0] for a in args.split(',')])
                  for ret, name, args in re.findall(r'([\w\s*]+?)\b(bild_\w+)\s*\(([^()]*)\)\s*;', text)}
    return structs, prototypes


def test_binding_matches_the_new_header(monkeypatch):
    structs, prototypes = visits_header()
    assert list(structs) == ['bild_dwell_visits_out'] and list(prototypes) == ['bild_gauss_dwell_visits'] == list(_lib._SIGNATURES_VISITS)
    assert '#include "bild_amd.h"' in open(os.path.join(AH.ROOT, 'include', 'bild_amd_visits.h')).read()
    # the two older tables and what the first exports stay as they were
    assert list(_lib._SIGNATURES_EXT) == ['bild_gauss_dwell_windows'] and 'bild_gauss_dwell_visits' not in _lib._SIGNATURES
    assert _lib.exported_symbols() == list(_lib._SIGNATURES) and list(_lib._SIGNATURES)[-1] == 'bild_choice_counts'
    fields = structs['bild_dwell_visits_out']
    assert [f[0] for f in _lib.DwellVisitsOut._fields_] == [f[0] for f in fields] == ['logev', 'n_nan_windows', 'log_visits', 'log_tail']
    assert all(f[1] is ctypes.c_void_p for f in _lib.DwellVisitsOut._fields_) and all(f[2] for f in fields)
    assert {f[0]: f[1] for f in fields} == {'logev': 'double', 'n_nan_windows': 'int64_t', 'log_visits': 'double', 'log_tail': 'double'}
    ret, params = prototypes['bild_gauss_dwell_visits']
    restype, argtypes = _lib._SIGNATURES_VISITS['bild_gauss_dwell_visits']
    assert ret == 'int' and restype is ctypes.c_int and len(argtypes) == len(params) == 13
    for (pname, ctype, pointer), t in zip(params, argtypes):
        assert AH._is_pointer(t) if pointer else t is AH.SCALARS[ctype], pname
    assert [p[0] for p in params] == ['m', 'ts', 'L', 'log_init', 'log_jump', 'log_dwell', 'log_surv', 'T_max', 'n_max', 'target', 'flags',
                                      'scratch_bytes', 'out']
    assert {p[0]: p[1] for p in params if not p[2]} == {'L': 'int', 'T_max': 'int', 'n_max': 'int', 'target': 'unsigned', 'flags': 'unsigned',
                                                        'scratch_bytes': 'int64_t'}

    # the wrapper on a recorder in place of the library: every argument at the position the header names
    rec = AH.Recorder()
    monkeypatch.setattr(_lib, 'lib', lambda: rec)
    S, T, L = 3, [1, 5], 5
    model = types.SimpleNamespace(_h=0x1000, S=S, d=1, Tmax=7)
    ts = types.SimpleNamespace(_h=0x2000, n_traj=len(T), T=np.array(T, dtype=np.int32))
    tables = (np.zeros(S), np.zeros((S, S)), np.zeros((S, L)), np.zeros((S, L)))
    for omit, scratch, target, n_max in ((True, 31, 5, 2), (False, 0, 2, 7)):
        res = _lib.gauss_dwell_visits(model, ts, *tables, target, n_max, omit=omit, scratch_bytes=scratch)
        name, args = rec.calls[-1]
        assert name == 'bild_gauss_dwell_visits' and len(args) == len(params)
        named = dict(zip([p[0] for p in params], args))
        given = dict(m=model._h, ts=ts._h, L=L, T_max=max(T), n_max=n_max, target=target, flags=int(omit), scratch_bytes=scratch,
                     log_init=tables[0], log_jump=tables[1], log_dwell=tables[2], log_surv=tables[3])
        for key, want in given.items():
            got = named[key]
            if isinstance(want, np.ndarray):
                assert got == want.ctypes.data, key
            else:
                assert got == want and type(got) is type(want), (key, got)
        spec = named['out']._obj
        assert type(spec) is _lib.DwellVisitsOut and list(res) == [f[0] for f in fields]
        for field, ctype, _ in fields:
            assert res[field].dtype == AH.DTYPES[ctype] and getattr(spec, field) == res[field].ctypes.data, field
        assert res['logev'].shape == res['log_tail'].shape == res['n_nan_windows'].shape == (2,) and res['log_visits'].shape == (2, n_max + 1, S)
    assert len(rec.calls) == 2
