"""
The exact switch counts and first-contact times under a dwell-time prior on the GPU (bild_amd.exact.exact_dwell_switch_counts,
exact_dwell_first_contact, csrc/gauss_dwellevent.hip): against the NumPy oracle
tests/dwell_event_oracle.py around the 64-frame tiles, the identities at T = 1000, the histograms of `exact_dwell_draw` as an
independent device route, the bit-identity properties and the refusals of the C calls.
"""
import ctypes

import numpy as np
import pytest

import bild_amd
import dwell_cases as DC
import dwell_event_cases as DEC
import segment_cases as C
from bild_amd import _lib

pytestmark = pytest.mark.gpu

# The issue's bounds, the siblings' device bounds: a finite log within 1e-10, -inf exactly, log_tail as a probability within 1e-12.
# Worst seen on these cases: DESIGN.md section 27.
TOL_LOG, TOL_TAIL = 1e-10, 1e-12


def log_deviation(got, want, what):
    """ the worst |got - want| over the finite logs; -inf must come back as -inf """
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    assert got.shape == want.shape and not np.any(np.isnan(got)), what
    assert np.array_equal(got == -np.inf, want == -np.inf), what
    fin = want > -np.inf
    return float(np.max(np.abs(got[fin] - want[fin]), initial=0.0))


@pytest.mark.parametrize('case', DEC.ORACLE_CASES, ids=DEC.case_id)
def test_against_oracle(case):
    S, T, missing, _, nan, targets, k_max = case
    model, x, prior, W, F = DEC.oracle_case(*case[:4])
    answers = DEC.oracle_answer(case)
    want = next(iter(answers.values()))
    ref = bild_amd.exact_dwell(x, model, prior, marginals=False, nan=nan)
    r = bild_amd.exact_dwell_switch_counts(x, model, prior, k_max=k_max, nan=nan)
    rows = T if k_max is None else k_max + 1
    assert r.log_count.shape == (rows, S) and r.n_nan_windows == want['n_nan_windows'] == ref.n_nan_windows
    assert (r.n_nan_windows > 0) == (missing == 'order0_gap')
    assert np.array_equal(r.log_evidence, ref.log_evidence, equal_nan=True)         # bit for bit `exact_dwell`'s
    contacts = {target: bild_amd.exact_dwell_first_contact(x, model, prior, target, nan=nan) for target in targets}
    for target, c in contacts.items():
        assert c.target == target and c.log_first.shape == (T,) and c.n_nan_windows == ref.n_nan_windows
        assert np.array_equal(c.log_evidence, ref.log_evidence, equal_nan=True)
    if np.isnan(want['logev']):
        assert nan == 'propagate' and np.isnan(r.log_evidence) and np.all(np.isnan(r.log_count)) and np.isnan(r.log_tail)
        assert all(np.all(np.isnan(c.log_first)) and np.isnan(c.log_never) for c in contacts.values())
        return
    devs = {'logev': abs(r.log_evidence - want['logev']), 'log_count': log_deviation(r.log_count, want['log_count'], 'log_count')}
    with np.errstate(divide='ignore'):
        devs['tail'] = abs(np.exp(r.log_tail) - np.exp(want['log_tail']))
    for target, c in contacts.items():
        devs[f"log_first{target}"] = log_deviation(c.log_first, answers[target]['log_first'], target)
        devs[f"log_never{target}"] = log_deviation(c.log_never, answers[target]['log_never'], target)
    print(f"{DEC.case_id(case)}: " + ', '.join(f"{k} {v:.1e}" for k, v in devs.items()))
    for name, v in devs.items():
        assert v < (TOL_TAIL if name == 'tail' else TOL_LOG), (case, name, v)
    if k_max is None:
        assert r.log_tail == -np.inf and abs(r.pmf().sum() - 1) < 2 * TOL_LOG      # (logs within TOL_LOG of an oracle that sums to 1)
    else:
        assert np.isfinite(r.log_tail) and abs(r.pmf().sum() + np.exp(r.log_tail) - 1) < TOL_TAIL
    if S == 1 or T == 1:
        assert np.all(r.log_count[1:] == -np.inf) and abs(np.log(r.pmf()[0])) < TOL_LOG


def hold_counts(r, want, ref, S, T, k_max, what):
    """ a `DwellSwitchCounts` against the oracle's answer and `exact_dwell`'s evidence: {name: deviation}, the bars asserted """
    rows = T if k_max is None else k_max + 1
    assert r.log_count.shape == (rows, S) and r.n_nan_windows == want['n_nan_windows'] == ref.n_nan_windows == 0, what
    assert np.isfinite(ref.log_evidence) and r.log_evidence == ref.log_evidence, what      # bit for bit `exact_dwell`'s
    devs = {'logev': abs(r.log_evidence - want['logev']), 'log_count': log_deviation(r.log_count, want['log_count'], what)}
    with np.errstate(divide='ignore'):
        devs['tail'] = abs(np.exp(r.log_tail) - np.exp(want['log_tail']))
    for name, v in devs.items():
        assert v < (TOL_TAIL if name == 'tail' else TOL_LOG), (what, name, v)
    if k_max is None or k_max >= T - 1:
        assert r.log_tail == -np.inf and abs(r.pmf().sum() - 1) < 2 * TOL_LOG, what
    else:
        assert not np.isnan(r.log_tail) and abs(r.pmf().sum() + np.exp(r.log_tail) - 1) < TOL_TAIL, what
    return devs


def hold_contact(c, want, ref, target, T, what):
    """ a `DwellFirstContact` against the oracle's answer and `exact_dwell`'s evidence: {name: deviation}, the bars asserted """
    assert c.target == target and c.log_first.shape == (T,) and c.n_nan_windows == want['n_nan_windows'] == ref.n_nan_windows == 0, what
    assert c.log_evidence == ref.log_evidence, what
    devs = {f"log_first{target}": log_deviation(c.log_first, want['log_first'], what),
            f"log_never{target}": log_deviation(c.log_never, want['log_never'], what)}
    for name, v in devs.items():
        assert v < TOL_LOG, (what, name, v)
    with np.errstate(divide='ignore'):
        assert abs(np.exp(c.log_first).sum() + np.exp(c.log_never) - 1) < 2 * TOL_LOG, what     # (as the pmf: logs within TOL_LOG)
    return devs


@pytest.mark.parametrize('item', DEC.WIDE_CASES, ids=DEC.wide_id)
def test_against_oracle_wide(item):
    """ four states, T > 256, non-geometric tables and the hard priors (tests/README_dwell_events.md, "The wide cases") """
    case, k_max = item
    S, T = case[:2]
    model, x, prior, _, _ = DC.oracle_case(case)
    want = DEC.wide_counts(case, k_max)
    ref = bild_amd.exact_dwell(x, model, prior, marginals=False)
    r = bild_amd.exact_dwell_switch_counts(x, model, prior, k_max=k_max)
    devs = hold_counts(r, want, ref, S, T, k_max, item)
    seconds = DEC.ORACLE_SECONDS[case, 'counts', k_max]
    for target in DEC.WIDE_TARGETS[S] if k_max is None else ():
        c = bild_amd.exact_dwell_first_contact(x, model, prior, target)
        devs.update(hold_contact(c, DEC.wide_contact(case, target), ref, target, T, (item, target)))
        seconds = max(seconds, DEC.ORACLE_SECONDS[case, target])
    print(f"{DEC.wide_id(item)}: slowest oracle answer {seconds:.2f} s; " + ', '.join(f"{k} {v:.1e}" for k, v in devs.items()))
    assert seconds < 20
    if S == 1:
        assert np.all(r.log_count[1:] == -np.inf) and abs(np.log(r.pmf()[0])) < TOL_LOG


def test_identities_at_T1000():
    T = 1000
    rng = np.random.default_rng(31)
    model = C.random_model(rng, 2, T + 8, orders=np.ones((2, 3), dtype=int), d=3)
    x = C.random_traj(rng, T, (100, 500, 501), d=3)
    prior = bild_amd.DwellPrior.markov([[0.98, 0.02], [0.05, 0.95]], [0.6, 0.4], n=T)
    ref = bild_amd.exact_dwell(x, model, prior)
    r = bild_amd.exact_dwell_switch_counts(x, model, prior)
    c = bild_amd.exact_dwell_first_contact(x, model, prior, 1)
    assert r.log_count.shape == (T, 2) and r.log_tail == -np.inf and r.n_nan_windows == 0
    assert r.log_evidence == ref.log_evidence == c.log_evidence and np.isfinite(r.log_evidence)
    post = np.exp(ref.log_marginal_posterior)
    jumps = ref.expected_jumps.sum()
    devs = {'sum pmf = 1': abs(r.pmf().sum() - 1),
            'mean = expected jumps (relative)': abs(r.mean() - jumps) / jumps,
            'sum_n count = last marginal': float(np.max(np.abs(np.exp(r.log_count).sum(axis=0) - post[:, T - 1]))),
            'sum first + never = 1': abs(np.exp(c.log_first).sum() + np.exp(c.log_never) - 1),
            'never = count[0][0]': abs(np.exp(c.log_never) - np.exp(r.log_count[0, 0])),
            'first[0] = first marginal': abs(np.exp(c.log_first[0]) - post[1, 0])}
    print(f"mean {r.mean():.6f} switches, mode {int(np.argmax(r.pmf()))}; " + ', '.join(f"{k}: {v:.1e}" for k, v in devs.items()))
    assert devs.pop('mean = expected jumps (relative)') < 1e-8
    assert all(v < 1e-9 for v in devs.values()), devs
    assert abs(c.cdf()[-1] + np.exp(c.log_never) - 1) < 1e-9


def test_against_the_histograms_of_the_draws():
    """ every bin within 5 sqrt(p (1 - p) / n) + 1 / n of the exact p: the binomial bound, nothing fitted """
    T, n = 130, 20000
    rng = np.random.default_rng(77)
    model = C.random_model(rng, 2, T + 8)
    x = C.random_traj(rng, T, (64,))
    prior = DC.make_prior('markov', rng, 2, T)
    draws = bild_amd.exact_dwell(x, model, prior).draw(n, seed=5)
    r = bild_amd.exact_dwell_switch_counts(x, model, prior)
    c = bild_amd.exact_dwell_first_contact(x, model, prior, 1)

    def hold(hist, p, what):
        slack = np.abs(hist - p) - (5 * np.sqrt(p * (1 - p) / n) + 1 / n)
        print(f"{what}: {len(p)} bins, largest |histogram - exact| {np.max(np.abs(hist - p)):.2e}, closest to its bound by {-np.max(slack):.2e}")
        assert np.all(slack <= 0), (what, int(np.argmax(slack)), float(np.max(slack)))

    hold(np.bincount(draws.n_switches, minlength=T)[:T] / n, r.pmf(), 'switch count')
    first = draws.first_contact(1)
    hold(np.bincount(first[first >= 0], minlength=T)[:T] / n, np.exp(c.log_first), 'first contact')
    hold(np.array([np.mean(first < 0)]), np.array([np.exp(c.log_never)]), 'never')
    assert np.all(draws.n_switches < T) and np.all(first < T)


FIELDS = {'counts': ('log_evidence', 'n_nan_windows', 'log_count', 'log_tail'),
          'contact': ('log_evidence', 'n_nan_windows', 'log_first', 'log_never')}


def same(a, b, kind):
    return all(np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True) for f in FIELDS[kind])


def test_bit_identity():
    rng = np.random.default_rng(41)
    model = C.random_model(rng, 2, 200)
    xs = [C.random_traj(rng, T, missing) for T, missing in ((40, ()), (65, (9,)), (193, (63, 65)), (65, ()))]
    prior = DC.make_prior('markov', rng, 2, 193)
    calls = {'counts': lambda trajs, **kw: bild_amd.exact_dwell_switch_counts(trajs, model, prior, **kw),
             'contact': lambda trajs, **kw: bild_amd.exact_dwell_first_contact(trajs, model, prior, 1, **kw)}
    for kind, call in calls.items():
        batch = call(xs)
        assert all(np.isfinite(r.log_evidence) for r in batch)
        assert all(same(a, b, kind) for a, b in zip(batch, call(xs)))
        order = [2, 0, 3, 1]
        permuted = call([xs[i] for i in order])
        assert all(same(permuted[j], batch[i], kind) for j, i in enumerate(order))
        for x, r in zip(xs, batch):
            alone = call(x)
            if kind == 'counts':        # alone, k_max is the trajectory's own T - 1: the levels it has are the batch's, the others -inf
                assert np.array_equal(alone.log_count, r.log_count[:len(x)]) and np.all(r.log_count[len(x):] == -np.inf)
                assert alone.log_evidence == r.log_evidence and alone.log_tail == r.log_tail == -np.inf
            else:
                assert same(alone, r, kind)
        # one trajectory per chunk, and two: a trajectory's share of a chunk, S = 2 and 193 frames (csrc/gauss_dwellevent.cpp)
        slot = 2 * 194
        forward = slot * 40 + 2 * 8 + 8 + 193
        per_traj = forward + (2 * slot + 193 * 2) * 8 if kind == 'counts' else 2 * forward + 2 * slot * 8 + 194 * 8
        for scratch in (1, 2 * per_traj + 8):
            assert all(same(a, b, kind) for a, b in zip(batch, call(xs, scratch_bytes=scratch)))
    complete, cut = calls['counts'](xs), calls['counts'](xs, k_max=5)
    for a, b in zip(complete, cut):
        assert b.log_count.shape == (6, 2) and np.array_equal(a.log_count[:6], b.log_count) and np.isfinite(b.log_tail)


def test_ragged_batch_against_oracle():
    """
    `dwell_cases.ragged_case` in one call: four states, non-geometric tables, T = 1 ... 257, so that five of the six have ld, slot
    and p.ntile that are not their own.  Each trajectory alone is held to its own oracle answer, and the batch is the
    trajectories alone bit for bit, whole and with one trajectory a chunk.  Six trajectories are two workgroups of
    dwell_contact_kernel, the second with two waves.
    """
    model, prior, xs, _ = DC.ragged_case()
    S, Tm = 4, max(len(x) for x in xs)
    refs = bild_amd.exact_dwell(xs, model, prior, marginals=False)
    calls = {'counts': lambda trajs, **kw: bild_amd.exact_dwell_switch_counts(trajs, model, prior, **kw)}
    for target in DEC.RAGGED_TARGETS:
        calls[target] = lambda trajs, target=target, **kw: bild_amd.exact_dwell_first_contact(trajs, model, prior, target, **kw)
    worst, seconds = {}, 0.0
    for key, call in calls.items():
        kind = 'counts' if key == 'counts' else 'contact'
        batch = call(xs)
        assert len(batch) == len(xs)
        for j, (x, r, ref) in enumerate(zip(xs, batch, refs)):
            T = len(x)
            alone = call(x)
            if kind == 'counts':
                devs = hold_counts(alone, DEC.ragged_counts(j), ref, S, T, None, ('ragged', j))
                seconds = max(seconds, DEC.ORACLE_SECONDS['ragged', j, 'counts'])
                # alone, k_max is the trajectory's own T - 1: the levels it has are the batch's, the others -inf
                assert r.log_count.shape == (Tm, S) and np.array_equal(alone.log_count, r.log_count[:T]) and np.all(r.log_count[T:] == -np.inf)
                assert alone.log_evidence == r.log_evidence and alone.log_tail == r.log_tail == -np.inf and r.n_nan_windows == 0
            else:
                devs = hold_contact(alone, DEC.ragged_contact(j, key), ref, key, T, ('ragged', j, key))
                seconds = max(seconds, DEC.ORACLE_SECONDS['ragged', j, key])
                assert same(alone, r, kind), (j, key)
            for name, v in devs.items():
                worst[name] = max(worst.get(name, 0.0), v)
        assert all(same(a, b, kind) for a, b in zip(batch, call(xs, scratch_bytes=1))), key
    print(f"ragged: slowest oracle answer {seconds:.2f} s; " + ', '.join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert seconds < 20


def test_first_contact_of_nine_trajectories():
    """
    nine trajectories in one call are three workgroups of dwell_contact_kernel (a wave per trajectory, four to a workgroup), the
    last with a single wave: each equals itself alone bit for bit, in one chunk and with two trajectories a chunk
    """
    model, prior, xs = DEC.nine_trajectories()
    assert len(xs) == 9
    S, Tm = 4, max(len(x) for x in xs)
    # a trajectory's share of a chunk (csrc/gauss_dwellevent.cpp), as `test_bit_identity` derives it: both forward tables, beta
    # and gamma, and the row of first
    slot = S * (Tm + 1)
    forward = slot * 40 + 2 * 8 + 8 + Tm
    per_traj = 2 * forward + 2 * slot * 8 + (Tm + 1) * 8
    for target in DEC.RAGGED_TARGETS:
        alone = [bild_amd.exact_dwell_first_contact(x, model, prior, target) for x in xs]
        assert all(np.isfinite(a.log_evidence) and not np.any(np.isnan(a.log_first)) for a in alone)
        for scratch in (0, 2 * per_traj + 8):
            batch = bild_amd.exact_dwell_first_contact(xs, model, prior, target, scratch_bytes=scratch)
            assert len(batch) == 9 and all(same(a, b, 'contact') for a, b in zip(alone, batch)), (target, scratch)


def test_trajectory_without_a_profile():
    rng = np.random.default_rng(3)
    model = C.random_model(rng, 2, 64)
    xs = [C.random_traj(rng, 50), C.random_traj(rng, 56)]
    no = DC.prior_of('impossible', rng, 2, 60, 50)
    r, c = bild_amd.exact_dwell_switch_counts(xs, model, no), bild_amd.exact_dwell_first_contact(xs, model, no, 1)
    assert r[0].log_evidence == -np.inf and np.all(np.isnan(r[0].log_count)) and np.isnan(r[0].log_tail)
    assert c[0].log_evidence == -np.inf and np.all(np.isnan(c[0].log_first)) and np.isnan(c[0].log_never)
    # 56 frames: the one segment in state 0 survives, no switch and no contact with state 1
    assert abs(r[1].log_count[0, 0]) < TOL_LOG and np.all(r[1].log_count.ravel()[1:] == -np.inf)
    assert abs(c[1].log_never) < TOL_LOG and np.all(c[1].log_first == -np.inf)


def test_c_abi_refusals():
    rng = np.random.default_rng(51)
    model = C.random_model(rng, 2, 40)
    x = C.random_traj(rng, 30)
    ts = model.trajset(x)
    p = DC.symmetric_chain(0.1, 30)
    good = (p.log_init, p.log_jump, p.log_dwell, p.log_surv)
    calls = (lambda *a, **k: _lib.gauss_dwell_switch_counts(model.handle(), ts, *a, k.pop('k_max', 29), **k),
             lambda *a, **k: _lib.gauss_dwell_first_contact(model.handle(), ts, *a, k.pop('target', 2), **k))
    for call in calls:
        call(*good)
        with pytest.raises(_lib.BildAmdError, match='more than the L = 29') as e:      # L shorter than the trajectory
            call(good[0], good[1], good[2][:, :29], good[3][:, :29])
        assert e.value.code == _lib.ERR_INVALID
        for i in range(4):                              # a NaN entry anywhere
            args = [a.copy() for a in good]
            args[i][(0,) * args[i].ndim] = np.nan
            with pytest.raises(_lib.BildAmdError) as e:
                call(*args)
            assert e.value.code == _lib.ERR_INVALID
        with pytest.raises(_lib.BildAmdError, match='negative'):
            call(*good, scratch_bytes=-1)
    for k_max in (-1, 30):
        with pytest.raises(_lib.BildAmdError, match='k_max') as e:
            calls[0](*good, k_max=k_max)
        assert e.value.code == _lib.ERR_INVALID
    for target in (0, 3, 4, 5):                         # empty, every state, a state the model does not have
        with pytest.raises(_lib.BildAmdError, match='target') as e:
            calls[1](*good, target=target)
        assert e.value.code == _lib.ERR_INVALID

    arrs = [_lib.f64(a) for a in good]

    def raw(name, extra, T_max=30, flags=0, scratch=0, out=True):
        spec = {'switch_counts': _lib.DwellSwitchCountsOut, 'first_contact': _lib.DwellFirstContactOut}[name]()
        return getattr(_lib.lib(), 'bild_gauss_dwell_' + name)(model.handle()._h, ts._h, 30, *[_lib.dptr(a) for a in arrs], T_max, extra, flags,
                                                              scratch, ctypes.byref(spec) if out else None)
    for name, extra in (('switch_counts', 29), ('first_contact', 1)):
        assert raw(name, extra) == _lib.OK       # (every output NULL: nothing is written)
        assert raw(name, extra, flags=2) == _lib.ERR_INVALID and raw(name, extra, scratch=-1) == _lib.ERR_INVALID
        assert raw(name, extra, T_max=29) == _lib.ERR_INVALID and raw(name, extra, out=False) == _lib.ERR_INVALID
    five = C.random_model(rng, 5, 40)
    p5 = DC.make_prior('markov', rng, 5, 30)
    ts5 = five.trajset(x)
    for call in (lambda: _lib.gauss_dwell_switch_counts(five.handle(), ts5, p5.log_init, p5.log_jump, p5.log_dwell, p5.log_surv, 3),
                 lambda: _lib.gauss_dwell_first_contact(five.handle(), ts5, p5.log_init, p5.log_jump, p5.log_dwell, p5.log_surv, 1)):
        with pytest.raises(_lib.BildAmdError, match='at most 4') as e:
            call()
        assert e.value.code == _lib.ERR_UNSUPPORTED
