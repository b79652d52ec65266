"""
The exact posterior of the number of visits to a set of states under a dwell-time prior on the GPU
(bild_amd.exact.exact_dwell_visits, csrc/gauss_dwellvis.hip): against the NumPy oracle
tests/dwell_visit_oracle.py, with all the mass at the seam between two tiles of n, cut by n_max, against `exact_dwell`,
`exact_dwell_first_contact` and `exact_dwell_switch_counts` on the device, the identities at T = 1000, the histogram of
`exact_dwell_draw` as an independent device route, the bit-identity properties and the refusals of the C call.
"""
import ctypes

import numpy as np
import pytest
from scipy.special import logsumexp

import bild_amd
import dwell_cases as DC
import dwell_event_cases as DEC
import dwell_visit_cases as DVC
import segment_cases as C
from bild_amd import _lib

pytestmark = pytest.mark.gpu

# The issue's bounds, the siblings' device bounds: a finite log within 1e-10, -inf exactly; 1e-9 at T = 1000.
# Worst seen on these cases: tests/README_dwell_visits.md.
TOL_LOG, TOL_LOG_T1000 = 1e-10, 1e-9


def log_deviation(got, want, what):
    """ the worst |got - want| over the finite logs; -inf must come back as -inf """
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    assert got.shape == want.shape and not np.any(np.isnan(got)) and not np.any(np.isnan(want)), what
    assert np.array_equal(got == -np.inf, want == -np.inf), what
    fin = want > -np.inf
    return float(np.max(np.abs(got[fin] - want[fin]), initial=0.0))


def log_pmf(r):
    """ log P(N = n | data) without leaving the logs """
    return logsumexp(r.log_visits, axis=1)


def tail_deviation(got, want, what, complete):
    """
    log_tail against the oracle's: -inf exactly at a complete n_max, where it is -inf by construction and not by arithmetic;
    within the bar of the logs where the oracle's tail exceeds 1e-6.  Below that the tail is a difference from 1, and either
    side may round to 0: the kept logs lie within TOL_LOG of the oracle's, so the kept probabilities and their sum, which is
    at most 1, within TOL_LOG of the oracle's, and the two tails are compared as probabilities to that.
    """
    if complete:
        assert got == want == -np.inf, what
        return 0.0
    if np.exp(want) > 1e-6:
        return abs(got - want)
    assert not np.isnan(got) and abs(np.exp(got) - np.exp(want)) < TOL_LOG, what
    return 0.0


def sibling_deviations(x, model, prior, target, nan, r=None):
    """ section 30's identities between the complete call and its siblings on the device, as deviations of logs: (devs, r) """
    S, T = model.msd.shape[0], len(x)
    inside = np.isin(np.arange(S), target)
    r = bild_amd.exact_dwell_visits(x, model, prior, target, nan=nan) if r is None else r
    ref = bild_amd.exact_dwell(x, model, prior, nan=nan)
    post = ref.log_marginal_posterior
    assert r.log_evidence == ref.log_evidence and r.log_tail == -np.inf and r.log_visits.shape == ((T + 1) // 2 + 1, S)
    lp = log_pmf(r)
    mean = np.exp(post[inside, 0]).sum() + ref.expected_jumps[np.ix_(~inside, inside)].sum()
    devs = {'sum pmf = 1': abs(logsumexp(lp)),
            'pmf[0] = never in G': log_deviation(lp[0], bild_amd.exact_dwell_first_contact(x, model, prior, target, nan=nan).log_never, 'pmf[0]'),
            'sum_n visits = last marginal': log_deviation(logsumexp(r.log_visits, axis=0), post[:, T - 1], 'columns'),
            'mean = starts in G + jumps into G': abs(np.log(r.mean()) - np.log(mean))}
    if S == 2:
        # the number of segments of a state from the switch counts: formed in linear space, where a log below -745 is 0
        seg = bild_amd.exact_dwell_switch_counts(x, model, prior, nan=nan).segment_count_pmf(target[0])
        pmf = r.pmf()
        assert len(seg) >= len(pmf) and np.all(seg[len(pmf):] == 0)
        seg = seg[:len(pmf)]
        big = seg > 1e-280
        assert np.all(pmf[~big] <= 1e-279) and np.array_equal(pmf == 0, seg == 0)
        devs['pmf = segment_count_pmf'] = float(np.max(np.abs(np.log(pmf[big]) - np.log(seg[big])), initial=0.0))
    return devs, r


@pytest.mark.parametrize('case', DVC.ORACLE_CASES, ids=DVC.case_id)
def test_against_oracle_and_siblings(case):
    S, T, missing, _, nan, targets, _ = case
    model, x, prior, W, F = DVC.oracle_case(*case[:4])
    answers = DVC.oracle_answer(case)
    ref = bild_amd.exact_dwell(x, model, prior, marginals=False, nan=nan)
    for target in targets + (() if S != 2 else ((0,),)):
        r = bild_amd.exact_dwell_visits(x, model, prior, target, nan=nan)
        assert r.target == target and r.log_visits.shape == ((T + 1) // 2 + 1, S)
        assert r.n_nan_windows == ref.n_nan_windows and (r.n_nan_windows > 0) == (missing == 'order0_gap')
        assert np.array_equal(r.log_evidence, ref.log_evidence, equal_nan=True)         # bit for bit `exact_dwell`'s
        if np.isnan(ref.log_evidence):
            assert nan == 'propagate' and np.all(np.isnan(r.log_visits)) and np.isnan(r.log_tail)
            continue
        devs = {}
        if target in answers:       # (the other state of two: the identities alone)
            want = answers[target]
            assert r.n_nan_windows == want['n_nan_windows']
            devs = {'logev': abs(r.log_evidence - want['logev']), 'log_visits': log_deviation(r.log_visits, want['log_visits'], target)}
            assert r.log_tail == want['log_tail'] == -np.inf
        sib, _ = sibling_deviations(x, model, prior, target, nan, r)
        pmf = r.pmf()
        print(f"{DVC.case_id(case)} {target}: oracle {DVC.ORACLE_SECONDS[case]:.2f} s, {int(np.sum(pmf > 1e-12))} bins above 1e-12, mean "
              f"{r.mean():.2f}, sd {np.sqrt(r.var()):.2f}, interval {r.interval()}; "
              + ', '.join(f"{k} {v:.1e}" for k, v in {**devs, **sib}.items()))
        for name, v in {**devs, **sib}.items():
            assert v < TOL_LOG, (case, target, name, v)
    assert DVC.ORACLE_SECONDS[case] < 20


def hold_visits(r, want, ref, target, S, rows, what):
    """ a `DwellVisits` against the oracle's answer and `exact_dwell`'s evidence: {name: deviation}, the bars asserted """
    assert r.target == target and r.log_visits.shape == (rows, S), what
    assert r.n_nan_windows == want['n_nan_windows'] == ref.n_nan_windows == 0, what
    assert np.isfinite(ref.log_evidence) and r.log_evidence == ref.log_evidence, what       # bit for bit `exact_dwell`'s
    devs = {'logev': abs(r.log_evidence - want['logev']), 'log_visits': log_deviation(r.log_visits, want['log_visits'][:rows], what),
            'log_tail': tail_deviation(r.log_tail, want['log_tail'], what, len(want['log_visits']) - 1 >= (len(r.traj) + 1) // 2)}
    assert np.all(want['log_visits'][rows:] == -np.inf), what
    if len(want['log_visits']) - 1 >= (len(r.traj) + 1) // 2:
        devs['sum pmf = 1'] = abs(logsumexp(log_pmf(r)))
    for name, v in devs.items():
        assert v < TOL_LOG, (what, name, v)
    return devs


@pytest.mark.parametrize('item', DVC.WIDE_CASES, ids=DVC.wide_id)
def test_against_oracle_wide(item):
    """ four states, T > 256 (the third tile of n), non-geometric tables and the hard priors, whose -inf pattern is compared """
    case, target = item
    S, T = case[:2]
    model, x, prior, _, _ = DC.oracle_case(case)
    want = DVC.wide_answer(case, target)
    ref = bild_amd.exact_dwell(x, model, prior, marginals=False)
    r = bild_amd.exact_dwell_visits(x, model, prior, target)
    devs = hold_visits(r, want, ref, target, S, (T + 1) // 2 + 1, item)
    print(f"{DVC.wide_id(item)}: oracle {DVC.ORACLE_SECONDS[case, target, None]:.2f} s, {int(np.sum(r.pmf() > 1e-12))} bins above 1e-12, "
          f"{int(np.sum(r.log_visits == -np.inf))} entries at -inf, mean {r.mean():.2f}; " + ', '.join(f"{k} {v:.1e}" for k, v in devs.items()))
    assert DVC.ORACLE_SECONDS[case, target, None] < 20


@pytest.mark.parametrize('T', DVC.SEAM_T)
def test_all_the_mass_at_the_tile_seam(T):
    """
    Under the `flip` prior the states alternate every frame, so the posterior of the visits to state 1 has its mass in two
    entries, listed in `dwell_visit_cases.SEAM_MASS`: around the rows 62 | 63, where the kernel's second tile of n begins and the
    jump mix takes row 62 from the lane that carries it, and 63 | 64.  n_max = 62, 63 and 64 cut there: what enters G from
    row n_max is dropped, and log_tail holds it.
    """
    model, x, prior, _, _ = DVC.seam_case(T)
    ref = bild_amd.exact_dwell(x, model, prior, marginals=False)
    full = None
    for n_max in DVC.SEAM_N_MAX:
        want = DVC.seam_answer(T, n_max)
        r = bild_amd.exact_dwell_visits(x, model, prior, 1, n_max=n_max)
        rows = min((T + 1) // 2 if n_max is None else n_max, (T + 1) // 2) + 1
        devs = hold_visits(r, want, ref, (1,), 2, rows, (T, n_max))
        finite = tuple(map(tuple, np.argwhere(r.log_visits > -np.inf).tolist()))
        assert finite == tuple(e for e in DVC.SEAM_MASS[T] if e[0] < rows), (T, n_max)
        full = r if n_max is None else full
        assert np.array_equal(r.log_visits, full.log_visits[:rows])
        print(f"T = {T}, n_max = {n_max}: finite at {finite}, log_tail {r.log_tail!r}; " + ', '.join(f"{k} {v:.1e}" for k, v in devs.items()))
    # the issue's numbers
    cut = lambda n: bild_amd.exact_dwell_visits(x, model, prior, 1, n_max=n)
    if T in (128, 129):
        r = cut(63)
        assert np.all(r.log_visits == -np.inf) and r.log_tail == 0.0
    if T == 127:
        assert abs(np.exp(cut(63).log_tail) - 0.00131) < 1e-5
    if T == 129:
        assert abs(np.exp(cut(64).log_tail) - 0.9613) < 1e-4


@pytest.mark.parametrize('item', DVC.CUT_CASES, ids=lambda item: DEC.wide_id(item))
def test_n_max_cuts_on_soft_priors(item):
    """ the kept rows are the complete call's bit for bit, and log_tail is the oracle's """
    case, n_max = item
    S, T = case[:2]
    target = DVC.CUT_TARGETS[S]
    model, x, prior, _, _ = DC.oracle_case(case)
    ref = bild_amd.exact_dwell(x, model, prior, marginals=False)
    full = bild_amd.exact_dwell_visits(x, model, prior, target)
    r = bild_amd.exact_dwell_visits(x, model, prior, target, n_max=n_max)
    assert n_max <= (T + 1) // 2 and r.log_visits.shape == (n_max + 1, S) and r.log_evidence == full.log_evidence
    assert np.array_equal(r.log_visits, full.log_visits[:n_max + 1])
    want = DVC.wide_answer(case, target, n_max)
    devs = hold_visits(r, want, ref, target, S, n_max + 1, item)
    print(f"{DEC.wide_id(item)} {target}: the oracle's tail {np.exp(want['log_tail']):.3e}, the device's {np.exp(r.log_tail):.3e}; "
          + ', '.join(f"{k} {v:.1e}" for k, v in devs.items()))
    assert DVC.ORACLE_SECONDS[case, target, n_max] < 20


FIELDS = ('log_evidence', 'n_nan_windows', 'log_visits', 'log_tail')


def same(a, b):
    return all(np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True) for f in FIELDS)


def test_ragged_batch_against_oracle():
    """
    `dwell_cases.ragged_case` in one call: four states, non-geometric tables, T = 1 ... 257, so that five of the six have a
    stride of alpha, a row length and a last row that are not their own, and end before the chunk's last end frame.  Each
    trajectory of the batch is held to its own oracle answer, and the batch is the trajectories alone bit for bit, whole and
    with one trajectory a chunk.
    """
    model, prior, xs, _ = DC.ragged_case()
    refs = bild_amd.exact_dwell(xs, model, prior, marginals=False)
    worst, seconds = {}, 0.0
    for target in DEC.RAGGED_TARGETS:
        batch = bild_amd.exact_dwell_visits(xs, model, prior, target)
        assert len(batch) == len(xs)
        for j, (x, r, ref) in enumerate(zip(xs, batch, refs)):
            devs = hold_visits(r, DVC.ragged_answer(j, target), ref, target, 4, (len(x) + 1) // 2 + 1, ('ragged', j, target))
            seconds = max(seconds, DVC.ORACLE_SECONDS['ragged', j, target])
            for name, v in devs.items():
                worst[name] = max(worst.get(name, 0.0), v)
            assert same(bild_amd.exact_dwell_visits(x, model, prior, target), r), (j, target)
        assert all(same(a, b) for a, b in zip(batch, bild_amd.exact_dwell_visits(xs, model, prior, target, scratch_bytes=1))), target
    print(f"ragged: slowest oracle answer {seconds:.2f} s; " + ', '.join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert seconds < 20


def test_identities_at_T1000():
    """ `test_gpu_dwell_occupancy.test_identities_at_T1000`'s data; both states as the target """
    T = 1000
    rng = np.random.default_rng(31)
    model = C.random_model(rng, 2, T + 8, orders=np.ones((2, 3), dtype=int), d=3)
    x = C.random_traj(rng, T, (100, 500, 501), d=3)
    prior = bild_amd.DwellPrior.markov([[0.98, 0.02], [0.05, 0.95]], [0.6, 0.4], n=T)
    for target in ((1,), (0,)):
        devs, r = sibling_deviations(x, model, prior, target, 'propagate')
        assert r.log_visits.shape == (T // 2 + 1, 2) and r.n_nan_windows == 0 and np.isfinite(r.log_evidence)
        assert not np.any(np.isnan(r.log_visits))
        print(f"{target}: mean {r.mean():.3f} visits, sd {np.sqrt(r.var()):.3f}, interval {r.interval()}, {int(np.sum(r.pmf() > 1e-12))} bins "
              f"above 1e-12; " + ', '.join(f"{k}: {v:.1e}" for k, v in devs.items()))
        assert all(v < TOL_LOG_T1000 for v in devs.values()), devs


def test_against_the_histogram_of_the_draws():
    """ every bin within 5 sqrt(p (1 - p) / n) + 1 / n of the exact p: the binomial bound, nothing fitted """
    T, n = 130, 20000
    rng = np.random.default_rng(77)
    model = C.random_model(rng, 2, T + 8)
    x = C.random_traj(rng, T, (64,))
    prior = DC.make_prior('markov', rng, 2, T)
    draws = bild_amd.exact_dwell(x, model, prior).draw(n, seed=5)
    p = bild_amd.exact_dwell_visits(x, model, prior, 1).pmf()
    count = draws.visits(1)
    assert count.shape == (n,) and count.min() >= 0 and count.max() <= (T + 1) // 2 and len(p) == (T + 1) // 2 + 1
    hist = np.bincount(count, minlength=len(p)) / n
    slack = np.abs(hist - p) - (5 * np.sqrt(p * (1 - p) / n) + 1 / n)
    print(f"{len(p)} bins, {int(np.sum(p > 1e-12))} above 1e-12, largest |histogram - exact| {np.max(np.abs(hist - p)):.2e}, closest to its "
          f"bound by {-np.max(slack):.2e}")
    assert np.all(slack <= 0), (int(np.argmax(slack)), float(np.max(slack)))


def test_bit_identity():
    rng = np.random.default_rng(41)
    model = C.random_model(rng, 2, 200)
    xs = [C.random_traj(rng, T, missing) for T, missing in ((40, ()), (65, (9,)), (193, (63, 65)), (65, ()))]
    prior = DC.make_prior('markov', rng, 2, 193)

    def call(trajs, **kw):
        return bild_amd.exact_dwell_visits(trajs, model, prior, 1, **kw)
    batch = call(xs)
    assert all(np.isfinite(r.log_evidence) and r.log_visits.shape == ((len(x) + 1) // 2 + 1, 2) for x, r in zip(xs, batch))
    assert all(same(a, b) for a, b in zip(batch, call(xs)))
    order = [2, 0, 3, 1]
    permuted = call([xs[i] for i in order])
    assert all(same(permuted[j], batch[i]) for j, i in enumerate(order))
    assert all(same(call(x), r) for x, r in zip(xs, batch))
    # one trajectory per chunk, and two: a trajectory's share of a chunk, S = 2, 193 frames and 98 rows (csrc/gauss_dwellvis.cpp)
    slot = 2 * 194
    forward = slot * 40 + 2 * 8 + 8 + 193
    per_traj = forward + (2 * 193 * 98 + 2 * 98) * 8
    for scratch in (1, 2 * per_traj + 8):
        assert all(same(a, b) for a, b in zip(batch, call(xs, scratch_bytes=scratch)))
    # a cut batch keeps the rows of the complete one
    cut = call(xs, n_max=30)
    assert all(np.array_equal(c.log_visits, r.log_visits[:31]) and c.log_evidence == r.log_evidence for c, r in zip(cut, batch))
    assert [c.log_visits.shape[0] for c in cut] == [21, 31, 31, 31] and cut[0].log_tail == -np.inf


def test_trajectory_without_a_profile():
    rng = np.random.default_rng(3)
    model = C.random_model(rng, 2, 64)
    xs = [C.random_traj(rng, 50), C.random_traj(rng, 56)]
    no = DC.prior_of('impossible', rng, 2, 60, 50)
    r = bild_amd.exact_dwell_visits(xs, model, no, 1)
    assert r[0].log_evidence == -np.inf and r[0].log_visits.shape == (26, 2) and np.all(np.isnan(r[0].log_visits)) and np.isnan(r[0].log_tail)
    assert r[0].n_nan_windows == 0
    # 56 frames: the one segment in state 0 survives, and state 1 is never visited
    assert r[1].log_visits.shape == (29, 2) and r[1].log_tail == -np.inf
    assert abs(r[1].log_visits[0, 0]) < TOL_LOG and np.all(r[1].log_visits.ravel()[1:] == -np.inf)
    other = bild_amd.exact_dwell_visits(xs, model, no, 0, n_max=3)
    assert np.all(np.isnan(other[0].log_visits)) and np.isnan(other[0].log_tail) and other[0].log_evidence == -np.inf
    assert other[1].log_visits.shape == (4, 2) and abs(other[1].log_visits[1, 0]) < TOL_LOG
    assert np.all(np.delete(other[1].log_visits.ravel(), 2) == -np.inf) and abs(np.exp(other[1].log_tail)) < 1e-14


def test_c_abi_refusals():
    rng = np.random.default_rng(51)
    model = C.random_model(rng, 2, 40)
    x = C.random_traj(rng, 30)
    ts = model.trajset(x)
    p = DC.symmetric_chain(0.1, 30)
    good = (p.log_init, p.log_jump, p.log_dwell, p.log_surv)

    def call(*a, **k):
        return _lib.gauss_dwell_visits(model.handle(), ts, *a, k.pop('target', 2), k.pop('n_max', 15), **k)
    res = call(*good)
    assert res['log_visits'].shape == (1, 16, 2) and abs(np.exp(res['log_visits']).sum() - 1) < TOL_LOG and res['log_tail'][0] == -np.inf
    wide = call(*good, n_max=40)        # rows beyond (T + 1) // 2 are -inf
    assert np.array_equal(wide['log_visits'][:, :16], res['log_visits']) and np.all(wide['log_visits'][:, 16:] == -np.inf)
    assert wide['log_tail'][0] == -np.inf
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
    with pytest.raises(_lib.BildAmdError, match='n_max = -1 is negative') as e:
        call(*good, n_max=-1)
    assert e.value.code == _lib.ERR_INVALID
    for target in (0, 3, 4, 5):                         # empty, every state, a state the model does not have
        with pytest.raises(_lib.BildAmdError, match='target') as e:
            call(*good, target=target)
        assert e.value.code == _lib.ERR_INVALID

    arrs = [_lib.f64(a) for a in good]

    def raw(target=1, n_max=15, T_max=30, flags=0, scratch=0, out=True):
        spec = _lib.DwellVisitsOut()
        return _lib.lib().bild_gauss_dwell_visits(model.handle()._h, ts._h, 30, *[_lib.dptr(a) for a in arrs], T_max, n_max, target, flags,
                                                  scratch, ctypes.byref(spec) if out else None)
    assert raw() == _lib.OK and raw(n_max=0) == _lib.OK         # (every output NULL: nothing is written)
    assert raw(flags=2) == _lib.ERR_INVALID and raw(scratch=-1) == _lib.ERR_INVALID
    assert raw(T_max=29) == _lib.ERR_INVALID and raw(out=False) == _lib.ERR_INVALID
    assert raw(target=0) == _lib.ERR_INVALID and raw(target=3) == _lib.ERR_INVALID and raw(target=4) == _lib.ERR_INVALID
    assert raw(n_max=-1) == _lib.ERR_INVALID
    one = C.random_model(rng, 1, 40)                    # one state has no proper subset
    p1 = DC.make_prior('markov', rng, 1, 30)
    ts1 = one.trajset(x)
    for target in (0, 1):
        with pytest.raises(_lib.BildAmdError, match='target') as e:
            _lib.gauss_dwell_visits(one.handle(), ts1, p1.log_init, p1.log_jump, p1.log_dwell, p1.log_surv, target, 3)
        assert e.value.code == _lib.ERR_INVALID
    five = C.random_model(rng, 5, 40)
    p5 = DC.make_prior('markov', rng, 5, 30)
    ts5 = five.trajset(x)
    with pytest.raises(_lib.BildAmdError, match='at most 4') as e:
        _lib.gauss_dwell_visits(five.handle(), ts5, p5.log_init, p5.log_jump, p5.log_dwell, p5.log_surv, 1, 3)
    assert e.value.code == _lib.ERR_UNSUPPORTED
