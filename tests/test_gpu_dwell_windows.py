"""
The exact window support under a dwell-time prior on the GPU (bild_amd.exact.exact_dwell_windows, csrc/gauss_dwellwin.hip,
DESIGN.md section 29): against the NumPy oracle tests/dwell_window_oracle.py on windows that place the edges of the kernel's
tiles, against `exact_dwell`, `exact_dwell_first_contact` and `exact_dwell_occupancy` on the device through section 29's
identities, also at T = 1000, the frequencies over `exact_dwell_draw` as an independent device route, the bit-identity
properties, `map_support` at T = 1000 and the refusals of the C call.  Deviations seen: tests/README_dwell_windows.md.
"""
import ctypes

import numpy as np
import pytest
from scipy.special import logsumexp

import bild_amd
import dwell_cases as DC
import dwell_window_cases as DWC
import segment_cases as C
from bild_amd import _lib

pytestmark = pytest.mark.gpu

# The issue's bounds, the siblings' device bounds: a finite log within 1e-10, -inf exactly; 1e-9 at T = 1000.
TOL_LOG, TOL_LOG_T1000 = 1e-10, 1e-9


def log_deviation(got, want, what):
    """ the worst |got - want| over the finite logs; -inf must come back as -inf """
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    assert got.shape == want.shape and not np.any(np.isnan(got)) and not np.any(np.isnan(want)), what
    assert np.array_equal(got == -np.inf, want == -np.inf), what
    fin = want > -np.inf
    return float(np.max(np.abs(got[fin] - want[fin]), initial=0.0))


@pytest.mark.parametrize('case', DWC.ORACLE_CASES, ids=DWC.case_id)
def test_against_oracle(case):
    S, T, missing, _, nan, _ = case
    model, x, prior, W, F = DWC.oracle_case(*case[:4])
    windows, want = DWC.case_windows(case), DWC.oracle_answer(case)
    assert 0 < len(windows) <= DWC.MAX_WINDOWS
    ref = bild_amd.exact_dwell(x, model, prior, marginals=False, nan=nan)
    r = bild_amd.exact_dwell_windows(x, model, prior, windows, nan=nan)
    assert r.windows.tolist() == [list(w[:2]) for w in windows] and r.targets == tuple(w[2] for w in windows)
    assert r.log_all.shape == (len(windows),)
    assert r.n_nan_windows == want['n_nan_windows'] == ref.n_nan_windows and (r.n_nan_windows > 0) == (missing == 'order0_gap')
    assert np.array_equal(r.log_evidence, ref.log_evidence, equal_nan=True)         # bit for bit `exact_dwell`'s
    if np.isnan(want['logev']):
        assert nan == 'propagate' and np.isnan(r.log_evidence) and np.all(np.isnan(r.log_all))
        return
    devs = {'logev': abs(r.log_evidence - want['logev']), 'log_all': log_deviation(r.log_all, want['log_all'], case)}
    print(f"{DWC.case_id(case)}: oracle {DWC.ORACLE_SECONDS[case]:.2f} s, {len(windows)} windows, log_all from {np.min(r.log_all):.3g} to "
          f"{np.max(r.log_all):.3g}; " + ', '.join(f"{k} {v:.1e}" for k, v in devs.items()))
    for name, v in devs.items():
        assert v < TOL_LOG, (case, name, v)


def hold_windows(r, want, ref, windows, what):
    """ a `DwellWindowSupport` against the oracle's answer and `exact_dwell`'s evidence: {name: deviation}, the bars asserted """
    assert r.windows.tolist() == [list(w[:2]) for w in windows] and r.targets == tuple(w[2] for w in windows), what
    assert r.log_all.shape == (len(windows),) and r.n_nan_windows == want['n_nan_windows'] == ref.n_nan_windows == 0, what
    assert np.isfinite(ref.log_evidence) and r.log_evidence == ref.log_evidence, what       # bit for bit `exact_dwell`'s
    devs = {'logev': abs(r.log_evidence - want['logev']), 'log_all': log_deviation(r.log_all, want['log_all'], what)}
    for name, v in devs.items():
        assert v < TOL_LOG, (what, name, v)
    return devs


@pytest.mark.parametrize('item', DWC.WIDE_CASES, ids=DWC.wide_id)
def test_against_oracle_wide(item):
    """ four states, T > 256, non-geometric tables and the hard priors (tests/README_dwell_windows.md, "The wide cases") """
    model, x, prior, _, _ = DC.oracle_case(item[0])
    windows, want = DWC.wide_windows(item), DWC.wide_answer(item)
    assert 0 < len(windows) <= DWC.MAX_WINDOWS
    ref = bild_amd.exact_dwell(x, model, prior, marginals=False)
    r = bild_amd.exact_dwell_windows(x, model, prior, windows)
    devs = hold_windows(r, want, ref, windows, item)
    fin = r.log_all[r.log_all > -np.inf]
    print(f"{DWC.wide_id(item)}: oracle {DWC.ORACLE_SECONDS[item]:.2f} s, {len(windows)} windows, {len(windows) - len(fin)} at -inf, finite log_all "
          f"from {np.min(fin, initial=0.0):.3g} to {np.max(fin, initial=-np.inf):.3g}; " + ', '.join(f"{k} {v:.1e}" for k, v in devs.items()))
    assert DWC.ORACLE_SECONDS[item] < 20


def test_ragged_batch_against_oracle():
    """
    `dwell_cases.ragged_case` in one call: four states, non-geometric tables, T = 1 ... 257, so that five of the six have ld, slot
    and kappa offsets that are not their own.  Each trajectory of the batch is held to its own oracle answer on the spans that
    fit it, and the batch is the trajectories alone bit for bit, whole and with one trajectory a chunk.
    """
    model, prior, xs, _ = DC.ragged_case()
    ws = [DWC.ragged_windows(len(x)) for x in xs]
    assert [len(w) for w in ws][0] == 2 and all(ws)
    refs = bild_amd.exact_dwell(xs, model, prior, marginals=False)
    batch = bild_amd.exact_dwell_windows(xs, model, prior, ws)
    worst, seconds = {}, 0.0
    for j, (x, w, r, ref) in enumerate(zip(xs, ws, batch, refs)):
        devs = hold_windows(r, DWC.ragged_answer(j), ref, w, ('ragged', j))
        seconds = max(seconds, DWC.ORACLE_SECONDS['ragged', j])
        for name, v in devs.items():
            worst[name] = max(worst.get(name, 0.0), v)
        assert same(bild_amd.exact_dwell_windows(x, model, prior, w), r), j
    assert all(same(a, b) for a, b in zip(batch, bild_amd.exact_dwell_windows(xs, model, prior, ws, scratch_bytes=1)))
    print(f"ragged: slowest oracle answer {seconds:.2f} s, {sum(map(len, ws))} windows; " + ', '.join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert seconds < 20


def sibling_deviations(x, model, prior, target, nan, frames):
    """ section 29's identities between the call and its siblings on the device, as deviations of logs, from ONE window call """
    S, T = model.msd.shape[0], len(x)
    rest = tuple(s for s in range(S) if s not in target)
    starts = sorted({0, 1, T // 2} & set(range(T)))
    windows = [(t, t + 1, target) for t in frames] + [(0, T, target)] + [(u, v, target) for u in starts for v in range(u + 1, T + 1, max(T // 40, 1))]
    r = bild_amd.exact_dwell_windows(x, model, prior, windows, nan=nan)
    ref = bild_amd.exact_dwell(x, model, prior, nan=nan)
    assert r.log_evidence == ref.log_evidence
    n = len(frames)
    devs = {'one frame = marginal': log_deviation(r.log_all[:n], logsumexp(ref.log_marginal_posterior[list(target)][:, frames], axis=0), 'marginal'),
            'whole = never outside G': log_deviation(r.log_all[n], bild_amd.exact_dwell_first_contact(x, model, prior, rest, nan=nan).log_never, 'never'),
            'whole = pmf[T]': log_deviation(r.log_all[n], logsumexp(bild_amd.exact_dwell_occupancy(x, model, prior, target, nan=nan).log_occupancy[T]),
                                            'occupancy')}
    at = n + 1
    rise = 0.0
    for u in starts:        # for fixed u non-increasing in v
        m = len(range(u + 1, T + 1, max(T // 40, 1)))
        run = r.log_all[at:at + m]
        rise = max(rise, float(np.max(np.diff(run), initial=0.0)))
        at += m
    assert at == len(windows)
    devs['rise along v'] = rise
    return devs


# the two wide cases of four states across seams, as (case,): every frame at T = 129, every 8th at T = 257
WIDE_SIBLINGS = [((4, 129, (64, 100), 'markov'),), ((4, 257, (100,), 'nongeometric'),)]


@pytest.mark.parametrize('traj', [t for t in DWC.TRAJECTORIES if t[4] == 'omit' or t[2] != 'order0_gap'] + WIDE_SIBLINGS,
                         ids=lambda t: DWC.DEC.wide_id(t[0]) + '_wide' if len(t) == 1 else DWC.case_id(t + (0,))[:-6])
def test_identities_against_the_siblings(traj):
    if len(traj) == 1:
        (S, T, _, _), nan = traj[0], 'propagate'
        model, x, prior, _, _ = DC.oracle_case(traj[0])
    else:
        S, T, _, _, nan = traj
        model, x, prior, _, _ = DWC.oracle_case(*traj[:4])
    for target in DWC.TARGETS[S]:
        devs = sibling_deviations(x, model, prior, target, nan, list(range(0, T, 8 if T > 256 else 1)))
        print(f"{target}: " + ', '.join(f"{k}: {v:.1e}" for k, v in devs.items()))
        assert all(v < TOL_LOG for v in devs.values()), (traj, target, devs)


def t1000_case():
    T = 1000
    rng = np.random.default_rng(31)
    model = C.random_model(rng, 2, T + 8, orders=np.ones((2, 3), dtype=int), d=3)
    x = C.random_traj(rng, T, (100, 500, 501), d=3)
    return model, x, bild_amd.DwellPrior.markov([[0.98, 0.02], [0.05, 0.95]], [0.6, 0.4], n=T)


def test_identities_at_T1000():
    model, x, prior = t1000_case()
    devs = sibling_deviations(x, model, prior, (1,), 'propagate', list(range(0, 1000, 7)) + [999])
    print(', '.join(f"{k}: {v:.1e}" for k, v in devs.items()))
    assert all(v < TOL_LOG_T1000 for v in devs.values()), devs


def test_map_support_at_T1000():
    model, x, prior = t1000_case()
    ref = bild_amd.exact_dwell(x, model, prior)
    sup = ref.map_support()
    n_seg = len(sup.seg_start)
    assert sup.radii == (0, 2, 5) and sup.n_queries == 2 * n_seg + (n_seg - 1) * 3 * 2 and sup.log_evidence == ref.log_evidence
    states = np.asarray(ref.map_profile[:])
    assert sup.seg_start[0] == 0 and sup.seg_end[-1] == 1000 and np.array_equal(sup.seg_start[1:], sup.seg_end[:-1])
    assert all(np.all(states[a:b] == s) for a, b, s in zip(sup.seg_start, sup.seg_end, sup.seg_state))
    assert not np.any(np.isnan(sup.log_whole)) and not np.any(np.isnan(sup.log_absent))
    post = ref.log_marginal_posterior
    for i, (a, b, s) in enumerate(zip(sup.seg_start, sup.seg_end, sup.seg_state)):
        # all frames in s implies each frame in s; a frame in s implies some frame in s
        assert sup.log_whole[i] <= post[s, a:b].min() + TOL_LOG_T1000, i
        assert sup.p_present()[i] >= np.exp(post[s, a:b].max()) - TOL_LOG_T1000, i
    p = sup.p_switch_within
    assert p.shape == (n_seg - 1, 3) and np.all(p >= -TOL_LOG_T1000) and np.all(p <= 1 + TOL_LOG_T1000)
    assert np.all(np.diff(p, axis=1) >= -TOL_LOG_T1000)
    print(f"{n_seg} segments, {sup.n_queries} queries; p_whole from {sup.p_whole().min():.3g} to {sup.p_whole().max():.3g}, p_present from "
          f"{sup.p_present().min():.3g}; p_switch_within medians {np.median(p, axis=0)}")


def test_against_the_frequencies_of_the_draws():
    """ every query within 5 sqrt(p (1 - p) / n) + 1 / n of the exact p: the binomial bound, nothing fitted """
    T, n = 130, 20000
    rng = np.random.default_rng(77)
    model = C.random_model(rng, 2, T + 8)
    x = C.random_traj(rng, T, (64,))
    prior = DC.make_prior('markov', rng, 2, T)
    windows = DWC.windows_of(2, T)
    draws = bild_amd.exact_dwell(x, model, prior).draw(n, seed=5)
    p = bild_amd.exact_dwell_windows(x, model, prior, windows).p_all()
    freq = np.array([draws.all_in(u, v, target) for u, v, target in windows])
    slack = np.abs(freq - p) - (5 * np.sqrt(p * (1 - p) / n) + 1 / n)
    print(f"{len(windows)} windows, {int(np.sum(p > 1e-12))} above 1e-12, largest |frequency - exact| {np.max(np.abs(freq - p)):.2e}, closest to "
          f"its bound by {-np.max(slack):.2e}")
    assert np.all(slack <= 0), (windows[int(np.argmax(slack))], float(np.max(slack)))


FIELDS = ('log_evidence', 'n_nan_windows', 'log_all')


def same(a, b):
    return all(np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True) for f in FIELDS)


def some_windows(T):
    return [(0, 1, 1), (T - 1, T, 0), (0, T, 1), (3, T - 2, 0), (5, 30, 1), (10, T, 1), (12, 28, 0), (0, T - 1, 0)]


def test_bit_identity():
    rng = np.random.default_rng(41)
    model = C.random_model(rng, 2, 200)
    xs = [C.random_traj(rng, T, missing) for T, missing in ((40, ()), (65, (9,)), (193, (63, 65)), (65, ()))]
    ws = [some_windows(len(x)) for x in xs]
    prior = DC.make_prior('markov', rng, 2, 193)

    def call(trajs, windows, **kw):
        return bild_amd.exact_dwell_windows(trajs, model, prior, windows, **kw)
    batch = call(xs, ws)
    assert all(np.isfinite(r.log_evidence) and r.log_all.shape == (8,) and not np.any(np.isnan(r.log_all)) for r in batch)
    assert all(same(a, b) for a, b in zip(batch, call(xs, ws)))
    order = [2, 0, 3, 1]
    permuted = call([xs[i] for i in order], [ws[i] for i in order])
    assert all(same(permuted[j], batch[i]) for j, i in enumerate(order))
    shuffle = [5, 2, 7, 0, 3, 6, 1, 4]
    shuffled = call(xs, [[w[i] for i in shuffle] for w in ws])
    assert all(np.array_equal(s.log_all, r.log_all[shuffle]) and s.log_evidence == r.log_evidence for s, r in zip(shuffled, batch))
    assert all(same(call(x, w), r) for x, w, r in zip(xs, ws, batch))
    # one trajectory per chunk, and two: a trajectory's share of a chunk, S = 2 and 193 frames (csrc/gauss_dwellwin.cpp): the
    # forward and backward tables, and per window its kappa row, its 24-byte descriptor and its output
    slot = 2 * 194
    tables = slot * 40 + 2 * 8 + 8 + 193 + slot * 16
    own = max(sum(2 * (v - u - 1) * 8 + 24 + 8 for u, v, _ in w) for w in ws)
    for scratch in (1, 2 * (tables + own) + 8):
        assert all(same(a, b) for a, b in zip(batch, call(xs, ws, scratch_bytes=scratch)))


def test_trajectory_without_a_profile():
    rng = np.random.default_rng(3)
    model = C.random_model(rng, 2, 64)
    xs = [C.random_traj(rng, 50), C.random_traj(rng, 56)]
    no = DC.prior_of('impossible', rng, 2, 60, 50)
    windows = [(0, 1, 0), (0, 1, 1), (10, 40, 0), (10, 40, 1)]
    r = bild_amd.exact_dwell_windows(xs, model, no, [windows + [(0, 50, 0)], windows + [(0, 56, 0), (55, 56, 1)]])
    assert r[0].log_evidence == -np.inf and r[0].log_all.shape == (5,) and np.all(np.isnan(r[0].log_all))
    # 56 frames: the one segment in state 0 survives, and no frame is in state 1
    assert np.isfinite(r[1].log_evidence) and np.all(np.abs(r[1].log_all[[0, 2, 4]]) < TOL_LOG) and np.all(r[1].log_all[[1, 3, 5]] == -np.inf)


def test_trajectory_without_windows():
    rng = np.random.default_rng(8)
    model = C.random_model(rng, 2, 80)
    xs = [C.random_traj(rng, T) for T in (30, 70, 45)]
    prior = DC.make_prior('markov', rng, 2, 70)
    ref = bild_amd.exact_dwell(xs, model, prior, marginals=False)
    ws = [some_windows(30), [], some_windows(45)]
    r = bild_amd.exact_dwell_windows(xs, model, prior, ws)
    assert [len(a.log_all) for a in r] == [8, 0, 8] and r[1].windows.shape == (0, 2) and r[1].targets == ()
    assert all(a.log_evidence == b.log_evidence and a.n_nan_windows == b.n_nan_windows for a, b in zip(r, ref))
    assert all(same(a, bild_amd.exact_dwell_windows(x, model, prior, w)) for a, x, w in zip(r, xs, ws))
    none = bild_amd.exact_dwell_windows(xs, model, prior, [[], [], []], scratch_bytes=1)
    assert all(a.log_evidence == b.log_evidence and a.log_all.shape == (0,) for a, b in zip(none, ref))


def test_c_abi_refusals():
    rng = np.random.default_rng(51)
    model = C.random_model(rng, 2, 40)
    xs = [C.random_traj(rng, 30), C.random_traj(rng, 20)]
    ts = model.trajset(xs)
    p = DC.symmetric_chain(0.1, 30)
    good = (p.log_init, p.log_jump, p.log_dwell, p.log_surv)
    win = dict(traj=[0, 0, 1], u=[0, 5, 0], v=[30, 6, 20], target=[1, 2, 1])

    def call(*a, **k):
        w = {**win, **{key: k.pop(key) for key in list(k) if key in win}}
        return _lib.gauss_dwell_windows(model.handle(), ts, *a, w['traj'], w['u'], w['v'], w['target'], **k)
    res = call(*good)
    assert res['log_all'].shape == (3,) and np.all(res['log_all'] <= TOL_LOG) and np.all(np.isfinite(res['logev']))
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
    for target in (0, 3, 4, 5):                         # empty, every state, a state the model does not have
        with pytest.raises(_lib.BildAmdError, match='win_target') as e:
            call(*good, target=[1, target, 1])
        assert e.value.code == _lib.ERR_INVALID
    for u, v in (([0, 5, 0], [30, 5, 20]), ([0, 6, 0], [30, 5, 20]), ([0, -1, 0], [30, 6, 20]), ([0, 5, 0], [31, 6, 20]),
                 ([0, 5, 0], [30, 6, 21])):           # empty, reversed, before 0, behind T of its own trajectory
        with pytest.raises(_lib.BildAmdError, match='window') as e:
            call(*good, u=u, v=v)
        assert e.value.code == _lib.ERR_INVALID
    with pytest.raises(_lib.BildAmdError, match='must not decrease') as e:
        call(*good, traj=[0, 1, 0], v=[30, 6, 20])
    assert e.value.code == _lib.ERR_INVALID
    for traj in ([0, 0, 2], [-1, 0, 1]):
        with pytest.raises(_lib.BildAmdError, match='win_traj') as e:
            call(*good, traj=traj)
        assert e.value.code == _lib.ERR_INVALID

    arrs = [_lib.f64(a) for a in good]
    w = [np.array(win[k], dtype=np.uint32 if k == 'target' else np.int32) for k in ('traj', 'u', 'v', 'target')]

    def raw(n_win=3, T_max=30, flags=0, scratch=0, out=True, null=None):
        spec = _lib.DwellWindowsOut()
        ptrs = [None if i == null else a.ctypes.data for i, a in enumerate(w)]
        return _lib.lib().bild_gauss_dwell_windows(model.handle()._h, ts._h, 30, *[_lib.dptr(a) for a in arrs], T_max, scratch, n_win, *ptrs,
                                                   flags, ctypes.byref(spec) if out else None)
    assert raw() == _lib.OK         # (every output NULL: nothing is written)
    assert raw(n_win=0, null=0) == _lib.OK
    assert raw(flags=2) == _lib.ERR_INVALID and raw(scratch=-1) == _lib.ERR_INVALID
    assert raw(T_max=29) == _lib.ERR_INVALID and raw(out=False) == _lib.ERR_INVALID
    assert raw(n_win=-1) == _lib.ERR_INVALID and all(raw(null=i) == _lib.ERR_INVALID for i in range(4))
    five = C.random_model(rng, 5, 40)
    p5 = DC.make_prior('markov', rng, 5, 30)
    ts5 = five.trajset(xs[0])
    with pytest.raises(_lib.BildAmdError, match='at most 4') as e:
        _lib.gauss_dwell_windows(five.handle(), ts5, p5.log_init, p5.log_jump, p5.log_dwell, p5.log_surv, [0], [0], [5], [1])
    assert e.value.code == _lib.ERR_UNSUPPORTED
