"""
The exact posterior of the looped time under a dwell-time prior on the GPU (bild_amd.exact.exact_dwell_occupancy,
csrc/gauss_dwellocc.hip): against the NumPy oracle tests/dwell_occupancy_oracle.py around the 64-value
tiles of n, against `exact_dwell` and `exact_dwell_first_contact` on the device, the identities at T = 1000, the histogram of
`exact_dwell_draw` as an independent device route, the bit-identity properties and the refusals of the C call.
"""
import ctypes

import numpy as np
import pytest
from scipy.special import logsumexp

import bild_amd
import dwell_cases as DC
import dwell_event_cases as DEC
import dwell_occupancy_cases as DQC
import segment_cases as C
from bild_amd import _lib

pytestmark = pytest.mark.gpu

# The issue's bounds, the siblings' device bounds: a finite log within 1e-10, -inf exactly; 1e-9 at T = 1000.
# Worst seen on these cases: tests/README_dwell_occupancy.md.
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
    return logsumexp(r.log_occupancy, axis=1)


def sibling_deviations(x, model, prior, target, nan, r=None):
    """ section 28's identities between the call and its siblings on the device, as deviations of logs: (devs, r) """
    S, T = model.msd.shape[0], len(x)
    rest = tuple(s for s in range(S) if s not in target)
    r = bild_amd.exact_dwell_occupancy(x, model, prior, target, nan=nan) if r is None else r
    other = bild_amd.exact_dwell_occupancy(x, model, prior, rest, nan=nan)
    ref = bild_amd.exact_dwell(x, model, prior, nan=nan)
    post = ref.log_marginal_posterior
    assert r.log_evidence == other.log_evidence == ref.log_evidence and other.target == rest
    lp = log_pmf(r)
    devs = {'mean = sum of the marginals over G': abs(np.log(r.mean()) - logsumexp(post[list(target)])),
            'pmf[0] = never in G': log_deviation(lp[0], bild_amd.exact_dwell_first_contact(x, model, prior, target, nan=nan).log_never, 'pmf[0]'),
            'pmf[T] = never outside G': log_deviation(lp[T], bild_amd.exact_dwell_first_contact(x, model, prior, rest, nan=nan).log_never, 'pmf[T]'),
            'sum_n occupancy = last marginal': log_deviation(logsumexp(r.log_occupancy, axis=0), post[:, T - 1], 'columns'),
            'complement reversed': log_deviation(log_pmf(other)[::-1], lp, 'complement'),
            'sum pmf = 1': abs(logsumexp(lp))}
    return devs, r


@pytest.mark.parametrize('case', DQC.ORACLE_CASES, ids=DQC.case_id)
def test_against_oracle_and_siblings(case):
    S, T, missing, _, nan, targets, _ = case
    model, x, prior, W, F = DQC.oracle_case(*case[:4])
    answers = DQC.oracle_answer(case)
    ref = bild_amd.exact_dwell(x, model, prior, marginals=False, nan=nan)
    for target in targets:
        want = answers[target]
        r = bild_amd.exact_dwell_occupancy(x, model, prior, target, nan=nan)
        assert r.target == target and r.log_occupancy.shape == (T + 1, S)
        assert r.n_nan_windows == want['n_nan_windows'] == ref.n_nan_windows and (r.n_nan_windows > 0) == (missing == 'order0_gap')
        assert np.array_equal(r.log_evidence, ref.log_evidence, equal_nan=True)         # bit for bit `exact_dwell`'s
        if np.isnan(want['logev']):
            assert nan == 'propagate' and np.isnan(r.log_evidence) and np.all(np.isnan(r.log_occupancy))
            continue
        devs = {'logev': abs(r.log_evidence - want['logev']),
                'log_occupancy': log_deviation(r.log_occupancy, want['log_occupancy'], target)}
        sib, _ = sibling_deviations(x, model, prior, target, nan, r)
        pmf = r.pmf()
        print(f"{DQC.case_id(case)} {target}: oracle {DQC.ORACLE_SECONDS[case]:.2f} s, {int(np.sum(pmf > 1e-12))} bins above 1e-12, mean "
              f"{r.mean():.2f}, sd {np.sqrt(r.var()):.2f}, interval {r.interval()}; "
              + ', '.join(f"{k} {v:.1e}" for k, v in {**devs, **sib}.items()))
        for name, v in {**devs, **sib}.items():
            assert v < TOL_LOG, (case, target, name, v)


def hold_occupancy(r, want, ref, target, S, T, what):
    """ a `DwellOccupancy` against the oracle's answer and `exact_dwell`'s evidence: {name: deviation}, the bars asserted """
    assert r.target == target and r.log_occupancy.shape == (T + 1, S), what
    assert r.n_nan_windows == want['n_nan_windows'] == ref.n_nan_windows == 0, what
    assert np.isfinite(ref.log_evidence) and r.log_evidence == ref.log_evidence, what       # bit for bit `exact_dwell`'s
    devs = {'logev': abs(r.log_evidence - want['logev']), 'log_occupancy': log_deviation(r.log_occupancy, want['log_occupancy'], what),
            'sum pmf = 1': abs(logsumexp(log_pmf(r)))}
    for name, v in devs.items():
        assert v < TOL_LOG, (what, name, v)
    return devs


@pytest.mark.parametrize('item', DQC.WIDE_CASES, ids=DQC.wide_id)
def test_against_oracle_wide(item):
    """ four states, T > 256, non-geometric tables and the hard priors (tests/README_dwell_occupancy.md, "The wide cases") """
    case, target = item
    S, T = case[:2]
    model, x, prior, _, _ = DC.oracle_case(case)
    want = DQC.wide_answer(case, target)
    ref = bild_amd.exact_dwell(x, model, prior, marginals=False)
    r = bild_amd.exact_dwell_occupancy(x, model, prior, target)
    devs = hold_occupancy(r, want, ref, target, S, T, item)
    print(f"{DQC.wide_id(item)}: oracle {DQC.ORACLE_SECONDS[item]:.2f} s, {int(np.sum(r.pmf() > 1e-12))} bins above 1e-12, mean {r.mean():.2f}; "
          + ', '.join(f"{k} {v:.1e}" for k, v in devs.items()))
    assert DQC.ORACLE_SECONDS[item] < 20


def test_ragged_batch_against_oracle():
    """
    `dwell_cases.ragged_case` in one call: four states, non-geometric tables, T = 1 ... 257, so that five of the six have ld, slot
    and the stride of alpha that are not their own, and end before the chunk's last end frame.  Each trajectory of the batch is
    held to its own oracle answer, and the batch is the trajectories alone bit for bit, whole and with one trajectory a chunk.
    """
    model, prior, xs, _ = DC.ragged_case()
    refs = bild_amd.exact_dwell(xs, model, prior, marginals=False)
    worst, seconds = {}, 0.0
    for target in DEC.RAGGED_TARGETS:
        batch = bild_amd.exact_dwell_occupancy(xs, model, prior, target)
        assert len(batch) == len(xs)
        for j, (x, r, ref) in enumerate(zip(xs, batch, refs)):
            devs = hold_occupancy(r, DQC.ragged_answer(j, target), ref, target, 4, len(x), ('ragged', j, target))
            seconds = max(seconds, DQC.ORACLE_SECONDS['ragged', j, target])
            for name, v in devs.items():
                worst[name] = max(worst.get(name, 0.0), v)
            assert same(bild_amd.exact_dwell_occupancy(x, model, prior, target), r), (j, target)
        assert all(same(a, b) for a, b in zip(batch, bild_amd.exact_dwell_occupancy(xs, model, prior, target, scratch_bytes=1))), target
    print(f"ragged: slowest oracle answer {seconds:.2f} s; " + ', '.join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert seconds < 20


def test_identities_at_T1000():
    T = 1000
    rng = np.random.default_rng(31)
    model = C.random_model(rng, 2, T + 8, orders=np.ones((2, 3), dtype=int), d=3)
    x = C.random_traj(rng, T, (100, 500, 501), d=3)
    prior = bild_amd.DwellPrior.markov([[0.98, 0.02], [0.05, 0.95]], [0.6, 0.4], n=T)
    devs, r = sibling_deviations(x, model, prior, (1,), 'propagate')
    assert r.log_occupancy.shape == (T + 1, 2) and r.n_nan_windows == 0 and np.isfinite(r.log_evidence)
    assert not np.any(np.isnan(r.log_occupancy))
    print(f"mean {r.mean():.3f} frames, sd {np.sqrt(r.var()):.3f}, interval {r.interval()}, {int(np.sum(r.pmf() > 1e-12))} bins above 1e-12; "
          + ', '.join(f"{k}: {v:.1e}" for k, v in devs.items()))
    assert all(v < TOL_LOG_T1000 for v in devs.values()), devs


def test_against_the_histogram_of_the_draws():
    """ every bin within 5 sqrt(p (1 - p) / n) + 1 / n of the exact p: the binomial bound, nothing fitted """
    T, n = 130, 20000
    rng = np.random.default_rng(77)
    model = C.random_model(rng, 2, T + 8)
    x = C.random_traj(rng, T, (64,))
    prior = DC.make_prior('markov', rng, 2, T)
    draws = bild_amd.exact_dwell(x, model, prior).draw(n, seed=5)
    p = bild_amd.exact_dwell_occupancy(x, model, prior, 1).pmf()
    count = draws.occupancy(1)
    assert count.shape == (n,) and count.min() >= 0 and count.max() <= T
    hist = np.bincount(count, minlength=T + 1) / n
    slack = np.abs(hist - p) - (5 * np.sqrt(p * (1 - p) / n) + 1 / n)
    print(f"{len(p)} bins, {int(np.sum(p > 1e-12))} above 1e-12, largest |histogram - exact| {np.max(np.abs(hist - p)):.2e}, closest to its "
          f"bound by {-np.max(slack):.2e}")
    assert np.all(slack <= 0), (int(np.argmax(slack)), float(np.max(slack)))


FIELDS = ('log_evidence', 'n_nan_windows', 'log_occupancy')


def same(a, b):
    return all(np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True) for f in FIELDS)


def test_bit_identity():
    rng = np.random.default_rng(41)
    model = C.random_model(rng, 2, 200)
    xs = [C.random_traj(rng, T, missing) for T, missing in ((40, ()), (65, (9,)), (193, (63, 65)), (65, ()))]
    prior = DC.make_prior('markov', rng, 2, 193)

    def call(trajs, **kw):
        return bild_amd.exact_dwell_occupancy(trajs, model, prior, 1, **kw)
    batch = call(xs)
    assert all(np.isfinite(r.log_evidence) and r.log_occupancy.shape == (len(x) + 1, 2) for x, r in zip(xs, batch))
    assert all(same(a, b) for a, b in zip(batch, call(xs)))
    order = [2, 0, 3, 1]
    permuted = call([xs[i] for i in order])
    assert all(same(permuted[j], batch[i]) for j, i in enumerate(order))
    assert all(same(call(x), r) for x, r in zip(xs, batch))
    # one trajectory per chunk, and two: a trajectory's share of a chunk, S = 2 and 193 frames (csrc/gauss_dwellocc.cpp)
    slot = 2 * 194
    forward = slot * 40 + 2 * 8 + 8 + 193
    per_traj = forward + (2 * 193 * 194 + slot) * 8
    for scratch in (1, 2 * per_traj + 8):
        assert all(same(a, b) for a, b in zip(batch, call(xs, scratch_bytes=scratch)))


def test_trajectory_without_a_profile():
    rng = np.random.default_rng(3)
    model = C.random_model(rng, 2, 64)
    xs = [C.random_traj(rng, 50), C.random_traj(rng, 56)]
    no = DC.prior_of('impossible', rng, 2, 60, 50)
    r = bild_amd.exact_dwell_occupancy(xs, model, no, 1)
    assert r[0].log_evidence == -np.inf and r[0].log_occupancy.shape == (51, 2) and np.all(np.isnan(r[0].log_occupancy))
    # 56 frames: the one segment in state 0 survives, and no frame is in state 1
    assert r[1].log_occupancy.shape == (57, 2)
    assert abs(r[1].log_occupancy[0, 0]) < TOL_LOG and np.all(r[1].log_occupancy.ravel()[1:] == -np.inf)
    other = bild_amd.exact_dwell_occupancy(xs, model, no, 0)
    assert np.all(np.isnan(other[0].log_occupancy))
    assert abs(other[1].log_occupancy[56, 0]) < TOL_LOG and np.all(other[1].log_occupancy.ravel()[:-2] == -np.inf)
    assert other[1].log_occupancy[56, 1] == -np.inf


def test_c_abi_refusals():
    rng = np.random.default_rng(51)
    model = C.random_model(rng, 2, 40)
    x = C.random_traj(rng, 30)
    ts = model.trajset(x)
    p = DC.symmetric_chain(0.1, 30)
    good = (p.log_init, p.log_jump, p.log_dwell, p.log_surv)

    def call(*a, **k):
        return _lib.gauss_dwell_occupancy(model.handle(), ts, *a, k.pop('target', 2), **k)
    res = call(*good)
    assert res['log_occ'].shape == (1, 31, 2) and abs(np.exp(res['log_occ']).sum() - 1) < TOL_LOG
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
        with pytest.raises(_lib.BildAmdError, match='target') as e:
            call(*good, target=target)
        assert e.value.code == _lib.ERR_INVALID

    arrs = [_lib.f64(a) for a in good]

    def raw(target=1, T_max=30, flags=0, scratch=0, out=True):
        spec = _lib.DwellOccupancyOut()
        return _lib.lib().bild_gauss_dwell_occupancy(model.handle()._h, ts._h, 30, *[_lib.dptr(a) for a in arrs], T_max, target, flags,
                                                     scratch, ctypes.byref(spec) if out else None)
    assert raw() == _lib.OK         # (every output NULL: nothing is written)
    assert raw(flags=2) == _lib.ERR_INVALID and raw(scratch=-1) == _lib.ERR_INVALID
    assert raw(T_max=29) == _lib.ERR_INVALID and raw(out=False) == _lib.ERR_INVALID
    assert raw(target=0) == _lib.ERR_INVALID and raw(target=3) == _lib.ERR_INVALID and raw(target=4) == _lib.ERR_INVALID
    five = C.random_model(rng, 5, 40)
    p5 = DC.make_prior('markov', rng, 5, 30)
    ts5 = five.trajset(x)
    with pytest.raises(_lib.BildAmdError, match='at most 4') as e:
        _lib.gauss_dwell_occupancy(five.handle(), ts5, p5.log_init, p5.log_jump, p5.log_dwell, p5.log_surv, 1)
    assert e.value.code == _lib.ERR_UNSUPPORTED
