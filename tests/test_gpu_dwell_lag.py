"""
Exact fixed-lag smoothing under a dwell-time prior on the GPU (bild_amd.exact.exact_dwell_lag, csrc/gauss_dwelllag.hip, DESIGN.md
section 26): against the NumPy oracle tests/dwell_lag_oracle.py at the smallest shapes where the kernels can go wrong
(`dwell_lag_cases.GPU_CASES`), against the parent's own device code (`exact_dwell` on every truncation x[:u] in one call,
`exact_dwell_filter` for column 0, `exact_dwell` for the columns of the whole trajectory), a ragged batch, bit-identity, T = 1000
and the refusals of the C call.  Bars as in tests/test_gpu_dwell_filter.py: finite log entries 1e-10, NaN and -inf patterns
identical, n_nan_windows exact.  `-s` prints the worst deviation of each; what the MI355X gave: tests/README_dwell_lag.md.
"""
import ctypes

import numpy as np
import pytest
from scipy.special import logsumexp

import bild_amd
import dwell_cases as DC
import dwell_filter_cases as FC
import dwell_lag_cases as LC
import segment_cases as C
from bild_amd import _lib

pytestmark = pytest.mark.gpu

BAR = 1e-10


def same_pattern(got, ref):
    """ NaN, +inf and -inf at the same places """
    return (np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(got == -np.inf, ref == -np.inf)
            and np.array_equal(got == np.inf, ref == np.inf))


def worst_of(got, ref, label):
    assert got.shape == ref.shape and same_pattern(got, ref), label
    fin = np.isfinite(ref)
    worst = np.max(np.abs(got[fin] - ref[fin]), initial=0.0)
    print(label, worst)
    return worst


def check_against_oracle(r, want, label=''):
    assert np.array_equal(r.n_nan_windows, want['n_nan_windows']) and r.n_nan_windows.dtype == np.int64
    assert worst_of(r.log_lagged, want['log_lagged'], label) < BAR, label


@pytest.mark.parametrize('case,lag', LC.GPU_CASES)
def test_against_oracle(case, lag):
    S, T, missing, kind = case
    model, x, prior, W, F = DC.oracle_case(case)
    want = LC.oracle_answer(case, lag)
    print(f"oracle {LC.ORACLE_SECONDS[case, lag]:.1f} s")
    r = bild_amd.exact_dwell_lag(x, model, prior, lag)
    assert r.lag == lag and r.log_lagged.shape == (S, T, lag + 1)
    check_against_oracle(r, want, f'{case} lag {lag}')
    full = DC.oracle_answer(case)
    if kind == 'impossible':
        assert r.log_evidence == -np.inf and np.all(np.isnan(r.log_lagged[:, -1])) and np.all(r.settling_lag()[-lag - 1:] == -1)
    else:
        assert abs(r.log_evidence - full['logev']) < BAR
        assert np.array_equal(r.fixed_lag(lag), r.log_lagged[:, :, lag]) and np.all(r.settling_lag() >= 0)


def truncations_against_exact_dwell(model, x, prior, lag, nan):
    """ entry (t, l) against frame t of `exact_dwell` of x[:min(t + l + 1, T)]: every truncation in ONE call of the parent's device code """
    T = len(x)
    r = bild_amd.exact_dwell_lag(x, model, prior, lag, nan=nan)
    cut = bild_amd.exact_dwell([x[:u] for u in range(1, T + 1)], model, prior, nan=nan)
    assert np.array_equal(r.n_nan_windows, [c.n_nan_windows for c in cut])
    ref = np.stack([np.stack([cut[LC.cut_of(T, t, l) - 1].log_marginal_posterior[:, t] for l in range(lag + 1)], axis=1)
                    for t in range(T)], axis=1)
    assert worst_of(r.log_lagged, ref, f'truncations {nan}') < BAR
    # column 0 is the filter; the evidence is exact_dwell's, bit for bit
    filt = bild_amd.exact_dwell_filter(x, model, prior, nan=nan)
    assert worst_of(r.log_lagged[:, :, 0], filt.log_filtered, 'column 0 against the filter') < BAR
    assert np.array_equal(r.n_nan_windows, filt.n_nan_windows)
    assert np.array_equal(r.log_evidence, cut[-1].log_evidence, equal_nan=True)
    return r, cut


@pytest.mark.parametrize('case,lag', LC.TRUNCATION_CASES)
def test_against_exact_dwell_of_every_truncation(case, lag):
    model, x, prior, _, _ = DC.oracle_case(case)
    r, cut = truncations_against_exact_dwell(model, x, prior, lag, 'propagate')
    assert np.all(r.n_nan_windows == 0) and not np.isnan(r.log_lagged).any()
    assert r.log_evidence == cut[-1].log_evidence


@pytest.mark.parametrize('nan', ['propagate', 'omit'])
def test_order0_gap_against_exact_dwell_of_every_truncation(nan):
    model, x, prior, _, _ = FC.gap_case()
    T, lag = len(x), LC.GAP_LAG
    r, cut = truncations_against_exact_dwell(model, x, prior, lag, nan)
    check_against_oracle(r, LC.gap_answer(nan), f'gap {nan}')
    bad = np.array([c.n_nan_windows > 0 for c in cut])
    assert bad.any() and not bad.all()
    if nan == 'propagate':      # NaN exactly where the entry's truncation is NaN
        cut_bad = np.array([[bad[LC.cut_of(T, t, l) - 1] for l in range(lag + 1)] for t in range(T)])
        assert np.array_equal(np.isnan(r.log_lagged), np.broadcast_to(cut_bad, (2, T, lag + 1))) and np.isnan(r.log_evidence)
        assert np.array_equal(r.settling_lag() == -1, cut_bad.any(axis=1))
    else:
        assert not np.isnan(r.log_lagged).any() and np.isfinite(r.log_evidence)


def test_whole_lag_is_the_smoother():
    """ with lag >= T - 1 column `lag` is `exact_dwell`'s marginal at every frame """
    for case, lag in (((2, 63, (5,), 'markov'), 63), ((2, 64, (), 'minlength'), 63), ((4, 64, (), 'minlength'), 63), ((2, 3, (), 'markov'), 5)):
        model, x, prior, _, _ = DC.oracle_case(case)
        r, full = bild_amd.exact_dwell_lag(x, model, prior, lag), bild_amd.exact_dwell(x, model, prior)
        assert r.log_evidence == full.log_evidence and r.n_nan_windows[-1] == full.n_nan_windows
        assert worst_of(r.fixed_lag(lag), full.log_marginal_posterior, f'{case} column {lag} against exact_dwell') < BAR


def test_ragged_batch_against_oracle():
    model, prior, xs, _ = DC.ragged_case()
    batch = bild_amd.exact_dwell_lag(xs, model, prior, LC.RAGGED_LAG)
    for j, (r, want) in enumerate(zip(batch, LC.ragged_answers())):
        assert len(r.traj) == len(xs[j]) and r.log_lagged.shape == (4, len(xs[j]), LC.RAGGED_LAG + 1)
        check_against_oracle(r, want, f'ragged {j}')
    # behind a trajectory's T the C call writes NaN and a count of 0
    ts = model.trajset(xs)
    res = _lib.gauss_dwell_lag(model.handle(), ts, prior.log_init, prior.log_jump, prior.log_dwell, prior.log_surv, LC.RAGGED_LAG)
    for j, x in enumerate(xs):
        assert np.all(np.isnan(res['log_lagged'][j, :, len(x):])) and np.all(res['n_nan_windows'][j, len(x):] == 0)
        assert not np.isnan(res['log_lagged'][j, :, :len(x)]).any()


FIELDS = ('log_evidence', 'log_lagged', 'n_nan_windows')


def same(a, b):
    return all(np.array_equal(getattr(a, name), getattr(b, name), equal_nan=True) for name in FIELDS)


def test_bit_identity():
    rng = np.random.default_rng(41)
    model = C.random_model(rng, 2, 200)
    xs = [C.random_traj(rng, T, missing) for T, missing in ((40, ()), (65, (9,)), (193, (63, 65)), (65, ()))]
    prior = DC.make_prior('markov', rng, 2, 193)
    smooth = bild_amd.exact_dwell_lag
    lag = 30
    batch = smooth(xs, model, prior, lag)
    assert all(not np.isnan(r.log_lagged).any() for r in batch)
    assert all(same(a, b) for a, b in zip(batch, smooth(xs, model, prior, lag)))
    order = [2, 0, 3, 1]
    permuted = smooth([xs[i] for i in order], model, prior, lag)
    assert all(same(permuted[j], batch[i]) for j, i in enumerate(order))
    for x, r in zip(xs, batch):
        assert same(smooth(x, model, prior, lag), r)
    # one trajectory per chunk, and two: the forward tables (S = 2, 194 entries a row), the filter's outputs, the bases and the answer
    per_traj = 2 * 194 * 40 + 4096 + 193 * (4 * 8 + 8) + 2 * (2 * 194 + 193 * (lag + 1)) * 8
    for scratch in (1, 2 * per_traj):
        assert all(same(a, b) for a, b in zip(batch, smooth(xs, model, prior, lag, scratch_bytes=scratch)))
    # another lag moves the split between the bases and the windows: the columns agree to rounding, the rest bit for bit
    for other in (5, 63):
        n = min(lag, other) + 1
        for a, b in zip(batch, smooth(xs, model, prior, other)):
            assert a.log_evidence == b.log_evidence and np.array_equal(a.n_nan_windows, b.n_nan_windows)
            assert worst_of(b.log_lagged[:, :, :n], a.log_lagged[:, :, :n], f'lag {other} against lag {lag}') < BAR


def test_T1000():
    T, lag = 1000, 63
    rng = np.random.default_rng(31)
    model = C.random_model(rng, 2, T + 8, orders=np.ones((2, 3), dtype=int), d=3)
    x = C.random_traj(rng, T, (100, 500, 501), d=3)
    prior = bild_amd.DwellPrior.markov([[0.98, 0.02], [0.05, 0.95]], [0.6, 0.4], n=T)
    r = bild_amd.exact_dwell_lag(x, model, prior, lag)
    full = bild_amd.exact_dwell(x, model, prior)
    filt = bild_amd.exact_dwell_filter(x, model, prior)
    assert np.all(r.n_nan_windows == 0) and not np.isnan(r.log_lagged).any() and r.log_evidence == full.log_evidence
    sums = np.max(np.abs(logsumexp(r.log_lagged, axis=0)))
    first = worst_of(r.fixed_lag(0), filt.log_filtered, 'column 0 against the filter')
    tail = 0.0
    for t in range(T - 1 - lag, T):     # the columns of the whole trajectory
        got = r.log_lagged[:, t, T - 1 - t:]
        tail = max(tail, worst_of(got, np.repeat(full.log_marginal_posterior[:, t, None], got.shape[1], axis=1), f'frame {t}'))
    print(sums, first, tail)
    assert max(sums, first, tail) < 1e-9
    settle = r.settling_lag()
    print('settling lag: median', np.median(settle), 'frames at the limit', int(np.sum(settle == lag)))
    assert np.all((settle >= 0) & (settle <= lag))


def test_c_abi_refusals():
    rng = np.random.default_rng(51)
    model = C.random_model(rng, 2, 40)
    x = C.random_traj(rng, 30)
    ts = model.trajset(x)
    p = DC.symmetric_chain(0.1, 30)
    good = (p.log_init, p.log_jump, p.log_dwell, p.log_surv)
    _lib.gauss_dwell_lag(model.handle(), ts, *good, 5)

    def bad(i, fn):
        args = [a.copy() for a in good]
        args[i] = fn(args[i])
        with pytest.raises(_lib.BildAmdError) as e:
            _lib.gauss_dwell_lag(model.handle(), ts, *args, 5)
        assert e.value.code == _lib.ERR_INVALID

    def put(index, value):
        def fn(a):
            a[index] = value
            return a
        return fn

    with pytest.raises(_lib.BildAmdError) as e:        # L shorter than the trajectory
        _lib.gauss_dwell_lag(model.handle(), ts, good[0], good[1], good[2][:, :29], good[3][:, :29], 5)
    assert e.value.code == _lib.ERR_INVALID
    for i in (0, 1, 2, 3):                          # a NaN or +inf entry anywhere
        bad(i, put((0,) * good[i].ndim, np.nan))
        bad(i, put((-1,) * good[i].ndim, np.inf))
    bad(1, put((1, 1), 0.0))                        # a self-jump
    bad(0, lambda a: np.full(2, -np.inf))

    out = np.empty((2, 30, 4))

    def raw(T_max=30, lag=3, flags=0, scratch=0, log_lagged=None, spec=True):
        arrs = [_lib.f64(a) for a in good]
        o = _lib.DwellLagOut(log_lagged=log_lagged)
        return _lib.lib().bild_gauss_dwell_lag(model.handle()._h, ts._h, 30, *[_lib.dptr(a) for a in arrs], T_max, lag, flags, scratch,
                                              ctypes.byref(o) if spec else None)
    assert raw() == _lib.OK and raw(lag=0) == _lib.OK and raw(lag=63) == _lib.OK    # (every output NULL: nothing is written)
    assert raw(log_lagged=_lib.aptr(out)) == _lib.OK and np.max(np.abs(logsumexp(out, axis=0))) < 1e-9
    assert raw(flags=2) == _lib.ERR_INVALID and raw(scratch=-1) == _lib.ERR_INVALID and raw(T_max=29) == _lib.ERR_INVALID
    assert raw(lag=-1) == _lib.ERR_INVALID and raw(lag=64) == _lib.ERR_UNSUPPORTED and raw(lag=1000) == _lib.ERR_UNSUPPORTED
    assert raw(spec=False) == _lib.ERR_INVALID
    five = C.random_model(rng, 5, 40)
    p5 = DC.make_prior('markov', rng, 5, 30)
    with pytest.raises(_lib.BildAmdError) as e:
        _lib.gauss_dwell_lag(five.handle(), five.trajset(x), p5.log_init, p5.log_jump, p5.log_dwell, p5.log_surv, 5)
    assert e.value.code == _lib.ERR_UNSUPPORTED
