"""
The exact online filter under a dwell-time prior on the GPU (bild_amd.exact.exact_dwell_filter, csrc/gauss_dwellfilt.hip,
DESIGN.md section 25): against the NumPy oracle tests/dwell_filter_oracle.py at the tile seams, at one to four states and under
the hard priors (`dwell_filter_cases.GPU_CASES`), against the parent's own device code (`exact_dwell` on every truncation x[:b]
in one call), the end of the trajectory against `exact_dwell`, S = 1 against the per-frame terms of `kalman`, a ragged batch,
bit-identity, T = 1000 and the refusals of the C call.  Bars as in tests/test_gpu_dwell.py: prefix evidences, log_filtered and
finite log_run entries 1e-10, log_predictive 2e-10 (a difference of two such values), run_mean 1e-9 relative; NaN and -inf
patterns identical, n_nan_windows exact.  `-s` prints the worst deviation of each; what the MI355X gave:
tests/README_dwell_filter.md.
"""
import ctypes

import numpy as np
import pytest
from scipy.special import logsumexp

import bild_amd
import dwell_cases as DC
import dwell_filter_cases as FC
import segment_cases as C
from bild_amd import _lib

pytestmark = pytest.mark.gpu

BARS = {'prefix_log_evidence': 1e-10, 'log_filtered': 1e-10, 'log_run_length': 1e-10, 'log_predictive': 2e-10}


def same_pattern(got, ref):
    """ NaN, +inf and -inf at the same places """
    return (np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(got == -np.inf, ref == -np.inf)
            and np.array_equal(got == np.inf, ref == np.inf))


def check_against_oracle(r, want, label=''):
    T = len(r.traj)
    assert np.array_equal(r.n_nan_windows, want['n_nan_windows']) and r.n_nan_windows.dtype == np.int64
    with np.errstate(invalid='ignore'):
        predictive = np.diff(want['prefix_logev'], prepend=0.0)
    for name, got, ref in (('prefix_log_evidence', r.prefix_log_evidence, want['prefix_logev']),
                           ('log_predictive', r.log_predictive, predictive), ('log_filtered', r.log_filtered, want['log_filtered']),
                           ('log_run_length', r.log_run_length, want['log_run'])):
        assert got.shape == ref.shape and same_pattern(got, ref), (label, name)
        fin = np.isfinite(ref)
        worst = np.max(np.abs(got[fin] - ref[fin]), initial=0.0)
        print(label, name, worst)
        assert worst < BARS[name], (label, name, worst)
    got, ref = r.run_length_mean, want['run_mean']
    assert got.shape == ref.shape == (T,) and same_pattern(got, ref)
    fin = np.isfinite(ref)
    print(label, 'run_length_mean', np.max(np.abs(got[fin] - ref[fin]) / ref[fin], initial=0.0))
    assert np.all(np.abs(got[fin] - ref[fin]) <= 1e-9 * ref[fin]), (label, got, ref)
    if np.isfinite(want['logev']):
        assert abs(r.log_evidence - want['logev']) < 1e-10
    else:
        assert np.array_equal(r.log_evidence, want['logev'], equal_nan=True)


@pytest.mark.parametrize('S,T,missing,kind', FC.GPU_CASES)
def test_against_oracle(S, T, missing, kind):
    case = (S, T, missing, kind)
    model, x, prior, W, F = DC.oracle_case(case)
    want = FC.oracle_answer(case)
    print(f"oracle {FC.ORACLE_SECONDS[case]:.1f} s")
    r = bild_amd.exact_dwell_filter(x, model, prior, run_max=FC.run_max_of(T))
    check_against_oracle(r, want, str(case))
    if kind == 'impossible':
        assert r.log_evidence == -np.inf == r.prefix_log_evidence[-1] and np.all(np.isnan(r.log_filtered[:, -1]))
        assert np.isnan(r.run_length_mean[-1]) and np.all(np.isnan(r.log_run_length[:, -1]))
    if kind == 'flip':
        assert np.max(np.abs(r.run_length_mean - 1)) < 1e-9 and np.all(r.log_run_length[:, 1:, 1:] == -np.inf)


def truncations_against_exact_dwell(model, x, prior, nan):
    """ frame t of the filter against `exact_dwell` of x[:t + 1]: every truncation in ONE call of the parent's device code """
    T = len(x)
    r = bild_amd.exact_dwell_filter(x, model, prior, nan=nan)
    cut = bild_amd.exact_dwell([x[:b] for b in range(1, T + 1)], model, prior, nan=nan)
    assert np.array_equal(r.n_nan_windows, [c.n_nan_windows for c in cut])
    for name, got, ref in (('logev', r.prefix_log_evidence, np.array([c.log_evidence for c in cut])),
                           ('last marginal', r.log_filtered, np.stack([c.log_marginal_posterior[:, -1] for c in cut], axis=1))):
        assert same_pattern(got, ref), name
        fin = np.isfinite(ref)
        print(nan, name, np.max(np.abs(got[fin] - ref[fin]), initial=0.0))
        assert np.max(np.abs(got[fin] - ref[fin]), initial=0.0) < 1e-10
    return r, cut


@pytest.mark.parametrize('S,T,missing,kind', FC.TRUNCATION_CASES)
def test_against_exact_dwell_of_every_truncation(S, T, missing, kind):
    model, x, prior, _, _ = DC.oracle_case((S, T, missing, kind))
    r, _ = truncations_against_exact_dwell(model, x, prior, 'propagate')
    assert np.all(r.n_nan_windows == 0) and np.all(np.isfinite(r.prefix_log_evidence))


@pytest.mark.parametrize('nan', ['propagate', 'omit'])
def test_order0_gap_against_exact_dwell_of_every_truncation(nan):
    model, x, prior, _, _ = FC.gap_case()
    r, cut = truncations_against_exact_dwell(model, x, prior, nan)
    check_against_oracle(bild_amd.exact_dwell_filter(x, model, prior, run_max=70, nan=nan), FC.gap_answer(nan), f'gap {nan}')
    bad = np.array([c.n_nan_windows > 0 for c in cut])
    assert bad.any() and not bad.all()
    if nan == 'propagate':      # NaN exactly at the frames whose truncation is NaN
        assert np.array_equal(np.isnan(r.prefix_log_evidence), bad) and np.array_equal(np.isnan(r.run_length_mean), bad)
        assert np.array_equal(np.isnan(r.log_filtered), np.broadcast_to(bad, (2, 70))) and np.isnan(r.log_evidence)
    else:
        assert np.all(np.isfinite(r.prefix_log_evidence)) and np.isfinite(r.log_evidence)


def test_end_of_the_trajectory():
    for case in ((3, 65, (7,), 'minlength'), (2, 130, (), 'bounded'), (4, 257, (100,), 'nongeometric')):
        model, x, prior, _, _ = DC.oracle_case(case)
        r, full = bild_amd.exact_dwell_filter(x, model, prior), bild_amd.exact_dwell(x, model, prior)
        assert r.log_evidence == full.log_evidence and r.log_run_length is None
        assert r.n_nan_windows[-1] == full.n_nan_windows
        print(case, abs(r.prefix_log_evidence[-1] - full.log_evidence), np.max(np.abs(r.log_filtered[:, -1] - full.log_marginal_posterior[:, -1])))
        assert abs(r.prefix_log_evidence[-1] - full.log_evidence) < 1e-10
        assert np.max(np.abs(r.log_filtered[:, -1] - full.log_marginal_posterior[:, -1])) < 1e-10


def test_one_state_predictive_is_the_flat_profile_per_frame():
    """ S = 1: the one profile is flat, and log p(x_t | x_0 .. x_{t-1}) is the frame's log-likelihood term """
    T = 65
    rng = np.random.default_rng(71)
    model = C.random_model(rng, 1, T + 8)
    x = C.random_traj(rng, T)
    r = bild_amd.exact_dwell_filter(x, model, bild_amd.DwellPrior.markov([[1.0]], n=T), run_max=T)
    terms = model.kalman([np.zeros(T, dtype=int)], x, outputs=('terms',)).terms[0].sum(axis=1)
    print(np.max(np.abs(r.log_predictive - terms)))
    assert terms.shape == (T,) and np.max(np.abs(r.log_predictive - terms)) < 1e-10
    assert np.all(r.log_filtered == 0) and np.array_equal(r.run_length_mean, np.arange(1.0, T + 1))
    assert abs(r.log_predictive.sum() - r.log_evidence) < 1e-10


def test_ragged_batch_against_oracle():
    model, prior, xs, _ = DC.ragged_case()
    batch = bild_amd.exact_dwell_filter(xs, model, prior, run_max=FC.RAGGED_RUN_MAX)
    for j, (r, want) in enumerate(zip(batch, FC.ragged_answers())):
        assert len(r.traj) == len(xs[j]) and r.log_run_length.shape == (4, len(xs[j]), FC.RAGGED_RUN_MAX)
        check_against_oracle(r, want, f'ragged {j}')


FIELDS = ('log_evidence', 'prefix_log_evidence', 'log_predictive', 'log_filtered', 'run_length_mean', 'n_nan_windows')


def same(a, b, fields=FIELDS + ('log_run_length',)):
    return all(np.array_equal(getattr(a, name), getattr(b, name), equal_nan=True) for name in fields)


def test_bit_identity():
    rng = np.random.default_rng(41)
    model = C.random_model(rng, 2, 200)
    xs = [C.random_traj(rng, T, missing) for T, missing in ((40, ()), (65, (9,)), (193, (63, 65)), (65, ()))]
    prior = DC.make_prior('markov', rng, 2, 193)
    filt = bild_amd.exact_dwell_filter
    batch = filt(xs, model, prior, run_max=70)
    assert all(np.all(np.isfinite(r.prefix_log_evidence)) for r in batch)
    assert all(same(a, b) for a, b in zip(batch, filt(xs, model, prior, run_max=70)))
    order = [2, 0, 3, 1]
    permuted = filt([xs[i] for i in order], model, prior, run_max=70)
    assert all(same(permuted[j], batch[i]) for j, i in enumerate(order))
    for x, r in zip(xs, batch):
        assert same(filt(x, model, prior, run_max=70), r)
    # one trajectory per chunk, and two: the forward tables (S = 2, 194 entries a row), the filter's outputs and log_run
    per_traj = 2 * 194 * 40 + 4096 + 193 * (4 * 8 + 8) + 2 * 193 * 70 * 8
    for scratch in (1, 2 * per_traj):
        assert all(same(a, b) for a, b in zip(batch, filt(xs, model, prior, run_max=70, scratch_bytes=scratch)))
    # without log_run the other outputs are the same bits
    plain = filt(xs, model, prior)
    assert all(p.log_run_length is None and same(p, b, FIELDS) for p, b in zip(plain, batch))


def test_T1000():
    T = 1000
    rng = np.random.default_rng(31)
    model = C.random_model(rng, 2, T + 8, orders=np.ones((2, 3), dtype=int), d=3)
    x = C.random_traj(rng, T, (100, 500, 501), d=3)
    prior = bild_amd.DwellPrior.markov([[0.98, 0.02], [0.05, 0.95]], [0.6, 0.4], n=T)
    r = bild_amd.exact_dwell_filter(x, model, prior, run_max=T)
    assert np.all(r.n_nan_windows == 0) and np.all(np.isfinite(r.prefix_log_evidence))
    assert r.log_evidence == bild_amd.exact_dwell(x, model, prior, marginals=False).log_evidence
    assert abs(r.prefix_log_evidence[-1] - r.log_evidence) < 1e-9 and abs(r.log_predictive.sum() - r.log_evidence) < 1e-9
    run = np.exp(r.log_run_length)
    worst = (np.max(np.abs(logsumexp(r.log_filtered, axis=0))), np.max(np.abs(run.sum(axis=(0, 2)) - 1)),
             np.max(np.abs(np.tensordot(run.sum(axis=0), np.arange(1.0, T + 1), axes=1) / r.run_length_mean - 1)),
             np.max(np.abs(run.sum(axis=2) - np.exp(r.log_filtered))))
    print(worst)
    assert max(worst) < 1e-9
    assert all(np.all(r.log_run_length[:, t, t + 1:] == -np.inf) for t in range(0, T, 37))


def test_c_abi_refusals():
    rng = np.random.default_rng(51)
    model = C.random_model(rng, 2, 40)
    x = C.random_traj(rng, 30)
    ts = model.trajset(x)
    p = DC.symmetric_chain(0.1, 30)
    good = (p.log_init, p.log_jump, p.log_dwell, p.log_surv)
    _lib.gauss_dwell_filter(model.handle(), ts, *good, run_max=5)

    def bad(i, fn):
        args = [a.copy() for a in good]
        args[i] = fn(args[i])
        with pytest.raises(_lib.BildAmdError) as e:
            _lib.gauss_dwell_filter(model.handle(), ts, *args)
        assert e.value.code == _lib.ERR_INVALID

    def put(index, value):
        def fn(a):
            a[index] = value
            return a
        return fn

    with pytest.raises(_lib.BildAmdError) as e:        # L shorter than the trajectory
        _lib.gauss_dwell_filter(model.handle(), ts, good[0], good[1], good[2][:, :29], good[3][:, :29])
    assert e.value.code == _lib.ERR_INVALID
    for i in (0, 1, 2, 3):                          # a NaN or +inf entry anywhere
        bad(i, put((0,) * good[i].ndim, np.nan))
        bad(i, put((-1,) * good[i].ndim, np.inf))
    bad(1, put((1, 1), 0.0))                        # a self-jump
    bad(0, lambda a: np.full(2, -np.inf))

    runs = np.empty((2, 30, 4))

    def raw(T_max=30, run_max=0, flags=0, scratch=0, log_run=None, out=True):
        arrs = [_lib.f64(a) for a in good]
        spec = _lib.DwellFilterOut(log_run=log_run)
        return _lib.lib().bild_gauss_dwell_filter(model.handle()._h, ts._h, 30, *[_lib.dptr(a) for a in arrs], T_max, run_max, flags,
                                                 scratch, ctypes.byref(spec) if out else None)
    assert raw() == _lib.OK and raw(run_max=4) == _lib.OK       # (every output NULL: nothing is written)
    assert raw(run_max=4, log_run=_lib.aptr(runs)) == _lib.OK and np.all(runs[:, 0, 1:] == -np.inf)
    assert raw(flags=2) == _lib.ERR_INVALID and raw(scratch=-1) == _lib.ERR_INVALID and raw(T_max=29) == _lib.ERR_INVALID
    assert raw(run_max=-1) == _lib.ERR_INVALID and raw(run_max=0, log_run=_lib.aptr(runs)) == _lib.ERR_INVALID
    assert raw(out=False) == _lib.ERR_INVALID
    five = C.random_model(rng, 5, 40)
    p5 = DC.make_prior('markov', rng, 5, 30)
    with pytest.raises(_lib.BildAmdError) as e:
        _lib.gauss_dwell_filter(five.handle(), five.trajset(x), p5.log_init, p5.log_jump, p5.log_dwell, p5.log_surv)
    assert e.value.code == _lib.ERR_UNSUPPORTED
