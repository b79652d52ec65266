"""
The expected segment-length counts and the fit of the dwell-time prior on the GPU (bild_amd.exact.exact_dwell_lengths,
fit_dwell_prior, csrc/gauss_dwelllen.hip): against the NumPy oracle tests/dwell_length_oracle.py around
the 64-length tiles and the 64-frame blocks of the length kernel, bit for bit against `exact_dwell`, the identities at
T = 1000, Fisher's identity by central differences of `exact_dwell`'s own evidence, the bit-identity properties, the refusals
of the C call, and the two fits.
"""
import ctypes
import time

import numpy as np
import pytest

import bild_amd
import dwell_cases as DC
import dwell_length_cases as DLC
import segment_cases as C
from bild_amd import _lib

pytestmark = pytest.mark.gpu

# The issue's bar for a count: 1e-9 relative with an absolute floor of 1e-12.  Worst seen on these cases: DESIGN.md section 24.
REL, FLOOR = 1e-9, 1e-12

FIELDS = ('log_evidence', 'n_nan_windows', 'expected_jumps', 'expected_init', 'expected_dwell', 'expected_censored')


def deviation(got, want):
    """ the largest |got - want| in units of its bound max(REL |want|, FLOOR), and the largest relative error above the floor """
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    assert got.shape == want.shape and np.all(np.isfinite(got))
    err = np.abs(got - want)
    big = np.abs(want) > FLOOR / REL
    return float(np.max(err / np.maximum(REL * np.abs(want), FLOOR), initial=0.0)), float(np.max(err[big] / np.abs(want[big]), initial=0.0))


def same(a, b):
    return all(np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True) for f in FIELDS)


@pytest.mark.parametrize('case', DLC.ORACLE_CASES, ids=lambda c: f"S{c[0]}_T{c[1]}_{c[3]}_{c[4]}" + ('_order0_gap' if c[2] == 'order0_gap' else ''))
def test_against_oracle(case):
    S, T, nan = case[0], case[1], case[4]
    model, x, prior, W, F = DLC.oracle_case(*case[:4])
    want = DLC.oracle_answer(case)
    r = bild_amd.exact_dwell_lengths(x, model, prior, nan=nan)
    assert r.expected_dwell.shape == (S, T) and r.expected_censored.shape == (S, T) and r.expected_init.shape == (S,)
    assert r.n_nan_windows == want['n_nan_windows'] and (r.n_nan_windows > 0) == (case[2] == 'order0_gap')
    if np.isnan(want['logev']):
        assert nan == 'propagate' and np.isnan(r.log_evidence)
        for f in FIELDS[2:]:
            assert np.all(np.isnan(getattr(r, f))), f
        assert np.all(np.isnan(r.lifetime_pmf(0)))
        return
    assert abs(r.log_evidence - want['logev']) < 1e-10
    devs = {'D': deviation(r.expected_dwell, want['dwell']), 'C': deviation(r.expected_censored, want['cens']),
            'I': deviation(r.expected_init, want['init']), 'jumps': deviation(r.expected_jumps, want['jumps'])}
    print(f"{case}: logev {abs(r.log_evidence - want['logev']):.1e}; in units of the bound and relative above the floor: "
          + ', '.join(f"{k} {u:.1e} / {v:.1e}" for k, (u, v) in devs.items()))
    for name, (units, _) in devs.items():
        assert units <= 1.0, (case, name, units)
    assert np.all(r.expected_dwell[:, T - 1] == 0)
    if case[3] == 'minlength':
        assert np.all(r.expected_dwell[:, 0] == 0)
    for s in range(S):
        pmf, total = r.lifetime_pmf(s), r.expected_dwell[s].sum()
        assert np.all(np.isnan(pmf)) if total == 0 else (np.array_equal(pmf, r.expected_dwell[s] / total) and abs(pmf.sum() - 1) < 1e-12)
    if S == 1 or T == 1:
        assert r.expected_dwell.sum() == 0 and r.expected_jumps.sum() == 0


def bit_case():
    rng = np.random.default_rng(41)
    model = C.random_model(rng, 2, 200)
    xs = [C.random_traj(rng, T, missing) for T, missing in ((40, ()), (65, (9,)), (193, (63, 65)), (65, ()))]
    return model, xs, DC.make_prior('nongeometric', rng, 2, 193)


def test_bit_for_bit_against_exact_dwell():
    """ the evidence, the NaN windows and the jumps are `exact_dwell`'s numbers: the same kernels on the same tables """
    model, xs, prior = bit_case()
    rng = np.random.default_rng(5)
    gap_model, gap_x = DLC.oracle_case(2, 130, 'order0_gap', 'markov')[:2]
    for m, trajs, pr, nan in ((model, xs, prior, 'propagate'), (gap_model, [gap_x], DC.make_prior('markov', rng, 2, 130), 'omit'),
                              (gap_model, [gap_x], DC.make_prior('markov', rng, 2, 130), 'propagate')):
        got, ref = bild_amd.exact_dwell_lengths(trajs, m, pr, nan=nan), bild_amd.exact_dwell(trajs, m, pr, nan=nan)
        for a, b in zip(got, ref):
            assert np.array_equal(a.log_evidence, b.log_evidence, equal_nan=True) and a.n_nan_windows == b.n_nan_windows
            assert np.array_equal(a.expected_jumps, b.expected_jumps, equal_nan=True)
            assert np.isnan(a.log_evidence) == (nan == 'propagate' and m is gap_model)


def test_init_and_identities_at_T1000():
    T = 1000
    rng = np.random.default_rng(31)
    model = C.random_model(rng, 2, T + 8, orders=np.ones((2, 3), dtype=int), d=3)
    x = C.random_traj(rng, T, (100, 500, 501), d=3)
    prior = bild_amd.DwellPrior.markov([[0.98, 0.02], [0.05, 0.95]], [0.6, 0.4], n=T)
    r, ref = bild_amd.exact_dwell_lengths(x, model, prior), bild_amd.exact_dwell(x, model, prior)
    assert r.n_nan_windows == 0 and np.isfinite(r.log_evidence) and r.log_evidence == ref.log_evidence
    D, Cn, lengths, post = r.expected_dwell, r.expected_censored, np.arange(1, T + 1), np.exp(ref.log_marginal_posterior)
    first = float(np.max(np.abs(r.expected_init - post[:, 0])))
    # sums of 10^3 terms whose total is of the order of T, or a count of jumps: 1e-8; shares of 1: 1e-9
    long_sums = {'sum D = jumps out': np.max(np.abs(D.sum(axis=1) - ref.expected_jumps.sum(axis=1))),
                 'sum (l - 1)(D + C) = stay': np.max(np.abs(((D + Cn) * (lengths - 1)).sum(axis=1) - ref.expected_stay)),
                 'sum l (D + C) = T': abs(((D + Cn) * lengths).sum() - T)}
    shares = {'sum C = 1': abs(Cn.sum() - 1), 'sum_l C = last marginal': np.max(np.abs(Cn.sum(axis=1) - post[:, T - 1]))}
    print(f"I = first marginal: {first:.1e}, " + ', '.join(f"{k}: {v:.1e}" for k, v in {**long_sums, **shares}.items()))
    assert first < 1e-10
    assert all(v < 1e-8 for v in long_sums.values()) and all(v < 1e-9 for v in shares.values())


def test_fisher_identity_by_central_differences():
    """ d logev / d log_dwell[s][l] = expected_dwell[s][l], d logev / d log_surv[s][l] = expected_censored[s][l] """
    S, T, h = 3, 65, 1e-5
    rng = np.random.default_rng(22)
    model = C.random_model(rng, S, T + 8)
    x = C.random_traj(rng, T, (30,))
    prior = DC.make_prior('nongeometric', rng, S, T)
    r = bild_amd.exact_dwell_lengths(x, model, prior)

    def logev(**tabs):
        tabs = {**{n: getattr(prior, n) for n in ('log_init', 'log_jump', 'log_dwell', 'log_surv')}, **tabs}
        return bild_amd.exact_dwell(x, model, bild_amd.DwellPrior(**tabs), marginals=False).log_evidence

    worst = 0.0
    for name, counts, picks in (('log_dwell', r.expected_dwell, (1, 2, 17, 63, T - 1)), ('log_surv', r.expected_censored, (1, 30, 64, T))):
        for s in range(S):
            for length in picks:
                up, dn = getattr(prior, name).copy(), getattr(prior, name).copy()
                assert np.isfinite(up[s, length - 1])
                up[s, length - 1] += h
                dn[s, length - 1] -= h
                rate = (logev(**{name: up}) - logev(**{name: dn})) / (2 * h)
                worst = max(worst, abs(rate - counts[s, length - 1]))
                assert abs(rate - counts[s, length - 1]) < 1e-6, (name, s, length, rate, counts[s, length - 1])
    print(f"worst deviation of a difference quotient from its count {worst:.1e}")


def test_bit_identity():
    model, xs, prior = bit_case()
    lengths = bild_amd.exact_dwell_lengths
    batch = lengths(xs, model, prior)
    assert all(np.isfinite(r.log_evidence) and np.all(np.isfinite(r.expected_dwell)) and r.expected_dwell.sum() > 0 for r in batch)
    assert all(same(a, b) for a, b in zip(batch, lengths(xs, model, prior)))
    order = [2, 0, 3, 1]
    permuted = lengths([xs[i] for i in order], model, prior)
    assert all(same(permuted[j], batch[i]) for j, i in enumerate(order))
    for x, r in zip(xs, batch):
        assert same(lengths(x, model, prior), r)
    # one trajectory per chunk, and two: a trajectory's share of a chunk, S = 2 and 193 frames (csrc/gauss_dwelllen.cpp)
    slot, part = 2 * 194, 2 * 4 * 193        # (four blocks of 64 start frames)
    per_traj = slot * 56 + (part + 2 * slot + 4 + 2) * 8 + 193 + 24
    for scratch in (1, 2 * per_traj + 8):
        assert all(same(a, b) for a, b in zip(batch, lengths(xs, model, prior, scratch_bytes=scratch)))


def test_trajectory_without_a_profile():
    rng = np.random.default_rng(3)
    model = C.random_model(rng, 2, 64)
    xs = [C.random_traj(rng, 50), C.random_traj(rng, 56)]
    no = DC.prior_of('impossible', rng, 2, 60, 50)
    r = bild_amd.exact_dwell_lengths(xs, model, no)
    assert r[0].log_evidence == -np.inf and all(np.all(np.isnan(getattr(r[0], f))) for f in FIELDS[2:])
    assert same(r[1], bild_amd.exact_dwell_lengths(xs[1], model, no))       # 56 frames: the one segment survives
    assert np.isfinite(r[1].log_evidence) and r[1].expected_dwell.sum() == 0 and abs(r[1].expected_censored[0, 55] - 1) < 1e-12


def test_c_abi_refusals():
    rng = np.random.default_rng(51)
    model = C.random_model(rng, 2, 40)
    x = C.random_traj(rng, 30)
    ts = model.trajset(x)
    p = DC.symmetric_chain(0.1, 30)
    good = (p.log_init, p.log_jump, p.log_dwell, p.log_surv)
    _lib.gauss_dwell_lengths(model.handle(), ts, *good)

    def bad(i, fn):
        args = [a.copy() for a in good]
        args[i] = fn(args[i])
        with pytest.raises(_lib.BildAmdError) as e:
            _lib.gauss_dwell_lengths(model.handle(), ts, *args)
        assert e.value.code == _lib.ERR_INVALID

    def put(index, value):
        def fn(a):
            a[index] = value
            return a
        return fn

    with pytest.raises(_lib.BildAmdError, match='more than the L = 29') as e:      # L shorter than the trajectory
        _lib.gauss_dwell_lengths(model.handle(), ts, good[0], good[1], good[2][:, :29], good[3][:, :29])
    assert e.value.code == _lib.ERR_INVALID
    for i in (0, 1, 2, 3):                          # a NaN or +inf entry anywhere
        bad(i, put((0,) * good[i].ndim, np.nan))
        bad(i, put((-1,) * good[i].ndim, np.inf))
    bad(1, put((1, 1), 0.0))                        # a self-jump
    bad(0, lambda a: np.full(2, -np.inf))
    with pytest.raises(_lib.BildAmdError, match='negative'):
        _lib.gauss_dwell_lengths(model.handle(), ts, *good, scratch_bytes=-1)

    def raw(T_max=30, flags=0, scratch=0, out=True):
        arrs = [_lib.f64(a) for a in good]
        spec = _lib.DwellLengthsOut()
        return _lib.lib().bild_gauss_dwell_lengths(model.handle()._h, ts._h, 30, *[_lib.dptr(a) for a in arrs], T_max, flags, scratch,
                                                  ctypes.byref(spec) if out else None)
    assert raw() == _lib.OK      # (every output NULL: nothing is written)
    assert raw(flags=2) == _lib.ERR_INVALID and raw(scratch=-1) == _lib.ERR_INVALID and raw(T_max=29) == _lib.ERR_INVALID
    assert raw(out=False) == _lib.ERR_INVALID
    five = C.random_model(rng, 5, 40)
    p5 = DC.make_prior('markov', rng, 5, 30)
    with pytest.raises(_lib.BildAmdError, match='at most 4') as e:
        _lib.gauss_dwell_lengths(five.handle(), five.trajset(x), p5.log_init, p5.log_jump, p5.log_dwell, p5.log_surv)
    assert e.value.code == _lib.ERR_UNSUPPORTED


# ---------------------------------------------------------------- the fits

def count_builds(monkeypatch):
    made = []
    real = _lib.GaussTrajSetHandle

    def counting(*a, **k):
        made.append(1)
        return real(*a, **k)
    monkeypatch.setattr(_lib, 'GaussTrajSetHandle', counting)
    return made


def test_fit_with_one_bin_is_fit_markov_prior(monkeypatch):
    """ edges = [1] is the Markov family: from the same start the two EMs take the same steps """
    model, trajs = DLC.markov_data()
    made = count_builds(monkeypatch)
    P0, init0 = DLC.MARKOV_START, np.array([0.5, 0.5])
    leave = 1 - np.diag(P0)
    start = (leave[:, None].copy(), (P0 - np.diag(np.diag(P0))) / leave[:, None], init0)
    worst_P = worst_ev = 0.0
    for k in range(1, 11):      # (a tol that no step meets: both return the parameters behind their k-th M-step)
        a = bild_amd.fit_markov_prior(trajs, model, start=(P0, init0), max_iter=k, tol=1e-300)
        b = bild_amd.fit_dwell_prior(trajs, model, edges=[1], start=start, max_iter=k, tol=1e-300)
        assert a.n_iter == b.n_iter == k and not a.converged and not b.converged and b.hazard.shape == (2, 1) and b.supported.all()
        P = b.jump * b.hazard + np.diag(1 - b.hazard[:, 0])
        worst_P = max(worst_P, float(np.max(np.abs(P - a.P))), float(np.max(np.abs(b.init - a.init))))
        worst_ev = max(worst_ev, float(np.max(np.abs(b.log_evidence - a.log_evidence))))
    print(f"10 iterations: evidence history within {worst_ev:.1e}, (P, init) within {worst_P:.1e}; totals {b.log_evidence[0]!r} -> {b.log_evidence[-1]!r}")
    assert worst_ev < 1e-9 and worst_P < 1e-9
    assert len(made) == 1


def test_fit_on_non_geometric_data(monkeypatch):
    model, trajs, profiles = DLC.hazard_data()
    T = len(trajs[0])
    made = count_builds(monkeypatch)
    clock = time.perf_counter()
    markov = bild_amd.fit_markov_prior(trajs, model, start=DLC.MARKOV_START)
    t_markov, clock = time.perf_counter() - clock, time.perf_counter()
    fit = bild_amd.fit_dwell_prior(trajs, model, edges=DLC.HAZARD_EDGES, start=markov)
    t_fit = time.perf_counter() - clock
    truth = DLC.hazard_prior(DLC.HAZARD_EDGES, DLC.HAZARD_TRUE, T)
    at_truth = sum(r.log_evidence for r in bild_amd.exact_dwell(trajs, model, truth, marginals=False))
    print(f"\nMarkov fit: {markov.n_iter} iterations, {t_markov:.2f} s (the table build among them), total {markov.log_evidence[-1]!r}, "
          f"P {markov.P.tolist()}\nhazard fit: {fit.n_iter} iterations, {t_fit:.2f} s, total {fit.log_evidence[0]!r} -> {fit.log_evidence[-1]!r}\n"
          f"  hazard {fit.hazard.tolist()} (generating {DLC.HAZARD_TRUE.tolist()}), supported {fit.supported.tolist()}\n"
          f"  init {fit.init.tolist()}, jump {fit.jump.tolist()}; total at the generating prior {at_truth!r}")
    assert markov.converged and fit.converged and fit.n_iter == len(fit.log_evidence)
    assert np.array_equal(fit.edges, [1, 4, 16]) and fit.hazard.shape == (2, 3) and fit.expected_dwell.shape == (2, T)
    assert np.all(np.diff(fit.log_evidence) >= -1e-9)                       # the history never decreases
    assert fit.log_evidence[-1] >= markov.log_evidence[-1] - 1e-9           # ... and starts at the Markov fit
    # one more EM step moves nothing by more than tol: from the fit's parameters the first M-step already meets tol
    again = bild_amd.fit_dwell_prior(trajs, model, edges=DLC.HAZARD_EDGES, start=(fit.hazard, fit.jump, fit.init), max_iter=1)
    assert again.converged and again.log_evidence[0] == fit.log_evidence[-1]
    assert np.array_equal(again.expected_dwell, fit.expected_dwell) and np.array_equal(again.expected_censored, fit.expected_censored)
    assert len(made) == 1                                                   # one trajectory set for the fits and the checks
    prior = fit.prior()
    assert isinstance(prior, bild_amd.DwellPrior) and prior.L == T
    bild_amd.DwellPrior(prior.log_init, prior.log_jump, prior.log_dwell, prior.log_surv)        # passes the checks
    total = sum(r.log_evidence for r in bild_amd.exact_dwell(trajs, model, prior, marginals=False))
    assert abs(total - fit.log_evidence[-1]) < 1e-9, (total, fit.log_evidence[-1])
