"""
The dwell-time recursion on the GPU (bild_amd.exact.exact_dwell, csrc/gauss_dwell.hip): against the
NumPy oracle tests/dwell_oracle.py around the 64-frame tiles, at one to four states, beyond the 256 frames of the statistics
kernels' first workgroup and under the priors of `dwell_cases.prior_of` (`dwell_cases.ORACLE_CASES`), a ragged batch of six
against the oracle, a sharp posterior, against `exact_sample` through the symmetric two-state chain, Fisher's identity for
the expected counts, T = 1000, bit-identity across calls, batch orders, batch sizes and chunking, and the EM fit of a Markov
prior.  Tolerances as in tests/test_gpu_segment_dp.py: logev, finite log marginals and the MAP log joint 1e-10, counts 1e-9
relative.  Worst seen on the MI355X: logev 1.1e-13, log marginals 1.6e-13, MAP log joint 3.4e-13, counts
5.0e-12 absolute; Fisher quotients within 2.5e-9 of the counts; `-s` prints every figure.
With the cases at S = 1 and 4, T > 256 and the hard priors, worst seen on the MI355X: logev 9.7e-13 (S = 1, T = 130, non-geometric:
one profile, the evidence is its log joint), log marginals 6.4e-12 (the absorbing prior; 9.7e-13 elsewhere), MAP log joint
2.3e-11 (S = 3, T = 321, frame 128 missing; 1.0e-12 elsewhere), counts 3.8e-11 absolute (an expected stay at T = 321).
The ragged batch: logev 2.3e-13, log marginals 4.8e-13, MAP log joint 6.8e-13, counts 1.4e-11 absolute.  The sharp case (its bar
3.7e-9): logev 2.8e-14, MAP log joint 2.8e-14, the 224 log marginals at or above -600 1.1e-13, counts 1.9e-12 absolute; of the 36
entries whose reference is below -600, the device has -inf on the 34 where the oracle has, and at most -707.48 on the other two.
"""
import ctypes

import numpy as np
import pytest

import bild_amd
import dwell_cases as DC
import dwell_oracle as DO
import gauss_oracle as G
import segment_cases as C
from bild_amd import _lib
from bild_amd.profiles import segments_from_states

pytestmark = pytest.mark.gpu


def check_against_oracle(r, want, W, F, prior, exact_map):
    T = F.shape[1] - 1
    assert r.n_nan_windows == want['n_nan_windows']
    for name, got, ref in (('logev', r.log_evidence, want['logev']), ('map_logjoint', r.map_log_joint, want['map_logjoint'])):
        print(name, got, ref, abs(got - ref))
        if np.isfinite(ref):
            assert abs(got - ref) < 1e-10, (name, got, ref)
        else:
            assert np.array_equal(got, ref, equal_nan=True), (name, got, ref)
    got, ref = r.log_marginal_posterior, want['log_post']
    assert got.shape == (F.shape[0], T)
    fin = np.isfinite(ref)
    assert np.array_equal(fin, np.isfinite(got)) and np.array_equal(np.isnan(got), np.isnan(ref))
    if fin.any():
        print('log_post', np.max(np.abs(got[fin] - ref[fin])))
        assert np.max(np.abs(got[fin] - ref[fin])) < 1e-10
    for name, got, ref in (('jumps', r.expected_jumps, want['exp_jumps']), ('stay', r.expected_stay, want['exp_stay'])):
        assert got.shape == ref.shape
        fin = np.isfinite(ref)
        # (a reference that is not finite: the same value at the same place)
        assert np.array_equal(got[~fin], ref[~fin], equal_nan=True), (name, got, ref)
        if fin.any():
            print(name, np.max(np.abs(got[fin] - ref[fin])))
            assert np.all(np.abs(got[fin] - ref[fin]) <= 1e-9 * np.abs(ref[fin])), (name, got, ref)
    if want['map_states'] is None:
        assert r.map_profile is None
        return
    states = np.asarray(r.map_profile[:])
    if exact_map:
        assert np.array_equal(states, want['map_states'])
    # (with missing frames every switch frame inside a gap ties: the profile is checked by its value)
    assert abs(prior.log_prob(states) + G.logl_tables(W, F, states) - want['map_logjoint']) < 1e-10


@pytest.mark.parametrize('S,T,missing,kind', DC.ORACLE_CASES)
def test_against_oracle(S, T, missing, kind):
    case = (S, T, missing, kind)
    model, x, prior, W, F = DC.oracle_case(case)
    want = DC.oracle_answer(case)
    print(f"oracle {DC.ORACLE_SECONDS[case]:.1f} s")
    r = bild_amd.exact_dwell(x, model, prior)
    check_against_oracle(r, want, W, F, prior, exact_map=not missing)
    # the forward pass alone gives the same evidence and MAP, bit for bit
    f = bild_amd.exact_dwell(x, model, prior, marginals=False)
    assert f.log_marginal_posterior is None and f.expected_jumps is None
    assert f.log_evidence == r.log_evidence and f.map_profile == r.map_profile
    assert np.array_equal(f.map_log_joint, r.map_log_joint, equal_nan=True)
    if kind == 'impossible':
        assert r.log_evidence == -np.inf and r.map_profile is None and np.isnan(r.map_log_joint)
        assert np.all(np.isnan(r.log_marginal_posterior)) and r.log_marginal_posterior.shape == (S, T)
        assert np.all(np.isnan(r.expected_jumps)) and np.all(np.isnan(r.expected_stay))
        with pytest.raises(ValueError, match='-inf: no profile of positive weight'):
            r.draw(8)
    else:
        assert np.isfinite(r.log_evidence) and r.map_profile is not None
    if kind == 'flip':
        assert r.expected_jumps.sum() == pytest.approx(T - 1, abs=1e-9)
        assert np.all(r.expected_stay <= 1e-12)
    if S == 1:
        assert np.array_equal(r.expected_jumps, [[0.0]]) and np.all(r.log_marginal_posterior == 0.0)
        assert r.map_profile is not None and np.all(np.asarray(r.map_profile[:]) == 0)


def test_ragged_batch_against_oracle():
    """ four states, non-geometric tables, six trajectories in one call: five are shorter than the call's longest """
    model, prior, xs, tabs = DC.ragged_case()
    batch = bild_amd.exact_dwell(xs, model, prior)
    for j, ((T, missing), r, want, (W, F)) in enumerate(zip(DC.RAGGED, batch, DC.ragged_answers(), tabs)):
        print(f"trajectory {j}, T = {T}, oracle {DC.ORACLE_SECONDS['ragged', j]:.1f} s")
        assert np.isfinite(want['logev']) and len(r.traj) == T
        check_against_oracle(r, want, W, F, prior, exact_map=not missing)
    # one trajectory per chunk
    chunked = bild_amd.exact_dwell(xs, model, prior, scratch_bytes=1)
    assert all(same(a, b) for a, b in zip(batch, chunked))


def test_sharp_posterior():
    """
    Steps that depend on the state 50-fold: W down to -1.1e5, and marginals that the oracle holds down to e^-710 and then at 0.
    The bars for logev, the MAP log joint and the log marginals are the file's 1e-10 times max|finite W| / 3e3 (about 3.7e-9):
    1e-10 was set where the summed terms are ~3e3 (the comment in `test_T1000`), and the rounding of an exponent grows with its size.
    A log marginal whose reference is below -600 or -inf must be -inf or below -590.
    """
    model, x, prior, st, W, F = DC.sharp_case()
    want = DC.sharp_answer()
    scale = max(1.0, np.max(np.abs(W[np.isfinite(W)])) / 3e3)
    bar = 1e-10 * scale
    r = bild_amd.exact_dwell(x, model, prior)
    assert r.n_nan_windows == 0 == want['n_nan_windows']
    assert np.array_equal(np.asarray(r.map_profile[:]), st) and np.array_equal(want['map_states'], st)
    print(f"sharp: oracle {DC.ORACLE_SECONDS['sharp']:.1f} s, min finite W {np.min(W[np.isfinite(W)]):.4g}, scale {scale:.2f}, bar {bar:.3g}")
    for name, got, ref in (('logev', r.log_evidence, want['logev']), ('map_logjoint', r.map_log_joint, want['map_logjoint'])):
        print(name, got, ref, abs(got - ref))
        assert abs(got - ref) < bar, (name, got, ref)
    got, ref = r.log_marginal_posterior, want['log_post']
    assert got.shape == ref.shape == (2, len(x)) and not np.any(np.isnan(got)) and not np.any(np.isnan(ref))
    firm = ref >= -600
    low = got[~firm]
    print(f"log_post: {int(firm.sum())} entries at or above -600: worst {np.max(np.abs(got[firm] - ref[firm])):.3e}; {low.size} below "
          f"(reference -inf on {int(np.sum(ref == -np.inf))}): device -inf on {int(np.sum(low == -np.inf))}, largest other "
          f"{np.max(low[low > -np.inf], initial=-np.inf):.2f}")
    assert np.max(np.abs(got[firm] - ref[firm])) < bar
    assert np.all((low == -np.inf) | (low < -590))
    for name, got, ref in (('jumps', r.expected_jumps, want['exp_jumps']), ('stay', r.expected_stay, want['exp_stay'])):
        print(name, np.max(np.abs(got - ref)), np.max(np.abs(got - ref) - 1e-9 * np.abs(ref)))
        assert np.all(np.abs(got - ref) <= 1e-9 * np.abs(ref) + 1e-12), (name, got, ref)


@pytest.mark.parametrize('nan', ['propagate', 'omit'])
def test_order0_gap_against_oracle(nan):
    T = 70
    rng = np.random.default_rng(7)
    model = bild_amd.GenericGaussianModel([[(np.append(np.arange(T + 8) * 0.5 + 0.1, 50.0), 0.3 * s, 0),
                                            (np.arange(T + 8) * (0.5 + s), 0.0, 1)] for s in range(2)])
    x = C.random_traj(rng, T)
    x[60:68, 0] = np.nan    # a later ss_order-0 segment inside frames 60 .. 67 has no valid value: across the tile's edge
    prior = DC.make_prior('markov', rng, 2, T)
    W, F = C.tables(model, x)
    want = DO.solve(W, F, prior, nan=nan)
    assert want['n_nan_windows'] > 0 and np.isnan(want['logev']) == (nan == 'propagate')
    r = bild_amd.exact_dwell(x, model, prior, nan=nan)
    check_against_oracle(r, want, W, F, prior, exact_map=False)
    assert r.map_profile is not None and np.isfinite(r.map_log_joint)


def test_symmetric_chain_against_exact_sample():
    T, p = 60, 0.08
    rng = np.random.default_rng(11)
    model = C.random_model(rng, 2, T + 8, orders=np.ones((2, 2), dtype=int))
    x = C.random_traj(rng, T, (17,))
    per_k = bild_amd.exact_sample(x, model, k_max=T - 1)
    logev, post = DC.symmetric_mixture(p, T, per_k.evidence, [per_k.log_marginal_posterior_k(k) for k in range(T)])
    r = bild_amd.exact_dwell(x, model, DC.symmetric_chain(p, T))
    print(r.log_evidence, logev, np.max(np.abs(np.exp(r.log_marginal_posterior) - post)))
    assert abs(r.log_evidence - logev) < 1e-9
    assert np.max(np.abs(np.exp(r.log_marginal_posterior) - post)) < 1e-9


def test_fisher_identity_by_central_differences():
    """ d logev / d log_jump[s'][s] = expected_jumps[s'][s]; d logev / d log P_ss = expected_stay[s] """
    S, T, h = 3, 65, 1e-5
    rng = np.random.default_rng(21)
    model = C.random_model(rng, S, T + 8)
    x = C.random_traj(rng, T, (30,))
    prior = DC.make_prior('markov', rng, S, T)
    r = bild_amd.exact_dwell(x, model, prior)

    def logev(jump=prior.log_jump, dwell=prior.log_dwell, surv=prior.log_surv):
        return bild_amd.exact_dwell(x, model, bild_amd.DwellPrior(prior.log_init, jump, dwell, surv), marginals=False).log_evidence

    n_checked = 0
    for a in range(S):
        for b in range(S):
            if prior.log_jump[a, b] == -np.inf:
                assert r.expected_jumps[a, b] == 0.0
                continue
            up, dn = prior.log_jump.copy(), prior.log_jump.copy()
            up[a, b] += h
            dn[a, b] -= h
            rate = (logev(jump=up) - logev(jump=dn)) / (2 * h)
            print('jump', a, b, rate, r.expected_jumps[a, b])
            assert abs(rate - r.expected_jumps[a, b]) < 1e-6
            n_checked += 1
    assert n_checked == 5       # 0 -> 2 is forbidden
    lm1 = np.arange(T, dtype=float)
    for s in range(S):
        # log P_ss enters log_dwell[s][l] and log_surv[s][l] as (l - 1) log P_ss
        rates = []
        for sign in (1, -1):
            dwell, surv = prior.log_dwell.copy(), prior.log_surv.copy()
            dwell[s] += sign * h * lm1
            surv[s] += sign * h * lm1
            rates.append(logev(dwell=dwell, surv=surv))
        rate = (rates[0] - rates[1]) / (2 * h)
        print('stay', s, rate, r.expected_stay[s])
        assert abs(rate - r.expected_stay[s]) < 1e-6


def test_T1000():
    T = 1000
    rng = np.random.default_rng(31)
    model = C.random_model(rng, 2, T + 8, orders=np.ones((2, 3), dtype=int), d=3)
    x = C.random_traj(rng, T, (100, 500, 501), d=3)
    prior = bild_amd.DwellPrior.markov([[0.98, 0.02], [0.05, 0.95]], [0.6, 0.4], n=T)
    r = bild_amd.exact_dwell(x, model, prior)
    assert r.n_nan_windows == 0 and np.isfinite(r.log_evidence)
    post = np.exp(r.log_marginal_posterior)
    # every segment weight carries the rounding of alpha + omega + W + gamma - logev, terms of size ~3e3: ~1e-12 relative;
    # a frame's marginals are a share of 1, the occupancy a sum over 999 frames
    print(np.max(np.abs(post.sum(axis=0) - 1)), r.expected_stay + r.expected_jumps.sum(axis=1) - post[:, :-1].sum(axis=1))
    assert np.max(np.abs(post.sum(axis=0) - 1)) < 1e-9
    assert np.max(np.abs(r.expected_stay + r.expected_jumps.sum(axis=1) - post[:, :-1].sum(axis=1))) < 1e-8

    def joint(profiles):
        seg_start, seg_state = segments_from_states(np.asarray(profiles))
        return model.logL_segments(seg_start, seg_state, [x]) + np.array([prior.log_prob(p) for p in profiles])

    states = np.asarray(r.map_profile[:])
    assert abs(joint([states])[0] - r.map_log_joint) < 1e-9
    # not beaten by random profiles (perturbations of the MAP among them) ...
    others = []
    for i in range(200):
        if i % 2:
            k = int(rng.integers(0, 12))
            cuts = np.sort(rng.choice(np.arange(1, T), size=k, replace=False))
            st = (np.searchsorted(cuts, np.arange(T), side='right') + int(rng.integers(0, 2))) % 2
        else:
            st = states.copy()
            a = int(rng.integers(0, T - 1))
            st[a:a + int(rng.integers(1, 30))] ^= 1
        others.append(st)
    assert np.all(joint(others) <= r.map_log_joint + 1e-9)
    # ... nor by the best profile of any k <= 20
    per_k = bild_amd.exact_sample(x, model, k_max=20, marginals=False)
    best = [np.asarray(per_k.map_profile(k)[:]) for k in range(21)]
    assert np.all(joint(best) <= r.map_log_joint + 1e-9)


def same(a, b):
    return (a.log_evidence == b.log_evidence and a.map_log_joint == b.map_log_joint and a.map_profile == b.map_profile
            and a.n_nan_windows == b.n_nan_windows and np.array_equal(a.log_marginal_posterior, b.log_marginal_posterior)
            and np.array_equal(a.expected_jumps, b.expected_jumps) and np.array_equal(a.expected_stay, b.expected_stay))


def test_bit_identity():
    rng = np.random.default_rng(41)
    model = C.random_model(rng, 2, 200)
    xs = [C.random_traj(rng, T, missing) for T, missing in ((40, ()), (65, (9,)), (193, (63, 65)), (65, ()))]
    prior = DC.make_prior('markov', rng, 2, 193)
    batch = bild_amd.exact_dwell(xs, model, prior)
    assert all(np.isfinite(r.log_evidence) for r in batch)
    again = bild_amd.exact_dwell(xs, model, prior)
    assert all(same(a, b) for a, b in zip(batch, again))
    order = [2, 0, 3, 1]
    permuted = bild_amd.exact_dwell([xs[i] for i in order], model, prior)
    assert all(same(permuted[j], batch[i]) for j, i in enumerate(order))
    for x, r in zip(xs, batch):
        assert same(bild_amd.exact_dwell(x, model, prior), r)
    # one trajectory per chunk, and two
    per_traj = 2 * 194 * 72 + 2 * 4 * 193 * 8 + 4096
    for scratch in (1, 2 * per_traj):
        chunked = bild_amd.exact_dwell(xs, model, prior, scratch_bytes=scratch)
        assert all(same(a, b) for a, b in zip(batch, chunked))


def test_c_abi_refusals():
    rng = np.random.default_rng(51)
    model = C.random_model(rng, 2, 40)
    x = C.random_traj(rng, 30)
    ts = model.trajset(x)
    p = DC.symmetric_chain(0.1, 30)
    good = (p.log_init, p.log_jump, p.log_dwell, p.log_surv)
    _lib.gauss_dwell_evidence(model.handle(), ts, *good)

    def bad(i, fn):
        args = [a.copy() for a in good]
        args[i] = fn(args[i])
        with pytest.raises(_lib.BildAmdError) as e:
            _lib.gauss_dwell_evidence(model.handle(), ts, *args)
        assert e.value.code == _lib.ERR_INVALID

    def put(index, value):
        def fn(a):
            a[index] = value
            return a
        return fn

    short = [good[0], good[1], good[2][:, :29], good[3][:, :29]]       # L shorter than the trajectory
    with pytest.raises(_lib.BildAmdError) as e:
        _lib.gauss_dwell_evidence(model.handle(), ts, *short)
    assert e.value.code == _lib.ERR_INVALID
    for i in (0, 1, 2, 3):                          # a NaN or +inf entry anywhere
        bad(i, put((0,) * good[i].ndim, np.nan))
        bad(i, put((-1,) * good[i].ndim, np.inf))
    bad(1, put((1, 1), 0.0))                        # a self-jump
    bad(0, lambda a: np.full(2, -np.inf))

    def raw(T_max=30, flags=0, scratch=0):
        arrs = [_lib.f64(a) for a in good]
        spec = _lib.DwellOut()
        return _lib.lib().bild_gauss_dwell_evidence(model.handle()._h, ts._h, 30, *[_lib.dptr(a) for a in arrs], T_max, flags, scratch,
                                                   ctypes.byref(spec))
    assert raw() == _lib.OK      # (every output NULL: nothing is written)
    assert raw(flags=2) == _lib.ERR_INVALID and raw(scratch=-1) == _lib.ERR_INVALID and raw(T_max=29) == _lib.ERR_INVALID


def test_fit_markov_prior(monkeypatch):
    n, T = 64, 200
    lags = np.arange(T + 8, dtype=float)
    model = bild_amd.GenericGaussianModel([[(np.where(lags > 0, g * lags ** a + 0.1, 0), 0.0, 1)] * 2
                                           for g, a in ((0.3, 0.6), (2.0, 0.9))])
    P_true, init_true = np.array([[0.95, 0.05], [0.1, 0.9]]), np.array([0.5, 0.5])
    rng = np.random.default_rng(61)
    profiles = []
    for _ in range(n):
        st = np.empty(T, dtype=int)
        st[0] = rng.choice(2, p=init_true)
        for t in range(1, T):
            st[t] = rng.choice(2, p=P_true[st[t - 1]])
        profiles.append(st)
    trajs = model.trajectories_from_loopingprofiles(profiles, seed=62)

    builds = []
    make = _lib.GaussTrajSetHandle

    def counted(*a, **k):
        builds.append(1)
        return make(*a, **k)
    monkeypatch.setattr(_lib, 'GaussTrajSetHandle', counted)
    start = np.array([[0.9, 0.1], [0.2, 0.8]])      # the switching probabilities 2x off
    fit = bild_amd.fit_markov_prior(trajs, model, start=start)
    assert len(builds) == 1
    print('n_iter', fit.n_iter, 'P', fit.P.tolist(), 'init', fit.init.tolist(), 'log evidence', fit.log_evidence[0], fit.log_evidence[-1])
    assert fit.converged and fit.n_iter == len(fit.log_evidence)
    assert np.all(np.diff(fit.log_evidence) >= -1e-9)
    at_truth = sum(r.log_evidence for r in bild_amd.exact_dwell(trajs, model, bild_amd.DwellPrior.markov(P_true, init_true, n=T),
                                                                marginals=False))
    print('at the truth', at_truth)
    assert fit.log_evidence[-1] >= at_truth - 1e-6
    more = bild_amd.fit_markov_prior(trajs, model, start=(fit.P, fit.init), max_iter=1)
    assert np.max(np.abs(more.P - fit.P)) < 1e-8
    assert len(builds) == 1                         # the same set serves every call
    assert np.allclose(fit.P.sum(axis=1), 1) and abs(fit.init.sum() - 1) < 1e-12
