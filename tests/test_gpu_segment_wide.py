"""
The three fixed-k exact paths on the GPU beyond S = 3 and T = 256 (tests/segment_wide_cases.py; tests/test_segment_wide.py
asserts the conditions on these inputs without a GPU):

* `exact_sample` (csrc/gauss_segdp.hip) against `segment_oracle.solve_fast` at one, four and five states, under transition
  matrices with a forced cycle, a state that is never left and one that is never entered, at five and six 64-frame tiles
  (the last workgroup of `segdp_cover_kernel` / `segdp_carry_kernel` partial), with NaN windows across a tile edge, in a
  ragged set of six, and with 264 (trajectory, k) rows for the 256 lanes of `segdp_backtrack_kernel`;
* `exact_draw` (csrc/gauss_segdraw.hip) replayed draw for draw against `segment_draw_oracle.draws` on the same cases;
* `exact_evidence` (csrc/exact.hip) against `exact_oracle` at k = 4 ... 15, S = 1, 4 and 5, whole blocks of 4096 profiles, and
  marginal accumulators up to the S T = 8192 allowed.

The bars are those of tests/test_gpu_segment_dp.py, test_gpu_segment_draw.py and test_gpu_exact.py, through their own
assertions.  `-s` prints the worst deviation of every case and the seconds of every oracle answer.
Worst seen on the MI355X: recursion -- logev 3.2e-12 and map_logL 3.2e-12 (the gap case; 2.3e-13 elsewhere), KL 8.9e-11 at (3, 321),
which is the double-precision oracle's own rounding there (8.9e-11 against `solve_fast` in long double), log marginals 2.7e-12; every
replayed draw equal to the oracle's; enumeration -- logev bit for bit, KL 6.5e-14, marginals 5.7e-14.  No oracle answer took more than
0.89 s on the GPU machine (the enumeration and reduction of 449 064 profiles).  Log marginals below -600, where the device's linear
weights underflow: `test_marginals_below_the_linear_range`.  T = 1800 and T = 2048 with marginals launch and agree: 73 984 B and 81 920 B of LDS a workgroup.
"""
import numpy as np
import pytest

import bild_amd
import exact_oracle as X
import segment_cases as C
import segment_wide_cases as WC
from bild_amd import _lib
from bild_amd.amis import CFC
from test_gpu_exact import rouse_model, rouse_traj
from test_gpu_exact import same as same_evidence
from test_gpu_segment_dp import check_against_enumeration, check_against_oracle, same
from test_gpu_segment_draw import check_replay as replay_assertions
from test_gpu_segment_draw import same_draws

pytestmark = pytest.mark.gpu


def within_time(*keys):
    for key in keys:
        print(f"oracle {key}: {WC.ORACLE_SECONDS[key]:.2f} s")
        assert WC.ORACLE_SECONDS[key] < WC.ORACLE_LIMIT, key


def report(label, r, out):
    """ the worst deviations of `ExactSamplingResults` r from the oracle's dictionary, printed before anything is asserted """
    worst = {}
    for name, got, want in (('logev', r.evidence, out['logev']), ('KL', r.KL, out['KL']), ('map_logL', r.map_logL, out['map_logL'])):
        fin = np.isfinite(want)
        worst[name] = float(np.max(np.abs(np.asarray(got)[fin] - want[fin]))) if fin.any() else 0.0
    got = np.array([r.log_marginal_posterior_k(k) for k in range(len(r.k))])
    fin = np.isfinite(out['log_post']) & np.isfinite(got)
    worst['log_post'] = float(np.max(np.abs(got[fin] - out['log_post'][fin]))) if fin.any() else 0.0
    print(f"{label}: " + ', '.join(f"{k} {v:.2e}" for k, v in worst.items()))
    return worst


# ------------------------------------------------------------------------------------------------ the segment recursion
@pytest.mark.parametrize('name', list(WC.SEGMENT_CASES))
def test_segment_recursion_against_oracle(name):
    S, T, missing, trans, _, _ = WC.SEGMENT_CASES[name]
    model, x, W, F, k_max, nan = WC.segment_case(name)
    out = WC.segment_answer(name)
    within_time(name)
    r = bild_amd.exact_sample(x, model, k_max=k_max, nan=nan)
    report(name, r, out)
    check_against_oracle(r, None, out, model, x, W, F, same_map=name in WC.SAME_MAP)
    if S == 1:
        assert r.n_profiles == [1] + [0] * k_max and np.isfinite(r.evidence[0]) and np.all(r.evidence[1:] == -np.inf)
        assert np.all(np.asarray(r.map_profile(0)[:]) == 0) and all(r.map_profile(k) is None for k in range(1, k_max + 1))
        assert np.all(np.isnan(r.log_marginal_posterior_k(1)))
    elif missing == 'gap':
        assert np.all(np.isfinite(r.evidence[:2])) and np.all(np.isfinite(r.map_logL))
        assert np.all(np.isnan(r.evidence[2:])) if nan == 'propagate' else np.all(np.isfinite(r.evidence)) and min(r.n_omitted[2:]) > 0
    else:
        assert np.array_equal(np.isfinite(r.evidence), np.arange(k_max + 1) <= T - 1)
    if trans == 'sink':         # state 3 is never left: a profile of k >= 1 switches cannot start there
        assert all(r.log_marginal_posterior_k(k)[3, 0] == -np.inf for k in range(1, k_max + 1))
    if trans == 'source':       # state 0 is never entered: past the first segment it is gone
        assert all(r.log_marginal_posterior_k(k)[0, -1] == -np.inf for k in range(1, k_max + 1))
    # the forward pass alone: the same evidence and MAP
    f = bild_amd.exact_sample(x, model, k_max=k_max, nan=nan, marginals=False)
    assert np.array_equal(f.evidence, r.evidence, equal_nan=True) and np.array_equal(f._seg_start, r._seg_start)


def test_ragged_set_against_oracle():
    """ six trajectories of four states in one call: `ld`, `slot`, `ntile` and `Tm` are the call's, not the trajectory's """
    model, xs, tabs = WC.ragged_case()
    answers = WC.ragged_answers()
    within_time(*[('ragged', j) for j in range(len(xs))])
    batch = bild_amd.exact_sample(xs, model, k_max=WC.RAGGED_K_MAX)
    for j, ((T, missing), r, out, (W, F)) in enumerate(zip(WC.RAGGED, batch, answers, tabs)):
        report(f"ragged {j} (T = {T})", r, out)
        check_against_oracle(r, None, out, model, xs[j], W, F, same_map=j in WC.RAGGED_SAME_MAP)
    for a, b in zip(batch, bild_amd.exact_sample(xs, model, k_max=WC.RAGGED_K_MAX, scratch_bytes=1)):      # one trajectory per chunk
        same(a, b)
    for x, a in zip(xs, batch):
        same(a, bild_amd.exact_sample(x, model, k_max=WC.RAGGED_K_MAX))


def test_backtrack_second_workgroup():
    """ 44 trajectories x 6 levels = 264 rows of `segdp_backtrack_kernel`: trajectories 42 and 43 reach the second workgroup """
    model, xs = WC.backtrack_case()
    batch = bild_amd.exact_sample(xs, model, k_max=WC.BACKTRACK_K_MAX)
    assert len(batch) * (WC.BACKTRACK_K_MAX + 1) > 256
    for x, a in zip(xs, batch):
        same(a, bild_amd.exact_sample(x, model, k_max=WC.BACKTRACK_K_MAX))
    for j in WC.BACKTRACK_ORACLE:
        W, F, out = WC.backtrack_answer(j)
        within_time(('backtrack', j))
        report(f"backtrack {j} (T = {len(xs[j])})", batch[j], out)
        check_against_oracle(batch[j], None, out, model, xs[j], W, F, same_map=False)
        assert all(np.count_nonzero(np.diff(np.asarray(batch[j].map_profile(k)[:]))) == k for k in range(min(5, len(xs[j]) - 1) + 1))


def test_marginals_below_the_linear_range():
    """
    `segdp_cover_kernel` sums the marginal weights of a level in linear scale against the level's `map_logL`, so a marginal
    more than a double's range below the MAP is 0: -inf where `segment_oracle` holds a finite value (DESIGN.md section 18,
    "Range").  Four states told far apart on 257 frames (five tiles): the oracle's log marginals reach -2960 at k = 0 and -955
    at k = 1.  Everything but the marginals is held as everywhere (`check_against_oracle`); a log marginal of the oracle
    at or above -600 to 1e-10; one between -700 and -600 must be finite and within `sharp_bar`, the digits the subnormal
    range leaves it (about 1e-6 at -700); one below -700 must be -inf or below -699; NaN nowhere, -inf where the oracle's is.
    On the MI355X: 3808 entries at or above -600, worst 1.5e-12; the 18 between (all at k = 1, the lowest -695.8) finite, worst
    2.2e-12 (bar 1.0e-10: at k = 1 the subnormal term is still below it); of the 286 below -700 the device has -inf on 280 (one
    state's whole row at k = 0, 23 entries at k = 1) and the oracle's value within 7.9e-4 on the other six (-742.0 ... -704.5).
    """
    model, x, W, F = WC.sharp_case()
    out = WC.sharp_answer()
    within_time('sharp')
    T = len(x)
    r = bild_amd.exact_sample(x, model, k_max=WC.SHARP_K_MAX)
    report('sharp', r, out)
    check_against_oracle(r, None, out, model, x, W, F, same_map=True, marginals=False)
    counts = np.zeros(4, dtype=int)
    worst = np.zeros(3)
    for k in range(WC.SHARP_K_MAX + 1):
        got, want = r.log_marginal_posterior_k(k), out['log_post'][k]
        assert got.shape == want.shape and not np.any(np.isnan(got)) and not np.any(np.isnan(want))
        assert np.all(got[want == -np.inf] == -np.inf)
        firm, low = want >= WC.SHARP_FIRM, want < WC.SHARP_FLOOR
        band = ~firm & ~low
        err = np.abs(got - np.where(np.isfinite(want), want, 0.0))
        bar = WC.sharp_bar(np.where(band, want, 0.0), k, T, out['n_profiles'][k])
        lost = low & (got == -np.inf)
        kept = low & np.isfinite(got)
        counts += [firm.sum(), band.sum(), lost.sum(), kept.sum()]
        worst = np.maximum(worst, [np.max(err[firm], initial=0.0), np.max(err[band], initial=0.0), np.max(err[kept], initial=0.0)])
        print(f"sharp k = {k}: {int(firm.sum())} at or above {WC.SHARP_FIRM:g}, worst {np.max(err[firm], initial=0.0):.2e}; {int(band.sum())} down to "
              f"{WC.SHARP_FLOOR:g} (lowest {np.min(want[band], initial=0.0):.1f}), worst {np.max(err[band], initial=0.0):.2e}, bars "
              f"{np.min(bar[band], initial=np.inf):.2e} ... {np.max(bar[band], initial=0.0):.2e}; {int(low.sum())} below: -inf on {int(lost.sum())}, finite on "
              f"{int(kept.sum())} ({np.min(want[kept], initial=0.0):.1f} ... {np.max(want[kept], initial=-np.inf):.1f}, worst {np.max(err[kept], initial=0.0):.2e})")
        assert np.all(err[firm] < 1e-10), (k, np.max(err[firm]))
        assert np.all(np.isfinite(got[band])) and np.all(err[band] <= bar[band]), k
        assert np.all((got[low] == -np.inf) | (got[low] < WC.SHARP_FLOOR + 1)), k
    print(f"sharp: {counts.tolist()} entries (firm, band, lost, kept below), worst {worst.tolist()}")
    assert counts[1] > 0 and counts[2] + counts[3] > 0      # (the case reaches both ranges: tests/test_segment_wide.py)


def test_sample_against_evidence_T257_S4():
    model, x, W, F, k_max, nan = WC.segment_case('s4_T257')
    r = bild_amd.exact_sample(x, model, k_max=k_max)
    for k in (0, 1):
        check_against_enumeration(r, k, bild_amd.exact_evidence(x, model, k), same_map=False)


# ------------------------------------------------------------------------------------------------------------ the draws
def check_replay(label, d, x, model, ks, want_start, want_state, fragile, consumed, allowed):
    """ the assertions of `test_gpu_segment_draw.test_replay_against_oracle`, its own helper, and every switch an allowed one """
    states = replay_assertions(label, d, x, model, ks, want_start, want_state, fragile, consumed, allowed)
    assert np.all(model.transitions[states[:, :-1], states[:, 1:]] | (states[:, :-1] == states[:, 1:]))


@pytest.mark.parametrize('name', WC.REPLAY_CASES)
def test_replay_against_oracle(name):
    model, x, W, F, k_max, nan = WC.segment_case(name)
    u, ks, want_start, want_state, fragile, consumed = WC.replay_answer(name)
    within_time(('replay', name))
    r = bild_amd.exact_sample(x, model, k_max=k_max, nan='omit', marginals=False)
    d = r.draw(WC.N_REPLAY, k=ks, uniforms=u)
    check_replay(name, d, x, model, ks, want_start, want_state, fragile, consumed, 0.001 * WC.N_REPLAY)
    if model.nStates == 1:
        assert np.all(d.k == 0) and np.all(d.seg_start[:, 1:] == len(x)) and np.all(d.states() == 0)


def test_ragged_draws_in_one_call():
    model, xs, tabs = WC.ragged_case()
    u, ks = WC.ragged_replay_inputs()
    n = WC.N_RAGGED_DRAWS
    res = bild_amd.exact_sample(xs, model, k_max=WC.RAGGED_K_MAX, nan='omit', marginals=False)
    draws = bild_amd.exact_draw(res, n, k=ks, uniforms=u)
    for j, (x, d) in enumerate(zip(xs, draws)):
        alone = bild_amd.exact_sample(x, model, k_max=WC.RAGGED_K_MAX, nan='omit', marginals=False)
        same_draws(d, alone.draw(n, k=ks[j], uniforms=u[j]))
    for j in WC.RAGGED_DRAWN:
        want_start, want_state, fragile, consumed = WC.ragged_replay_answer(j)
        within_time(('ragged_replay', j))
        check_replay(f"ragged {j}", draws[j], xs[j], model, ks[j], want_start, want_state, fragile, consumed, 1)


# ------------------------------------------------------------------------------------------------------ the enumeration
def check_enumeration(label, got, model, x, k, tables=False):
    """ the assertions of `test_gpu_exact.test_million_profiles_against_oracle`, the logLs from the model's own `logL_segments` """
    T, S = len(x), model.nStates
    want, seg_start, seg_state, logL = WC.enum_reference(model, x, k, model.logL_segments, key=('enum', label))
    within_time(('enum', label))
    assert got.n_profiles == len(seg_start) == want['n_profiles'] and got.n_nan == 0 == want['n_nan']
    if tables:
        W, F = WC.fast_tables(model, x)
        worst = float(np.max(np.abs(logL - C.table_logl(W, F, seg_start, seg_state, T))))
        print(f"{label}: max |logL_segments - table_logl| = {worst:.3e}")
        assert worst < 1e-10
    fin = np.isfinite(want['log_post'])
    lp, wp = got.log_marginal_posterior[fin], want['log_post'][fin]
    normal = wp > -600
    err = np.abs(lp - wp)
    print(f"{label}: {got.n_profiles} profiles, logev {abs(got.logev - want['logev']) / abs(want['logev']):.2e} relative, "
          f"KL {abs(got.KL - want['KL']) / max(1.0, abs(want['KL'])):.2e}, marginals {np.max(err[normal], initial=0.0):.2e}")
    assert abs(got.logev - want['logev']) <= 1e-11 * abs(want['logev'])
    assert abs(got.KL - want['KL']) <= 1e-11 * max(1.0, abs(want['KL']))
    j = want['map_index']
    assert got.map_logL == want['map_logL']
    assert np.array_equal(got.map_profile[:], X.states_from_segments(seg_start[j:j + 1], seg_state[j:j + 1], T)[0])
    assert got.log_marginal_posterior.shape == (S, T) and np.array_equal(fin, np.isfinite(got.log_marginal_posterior))
    assert not np.any(np.isnan(got.log_marginal_posterior))
    assert np.max(err[normal], initial=0.0) < 1e-11, (np.argmax(err[normal]), np.max(err[normal]))
    assert np.all(err[~normal] < 0.1)


def check_empty(e, S, T):
    assert e.n_profiles == 0 and e.logev == -np.inf and np.isnan(e.KL) and e.map_profile is None and np.isnan(e.map_logL)
    assert e.n_nan == 0 and e.log_marginal_posterior.shape == (S, T) and np.all(np.isnan(e.log_marginal_posterior))


@pytest.mark.parametrize('name', list(WC.ENUM_CASES))
def test_enumeration_against_oracle(name):
    """
    The long cases launch `exact_reduce_kernel` with 10 240 B of static LDS and, at T = 1800 and 2048, 63 744 B and 71 680 B
    of dynamic LDS on top: above 64 KiB in sum at T = 1800 without the attribute being raised, above it alone at T = 2048.
    """
    S, T, trans, k, marg, T2 = WC.ENUM_CASES[name]
    model, x, other, _ = WC.enum_case(name)
    got = bild_amd.exact_evidence(x, model, k)
    if name == 's1_T20_k1':
        check_empty(got, S, T)
        assert X.enumerate_profiles(T, k, model.transitions)[0].shape == (0, 2)
    else:
        check_enumeration(name, got, model, x, k, tables=T <= 40)
    if other is None:
        same_evidence(got, bild_amd.exact_evidence(x, model, k))       # a second call: bit for bit
        return
    # the trajectory and a shorter companion in one call of one block per chunk: each bit for bit what it is alone
    # (a call has one model and one k, so the batch is the case's own)
    batch = bild_amd.exact_evidence([x, other], model, k, scratch_bytes=1)
    same_evidence(batch[0], got)
    same_evidence(batch[1], bild_amd.exact_evidence(other, model, k))
    if T2 - 1 < k or S == 1 and k:
        check_empty(batch[1], S, T2)


def test_enumeration_refusals():
    """ host-side checks that answer before any launch: k = 16, and marginals of S T = 8195 > 8192 """
    model, x, _, _ = WC.enum_case('s2_T17_k15')
    with pytest.raises(ValueError, match='0 <= k <= 15'):
        bild_amd.exact_evidence(x, model, 16)
    with pytest.raises(_lib.BildAmdError, match='0 <= k <= 15') as e:
        _lib.exact_evidence(model.handle(), model.trajset(x), 16, model.transitions, gauss=True)
    assert e.value.code == _lib.ERR_UNSUPPORTED
    model, x = WC.make(5, 1639, (), 'full', seed=9000 * 5 + 1639, d=1)     # (one dimension: the set's table build is the test's time)
    with pytest.raises(ValueError, match='exceed the 8192'):
        bild_amd.exact_evidence(x, model, 1)
    with pytest.raises(_lib.BildAmdError, match='exceed the 8192') as e:
        _lib.exact_evidence(model.handle(), model.trajset(x), 1, model.transitions, gauss=True)
    assert e.value.code == _lib.ERR_UNSUPPORTED
    # the set is still usable after the refusal: without marginals the trajectory runs
    bare = bild_amd.exact_evidence(x, model, 1, marginals=False)
    assert bare.n_profiles == 20 * 1638 and np.isfinite(bare.logev) and bare.log_marginal_posterior is None


@pytest.mark.parametrize('kind', ['rouse', 'gauss'])
def test_enumeration_entry_points_k5(kind):
    """ S = 3 without 0 -> 2, k = 5, T = 14: C(13, 5) = 1287 combinations a trace, through both entry points """
    rng = np.random.default_rng(514)
    if kind == 'rouse':
        model = rouse_model(3)
        x = rouse_traj(model, 14, rng)
    else:
        model, x = WC.make(3, 14, (), 'no02')
    got = bild_amd.exact_evidence(x, model, 5)
    assert got.n_profiles == 1287 * int(CFC(model.transitions).N_total(5))
    check_enumeration(f"{kind} S = 3 k = 5", got, model, x, 5, tables=kind == 'gauss')
