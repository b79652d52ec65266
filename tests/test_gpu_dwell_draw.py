"""
The draws under a dwell-time prior on the GPU (bild_amd.exact.exact_dwell_draw, csrc/gauss_dwelldraw.hip, DESIGN.md section
22): replay against the NumPy oracle tests/dwell_draw_oracle.py draw for draw around the 64-lane scan, at one to four states, beyond
256 frames and under non-geometric and bounded priors, six trajectories in one call, device mode as replay
of its own uniforms, bit-identity across call shapes, the distribution against the enumeration and against `exact_dwell`'s
marginals, T = 1000, `posterior_distance`, and the refusals of the C call.

The count bound of the distribution tests is that of tests/test_segment_draw.py: |count - N p| <= 5.5 sqrt(N p (1 - p)) + 3 per
comparison.  `-s` prints the largest ratio of every case.
"""
import ctypes

import numpy as np
import pytest

import bild_amd
import dwell_cases as DC
import dwell_draw_cases as DDC
import dwell_draw_oracle as DDO
import segment_cases as C
from bild_amd import _lib
from bild_amd.profiles import segments_from_states
from test_dwell import build
from test_dwell_draw import ENUM_CASES, profile_counts
from test_segment_draw import check_counts

pytestmark = pytest.mark.gpu


def log_prob(prior, states):
    return np.array([prior.log_prob(row) for row in states])


def logl_segments(model, x, d):
    seg_start, seg_state = d.segments()
    return model.logL_segments(seg_start, seg_state, [x] if np.ndim(x) == 2 else x)


@pytest.mark.parametrize('name', list(DDC.REPLAY_CASES))
def test_replay_against_oracle(name):
    model, x, prior, u = DDC.replay_case(name)
    want = DDC.oracle_replay(name)
    fragile, n = want['fragile'], DDC.n_replay(name)
    assert len(u) == n == len(fragile)
    # the excused share: a condition on the inputs (tests/test_dwell_draw.py asserts that it is 0 for these seeds)
    assert fragile.sum() <= 0.001 * n
    if 'order0' in name:
        r = bild_amd.exact_dwell(x, model, prior)
        assert r.n_nan_windows > 0 and np.isnan(r.log_evidence)
        with pytest.raises(ValueError, match="nan='omit'"):
            r.draw(n, uniforms=u)
        r = bild_amd.exact_dwell(x, model, prior, nan='omit')
        assert r.n_nan_windows > 0
    else:
        r = bild_amd.exact_dwell(x, model, prior)
    d = r.draw(n, uniforms=u)
    firm = ~fragile
    states = d.states()
    assert states.shape == (n, len(x)) and d.T == len(x) and len(d) == n
    assert np.array_equal(states[firm], want['states'][firm])
    assert np.array_equal(d.n_switches[firm], want['n_switches'][firm]) and np.array_equal(d.n_uniforms[firm], want['n_uniforms'][firm])
    assert np.array_equal(d.n_uniforms, 1 + 2 * d.n_switches)
    assert np.array_equal(np.count_nonzero(np.diff(states, axis=1), axis=1), d.n_switches)
    used = np.arange(u.shape[1])[None, :] < d.n_uniforms[:, None]
    assert np.array_equal(d.uniforms, np.where(used, u, 0.0))
    logL = logl_segments(model, x, d)
    lp = log_prob(prior, states)
    assert not np.any(np.isnan(d.logL)) and np.all(np.isfinite(d.log_prior))
    print(f"{name}: fragile {int(fragile.sum())}, switches {d.n_switches.min()} ... {d.n_switches.max()}, max |logL - logL_segments| = "
          f"{np.max(np.abs(d.logL - logL)):.3e}, max |log_prior - log_prob| = {np.max(np.abs(d.log_prior - lp)):.3e}")
    assert np.max(np.abs(d.logL - logL)) < 1e-10
    assert np.max(np.abs(d.log_prior - lp)) < 1e-10


def same_draws(a, b):
    assert a.T == b.T
    for name in ('n_switches', 'logL', 'log_prior', 'n_uniforms', 'uniforms'):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    assert np.array_equal(a.states(), b.states())


def test_six_trajectories_in_one_call():
    """ more than four trajectories: `dwelldraw_head_kernel`'s second workgroup, on a ragged set of four states """
    model, prior, xs, tabs = DC.ragged_case()
    n, u = DDC.N_SIX, DDC.six_uniforms()
    res = bild_amd.exact_dwell(xs, model, prior, marginals=False)
    together = bild_amd.exact_dwell_draw(res, n, uniforms=u)
    assert [d.T for d in together] == [T for T, _ in DC.RAGGED]
    for j, d in enumerate(together):    # a trajectory alone, on a set of its own
        same_draws(d, bild_amd.exact_dwell(xs[j], model, prior, marginals=False).draw(n, uniforms=u[j]))
        assert np.array_equal(d.n_uniforms, 1 + 2 * d.n_switches) and np.max(np.abs(d.logL - logl_segments(model, xs[j], d))) < 1e-10
    for j in (1, 5):
        want = DDC.oracle_six(j)
        firm = ~want['fragile']
        print(f"trajectory {j}: fragile {int(want['fragile'].sum())}, switches {together[j].n_switches.min()} ... {together[j].n_switches.max()}")
        assert want['fragile'].sum() <= 1
        assert np.array_equal(together[j].states()[firm], want['states'][firm])
        assert np.array_equal(together[j].n_switches[firm], want['n_switches'][firm])


def test_device_mode_is_replay_of_its_own_uniforms():
    model, x, prior, _ = DDC.replay_case('s3_T65_minlength')
    T, n = len(x), DDC.N_REPLAY
    r = bild_amd.exact_dwell(x, model, prior)
    d = r.draw(n, seed=7, keep_uniforms=2 * T - 1)
    assert np.array_equal(d.n_uniforms, 1 + 2 * d.n_switches) and d.uniforms.shape == (n, 2 * T - 1)
    used = np.arange(2 * T - 1)[None, :] < d.n_uniforms[:, None]
    assert np.all((d.uniforms >= 0) & (d.uniforms < 1)) and np.all(d.uniforms[~used] == 0)
    assert np.all(d.uniforms[used] > 0) and len(np.unique(d.uniforms[used])) == used.sum()      # (53 random bits each)
    assert abs(np.mean(d.uniforms[used]) - 0.5) < 5 / np.sqrt(12 * used.sum())
    same_draws(d, r.draw(n, uniforms=d.uniforms))
    same_draws(d, r.draw(n, seed=7, keep_uniforms=2 * T - 1))
    # fewer uniforms kept, or none: the same draws
    few = r.draw(n, seed=7, keep_uniforms=3)
    assert np.array_equal(few.uniforms, d.uniforms[:, :3]) and np.array_equal(few.states(), d.states())
    none = r.draw(n, seed=7)
    assert none.uniforms is None and np.array_equal(none.states(), d.states()) and np.array_equal(none.logL, d.logL)
    other = r.draw(n, seed=8, keep_uniforms=2 * T - 1)
    assert not np.array_equal(other.uniforms, d.uniforms) and not np.array_equal(other.states(), d.states())
    # the same consumed uniforms through the oracle
    W, F = C.tables(model, x)
    want = DDO.draws(W, F, prior, d.uniforms[:1024])
    firm = ~want['fragile']
    assert want['fragile'].sum() <= 1
    assert np.array_equal(d.states()[:1024][firm], want['states'][firm])
    # a replay row that is too short: refused with the draw and the width that always does
    k = d.n_switches
    assert k.max() > 1
    with pytest.raises(ValueError, match=f"draw {int(np.flatnonzero(1 + 2 * k > 3)[0])} needs more than the 3 uniforms.*{2 * T - 1}"):
        r.draw(n, uniforms=d.uniforms[:, :3])


def test_bit_identity_across_call_shapes():
    rng = np.random.default_rng(41)
    model = C.random_model(rng, 2, 200)
    xs = [C.random_traj(rng, T, missing) for T, missing in ((40, ()), (65, (9,)), (193, (63, 65)), (65, ()))]
    prior = DC.make_prior('markov', rng, 2, 193)
    n = 300
    u = rng.random((len(xs), n, 2 * 193 - 1))
    res = bild_amd.exact_dwell(xs, model, prior, marginals=False)
    first = bild_amd.exact_dwell_draw(res, n, uniforms=u)
    assert isinstance(first, list) and [d.T for d in first] == [40, 65, 193, 65]
    for j, d in enumerate(first):
        assert np.all(d.n_switches >= 0) and np.max(np.abs(d.logL - logl_segments(model, xs[j], d))) < 1e-10
    for a, b in zip(first, bild_amd.exact_dwell_draw(res, n, uniforms=u)):      # a repeated call
        same_draws(a, b)
    for j in range(len(xs)):    # a trajectory alone, on a set of its own
        same_draws(first[j], bild_amd.exact_dwell(xs[j], model, prior, marginals=False).draw(n, uniforms=u[j]))
    order = [2, 0, 3, 1]
    permuted = bild_amd.exact_dwell([xs[j] for j in order], model, prior, marginals=False)
    for j, b in zip(order, bild_amd.exact_dwell_draw(permuted, n, uniforms=u[order])):
        same_draws(first[j], b)
    per_traj = 16 * 2 * 194 + 16
    for scratch in (1, 2 * per_traj):       # one trajectory a chunk, and two
        for a, b in zip(first, bild_amd.exact_dwell_draw(res, n, uniforms=u, scratch_bytes=scratch)):
            same_draws(a, b)
    # draws on some of the set's trajectories only: the others are skipped
    ts = model.trajset(xs)
    part = _lib.gauss_dwell_draw(model.handle(), ts, prior.log_init, prior.log_jump, prior.log_dwell, prior.log_surv, np.full(n, 1),
                                 uniforms=u[1])
    assert np.array_equal(part['states'][:, :65], first[1].states()) and np.all(part['states'][:, 65:] == 255)
    assert np.array_equal(part['logl'], first[1].logL)
    # device mode: draw i of result j is stream j n + i, whatever the chunks and the call's other draws
    dev = bild_amd.exact_dwell_draw(res, n, seed=5, keep_uniforms=7)
    for a, b in zip(dev, bild_amd.exact_dwell_draw(res, n, seed=5, keep_uniforms=7, scratch_bytes=1)):
        same_draws(a, b)
    alone = _lib.gauss_dwell_draw(model.handle(), ts, prior.log_init, prior.log_jump, prior.log_dwell, prior.log_surv, np.full(n, 2),
                                  draw_stream=2 * n + np.arange(n), keep_uniforms=7, seed=5)
    assert np.array_equal(alone['states'], dev[2].states()) and np.array_equal(alone['uniforms'], dev[2].uniforms)


@pytest.mark.parametrize('name,kind,nan', ENUM_CASES)
def test_distribution_against_enumeration(name, kind, nan):
    model, x, prior = build(name, kind)
    W, F = C.tables(model, x)
    N = 200000
    states, joint, p, bad = DDO.profile_posterior(W, F, prior)
    r = bild_amd.exact_dwell(x, model, prior, nan=nan, marginals=False)
    d = r.draw(N, seed=sum(map(ord, name + kind)))
    assert np.all(d.n_switches >= 0)
    counts = profile_counts(states, d.states())
    assert np.all(counts[bad] == 0) and np.all(counts[joint == -np.inf] == 0)       # a NaN profile is never drawn
    worst = check_counts(counts, p, N)
    k = np.count_nonzero(np.diff(states, axis=1), axis=1)
    p_k = np.bincount(k, weights=p, minlength=len(x))
    worst_k = check_counts(np.bincount(d.n_switches, minlength=len(x)), p_k, N)
    print(f"{name} {kind}: largest |count - N p| / bound = {worst:.3f} (profiles), {worst_k:.3f} (k)")


def check_marginals(d, log_post, N):
    """ the draws' state counts per frame against exp(log_post) (S, T) """
    states = d.states()
    assert len(states) == N
    counts = np.array([np.sum(states == s, axis=0) for s in range(log_post.shape[0])])
    with np.errstate(under='ignore'):
        p = np.exp(log_post)
    excess = np.abs(counts - N * p) - (5.5 * np.sqrt(N * p * (1 - p)) + 3)
    assert np.all(excess <= 0), (np.unravel_index(np.argmax(excess), excess.shape), float(np.max(excess)))
    return float(np.max(np.abs(counts - N * p) / (5.5 * np.sqrt(N * p * (1 - p)) + 3)))


def test_distribution_against_marginals_T200():
    T, N = 200, 20000
    rng = np.random.default_rng(200)
    model = C.random_model(rng, 2, T + 8)
    x = C.random_traj(rng, T, (50,))
    prior = DC.make_prior('markov', rng, 2, T)
    r = bild_amd.exact_dwell(x, model, prior)
    d = r.draw(N, seed=17)
    worst = check_marginals(d, r.log_marginal_posterior, N)
    print(f"T = 200: largest |count - N p| / bound = {worst:.3f}")


def test_T1000():
    T, N = 1000, 10000
    rng = np.random.default_rng(31)
    model = C.random_model(rng, 2, T + 8, orders=np.ones((2, 3), dtype=int), d=3)
    x = C.random_traj(rng, T, (100, 500, 501), d=3)
    prior = bild_amd.DwellPrior.markov([[0.98, 0.02], [0.05, 0.95]], [0.5, 0.5], n=T)
    r = bild_amd.exact_dwell(x, model, prior)
    d = r.draw(N, seed=3)
    states = d.states()
    assert np.all(d.n_switches >= 0) and np.array_equal(np.count_nonzero(np.diff(states, axis=1), axis=1), d.n_switches)
    assert np.array_equal(d.n_uniforms, 1 + 2 * d.n_switches)
    # the walk's left-to-right order of addition: bit for bit
    assert np.array_equal(d.logL, logl_segments(model, x, d))
    lp = log_prob(prior, states)
    print(f"T = 1000: switches {d.n_switches.min()} ... {d.n_switches.max()}, max |log_prior - log_prob| = {np.max(np.abs(d.log_prior - lp)):.3e}, "
          f"largest log joint - MAP = {np.max(d.logL + d.log_prior) - r.map_log_joint:.3f}")
    assert np.max(np.abs(d.log_prior - lp)) < 1e-10
    assert np.all(d.logL + d.log_prior <= r.map_log_joint + 1e-9)
    assert len(np.unique(states, axis=0)) > N // 2
    worst = check_marginals(d, r.log_marginal_posterior, N)
    print(f"T = 1000: largest |count - N p| / bound = {worst:.3f}")


def test_posterior_distance():
    model, x, prior, _ = DDC.replay_case('s2_T70_order0_gap')
    x = x.copy()
    x[40] = np.nan
    r = bild_amd.exact_dwell(x, model, prior, nan='omit')
    mean, var = r.posterior_distance(n=500, seed=3)
    d = r.draw(500, seed=3)
    seg_start, seg_state = segments_from_states(d.states())
    want_mean, want_var = model.kalman_mixture((seg_start, seg_state), [x], np.zeros(500))
    assert mean.shape == var.shape == x.shape
    assert np.array_equal(mean, want_mean[0]) and np.array_equal(var, want_var[0])
    valid = ~np.isnan(x)
    assert np.array_equal(mean[valid], x[valid]) and np.all(var[valid] == 0)
    assert np.all(np.isfinite(mean)) and np.all(var[~valid] > 0)


def test_c_level_refusals():
    rng = np.random.default_rng(51)
    model = C.random_model(rng, 2, 40)
    x = C.random_traj(rng, 30)
    ts = model.trajset([x, x[:20]])
    h = model.handle()
    p = DC.symmetric_chain(0.1, 30)
    good = [p.log_init, p.log_jump, p.log_dwell, p.log_surv]
    n = 64
    tj, u = np.arange(n) % 2, rng.random((n, 59))

    def refused(match, code=_lib.ERR_INVALID, tables=good, draw_traj=tj, uniforms=u, scratch_bytes=0):
        with pytest.raises(_lib.BildAmdError, match=match) as e:
            _lib.gauss_dwell_draw(h, ts, *tables, draw_traj, uniforms=uniforms, scratch_bytes=scratch_bytes)
        assert e.value.code == code

    for bad in (2, -1):
        refused('draw_traj', draw_traj=np.where(np.arange(n) == 5, bad, tj))
    for bad in (1.0, np.nan, -0.25):
        v = u.copy()
        v[6, 4] = bad
        refused('uniforms', uniforms=v)
    refused('scratch_bytes', scratch_bytes=-1)
    # what bild_gauss_dwell_evidence refuses
    for i in range(4):
        for where, value in (((0,) * good[i].ndim, np.nan), ((-1,) * good[i].ndim, np.inf)):
            tables = [a.copy() for a in good]
            tables[i][where] = value
            refused('finite or -inf', tables=tables)
    tables = [a.copy() for a in good]
    tables[1][1, 1] = 0.0
    refused('diagonal', tables=tables)
    refused('log_init', tables=[np.full(2, -np.inf)] + good[1:])
    refused('lengths', tables=[good[0], good[1], good[2][:, :29], good[3][:, :29]])
    five = C.random_model(rng, 5, 40)
    p5 = DC.make_prior('markov', rng, 5, 30)
    with pytest.raises(_lib.BildAmdError, match='at most 4') as e:
        _lib.gauss_dwell_draw(five.handle(), five.trajset(x), p5.log_init, p5.log_jump, p5.log_dwell, p5.log_surv, np.zeros(4, dtype=int))
    assert e.value.code == _lib.ERR_UNSUPPORTED

    arrs = [_lib.f64(a) for a in good]
    lib = _lib.lib()

    def raw(T_max=30, scratch=0, n_draws=0, draw_traj=None, U=0, uniforms=None, spec=None):
        spec = _lib.DwelldrawOut() if spec is None else spec
        return lib.bild_gauss_dwell_draw(h._h, ts._h, 30, *[_lib.dptr(a) for a in arrs], T_max, scratch, n_draws,
                                         None if draw_traj is None else _lib.aptr(draw_traj), None, U,
                                         None if uniforms is None else _lib.aptr(uniforms), 0, ctypes.byref(spec))
    assert raw() == _lib.OK         # n_draws = 0 returns at once
    assert raw(n_draws=-1) == _lib.ERR_INVALID and raw(T_max=29) == _lib.ERR_INVALID and raw(U=-1) == _lib.ERR_INVALID
    assert raw(scratch=-1) == _lib.ERR_INVALID
    t4, u0 = _lib.i32(np.zeros(4)), np.zeros((4, 1))
    assert raw(n_draws=4, draw_traj=t4, U=0, uniforms=u0) == _lib.ERR_INVALID       # a replay with U < 1
    assert raw(n_draws=4) == _lib.ERR_INVALID                                       # draw_traj is NULL
    assert raw(n_draws=4, draw_traj=t4) == _lib.OK                                  # every output NULL: nothing is written
    # the set is still usable, and one uniform a draw serves the draws without a switch
    res = _lib.gauss_dwell_draw(h, ts, *good, tj, uniforms=u)
    assert np.all(res['n_switches'] >= 0) and np.all(res['states'][tj == 1, 20:] == 255) and np.all(res['states'][tj == 0] < 2)
    res = _lib.gauss_dwell_draw(h, ts, *good, tj, uniforms=u[:, :1])
    done = res['n_uniforms'] == 1
    assert np.all(res['n_switches'][done] == 0) and np.all(res['n_uniforms'][~done] == -1) and np.all(res['states'][~done] == 255)
    assert np.all(np.isnan(res['logl'][~done])) and np.all(res['n_switches'][~done] == -1)
