"""
The five device-side consumers of csrc/philox.h against the host statement of their streams, tests/philox_oracle.py: the
counter layouts that include/bild_amd.h documents are a contract -- a draw is a pure function of (seed, index, frame, ...)
-- and this file holds each kernel to it draw by draw.  The statistical tests of the neighbouring files stay the check of the
law; this is the check of the stream.  Cases: tests/device_stream_cases.py; their conditions: tests/test_philox_oracle.py;
what the MI355X gave: tests/README_device_streams.md.  `-s` prints every figure.

Uniforms are exact (53 bits), so they are compared bit for bit.  The normals go through the device's log, sqrt and
sincospi, so the generators are compared through replay mode, which the tests of test_gpu_simulate.py and
test_gpu_gauss_simulate.py hold to the CPU loops: the device mode against the replay of the oracle's normals, under the
replay tests' own bar of 1e-9 max |data| per trajectory.  The mutation checks replay what the contract rules out -- ordinary
replay calls -- and must miss the device mode by 1e-3 max |data| in some trajectory: they show that the bar can fail.
"""
import time

import numpy as np
import pytest

import bild_amd
import device_stream_cases as DS
import philox_oracle as PO
from bild_amd import _lib

pytestmark = pytest.mark.gpu

BAR = 1e-9
MUTATION = 1e-3


def deviations(got, want, T):
    """ per trajectory max |got - want| / max |want| over the frames that are not NaN; the NaN patterns must be equal """
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    offs = np.concatenate([[0], np.cumsum(T)])
    out = np.zeros(len(T))
    for i in range(len(T)):
        g, w = got[offs[i]:offs[i + 1]], want[offs[i]:offs[i + 1]]
        ok = ~np.isnan(w)
        if ok.any():
            out[i] = np.max(np.abs(g[ok] - w[ok])) / np.max(np.abs(w[ok]))
    return out


# ---------------------------------------------------------------- profile draws: uniforms bit for bit

def consumed(uniforms, count):
    """ the first count[r] entries of row r, 0 behind them """
    used = np.arange(uniforms.shape[1])[None, :] < np.asarray(count)[:, None]
    return np.where(used, uniforms, 0.0)


@pytest.mark.parametrize('S,seed', DS.DRAW_CASES)
def test_exact_draws_take_the_documented_uniforms(S, seed):
    model, xs, _ = DS.draw_case(S)
    n, ks, U = DS.N_DRAWS, DS.draw_ks(), 2 * DS.DRAW_K_MAX
    res = bild_amd.exact_sample(xs, model, k_max=DS.DRAW_K_MAX, marginals=False)
    dev = bild_amd.exact_draw(res, n, k=ks, seed=seed)
    want = PO.segdraw_uniforms(seed, np.arange(3 * n), U).reshape(3, n, U)      # draw i of result j is stream j n + i
    for j, d in enumerate(dev):
        assert np.all(d.seg_start[:, 0] == 0) and not np.any(np.isnan(d.logL))
        assert np.array_equal(d.uniforms, consumed(want[j], np.maximum(1, 2 * ks[j])))
    assert len(np.unique(want)) == want.size
    # the oracle's uniforms replayed: the same draws bit for bit
    for a, b in zip(dev, bild_amd.exact_draw(res, n, k=ks, uniforms=want)):
        for name in ('k', 'seg_start', 'seg_state', 'logL', 'uniforms'):
            assert np.array_equal(getattr(a, name), getattr(b, name)), name
    # a trajectory of the set alone, one draw fewer (four draws a workgroup: the last one partial): streams 0 ... n - 2
    alone = bild_amd.exact_draw(res[2], n - 1, k=ks[2][:-1], seed=seed)
    assert np.array_equal(alone.uniforms, consumed(want[0][:-1], np.maximum(1, 2 * ks[2][:-1])))


@pytest.mark.parametrize('S,seed', DS.DRAW_CASES)
def test_dwell_draws_take_the_documented_uniforms(S, seed):
    model, xs, prior = DS.draw_case(S)
    n, U = DS.N_DRAWS, 2 * max(DS.DRAW_LENGTHS) - 1
    res = bild_amd.exact_dwell(xs, model, prior, marginals=False)
    dev = bild_amd.exact_dwell_draw(res, n, seed=seed, keep_uniforms=U)
    want = PO.dwelldraw_uniforms(seed, np.arange(3 * n), U).reshape(3, n, U)
    for j, d in enumerate(dev):
        assert np.all(d.n_switches >= 0) and np.array_equal(d.n_uniforms, 1 + 2 * d.n_switches)
        assert np.array_equal(d.uniforms, consumed(want[j], d.n_uniforms))
    assert max(d.n_switches.max() for d in dev) > 1       # more than two blocks of a stream are read
    for a, b in zip(dev, bild_amd.exact_dwell_draw(res, n, uniforms=want)):
        for name in ('n_switches', 'logL', 'log_prior', 'n_uniforms', 'uniforms'):
            assert np.array_equal(getattr(a, name), getattr(b, name)), name
        assert np.array_equal(a.states(), b.states())
    # a trajectory of the set alone, one draw fewer (four draws a workgroup: the last one partial): streams 0 ... n - 2
    alone = res[2].draw(n - 1, seed=seed, keep_uniforms=U)
    assert np.array_equal(alone.uniforms, consumed(want[0][:-1], alone.n_uniforms))
    # explicit stream indices through the C call, beyond 32 bits, each on all three trajectories
    streams = np.repeat(np.array(DS.DWELL_STREAMS, dtype=np.int64), 3)
    trajs = np.tile(np.arange(3), len(DS.DWELL_STREAMS))
    raw = _lib.gauss_dwell_draw(model.handle(), model.trajset(xs), prior.log_init, prior.log_jump, prior.log_dwell, prior.log_surv,
                                trajs, draw_stream=streams, keep_uniforms=U, seed=seed)
    assert np.all(raw['n_uniforms'] >= 1)
    assert np.array_equal(raw['uniforms'], consumed(PO.dwelldraw_uniforms(seed, streams, U), raw['n_uniforms']))
    for a in range(0, len(streams), 3):     # equal stream index on different trajectories: equal uniforms, as far as both read
        for b in (a + 1, a + 2):
            m = min(raw['n_uniforms'][a], raw['n_uniforms'][b])
            assert np.array_equal(raw['uniforms'][a, :m], raw['uniforms'][b, :m])
    assert raw['n_uniforms'].max() > 1
    # stream index r below 2^32 is draw r without indices
    assert np.array_equal(raw['uniforms'][:3], consumed(want[0][:1].repeat(3, axis=0), raw['n_uniforms'][:3]))


# ---------------------------------------------------------------- the Rouse generator

ROUSE_MUTATIONS = {
    'cosine and sine exchanged': lambda seed: dict(seed=seed, swap=True),
    'trajectory index off by one': lambda seed: dict(seed=seed, shift=1),
    'stream 8 j + k': lambda seed: dict(seed=seed, mode_stride=8),
    'seed halves exchanged': lambda seed: dict(seed=DS.swap_halves(seed)),
    'noise without the 2^31 offset': lambda seed: dict(seed=seed, noise_base=0),
}


@pytest.mark.parametrize('N,d,seed', DS.ROUSE_CASES)
def test_rouse_device_mode_is_the_replay_of_the_oracle(N, d, seed):
    arrays, w = DS.rouse_inputs(N, d)
    assert DS.rouse_condition(arrays, w) > DS.CONDITION
    T, seg_start, seg_state, missing, loc_err = DS.rouse_call(N, d)

    def run(T, seg_start, seg_state, missing, loc_err, **kw):
        return _lib.rouse_simulate(*arrays, w, T, seg_start, seg_state, missing, loc_err, **kw)

    dev = run(T, seg_start, seg_state, missing, loc_err, seed=seed)
    assert np.array_equal(np.isnan(dev[:, 0]), missing) and np.all(np.isfinite(dev[~missing]))
    t0 = time.perf_counter()
    z = DS.rouse_oracle(N, d, seed)
    took = time.perf_counter() - t0
    dev_rel = deviations(dev, run(T, seg_start, seg_state, missing, loc_err, normals=z), T)
    print(f"rouse N={N} d={d} seed={seed:#x}: worst |device - replay of the oracle| / max|data| = {dev_rel.max():.2e} "
          f"(oracle {took:.2f} s)")
    assert dev_rel.max() <= BAR
    for name, kw in ROUSE_MUTATIONS.items():
        if N == 1 and name == 'stream 8 j + k':
            continue        # mode 0 is stream k under either stride: nothing differs at N = 1
        kw = kw(seed)
        rel = deviations(dev, run(T, seg_start, seg_state, missing, loc_err, normals=DS.rouse_oracle(N, d, kw.pop('seed'), **kw)), T)
        print(f"    {name}: largest deviation {rel.max():.2e}")
        assert rel.max() > MUTATION, name

    # the index of a trajectory is its index in the call: a call on the trajectories from ROUSE_SUB on, under 2^64 - 1, and
    # its replay uploaded a trajectory at a time
    first, seed2 = DS.ROUSE_SUB, DS.SEEDS[3]
    sub = DS.rouse_call(N, d, first=first)
    budget = int(np.max(sub[0])) * (N + 1) * d * 8
    dev2 = run(*sub, seed=seed2, scratch_bytes=budget)
    assert np.array_equal(dev2, run(*sub, seed=seed2), equal_nan=True)
    rel2 = deviations(dev2, run(*sub, normals=DS.rouse_oracle(N, d, seed2, first=first), scratch_bytes=budget), sub[0])
    off = deviations(dev2, run(*sub, normals=DS.rouse_oracle(N, d, seed2, first=first, shift=first)), sub[0])
    print(f"    sub-batch from trajectory {first}: worst {rel2.max():.2e}; indexed by the position in the whole call instead {off.max():.2e}")
    assert rel2.max() <= BAR and off.max() > MUTATION


# ---------------------------------------------------------------- the GenericGaussianModel generator

@pytest.mark.parametrize('model_seed,seed', DS.GAUSS_CASES)
def test_gauss_device_mode_is_the_replay_of_the_oracle(model_seed, seed):
    model = DS.gauss_model(model_seed)
    T, seg_start, seg_state, missing = DS.gauss_call()
    h = model.handle()
    dev = _lib.gauss_simulate(h, T, seg_start, seg_state, missing, seed=seed)
    assert np.array_equal(np.isnan(dev[:, 0]), missing) and np.all(np.isfinite(dev[~missing]))
    # chunks of the normals: bit for bit the same
    assert np.array_equal(dev, _lib.gauss_simulate(h, T, seg_start, seg_state, missing, seed=seed, scratch_bytes=DS.GAUSS_SCRATCH),
                          equal_nan=True)
    t0 = time.perf_counter()
    z = DS.gauss_oracle(model, seed)
    took = time.perf_counter() - t0
    rel = deviations(dev, _lib.gauss_simulate(h, T, seg_start, seg_state, missing, normals=z), T)
    print(f"gauss model {model_seed} seed={seed:#x}: worst |device - replay of the oracle| / max|data| = {rel.max():.2e} (oracle {took:.2f} s)")
    assert rel.max() <= BAR
    small = deviations(dev, _lib.gauss_simulate(h, T, seg_start, seg_state, missing, normals=z, scratch_bytes=DS.GAUSS_SCRATCH), T)
    assert small.max() <= BAR
    for name, kw in (('cosine and sine exchanged', dict(seed=seed, swap=True)), ('trajectory index off by one', dict(seed=seed, shift=1)),
                     ('seed halves exchanged', dict(seed=DS.swap_halves(seed)))):
        mut = deviations(dev, _lib.gauss_simulate(h, T, seg_start, seg_state, missing, normals=DS.gauss_oracle(model, **kw)), T)
        print(f"    {name}: largest deviation {mut.max():.2e}")
        assert mut.max() > MUTATION, name


# ---------------------------------------------------------------- the AMIS draws

def amis_compare(label, got, want):
    ss, thetas = got
    want_ss, want_thetas, _, fragile = want
    firm = ~fragile
    assert fragile.sum() <= DS.FRAGILE_CAP * len(fragile)
    assert ss.shape == want_ss.shape and thetas.shape == want_thetas.shape
    worst = float(np.max(np.abs(ss[firm] - want_ss[firm])))
    print(f"{label}: fragile {int(fragile.sum())} of {len(fragile)}, worst |ss - oracle| = {worst:.2e}, "
          f"traces that differ {int(np.any(thetas[firm] != want_thetas[firm], axis=1).sum())}")
    assert np.array_equal(thetas[firm], want_thetas[firm])
    assert worst <= 1e-12


def amis_step(core, model, traj, seed):
    """ a step whose samples are drawn on the device; -> whether the fit of the next proposal converged (the samples are pooled either way) """
    try:
        core.step_device_rng(model.handle(), model.trajset(traj), DS.AMIS_N, seed)
        return True
    except RuntimeError as e:       # (the fit of a proposal to corner samples need not converge: not this file's business)
        print(f"    the step's fit: {e}")
        return False


@pytest.mark.parametrize('name', list(DS.AMIS_CASES))
def test_amis_draws_are_the_oracle_s(built_lib, name):
    trans, a0, logp0, seed = DS.amis_case(name)
    model, traj = DS.amis_target(trans.shape[0])
    core = _lib.AmisCore(trans, a0, logp0, 1e-2, 1e-3, 0.0)
    core.use_device(True)
    converged = amis_step(core, model, traj, seed)
    assert len(core) == DS.AMIS_N
    ss, thetas = core.pool_samples()
    amis_compare(name, (ss, thetas), DS.amis_oracle(name))
    if name != 'regimes_s2':
        return
    # the same seed under k1 one larger is another stream (the case k1_5_s2 holds that core to the oracle)
    other = DS.amis_oracle('k1_5_s2')
    assert not np.any(other[0][:, 0] == ss[:, 0])
    # a second step: the pool index goes on at N, the proposal is the fitted one
    assert converged
    a1, logp1 = core.params(-1)
    assert not np.array_equal(a1, a0)
    assert amis_step(core, model, traj, seed) or len(core) == 2 * DS.AMIS_N
    ss2, thetas2 = core.pool_samples()
    assert len(ss2) == 2 * DS.AMIS_N and np.array_equal(ss2[:DS.AMIS_N], ss) and np.array_equal(thetas2[:DS.AMIS_N], thetas)
    want = PO.amis_draw(seed, len(a0), DS.AMIS_N, DS.AMIS_N, a1, PO.amis_prob(logp1), trans)
    amis_compare(name + ', second step', (ss2[DS.AMIS_N:], thetas2[DS.AMIS_N:]), want)
    # ... and not the streams of the first step again
    again = PO.amis_draw(seed, len(a0), 0, 50, a1, PO.amis_prob(logp1), trans)
    assert not np.any(np.all(again[0] == ss2[DS.AMIS_N:DS.AMIS_N + 50], axis=1))
