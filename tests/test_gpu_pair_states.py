"""
The pair state table (csrc/common.h): a chain of close switches t1 < t2 < t3 ... starts at its THIRD
switch, from the state the candidate that built the pair entry (t1, g1 = t2 - t1) left behind every `stride`-th frame of the gap
t2 ... -- where that candidate provably ran every frame up to t3 (logl_body.h: begin_chain, conditions (a)-(c)).

Hand-placed chains of 3, 4 and 5 close switches: g1 in {1, 2, 3, 4, m1 - 1}, g2 = 1 ... 72 -- every stride remainder, and every
value around the three conditions, whose edges (the end of the covered gaps, m_pair - g1, m_ref + tail_margin; all below 72 for
these models) are MEASURED on a set without transient table: there a candidate of one switch runs exactly the m frames of its
table entry, one of two switches the m of its pair entry.  The default path must equal states=False, split=False and
BILD_NO_ONE_LAUNCH and the same rows inside a large random batch bit for bit, and the oracle to 1e-8; the frames counted on the
device must fall by what the skipped gaps hold for the chains the measured edges say qualify, and not at all for the others.
"""
import ctypes
import os

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

TOL = 1e-8
G2_MAX = 72
MARGIN = 8   # BILD_TAIL_MARGIN's default
STRIDE = 3   # BILD_PAIR_STATES_STRIDE's default


def _under(settings, fn):
    """ fn() with the environment switches `settings` (NAME or NAME=value) in force """
    from bild_amd import _lib
    pairs = [(item.split('=') + ['1'])[:2] for item in settings]
    before = {name: os.environ.get(name) for name, _ in pairs}  # (calls nest: a switch may be in force already)
    for name, value in pairs:
        os.environ[name] = value
    _lib.config_reload()
    try:
        return fn()
    finally:
        for name, value in before.items():
            if value is None:
                del os.environ[name]
            else:
                os.environ[name] = value
        _lib.config_reload()


def _fresh(data):
    """ a new trajectory object over the same data: a trajectory set, and tables, of its own """
    import bild_amd
    if isinstance(data, (list, tuple)):
        return [_fresh(d) for d in data]
    return bild_amd.Trajectory(data[:].copy(), localization_error=data.localization_error)


def _frames_per_task(model, ts, seg_start, seg_state):
    """ frames every task of the batch ran itself (bild_debug_frames_per_task), (n, d*) """
    import torch
    from bild_amd import _lib
    dev = torch.device('cuda', 0)
    n, K1 = seg_start.shape
    dstar = max(1, len(np.unique(np.atleast_1d(model.localization_error))))
    d_a, d_b = torch.from_numpy(seg_start.astype(np.int32)).to(dev), torch.from_numpy(seg_state.astype(np.int32)).to(dev)
    out = torch.empty(n, dtype=torch.float64, device=dev)
    frames = torch.full((n * dstar,), -1, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    _lib.logl_segments_device(model.handle(), ts, 1, K1, d_a.data_ptr(), d_b.data_ptr(), 0, out.data_ptr(), stream=stream)  # (tables)
    torch.cuda.synchronize()
    _lib.lib().bild_debug_frames_per_task(ctypes.c_void_p(frames.data_ptr()))
    try:
        _lib.logl_segments_device(model.handle(), ts, n, K1, d_a.data_ptr(), d_b.data_ptr(), 0, out.data_ptr(), stream=stream)
        torch.cuda.synchronize()
    finally:
        _lib.lib().bild_debug_frames_per_task(None)
    return frames.cpu().numpy().reshape(n, dstar)


def _frames_total(model, fn):
    from bild_amd import _lib
    h = model.handle()
    _lib.kernel_timing_read()
    _lib.kernel_timing_read_walk()
    _lib.frames_run_read(h)
    _lib.kernel_timing(True)
    try:
        got = fn()
    finally:
        _lib.kernel_timing(False)
    _lib.kernel_timing_read()
    _lib.kernel_timing_read_walk()
    return got, _lib.frames_run_read(h)


def measured_single(model, data, S, T):
    """ m[s, sn, t]: frames the transient of a switch s -> sn at frame t runs until it has converged (the transient table's m),
    measured on a set that has no transient table and no tails: every candidate runs its transient itself, look by look """
    rows = [(s, sn, t) for s in range(S) for sn in range(S) if sn != s for t in range(1, T)]
    a = np.zeros((len(rows), 2), dtype=np.int32)
    b = np.zeros((len(rows), 2), dtype=np.int32)
    for r, (s, sn, t) in enumerate(rows):
        a[r, 1], b[r, 0], b[r, 1] = t, s, sn
    fr = _under(['BILD_NO_TRANSIENTS', 'BILD_NO_TAIL'], lambda: _frames_per_task(model, model.trajset(_fresh(data)), a, b))[:, 0]
    m = np.zeros((S, S, T), dtype=np.int64)
    for r, (s, sn, t) in enumerate(rows):
        m[s, sn, t] = fr[r]
    return m


def measured_pairs(model, data, keys):
    """ m_pair[(s, sn, sm, t1, g1)]: likewise for two switches """
    keys = sorted(set(keys))
    a = np.zeros((len(keys), 3), dtype=np.int32)
    b = np.zeros((len(keys), 3), dtype=np.int32)
    for r, (s, sn, sm, t1, g1) in enumerate(keys):
        a[r, 1:], b[r] = (t1, t1 + g1), (s, sn, sm)
    fr = _under(['BILD_NO_TRANSIENTS', 'BILD_NO_TAIL'], lambda: _frames_per_task(model, model.trajset(_fresh(data)), a, b))[:, 0]
    return {k: int(fr[r]) for r, k in enumerate(keys)}


def next_state(rng, s, S):
    return int((s + 1 + rng.integers(S - 1)) % S)


def chains(rng, T, S, K1, t1s, g1s, tails):
    """ one row per (t1, g1, g2): switches at t1, t1 + g1, t1 + g1 + g2, then what `tails` says: () a chain of three, (g3,) of
    four, (g3, g4) of five.  Unused segments lie behind the trajectory (cleaned away).  Also the rows' (s, sn, sm, t1, g1, g2). """
    a, b, keys = [], [], []
    for t1 in t1s:
        for g1 in g1s:
            for g2 in range(1, G2_MAX + 1):
                for tail in tails:
                    starts = [0, t1, t1 + g1, t1 + g1 + g2]
                    for g in tail:
                        starts.append(starts[-1] + g)
                    if starts[-1] >= T or len(starts) > K1:
                        continue
                    starts += [T + 3 + i for i in range(K1 - len(starts))]
                    states = [int(rng.integers(S))]
                    for _ in range(K1 - 1):
                        states.append(next_state(rng, states[-1], S))
                    a.append(starts)
                    b.append(states)
                    keys.append((states[0], states[1], states[2], t1, g1, g2, len(tail)))
    return np.array(a, dtype=np.int32), np.array(b, dtype=np.int32), keys


def make(S=2, T=250, err=0.1, missing=None, seed=0):
    import bild_amd
    rng = np.random.default_rng(1000 + seed)
    model = bild_amd.MultiStateRouse(20, 1, 5, d=3, looppositions=H.LOOPS[S], localization_error=err)
    data = model.trajectory_from_loopingprofile(H.random_profile(rng, T, S, T // 5), missing_frames=missing, rng=rng)
    return rng, model, data


def sweep(rng, model, data, S, T, K1, m1, t1s, n_random=3000):
    """ the rows of the sweep and their results on a fresh set: the default path against every switch that must not matter """
    from bild_amd import _lib
    g1s = lambda t1: sorted({1, 2, 3, 4, max(1, int(m1[:, :, t1][m1[:, :, t1] > 0].min()) - 1)})
    parts = [chains(rng, T, S, K1, [t1], g1s(t1), [(), (5,), (30,), (4, 7)][:(3 if K1 < 6 else 4)]) for t1 in t1s]
    a = np.concatenate([p[0] for p in parts])
    b = np.concatenate([p[1] for p in parts])
    keys = [k for p in parts for k in p[2]]
    ts = model.trajset(_fresh(data))
    h = model.handle()
    got = _lib.logl_segments(h, ts, a, b)
    assert np.all(np.isfinite(got))
    assert np.array_equal(got, _lib.logl_segments(h, ts, a, b)), 'second evaluation'
    assert np.array_equal(got, _lib.logl_segments(h, ts, a, b, states=False)), 'states=False'
    assert np.array_equal(got, _lib.logl_segments(h, ts, a, b, split=False)), 'split=False'
    assert np.array_equal(got, _under(['BILD_NO_ONE_LAUNCH'], lambda: _lib.logl_segments(h, ts, a, b))), 'BILD_NO_ONE_LAUNCH'
    # the same rows inside a large random batch
    ss, thetas = H.candidate_profiles(rng, n_random, K1 - 1, S)
    ra, rb = np.zeros((n_random, K1), dtype=np.int32), np.zeros((n_random, K1), dtype=np.int32)
    states = H.expand(ss, thetas, T)
    for r in range(n_random):
        cuts = np.nonzero(np.diff(states[r]))[0] + 1
        starts = [0] + [int(c) for c in cuts]
        ra[r] = starts + [T + 3 + i for i in range(K1 - len(starts))]
        rb[r, :len(starts)] = states[r][starts]
        for i in range(len(starts), K1):
            rb[r, i] = (rb[r, i - 1] + 1) % S
    where = rng.permutation(n_random + len(a))
    big_a, big_b = np.concatenate([a, ra])[where], np.concatenate([b, rb])[where]
    big = _lib.logl_segments(h, ts, big_a, big_b)
    back = np.empty(len(where), dtype=np.int64)
    back[where] = np.arange(len(where))
    assert np.array_equal(got, big[back[:len(a)]]), 'inside a large random batch'
    return a, b, keys, got, ts


def against_oracle(rng, model, data, a, b, got, T, n=32):
    from oracle import oracle
    from bild_amd import profiles
    pick = rng.choice(len(a), min(n, len(a)), replace=False)
    want = oracle.logl_batch(model.arrays(), model.measurement, model.localization_error, data[:], profiles.states_from_segments(a[pick], b[pick], T))
    err = float(np.max(np.abs(got[pick] - want)))
    print(f"max |logL - oracle| over {len(pick)} = {err:.2e}")
    assert err < TOL


@pytest.mark.parametrize('K1', [5, 6])
def test_sweep_two_states(built_lib, K1):
    """ chains of three and four (K1 = 5: the one-launch kernel) and of five close switches (K1 = 6: walk and listed frame loop) """
    S, T = 2, 250
    rng, model, data = make(S, T)
    m1 = measured_single(model, data, S, T)
    a, b, keys, got, _ = sweep(rng, model, data, S, T, K1, m1, t1s=[40, T - 70])
    against_oracle(rng, model, data, a, b, got, T)


def test_frames_saved_where_the_conditions_hold(built_lib):
    """ three-switch chains from a synchronised start: which of them start at their third switch, told from measured table entries """
    from bild_amd import _lib
    S, T = 2, 250
    rng, model, data = make(S, T, seed=1)
    m1 = measured_single(model, data, S, T)
    conv = [m1[s, sn, t] for s in range(S) for sn in range(S) if sn != s for t in range(1, T) if t + m1[s, sn, t] < T]
    m_max = int(max(conv))                      # the set's longest converged transient: what the tables' ranges are sized by
    gap_max, pgap = min(128, m_max), min(128, m_max + 1)
    t1s = [40, 121, T - 70]
    parts = [chains(rng, T, S, 5, [t1], sorted({1, 2, 3, 4, int(min(m1[0, 1, t1], m1[1, 0, t1])) - 1}), [()]) for t1 in t1s]
    a, b = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    keys = [k for p in parts for k in p[2]]
    m_pair = measured_pairs(model, data, [k[:5] for k in keys])
    ok, saved = np.zeros(len(keys), dtype=bool), np.zeros(len(keys), dtype=np.int64)
    seen = {'a': set(), 'b': set(), 'c': set()}
    for r, (s, sn, sm, t1, g1, g2, _) in enumerate(keys):
        chain = g1 < m1[s, sn, t1]                                          # (else the first switch comes out of the single table)
        ca = g1 < gap_max and g2 < pgap                                     # (a) a record exists
        cb = g1 + g2 < m_pair[(s, sn, sm, t1, g1)]                          # (b) the builder ran beyond t3
        m_ref = m1[sn, sm, t1 + g1]
        cc = g2 < m_ref + MARGIN                                            # (c) no tail in the gap
        for name, c in (('a', ca), ('b', cb), ('c', cc)):
            seen[name].add(bool(c))
        ok[r] = chain and ca and cb and cc
        saved[r] = g2 - STRIDE + 1
    assert all(v == {True, False} for v in seen.values()), seen             # every condition met and missed in the sweep
    assert ok.sum() >= 100 and (~ok).sum() >= 100
    ts = model.trajset(_fresh(data))
    h = model.handle()
    run = lambda rows: _lib.logl_segments(h, ts, a[rows], b[rows])
    run(ok)  # (tables)
    on = {w: _frames_total(model, lambda: run(sel)) for w, sel in (('ok', ok), ('not', ~ok))}
    off = {w: _under(['BILD_NO_PAIR_STATES'], lambda: _frames_total(model, lambda: run(sel))) for w, sel in (('ok', ok), ('not', ~ok))}
    print(f"{ok.sum()} chains qualify: frames {off['ok'][1]} -> {on['ok'][1]} (bound {saved[ok].sum()}); {(~ok).sum()} do not: "
          f"{off['not'][1]} -> {on['not'][1]}")
    for w in ('ok', 'not'):
        assert np.array_equal(on[w][0], off[w][0]), w
    assert off['ok'][1] - on['ok'][1] >= saved[ok].sum()
    assert off['not'][1] == on['not'][1]


VARIATIONS = {
    'three_states':   dict(S=3),
    'missing_iid':    dict(missing='iid'),
    'missing_in_gaps': dict(missing='gaps'),
    'dstar2':         dict(err=[0.1, 0.1, 0.3]),
    'last_frames':    dict(t1s='end'),
    'tail_margin_0':  dict(env=['BILD_TAIL_MARGIN=0']),
    'no_tail':        dict(env=['BILD_NO_TAIL']),
    'stride_1':       dict(env=['BILD_PAIR_STATES_STRIDE=1']),
    'first_level_only': dict(env=['BILD_STATES_MAX_BYTES=60000000'], refused=True),
}


@pytest.mark.parametrize('name', sorted(VARIATIONS))
def test_sweep_under_variations(built_lib, name):
    from bild_amd import _lib
    v = VARIATIONS[name]
    S, T = v.get('S', 2), 220
    missing = None
    if v.get('missing') == 'iid':
        missing = H.missing_mask(np.random.default_rng(5), T, 'iid')
    elif v.get('missing') == 'gaps':
        missing = np.array([42, 45, 52, 123, 126, 140])   # inside the first and the second gap of the chains at t1 = 40 and 121
    rng, model, data = make(S, T, err=v.get('err', 0.1), missing=missing, seed=2 + sorted(VARIATIONS).index(name))

    def body():
        m1 = measured_single(model, data, S, T)
        # (t1s 'end': the third switch on the last frames of the trajectory for the largest g1 + g2 of the sweep and before)
        t1s = [T - 66, T - 40, T - 12] if v.get('t1s') == 'end' else [40, 121]
        a, b, keys, got, ts = sweep(rng, model, data, S, T, 5, m1, t1s, n_random=1000)
        against_oracle(rng, model, data, a, b, got, T, n=16)
        return ts

    ts = _under(v.get('env', []), body)
    if 'refused' in v:
        # the budget holds the first level (gaps x T x 2 records of 1104 bytes: ~20 MB) and not the second: the bytes are those of
        # a set that was told to build no pair state table
        other = model.trajset(_fresh(data))
        _under(v['env'] + ['BILD_NO_PAIR_STATES'], lambda: _lib.logl_segments(model.handle(), other, np.array([[0, 50, 60, 70]], dtype=np.int32),
                                                                              np.array([[0, 1, 0, 1]], dtype=np.int32)))
        assert _lib.prefix_info(ts)[0] == _lib.prefix_info(other)[0] > 0


def test_three_trajectories(built_lib):
    """ three trajectories of different lengths through traj_id: the per-trajectory bases of the index """
    from bild_amd import _lib
    from oracle import oracle
    from bild_amd import profiles
    S = 2
    rng, model, _ = make(S, 100, seed=20)
    Ts = [180, 250, 131]
    datas = [model.trajectory_from_loopingprofile(H.random_profile(rng, T, S, T // 5), rng=rng) for T in Ts]
    a, b, tid = [], [], []
    for j, T in enumerate(Ts):
        aj, bj, _ = chains(rng, T, S, 5, [30, T - 70], [1, 3, 20], [(), (6,)])
        aj[aj >= T] += max(Ts)  # (behind every trajectory)
        a.append(aj), b.append(bj), tid.append(np.full(len(aj), j, dtype=np.int32))
    a, b, tid = np.concatenate(a), np.concatenate(b), np.concatenate(tid)
    ts = model.trajset(_fresh(datas))
    h = model.handle()
    got = _lib.logl_segments(h, ts, a, b, tid)
    assert np.all(np.isfinite(got))
    assert np.array_equal(got, _lib.logl_segments(h, ts, a, b, tid, states=False))
    assert np.array_equal(got, _lib.logl_segments(h, ts, a, b, tid, split=False))
    assert np.array_equal(got, _under(['BILD_NO_ONE_LAUNCH'], lambda: _lib.logl_segments(h, ts, a, b, tid)))
    off = _under(['BILD_NO_PAIR_STATES'], lambda: _lib.logl_segments(h, model.trajset(_fresh(datas)), a, b, tid))
    assert np.array_equal(got, off)
    for j, T in enumerate(Ts):
        rows = np.nonzero(tid == j)[0]
        pick = rng.choice(rows, 8, replace=False)
        want = oracle.logl_batch(model.arrays(), model.measurement, model.localization_error, datas[j][:],
                                 profiles.states_from_segments(a[pick], b[pick], T))
        assert np.max(np.abs(got[pick] - want)) < TOL


def test_table_accounting(built_lib):
    """ prefix_info counts the table: T x S (S - 1)^2 x (gap_max - 1) x records per entry x 1104 bytes for 10 modes """
    from bild_amd import _lib
    S, T = 2, 250
    rng, model, data = make(S, T, seed=30)
    m1 = measured_single(model, data, S, T)
    m_max = int(max(m1[s, sn, t] for s in range(S) for sn in range(S) if sn != s for t in range(1, T) if t + m1[s, sn, t] < T))
    a, b, _ = chains(rng, T, S, 5, [40], [2], [()])
    h = model.handle()
    with_table, without = model.trajset(_fresh(data)), model.trajset(_fresh(data))
    got = _lib.logl_segments(h, with_table, a, b)
    off = _under(['BILD_NO_PAIR_STATES'], lambda: _lib.logl_segments(h, without, a, b))
    assert np.array_equal(got, off)
    assert np.array_equal(got, _lib.logl_segments(h, with_table, a, b))
    assert h.query(4) == 10
    records = T * S * (S - 1) ** 2 * (min(128, m_max) - 1) * ((min(128, m_max + 1) - 2) // STRIDE + 1)
    assert _lib.prefix_info(with_table)[0] - _lib.prefix_info(without)[0] == records * 1104
