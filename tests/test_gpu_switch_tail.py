"""
The switch tail (csrc/tail.hip "switch tails", logl_body.h: compare_with_table): behind the third switch
of a chain of close switches, a look that finds the covariance converged but the next switch too close for the ordinary first-order
tail ends the chain all the same -- with the dot product of the means' deviation and a vector whose adjoint runs THROUGH that switch.

Hand-placed chains of 4-6 switches on T = 300: g1, g2 in [2, 20), a later gap swept from 20 to the set's longest transient (measured
on a set without transient table), room behind the switch the tail goes through.  Sub-batches by construction:
  'q'   the long gap is the chain's third, the switch behind it has >= 70 frames of room: the tail may be taken;
  'q2'  two long gaps in a row (third and fourth): the look in the third is refused by (c), the one in the fourth may take the tail;
  'c'   as 'q', but the last switch lies within 8 frames of the trajectory's end: rule (c) refuses (no transient entry fits);
  'd'   the long gap is the chain's SECOND: rule (d) refuses.
The inputs are steered, not only seeded: in the two-state models the third switch of seven 'q' rows in eight is 1 -> 0, behind which
the covariance is within 2^-52 of the table's at the first look; behind 0 -> 1 it is at 2^-43.5 -- inside the kernel's tolerance,
outside the quarter of it that the NumPy criterion asks for.  Rows of the other direction are held to the same assertions where they
clear the criterion.  The factored basis change (five and more states at 16 modes) is not reached by these models.
Accuracy against the frame-by-frame run with test_gpu_tail.py's scale and bars; the bit-identities of the default path; frames
counted per task on the device.
"""
import ctypes

import numpy as np
import pytest

import helpers as H
from test_gpu_pair_states import _fresh, _under

pytestmark = pytest.mark.gpu

T = 300
K1 = {4: 5, 6: 7}   # switches -> segments per row (5: the one-launch kernel; 7: table walk and listed frame loop)
JUMP_FIRST = 24     # first look behind a switch (BILD_JUMP_FIRST)
MARGIN = 8          # BILD_TAIL_MARGIN's default
NEVER = 1 << 30
WAIT_MAX = 44       # the longest wait a look schedules for a deviation that is a number (compare_with_table)


def _frames_per_task(model, ts, a, b, **kw):
    """ frames every task of the batch ran itself (bild_debug_frames_per_task), (n, d*), and the results """
    import torch
    from bild_amd import _lib
    dev = torch.device('cuda', 0)
    n, k1 = a.shape
    dstar = max(1, len(np.unique(np.atleast_1d(model.localization_error))))
    d_a, d_b = torch.from_numpy(a.astype(np.int32)).to(dev), torch.from_numpy(b.astype(np.int32)).to(dev)
    out = torch.empty(n, dtype=torch.float64, device=dev)
    frames = torch.full((n * dstar,), -1, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    _lib.lib().bild_debug_frames_per_task(ctypes.c_void_p(frames.data_ptr()))
    try:
        _lib.logl_segments_device(model.handle(), ts, n, k1, d_a.data_ptr(), d_b.data_ptr(), 0, out.data_ptr(), stream=stream, **kw)
        torch.cuda.synchronize()
    finally:
        _lib.lib().bild_debug_frames_per_task(None)
    return frames.cpu().numpy().reshape(n, dstar), out.cpu().numpy()


def _measured_transients(model, data, S):
    """ m[s, sn, t, e]: frames the transient of a switch s -> sn at frame t runs in chain e until it has converged (the transient
    table's m), measured on a set that has no transient table and no tails: every candidate runs its transient itself """
    rows = [(s, sn, t) for s in range(S) for sn in range(S) if sn != s for t in range(1, T)]
    a = np.zeros((len(rows), 2), dtype=np.int32)
    b = np.zeros((len(rows), 2), dtype=np.int32)
    for r, (s, sn, t) in enumerate(rows):
        a[r, 1], b[r, 0], b[r, 1] = t, s, sn

    def run():
        ts = model.trajset(_fresh(data))
        _frames_per_task(model, ts, a[:1], b[:1])   # (tables)
        return _frames_per_task(model, ts, a, b)[0]

    fr = _under(['BILD_NO_TRANSIENTS', 'BILD_NO_TAIL'], run)
    m = np.zeros((S, S, T, fr.shape[1]), dtype=np.int64)
    for r, (s, sn, t) in enumerate(rows):
        m[s, sn, t] = fr[r]
    return m


def _rows(rng, S, m_max, n_switches):
    """ segment lists of K1[n_switches] segments, their kind, and (t3, long gap) of the kinds that may take the tail """
    k1 = K1[n_switches]
    a, b, kind, info = [], [], [], []

    def put(starts, what, t3=0, gap=0):
        assert all(y > x for x, y in zip(starts, starts[1:])) and starts[-1] < T and len(starts) <= k1, (starts, what)
        starts = starts + [T + 3 + i for i in range(k1 - len(starts))]
        # (two states: the covariance behind a switch 1 -> 0 is within 2^-52 of the table's at the first look, behind 0 -> 1 at
        # 2^-43.5 -- inside the kernel's tolerance, outside a quarter of it: most 'q' rows get the first kind as their third switch)
        states = [1 if S == 2 and what == 'q' and rng.random() < 0.875 else int(rng.integers(S))]
        for _ in range(k1 - 1):
            states.append(int((states[-1] + 1 + rng.integers(S - 1)) % S))
        a.append(starts), b.append(states), kind.append(what), info.append((t3, gap))

    # (room behind the switch a tail goes through: what rule (c) can ask for at most, and more than any transient lasts)
    room = max(75, (40 * m_max + 29) // 30 + 5)
    gaps = range(20, m_max + 1, 1 + (m_max - 19) // 40)
    for rep in range(64):
        if len(a) >= 300:
            break
        for gap in gaps:
            t1, g1, g2 = (int(v) for v in (rng.integers(5, 30), rng.integers(2, 20), rng.integers(2, 20)))
            t3 = t1 + g1 + g2
            # 'q': t1 t2 t3 | gap | t4, room; with six switches a far pair behind (comes out of the pair table)
            far = [t3 + gap + room, t3 + gap + room + int(rng.integers(2, 12))] if n_switches == 6 else []
            put([0, t1, t1 + g1, t3, t3 + gap] + far, 'q', t3, gap)
            # 'c': the same chain pushed to the end of the trajectory, 1 .. 8 frames behind the last switch
            shift = T - int(rng.integers(1, 9)) - (t3 + gap)
            pre = [5, 5 + int(rng.integers(2, 12))] if n_switches == 6 else []   # (a far pair in front)
            put([0] + pre + [t1 + shift, t1 + g1 + shift, t3 + shift, t3 + gap + shift], 'c')
            if rep % 2 == 0:
                # 'd': t1 t2 | gap | t3, room, then far switches (four or five in all)
                far = [t1 + g1 + gap + room + 10 + (room + 10) * i for i in range(1 if n_switches == 4 else 2)]
                put([0, t1, t1 + g1, t1 + g1 + gap] + [f for f in far if f < T - 1], 'd')
                if n_switches == 6:
                    # 'q2': t1 t2 t3 | gap | t4 | gap2 | t5, room, a far sixth switch
                    gap2 = int(rng.integers(20, m_max + 1))
                    put([0, t1, t1 + g1, t3, t3 + gap, t3 + gap + gap2] + [f for f in [t3 + gap + gap2 + room] if f < T - 1], 'q2')
    return np.array(a, dtype=np.int32), np.array(b, dtype=np.int32), np.array(kind), np.array(info)


def _first_clear_look(model, data, a, b, t3s, t4s):
    """ per row and chain e: the first frame u = t - t3, 24 <= u <= t4 - t3, of a look at frame t (the state after frame t - 1 against
    the switch-free filter of the same state) with covariance columns within 2^-45 and mean columns within 2^-22 -- the kernel's
    criteria (relative to the column's largest entry; means: plus the floor TrajDesc::mscale), a factor 4 inside both; NEVER where
    there is none.  NumPy, the modal algorithm from the library's own host analysis (tests/test_abi.py) """
    from bild_amd import _lib as L
    from bild_amd import profiles
    h = model.handle()
    S, n = len(model.arrays()['B']), h.query(L.Q_NEFF)
    lam = [h.export(L.X_LAMBDA, s) for s in range(S)]
    sig = [h.export(L.X_SIGMA, s) for s in range(S)]
    wq = [h.export(L.X_WQ, s) for s in range(S)]
    C0q = [h.export(L.X_C0Q, s) for s in range(S)]
    R = {(p, q): h.export(L.X_R, p, q) for p in range(S) for q in range(S)}
    x = np.asarray(data[:], dtype=float)
    errs = np.broadcast_to(np.atleast_1d(np.asarray(model.localization_error, dtype=float)), (x.shape[1],))
    chains = [(e, np.nonzero(errs == e)[0]) for e in np.unique(errs)]
    wCw = max(float(wq[s] @ C0q[s] @ wq[s]) for s in range(S))

    def run(states, dims, s2, upto):
        """ the states after frames 0 .. upto - 1 """
        s = states[0]
        C, M = C0q[s].copy(), np.zeros((n, len(dims)))
        out = []
        for t in range(upto):
            if t > 0:
                if states[t] != s:
                    Rm = R[(s, states[t])]
                    C, M, s = Rm @ C @ Rm.T, Rm @ M, states[t]
                C = np.outer(lam[s], lam[s]) * C + np.diag(sig[s])
                M = lam[s][:, None] * M
            if not np.isnan(x[t]).any():
                Cw = C @ wq[s]
                Sv = wq[s] @ Cw + s2
                nu = x[t, dims] - wq[s] @ M
                C = C - np.outer(Cw, Cw) / Sv
                M = M + np.outer(Cw, nu) / Sv
            out.append((C, M))
        return out

    free = {(s, c): run(np.full(T, s), dims, err ** 2, T) for s in range(S) for c, (err, dims) in enumerate(chains)}
    first = np.full((len(a), len(chains)), NEVER, dtype=np.int64)
    for r in range(len(a)):
        t3, t4 = int(t3s[r]), int(t4s[r])
        states = profiles.states_from_segments(a[r:r + 1], b[r:r + 1], T)[0]
        for c, (err, dims) in enumerate(chains):
            own = run(states, dims, err ** 2, t4)
            mscale = min(np.nanmax(np.abs(x)), 6 * np.sqrt(err ** 2 + wCw))
            for t in range(t3 + JUMP_FIRST, t4 + 1):
                (C, M), (Ct, Mt) = own[t - 1], free[(int(states[t - 1]), c)][t - 1]
                cov = np.all(np.max(np.abs(C - Ct), axis=0) <= 2.0 ** -45 * np.max(np.abs(Ct), axis=0))
                mean = np.all(np.max(np.abs(M - Mt), axis=0) <= 2.0 ** -22 * np.maximum(np.max(np.abs(Mt), axis=0), mscale))
                if cov and mean:
                    first[r, c] = t - t3
                    break
    return first


CASES = {
    'two_states':   dict(N=20, S=2, err=0.1, miss='none', seed=3, first_look=True, later_looks=()),
    # (three states with bursts of missing frames: the covariance is at 2^-29 ... 2^-37 of the table's at the first look for every one
    # of the six switches (NumPy), so no input clears the criterion there by more than chance; the tails are taken at later looks,
    # and the frames saved are asserted there, by the same criterion at the first frame that meets it.  With six switches the gaps
    # end at 80 frames and no row has a look surely in reach of that frame (WAIT_MAX): 14 + 4 rows x chains hold the property with
    # four switches, none with six)
    'three_states': dict(N=20, S=3, err=[0.1, 0.1, 0.3], miss='bursty', seed=4, first_look=False, later_looks=(4,)),
    # (six modes: the longest transient is the 24 frames in front of the first look, every chain has converged there by the full
    # criterion and no chain runs through its fourth switch: the case holds the identities, and that nothing changes)
    'six_modes':    dict(N=12, S=2, err=0.1, miss='none', seed=5, first_look=False, later_looks=()),
}


@pytest.mark.parametrize('n_switches', [4, 6])
@pytest.mark.parametrize('name', sorted(CASES))
def test_switch_tails(built_lib, name, n_switches):
    import bild_amd
    from bild_amd import _lib
    v = CASES[name]
    S = v['S']
    rng = np.random.default_rng(100 * v['seed'] + n_switches)
    model = bild_amd.MultiStateRouse(v['N'], 1, 5, d=3, looppositions=H.LOOPS[S], localization_error=v['err'])
    data = model.trajectory_from_loopingprofile(H.random_profile(rng, T, S, T // 5), missing_frames=H.missing_mask(rng, T, v['miss']), rng=rng)
    m1 = _measured_transients(model, data, S)
    m_max = int(max(m1[s, sn, t, 0] for s in range(S) for sn in range(S) if sn != s for t in range(1, T) if t + m1[s, sn, t, 0] < T))
    a, b, kind, info = _rows(rng, S, m_max, n_switches)
    assert 300 <= len(a) <= 600, len(a)
    h, ts = model.handle(), model.trajset(_fresh(data))
    _lib.logl_segments(h, ts, a[:4], b[:4])                                   # tables

    def bytes_without():
        other = model.trajset(_fresh(data))
        _lib.logl_segments(h, other, a[:4], b[:4])
        return _lib.prefix_info(other)[0]

    assert _lib.prefix_info(ts)[0] > _under(['BILD_NO_SWITCH_TAIL'], bytes_without) > 0   # (the table exists, and is accounted for)

    # accuracy: test_gpu_tail.py's scale and bars
    on = _lib.logl_segments(h, ts, a, b)
    off = _lib.logl_segments(h, ts, a, b, switch_tail=False)
    exact = _lib.logl_segments(h, ts, a, b, jump=False)
    scale = max(1.0, float(np.max(np.abs(exact))) / 1e4)
    e_on, e_off = float(np.max(np.abs(on - exact))), float(np.max(np.abs(off - exact)))
    print(f"{name}, {n_switches} switches, {len(a)} rows, longest transient {m_max}: |switch tails - frame by frame| {e_on:.2e}, "
          f"|without - frame by frame| {e_off:.2e}, rows changed {int(np.sum(on != off))}")
    assert e_on < 2e-10 * scale
    assert e_on < e_off + 2e-11 * scale

    # bit-identities of the default path
    assert np.array_equal(on, _lib.logl_segments(h, ts, a, b, split=False)), 'split=False'
    assert np.array_equal(on, _lib.logl_segments(h, ts, a, b, states=False)), 'states=False'
    assert np.array_equal(on, _lib.logl_segments(h, ts, a, b, states=False, split=False)), 'states=False, split=False'
    assert np.array_equal(on, _under(['BILD_NO_ONE_LAUNCH'], lambda: _lib.logl_segments(h, ts, a, b))), 'BILD_NO_ONE_LAUNCH'
    assert np.array_equal(off, _under(['BILD_NO_SWITCH_TAIL'], lambda: _lib.logl_segments(h, model.trajset(_fresh(data)), a, b))), 'BILD_NO_SWITCH_TAIL'
    assert np.array_equal(off, _lib.logl_segments(h, ts, a, b, tail=True, switch_tail=False))
    assert np.array_equal(_lib.logl_segments(h, ts, a, b, tail=False), _lib.logl_segments(h, ts, a, b, tail=False, switch_tail=False)), 'tail=False'

    # frames, counted on the device
    f_on, r_on = _frames_per_task(model, ts, a, b)
    f_off, r_off = _frames_per_task(model, ts, a, b, switch_tail=False)
    assert np.array_equal(r_on, on) and np.array_equal(r_off, off)
    assert np.all(f_on <= f_off)
    refused = (kind == 'c') | (kind == 'd')
    assert np.array_equal(f_on[refused], f_off[refused])
    # the qualifying rows and chains: the first look behind the third switch lies in the gap, and without the switch tail the
    # chain runs through the gap and the fourth switch to the first look behind it at least (counted on the device: gap + 24 frames).
    # In a gap longer than its transient a chain converges by the full criterion in front of the fourth switch -- looks come every
    # 4 ... 12 frames there, so "shorter than the measured transient of the third switch" does not decide it to the frame -- and has
    # fewer than gap - 28 frames to save.
    q = (kind == 'q') & (info[:, 1] >= JUMP_FIRST)
    # (by construction: a repetition holds at most four rows per gap, 300 rows take 300 / (4 x gaps) repetitions at least, and each
    # has a 'q' row for every gap from 24 on -- one gap of five at least, where the longest transient is those 24 frames)
    assert q.sum() >= 15, int(q.sum())
    m_ref = m1[b[:, 2], b[:, 3], a[:, 3]][q]
    gap = info[q, 1][:, None]
    qual = f_off[q] >= gap + JUMP_FIRST
    u = _first_clear_look(model, data, a[q], b[q], info[q, 0], a[q][:, 4])
    clear = (u == JUMP_FIRST) & qual
    saved = (f_off - f_on)[q]
    # ... and where the criterion is met at a later frame u only: a look that fails schedules the next one at most WAIT_MAX frames on, so
    # a look falls on one of the frames t3 + u ... t3 + u + WAIT_MAX - 1; where these lie in the gap it takes the tail, and the chain has
    # run u + WAIT_MAX - 1 frames at most, with the <= 2 frames in front of the third switch, instead of gap + 24 at least
    later = (u > JUMP_FIRST) & (u + WAIT_MAX - 1 <= gap) & qual
    bound = np.where(clear, gap - 28, gap + JUMP_FIRST - (u + WAIT_MAX - 1) - 2)
    held = clear | later
    print(f"  frames {int(f_off.sum())} -> {int(f_on.sum())}; 'q' rows {int(q.sum())}, rows x chains that run through the fourth switch without "
          f"switch tails {int(qual.sum())}, of them converged at the first look by NumPy {int(clear.sum())} (saving >= gap - 28: "
          f"{int(np.sum((saved >= gap - 28) & clear))}), at a later frame with a look in reach {int(later.sum())} (saving their bound: "
          f"{int(np.sum((saved >= bound) & later))}; bound {int(bound[later].sum())}, saved {int(saved[later].sum())} frames); q2 rows saving: "
          f"{int(np.sum(np.any((f_off - f_on)[kind == 'q2'] > 0, axis=1)))} of {int(np.sum(kind == 'q2'))}")
    for r, c in zip(*np.nonzero(held & (saved < bound))):
        print(f"  NOT SAVED: row {np.nonzero(q)[0][r]} chain {c}: starts {a[q][r]} states {b[q][r]} gap {gap[r, 0]} u {u[r, c]} bound {bound[r, c]} "
              f"m_ref {m_ref[r]} m1 of the next switch {m1[b[q][r, 3], b[q][r, 4], a[q][r, 4]]} frames {f_off[q][r, c]} -> {f_on[q][r, c]}")
    # conditions on the inputs, checked when the seeds were chosen
    if v['first_look']:
        assert qual.sum() >= 20 and clear.sum() >= 0.75 * qual.sum()
    if n_switches in v['later_looks']:
        assert later.sum() >= 3, int(later.sum())
    if not v['first_look'] and not v['later_looks']:
        assert np.array_equal(f_on, f_off) and np.array_equal(on, off)                        # (nothing to save: nothing changes)
    assert np.all(saved[held] >= bound[held])
