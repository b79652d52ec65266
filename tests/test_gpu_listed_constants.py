"""
Tasks with DIFFERENT descriptors on the row pairs of one workgroup and in the successive layers of one row of the listed frame
loop (kernels.hip: logl_one_kernel, logl_body).  The events of a task -- looks at the table, jumps, starts, tails -- address the
tables through the task's trajectory descriptor and chain: record base, mscale, the bases of the transient and state tables.  The
cases of test_gpu_pair_events.py give all tasks of a workgroup the same descriptor or nearly so; a change that keeps such per-task
constants anywhere a neighbouring or a later task can see them (the LDS area of a row, say: DESIGN.md section 4, round 7) can go
wrong only where neighbours and successors differ.

The batch: three trajectories of different lengths (T = 150, 300, 450; candidate r on trajectory r % 3) with localisation errors
(0.1, 0.1, 0.3), so that every candidate is two tasks, chain e = 0 and chain e = 1, with different s2 and mscale, next to each other
in the workgroup's slice; frames missing as in the pair-events test; candidates only chains of three and four close switches.
n = 2048: every workgroup of the one-launch grid lists its tasks on row pairs; n = 12 000: more than 16 listed tasks per workgroup,
the one-row frame and later layers.  Each size: the default path bit for bit equal to BILD_NO_ONE_LAUNCH, BILD_NO_SPLIT and
BILD_NO_STATES, finite, the frames run equal to those of the two-kernel path, the small batch's results equal where its candidates
sit inside the large one, and 24 random candidates within 1e-8 of the oracle.  And the headline's flavour: two states, one
trajectory, no frame missing, T = 200, n = 64.

`chains` restates the generator of the pair-events test with one trajectory length per candidate.  One kind differs: a chain that
"runs into the trajectory's end" has four switches and keeps the first three inside (only the fourth may fall beyond the last
frame), so that every candidate is a chain of at least three kept switches -- which test_chains_keep_three_switches checks
without a GPU.
"""
import os

import numpy as np
import pytest

import helpers as H

TOL = 1e-8
ONE = 'logl_one_kernel<modal>'
K1 = 5
LENGTHS = (150, 300, 450)
SIZES = (2048, 12000)
N_HEADLINE, T_HEADLINE = 64, 200

_skipped = []


def _under(names, fn):
    from bild_amd import _lib
    for name in names:
        os.environ[name] = '1'
    _lib.config_reload()
    try:
        return fn()
    finally:
        for name in names:
            del os.environ[name]
        _lib.config_reload()


def _timed(handle, fn):
    """ result, timed kernel name and frames run of one evaluation """
    from bild_amd import _lib
    _lib.kernel_timing_read()
    _lib.kernel_timing_read_walk()
    _lib.frames_run_read(handle)
    _lib.kernel_timing(True)
    try:
        got = fn()
    finally:
        _lib.kernel_timing(False)
    _, _, name = _lib.kernel_timing_read()
    _lib.kernel_timing_read_walk()
    return got, name, _lib.frames_run_read(handle)


def chains(rng, Ts, S):
    """ (n, K1) segment lists, candidate r on a trajectory of Ts[r] frames: three or four switches with gaps of 1 ... 40 frames """
    n = len(Ts)
    seg_start = np.zeros((n, K1), dtype=np.int32)
    seg_state = np.zeros((n, K1), dtype=np.int32)
    for r in range(n):
        T = int(Ts[r])
        kind = r % 8
        links = 4 if kind == 6 else 3 + (r & 1)
        gaps = rng.integers(1, 41, size=links - 1)
        span = int(gaps.sum())
        if kind == 2:
            t1 = 1                                   # right at the start
        elif kind == 4:
            t1 = T - 1 - span                        # the last switch on the last frame
        elif kind == 6:
            t1 = T - 1 - int(rng.integers(int(gaps[0] + gaps[1]), span + 1))  # a fourth switch may fall beyond the end
        else:
            t1 = int(rng.integers(1, T - span))
        seg_start[r, 1] = t1
        seg_start[r, 2:1 + links] = t1 + np.cumsum(gaps)
        if links == 3:
            seg_start[r, 4] = max(T, seg_start[r, 3]) + 3  # (a fifth segment beyond the trajectory: cleaned away)
        s = int(rng.integers(S))
        for i in range(K1):
            seg_state[r, i] = s
            s = int((s + 1 + rng.integers(S - 1)) % S)
    return seg_start, seg_state


def kept_switches(seg_start, seg_state, Ts):
    """ per candidate: boundaries that are real switches inside the trajectory (what the kernel's cleaned list holds) """
    kept = np.zeros(len(Ts), dtype=np.int64)
    for r in range(len(Ts)):
        prev = seg_state[r, 0]
        for i in range(1, K1):
            start = seg_start[r, i]
            end = seg_start[r, i + 1] if i + 1 < K1 else np.iinfo(np.int32).max
            if start >= Ts[r]:
                break
            if end <= start or seg_state[r, i] == prev:
                continue
            prev = seg_state[r, i]
            kept[r] += 1
    return kept


def gap_mask(rng, T):
    """ 5 % of the frames missing, and one gap of 60 ... 120 frames """
    mask = rng.random(T) < 0.05
    start = int(rng.integers(T // 4, T // 2))
    mask[start:start + int(rng.integers(60, 121))] = True
    mask[0] = False
    return np.nonzero(mask)[0]


def _lengths(n):
    return np.asarray(LENGTHS, dtype=np.int64)[np.arange(n) % len(LENGTHS)]


def test_chains_keep_three_switches():
    """ no GPU: every candidate of the shapes below is a chain of three or four switches inside its trajectory, gaps 1 ... 40 """
    for seed, Ts, S in ((700, _lengths(max(SIZES)), 2), (701, np.full(N_HEADLINE, T_HEADLINE), 2)):
        seg_start, seg_state = chains(np.random.default_rng(seed), Ts, S)
        kept = kept_switches(seg_start, seg_state, Ts)
        assert kept.min() >= 3 and kept.max() <= 4, (kept.min(), kept.max())
        assert np.any(kept == 3) and np.any(kept == 4)
        assert np.all(seg_start[:, 1] >= 1)
        gaps = np.diff(seg_start[:, 1:4], axis=1)
        assert gaps.min() >= 1 and gaps.max() <= 40
        assert seg_state.min() >= 0 and seg_state.max() < S
        # candidates of the same trajectory come in both chain lengths
        assert {(int(T), int(k)) for T, k in zip(Ts, kept)} >= {(int(T), k) for T in set(Ts.tolist()) for k in (3, 4)}


@pytest.fixture(scope='module')
def batch(built_lib):
    """ the three-trajectory batch, and the default path's results per size (each computed once, shared, left unchanged) """
    import bild_amd
    rng = np.random.default_rng(700)
    Ts = _lengths(max(SIZES))
    seg_start, seg_state = chains(rng, Ts, 2)
    model = bild_amd.MultiStateRouse(20, 1, 5, d=3, localization_error=[0.1, 0.1, 0.3])
    assert model.nStates == 2
    trng = np.random.default_rng(702)
    trajs = [model.trajectory_from_loopingprofile(H.random_profile(trng, T, 2, T // 5), missing_frames=gap_mask(trng, T), rng=trng)
             for T in LENGTHS]
    traj_id = (np.arange(max(SIZES)) % len(LENGTHS)).astype(np.int32)
    b = dict(model=model, trajs=trajs, seg_start=seg_start, seg_state=seg_state, traj_id=traj_id, Ts=Ts, default={})

    def run(n):
        return model.logL_segments(seg_start[:n], seg_state[:n], trajs, traj_id[:n])

    b['run'] = run
    run(SIZES[0])  # (tables built by the first evaluation of the set)
    for n in SIZES:
        got, kernel, frames = _timed(model.handle(), lambda: run(n))
        got.setflags(write=False)
        b['default'][n] = (got, kernel, frames)
    return b


def _reached_one_launch(kernel, what):
    if kernel != ONE:
        assert not _skipped, f"{what} runs {kernel}, and {_skipped[0]} did not reach the one-launch path either"
        _skipped.append(what)
        pytest.skip(f"{what} does not reach the one-launch path: its listed frame loop runs {kernel}")


@pytest.mark.gpu
@pytest.mark.parametrize('n', SIZES)
def test_tasks_of_different_descriptors(batch, n):
    from oracle import oracle
    from bild_amd import profiles
    model, run = batch['model'], batch['run']
    h = model.handle()
    assert h.query(4) == 10  # BILD_Q_NP: geometry 23, the listed frame loop with row pairs and one launch
    got, kernel, frames = batch['default'][n]
    _reached_one_launch(kernel, f"n = {n}")
    assert np.all(np.isfinite(got))
    two, kernel2, frames2 = _under(['BILD_NO_ONE_LAUNCH'], lambda: _timed(h, lambda: run(n)))
    assert kernel2 != ONE
    print(f"n = {n}: frames run {frames} (one launch) / {frames2} (two kernels)")
    assert np.max(np.abs(got - two)) == 0.0, 'BILD_NO_ONE_LAUNCH'
    assert frames == frames2 and frames > 0
    for flag in ('BILD_NO_SPLIT', 'BILD_NO_STATES'):
        other = _under([flag], lambda: run(n))
        assert np.max(np.abs(got - other)) == 0.0, flag
    # the small batch's candidates inside the large one: row pairs there, the one-row frame and later layers here
    small, large = batch['default'][SIZES[0]][0], batch['default'][SIZES[1]][0]
    assert np.max(np.abs(small - large[:SIZES[0]])) == 0.0, 'small batch inside the large one'
    pick = np.random.default_rng(703 + n).choice(n, 24, replace=False)
    want = np.empty(len(pick))
    for j, T in enumerate(LENGTHS):
        on_j = (pick % len(LENGTHS)) == j
        states = profiles.states_from_segments(batch['seg_start'][pick[on_j]], batch['seg_state'][pick[on_j]], T)
        want[on_j] = oracle.logl_batch(model.arrays(), model.measurement, model.localization_error, batch['trajs'][j][:], states)
    err = float(np.max(np.abs(got[pick] - want)))
    print(f"n = {n}: max |logL - oracle| over 24 = {err:.2e}")
    assert err < TOL


@pytest.mark.gpu
def test_headline_flavour(built_lib):
    """ two states, one trajectory, every frame observed: the flavour of the headline batch, one task per workgroup """
    import bild_amd
    from oracle import oracle
    from bild_amd import profiles
    rng = np.random.default_rng(701)
    n, T = N_HEADLINE, T_HEADLINE
    seg_start, seg_state = chains(rng, np.full(n, T), 2)
    model = bild_amd.MultiStateRouse(20, 1, 5, d=3, localization_error=0.1)
    traj = model.trajectory_from_loopingprofile(H.random_profile(rng, T, 2, T // 5), rng=rng)
    h = model.handle()

    def run():
        return model.logL_segments(seg_start, seg_state, traj, None)

    run()
    got, kernel, frames = _timed(h, run)
    _reached_one_launch(kernel, "the headline's flavour")
    assert np.all(np.isfinite(got))
    two, kernel2, frames2 = _under(['BILD_NO_ONE_LAUNCH'], lambda: _timed(h, run))
    assert kernel2 != ONE
    assert np.max(np.abs(got - two)) == 0.0, 'BILD_NO_ONE_LAUNCH'
    assert frames == frames2 and frames > 0
    for flag in ('BILD_NO_SPLIT', 'BILD_NO_STATES'):
        other = _under([flag], run)
        assert np.max(np.abs(got - other)) == 0.0, flag
    pick = rng.choice(n, 24, replace=False)
    states = profiles.states_from_segments(seg_start[pick], seg_state[pick], T)
    want = oracle.logl_batch(model.arrays(), model.measurement, model.localization_error, traj[:], states)
    err = float(np.max(np.abs(got[pick] - want)))
    print(f"headline flavour: max |logL - oracle| over 24 = {err:.2e}")
    assert err < TOL
