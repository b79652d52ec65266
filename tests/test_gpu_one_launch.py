"""
The one-launch path (kernels.hip: logl_one_kernel): on a small split batch the table walk and the listed frame loop share one
grid, handing the listed tasks over in LDS.  It must give the bits of the two-kernel path (BILD_NO_ONE_LAUNCH) and of the
unsplit launch (BILD_NO_SPLIT), run the same frames as the two kernels, and really be the kernel that ran (the timed name).
Fused and two-kernel launches alternate on one model: the fused launch must leave the work-list counter sets alone.
"""
import os

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

ONE = 'logl_one_kernel<modal>'
BOUND = 32768  # likelihood.h: kOneLaunchMaxTasks
MAX_K = 4      # likelihood.h: kOneLaunchMaxK1 = 5 segments


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
    """ result, timed kernel name and frames run of one evaluation (handle: the model's native handle) """
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


def _check(handle, run, fused):
    """ fused (default), two kernels, unsplit: the same bits; fused and two kernels: the same frames """
    run()  # (tables built by the first evaluation of the set)
    got, name, frames = _timed(handle, run)
    two, name2, frames2 = _under(['BILD_NO_ONE_LAUNCH'], lambda: _timed(handle, run))
    ref = _under(['BILD_NO_SPLIT'], run)
    if fused is not None:
        assert (name == ONE) == fused, name
    assert name2 != ONE
    assert np.array_equal(got, two, equal_nan=True)
    assert np.array_equal(got, ref, equal_nan=True)
    assert frames == frames2
    return got


@pytest.mark.parametrize('k', [3, 4, 5, 8, 15])
def test_bench_batch(built_lib, k):
    import bench
    model, trajs, ss, thetas = bench.build_workload(0, 10000, 1000, k)
    got = _check(model.handle(), lambda: model.logL_st_batch(ss, thetas, trajs[0]), k <= MAX_K)
    assert np.all(np.isfinite(got))


@pytest.mark.parametrize('n', [1, 37, BOUND + 1])
def test_batch_sizes(built_lib, n):
    import bench
    model, trajs, ss, thetas = bench.build_workload(3, n, 1000, 4)
    _check(model.handle(), lambda: model.logL_st_batch(ss, thetas, trajs[0]), n <= BOUND)


@pytest.mark.parametrize('S,k', [(2, 3), (2, 4), (3, 4), (3, 8)])
def test_trajectories_missing_dstar2(built_lib, S, k):
    """ three trajectories (traj_id), bursts of missing frames, d* = 2.  Two states: the fused path (geometry 23); three states reduce
    to 16 rows, whose listed geometry (24) keeps the two kernels """
    import bild_amd
    from bild_amd import profiles
    rng = np.random.default_rng(11 * S + k)
    T, n = 300, 3000
    model = bild_amd.MultiStateRouse(20, 1, 5, d=3, looppositions=H.LOOPS[S], localization_error=[0.1, 0.1, 0.3])
    trajs = [model.trajectory_from_loopingprofile(H.random_profile(rng, T, S, T // 5), missing_frames=H.missing_mask(rng, T, 'bursty'),
                                                  rng=rng) for _ in range(3)]
    ss, thetas = H.candidate_profiles(rng, n, k, S)
    seg_start, seg_state = profiles.segments_from_st(ss, thetas, T)
    traj_id = (np.arange(n) % 3).astype(np.int32)
    h = model.handle()
    assert h.query(4) == (10 if S == 2 else 16)  # BILD_Q_NP
    _check(h, lambda: model.logL_segments(seg_start, seg_state, trajs, traj_id), S == 2 and k <= MAX_K)


def test_uncleaned_lists(built_lib):
    """ boundaries that switch nothing, empty segments and segments beyond the trajectory's end """
    import bench
    from bild_amd import profiles
    model, trajs, ss, thetas = bench.build_workload(5, 4000, 400, 4)
    T = len(trajs[0])
    seg_start, seg_state = profiles.segments_from_st(ss, thetas, T)
    seg_start, seg_state = seg_start.copy(), seg_state.copy()
    rng = np.random.default_rng(5)
    rows = rng.choice(len(ss), 1500, replace=False)
    for r in rows[:500]:  # a boundary that switches nothing
        seg_state[r, 2] = seg_state[r, 1]
    for r in rows[500:1000]:  # an empty segment
        seg_start[r, 3] = seg_start[r, 2]
    for r in rows[1000:]:  # the list's tail beyond the trajectory
        seg_start[r, 4:] = T + 3
    _check(model.handle(), lambda: model.logL_segments(seg_start, seg_state, trajs[0]), True)


@pytest.mark.parametrize('T', [80, 200])
def test_most_tasks_listed(built_lib, T):
    """ short trajectories: switches close together, most tasks listed; slices of 63 tasks.  Workgroups then list more tasks than
    they have row pairs (the fused one-row frame) and more than they have rows (later layers: the whole prologue, on lists the same
    launch wrote) """
    import bench
    n = 32000
    model, trajs, ss, thetas = bench.build_workload(11, n, T, 4)
    got = _check(model.handle(), lambda: model.logL_st_batch(ss, thetas, trajs[0]), True)
    assert np.all(np.isfinite(got))


def test_refused_rows_device(built_lib):
    """ (s, theta) rows that are no point on the simplex: NaN and the status word, as in the two-kernel path """
    import torch
    import bench
    from bild_amd import _lib
    model, trajs, ss, thetas = bench.build_workload(7, 2000, 1000, 4)
    ss, thetas = ss.copy(), thetas.copy()
    ss[5, 1] = -0.25
    thetas[17, 2] = 9
    ss[1999, 0] = np.nan
    h, ts = model.handle(), model.trajset(trajs[0])
    dev = torch.device('cuda', 0)
    d_ss = torch.from_numpy(np.ascontiguousarray(ss)).to(dev)
    d_th = torch.from_numpy(np.ascontiguousarray(thetas).astype(np.uint8)).to(dev)

    def run():
        d_out = torch.empty(len(ss), dtype=torch.float64, device=dev)
        d_status = torch.zeros(2, dtype=torch.int32, device=dev)
        _lib.logl_st_device(h, ts, len(ss), ss.shape[1], d_ss.data_ptr(), d_th.data_ptr(), d_out.data_ptr(), d_status=d_status.data_ptr())
        torch.cuda.synchronize()
        return np.concatenate([d_out.cpu().numpy(), d_status.cpu().numpy()[:1].astype(np.float64)])

    got = _check(h, run, True)
    assert np.all(np.isnan(got[[5, 17, 1999]])) and got[-1] != 0
    assert np.sum(np.isnan(got[:-1])) == 3


def test_alternating_on_one_stream(built_lib):
    """ fused and two-kernel launches in turn on one model: each gives the bits of the unsplit launch """
    import bench
    model, trajs, ss, thetas = bench.build_workload(9, 6000, 1000, 4)
    run = lambda: model.logL_st_batch(ss, thetas, trajs[0])  # noqa: E731
    ref = _under(['BILD_NO_SPLIT'], run)
    for i in range(6):
        got = _under(['BILD_NO_ONE_LAUNCH'], run) if i % 2 else run()
        assert np.array_equal(got, ref, equal_nan=True), i
