"""
The frame loop over the work lists (geometry 23) runs a short list on row PAIRS -- each row holds half of every column
(kernels.hip, logl_kernel) -- and a long one on single rows.  Both must give the bits of the unsplit launch and of the
launch without the transient state table, on the bench's own batch at k = 4 / 8 / 15 and on a batch over three trajectories.
"""
import os

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

TOL = 1e-8


def _under(name, fn):
    from bild_amd import _lib
    os.environ[name] = '1'
    _lib.config_reload()
    try:
        return fn()
    finally:
        del os.environ[name]
        _lib.config_reload()


def _check(model, run, want_fn, n):
    got = run()
    assert np.all(np.isfinite(got))
    for name in ('BILD_NO_SPLIT', 'BILD_NO_STATES'):
        other = _under(name, run)
        assert np.max(np.abs(got - other)) == 0.0, name
    rng = np.random.default_rng(n)
    pick = rng.choice(n, 24, replace=False)
    assert np.max(np.abs(got[pick] - want_fn(pick))) < TOL


@pytest.mark.parametrize('k', [4, 8, 15])
def test_bench_batch(built_lib, k):
    import bench
    from oracle import oracle
    model, trajs, ss, thetas = bench.build_workload(0, 10000, 1000, k)
    traj = trajs[0]
    T = len(traj)

    def want(pick):
        return oracle.logl_batch(model.arrays(), model.measurement, model.localization_error, traj[:],
                                 H.expand(ss[pick], thetas[pick], T))
    _check(model, lambda: model.logL_st_batch(ss, thetas, traj), want, len(ss))


def test_three_trajectories(built_lib):
    import bench
    from bild_amd import profiles
    from oracle import oracle
    n = 3000
    model, trajs, ss, thetas = bench.build_workload(1, n, 400, 6, n_traj=3)
    T = len(trajs[0])
    seg_start, seg_state = profiles.segments_from_st(ss, thetas, T)
    traj_id = (np.arange(len(ss)) % 3).astype(np.int32)

    def want(pick):
        res = np.empty(len(pick))
        for j in range(3):
            on_j = traj_id[pick] == j
            sel = pick[on_j]
            res[on_j] = oracle.logl_batch(model.arrays(), model.measurement, model.localization_error, trajs[j][:],
                                          H.expand(ss[sel], thetas[sel], T))
        return res
    _check(model, lambda: model.logL_segments(seg_start, seg_state, trajs, traj_id), want, len(ss))
