"""
The events of the two-row frame (kernels.hip, logl_body<..., PAIR>): a task on a row pair changes basis with each row computing
the outputs it keeps (sandwich_pair) and looks at the table on its half columns; whole columns exist only in the tail of a look
and where a record is loaded.
Batches made ONLY of chains of three and of four close switches, few enough that the one-launch path runs every one on a
row pair, so that every basis change, look, tail and jump of the pair path runs many times -- and the same candidates again
inside a batch so large that the workgroups list more tasks than they have row pairs (one-row frame).  Each case: the default
path bit for bit equal to BILD_NO_SPLIT, BILD_NO_ONE_LAUNCH and BILD_NO_STATES and to its own results inside the large batch,
finite, the frames run equal to those of the two-kernel path (which pins the decisions of the looks, not only their sums), and a
random subset of 24 within 1e-8 of the oracle.

The row pair exists for 10 modes only (geometry 23; 12 modes run the listed loop on geometry 22, which has no two-row frame), so
the 3-state and the factored-table models are 20-bead chains whose extra bonds are mirror-symmetric (i, N - 1 - i): the end-to-end
measurement then sees the 10 antisymmetric modes whatever the number of states.  The 12-mode models (24 beads; 12 beads with 9
states) are held to the same equalities on the path they take.
"""
import os

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

TOL = 1e-8
ONE = 'logl_one_kernel<modal>'
N_SMALL = 64    # tasks <= 512 workgroups of the one-launch grid: one task per workgroup, on a row pair
N_LARGE = 6000  # slices of 12 tasks and more per workgroup, all of them chains: more than its 8 row pairs
K1 = 5


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


def chains(rng, n, T, S):
    """ (n, K1) segment lists: three or four switches with gaps of 1 ... 40 frames, anywhere in the trajectory """
    seg_start = np.zeros((n, K1), dtype=np.int32)
    seg_state = np.zeros((n, K1), dtype=np.int32)
    for r in range(n):
        links = 3 + (r & 1)
        gaps = rng.integers(1, 41, size=links - 1)
        span = int(gaps.sum())
        kind = r % 8
        if kind == 2:
            t1 = 1                                   # right at the start
        elif kind == 4:
            t1 = T - 1 - span                        # the last switch on the last frame
        elif kind == 6:
            t1 = T - 1 - int(rng.integers(0, span))  # the chain runs into the trajectory's end
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


def many_state_model(S):
    """ 12 beads, S states of distinct extra bonds (as test_gpu_parity.test_many_states builds them): 12 modes, one R per ordered
    pair of states up to S = 5, the factors Q[s], Q[s]^T (a basis change in two steps) at S = 9 """
    import bild_amd
    N = 12
    pairs = [(a, b) for span in range(2, N) for a in range(N - span) for b in [a + span]]
    loops = [None] + [pairs[i % len(pairs)] + (1.0 + 0.5 * (i // len(pairs)),) for i in range(S - 1)]
    model = bild_amd.MultiStateRouse(N, 1, 3, d=2, looppositions=tuple(loops), localization_error=0.1)
    assert model.nStates == S
    return model


def gap_mask(rng, T):
    """ 5 % of the frames missing, and one gap of 60 ... 120 frames """
    mask = rng.random(T) < 0.05
    start = int(rng.integers(T // 4, T // 2))
    mask[start:start + int(rng.integers(60, 121))] = True
    mask[0] = False
    return np.nonzero(mask)[0]


CASES = {
    'default':         dict(np_modes=10),
    'beads24':         dict(N=24, np_modes=12),
    'three_states':    dict(loops=(None, (0, -1), (5, 14)), T=300, np_modes=10),
    'factored_tables': dict(loops=(None,) + tuple((i, 19 - i) for i in range(6)), T=300, np_modes=10),  # 7 states: Q[s], Q[s]^T
    'factored_12modes': dict(many=9, T=300, np_modes=12),
    'dstar2_missing':  dict(err=[0.1, 0.1, 0.3], missing=True, np_modes=10),
    'three_trajs':     dict(n_traj=3, T=400, np_modes=10),
}


def _case(name):
    import bild_amd
    rng = np.random.default_rng(sorted(CASES).index(name) + 600)
    c = CASES[name]
    T = c.get('T', 500)
    if c.get('many'):
        model = many_state_model(c['many'])
    else:
        model = bild_amd.MultiStateRouse(c.get('N', 20), 1, 5, d=3, localization_error=c.get('err', 0.1),
                                         **(dict(looppositions=c['loops']) if 'loops' in c else {}))
    S = model.nStates
    trajs = [model.trajectory_from_loopingprofile(H.random_profile(rng, T, S, T // 5),
                                                  missing_frames=gap_mask(rng, T) if c.get('missing') else None, rng=rng)
             for _ in range(c.get('n_traj', 1))]
    return rng, model, trajs, S, T, c


@pytest.mark.parametrize('name', sorted(CASES))
def test_chains_on_row_pairs(built_lib, name):
    from oracle import oracle
    from bild_amd import profiles
    rng, model, trajs, S, T, c = _case(name)
    h = model.handle()
    assert h.query(4) == c['np_modes']  # BILD_Q_NP
    pair = c['np_modes'] == 10          # the listed frame loop of 10 modes is geometry 23, the one with row pairs and one launch
    seg_start, seg_state = chains(rng, N_LARGE, T, S)
    n_traj = len(trajs)
    traj_id = (np.arange(N_LARGE) % n_traj).astype(np.int32) if n_traj > 1 else None
    small = (seg_start[:N_SMALL], seg_state[:N_SMALL], None if traj_id is None else traj_id[:N_SMALL])

    def run(batch=small):
        return model.logL_segments(batch[0], batch[1], trajs if n_traj > 1 else trajs[0], batch[2])

    run()  # (tables built by the first evaluation of the set)
    got, kernel, frames = _timed(h, run)
    assert (kernel == ONE) == pair, kernel  # one launch, one task per workgroup: every task on a row pair
    assert np.all(np.isfinite(got))
    two, kernel2, frames2 = _under(['BILD_NO_ONE_LAUNCH'], lambda: _timed(h, run))
    assert kernel2 != ONE
    print(f"{name}: {N_SMALL} chains, frames run {frames} (one launch) / {frames2} (two kernels)")
    assert np.max(np.abs(got - two)) == 0.0, 'BILD_NO_ONE_LAUNCH'
    assert frames == frames2 and frames > 0
    for flag in ('BILD_NO_SPLIT', 'BILD_NO_STATES'):
        other = _under([flag], run)
        assert np.max(np.abs(got - other)) == 0.0, flag
    # the same candidates where the list no longer fits the row pairs: the one-row frame of the same kernel
    large, kernel3, _ = _timed(h, lambda: run((seg_start, seg_state, traj_id)))
    assert (kernel3 == ONE) == pair, kernel3
    assert np.all(np.isfinite(large))
    assert np.max(np.abs(got - large[:N_SMALL])) == 0.0, 'one-row frame'
    pick = rng.choice(N_SMALL, 24, replace=False)
    states = profiles.states_from_segments(seg_start[pick], seg_state[pick], T)
    want = np.empty(len(pick))
    for j in range(n_traj):
        on_j = (pick % n_traj) == j
        want[on_j] = oracle.logl_batch(model.arrays(), model.measurement, model.localization_error, trajs[j][:], states[on_j])
    err = float(np.max(np.abs(got[pick] - want)))
    print(f"{name}: max |logL - oracle| over 24 = {err:.2e}")
    assert err < TOL
