"""
Throughput of GenericGaussianModel.logL_sensitivities (csrc/gauss_sens.hip) and wall time of GenericGaussianModel.fit:
S = 2, d = 3 (ss_order 0, 1, 0), T = 1000, candidates with k = 4 switches spread over 10 trajectories, gap-free and with
10 % missing frames, at P = 0, 1 and 3 parameters, next to the table build of the same trajectories (bild_gauss_trajset);
a fit of two parameters on 256 simulated trajectories from a start 2x off; the NumPy tangent oracle
(tests/gauss_sensitivity_oracle.py) at P = 3 on a few candidates, one host core.

    python tools/gauss_fit_bench.py [--n 10000] [--fit 256] [--oracle 2] [--missing 0 0.1]
"""
import argparse
import json
import os
import sys
import time

for _v in ('OMP_NUM_THREADS', 'OPENBLAS_NUM_THREADS', 'MKL_NUM_THREADS'):     # the oracle on one host core
    os.environ[_v] = '1'

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

T, N_TRAJ = 1000, 10


def family(A, G):
    from gauss_sim_cases import msd_exp, msd_pow
    return [[(msd_exp(A, 10.0, 0.3, T), 0.1, 0), (msd_pow(G, 0.8, 0.3, T), 0.05, 1), (msd_exp(0.5 * A, 20.0, 0.3, T), 0.0, 0)],
            [(msd_exp(2 * A, 4.0, 0.3, T), -0.1, 0), (msd_pow(0.5 * G, 1.2, 0.3, T), 0.0, 1), (msd_exp(A, 8.0, 0.3, T), 0.2, 0)]]


def candidates(rng, n, k, S=2):
    seg_start = np.zeros((n, k + 1), dtype=np.int32)
    seg_start[:, 1:] = np.sort(rng.integers(1, T, size=(n, k)), axis=1)
    seg_state = rng.integers(S, size=(n, k + 1)).astype(np.int32)
    return seg_start, seg_state


def derivs(model, P):
    """ P of: a scale of state 0's MSDs, of state 1's, a shift of all means """
    S, d, L = model.msd.shape
    dm = dict(dmsd=np.zeros((P, S, d, L)), dmsd_inf=np.zeros((P, S, d)), dmean=np.zeros((P, S, d)))
    for p in range(P):
        if p < S:
            dm['dmsd'][p, p], dm['dmsd_inf'][p, p] = model.msd[p], model.msd_inf[p]
        else:
            dm['dmean'][p] = 1.0
    return dm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=10000)
    ap.add_argument('--fit', type=int, default=256)
    ap.add_argument('--oracle', type=int, default=2)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--missing', type=float, nargs='+', default=[0.0, 0.1])
    ap.add_argument('--P', type=int, nargs='+', default=[0, 1, 3])
    a = ap.parse_args()
    import bild_amd
    from bild_amd import _lib
    import gauss_sensitivity_oracle as GS

    rng = np.random.default_rng(0)
    model = bild_amd.GenericGaussianModel(family(1.0, 0.5))
    out = {}
    for miss in a.missing:
        tag = f'miss{miss:g}'
        truth = [np.full(T, rng.integers(2)) for _ in range(N_TRAJ)]
        trajs = [t[:] for t in model.trajectories_from_loopingprofiles(truth, missing_frames=miss or None, seed=1)]
        ss, st = candidates(rng, a.n, 4)
        tid = (np.arange(a.n) % N_TRAJ).astype(np.int32)
        t0 = time.perf_counter()
        ts = _lib.GaussTrajSetHandle(model.handle(), trajs)
        out[f'{tag}_tables_wall_s'] = time.perf_counter() - t0
        out[f'{tag}_tables_build_ms'] = ts.info()[1]
        t0 = time.perf_counter()
        _lib.gauss_logl_segments(model.handle(), ts, ss, st, tid)
        out[f'{tag}_walk_s'] = time.perf_counter() - t0
        del ts
        for P in a.P:
            dm = derivs(model, P)
            fn = lambda: model.logL_sensitivities((ss, st), trajs, traj_id=tid, **dm)   # noqa: E731
            fn()
            t0 = time.perf_counter()
            for _ in range(a.reps):
                fn()
            dt = (time.perf_counter() - t0) / a.reps
            out[f'{tag}_P{P}_s'] = dt
            out[f'{tag}_P{P}_cand_per_s'] = a.n / dt
            print(json.dumps({k: v for k, v in out.items() if k.startswith(tag)}), flush=True)

        # the NumPy oracle, P = 3, one host core
        dm = derivs(model, 3)
        t0 = time.perf_counter()
        for r in range(a.oracle):
            states = np.zeros(T, dtype=int)
            for q in range(ss.shape[1]):
                states[ss[r, q]:] = st[r, q]
            GS.sensitivities(model.msd, model.msd_inf, model.mean, model.ss_order, trajs[tid[r]], states, **dm)
        out[f'{tag}_oracle_s_per_cand'] = (time.perf_counter() - t0) / max(a.oracle, 1)

    # fit: simulated trajectories with k = 4 switches, start 2x off
    if a.fit:
        truth = {'A': 1.0, 'G': 0.5}
        profiles = []
        for _ in range(a.fit):
            s = np.zeros(T, dtype=int)
            for t in np.sort(rng.integers(1, T, size=4)):
                s[t:] = 1 - s[t - 1]
            profiles.append(s)
        trajs = model.trajectories_from_loopingprofiles(profiles, seed=2)
        t0 = time.perf_counter()
        res = bild_amd.GenericGaussianModel.fit(trajs, profiles, family, {k: 2 * v for k, v in truth.items()})
        out['fit_s'] = time.perf_counter() - t0
        out['fit_device_calls'] = res.n_iter
        out['fit_converged'] = res.converged
        out['fit_params'] = res.params
        out['fit_se'] = res.se
    print(json.dumps(out))


if __name__ == '__main__':
    main()
