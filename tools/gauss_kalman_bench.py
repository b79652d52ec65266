"""
Wall time of GenericGaussianModel.kalman and kalman_mixture (csrc/gauss_kalman.hip): S = 2, d = 3 (ss_order 0, 1, 0),
T = 1000, candidates with k = 4 switches spread over 10 trajectories, gap-free and with 10 % missing frames, next to
logL_sensitivities at P = 0 on the same batch (tools/gauss_fit_bench.py's setting); the smoothed track alone and every
output; the NumPy oracle (tests/gauss_kalman_oracle.py) on a few candidates, one host core.

    python tools/gauss_kalman_bench.py [--n 10000] [--reps 3] [--oracle 2] [--missing 0 0.1]
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
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from gauss_fit_bench import N_TRAJ, T, candidates, family  # noqa: E402


def timed(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=10000)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--oracle', type=int, default=2)
    ap.add_argument('--missing', type=float, nargs='+', default=[0.0, 0.1])
    a = ap.parse_args()
    import bild_amd
    import gauss_kalman_oracle as GK

    rng = np.random.default_rng(0)
    model = bild_amd.GenericGaussianModel(family(1.0, 0.5))
    out = {}
    for miss in a.missing:
        tag = f'miss{miss:g}'
        truth = [np.full(T, rng.integers(2)) for _ in range(N_TRAJ)]
        trajs = [t[:] for t in model.trajectories_from_loopingprofiles(truth, missing_frames=miss or None, seed=1)]
        ss, st = candidates(rng, a.n, 4)
        tid = (np.arange(a.n) % N_TRAJ).astype(np.int32)
        lw = rng.normal(size=a.n)
        out[f'{tag}_sens_P0_s'] = timed(lambda: model.logL_sensitivities((ss, st), trajs, traj_id=tid, fisher=False), a.reps)
        out[f'{tag}_smooth_s'] = timed(lambda: model.kalman((ss, st), trajs, traj_id=tid), a.reps)
        out[f'{tag}_all_s'] = timed(lambda: model.kalman((ss, st), trajs, traj_id=tid,
                                                         outputs=('terms', 'pred', 'smooth', 'innov')), a.reps)
        out[f'{tag}_mixture_s'] = timed(lambda: model.kalman_mixture((ss, st), trajs, lw, traj_id=tid), a.reps)
        out[f'{tag}_output_bytes_smooth'] = 2 * a.n * T * model.d * 8
        print(json.dumps({k: v for k, v in out.items() if k.startswith(tag)}), flush=True)

        t0 = time.perf_counter()
        for r in range(a.oracle):
            states = np.zeros(T, dtype=int)
            for q in range(ss.shape[1]):
                states[ss[r, q]:] = st[r, q]
            GK.kalman(model.msd, model.msd_inf, model.mean, model.ss_order, trajs[tid[r]], states, cholesky=True)
        out[f'{tag}_oracle_s_per_cand'] = (time.perf_counter() - t0) / max(a.oracle, 1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
