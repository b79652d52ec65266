#!/usr/bin/env python3
"""
Trajectories per second of the GenericGaussianModel generator, one JSON line per trajectory length: n = 10 000
trajectories of T = 200, 1000 and 2048 frames, S = 2 (state 0 ss_order 0, state 1 ss_order 1), d = 3, four switches each,
for
  cpu     the loop of GenericGaussianModel.trajectory_from_loopingprofile, timed on --cpu-n trajectories and scaled up,
  replay  trajectories_from_loopingprofiles(rng=...): host-drawn normals, arithmetic on the GPU,
  device  trajectories_from_loopingprofiles(seed=...): normals drawn on the GPU.
Host clock around whole calls, which end in a device synchronise; the device-to-host copy and the Trajectory objects are
included.  `first_call_s` is a fresh model's first call on 16 trajectories of the full length, which builds the S d
Toeplitz factors; the timed calls come after it and reuse them.  Needs the GPU.

    python tools/gauss_sim_bench.py [--n 10000] [--T 200 1000 2048] [--modes cpu replay device]

Kernel time: a run of its own under the profiler, device mode only, e.g.
    rocprofv3 --kernel-trace --stats -d OUT -o gsim -- python tools/gauss_sim_bench.py --modes device
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def profiles(rng, n, T, S, switches=4):
    out = np.empty((n, T), dtype=np.int64)
    for i in range(n):
        st = np.full(T, rng.integers(S))
        for t in np.sort(rng.choice(np.arange(1, T), size=switches, replace=False)):
            st[t:] = (st[t - 1] + 1) % S
        out[i] = st
    return out


def make_model(L=2048, d=3):
    import bild_amd
    t = np.arange(L, dtype=np.float64)
    exp = 2 * 1.0 * (1 - np.exp(-t / 10.0)) + 2 * 0.3 ** 2
    exp[0] = 0.0
    exp = np.append(exp, 2 * 1.0 + 2 * 0.3 ** 2)
    pw = 0.5 * t ** 0.8 + 2 * 0.3 ** 2
    pw[0] = 0.0
    return bild_amd.GenericGaussianModel([[(exp, 0.0, 0)] * d, [(pw, 0.1, 1)] * d])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=10000)
    ap.add_argument('--T', type=int, nargs='+', default=[200, 1000, 2048])
    ap.add_argument('--cpu-n', type=int, default=100)
    ap.add_argument('--modes', nargs='+', default=['cpu', 'replay', 'device'])
    args = ap.parse_args()

    import bild_amd
    S, d = 2, 3
    for T in args.T:
        prof = profiles(np.random.default_rng(T), args.n, T, S)
        res = dict(n=args.n, T=T, S=S, d=d)
        if 'cpu' in args.modes:
            model = make_model()
            rng = np.random.default_rng(1)
            t0 = time.perf_counter()
            for p in prof[:args.cpu_n]:
                model.trajectory_from_loopingprofile(bild_amd.Loopingprofile(p), rng=rng)
            dt = time.perf_counter() - t0
            res['cpu_ms_per_traj'] = 1e3 * dt / args.cpu_n
            res['cpu_traj_per_s'] = args.cpu_n / dt
        for mode in ('replay', 'device'):
            if mode not in args.modes:
                continue
            model = make_model()
            kw = (lambda: dict(rng=np.random.default_rng(2))) if mode == 'replay' else (lambda: dict(seed=2))
            t0 = time.perf_counter()
            model.trajectories_from_loopingprofiles(prof[:16], **kw())     # first call: the factors
            res[f'{mode}_first_call_s'] = time.perf_counter() - t0
            t0 = time.perf_counter()
            trajs = model.trajectories_from_loopingprofiles(prof, **kw())
            dt = time.perf_counter() - t0
            assert len(trajs) == args.n and np.all(np.isfinite(trajs[-1][:]))
            res[f'{mode}_s'] = dt
            res[f'{mode}_traj_per_s'] = args.n / dt
            if 'cpu_traj_per_s' in res:
                res[f'{mode}_speedup_vs_cpu'] = res[f'{mode}_traj_per_s'] / res['cpu_traj_per_s']
        print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
