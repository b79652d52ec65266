#!/usr/bin/env python3
"""
Trajectories per second of the Rouse generator, one JSON line per chain length: n = 10 000 trajectories of T = 1000
frames, S = 2, d = 3, at N = 20 and N = 64, for
  cpu     the loop of MultiStateRouse.trajectory_from_loopingprofile, timed on --cpu-n trajectories and scaled up,
  replay  trajectories_from_loopingprofiles(rng=...): host-drawn normals, arithmetic on the GPU,
  device  trajectories_from_loopingprofiles(seed=...): normals drawn on the GPU.
Host clock around whole calls, which end in a device synchronise; the device-to-host copy and the Trajectory objects are
included.  Each GPU mode is warmed up once on a small batch first.  Needs the GPU.

    python tools/sim_bench.py [--n 10000] [--T 1000] [--N 20 64] [--modes cpu replay device]

Kernel time: a run of its own under the profiler, device mode only, e.g.
    rocprofv3 --kernel-trace --stats -d OUT -o sim -- python tools/sim_bench.py --modes device
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=10000)
    ap.add_argument('--T', type=int, default=1000)
    ap.add_argument('--N', type=int, nargs='+', default=[20, 64])
    ap.add_argument('--cpu-n', type=int, default=100)
    ap.add_argument('--modes', nargs='+', default=['cpu', 'replay', 'device'])
    args = ap.parse_args()

    import bild_amd
    S, d = 2, 3
    for N in args.N:
        model = bild_amd.MultiStateRouse(N, 1.0, 1.0, d=d, looppositions=(None, (0, -1)), localization_error=0.1)
        prof = profiles(np.random.default_rng(N), args.n, args.T, S)
        res = dict(N=N, n=args.n, T=args.T, S=S, d=d)
        if 'cpu' in args.modes:
            rng = np.random.default_rng(1)
            t0 = time.perf_counter()
            for p in prof[:args.cpu_n]:
                model.trajectory_from_loopingprofile(p, rng=rng)
            dt = time.perf_counter() - t0
            res['cpu_ms_per_traj'] = 1e3 * dt / args.cpu_n
            res['cpu_traj_per_s'] = args.cpu_n / dt
        for mode in ('replay', 'device'):
            if mode not in args.modes:
                continue
            kw = (lambda: dict(rng=np.random.default_rng(2))) if mode == 'replay' else (lambda: dict(seed=2))
            model.trajectories_from_loopingprofiles(prof[:16], **kw())     # warm-up
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
