"""
Wall time of the exact posterior draws under a dwell-time prior (bild_amd.exact_dwell_draw) on the
data of tools/dwell_bench.py (GenericGaussianModel, T = 1000 frames, S = 2, d = 3, prior P = [[0.98, 0.02], [0.05, 0.95]]):
the yardstick `exact_dwell(marginals=True)` on one trajectory, 10 000 draws on that trajectory, and 256 trajectories x 1 000
draws in one call, all host to host with the tables built.  Each configuration runs once untimed, then `--reps` times; the
best and the median wall time of a synchronous call are reported.  One JSON line per configuration.

    python tools/dwell_draw_bench.py [--T 1000] [--draws 10000] [--batch 256] [--batch-draws 1000] [--reps 5]
                                     [--single-only | --yardstick-only] [--out profiles/dwell_draw_bench.jsonl]

`--single-only` runs the draws on one trajectory alone: the part a `rocprofv3 --kernel-trace --stats` run is made of.
`--yardstick-only` runs `exact_dwell(marginals=True)` alone (with BILD_AMD_LIB: on another build of the library).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import bild_amd  # noqa: E402


def timed(call, reps):
    res = call()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        res = call()
        times.append(time.perf_counter() - t0)
    return min(times), float(np.median(times)), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--T', type=int, default=1000)
    ap.add_argument('--draws', type=int, default=10000)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--batch-draws', type=int, default=1000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--single-only', action='store_true')
    ap.add_argument('--yardstick-only', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    T = a.T
    lags = np.arange(T + 1, dtype=float)
    # (the model, the trajectories and the prior of tools/dwell_bench.py)
    model = bild_amd.GenericGaussianModel([[(0.8 * lags ** 0.6 + np.where(lags > 0, 0.2, 0.0), m, 1)] * 3 for m in (0.0, 0.3)])
    trajs = [np.cumsum(rng.normal(size=(T, 3)), axis=0) for _ in range(a.batch)]
    prior = bild_amd.DwellPrior.markov([[0.98, 0.02], [0.05, 0.95]], [0.5, 0.5], n=T)
    lines = []

    def report(line):
        line.update({'T': T, 'S': 2, 'd': 3, 'library': os.environ.get('BILD_AMD_LIB') or 'default'})
        print(json.dumps(line), flush=True)
        lines.append(line)

    model.trajset(trajs[0])
    if not a.single_only:
        best, median, r = timed(lambda: bild_amd.exact_dwell(trajs[0], model, prior, marginals=True), a.reps)
        report({'what': 'exact_dwell', 'n_traj': 1, 'marginals': True, 'seconds': best, 'median_seconds': median,
                'log_evidence': r.log_evidence})
    else:
        r = bild_amd.exact_dwell(trajs[0], model, prior, marginals=False)
    if not a.yardstick_only:
        best, median, d = timed(lambda: r.draw(a.draws, seed=1), a.reps)
        report({'what': 'exact_dwell_draw', 'n_traj': 1, 'draws': a.draws, 'seconds': best, 'median_seconds': median,
                'draws_per_s': a.draws / best, 'mean_switches': float(np.mean(d.n_switches)), 'max_switches': int(np.max(d.n_switches))})
    if not a.single_only and not a.yardstick_only:
        model.trajset(trajs)
        res = bild_amd.exact_dwell(trajs, model, prior, marginals=False)
        best, median, ds = timed(lambda: bild_amd.exact_dwell_draw(res, a.batch_draws, seed=1), a.reps)
        report({'what': 'exact_dwell_draw', 'n_traj': a.batch, 'draws': a.batch * a.batch_draws, 'seconds': best, 'median_seconds': median,
                'draws_per_s': a.batch * a.batch_draws / best, 'mean_switches': float(np.mean([np.mean(d.n_switches) for d in ds]))})
    if a.out:
        with open(a.out, 'w') as f:
            for line in lines:
                f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
