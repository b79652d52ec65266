"""
Wall time of the exact posterior of the looped time under a dwell-time prior (bild_amd.exact_dwell_occupancy, DESIGN.md
section 28) on the data of tools/dwell_bench.py (GenericGaussianModel, T = 1000 frames, S = 2, d = 3, P = [[0.98, 0.02],
[0.05, 0.95]]): one trajectory and a batch of 256, the frames in state 1, and in the same run the route it replaces --
`exact_dwell` with its marginals, `--draws` profiles per trajectory by `exact_dwell_draw` and the host histogram of their
frames in state 1 -- and `exact_dwell` alone.  Each configuration runs once untimed (tables built, code loaded), then `--reps`
times; the best wall time of a synchronous call is reported.  One JSON line per configuration.

    python tools/dwell_occupancy_bench.py [--T 1000] [--batch 256] [--draws 10000] [--reps 5] [--single-only] [--out FILE]

`--single-only` runs the single-trajectory call alone: the part a `rocprofv3 --kernel-trace --stats` run is made of.  The
kernel's terms, for its exp rate: end frame b of a trajectory with S states adds S sum_{c = 1 .. b - 1} (c + 1) terms, one exp
each (alpha(c, ., n) has c + 1 entries, and every one of them feeds one n of end frame b), about S T^3 / 6 in all.
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


def best_of(call, reps):
    res = call()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        res = call()
        times.append(time.perf_counter() - t0)
    return min(times), res


def occupancy_terms(T, S):
    """ the terms (one exp each) of the end frames 1 ... T of one trajectory """
    return sum(S * ((b - 1) * b // 2 + (b - 1)) for b in range(1, T + 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--T', type=int, default=1000)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--draws', type=int, default=10000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--single-only', action='store_true')
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
        print(json.dumps(line), flush=True)
        lines.append(line)

    def histograms(res):
        """ the route that the exact call replaces: draws of every result, then the host histogram per trajectory """
        return [np.bincount(d.occupancy(1), minlength=T + 1) / len(d) for d in bild_amd.exact_dwell_draw(res, a.draws, seed=1)]

    for n in ([1] if a.single_only else sorted({1, a.batch})):
        arg = trajs[0] if n == 1 else trajs[:n]
        base = {'n_traj': n, 'T': T, 'S': 2, 'd': 3}
        model.trajset(arg)
        best, res = best_of(lambda: bild_amd.exact_dwell_occupancy(arg, model, prior, 1), a.reps)
        first = res if n == 1 else res[0]
        lo, hi = first.interval()
        report({'what': 'exact_dwell_occupancy', **base, 'target': [1], 'seconds': best, 'trajectories_per_s': n / best, 'launches': T,
                'terms': n * occupancy_terms(T, 2), 'mean_frames': first.mean(), 'sd_frames': first.var() ** 0.5, 'interval95': [lo, hi],
                'p_above_30_percent': float(first.pmf()[int(0.3 * T) + 1:].sum()), 'sum_pmf_minus_1': float(first.pmf().sum() - 1),
                'log_evidence': first.log_evidence})
        if a.single_only:
            break
        best, res = best_of(lambda: bild_amd.exact_dwell(arg, model, prior), a.reps)
        report({'what': 'exact_dwell', **base, 'marginals': True, 'seconds': best, 'trajectories_per_s': n / best})
        results = [res] if n == 1 else res
        best, hist = best_of(lambda: histograms([bild_amd.exact_dwell(arg, model, prior)] if n == 1 else bild_amd.exact_dwell(arg, model, prior)),
                             a.reps)
        report({'what': 'exact_dwell + draws + histogram', **base, 'draws': a.draws, 'seconds': best, 'trajectories_per_s': n / best,
                'mean_frames': float(np.arange(T + 1) @ hist[0]), 'p_above_30_percent': float(hist[0][int(0.3 * T) + 1:].sum()),
                'n_results': len(results)})
    if a.out:
        with open(a.out, 'w') as f:
            for line in lines:
                f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
