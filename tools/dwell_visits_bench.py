"""
Wall time of the exact posterior of the number of visits to a set of states under a dwell-time prior
(bild_amd.exact_dwell_visits) on the data of tools/dwell_bench.py (GenericGaussianModel, T = 1000
frames, S = 2, d = 3, P = [[0.98, 0.02], [0.05, 0.95]]): one trajectory and a batch of 256, the visits to state 1, at the
complete n_max and at `--n-max`, and in the same run `exact_dwell_occupancy` on the same data (the sibling with the same launch
structure), the route the call replaces -- `exact_dwell` with its marginals, `--draws` profiles per trajectory by
`exact_dwell_draw` and the host histogram of their visits to state 1 -- and `exact_dwell` alone.  Each configuration runs once
untimed (tables built, code loaded), then `--reps` times; the best wall time of a synchronous call is reported, with the
spread of the repetitions.  One JSON line per configuration.

    python tools/dwell_visits_bench.py [--T 1000] [--batch 256] [--n-max 127] [--draws 10000] [--reps 5] [--single-only] [--out FILE]

`--single-only` runs the single-trajectory calls of `exact_dwell_visits` alone: the part a `rocprofv3 --kernel-trace --stats`
run is made of.  The kernel's terms, for its exp rate: end frame b of a trajectory with S states adds, for every switch frame
c < b, the rows n = 0 ... min(n_max, (c + 1) // 2 + 1) that end frame c wrote, one exp each: about S T^3 / 12 in all at the
complete n_max, half of the occupancy kernel's.
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
    return min(times), {'seconds_median': float(np.median(times)), 'seconds_max': max(times), 'reps': reps}, res


def visit_terms(T, S, n_max):
    """ the terms (one exp each) of the end frames 1 ... T of one trajectory """
    rows = np.minimum(n_max, (np.arange(T) + 1) // 2 + 1) + 1      # of switch frame c, at [c]
    below = np.concatenate(([0], np.cumsum(rows[1:])))             # sum over c = 1 .. b - 1, at [b - 1]
    return int(S * below[:T].sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--T', type=int, default=1000)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--n-max', type=int, default=127)
    ap.add_argument('--draws', type=int, default=10000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--single-only', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    T = a.T
    top = (T + 1) // 2
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
        return [np.bincount(d.visits(1), minlength=top + 1) / len(d) for d in bild_amd.exact_dwell_draw(res, a.draws, seed=1)]

    for n in ([1] if a.single_only else sorted({1, a.batch})):
        arg = trajs[0] if n == 1 else trajs[:n]
        base = {'n_traj': n, 'T': T, 'S': 2, 'd': 3}
        model.trajset(arg)
        for n_max in (None, a.n_max):
            best, spread, res = best_of(lambda: bild_amd.exact_dwell_visits(arg, model, prior, 1, n_max=n_max), a.reps)
            first = res if n == 1 else res[0]
            rows = top if n_max is None else n_max
            lo, hi = first.interval()
            report({'what': 'exact_dwell_visits', **base, 'target': [1], 'n_max': rows, 'complete': n_max is None, 'seconds': best, **spread,
                    'trajectories_per_s': n / best, 'launches': T, 'terms': n * visit_terms(T, 2, rows), 'mean_visits': first.mean(),
                    'sd_visits': first.var() ** 0.5, 'interval95': [lo, hi], 'p_never': float(first.pmf()[0]),
                    'sum_pmf_minus_1': float(first.pmf().sum() - 1), 'log_tail': first.log_tail, 'log_evidence': first.log_evidence})
        if a.single_only:
            break
        best, spread, res = best_of(lambda: bild_amd.exact_dwell_occupancy(arg, model, prior, 1), a.reps)
        report({'what': 'exact_dwell_occupancy', **base, 'target': [1], 'seconds': best, **spread, 'trajectories_per_s': n / best, 'launches': T})
        best, spread, res = best_of(lambda: bild_amd.exact_dwell(arg, model, prior), a.reps)
        report({'what': 'exact_dwell', **base, 'marginals': True, 'seconds': best, **spread, 'trajectories_per_s': n / best})
        results = [res] if n == 1 else res
        best, spread, hist = best_of(lambda: histograms([bild_amd.exact_dwell(arg, model, prior)] if n == 1 else bild_amd.exact_dwell(arg, model, prior)),
                                     a.reps)
        report({'what': 'exact_dwell + draws + histogram', **base, 'draws': a.draws, 'seconds': best, **spread, 'trajectories_per_s': n / best,
                'mean_visits': float(np.arange(top + 1) @ hist[0]), 'p_never': float(hist[0][0]), 'n_results': len(results)})
    if a.out:
        with open(a.out, 'w') as f:
            for line in lines:
                f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
