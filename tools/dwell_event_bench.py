"""
Wall time of the exact switch counts and first-contact times under a dwell-time prior (bild_amd.exact_dwell_switch_counts,
exact_dwell_first_contact) on the data of tools/dwell_bench.py (GenericGaussianModel, T = 1000 frames,
S = 2, d = 3, P = [[0.98, 0.02], [0.05, 0.95]]): one trajectory and a batch of 256, the switch counts at `--kmax` and at the
complete k_max, the first contact with state 1, and in the same run the route they replace -- `exact_dwell` with its
marginals, `--draws` profiles per trajectory by `exact_dwell_draw` and the two host histograms -- and `exact_dwell` alone.
Each configuration runs once untimed (tables built, code loaded), then `--reps` times; the best wall time of a synchronous
call is reported.  One JSON line per configuration.

    python tools/dwell_event_bench.py [--T 1000] [--kmax 127] [--batch 256] [--draws 10000] [--reps 5] [--single-only] [--out FILE]

`--single-only` runs the single-trajectory switch counts (complete k_max) and first contact alone: the part a
`rocprofv3 --kernel-trace --stats` run is made of.  The level kernel's terms, for its exp rate: level n of a trajectory of T
frames with S states adds S (T - n) (T - n + 1) / 2 terms, one exp each.
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


def level_terms(T, S, k_max):
    """ the terms (one exp each) of the levels 1 ... k_max of one trajectory """
    return sum(S * (T - n) * (T - n + 1) // 2 for n in range(1, min(k_max, T - 1) + 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--T', type=int, default=1000)
    ap.add_argument('--kmax', type=int, default=127)
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
        """ the route that the exact calls replace: draws of every result, then the two host histograms per trajectory """
        out = []
        for d in bild_amd.exact_dwell_draw(res, a.draws, seed=1):
            first = d.first_contact(1)
            out.append((np.bincount(d.n_switches, minlength=T) / len(d), np.bincount(first[first >= 0], minlength=T) / len(d),
                        float(np.mean(first < 0))))
        return out

    for n in ([1] if a.single_only else sorted({1, a.batch})):
        arg = trajs[0] if n == 1 else trajs[:n]
        base = {'n_traj': n, 'T': T, 'S': 2, 'd': 3}
        model.trajset(arg)
        for k_max in ([None] if a.single_only else [a.kmax, None]):
            best, res = best_of(lambda: bild_amd.exact_dwell_switch_counts(arg, model, prior, k_max=k_max), a.reps)
            first = res if n == 1 else res[0]
            levels = len(first.log_count)
            report({'what': 'exact_dwell_switch_counts', **base, 'k_max': levels - 1, 'seconds': best, 'trajectories_per_s': n / best,
                    'levels': levels, 'level_terms': n * level_terms(T, 2, levels - 1), 'mean_switches': first.mean(),
                    'mode_switches': int(np.argmax(first.pmf())), 'log_tail': first.log_tail, 'log_evidence': first.log_evidence})
        best, res = best_of(lambda: bild_amd.exact_dwell_first_contact(arg, model, prior, 1), a.reps)
        first = res if n == 1 else res[0]
        report({'what': 'exact_dwell_first_contact', **base, 'target': [1], 'seconds': best, 'trajectories_per_s': n / best,
                'log_never': first.log_never, 'median_first_frame': int(np.searchsorted(first.cdf(), 0.5)), 'log_evidence': first.log_evidence})
        if a.single_only:
            break
        best, res = best_of(lambda: bild_amd.exact_dwell(arg, model, prior), a.reps)
        report({'what': 'exact_dwell', **base, 'marginals': True, 'seconds': best, 'trajectories_per_s': n / best})
        results = [res] if n == 1 else res
        best, hist = best_of(lambda: histograms([bild_amd.exact_dwell(arg, model, prior)] if n == 1 else bild_amd.exact_dwell(arg, model, prior)),
                             a.reps)
        report({'what': 'exact_dwell + draws + histograms', **base, 'draws': a.draws, 'seconds': best, 'trajectories_per_s': n / best,
                'mean_switches': float(np.arange(T) @ hist[0][0]), 'never_share': hist[0][2], 'n_results': len(results)})
    if a.out:
        with open(a.out, 'w') as f:
            for line in lines:
                f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
