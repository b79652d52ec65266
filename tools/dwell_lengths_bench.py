"""
Wall time of the expected segment-length counts under a dwell-time prior (bild_amd.exact_dwell_lengths)
on the data of tools/dwell_bench.py (GenericGaussianModel, T = 1000 frames, S = 2, d = 3): one trajectory and a batch of 256,
next to `exact_dwell(marginals=True)` on the same data in the same session; the two fits of tests/test_gpu_dwell_lengths.py
(`fit_markov_prior` and `fit_dwell_prior` with one bin on the Markov data; the Markov fit and the hazard fit on the
non-geometric data) with their device calls and the table build apart; and the distance of `lifetime_pmf` from the histogram of
the completed lifetimes of `--draws` exact draws on one trajectory.  Each timed call runs once untimed (tables built, code
loaded), then `--reps` times; the best wall time of a synchronous call is reported.  One JSON line per configuration.

    python tools/dwell_lengths_bench.py [--T 1000] [--batch 256] [--reps 5] [--draws 10000] [--single-only] [--out FILE]

`--single-only` runs the single-trajectory `exact_dwell_lengths` alone: the part a `rocprofv3 --kernel-trace --stats` run is
made of.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np  # noqa: E402

import bild_amd  # noqa: E402
import dwell_length_cases as DLC  # noqa: E402
from dwell_bench import best_of  # noqa: E402


def timed(call):
    t0 = time.perf_counter()
    res = call()
    return time.perf_counter() - t0, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--T', type=int, default=1000)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--draws', type=int, default=10000)
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

    for n in ([1] if a.single_only else sorted({1, a.batch})):
        arg = trajs[0] if n == 1 else trajs[:n]
        build, _ = timed(lambda: model.trajset(arg))
        best, res = best_of(lambda: bild_amd.exact_dwell_lengths(arg, model, prior), a.reps)
        first = res if n == 1 else res[0]
        report({'what': 'exact_dwell_lengths', 'n_traj': n, 'T': T, 'S': 2, 'd': 3, 'seconds': best, 'trajectories_per_s': n / best,
                'table_build_seconds': build, 'log_evidence': first.log_evidence,
                'expected_completed_segments': first.expected_dwell.sum(axis=1).tolist()})
        if a.single_only:
            break
        best, res = best_of(lambda: bild_amd.exact_dwell(arg, model, prior, marginals=True), a.reps)
        report({'what': 'exact_dwell', 'n_traj': n, 'T': T, 'S': 2, 'd': 3, 'marginals': True, 'seconds': best,
                'trajectories_per_s': n / best, 'log_evidence': (res if n == 1 else res[0]).log_evidence})
    if a.single_only:
        return

    # lifetime_pmf against the histogram of exact draws: a plausibility figure, the histogram carries the sampling noise
    x = trajs[0]
    counts = bild_amd.exact_dwell_lengths(x, model, prior)
    draws = bild_amd.exact_dwell(x, model, prior).draw(a.draws, seed=1)
    for s in range(2):
        lifetimes = np.asarray(draws.dwell_lengths(s), dtype=int)
        hist = np.bincount(lifetimes, minlength=T + 1)[1:] / max(len(lifetimes), 1)
        pmf = counts.lifetime_pmf(s)
        report({'what': 'lifetime_pmf against draws', 'state': s, 'draws': a.draws, 'completed_segments_drawn': int(len(lifetimes)),
                'expected_per_draw': float(counts.expected_dwell[s].sum()), 'drawn_per_draw': len(lifetimes) / a.draws,
                'max_abs_deviation': float(np.max(np.abs(hist - pmf))), 'total_variation': float(0.5 * np.sum(np.abs(hist - pmf))),
                'mean_lifetime_exact': float(pmf @ np.arange(1, T + 1)), 'mean_lifetime_drawn': float(lifetimes.mean())})

    # the fits of tests/test_gpu_dwell_lengths.py
    fmodel, ftrajs = DLC.markov_data()
    build, _ = timed(lambda: fmodel.trajset(ftrajs))
    seconds, markov = timed(lambda: bild_amd.fit_markov_prior(ftrajs, fmodel, start=DLC.MARKOV_START))
    report({'what': 'fit_markov_prior', 'data': 'markov', 'n_traj': len(ftrajs), 'T': 200, 'device_calls': markov.n_iter,
            'converged': bool(markov.converged), 'seconds': seconds, 'seconds_per_call': seconds / markov.n_iter,
            'table_build_seconds': build, 'P': markov.P.tolist(), 'log_evidence_last': float(markov.log_evidence[-1])})
    leave = 1 - np.diag(DLC.MARKOV_START)
    start = (leave[:, None], (DLC.MARKOV_START - np.diag(np.diag(DLC.MARKOV_START))) / leave[:, None], np.array([0.5, 0.5]))
    seconds, fit = timed(lambda: bild_amd.fit_dwell_prior(ftrajs, fmodel, edges=[1], start=start))
    report({'what': 'fit_dwell_prior', 'data': 'markov', 'edges': [1], 'n_traj': len(ftrajs), 'T': 200, 'device_calls': fit.n_iter,
            'converged': bool(fit.converged), 'seconds': seconds, 'seconds_per_call': seconds / fit.n_iter, 'hazard': fit.hazard.tolist(),
            'log_evidence_last': float(fit.log_evidence[-1])})

    hmodel, htrajs, _ = DLC.hazard_data()
    build, _ = timed(lambda: hmodel.trajset(htrajs))
    seconds, markov = timed(lambda: bild_amd.fit_markov_prior(htrajs, hmodel, start=DLC.MARKOV_START))
    report({'what': 'fit_markov_prior', 'data': 'hazard', 'n_traj': len(htrajs), 'T': 200, 'device_calls': markov.n_iter,
            'converged': bool(markov.converged), 'seconds': seconds, 'seconds_per_call': seconds / markov.n_iter,
            'table_build_seconds': build, 'P': markov.P.tolist(), 'log_evidence_last': float(markov.log_evidence[-1])})
    seconds, fit = timed(lambda: bild_amd.fit_dwell_prior(htrajs, hmodel, edges=DLC.HAZARD_EDGES, start=markov))
    truth = DLC.hazard_prior(DLC.HAZARD_EDGES, DLC.HAZARD_TRUE, 200)
    at_truth = float(sum(r.log_evidence for r in bild_amd.exact_dwell(htrajs, hmodel, truth, marginals=False)))
    report({'what': 'fit_dwell_prior', 'data': 'hazard', 'edges': DLC.HAZARD_EDGES.tolist(), 'n_traj': len(htrajs), 'T': 200,
            'device_calls': fit.n_iter, 'converged': bool(fit.converged), 'seconds': seconds, 'seconds_per_call': seconds / fit.n_iter,
            'hazard': fit.hazard.tolist(), 'hazard_true': DLC.HAZARD_TRUE.tolist(), 'supported': fit.supported.tolist(),
            'init': fit.init.tolist(), 'log_evidence_first': float(fit.log_evidence[0]), 'log_evidence_last': float(fit.log_evidence[-1]),
            'log_evidence_at_truth': at_truth})
    if a.out:
        with open(a.out, 'w') as f:
            for line in lines:
                f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
