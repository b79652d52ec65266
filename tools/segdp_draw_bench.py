"""
Wall time of exact posterior draws (bild_amd.exact_draw) on the GenericGaussianModel trajectories of
tools/segdp_bench.py (T = 1000 frames, S = 2, d = 3, k_max = 20): 10 000 draws at k = 20 and at `best_k` on one trajectory,
host to host with the tables built, next to the yardstick `exact_sample(marginals=True)` on the same trajectory (the draws
have to take no longer than that call), and 1 000 draws on each trajectory of a batch of 256.  Each configuration runs once
untimed, then `--reps` times; the best and the median wall time of a synchronous call are reported.  `--oracle` adds the
NumPy oracle tests/segment_draw_oracle.py on one host core (T = 200, k_max = 5: its backward table is a Python loop).
One JSON line per configuration.

    python tools/segdp_draw_bench.py [--T 1000] [--kmax 20] [--draws 10000] [--batch 256] [--batch-draws 1000] [--reps 7]
                                     [--oracle] [--out FILE]
"""
import argparse
import json
import os
import statistics
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
    return min(times), statistics.median(times), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--T', type=int, default=1000)
    ap.add_argument('--kmax', type=int, default=20)
    ap.add_argument('--draws', type=int, default=10000)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--batch-draws', type=int, default=1000)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--oracle', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    T = a.T
    lags = np.arange(T + 1, dtype=float)
    model = bild_amd.GenericGaussianModel([[(0.8 * lags ** 0.6 + np.where(lags > 0, 0.2, 0.0), m, 1)] * 3 for m in (0.0, 0.3)])
    trajs = [np.cumsum(rng.normal(size=(T, 3)), axis=0) for _ in range(max(a.batch, 1))]
    lines = []

    def report(line):
        print(json.dumps(line), flush=True)
        lines.append(line)

    shape = {'T': T, 'S': 2, 'd': 3, 'k_max': a.kmax}
    best, med, r = timed(lambda: bild_amd.exact_sample(trajs[0], model, k_max=a.kmax, marginals=True), a.reps)
    yardstick = best
    report({'what': 'exact_sample', 'n_traj': 1, **shape, 'marginals': True, 'seconds': best, 'median_seconds': med, 'best_k': r.best_k()})
    for label, k in (('k_max', a.kmax), ('best_k', r.best_k())):
        best, med, d = timed(lambda: r.draw(a.draws, k=k, seed=1), a.reps)
        report({'what': 'exact_draw', 'n_traj': 1, **shape, 'k': k, 'at': label, 'draws': a.draws, 'seconds': best, 'median_seconds': med,
                'draws_per_s': a.draws / best, 'yardstick_seconds': yardstick, 'no_longer_than_yardstick': best <= yardstick,
                'mean_logL': float(np.mean(d.logL))})
    if a.batch > 1:
        res = bild_amd.exact_sample(trajs[:a.batch], model, k_max=a.kmax, marginals=False)
        best, med, ds = timed(lambda: bild_amd.exact_draw(res, a.batch_draws, seed=2), a.reps)
        n = a.batch * a.batch_draws
        report({'what': 'exact_draw', 'n_traj': a.batch, **shape, 'at': 'best_k', 'draws': n, 'seconds': best, 'median_seconds': med,
                'draws_per_s': n / best, 'best_k_histogram': np.bincount([int(d.k[0]) for d in ds]).tolist()})
    if a.oracle:
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
        import segment_cases as C
        import segment_draw_oracle as DO
        import segment_oracle as SO
        To, ko, no = 200, 5, 2000
        small = bild_amd.GenericGaussianModel([[(0.8 * lags[:To + 1] ** 0.6 + np.where(lags[:To + 1] > 0, 0.2, 0.0), m, 1)] * 3
                                               for m in (0.0, 0.3)])
        x = trajs[0][:To]
        t0 = time.perf_counter()
        W, F = C.tables(small, x)
        G = SO.backward(W, small.transitions, ko)
        tables = time.perf_counter() - t0
        t0 = time.perf_counter()
        DO.draws(W, F, G, small.transitions, np.full(no, ko), rng.random((no, 2 * ko)))
        per_draw = (time.perf_counter() - t0) / no
        report({'what': 'numpy_oracle', 'T': To, 'S': 2, 'd': 3, 'k': ko, 'draws': no, 'table_seconds': tables, 'seconds_per_draw': per_draw})
    if a.out:
        with open(a.out, 'w') as f:
            for line in lines:
                f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
