"""
Wall time of the exact window support under a dwell-time prior (bild_amd.exact_dwell_windows through
`ExactDwellResults.map_support`) on the data of tools/dwell_bench.py (GenericGaussianModel, T = 1000
frames, S = 2, d = 3, P = [[0.98, 0.02], [0.05, 0.95]]): one trajectory and a batch of 256.  Timed: `map_support()` (one device
call and one trajectory set a result), the queries that `map_support` asks of the whole batch in ONE `exact_dwell_windows`
call, and in the same run the route they replace -- `exact_dwell`, `--draws` profiles per trajectory by `exact_dwell_draw` and
the host count `ExactDwellDraws.all_in` of every query -- and `exact_dwell` with its marginals alone.  In the batch
`map_support` builds a trajectory set of one trajectory per result (0.7 s of table build each at T = 1000, and the model
caches eight sets) and the draw route's host count takes a good part of a second a trajectory, so there they run once, on the
first `--draw-batch` trajectories, and are reported per trajectory.  Else each configuration runs once untimed (tables built, code
loaded), then `--reps` times; the best wall time of a synchronous call is reported.  One JSON line per configuration.

    python tools/dwell_window_bench.py [--T 1000] [--batch 256] [--draws 10000] [--draw-batch 4] [--reps 5] [--single-only] [--out FILE]

`--single-only` runs `exact_dwell` and `map_support` of one trajectory alone: the part a `rocprofv3 --kernel-trace --stats`
run is made of.  The kernel's terms, one exp each: a query (u, v, G) has |G| (u + 1 + (v - u - 2) / 2) (v - u - 1) terms in its
window chain and |G| v (T - v + 1) in its closure.
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


def map_windows(sup, S, T):
    """ the windows of `map_support`, rebuilt from its result """
    out = []
    for a, b, s in zip(sup.seg_start, sup.seg_end, sup.seg_state):
        out += [(int(a), int(b), (int(s),)), (int(a), int(b), tuple(r for r in range(S) if r != s))]
    for c in sup.switch_frames:
        for r in sup.radii:
            out += [(max(int(c) - r - 1, 0), min(int(c) + r + 1, T), (s,)) for s in range(S)]
    return out


def profile_windows(states, radii, S):
    """ the windows that `map_support` asks about a called profile: one `exact_dwell_windows` call serves those of a batch """
    T = len(states)
    starts = np.concatenate(([0], np.flatnonzero(np.diff(states) != 0) + 1))
    out = []
    for a, b in zip(starts, np.append(starts[1:], T)):
        s = int(states[a])
        out += [(int(a), int(b), (s,)), (int(a), int(b), tuple(r for r in range(S) if r != s))]
    for c in starts[1:]:
        for r in radii:
            out += [(max(int(c) - r - 1, 0), min(int(c) + r + 1, T), (s,)) for s in range(S)]
    return out


def terms(windows, T):
    """ (chain, closure): the terms of the two parts of the kernel over a list of windows """
    chain = sum(len(g) * (v - u - 1) * (2 * (u + 1) + (v - u - 2)) // 2 for u, v, g in windows)
    return chain, sum(len(g) * v * (T - v + 1) for u, v, g in windows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--T', type=int, default=1000)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--draws', type=int, default=10000)
    ap.add_argument('--draw-batch', type=int, default=4)
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

    def count(results, windows):
        """ the route that the exact call replaces: draws of every result, then the host count of every query """
        return [[d.all_in(u, v, g) for u, v, g in w] for d, w in zip(bild_amd.exact_dwell_draw(results, a.draws, seed=1), windows)]

    for n in ([1] if a.single_only else sorted({1, a.batch})):
        xs = trajs[:n]
        base = {'n_traj': n, 'T': T, 'S': 2, 'd': 3}
        model.trajset(xs)
        best, results = best_of(lambda: bild_amd.exact_dwell(xs, model, prior), a.reps)
        report({'what': 'exact_dwell', **base, 'marginals': True, 'seconds': best, 'trajectories_per_s': n / best})
        windows = [profile_windows(np.asarray(r.map_profile[:]), (0, 2, 5), 2) for r in results]
        m = min(n, a.draw_batch)
        if not a.single_only:       # (before `map_support` below, whose one-trajectory sets push the batch's set out of the model's cache)
            queries = sum(len(w) for w in windows)
            chain, closure = (sum(t) for t in zip(*(terms(w, T) for w in windows)))
            best, res = best_of(lambda: bild_amd.exact_dwell_windows(xs, model, prior, windows), a.reps)
            report({'what': 'exact_dwell_windows', **base, 'device_calls': 1, 'queries': queries, 'chain_terms': chain, 'closure_terms': closure,
                    'seconds': best, 'trajectories_per_s': n / best, 'queries_per_s': queries / best})
        best, sups = best_of(lambda: [r.map_support() for r in results[:m]], a.reps if n == 1 else 1)
        assert windows[0] == map_windows(sups[0], 2, T)
        queries = sum(len(w) for w in windows[:m])
        first = sups[0]
        report({'what': 'map_support', **base, 'n_traj': m, 'device_calls': m, 'queries': queries,
                'segments': int(sum(len(s.seg_start) for s in sups)), 'radii': list(first.radii), 'seconds': best, 'trajectories_per_s': m / best,
                'queries_per_s': queries / best, 'p_whole_median': float(np.median(first.p_whole())),
                'p_switch_within_median': np.median(first.p_switch_within, axis=0).tolist(), 'log_evidence': first.log_evidence})
        if a.single_only:
            break
        assert all(np.array_equal(r.log_all[0:2 * len(s.seg_start):2], s.log_whole) for r, s in zip(res, sups))     # the same bits
        best, freq = best_of(lambda: count(bild_amd.exact_dwell(xs[:m], model, prior), windows[:m]), a.reps if n == 1 else 1)
        worst = max(float(np.max(np.abs(np.array(f) - r.p_all()))) for f, r in zip(freq, res))
        report({'what': 'exact_dwell + draws + count', **base, 'n_traj': m, 'draws': a.draws, 'queries': sum(len(w) for w in windows[:m]),
                'seconds': best, 'trajectories_per_s': m / best, 'largest_deviation_from_exact': worst})
    if a.out:
        with open(a.out, 'w') as f:
            for line in lines:
                f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
