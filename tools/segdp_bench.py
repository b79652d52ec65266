"""
Wall time of the exact evidence of every k by the segment recursion (bild_amd.exact_sample) on
GenericGaussianModel trajectories of T = 1000 frames, S = 2, d = 3, k_max = 20: one trajectory and a batch of 256, with and
without the posterior marginals, next to the enumeration `exact_evidence` at k = 3 on the same single trajectory (the
yardstick: twenty-one values of k have to take less time than k = 3 alone by enumeration).  Each configuration runs once
untimed (tables already built, code loaded), then `--reps` times; the best wall time of a synchronous call is reported.
One JSON line per configuration.

    python tools/segdp_bench.py [--T 1000] [--kmax 20] [--batch 256] [--reps 3] [--no-enumeration] [--out FILE]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--T', type=int, default=1000)
    ap.add_argument('--kmax', type=int, default=20)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--no-enumeration', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    T = a.T
    lags = np.arange(T + 1, dtype=float)
    # (the model and the first trajectory of tools/exact_bench.py)
    model = bild_amd.GenericGaussianModel([[(0.8 * lags ** 0.6 + np.where(lags > 0, 0.2, 0.0), m, 1)] * 3 for m in (0.0, 0.3)])
    trajs = [np.cumsum(rng.normal(size=(T, 3)), axis=0) for _ in range(a.batch)]
    lines = []

    def report(line):
        print(json.dumps(line), flush=True)
        lines.append(line)

    for n in sorted({1, a.batch}):
        arg = trajs[0] if n == 1 else trajs[:n]
        t0 = time.perf_counter()
        model.trajset(arg)
        build = time.perf_counter() - t0
        for marg in (False, True):
            best, res = best_of(lambda: bild_amd.exact_sample(arg, model, k_max=a.kmax, marginals=marg), a.reps)
            first = res if n == 1 else res[0]
            report({'what': 'exact_sample', 'n_traj': n, 'T': T, 'S': 2, 'd': 3, 'k_max': a.kmax, 'marginals': marg, 'seconds': best,
                    'trajectories_per_s': n / best, 'table_build_seconds': build, 'best_k': first.best_k(),
                    'evidence': first.evidence.tolist()})
    if not a.no_enumeration:
        for marg in (False, True):
            best, res = best_of(lambda: bild_amd.exact_evidence(trajs[0], model, 3, marginals=marg), a.reps)
            report({'what': 'exact_evidence', 'n_traj': 1, 'T': T, 'S': 2, 'd': 3, 'k': 3, 'marginals': marg, 'seconds': best,
                    'n_profiles': res.n_profiles, 'logev': res.logev})
        ours = {line['marginals']: line for line in lines if line['what'] == 'exact_sample' and line['n_traj'] == 1}
        for line in lines:
            if line['what'] == 'exact_evidence':
                mine = ours[line['marginals']]
                report({'what': 'comparison', 'marginals': line['marginals'], 'all_k_seconds': mine['seconds'],
                        'k3_enumeration_seconds': line['seconds'], 'faster': mine['seconds'] < line['seconds'],
                        'logev_k3_difference': mine['evidence'][3] - line['logev']})
    if a.out:
        with open(a.out, 'w') as f:
            for line in lines:
                f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
