"""
Profiles per second of the exact evidence by enumeration (bild_amd.exact_evidence) on one trajectory of T = 1000 frames
and two states, for MultiStateRouse and GenericGaussianModel, k = 1, 2, 3, with and without the posterior marginals.
Each configuration runs once untimed (the set's tables, code loading), then `--reps` times; the best wall time of a
synchronous call is reported.  One JSON line per configuration.

    python tools/exact_bench.py [--T 1000] [--kmax 3] [--reps 3] [--out FILE]
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


def models(T, rng):
    rouse = bild_amd.MultiStateRouse(20, 1, 5, d=3, localization_error=0.1)
    states = np.repeat([0, 1, 0], [T // 3, T // 3, T - 2 * (T // 3)])
    traj_r = rouse.trajectory_from_loopingprofile(bild_amd.Loopingprofile(states), rng=rng)
    lags = np.arange(T + 1, dtype=float)
    gauss = bild_amd.GenericGaussianModel([[(0.8 * lags ** 0.6 + np.where(lags > 0, 0.2, 0.0), m, 1)] * 3 for m in (0.0, 0.3)])
    traj_g = np.cumsum(rng.normal(size=(T, 3)), axis=0)
    return [('MultiStateRouse', rouse, traj_r), ('GenericGaussianModel', gauss, traj_g)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--T', type=int, default=1000)
    ap.add_argument('--kmax', type=int, default=3)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    lines = []
    for name, model, traj in models(a.T, rng):
        for k in range(1, a.kmax + 1):
            for marg in (False, True):
                res = bild_amd.exact_evidence(traj, model, k, marginals=marg)
                times = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    res = bild_amd.exact_evidence(traj, model, k, marginals=marg)
                    times.append(time.perf_counter() - t0)
                best = min(times)
                line = {'model': name, 'T': a.T, 'S': 2, 'k': k, 'marginals': marg, 'n_profiles': res.n_profiles,
                        'seconds': best, 'profiles_per_s': res.n_profiles / best, 'logev': res.logev, 'KL': res.KL}
                print(json.dumps(line), flush=True)
                lines.append(line)
    if a.out:
        with open(a.out, 'w') as f:
            for line in lines:
                f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
