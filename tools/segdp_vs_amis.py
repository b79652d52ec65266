"""
AMIS evidences of GenericGaussianModel against the exact ones for EVERY k the samplers visited: trajectories of T = 1000
frames are simulated in one batch with the model's GPU generator (the setup of tools/exact_vs_amis.py), `sample_many` runs
the adaptive-k inference on them, `exact_sample` gives the exact evidence of every k <= k_max in one call, and every
sampler is compared at its k: z = (AMIS logev - exact logev) / evidence_se.  Also: does the k the sampler picks agree with
the exact best k?  A measurement, not a test (DESIGN.md section 18 records its output).

    python tools/segdp_vs_amis.py [--n 12] [--T 1000] [--kmax 20] [--seed 0] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import bild_amd  # noqa: E402
from exact_vs_amis import truth_profiles  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=12)
    ap.add_argument('--T', type=int, default=1000)
    ap.add_argument('--kmax', type=int, default=20)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    np.random.seed(a.seed)
    profiles = truth_profiles(rng, a.n, a.T)
    lags = np.arange(a.T + 1, dtype=float)
    model = bild_amd.GenericGaussianModel([[(0.8 * lags ** 0.6 + np.where(lags > 0, 0.2, 0.0), m, 1)] * 3 for m in (0.0, 0.1)])
    trajs = model.trajectories_from_loopingprofiles(profiles, seed=a.seed)
    results = bild_amd.sample_many(trajs, model)
    exact = bild_amd.exact_sample(trajs, model, k_max=a.kmax, marginals=False)
    lines = []

    def report(line):
        print(json.dumps(line), flush=True)
        lines.append(line)

    rows = []
    for j, (res, ex) in enumerate(zip(results, exact)):
        for s in res.samplers:
            if s.k > a.kmax:
                continue
            logev, se = s.evidences[-1][:2]
            rows.append({'traj': j, 'k': int(s.k), 'true_k': int(np.sum(np.diff(profiles[j]) != 0)), 'exhausted': bool(s.exhausted),
                         'amis_logev': float(logev), 'evidence_se': float(se), 'exact_logev': float(ex.evidence[s.k]),
                         'diff': float(logev - ex.evidence[s.k]), 'z': float((logev - ex.evidence[s.k]) / se) if se > 0 else None})
            report(rows[-1])
        report({'traj': j, 'true_k': rows[-1]['true_k'], 'amis_best_k': int(res.best_k()), 'exact_best_k': ex.best_k(res.dE),
                'exact_best_k_dE0': ex.best_k(0), 'k_visited': [int(s.k) for s in res.samplers]})
    for k in sorted({r['k'] for r in rows}):
        sel = [r for r in rows if r['k'] == k and not r['exhausted'] and r['z'] is not None]
        if sel:
            z, d = np.array([r['z'] for r in sel]), np.array([r['diff'] for r in sel])
            report({'k': k, 'samplers': len(sel), 'mean_diff': float(d.mean()), 'min_diff': float(d.min()), 'max_diff': float(d.max()),
                    'median_z': float(np.median(z)), 'share_z_below_-1': float(np.mean(z < -1)), 'share_z_above_1': float(np.mean(z > 1))})
    if a.out:
        with open(a.out, 'w') as f:
            for line in lines:
                f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
