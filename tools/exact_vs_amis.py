"""
AMIS evidences against the exact ones at realistic T: trajectories of T = 1000 frames are simulated in one batch with the
model's GPU generator, `sample_many` runs the adaptive-k inference on them, and every sampler it left at 1 <= k <= kmax is
compared with `exact_evidence` at that k: z = (AMIS logev - exact logev) / evidence_se.  A measurement, not a test
(DESIGN.md section 17 records its output); the small-T counterpart is tools/rng_check.py.

    python tools/exact_vs_amis.py [--n 16] [--T 1000] [--kmax 2] [--seed 0] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import bild_amd  # noqa: E402


def truth_profiles(rng, n, T):
    out = []
    for _ in range(n):
        k = int(rng.integers(0, 3))
        cuts = np.sort(rng.choice(np.arange(50, T - 50), size=k, replace=False))
        states = (int(rng.integers(0, 2)) + np.arange(k + 1)) % 2
        out.append(np.repeat(states, np.diff(np.r_[0, cuts, T])))
    return np.array(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=16)
    ap.add_argument('--T', type=int, default=1000)
    ap.add_argument('--kmax', type=int, default=2)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    np.random.seed(a.seed)
    profiles = truth_profiles(rng, a.n, a.T)
    lags = np.arange(a.T + 1, dtype=float)
    cases = [
        ('MultiStateRouse', bild_amd.MultiStateRouse(20, 1, 5, d=3, localization_error=0.1)),
        ('GenericGaussianModel', bild_amd.GenericGaussianModel(
            [[(0.8 * lags ** 0.6 + np.where(lags > 0, 0.2, 0.0), m, 1)] * 3 for m in (0.0, 0.1)])),
    ]
    rows = []
    for name, model in cases:
        trajs = model.trajectories_from_loopingprofiles(profiles, seed=a.seed)
        results = bild_amd.sample_many(trajs, model)
        for j, res in enumerate(results):
            for s in res.samplers:
                if not 1 <= s.k <= a.kmax or s.exhausted:
                    continue
                ex = bild_amd.exact_evidence(trajs[j], model, s.k, marginals=False)
                logev, se = s.evidences[-1][:2]
                rows.append({'model': name, 'traj': j, 'k': s.k, 'true_k': int(np.sum(np.diff(profiles[j]) != 0)),
                             'amis_logev': float(logev), 'evidence_se': float(se), 'exact_logev': ex.logev,
                             'diff': float(logev - ex.logev), 'z': float((logev - ex.logev) / se), 'amis_steps': len(s.evidences)})
                print(json.dumps(rows[-1]), flush=True)
    for name, _ in cases:
        for k in range(1, a.kmax + 1):
            z = np.array([r['z'] for r in rows if r['model'] == name and r['k'] == k])
            d = np.array([r['diff'] for r in rows if r['model'] == name and r['k'] == k])
            if len(z):
                print(json.dumps({'model': name, 'k': k, 'samplers': len(z), 'mean_diff': float(d.mean()),
                                  'mean_z': float(z.mean()), 'median_z': float(np.median(z)), 'share_z_below_-1': float(np.mean(z < -1)),
                                  'share_z_above_1': float(np.mean(z > 1))}), flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            for r in rows:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
