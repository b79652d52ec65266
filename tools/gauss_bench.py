#!/usr/bin/env python3
"""
GenericGaussianModel costs, one JSON line: the table build (ms, bytes) at T = 200 and 1000 for S = 2, d = 3, without
and with 10 % missing values; evaluations per second of a 10 000-candidate k = 4 (s, theta) batch on the T = 1000
tables; and, for comparison, seconds per evaluation of the NumPy restatement of the reference loop on one core
(tests/gauss_oracle.py).  Needs the GPU.

    python tools/gauss_bench.py [--reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def case(rng, T, p_missing, S=2, d=3):
    lags = np.arange(T, dtype=float)
    msd = np.zeros((S, d, T))
    inf = np.zeros((S, d))
    for n in range(S):
        for k in range(d):
            msd[n, k] = np.where(lags > 0, (1 + n) * lags ** (0.5 + 0.1 * k) + 0.2, 0)
            inf[n, k] = 2 * (1 + n) * T ** (0.5 + 0.1 * k) + 5
    order = np.array([[0, 1, 0], [1, 0, 0]])[:S, :d]
    mean = np.full((S, d), 0.1)
    x = np.cumsum(rng.normal(size=(T, d)), axis=0)
    if p_missing:
        x[rng.random((T, d)) < p_missing] = np.nan
    return msd, inf, mean, order, x


def model(msd, inf, mean, order):
    import bild_amd
    S, d = order.shape
    return bild_amd.GenericGaussianModel([[(msd[n, k] if order[n, k] else np.append(msd[n, k], inf[n, k]), mean[n, k],
                                            int(order[n, k])) for k in range(d)] for n in range(S)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
    os.environ.setdefault('OMP_NUM_THREADS', '1')
    import gauss_oracle as G
    rng = np.random.default_rng(0)
    out = {'config': 'GenericGaussianModel S=2 d=3'}
    keep = {}
    for T in (200, 1000):
        for p in (0.0, 0.1):
            c = case(rng, T, p)
            m = model(*c[:4])
            ms = []
            for _ in range(args.reps):
                m.invalidate()
                ts = m.trajset(c[4])
                b, t = ts.info()
                ms.append(t)
            tag = f"T{T}_{'missing10' if p else 'gapfree'}"
            out[f'build_ms_{tag}'] = round(float(np.median(ms)), 3)
            out[f'table_bytes_{tag}'] = int(b)
            keep[T, p] = (m, c)
    m, c = keep[1000, 0.1]
    n, k = 10000, 4
    ss = rng.dirichlet(np.ones(k + 1), size=n)
    th = np.zeros((n, k + 1), dtype=np.int64)
    th[:, 0] = rng.integers(2, size=n)
    for i in range(1, k + 1):
        th[:, i] = 1 - th[:, i - 1]
    m.logL_st_batch(ss, th, c[4])
    ts = []
    for _ in range(args.reps * 4):
        t0 = time.perf_counter()
        m.logL_st_batch(ss, th, c[4])
        ts.append(time.perf_counter() - t0)
    out['evals_per_s_k4_T1000_missing10'] = round(n / float(np.median(ts)), 1)
    out['eval_batch_ms'] = round(1e3 * float(np.median(ts)), 3)
    # the NumPy oracle of the reference loop, a few profiles
    from bild_amd.amis import FixedkSampler
    import bild_amd
    fs = FixedkSampler(bild_amd.Trajectory(c[4]), m, k=k, N=10)
    t0 = time.perf_counter()
    for r in range(3):
        G.logl_reference(*c[:5], np.asarray(fs.st2profile(ss[r], th[r])[:]))
    out['oracle_s_per_eval_T1000_missing10'] = round((time.perf_counter() - t0) / 3, 4)
    out['build_breakeven_evals_T1000_missing10'] = round(out['build_ms_T1000_missing10'] / 1e3 / out['oracle_s_per_eval_T1000_missing10'], 1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
