"""
Throughput of MultiStateRouse.kalman (csrc/kalman.hip) and of the posterior mixture (bild_kalman_mixture):
10 000 candidates (k = 4 switches) on one T = 1000 trajectory, N = 20, d = 3, S = 2; the mixture over a pool of 10^5
samples; the NumPy oracle (tests/kalman_oracle.py: dense filter + RTS smoother) on 20 candidates, one host core.

    python tools/kalman_bench.py [--n 10000] [--pool 100000] [--oracle 20]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def candidates(rng, n, T, k, S=2):
    seg_start = np.zeros((n, k + 1), dtype=np.int32)
    seg_start[:, 1:] = np.sort(rng.integers(1, T, size=(n, k)), axis=1)
    seg_state = rng.integers(S, size=(n, k + 1)).astype(np.int32)
    return seg_start, seg_state


def timed(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=10000)
    ap.add_argument('--pool', type=int, default=100000)
    ap.add_argument('--oracle', type=int, default=20)
    ap.add_argument('--reps', type=int, default=3)
    a = ap.parse_args()
    import bild_amd
    import helpers as H
    import kalman_oracle as KO
    rng = np.random.default_rng(0)
    T = 1000
    model = bild_amd.MultiStateRouse(20, 1.0, 5.0, d=3, localization_error=0.1)
    x = np.array(H.synth_trajectory(model, H.random_profile(rng, T, 2, 200), 0.1, rng)[:])
    ss, st = candidates(rng, a.n, T, 4)
    model.kalman((ss[:1], st[:1]), [x])  # set upload, model tables
    for label, outs in (('smooth', ('smooth',)), ('all outputs', ('terms', 'pred', 'filt', 'smooth', 'innov'))):
        dt = timed(lambda: model.kalman((ss, st), [x], outputs=outs), a.reps)
        print(f"kalman ({label}): {a.n} candidates x {T} frames in {dt * 1e3:.1f} ms = {a.n / dt:.3g} candidates/s, "
              f"{a.n * T / dt:.3g} frames/s")
    ps, pt = candidates(rng, a.pool, T, 4)
    lw = rng.normal(scale=3.0, size=a.pool)
    dt = timed(lambda: model.kalman_mixture((ps, pt), [x], lw), 1)
    print(f"mixture: {a.pool} samples x {T} frames in {dt * 1e3:.1f} ms = {a.pool / dt:.3g} samples/s")
    arrays = model.arrays()
    states = [np.repeat(st[r], np.diff(np.append(ss[r], T))) for r in range(a.oracle)]
    t0 = time.perf_counter()
    for r in range(a.oracle):
        KO.filter_smoother(arrays, model.measurement, model.localization_error, x, states[r])
    do = (time.perf_counter() - t0) / a.oracle
    dg = timed(lambda: model.kalman((ss, st), [x], outputs=('smooth',)), 1) / a.n
    print(f"NumPy oracle: {do * 1e3:.1f} ms per candidate (one host core); device {dg * 1e6:.2f} us per candidate: "
          f"{do / dg:.0f}x")


if __name__ == '__main__':
    main()
