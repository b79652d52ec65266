"""
Throughput of MultiStateRouse.logL_sensitivities (csrc/sens.hip) and wall time of MultiStateRouse.fit:
10 000 candidates (k = 4 switches) on one T = 1000 trajectory, N = 20, d = 3, S = 2, at P = 0, 1 and 3 parameters; a fit of
(D, k, localization_error) on 256 simulated trajectories of T = 1000 from a start 2x off in every parameter; the NumPy
tangent filter (tests/sensitivity_oracle.py) at P = 3 on a few candidates, one host core.

    python tools/fit_bench.py [--n 10000] [--fit 256] [--oracle 3]
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


def candidates(rng, n, T, k, S=2):
    seg_start = np.zeros((n, k + 1), dtype=np.int32)
    seg_start[:, 1:] = np.sort(rng.integers(1, T, size=(n, k)), axis=1)
    seg_state = rng.integers(S, size=(n, k + 1)).astype(np.int32)
    return seg_start, seg_state


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=10000)
    ap.add_argument('--fit', type=int, default=256)
    ap.add_argument('--oracle', type=int, default=3)
    ap.add_argument('--reps', type=int, default=3)
    a = ap.parse_args()
    import bild_amd
    import helpers as H
    import sensitivity_oracle as SO

    rng = np.random.default_rng(0)
    T = 1000
    model = bild_amd.MultiStateRouse(20, 1.0, 5.0, d=3, localization_error=0.1)
    traj = model.trajectory_from_loopingprofile(H.random_profile(rng, T, 2, 200), rng=rng)
    ss, st = candidates(rng, a.n, T, 4)
    out = {}
    for params in ((), ('D',), ('D', 'k', 'localization_error')):
        fn = lambda: model.logL_sensitivities((ss, st), traj, params=params)   # noqa: E731
        fn()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
        dt = (time.perf_counter() - t0) / a.reps
        out[f'P{len(params)}_s'] = dt
        out[f'P{len(params)}_cand_per_s'] = a.n / dt

    # fit: 256 simulated trajectories, start 2x off
    profiles = [H.random_profile(rng, T, 2, 200) for _ in range(a.fit)]
    trajs = model.trajectories_from_loopingprofiles(profiles, seed=1)
    t0 = time.perf_counter()
    res = model.fit(trajs, profiles, start={'D': 2.0, 'k': 10.0, 'localization_error': 0.2})
    out['fit_s'] = time.perf_counter() - t0
    out['fit_iter'] = res.n_iter
    out['fit_converged'] = res.converged
    out['fit_params'] = res.params
    out['fit_se'] = res.se

    # the NumPy oracle, P = 3, one host core
    D_k = SO.rouse_family(20, [None, (0, -1)], d=3)[1](1.0, 5.0)
    derivs = {k: np.concatenate([v, np.zeros((1,) + v.shape[1:])]) for k, v in D_k.items()}
    ds2 = np.zeros((3, 3))
    ds2[2] = 0.2
    arrays, x = model.arrays(), traj[:]
    t0 = time.perf_counter()
    for r in range(a.oracle):
        states = np.zeros(T, dtype=int)
        for q in range(ss.shape[1]):
            states[ss[r, q]:] = st[r, q]
        SO.tangent_filter(arrays, model.measurement, model.localization_error, x, states, derivs, ds2)
    out['oracle_s_per_cand'] = (time.perf_counter() - t0) / max(a.oracle, 1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
