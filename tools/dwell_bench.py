"""
Wall time of the exact inference under a dwell-time prior (bild_amd.exact_dwell) on the data of
tools/segdp_bench.py (GenericGaussianModel, T = 1000 frames, S = 2, d = 3): one trajectory and a batch of 256, with the
marginals and the expected counts, the online filter `exact_dwell_filter` (without run lengths, and on
the single trajectory with all of them), the fixed-lag smoother `exact_dwell_lag` at every `--lags`
and `exact_sample(k_max=20, marginals=True)` on the same data in the same session,
and one `fit_markov_prior` on 64 simulated trajectories of T = 200 (the data set of tests/test_gpu_dwell.py) with its number
of device calls and the share of the one table build.  Each configuration runs once untimed (tables built, code loaded),
then `--reps` times; the best wall time of a synchronous call is reported.  One JSON line per configuration.

    python tools/dwell_bench.py [--T 1000] [--kmax 20] [--batch 256] [--reps 5] [--lags 15 63] [--single-only] [--dwell-only]
                                [--out FILE]

`--single-only` runs the single-trajectory `exact_dwell`, `exact_dwell_filter` and `exact_dwell_lag` alone: the part a
`rocprofv3 --kernel-trace --stats` run is made of.  `--dwell-only` leaves out `exact_sample` and the fit.
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


def fit_data(n=64, T=200):
    """ the model, the true chain and the simulated trajectories of tests/test_gpu_dwell.py::test_fit_markov_prior """
    lags = np.arange(T + 8, dtype=float)
    model = bild_amd.GenericGaussianModel([[(np.where(lags > 0, g * lags ** a + 0.1, 0), 0.0, 1)] * 2
                                           for g, a in ((0.3, 0.6), (2.0, 0.9))])
    P_true, init_true = np.array([[0.95, 0.05], [0.1, 0.9]]), np.array([0.5, 0.5])
    rng = np.random.default_rng(61)
    profiles = []
    for _ in range(n):
        st = np.empty(T, dtype=int)
        st[0] = rng.choice(2, p=init_true)
        for t in range(1, T):
            st[t] = rng.choice(2, p=P_true[st[t - 1]])
        profiles.append(st)
    return model, P_true, init_true, model.trajectories_from_loopingprofiles(profiles, seed=62)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--T', type=int, default=1000)
    ap.add_argument('--kmax', type=int, default=20)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--lags', type=int, nargs='*', default=[15, 63])
    ap.add_argument('--single-only', action='store_true')
    ap.add_argument('--dwell-only', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    T = a.T
    lags = np.arange(T + 1, dtype=float)
    # (the model and the trajectories of tools/segdp_bench.py)
    model = bild_amd.GenericGaussianModel([[(0.8 * lags ** 0.6 + np.where(lags > 0, 0.2, 0.0), m, 1)] * 3 for m in (0.0, 0.3)])
    trajs = [np.cumsum(rng.normal(size=(T, 3)), axis=0) for _ in range(a.batch)]
    prior = bild_amd.DwellPrior.markov([[0.98, 0.02], [0.05, 0.95]], [0.5, 0.5], n=T)
    lines = []

    def report(line):
        print(json.dumps(line), flush=True)
        lines.append(line)

    for n in ([1] if a.single_only else sorted({1, a.batch})):
        arg = trajs[0] if n == 1 else trajs[:n]
        t0 = time.perf_counter()
        model.trajset(arg)
        build = time.perf_counter() - t0
        for marg in (False, True):
            best, res = best_of(lambda: bild_amd.exact_dwell(arg, model, prior, marginals=marg), a.reps)
            first = res if n == 1 else res[0]
            report({'what': 'exact_dwell', 'n_traj': n, 'T': T, 'S': 2, 'd': 3, 'marginals': marg, 'seconds': best,
                    'trajectories_per_s': n / best, 'table_build_seconds': build, 'log_evidence': first.log_evidence,
                    'map_switches': int(np.count_nonzero(np.diff(first.map_profile[:])))})
        for run_max in ([0, T] if n == 1 else [0]):
            best, res = best_of(lambda: bild_amd.exact_dwell_filter(arg, model, prior, run_max=run_max), a.reps)
            first = res if n == 1 else res[0]
            report({'what': 'exact_dwell_filter', 'n_traj': n, 'T': T, 'S': 2, 'd': 3, 'run_max': run_max, 'seconds': best,
                    'trajectories_per_s': n / best, 'table_build_seconds': build, 'log_evidence': first.log_evidence,
                    'prefix_log_evidence_last': float(first.prefix_log_evidence[-1]),
                    'run_length_mean_last': float(first.run_length_mean[-1])})
        for lag in a.lags:
            best, res = best_of(lambda: bild_amd.exact_dwell_lag(arg, model, prior, lag), a.reps)
            first = res if n == 1 else res[0]
            settle = first.settling_lag()
            report({'what': 'exact_dwell_lag', 'n_traj': n, 'T': T, 'S': 2, 'd': 3, 'lag': lag, 'seconds': best,
                    'trajectories_per_s': n / best, 'table_build_seconds': build, 'log_evidence': first.log_evidence,
                    'settling_lag_median': float(np.median(settle)), 'frames_not_settled': int(np.sum(settle == lag))})
        if a.single_only:
            break
        if a.dwell_only:
            continue
        best, res = best_of(lambda: bild_amd.exact_sample(arg, model, k_max=a.kmax, marginals=True), a.reps)
        report({'what': 'exact_sample', 'n_traj': n, 'T': T, 'S': 2, 'd': 3, 'k_max': a.kmax, 'marginals': True, 'seconds': best,
                'trajectories_per_s': n / best})
    if not a.single_only and not a.dwell_only:
        fmodel, P_true, init_true, ftrajs = fit_data()
        t0 = time.perf_counter()
        fmodel.trajset(ftrajs)
        build = time.perf_counter() - t0
        t0 = time.perf_counter()
        fit = bild_amd.fit_markov_prior(ftrajs, fmodel, start=np.array([[0.9, 0.1], [0.2, 0.8]]))
        seconds = time.perf_counter() - t0
        report({'what': 'fit_markov_prior', 'n_traj': len(ftrajs), 'T': 200, 'device_calls': fit.n_iter, 'converged': bool(fit.converged),
                'seconds': seconds, 'seconds_per_call': seconds / fit.n_iter, 'table_build_seconds': build,
                'table_build_share': build / (build + seconds), 'P': fit.P.tolist(), 'init': fit.init.tolist(),
                'P_true': P_true.tolist(), 'init_true': init_true.tolist(), 'log_evidence_first': float(fit.log_evidence[0]),
                'log_evidence_last': float(fit.log_evidence[-1])})
    if a.out:
        with open(a.out, 'w') as f:
            for line in lines:
                f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
