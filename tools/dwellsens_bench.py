"""
Cost of bild_amd.exact_dwell_sensitivities (csrc/gauss_dwellsens.hip) next to its yardsticks, one JSON line
per measurement: section 20's data -- S = 2, d = 3 (ss_order 0), T = 1000 -- under section 21's prior, P = 0, 1 and 3, one
trajectory and a batch; per case `exact_dwell` without marginals (the forward pass alone) and with, `exact_sensitivities` at
k_max = 20 and the same P in the same session, and the table build of the set; and the `fit_dwell` of
tests/test_gpu_dwell_sensitivity.py (the same data set, start and call), its wall time split into table builds, the inner EM
and the gradient calls.  The family and the profile generator are those of tests/dwell_sensitivity_cases.py.

    python tools/dwellsens_bench.py [--batch 64] [--P 0 1 3] [--reps 3] [--fit 32] [--out profiles/dwellsens_bench.jsonl]

The weight kernel next to section 20's comes from a run of its own:
    rocprofv3 --kernel-trace --stats -- python tools/dwellsens_bench.py --batch 0 --fit 0 --reps 1 --out /dev/null
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

T, K_MAX, D = 1000, 20, 3
PRIOR_P = np.array([[0.98, 0.02], [0.05, 0.95]])      # section 21's prior


def timed(fn, reps):
    fn()        # warm-up: the first call of a kernel loads its code object
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    return (time.perf_counter() - t0) / reps, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64, help='trajectories of the batch (0: skip)')
    ap.add_argument('--P', type=int, nargs='+', default=[0, 1, 3])
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--fit', type=int, default=32, help='trajectories of the fit, T = 128 (0: skip)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'dwellsens_bench.jsonl'))
    a = ap.parse_args()
    import bild_amd
    import dwell_sensitivity_cases as DSC
    from bild_amd import _lib, exact

    lines = []

    def emit(**kw):
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    family, derivs = DSC.exp_family(T, d=D)
    theta = (1.5, 1 / 1.5, 1.5 * DSC.NOISE)         # off the truth: a gradient far from zero

    def derivatives(P):
        dmsd, dinf, _ = derivs(*theta)
        return dict(dmsd=dmsd[:P], dmsd_inf=dinf[:P])

    rng = np.random.default_rng(0)
    truth = bild_amd.GenericGaussianModel(family(1.0, 1.0))
    model = bild_amd.GenericGaussianModel(family(*theta))
    prior = bild_amd.DwellPrior.markov(PRIOR_P, [0.5, 0.5], n=T)
    for n in (1, a.batch):
        if n == 0:
            continue
        trajs = [t[:] for t in truth.trajectories_from_loopingprofiles(DSC.markov_profiles(rng, n, T, PRIOR_P), seed=3)]
        t0 = time.perf_counter()
        ts = model.trajset(trajs)
        case = dict(T=T, S=2, d=D, n_traj=n, reps=a.reps)
        emit(what='table_build', **case, wall_s=time.perf_counter() - t0, build_ms=ts.info()[1])
        for marg in (False, True):
            dt, _ = timed(lambda: bild_amd.exact_dwell(trajs, model, prior, marginals=marg), a.reps)
            emit(what='exact_dwell', **case, marginals=marg, seconds=dt)
        for P in a.P:
            dt, r = timed(lambda: bild_amd.exact_dwell_sensitivities(trajs, model, prior, **derivatives(P)), a.reps)
            emit(what='exact_dwell_sensitivities', **case, P=P, seconds=dt, grad=r.grad[0].tolist(), log_evidence=float(r.log_evidence[0]))
            dt, r = timed(lambda: bild_amd.exact_sensitivities(trajs, model, k_max=K_MAX, **derivatives(P)), a.reps)
            emit(what='exact_sensitivities', **case, k_max=K_MAX, P=P, seconds=dt, grad=r.grad[0].tolist())
        model._trajsets.clear()

    if a.fit:
        # the data set and the call of tests/test_gpu_dwell_sensitivity.py::test_fit_dwell_with_a_fitted_markov_prior
        Tf = 128
        fam, fam_derivs = DSC.exp_family(Tf, with_noise=False)
        gen = bild_amd.GenericGaussianModel(fam(1.0, 1.0))
        trajs = [t[:] for t in gen.trajectories_from_loopingprofiles(DSC.markov_profiles(np.random.default_rng(128), a.fit, Tf, DSC.FIT_P), seed=9)]
        spent = {'build': 0.0, 'em': 0.0, 'grad': 0.0}
        create, em, grad = _lib.GaussTrajSetHandle.__init__, exact.fit_markov_prior, exact.exact_dwell_sensitivities

        def clocked(key, fn):
            def wrapper(*args, **kw):
                t0 = time.perf_counter()
                try:
                    return fn(*args, **kw)
                finally:
                    spent[key] += time.perf_counter() - t0
            return wrapper
        _lib.GaussTrajSetHandle.__init__ = clocked('build', create)
        exact.fit_markov_prior, exact.exact_dwell_sensitivities = clocked('em', em), clocked('grad', grad)
        try:
            t0 = time.perf_counter()
            res = bild_amd.GenericGaussianModel.fit_dwell(trajs, fam, dict(t0=1.5, t1=1 / 1.5),
                                                          markov_start=np.array([[0.9, 0.1], [0.2, 0.8]]), derivatives=fam_derivs)
            wall = time.perf_counter() - t0
        finally:
            _lib.GaussTrajSetHandle.__init__ = create
            exact.fit_markov_prior, exact.exact_dwell_sensitivities = em, grad
        # (the set is built inside the inner EM's first call: its time is taken out of the EM's)
        emit(what='fit_dwell', T=Tf, n_traj=a.fit, P=2, evaluations=res.n_iter, converged=res.converged, wall_s=wall,
             table_build_s=spent['build'], inner_em_s=spent['em'] - spent['build'], gradient_calls_s=spent['grad'],
             params=res.params, se=res.se, markov_P=res.prior_fit.P.tolist(), single_run=True)

    if a.out != os.devnull:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            for kw in lines:
                f.write(json.dumps(kw) + '\n')


if __name__ == '__main__':
    main()
