"""
Cost of bild_amd.exact_sensitivities (csrc/gauss_segsens.hip) next to its yardsticks, one JSON line
per measurement: S = 2, d = 3 (ss_order 0), T = 1000, k_max = 20, P = 0, 1 and 3, one trajectory and a batch, gap-free and
with 10 % missing frames (nan='omit'); per case the table build of the same set (bild_gauss_trajset_info), `exact_sample`
with marginals (the cover kernel's call) and without; the alternative without new kernels, `exact_draw` of 1 000 profiles and
`logL_sensitivities` on them, with the scatter of its gradient over repeats; and a whole `fit_marginal`.

    python tools/segsens_bench.py [--batch 64] [--batch-missing 0] [--P 0 1 3] [--fit 64] [--out profiles/segsens_bench.jsonl]

A kernel breakdown is a run of its own: rocprofv3 --kernel-trace --stats -- python tools/segsens_bench.py --batch 0 --fit 0 --draws 0
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T, K_MAX, D = 1000, 20, 3
BASE, TAU, NOISE = (0.5, 4.0), (3.0, 6.0), 0.02


def make_family(L, d):
    lags = np.arange(L, dtype=np.float64)

    def family(t0, t1, n=NOISE):
        return [[(np.append(t * b * (1 - np.exp(-lags / tau)) + n * (lags > 0), t * b + n), 0.0, 0)] * d
                for t, b, tau in zip((t0, t1), BASE, TAU)]

    def derivatives(P):
        dmsd, dinf = np.zeros((3, 2, d, L)), np.zeros((3, 2, d))
        for s in range(2):
            dmsd[s, s] = BASE[s] * (1 - np.exp(-lags / TAU[s]))
            dinf[s, s] = BASE[s]
        dmsd[2, :, :, 1:] = 1.0
        dinf[2] = 1.0
        return dict(dmsd=dmsd[:P], dmsd_inf=dinf[:P])

    return family, derivatives


def prior_profiles(rng, n, T, k_max):
    out = []
    for _ in range(n):
        k = int(rng.integers(0, k_max + 1))
        sw = np.sort(rng.choice(np.arange(1, T), size=k, replace=False))
        s = int(rng.integers(0, 2))
        states = np.zeros(T, dtype=int)
        edges = [0, *sw, T]
        for i in range(k + 1):
            states[edges[i]:edges[i + 1]] = (s + i) % 2
        out.append(states)
    return out


def timed(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    return (time.perf_counter() - t0) / reps, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64, help='trajectories of the gap-free batch (0: skip)')
    ap.add_argument('--batch-missing', type=int, default=0, help='trajectories of the batch with missing frames (0: skip)')
    ap.add_argument('--P', type=int, nargs='+', default=[0, 1, 3])
    ap.add_argument('--reps', type=int, default=2)
    ap.add_argument('--draws', type=int, default=1000, help='profiles of the sampled alternative (0: skip)')
    ap.add_argument('--fit', type=int, default=64, help='trajectories of the fit, T = 200, k_max = 3 (0: skip)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'segsens_bench.jsonl'))
    a = ap.parse_args()
    import bild_amd
    from bild_amd import _lib

    lines = []

    def emit(**kw):
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    family, derivatives = make_family(T, D)
    rng = np.random.default_rng(0)
    truth = bild_amd.GenericGaussianModel(family(1.0, 1.0))
    model = bild_amd.GenericGaussianModel(family(1.5, 1 / 1.5, 1.5 * NOISE))        # off the truth: a gradient far from zero
    for miss, n in ((0.0, 1), (0.1, 1), (0.0, a.batch), (0.1, a.batch_missing)):
        if n == 0:
            continue
        nan = 'omit' if miss else 'propagate'
        trajs = [t[:] for t in truth.trajectories_from_loopingprofiles(prior_profiles(rng, n, T, 6), missing_frames=miss or None, seed=3)]
        t0 = time.perf_counter()
        ts = model.trajset(trajs)
        case = dict(T=T, S=2, d=D, k_max=K_MAX, n_traj=n, missing=miss)
        emit(what='table_build', **case, wall_s=time.perf_counter() - t0, build_ms=ts.info()[1])
        for marg in (False, True):
            dt, _ = timed(lambda: bild_amd.exact_sample(trajs, model, k_max=K_MAX, marginals=marg, nan=nan), a.reps)
            emit(what='exact_sample', **case, marginals=marg, seconds=dt)
        for P in a.P:
            dt, r = timed(lambda: bild_amd.exact_sensitivities(trajs, model, k_max=K_MAX, nan=nan, **derivatives(P)), a.reps)
            emit(what='exact_sensitivities', **case, P=P, seconds=dt, grad=r.grad[0].tolist(), log_marginal=float(r.log_marginal[0]))
        if n == 1 and a.draws:
            # the alternative without new kernels: profiles drawn from the exact posterior, their sensitivities averaged
            res = bild_amd.exact_sample(trajs[0], model, k_max=K_MAX, marginals=False, nan=nan)
            dm = derivatives(3)
            grads, secs = [], []
            for seed in range(5):
                t0 = time.perf_counter()
                draws = bild_amd.exact_draw(res, a.draws, k='average', seed=seed)
                _, g, _ = model.logL_sensitivities((draws.seg_start, draws.seg_state), [trajs[0]],
                                                   traj_id=np.zeros(a.draws, dtype=np.int32), fisher=False, **dm)
                secs.append(time.perf_counter() - t0)
                grads.append(g.mean(axis=0))
            grads = np.array(grads)
            emit(what='drawn_alternative', **case, P=3, draws=a.draws, seconds=float(np.mean(secs[1:])),
                 grad_mean=grads.mean(axis=0).tolist(), grad_scatter=grads.std(axis=0, ddof=1).tolist(), exact_grad=r.grad[0].tolist())
        model._trajsets.clear()

    if a.fit:
        Tf, kf = 200, 3
        fam, _ = make_family(Tf, 2)
        gen = bild_amd.GenericGaussianModel(fam(1.0, 1.0))
        trajs = [t[:] for t in gen.trajectories_from_loopingprofiles(prior_profiles(np.random.default_rng(64), a.fit, Tf, kf), seed=9)]
        build_s = [0.0]
        create = _lib.GaussTrajSetHandle.__init__

        def counted(self, *args):
            t0 = time.perf_counter()
            create(self, *args)
            build_s[0] += time.perf_counter() - t0
        _lib.GaussTrajSetHandle.__init__ = counted
        try:
            t0 = time.perf_counter()
            res = bild_amd.GenericGaussianModel.fit_marginal(trajs, lambda t0, t1: fam(t0, t1), dict(t0=1.5, t1=1 / 1.5), k_max=kf)
            wall = time.perf_counter() - t0
        finally:
            _lib.GaussTrajSetHandle.__init__ = create
        emit(what='fit_marginal', T=Tf, n_traj=a.fit, k_max=kf, P=2, evaluations=res.n_iter, converged=res.converged, wall_s=wall,
             table_build_s=build_s[0], table_share=build_s[0] / wall, params=res.params, se=res.se)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        for kw in lines:
            f.write(json.dumps(kw) + '\n')


if __name__ == '__main__':
    main()
