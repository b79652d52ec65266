"""
Cases shared by the tests of the segment recursion (tests/test_segment_dp.py, tests/test_gpu_segment_dp.py): models,
trajectories, and the oracle's answer in the layout of `bild_amd._lib.gauss_segment_evidence`.
"""
import numpy as np

import bild_amd
import gauss_oracle as G
import segment_oracle as SO
from bild_amd.profiles import segments_from_states


def random_model(rng, S, n_lags, orders=None, d=2):
    """ S states with random power-law MSDs; orders: (S, d) ss_orders, random where None; S = 3 forbids 0 -> 2 """
    lags = np.arange(n_lags, dtype=float)
    spec = []
    for n in range(S):
        row = []
        for k in range(d):
            G_, a, s2 = rng.uniform(0.3, 2), rng.uniform(0.4, 1.2), rng.uniform(0.05, 0.3)
            msd = np.where(lags > 0, G_ * lags ** a + 2 * s2, 0)
            order = int(rng.integers(0, 2)) if orders is None else int(orders[n][k])
            mean = rng.normal(scale=0.3)
            row.append((msd if order == 1 else np.append(msd, 2 * G_ * n_lags ** a + 4 + 2 * s2), mean, order))
        spec.append(row)
    model = bild_amd.GenericGaussianModel(spec)
    if S == 3:
        model.transitions[0, 2] = False
    return model


def random_traj(rng, T, missing=(), d=2):
    x = np.cumsum(rng.normal(size=(T, d)), axis=0)
    x[np.asarray(missing, dtype=int)] = np.nan
    return x


def tables(model, x):
    return G.tables(model.msd, model.msd_inf, model.mean, model.ss_order, np.asarray(x, dtype=np.float64))


def oracle_arrays(model, x, k_max, nan='propagate', with_marginals=True):
    """ the oracle's answer for one trajectory as the dict `_lib.gauss_segment_evidence` returns (n_traj = 1) """
    W, F = tables(model, x)
    T, K, S = len(x), k_max + 1, model.nStates
    out = SO.solve(W, F, model.transitions, k_max, nan=nan, with_marginals=with_marginals)
    seg_start = np.full((1, K, K), -1, dtype=np.int32)
    seg_state = np.full((1, K, K), -1, dtype=np.int32)
    for k, states in enumerate(out['map_states']):
        if states is None:
            continue
        a, b = segments_from_states(states)
        seg_start[0, k], seg_state[0, k] = T, 0
        seg_start[0, k, :k + 1], seg_state[0, k, :k + 1] = a[0], b[0]
    return {'logev': out['logev'][None], 'kl': out['KL'][None], 'map_logl': out['map_logL'][None],
            'n_profiles': np.array([out['n_profiles']], dtype=float), 'n_omitted': np.array([out['n_omitted']], dtype=float),
            'map_seg_start': seg_start, 'map_seg_state': seg_state,
            'log_post': out['log_post'][None] if with_marginals else None}, out


def table_logl(W, F, seg_start, seg_state, T):
    """ F[n_0][t1_0] + sum_i W[n_i][t0_i - 1][t1_i] of segment rows (n, k + 1) whose starts strictly increase """
    seg_start, seg_state = np.asarray(seg_start), np.asarray(seg_state)
    ends = np.concatenate([seg_start[:, 1:], np.full((len(seg_start), 1), T)], axis=1)
    total = F[seg_state[:, 0], ends[:, 0]].copy()
    for i in range(1, seg_start.shape[1]):
        total += W[seg_state[:, i], seg_start[:, i] - 1, ends[:, i]]
    return total
