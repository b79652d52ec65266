"""
Every compiled `kalman_kernel<L>` (csrc/kalman.hip) and `sens_kernel<L, P>` (csrc/sens.hip) against the NumPy oracles
(tests/kalman_oracle.py, tests/sensitivity_oracle.py): L = 8, 16 and 32 lanes at their fullest and emptiest mode count,
P = 0 ... 4 tangents (P = 0 alone at 32 lanes), on one ragged batch whose trajectories have one, two and three covariance
chains, T = 1 and T = 2 among them (tests/modal_cases.py).  The bars are those of tests/test_gpu_kalman.py (goldens) and
tests/test_gpu_sensitivity.py.  `-s` prints the worst deviation over its bar per configuration.
"""
import numpy as np
import pytest

import kalman_oracle as KO
import modal_cases as MC
from test_gpu_kalman import ALL, _compare, _result_dict
from test_gpu_sensitivity import REL, _rel

pytestmark = pytest.mark.gpu


def _kalman(c, model=None, rows=None, **kw):
    model = c.model() if model is None else model
    rows = slice(None) if rows is None else rows
    return _result_dict(model.kalman((c.seg_start[rows], c.seg_state[rows]), c.trajectories(), traj_id=c.tid[rows], outputs=ALL, **kw))


def _sens(c, P, model=None, rows=None, **kw):
    model = c.model() if model is None else model
    rows = slice(None) if rows is None else rows
    return model.logL_sensitivities((c.seg_start[rows], c.seg_state[rows]), c.trajectories(), traj_id=c.tid[rows], log=False,
                                    derivatives=c.derivatives(P), **kw)


def _over_bar(got, want, c):
    """ deviation over bar per output, measured before `_compare` asserts (the bars of `_compare`, restated) """
    xs = max(1.0, float(np.nanmax(np.abs(c.data()))))
    bars = {k: 1e-10 if k == 'terms' else 1e-9 * xs if k.endswith('mean') else 1e-8 if k == 'innov' else 1e-9 * c.var_scale()
            for k in KO.OUTPUTS}
    return {k: float(np.nanmax(np.abs(got[k] - want[k]))) / bars[k] for k in KO.OUTPUTS}


@pytest.mark.parametrize('cfg', MC.KALMAN_CONFIGS, ids=lambda c: 'n%d_S%d_d%d' % c)
def test_smoother_against_oracle(built_lib, cfg):
    c = MC.config(*cfg)
    want = MC.kalman_answer(*cfg)
    got = _kalman(c)
    print(f"\nkalman<{MC.lanes(cfg[0])}> n = {cfg[0]}, S = {cfg[1]}, d = {cfg[2]}: deviation / bar: "
          + ', '.join(f"{k} {v:.2g}" for k, v in _over_bar(got, want, c).items()))
    assert np.any(np.isnan(want['smooth_mean']))    # the NaN tails behind C, D and E are compared
    _compare(got, want, c.data(), c.var_scale(), label=str(cfg))


@pytest.mark.parametrize('cfg', MC.SENS_CONFIGS, ids=lambda c: 'n%d_S%d_d%d_P%d' % c)
def test_sensitivities_against_oracle(built_lib, cfg):
    n, S, d, P = cfg
    c = MC.config(n, S, d)
    oll, og, oF = MC.sens_answer(*cfg)
    model = c.model()
    ll, g, F = _sens(c, P, model=model)
    seg = model.logL_segments(c.seg_start, c.seg_state, c.trajectories(), c.tid)
    figures = dict(logL=_rel(ll, oll), segments=_rel(ll, seg), grad=_rel(g, og), fisher=_rel(F, oF))
    print(f"\nsens<{MC.lanes(n)}, {P}> n = {n}, S = {S}, d = {d}: deviation / bar: "
          + ', '.join(f"{k} {v / REL:.2g}" for k, v in figures.items()))
    assert g.shape == og.shape and F.shape == oF.shape
    assert np.all(np.isfinite(ll)) and np.all(np.isfinite(g)) and np.all(np.isfinite(F))
    for k, v in figures.items():
        assert v < REL, (cfg, k, v)


@pytest.mark.parametrize('cfg', MC.BIT_CONFIGS, ids=lambda c: 'n%d_S%d_d%d_P%d' % c)
def test_bit_identity(built_lib, cfg):
    """ the batch equals itself permuted, one candidate alone, and one candidate a chunk """
    n, S, d, P = cfg
    c = MC.config(n, S, d)
    model = c.model()
    rng = np.random.default_rng(n)
    perm = rng.permutation(len(c.cands))
    kal = _kalman(c, model=model)
    sens = _sens(c, P, model=model)
    kal_perm = _kalman(c, model=model, rows=perm)
    sens_perm = _sens(c, P, model=model, rows=perm)
    kal_chunk = _kalman(c, model=model, scratch_bytes=1)
    sens_chunk = _sens(c, P, model=model, scratch_bytes=1)
    for k in KO.OUTPUTS:
        assert np.array_equal(kal[k][perm], kal_perm[k], equal_nan=True), ('permuted', k)
        assert np.array_equal(kal[k], kal_chunk[k], equal_nan=True), ('chunked', k)
    for a, b, ch in zip(sens, sens_perm, sens_chunk):
        assert np.array_equal(a[perm], b) and np.array_equal(a, ch)
    # alone: the first candidate of each trajectory (A's six changes, B's across the gap, C's, T = 1, T = 2)
    for j in range(len(c.trajs)):
        r = int(np.flatnonzero(c.tid == j)[0])
        one = _kalman(c, model=model, rows=slice(r, r + 1))
        for k in KO.OUTPUTS:
            assert np.array_equal(kal[k][r:r + 1], one[k], equal_nan=True), ('alone', j, k)
        for a, b in zip(sens, _sens(c, P, model=model, rows=slice(r, r + 1))):
            assert np.array_equal(a[r:r + 1], b), ('alone', j)
