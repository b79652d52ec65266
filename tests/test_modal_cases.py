"""
The inputs of tests/test_gpu_modal_configs.py (tests/modal_cases.py), checked without a GPU: every model has exactly the modes it
is named for and takes the modal path, the mode counts cover each lane width at its fullest and emptiest, the batch is what
the GPU test relies on (all six ordered state changes, an odd task count, chains that differ inside the set), the oracle's
answers are finite exactly off the NaN tails, and the four derivative directions are the derivatives of the family.
"""
import numpy as np
import pytest

import kalman_oracle as KO
import modal_cases as MC


def _model_configs():
    return sorted({c[:3] for c in MC.KALMAN_CONFIGS} | {c[:3] for c in MC.SENS_CONFIGS})


@pytest.mark.parametrize('cfg', _model_configs(), ids=lambda c: 'n%d_S%d_d%d' % c)
def test_models_have_the_modes_they_are_named_for(cfg):
    from bild_amd import _lib
    h = MC.config(*cfg).model().handle()    # model creation is host-only
    assert h.query(_lib.Q_NEFF) == cfg[0]
    assert h.query(_lib.Q_MODAL_OK) == 1
    assert h.query(_lib.Q_HAS_G) == 1
    assert h.query(_lib.Q_S) == cfg[1] and h.query(_lib.Q_D) == cfg[2]


def test_lane_widths_at_their_fullest_and_emptiest():
    by_width = {}
    for n in MC.MODES:
        by_width.setdefault(MC.lanes(n), []).append(n)
    assert by_width == {8: [2, 8], 16: [9, 16], 32: [17, 32]}
    # every compiled sens_kernel<L, P>: P = 0 ... 4 below 32 lanes at both fill levels, P = 0 alone at 32
    got = {(n, P) for n, S, d, P in MC.SENS_CONFIGS if (S, d) == (3, 3)}
    assert got == {(n, P) for n in (2, 4, 8, 9, 16) for P in range(5)} | {(17, 0), (32, 0)}
    assert {n for n, S, d in MC.KALMAN_CONFIGS if (S, d) == (3, 3)} == set(MC.MODES) | set(MC.MODES_EXTRA)
    # the bit-identity cases are among those held to the oracle
    assert set(MC.BIT_CONFIGS) <= set(MC.SENS_CONFIGS)


def test_states_have_bases_of_their_own():
    """
    A basis change can only be wrong where the bases differ: from n = 4 on no two states' B commute.  At n = 2 all do (the
    case still has the emptiest 8-lane group, its padding lanes and the bookkeeping of a switch), which is why n = 4 runs too.
    """
    def commutators(n):
        B = MC.config(n).arrays['B']
        return [float(np.max(np.abs(B[a] @ B[b] - B[b] @ B[a]))) for a in range(3) for b in range(a + 1, 3)]
    assert max(commutators(2)) < 1e-15
    for n in MC.MODES[1:] + MC.MODES_EXTRA:
        assert min(commutators(n)) > 1e-4, n
    assert MC.lanes(4) == 8


def test_batch_is_what_the_gpu_test_relies_on():
    c = MC.config(9)
    first = c.cands[0]
    assert c.tid[0] == 0 and len(first) == 40
    changes = {(int(a), int(b)) for a, b in zip(first[:-1], first[1:]) if a != b}
    assert changes == {(a, b) for a in range(3) for b in range(3) if a != b}
    # one of its switches lies inside B's gap, on B's own copy of the profile
    b_six = c.cands[1]
    assert c.tid[1] == 1 and np.array_equal(b_six, first)
    gap = np.flatnonzero(np.any(np.isnan(c.trajs[1]), axis=1))
    assert gap.tolist() == [0] + list(range(17, 23)) + [39]
    switches = np.flatnonzero(np.diff(b_six)) + 1
    assert np.any((switches > 17) & (switches < 22))
    assert np.flatnonzero(np.any(np.isnan(c.trajs[2]), axis=1)).tolist() == [5]
    assert np.flatnonzero(np.any(np.isnan(c.trajs[4]), axis=1)).tolist() == [1]
    assert [len(x) for x in c.trajs] == [40, 40, 23, 1, 2]
    # the adjacent switches and the switches at frames 1 and T - 1 are there, on every trajectory long enough
    for j, T in ((0, 40), (1, 40), (2, 23)):
        mine = [st for st, t in zip(c.cands, c.tid) if t == j]
        assert len(mine) == 4
        assert any(st[:6].tolist() == [0, 0, 0, 1, 2, 1] for st in mine)
        assert any((np.flatnonzero(np.diff(st)) + 1).tolist() == [1, T - 1] for st in mine)
        assert any(np.all(st == 2) for st in mine)
    assert [int(np.sum(c.tid == j)) for j in (3, 4)] == [1, 2]
    # an odd task count: the last workgroup is partial at 8, 4 and 2 tasks a wave; at most 19 candidates of 40 frames
    n_tasks = len(c.cands) * max(MC.N_CHAINS[3])
    assert n_tasks % 2 == 1 and len(c.cands) <= 19
    assert all(n_tasks % (64 // L) for L in (8, 16, 32))
    # neighbours differ in their trajectory
    assert np.all(np.diff(c.tid[:10]) != 0)
    # the chains differ inside one set
    for d, chains in MC.N_CHAINS.items():
        for err, want in zip(MC.ERRORS[d], chains):
            counts = np.unique(err, return_counts=True)[1]
            assert sum(-(-int(k) // 3) for k in counts) == want and len(err) == d
    assert len(set(MC.N_CHAINS[3])) == 3 and MC.ERRORS[5][1] == (0.3, 0.3, 0.3, 0.3, 0.5)
    # the run-length encoding gives the profiles back
    from bild_amd.profiles import states_from_segments
    full = states_from_segments(c.seg_start, c.seg_state, 40)
    for r, st in enumerate(c.cands):
        assert np.array_equal(full[r, :len(st)], st)
    # one state: a constant profile per trajectory, still an odd task count
    one = MC.config(2, 1, 3)
    assert len(one.cands) == 5 and all(np.all(st == 0) for st in one.cands)


@pytest.mark.parametrize('cfg', MC.KALMAN_CONFIGS, ids=lambda c: 'n%d_S%d_d%d' % c)
def test_smoother_oracle_is_finite_off_the_tails(cfg):
    c = MC.config(*cfg)
    want = MC.kalman_answer(*cfg)
    nan = MC.expected_nan(c)
    for k in KO.OUTPUTS:
        assert np.array_equal(np.isnan(want[k]), nan[k]), k
        assert np.all(np.isfinite(want[k][~nan[k]])), k
    for k in ('pred_var', 'filt_var', 'smooth_var'):
        assert np.all(want[k][~nan[k]] > 0), k
    assert np.any(nan['terms'])    # the tails behind C, D and E are in the comparison
    assert MC.ORACLE_SECONDS[('kalman',) + tuple(cfg)] < 5.0


@pytest.mark.parametrize('cfg', MC.SENS_CONFIGS, ids=lambda c: 'n%d_S%d_d%d_P%d' % c)
def test_sensitivity_oracle_is_finite(cfg):
    n, S, d, P = cfg
    c = MC.config(n, S, d)
    ll, g, F = MC.sens_answer(*cfg)
    assert ll.shape == (len(c.cands),) and g.shape == (len(c.cands), P) and F.shape == (len(c.cands), P, P)
    assert np.all(np.isfinite(ll)) and np.all(np.isfinite(g)) and np.all(np.isfinite(F))
    assert MC.ORACLE_SECONDS[('sens',) + tuple(cfg)] < 5.0
    # the two oracles agree on logL (test_sensitivity.py: 1e-12 relative)
    terms = np.nansum(MC.kalman_answer(n, S, d)['terms'], axis=(1, 2))
    assert np.max(np.abs(ll - terms) / np.maximum(1.0, np.abs(ll))) <= 1e-12
    if P:   # every direction is in play on some candidate, and the Fisher matrices are positive semi-definite
        assert np.all(np.max(np.abs(g), axis=0) > 0)
        assert all(np.all(np.linalg.eigvalsh(f) >= -1e-10 * np.max(np.abs(f))) for f in F)


def _logl(c, D, k, f, errs, r):
    j = c.tid[r]
    return float(KO.filter_smoother(c.arrays_at(D, k, f), c.w, errs[j], c.trajs[j], c.cands[r])['terms'].sum())


def test_four_parameter_gradient_against_differences():
    """ n = 9, P = 4: central differences of kalman_oracle's logL in D, k, f and sigma, as test_sensitivity.py does at P = 3 """
    c = MC.config(9)
    _, g, _ = MC.sens_answer(9, 3, 3, 4)
    h = 1e-5
    worst = 0.0
    for r in range(len(c.cands)):
        for p in range(3):
            up = [MC.D0, MC.K0, MC.F0]
            dn = list(up)
            step = h * up[p]
            up[p] += step
            dn[p] -= step
            fd = (_logl(c, *up, c.errs, r) - _logl(c, *dn, c.errs, r)) / (2 * step)
            worst = max(worst, abs(g[r, p] - fd) / max(1.0, abs(fd)))
            assert abs(g[r, p] - fd) <= 1e-6 * max(1.0, abs(fd)), (r, p, g[r, p], fd)
    # the localization error: ds2 = 2 sigma differentiates each sigma by itself, so shift every sigma by the same +-h
    for r in range(len(c.cands)):
        fd = (_logl(c, MC.D0, MC.K0, MC.F0, c.errs + h, r) - _logl(c, MC.D0, MC.K0, MC.F0, c.errs - h, r)) / (2 * h)
        worst = max(worst, abs(g[r, 3] - fd) / max(1.0, abs(fd)))
        assert abs(g[r, 3] - fd) <= 1e-6 * max(1.0, abs(fd)), (r, 3, g[r, 3], fd)
    print(f"\nn = 9, P = 4: oracle gradient against central differences, worst relative {worst:.2g}")
