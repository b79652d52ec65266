"""
The draws under a dwell-time prior without a GPU (bild_amd.exact.exact_dwell_draw): the NumPy oracle
tests/dwell_draw_oracle.py against the enumeration of every profile of every k on the cases of tests/test_dwell.py, its
special cases, the host helpers of `ExactDwellDraws`, the refusals of `exact_dwell_draw`, which are raised before any upload,
and the condition on the GPU test's inputs that no draw of them is fragile.

The count bound is that of tests/test_segment_draw.py: of N independent draws a profile of posterior p is drawn
Binomial(N, p) times, and |count - N p| <= 5.5 sqrt(N p (1 - p)) + 3 is asked of every profile (two-sided normal tail 4e-8 per
comparison, + 3 for the Poisson regime of small N p).  The 20 cases make 2.6e4 comparisons: a correct sampler fails with
probability about 1e-3, and with the fixed seeds not at all once it has passed.
"""
import numpy as np
import pytest

import bild_amd
import dwell_cases as DC
import dwell_draw_cases as DDC
import dwell_draw_oracle as DDO
import dwell_oracle as DO
import segment_cases as C
from bild_amd import _lib
from bild_amd.profiles import states_from_segments
from test_dwell import CASES, build
from test_segment_draw import check_counts

N_DRAWS = 20000

ENUM_CASES = [(name, kind, 'propagate') for name in CASES if 'order0' not in name for kind in ('markov', 'nongeometric', 'minlength')] \
    + [('s2_order0_inner_gap', kind, 'omit') for kind in ('markov', 'minlength')]


def profile_counts(all_states, drawn):
    """ how often each enumerated profile (rows of all_states) occurs among the drawn rows; a row that is no profile: KeyError """
    index = {row.tobytes(): i for i, row in enumerate(all_states.astype(np.uint8))}
    rows, c = np.unique(np.asarray(drawn, dtype=np.uint8), axis=0, return_counts=True)
    counts = np.zeros(len(all_states), dtype=np.int64)
    for row, n in zip(rows, c):
        counts[index[row.tobytes()]] = n
    return counts


@pytest.mark.parametrize('name,kind,nan', ENUM_CASES)
def test_oracle_draws_against_enumeration(name, kind, nan):
    model, x, prior = build(name, kind)
    W, F = C.tables(model, x)
    T = len(x)
    states, joint, p, bad = DDO.profile_posterior(W, F, prior)
    want = DO.enumerate_all(W, F, prior, nan=nan)
    assert (bad.sum() > 0) == ('order0' in name) and want['n_nan'] == bad.sum()
    live = np.where(bad, -np.inf, joint)
    assert abs(np.logaddexp.reduce(live) - want['logev']) < 1e-12       # the same profiles and log joints as enumerate_all
    u = np.random.default_rng(sum(map(ord, name + kind)) + 1).random((N_DRAWS, 2 * T - 1))
    d = DDO.draws(W, F, prior, u)
    assert np.all(d['n_switches'] >= 0) and np.all(d['states'] < model.nStates)
    assert np.array_equal(np.count_nonzero(np.diff(d['states'].astype(int), axis=1), axis=1), d['n_switches'])
    assert np.array_equal(d['n_uniforms'], 1 + 2 * d['n_switches'])     # a pick with one candidate included
    counts = profile_counts(states, d['states'])
    assert np.all(counts[bad] == 0) and np.all(counts[joint == -np.inf] == 0)       # no NaN window, no prior weight 0
    worst = check_counts(counts, p, N_DRAWS)
    index = {row.tobytes(): i for i, row in enumerate(states.astype(np.uint8))}
    which = np.array([index[row.tobytes()] for row in d['states']])
    assert np.max(np.abs(d['logl'] + d['log_prior'] - joint[which])) < 1e-12
    print(f"{name} {kind}: {len(p)} profiles, largest |count - N p| / bound = {worst:.3f}")


def test_T1():
    rng = np.random.default_rng(1)
    model = C.random_model(rng, 3, 8)
    x = C.random_traj(rng, 1)
    prior = DC.make_prior('markov', rng, 3, 4)
    W, F = C.tables(model, x)
    d = DDO.draws(W, F, prior, rng.random((N_DRAWS, 1)))
    assert np.all(d['n_switches'] == 0) and np.all(d['n_uniforms'] == 1) and d['states'].shape == (N_DRAWS, 1)
    logw = prior.log_init + prior.log_surv[:, 0] + F[:, 1]
    p = np.exp(logw - np.logaddexp.reduce(logw))
    check_counts(np.bincount(d['states'][:, 0], minlength=3), p, N_DRAWS)
    assert np.array_equal(d['logl'], F[d['states'][:, 0], 1])
    assert np.array_equal(d['log_prior'], (prior.log_init + prior.log_surv[:, 0])[d['states'][:, 0]])


def test_absorbing_state_and_minimum_length():
    rng = np.random.default_rng(2)
    T = 12
    model = C.random_model(rng, 3, T + 4)
    x = C.random_traj(rng, T, (4,))
    W, F = C.tables(model, x)
    prior = DC.absorbing_prior(rng, T)
    B, G = DDO.backward(W, F, prior)
    assert np.all(G[1:T, 2] == -np.inf) and G[T, 2] == 0 and np.all(np.isfinite(G[1:T, :2]))
    d = DDO.draws(W, F, prior, rng.random((5000, 2 * T - 1)))
    st = d['states'].astype(int)
    assert np.all(d['n_switches'] >= 0) and np.any(st == 2)
    # nothing follows state 2, 0 -> 2 never happens, and the log prior is that of `log_prob`
    assert not np.any((st[:, :-1] == 2) & (st[:, 1:] != 2)) and not np.any((st[:, :-1] == 0) & (st[:, 1:] == 2))
    assert np.max(np.abs(d['log_prior'] - np.array([prior.log_prob(row) for row in st]))) == 0
    # the minimum-length prior of dwell_cases: no completed segment of one frame
    prior = DC.make_prior('minlength', rng, 3, T)
    d = DDO.draws(W, F, prior, rng.random((5000, 2 * T - 1)))
    draws = bild_amd.ExactDwellDraws(T, d['states'], d['n_switches'], d['logl'], d['log_prior'], d['n_uniforms'], None)
    for s in range(3):
        lengths = draws.dwell_lengths(s)
        assert len(lengths) and np.min(lengths) >= 2
    assert any(np.min(draws.dwell_lengths(s, completed=False)) == 1 for s in range(3))      # a censored last frame is allowed
    assert np.all(np.isfinite(d['log_prior']))


def test_replay_with_too_few_uniforms():
    model, x, prior = build('s2_gapfree', 'markov')
    W, F = C.tables(model, x)
    T = len(x)
    u = np.random.default_rng(3).random((2000, 2 * T - 1))
    full = DDO.draws(W, F, prior, u)
    for width in (1, 2, 3, 6):
        cut = DDO.draws(W, F, prior, u[:, :width])
        fits = full['n_uniforms'] <= width
        assert fits.any() and not fits.all()
        assert np.array_equal(cut['states'][fits], full['states'][fits]) and np.array_equal(cut['n_uniforms'][fits], full['n_uniforms'][fits])
        assert np.all(cut['states'][~fits] == 255) and np.all(cut['n_uniforms'][~fits] == -1) and np.all(cut['n_switches'][~fits] == -1)
        assert np.all(np.isnan(cut['logl'][~fits])) and np.all(np.isnan(cut['log_prior'][~fits]))


def test_no_profile_of_positive_weight():
    model, x, prior = build('s2_gapfree', 'markov')
    W, F = C.tables(model, x)
    F = np.full_like(F, np.nan)
    d = DDO.draws(W, F, prior, np.full((3, 5), 0.5))
    assert np.all(d['states'] == 255) and np.all(d['n_switches'] == -1) and np.all(d['n_uniforms'] == 0) and np.all(np.isnan(d['logl']))


def test_draws_helpers():
    states = np.array([[0, 0, 1, 1, 1, 0], [1, 1, 1, 1, 1, 1], [0, 1, 0, 1, 1, 1], [255] * 6], dtype=np.uint8)[:3]
    padded = np.concatenate([states, np.full((3, 2), 255, dtype=np.uint8)], axis=1)       # rows of a longer T_max
    d = bild_amd.ExactDwellDraws(6, padded, [2, 0, 3], np.zeros(3), np.zeros(3), [5, 1, 7], None)
    assert len(d) == 3 and d.T == 6 and d.uniforms is None and np.array_equal(d.states(), states)
    assert [list(p[:]) for p in d.profiles()] == states.tolist()
    seg_start, seg_state = d.segments()
    assert seg_start.shape == (3, 4) and np.array_equal(states_from_segments(seg_start, seg_state, 6), states)
    assert d.dwell_lengths(0).tolist() == [2, 1, 1] and d.dwell_lengths(0, completed=False).tolist() == [2, 1, 1, 1]
    assert d.dwell_lengths(1).tolist() == [3, 1] and d.dwell_lengths(1, completed=False).tolist() == [3, 6, 1, 3]
    assert d.dwell_lengths(2).tolist() == []
    empty = bild_amd.ExactDwellDraws(6, np.zeros((0, 6), dtype=np.uint8), [], [], [], [], None)
    assert len(empty) == 0 and empty.states().shape == (0, 6) and empty.profiles() == [] and len(empty.dwell_lengths(0)) == 0


def results(model, x, prior, nan='propagate', log_evidence=-12.5, n_nan_windows=0):
    return bild_amd.ExactDwellResults(traj=x, model=model, prior=prior, nan=nan, log_evidence=log_evidence, map_profile=None,
                                      map_log_joint=np.nan, log_marginal_posterior=None, expected_jumps=None, expected_stay=None,
                                      n_nan_windows=n_nan_windows)


def test_refusals_come_before_any_upload(monkeypatch):
    def no_upload(*a, **k):
        raise AssertionError("a trajectory set was made")
    monkeypatch.setattr(_lib, 'GaussTrajSetHandle', no_upload)
    rng = np.random.default_rng(3)
    model = C.random_model(rng, 2, 24)
    x = C.random_traj(rng, 20)
    prior = DC.symmetric_chain(0.1, 20)
    r = results(model, x, prior)
    for bad in ('x', None, 3, (model, x)):
        with pytest.raises(TypeError):
            bild_amd.exact_dwell_draw(bad, 4)
    with pytest.raises(TypeError):
        bild_amd.exact_dwell_draw([r, 'x'], 4)
    per_k = bild_amd.ExactSamplingResults(x, model, 0, [0.0], [0.0], [0.0], [1], [0], [[0]], [[0]], None)
    with pytest.raises(TypeError):      # the results of `exact_sample` have `exact_draw`
        bild_amd.exact_dwell_draw(per_k, 4)
    with pytest.raises(ValueError, match='one model'):
        bild_amd.exact_dwell_draw([r, results(C.random_model(rng, 2, 24), x, prior)], 4)
    with pytest.raises(ValueError, match='one prior'):
        bild_amd.exact_dwell_draw([r, results(model, x, DC.symmetric_chain(0.1, 20))], 4)
    for bad_n in (-1, 2.5, True, '3'):
        with pytest.raises(ValueError, match='n = '):
            r.draw(bad_n)
    for bad_keep in (-1, 1.5, True):
        with pytest.raises(ValueError, match='keep_uniforms'):
            r.draw(4, keep_uniforms=bad_keep)
    for shape in ((5, 9), (4,), (4, 0), (1, 4, 9)):
        with pytest.raises(ValueError, match='uniforms has shape'):
            r.draw(4, uniforms=np.zeros(shape))
    with pytest.raises(ValueError, match='uniforms has shape'):
        bild_amd.exact_dwell_draw([r, r], 4, uniforms=np.zeros((4, 9)))
    u = np.full((4, 10), 0.5)
    for bad_u in (1.0, np.nan, -1e-9):
        u[2, 3] = bad_u
        with pytest.raises(ValueError, match=r'\[0, 1\)'):
            r.draw(4, uniforms=u)
    with pytest.raises(ValueError, match="nan='omit'"):
        results(model, x, prior, log_evidence=np.nan, n_nan_windows=3).draw(4)
    with pytest.raises(ValueError, match="nan='omit'"):
        bild_amd.exact_dwell_draw([r, results(model, x, prior, log_evidence=np.nan, n_nan_windows=1)], 4)
    with pytest.raises(ValueError, match='-inf'):
        results(model, x, prior, log_evidence=-np.inf).draw(4)
    with pytest.raises(ValueError, match='-inf'):
        results(model, x, prior, log_evidence=-np.inf).posterior_distance(n=10)
    assert bild_amd.exact_dwell_draw([], 4) == []
    # n = 0: empty draws, still no device work; NaN windows are no obstacle under nan='omit'
    d = results(model, x, prior, nan='omit', n_nan_windows=3).draw(0)
    assert isinstance(d, bild_amd.ExactDwellDraws) and len(d) == 0 and d.states().shape == (0, 20) and d.uniforms is None
    both = bild_amd.exact_dwell_draw([r, r], 0, keep_uniforms=5)
    assert len(both) == 2 and both[1].uniforms.shape == (0, 5)
    assert len(model._trajsets) == 0


@pytest.mark.parametrize('name', list(DDC.REPLAY_CASES))
def test_gpu_replay_inputs_are_not_fragile(name):
    """ a condition on the GPU test's inputs: the oracle alone flags none of their draws (expectation ~2 DELTA per pick) """
    want = DDC.oracle_replay(name)
    S, T = DDC.REPLAY_CASES[name][:2]
    n = DDC.n_replay(name)
    assert n in (1024, DDC.N_REPLAY)
    assert not want['fragile'].any()
    assert np.all(want['n_switches'] >= 0) and np.array_equal(want['n_uniforms'], 1 + 2 * want['n_switches'])
    assert want['states'].shape == (n, T) and np.all(want['states'] < S)
    if S == 1:
        assert np.all(want['n_switches'] == 0) and np.all(want['states'] == 0)     # one profile, one uniform a draw
    elif T > 3:
        assert len(np.unique(want['states'], axis=0)) > n // 20


@pytest.mark.parametrize('j', [1, 5])
def test_gpu_six_trajectory_inputs(j):
    """ a condition on the GPU test's inputs: the oracle excuses at most one of a trajectory's draws """
    want = DDC.oracle_six(j)
    T = DC.RAGGED[j][0]
    assert want['states'].shape == (DDC.N_SIX, T) and np.all(want['states'] < 4) and want['fragile'].sum() <= 1
    assert np.all(want['n_switches'] >= 0) and len(np.unique(want['states'], axis=0)) > DDC.N_SIX // 20
