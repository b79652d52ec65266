"""
Every entry of GenericGaussianModel's interval tables (csrc/gauss.hip, csrc/gauss.cpp: `build_one`) against the NumPy
oracle, read out through `logL_segments` by rows that sum at most three entries each (tests/gauss_table_cases.py), at
the data-dependent branches of the build: the trailing gap-free run and its shared factor, dimensions with 0, 1 or 2
valid frames, the centred first-interval row of ss_order 0, lengths at the 256-lane stride, more factorisation jobs than
scratch slots at T = 2048, the offsets of a ragged set and of a set beyond 2^31 entries; a seeded sweep that also runs
the consumers that factor windows themselves (`kalman`, `logL_sensitivities`) and the (s, theta) entry; the segment
recursion at the edges of its tile.

The bar of every row is the one of tests/test_gpu_gauss.py, |got - want| <= 1e-11 |want| + 1e-8, with identical NaN
patterns.  `-s` prints per case the rows compared, the share of NaN rows and the worst deviation.

The oracle must be finite in at least 95 % of the rows of a case, so that a read-out cannot pass on NaN alone.  Exempt
are the cases whose missing frames force NaN (`gauss_table_cases.forces_nan`): a dimension in which some state has
ss_order 0 and which has V <= 2 valid frames, or has gaps on a trajectory below T = 127.  A later ss_order-0 window is NaN
unless it contains a valid frame, which makes 99.6 % (V = 0), 62 % (V = 1) and 50 % (V = 2) of the rows of the designed
cases NaN in the oracle: the issue names the first two as NaN cases, the third is one by the same construction.  In every
case, exempt or not, the oracle's NaN rows must be exactly those that the missing frames predict
(`gauss_table_cases.expected_nan`, which does not look at the tables), and the exempt designed cases state their number
of finite rows.
"""
import os
import time

import numpy as np
import pytest

import gauss_kalman_oracle as GK
import gauss_oracle as G
import gauss_sensitivity_oracle as GS
import gauss_table_cases as C
import segment_cases as SC
from gauss_table_cases import model_from
from test_gpu_gauss import st_batch
from test_gpu_gauss_kalman import ALL, compare
from test_gpu_gauss_sensitivity import _rel, random_derivs
from test_gpu_segment_dp import check_against_oracle

pytestmark = pytest.mark.gpu


def compare_rows(got, want, names, label, nan_case=False, predicted=None):
    """
    rows against the oracle under the bar; names: row index -> text with the entries' indices; predicted: the NaN rows
    as the missing frames give them.  -> worst |diff|
    """
    assert got.shape == want.shape
    nan = np.isnan(want)
    if predicted is not None:
        assert np.array_equal(nan, predicted), f"{label}: the oracle's NaN rows are not those the missing frames predict"
    share = float(nan.mean())
    differs = np.nonzero(np.isnan(got) != nan)[0]
    assert len(differs) == 0, (f"{label}: NaN pattern differs in {len(differs)} rows, first {names(differs[0])}: "
                               f"got {got[differs[0]]}, want {want[differs[0]]}")
    ok = np.nonzero(~nan)[0]
    err = np.abs(got[ok] - want[ok])
    bar = 1e-11 * np.abs(want[ok]) + 1e-8
    w = int(np.argmax(err / bar)) if len(ok) else 0
    worst = float(err[w]) if len(ok) else 0.0
    print(f"\n{label}: {len(want)} rows, {100 * share:.3g} % NaN, worst |diff| {worst:.3g}"
          + (f" ({err[w] / bar[w]:.2g} of the bar, {names(ok[w])})" if len(ok) else ""))
    if not nan_case:
        assert share <= 0.05, f"{label}: {100 * share:.3g} % of the oracle's rows are NaN"
    assert len(ok) == 0 or err[w] <= bar[w], (f"{label}: worst row {names(ok[w])}: got {got[ok[w]]!r}, want {want[ok[w]]!r}, "
                                             f"|diff| {err[w]:.3g} > {bar[w]:.3g}")
    return worst


def read_out(model, x, rw):
    return model.logL_segments(*rw.segments(), x)


# ------------------------------------------------------------------------------------------ a. designed, full read-out
DESIGNED_CASES = [(name, 257) for name in C.DESIGNED] + [(name, T) for T in (255, 256) for name in ('no_gaps', 'iid_10_percent')]
# Finite rows of the cases in which dimension 1 has V <= 2 valid frames (S = 2, T = 257; state 1 is ss_order 0 there, and a
# later window of state 1 is finite only if it contains a valid frame of dimension 1), out of 65 794, counted from the
# missing frames.  V = 0: the 2 K1 = 1 rows and the 256 K1 = 2 rows whose later interval is in state 0.  V = 1 (frame 128)
# and V = 2 (frames 5 and 200) add the rows whose windows of state 1 hold a valid frame.
MIN_FINITE = {'all_nan_dim1': 258, 'one_valid_dim1': 25154, 'two_valid_dim1': 32983}


@pytest.mark.parametrize('name,T', DESIGNED_CASES, ids=[f"{n}-{T}" for n, T in DESIGNED_CASES])
def test_full_readout_designed(name, T):
    msd, inf, mean, order, x = C.designed_case(name, T)
    assert np.array_equal(order, C.DESIGNED_ORDERS)
    model = model_from(msd, inf, mean, order)
    W, F = G.tables(msd, inf, mean, order, x)
    rw = C.rows(T, 2)
    want = rw.evaluate(W, F)
    assert np.all(np.isfinite(F[:, 1:]))
    sparse = C.forces_nan(T, C.DESIGNED[name], order)
    assert sparse == (name in MIN_FINITE)
    if sparse:
        assert np.sum(np.isfinite(want)) == MIN_FINITE[name]
    compare_rows(read_out(model, x, rw), want, rw.name, f"{name}, T = {T}", nan_case=sparse, predicted=C.expected_nan(rw, order, x))
    # F itself stays finite: the K1 = 1 rows, and F[s0][a] wherever the rest of the row is finite
    assert np.all(np.isfinite(want[rw.kind == 1]))


# ----------------------------------------------------------------------------------------------------- b. T = 1000
@pytest.mark.parametrize('gaps', [False, True], ids=['gap_free', 'early_gaps'])
def test_full_readout_T1000(gaps):
    rng = np.random.default_rng(1000 + gaps)
    S, d, T = 2, 3, 1000
    msd, inf, mean, order, x = C.model_arrays(rng, S, d, T, [[0, 1, 0], [1, 0, 1]])
    if gaps:        # among the first 60 frames only: 60 factorisations per state and dimension for the oracle
        x[:60][rng.random((60, d)) < 0.1] = np.nan
        x[0, 1] = np.nan
    model = model_from(msd, inf, mean, order)
    W, F = C.tables_fast(msd, inf, mean, order, x)
    rw = C.rows(T, S)
    assert len(rw) == S * (1 + (T - 1) + (T - 1) * (T - 2) // 2)
    compare_rows(read_out(model, x, rw), rw.evaluate(W, F), rw.name, f"T = 1000, {'early gaps' if gaps else 'gap-free'}")


# ----------------------------------------------------------------------------------------------------- c. T = 2048
T_MAX = 2048
A_SEL = sorted(set(range(1, 51)) | {64, 100, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1500, 2000, T_MAX - 2})
B_SEL = sorted(set(range(2, 16)) | set(range(44, 54)) | {255, 256, 257, 258, 511, 512, 513, 1023, 1024, 1025, 1026, 1535, 1536,
                                                         1537, 1791, 1792, 1793, 2000, 2044, 2045, T_MAX - 2, T_MAX - 1}
               | set(range(100, 2000, 100)) - {1000, 2000})


def limit_case(ss_order, gaps=True):
    rng = np.random.default_rng(2048 + ss_order)
    msd, inf, mean, order, x = C.model_arrays(rng, 2, 1, T_MAX, ss_order)
    if gaps:
        x[[10, 11, 12, 47]] = np.nan
    return msd, inf, mean, order, x


@pytest.mark.parametrize('ss_order', [0, 1])
def test_readout_at_the_limit_T2048(ss_order):
    # starts 0 ... 47 lie before the last gap: 48 factorisation jobs (49 with the centred first interval of ss_order 0) of
    # n ~ 2000, 33.5 MB of scratch each; 1 GiB holds 31, so the chunk loop of build_one runs twice
    assert len(A_SEL) == 64 and len(B_SEL) == 64
    assert set(range(1, 50)) | {1, 1023, 1024, 1025, T_MAX - 2} <= set(A_SEL)
    msd, inf, mean, order, x = limit_case(ss_order)
    model = model_from(msd, inf, mean, order)
    t0 = time.perf_counter()
    W, F = C.tables_fast(msd, inf, mean, order, x)
    took = time.perf_counter() - t0
    rw = C.rows(T_MAX, 2, a_sel=A_SEL, b_sel=B_SEL)
    assert np.sum(rw.kind == 1) == 2 and np.sum(rw.kind == 2) == 2 * (T_MAX - 1)
    compare_rows(read_out(model, x, rw), rw.evaluate(W, F), rw.name, f"T = 2048, ss_order {ss_order} (oracle {took:.1f} s)")
    assert took < 60.0, f"tables_fast took {took:.1f} s"


# ------------------------------------------------------------------------------------------------------ d. ragged set
def test_ragged_set():
    lengths = (1, 2, 65, 257, 64, 3)
    rng = np.random.default_rng(65257)
    msd, inf, mean, order, _ = C.model_arrays(rng, 2, 2, max(lengths), C.DESIGNED_ORDERS)
    model = model_from(msd, inf, mean, order)
    trajs, sets, want = [], [], []
    for T in lengths:
        x = np.cumsum(rng.normal(size=(T, 2)), axis=0)
        if T >= 64:
            x = C.apply_patterns(rng, x, ('iid10', 'iid10'))
        trajs.append(x)
        rw = C.rows(T, 2)
        sets.append(rw)
        want.append(rw.evaluate(*G.tables(msd[:, :, :T], inf, mean, order, x)))
    start = np.concatenate([rw.segments()[0] for rw in sets])
    state = np.concatenate([rw.segments()[1] for rw in sets])
    tid = np.concatenate([np.full(len(rw), j, dtype=np.int32) for j, rw in enumerate(sets)])
    owner = np.concatenate([np.arange(len(rw)) for rw in sets])
    got = model.logL_segments(start, state, trajs, tid)
    names = lambda r: f"trajectory {tid[r]} (T = {lengths[tid[r]]}), {sets[tid[r]].name(owner[r])}"
    compare_rows(got, np.concatenate(want), names, "ragged set T = (1, 2, 65, 257, 64, 3)")
    for j, (x, rw) in enumerate(zip(trajs, sets)):
        alone = read_out(model, x, rw)
        assert alone.tobytes() == got[tid == j].tobytes(), f"trajectory {j} (T = {lengths[j]}) differs from its own set"


# ---------------------------------------------------------------------------------- T = 2048 gap-free: solve jobs only
def test_gap_free_T2048_first_and_last_windows():
    # every start is a solve job on the one shared factor of n = 2047, the longest the solve kernel's LDS vector holds
    msd, inf, mean, order, x = limit_case(1, gaps=False)
    model = model_from(msd, inf, mean, order)
    rw = C.rows(T_MAX, 2, a_sel=[], b_sel=[])          # the K1 <= 2 rows
    assert np.all(rw.kind <= 2) and len(rw) == 2 * T_MAX
    W, F = C.tables_fast(msd, inf, mean, order, x)
    compare_rows(read_out(model, x, rw), rw.evaluate(W, F), rw.name, "T = 2048 gap-free, K1 <= 2")


# --------------------------------------------------------------------------------------------- e. offsets beyond 2^31
def test_offsets_beyond_2_to_31():
    # The table of a set passes 2^31 doubles.  513 copies of a gap-free T = 2048 trajectory would do, but their build
    # runs 1026 factorisations of n = 2047 on one workgroup each and did not finish in seven minutes; the offsets do not
    # depend on the length, so the set is 16 070 copies of a gap-free T = 257 trajectory (S = 4, d = 1; 17.2 GB).
    import torch
    S, T, copies = 4, 257, 16070
    free, _ = torch.cuda.mem_get_info()
    if free < 48e9:
        pytest.skip(f"{free / 1e9:.1f} GB of device memory free; the 17.2 GB table and its build need 48 GB")
    rng = np.random.default_rng(2 ** 31 % 1000)
    msd, inf, mean, order, x = C.model_arrays(rng, S, 1, T, [[0], [1], [0], [1]])
    model = model_from(msd, inf, mean, order)
    rw = C.rows(T, S)
    single = read_out(model, x, rw)
    compare_rows(single, rw.evaluate(*G.tables(msd, inf, mean, order, x)), rw.name, "T = 257 gap-free, set of one")
    per_traj = S * (T * (T + 1) // 2 + T + 1)
    assert copies * per_traj > 2 ** 31 > (copies // 2 + 1) * per_traj       # the middle member starts below, the last beyond
    trajs = [x.copy() for _ in range(copies)]
    members = (0, copies // 2, copies - 1)
    start, state = rw.segments()
    tid = np.repeat(np.array(members, dtype=np.int32), len(rw))
    t0 = time.perf_counter()
    got = model.logL_segments(np.tile(start, (3, 1)), np.tile(state, (3, 1)), trajs, tid)
    nbytes, _ = model.trajset(trajs).info()
    print(f"\n{copies} copies: table of {nbytes / 1e9:.1f} GB, built and read in {time.perf_counter() - t0:.1f} s")
    assert nbytes == 8 * copies * per_traj
    for i, j in enumerate(members):
        assert got[i * len(rw):(i + 1) * len(rw)].tobytes() == single.tobytes(), f"member {j} differs from the set of one"
    model.invalidate()


# -------------------------------------------------------------------------------------------------- f. seeded sweep
def _nansum_rows(terms, ll):
    flat = terms.reshape(len(terms), -1)
    return np.array([np.sum(r[~np.isnan(r)]) if not np.isnan(l) else np.nan for r, l in zip(flat, ll)])


# BILD_FUZZ_SEEDS=<n> replaces the number of seeds, as in tests/test_gpu_fuzz.py
@pytest.mark.parametrize('seed', range(int(os.environ.get('BILD_FUZZ_SEEDS', '40'))))
def test_sweep(seed):
    from bild_amd.profiles import segments_from_st, states_from_segments
    c = C.sweep_case(seed)
    S, d, T, x, rng = c['S'], c['d'], c['T'], c['x'], c['rng']
    msd, inf, mean, order = c['msd'], c['inf'], c['mean'], c['order']
    label = f"seed {seed}: S = {S}, d = {d}, T = {T}, ss_orders {c['mode']}, missing {'/'.join(c['patterns'])}"
    model = model_from(msd, inf, mean, order)

    # the full read-out
    W, F = G.tables(msd, inf, mean, order, x)
    rw = C.rows(T, S)
    assert len(rw) == (1 if S == 1 else S * (1 + (T - 1) + (T - 1) * (T - 2) // 2))
    exempt = C.forces_nan(T, c['patterns'], order)
    predicted = C.expected_nan(rw, order, x)
    assert np.sum(~predicted) >= S          # the K1 = 1 rows at the least: F is always finite
    compare_rows(read_out(model, x, rw), rw.evaluate(W, F), rw.name, label, nan_case=exempt, predicted=predicted)

    # the consumers that factor windows themselves, on six candidates
    states = np.stack(C.sweep_profiles(rng, T, S, x))
    arrs = (model.msd, model.msd_inf, model.mean, model.ss_order)
    ll = model.logL_batch(states, x)
    want_ll = np.array([G.logl_tables(W, F, st) for st in states])
    # (six rows: the cap would allow no NaN at all, and two adjacent switches inside a gap are NaN in any seed; the NaN
    # candidates are instead held to those the missing frames predict)
    predicted = np.array([C.expected_nan_profile(st, order, x) for st in states])
    compare_rows(ll, want_ll, lambda r: f"candidate {r}", label + ", candidates", nan_case=True, predicted=predicted)
    res = model.kalman(states, x, outputs=ALL)
    xscale = float(np.nanmax(np.abs(x))) if np.any(~np.isnan(x)) else 1.0
    compare(res, GK.batch(*arrs, [x], list(states)), xscale, label + ", kalman")
    ok = ~np.isnan(ll)
    total = _nansum_rows(res.terms, ll)
    if ok.any():
        assert np.max(np.abs(total[ok] - ll[ok]) / np.maximum(1.0, np.abs(ll[ok]))) < 1e-10, label

    P = int(rng.integers(0, 5))
    dm = random_derivs(rng, model, P)
    sl, grad, fisher = model.logL_sensitivities(states, x, **dm)
    ol, og, oF = GS.batch(*arrs, [x], list(states), **dm)
    assert grad.shape == (len(states), P) and fisher.shape == (len(states), P, P)
    assert np.array_equal(np.isnan(sl), ~ok) and np.array_equal(np.isnan(ol), ~ok), label
    assert np.all(np.isnan(grad[~ok])) and np.all(np.isnan(fisher[~ok])), label
    if ok.any():
        e = (_rel(sl[ok], ol[ok]), _rel(sl[ok], ll[ok]), _rel(grad[ok], og[ok]), _rel(fisher[ok], oF[ok]))
        print(f"sensitivities P = {P}: logL {e[0]:.2g} (oracle) {e[1]:.2g} (table), grad {e[2]:.2g}, fisher {e[3]:.2g}")
        assert e[0] < 1e-10 and e[1] < 1e-10 and e[2] < 1e-8 and e[3] < 1e-8, (label, e)

    # the (s, theta) entry against the expansion of its rows
    k = int(rng.integers(0, 5))
    if S > 1:
        ss, thetas = st_batch(rng, 50, k, S)
    else:
        ss, thetas = rng.dirichlet(np.ones(k + 1), size=50), np.zeros((50, k + 1), dtype=np.int64)
    expanded = states_from_segments(*segments_from_st(ss, thetas, T), T)
    assert model.logL_st_batch(ss, thetas, x).tobytes() == model.logL_batch(expanded, x).tobytes(), label


# ------------------------------------------------------------------------------- g. the tile of the segment recursion
@pytest.mark.parametrize('T', [63, 65, 127, 129])
def test_segment_recursion_at_tile_edges(T):
    import bild_amd
    rng = np.random.default_rng(7000 + T)
    model = SC.random_model(rng, 2, T + 8)
    x = SC.random_traj(rng, T, (T // 3, (2 * T) // 3))       # isolated missing frames: nothing is NaN
    t0 = time.perf_counter()
    res, out = SC.oracle_arrays(model, x, 4)
    W, F = SC.tables(model, x)
    print(f"\nT = {T}: oracle {time.perf_counter() - t0:.1f} s")
    r = bild_amd.exact_sample(x, model, k_max=4)
    check_against_oracle(r, res, out, model, x, W, F, same_map=False)
    assert np.all(np.isfinite(r.evidence))
