"""
The tools of the table read-out (tests/gauss_table_cases.py) without a GPU: `tables_fast` against `gauss_oracle.tables`,
the row builders against `logl_tables` and the reference loop `logl_reference` on expanded profiles, and the claim that
the full row set reads every entry of the tables.
"""
import numpy as np
import pytest

import gauss_oracle as G
import gauss_table_cases as C


def _pattern_case(T, i):
    """ S = 2, d = 2, both orders in both dimensions; pattern i in dimension 0 and pattern i + 1 in dimension 1 """
    rng = np.random.default_rng(100 * T + i)
    msd, inf, mean, order, x = C.model_arrays(rng, 2, 2, T, C.DESIGNED_ORDERS)
    names = (C.PATTERNS[i], C.PATTERNS[(i + 1) % len(C.PATTERNS)])
    return msd, inf, mean, order, C.apply_patterns(rng, x, names)


@pytest.mark.parametrize('T', [1, 2, 3, 65, 257])
@pytest.mark.parametrize('i', range(len(C.PATTERNS)), ids=C.PATTERNS)
def test_tables_fast_against_tables(T, i):
    # `tables` agrees with the reference loop to 2e-14 ... 4e-14 relative on two-switch profiles at T = 257 and 513, so
    # 1e-12 max(1, |entry|) leaves two orders of margin
    msd, inf, mean, order, x = _pattern_case(T, i)
    W, F = G.tables(msd, inf, mean, order, x)
    Wf, Ff = C.tables_fast(msd, inf, mean, order, x)
    worst = 0.0
    for got, want in ((Wf, W), (Ff, F)):
        assert got.shape == want.shape
        assert np.array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        if ok.any():
            worst = max(worst, float(np.max(np.abs(got[ok] - want[ok]) / np.maximum(1.0, np.abs(want[ok])))))
    print(f"\nT = {T}, {C.PATTERNS[i]}: worst {worst:.2g}")
    assert worst <= 1e-12
    assert np.all(np.isfinite(Ff))


def test_tables_fast_does_not_use_the_native_library(monkeypatch):
    from bild_amd import _lib

    def refuse(*a, **k):
        raise AssertionError("tables_fast called into the native library")

    monkeypatch.setattr(_lib, 'lib', refuse)
    msd, inf, mean, order, x = _pattern_case(17, 4)
    W, F = C.tables_fast(msd, inf, mean, order, x)
    assert W.shape == (2, 17, 18) and F.shape == (2, 18)


@pytest.mark.parametrize('S,T', [(1, 9), (2, 11), (3, 9), (4, 7), (2, 1), (3, 2), (2, 3)])
def test_rows_against_expanded_profiles(S, T):
    # the indices a - 1 and b of a row against the decomposition's own walk and the reference loop
    rng = np.random.default_rng(10 * S + T)
    msd, inf, mean, order, x = C.model_arrays(rng, S, 2, T)
    x = C.apply_patterns(rng, x, ('none', 'iid10'))
    order[:, 1] = 1                 # gaps in an ss_order-1 dimension only: every profile is finite
    W, F = G.tables(msd, inf, mean, order, x)
    rw = C.rows(T, S)
    got = rw.evaluate(W, F)
    n1 = S
    n2 = S * (T - 1) if S > 1 else 0
    n3 = S * (T - 1) * (T - 2) // 2 if S > 1 else 0
    assert len(rw) == n1 + n2 + n3
    start, state = rw.segments()
    assert start.dtype == np.int32 and start.shape == (len(rw), 3) and np.all(start[:, 0] == 0)
    assert np.all(np.diff(start, axis=1) >= 0) and np.all(start[:, 1:] >= 1)
    for r in range(len(rw)):
        st = rw.expanded(r)
        assert len(st) == T
        assert len(G.intervals(st)) == rw.kind[r], rw.name(r)
        # the segments are the profile's runs, padded at T
        iv = G.intervals(st)
        assert [t0 for t0, _, _ in iv] + [T] * (3 - len(iv)) == list(start[r]), rw.name(r)
        assert [n for _, _, n in iv] == list(state[r, :len(iv)]), rw.name(r)
        assert got[r] == pytest.approx(G.logl_tables(W, F, st), rel=1e-13, abs=1e-13), rw.name(r)
        ref = G.logl_reference(msd, inf, mean, order, x, st)
        assert np.isfinite(ref)
        assert abs(got[r] - ref) <= 1e-11 * abs(ref) + 1e-9, rw.name(r)


def test_row_names_state_the_entries():
    rw = C.rows(6, 3)
    r = int(np.nonzero((rw.kind == 3) & (rw.a == 2) & (rw.b == 4) & (rw.states[:, 1] == 0))[0][0])
    assert rw.name(r) == "K1=3 starts (0, 2, 4) states (1, 0, 2): F[1][2] + W[0][1][4] + W[2][3][6]"


@pytest.mark.parametrize('S,T', [(2, 1), (2, 2), (2, 3), (2, 40), (3, 17), (4, 9)])
def test_full_rows_read_every_entry(S, T):
    # every W[s][a - 1][b] of an interval [a, b), 1 <= a < b <= T, and every F[s][b], 1 <= b <= T; nothing else
    rw = C.rows(T, S)
    cW, cF = C.touched(rw)
    a1, b = np.meshgrid(np.arange(T), np.arange(T + 1), indexing='ij')      # a1 = a - 1
    readable = b >= a1 + 2
    assert np.all(cW[:, readable] >= 1) and np.all(cW[:, ~readable] == 0)
    assert np.all(cF[:, 1:] >= 1) and np.all(cF[:, 0] == 0)
    # every state in every role
    if T >= 3:
        for role in range(3):
            assert set(rw.states[rw.kind == 3, role]) == set(range(S))
    # no row sums more than three entries, and neighbours differ: the walk reads a boundary between equal states as none
    k3 = rw.kind == 3
    assert np.all(rw.states[k3, 0] != rw.states[k3, 1]) and np.all(rw.states[k3, 1] != rw.states[k3, 2])
    k2 = rw.kind == 2
    assert np.all(rw.states[k2, 0] != rw.states[k2, 1])


def test_restricted_rows():
    T, S = 30, 2
    full = C.rows(T, S)
    part = C.rows(T, S, a_sel=[1, 5, T - 2], b_sel=[2, 17])
    key = lambda rw: set(zip(rw.kind, map(tuple, rw.states), rw.a, rw.b))
    assert key(part) <= key(full)
    k3 = part.kind == 3
    assert np.all(np.isin(part.a[k3], [1, 5, T - 2]) | np.isin(part.b[k3], [2, 17]))
    for a in (1, 5, T - 2):         # a chosen a with every b
        assert set(part.b[k3 & (part.a == a) & (part.states[:, 1] == 0)]) == set(range(a + 1, T))
    for b in (2, 17):               # a chosen b with every a
        assert set(part.a[k3 & (part.b == b) & (part.states[:, 1] == 1)]) == set(range(1, b))
    assert np.sum(part.kind == 2) == np.sum(full.kind == 2) and np.sum(part.kind == 1) == S


def test_sweep_cases_cover_the_lengths_and_patterns():
    cases = [C.sweep_case(seed) for seed in range(40)]
    assert {c['T'] for c in cases} == set(C.SWEEP_T)
    assert {c['mode'] for c in cases} == {'zero', 'one', 'random'}
    assert {p for c in cases for p in c['patterns']} == set(C.PATTERNS)
    assert {c['S'] for c in cases} == {1, 2, 3, 4} and {c['d'] for c in cases} == {1, 2, 3, 4}
    for c in cases[:13]:
        for st in C.sweep_profiles(c['rng'], c['T'], c['S'], c['x']):
            assert st.shape == (c['T'],) and st.min() >= 0 and st.max() < c['S']
