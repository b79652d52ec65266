"""
Every compiled configuration of the likelihood kernels against the oracle -- not only the ones the automatic choice picks for
the workloads of the other files.

* The vector kernels (kernels.hip): each geometry of `BILD_GEOMETRIES`, parsed out of the source so that a geometry added
  later is swept too, is forced with BILD_GEOM on chains of its padded row count (unreduced, n = NP and the smallest n that
  pads to NP), error patterns whose mean vectors fit it, the three flavours (all frames valid, missing frames, external
  force), frame by frame (T = 1, 2, 150), with tables split and unsplit, and on the dense path (BILD_DENSE_VALU=1).
  BILD_Q_LAST_GEOMETRY confirms every forced run; the geometries of one chain length must agree bit for bit (launch.cpp,
  geometry_for), the split launch must agree bit for bit with the single one, and tables built while another geometry is
  forced must give the same bits.  Once per chain length a batch large enough to wrap the grid-stride loop.
* The LDS-resident kernel (wide.hip) at odd chain lengths and at each width (BILD_WIDE_THREADS), the modal tile kernel
  (modal_mfma.hip) on and off its padding rows, the dense matrix-pipe kernel (dense_mfma.hip) from a single mode on.

Switches are flipped inside the process with bild_config_reload and restored behind each use.  `-s` prints the worst
|delta logL| of every (geometry, path, launch kind, flavour) and the (geometry, path) pairs that forcing refuses by design.
"""
import collections
import contextlib
import os
import re

import numpy as np
import pytest

import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = os.path.join(ROOT, 'bild_amd', 'csrc', 'kernels.hip')
TOL = 1e-8
KDMAX = 3          # mean vectors a task carries at most (common.h: kDMax)
MAX_BLOCKS = 256 * 16   # grid of a launch that does not split (launch.cpp); a larger batch wraps the grid-stride loop


# ---- the geometry table -------------------------------------------------------------------------------------------------

class Geom(collections.namedtuple('Geom', 'id NP CPL G W OCC LAY MODES')):
    @property
    def mean_slots(self):
        return min(self.CPL * self.G - self.NP, KDMAX)

    @property
    def tasks_per_wave(self):
        return 64 // self.G

    def forcible(self, path):
        """ the rule of geometry_for: a forced geometry serves the paths of its last field, 0 counting as modal """
        return bool((self.MODES or 2) & (1 if path == 'dense' else 2))


def parse_geometries(path=KERNELS):
    text = open(path).read()
    body = re.search(r'#define BILD_GEOMETRIES\(X\)\s*\\\n((?:[^\n]*\\\n)*[^\n]*\n)', text).group(1)
    row_occ = int(re.search(r'#define BILD_ROW_OCC (\d+)', text).group(1))
    geoms = []
    for fields in re.findall(r'X\(([^)]*)\)', body):
        f = [v.strip() for v in fields.split(',')]
        geoms.append(Geom(*(row_occ if v == 'BILD_ROW_OCC' else int(v) for v in f)))
    return geoms


GEOMS = parse_geometries()
NPS = sorted({g.NP for g in GEOMS})


def padded_rows(n):
    """ kernels.hip: padded_rows -- the first listed geometry with room for n rows """
    return next((g.NP for g in GEOMS if g.NP >= n), 0)


def smallest_n(NP):
    return 2 if NP == 4 else min(n for n in range(1, NP + 1) if padded_rows(n) == NP)


# (geometry, path) pairs that no run can reach, with the reason.  Forcing one of them is refused: the automatic choice serves
# the launch, and the test asserts that it did.  Written out, so that the forcing rule of geometry_for and this list are checked
# against each other (test_geometry_table_parses).
_DENSE_ONLY = 'dense-only geometry (last field 1): several columns per lane, which the modal frame loop spills'
_MODAL_ONLY = 'modal-only geometry (last field 2): the row layout / its packed twin of the modal frame loop'
_BLOCK = 'block layout (last field 0): a modal layout, S on the matrix pipe; never on the dense path'
_LEAN = 'lean frame loop of split launches (last field 0): a modal layout; never on the dense path'
UNREACHABLE = {
    (7, 'dense'): _MODAL_ONLY, (9, 'dense'): _MODAL_ONLY, (21, 'dense'): _MODAL_ONLY, (22, 'dense'): _MODAL_ONLY,
    (8, 'modal'): _DENSE_ONLY, (10, 'modal'): _DENSE_ONLY, (11, 'modal'): _DENSE_ONLY,
    (15, 'dense'): _BLOCK, (16, 'dense'): _BLOCK,
    (23, 'dense'): _LEAN, (24, 'dense'): _LEAN, (25, 'dense'): _LEAN,
}


def test_geometry_table_parses():
    """ (CPU) the parse of BILD_GEOMETRIES the GPU sweep relies on """
    assert len(GEOMS) == 26
    assert len({g.id for g in GEOMS}) == len(GEOMS)
    assert sorted(g.id for g in GEOMS) == list(range(26))
    for g in GEOMS:
        assert g.CPL * g.G - g.NP >= 1, g
        assert padded_rows(g.NP) == g.NP, g
        assert 64 % g.G < g.G and g.W >= 1 and g.OCC >= 1 and 0 <= g.LAY <= 4 and 0 <= g.MODES <= 3, g
    # the row counts the CPU build's stubs list (asan_stubs.cpp) are the same
    stubs = open(os.path.join(ROOT, 'bild_amd', 'csrc', 'asan_stubs.cpp')).read()
    listed = [int(v) for v in re.search(r'rows\[\] = \{([^}]*)\}', stubs).group(1).split(',')]
    assert listed == NPS
    # every pair the sweep cannot run is listed, and nothing else
    for g in GEOMS:
        for path in ('modal', 'dense'):
            assert ((g.id, path) in UNREACHABLE) == (not g.forcible(path)), (g, path)


def test_padded_rows_match_the_library():
    """ (CPU) the library pads an unreduced chain of n modes to the parsed padded_rows(n) (model creation is host-only) """
    from bild_amd import _lib
    for n in range(2, 33):
        a = H.DuckModel(N=n, d=1).arrays()
        h = _lib.ModelHandle(a['B'], a['G'], a['Sig'], a['M0'], a['C0'], H.end2end(n), reduce=False)
        assert h.query(_lib.Q_NEFF) == n
        assert h.query(_lib.Q_NP) == padded_rows(n), n
        assert h.query(_lib.Q_LAST_GEOMETRY) == -1


# ---- references ---------------------------------------------------------------------------------------------------------

def textbook(a, w, err, x, states):
    """
    The Kalman filter of the model as this library defines it -- M <- B M + G, C <- B C B^T + Sig, each dimension on its own
    -- for every row of `states` at once.  The reference's kernels read B as symmetric; this one serves the non-symmetric
    models of the dense path (and is held to the oracle on symmetric ones below).
    """
    B, G, Sig, M0, C0 = (a[k] for k in ('B', 'G', 'Sig', 'M0', 'C0'))
    states = np.atleast_2d(states)
    n, T = states.shape
    tot = np.zeros(n)
    for j in range(x.shape[1]):
        M = M0[states[:, 0], :, j].copy()
        C = C0[states[:, 0]].copy()
        for t in range(T):
            if t > 0:
                Bt = B[states[:, t]]
                M = np.einsum('rij,rj->ri', Bt, M) + G[states[:, t], :, j]
                C = Bt @ C @ Bt.transpose(0, 2, 1) + Sig[states[:, t]]
            if np.isnan(x[t, 0]):
                continue
            Cw = C @ w
            S = Cw @ w + err[j] ** 2
            nu = x[t, j] - M @ w
            tot += -0.5 * (nu * nu / S + np.log(S) + np.log(2 * np.pi))
            M = M + Cw * (nu / S)[:, None]
            C = C - Cw[:, :, None] * Cw[:, None, :] / S[:, None, None]
    return tot


def test_textbook_filter_agrees_with_the_oracle():
    """ (CPU) the textbook filter above against the oracle on a symmetric model: force, missing frames, distinct errors """
    from oracle import oracle
    rng = np.random.default_rng(5)
    c = make_case(7, 'd3x', 'force', 80, rng=rng)
    want = oracle.logl_batch(c.a, c.w, c.err, c.x, c.states)
    assert np.max(np.abs(textbook(c.a, c.w, c.err, c.x, c.states) - want)) < 1e-9


# ---- inputs -------------------------------------------------------------------------------------------------------------

# error patterns: (d, localization errors, mean vectors of a covariance chain)
PATTERNS = {
    'd1': (1, [0.1], 1),
    'd2': (2, [0.15, 0.15], 2),
    'd3': (3, [0.1, 0.1, 0.1], 3),
    'd3x': (3, [0.08, 0.12, 0.2], 1),     # three distinct errors: d* = 3 chains of one mean vector each
}
FLAVOURS = ('valid', 'masked', 'force')
K1 = 6


def segment_batch(rng, T, n=61):
    """
    About 60 rows of segment lists (K1 = 6, two states): no switch, switches at frame 1 and T - 1, two switches one frame
    apart, chains of three and more close switches (the frame loop runs behind the table walk), random rows.  Switches at
    or beyond T are segments outside the trajectory (the kernels drop them).
    """
    t = max(T // 3, 1)
    fixed = [[], [], [1], [T - 1], [1, T - 1], [1, 2], [T - 2, T - 1], [t, t + 1], [t, t + 1, t + 2], [t, t + 2, t + 4],
             [t, t + 1, t + 2, t + 3, t + 4], [t, t + 3, t + 7, t + 9, t + 12], [1, 2, 3], [T - 4, T - 3, T - 2, T - 1],
             [2 * t, 2 * t + 1, 2 * t + 3], [5, 40, 41, 42, T - 1]]
    rows = []
    for i in range(n):
        if i < len(fixed):
            sw = fixed[i]
        elif i % 3 == 0:            # a cluster of close switches somewhere
            c = int(rng.integers(1, max(T - 1, 2)))
            sw = list(c + np.cumsum(rng.integers(1, 4, size=int(rng.integers(3, 6)))) - 1)
        else:
            sw = sorted(rng.choice(np.arange(1, max(T, 2)), size=int(rng.integers(1, 6)), replace=True))
        sw = sorted({min(int(v), T) for v in sw if v >= 1})[:K1 - 1]
        s0 = i % 2
        starts = [0] + sw + [T] * (K1 - 1 - len(sw))
        states = [(s0 + min(j, len(sw))) % 2 for j in range(K1)]
        rows.append((starts, states))
    seg_start = np.array([r[0] for r in rows], dtype=np.int32)
    seg_state = np.array([r[1] for r in rows], dtype=np.int32)
    return seg_start, seg_state


class Case:
    """ a model, a trajectory and a batch, with the oracle's answer (computed once, shared by every geometry) """

    def __init__(self, a, w, err, x, seg_start, seg_state, asym=False):
        from bild_amd.profiles import states_from_segments
        self.a, self.w, self.err, self.x = a, w, np.asarray(err, dtype=float), x
        self.seg_start, self.seg_state = seg_start, seg_state
        self.states = states_from_segments(seg_start, seg_state, len(x))
        self.asym = asym
        self._want = None
        self._handle = None
        self._shared = None

    @property
    def want(self):
        if self._want is None:
            if self.asym:
                self._want = textbook(self.a, self.w, self.err, self.x, self.states)
            else:
                from oracle import oracle
                self._want = oracle.logl_batch(self.a, self.w, self.err, self.x, self.states)
        return self._want

    def handle(self):
        from bild_amd import _lib
        if self._handle is None:
            a = self.a
            self._handle = _lib.ModelHandle(a['B'], a['G'], a['Sig'], a['M0'], a['C0'], self.w, reduce=False)
        return self._handle

    def trajset(self):
        from bild_amd import _lib
        return _lib.TrajSetHandle(self.handle(), [self.x], [self.err])

    def shared(self):
        """ one set for every geometry, its tables built at a first evaluation under the automatic choice """
        from bild_amd import _lib
        if self._shared is None:
            with switches(BILD_GEOM=-1):
                ts = self.trajset()
                _lib.logl_segments(self.handle(), ts, self.seg_start, self.seg_state, path='modal')
            assert _lib.prefix_info(ts)[0] > 0
            self._shared = ts
        return self._shared


def model_arrays(n, d, force=False, asym=False):
    duck = H.DuckModel(N=n, d=d)
    if force:                    # as test_gpu_parity's N40_force: a force on the two end beads
        for mi, mod in enumerate(duck.models):
            mod.F[0, :] = [0.5, -0.25, 0.1 * (mi + 1)][:d]
            mod.F[-1, :] = [-0.5, 0.25, -0.1 * (mi + 1)][:d]
    a = {k: v.copy() for k, v in duck.arrays().items()}
    if asym:                     # a propagator that is not symmetric (from_arrays input only): the dense path keeps NP = n
        a['B'][0, 0, 1] += 0.02
        a['B'][1, n - 1, n - 2] -= 0.015
    return duck, a


def make_case(n, pattern, flavour, T, rng=None, asym=False, rows=61):
    d, err, _ = PATTERNS[pattern]
    rng = np.random.default_rng([n, d, len(err), FLAVOURS.index(flavour), T, int(asym)]) if rng is None else rng
    duck, a = model_arrays(n, d, force=flavour == 'force', asym=asym)
    missing = []
    if flavour == 'masked' and T > 1:
        missing = [0] + list(range(T // 3, min(T // 3 + 45, T))) + list(np.nonzero(rng.random(T) < 0.05)[0])
    elif flavour == 'force' and T > 2:
        missing = list(np.nonzero(rng.random(T) < 0.05)[0][1:])
    truth = H.random_profile(rng, T, 2, max(T // 4, 1))
    x = np.asarray(H.synth_trajectory(duck, truth, err, rng, missing=sorted(set(missing)))[:], dtype=float)
    seg_start, seg_state = segment_batch(rng, T, rows)
    return Case(a, H.end2end(n), err, x, seg_start, seg_state, asym=asym)


_CASES = {}


def case(n, pattern, flavour, T, asym=False, rows=61):
    key = (n, pattern, flavour, T, asym, rows)
    if key not in _CASES:
        _CASES[key] = make_case(n, pattern, flavour, T, asym=asym, rows=rows)
    return _CASES[key]


# ---- switches -----------------------------------------------------------------------------------------------------------

@contextlib.contextmanager
def switches(**env):
    """ BILD_* switches set for the body (bild_config_reload), the previous environment restored behind it """
    from bild_amd import _lib
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    _lib.config_reload()
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        _lib.config_reload()


@pytest.fixture
def clean_switches(built_lib):
    """ no switch of this file leaks into the next test, whatever happens in this one """
    from bild_amd import _lib
    names = ('BILD_GEOM', 'BILD_DENSE_VALU', 'BILD_WIDE_THREADS')
    assert not any(k in os.environ for k in names)
    yield
    for k in names:
        os.environ.pop(k, None)
    _lib.config_reload()


# ---- the report ---------------------------------------------------------------------------------------------------------

WORST = collections.defaultdict(float)   # (geometry id, path, launch kind, flavour) -> worst |delta logL|
RAN = set()                              # geometry ids confirmed by BILD_Q_LAST_GEOMETRY
DONE = set()


def run(c, path, ts=None, **kw):
    """ one launch of case c; returns (logL, the geometry that ran) """
    from bild_amd import _lib
    h = c.handle()
    got = _lib.logl_segments(h, c.trajset() if ts is None else ts, c.seg_start, c.seg_state, path=path, **kw)
    return got, h.query(_lib.Q_LAST_GEOMETRY)


def check(c, got, tag):
    err = float(np.max(np.abs(got - c.want)))
    assert np.all(np.isfinite(got)) and err < TOL, (tag, err)
    WORST[tag] = max(WORST[tag], err)


def jumps_refused(g):
    """ the block layout (15 / 16) runs frame by frame only (kernels.hip, geometry_for): with tables forcing it is refused """
    return g.LAY == 1


def sweep_modal(g, c, flavour, out):
    """ frame by frame, split with tables, unsplit with tables, tables built while g is forced; results into `out` """
    from bild_amd import _lib
    got, ran = run(c, 'modal', prefix=False)
    assert ran == g.id, (g, ran)
    check(c, got, (g.id, 'modal', 'frames', flavour))
    out['frames'] = got
    if len(c.x) < 150:
        return

    def forced(ran):
        return ran != g.id if jumps_refused(g) else ran == g.id

    shared = c.shared()
    split, ran = run(c, 'modal', ts=shared)
    assert forced(ran), (g, ran)
    check(c, split, (g.id, 'modal', 'split', flavour))
    unsplit, ran = run(c, 'modal', ts=shared, split=False)
    assert forced(ran), (g, ran)
    check(c, unsplit, (g.id, 'modal', 'unsplit', flavour))
    # the split launch (table walk, frame loop over the work lists) adds the same numbers in the same order as the single launch
    assert np.array_equal(split, unsplit), (g, flavour, np.max(np.abs(split - unsplit)))
    # a fresh set whose tables are built while g is forced (builders take the automatic geometry: the same tables); its first
    # launch builds them and reads no transient state table yet -- its chains run from their first switch, with the same bits
    fresh = c.trajset()
    first, _ = run(c, 'modal', ts=fresh)
    again, ran = run(c, 'modal', ts=fresh)
    assert forced(ran) and _lib.prefix_info(fresh)[0] > 0
    check(c, first, (g.id, 'modal', 'first', flavour))
    assert np.array_equal(again, split), (g, flavour)
    assert np.array_equal(first, unsplit), (g, flavour, np.max(np.abs(first - unsplit)))
    if not jumps_refused(g):
        out['split'], out['unsplit'] = split, unsplit


def sizes(NP):
    return sorted({NP, smallest_n(NP)})


def patterns_for(g):
    """ the error patterns whose mean vectors fit g; three distinct errors (three chains, the costliest oracle) where one fits """
    return [p for p, (_, _, means) in PATTERNS.items() if means <= g.mean_slots and (p != 'd3x' or g.mean_slots == 1)]


@pytest.mark.gpu
@pytest.mark.parametrize('NP', NPS)
def test_vector_geometries(clean_switches, NP):
    """
    Every geometry of one padded row count, forced in turn on the modal path (frame by frame, tables split and unsplit) and
    the dense vector path, against the oracle; the geometries of the chain length agree bit for bit with each other.
    """
    geoms = [g for g in GEOMS if g.NP == NP]
    results = collections.defaultdict(dict)      # (path, kind, n, pattern, flavour, T) -> {geometry id: logL}
    for g in geoms:
        with switches(BILD_GEOM=g.id):
            for n in sizes(NP):
                for pattern in patterns_for(g):
                    for flavour in FLAVOURS:
                        for T in (1, 2, 150):
                            if T < 150 and flavour == 'masked':
                                continue                      # (frame 0 is the missing one)
                            c = case(n, pattern, flavour, T)
                            out = {}
                            if g.forcible('modal'):
                                sweep_modal(g, c, flavour, out)
                                RAN.add(g.id)
                            for kind, got in out.items():
                                results[('modal', kind, n, pattern, flavour, T)][g.id] = got
            if g.forcible('dense'):
                with switches(BILD_DENSE_VALU=1):
                    for n in sizes(NP):
                        for pattern in patterns_for(g):
                            for flavour in FLAVOURS:
                                for T in (2, 150):
                                    if T < 150 and flavour == 'masked':
                                        continue
                                    c = case(n, pattern, flavour, T, asym=NP % 4 != 0)
                                    got, ran = run(c, 'dense')
                                    assert ran == g.id, (g, ran)
                                    check(c, got, (g.id, 'dense', 'frames', flavour))
                                    results[('dense', 'frames', n, pattern, flavour, T)][g.id] = got
                                    RAN.add(g.id)
        # the pairs refused by design: the automatic choice serves the launch, and the query shows it
        for path in ('modal', 'dense'):
            if g.forcible(path):
                continue
            c = case(NP, patterns_for(g)[0], 'valid', 150, asym=path == 'dense' and NP % 4 != 0)
            with switches(BILD_GEOM=g.id, BILD_DENSE_VALU=1):
                got, ran = run(c, path, prefix=False)
            assert ran != g.id and ran in {h.id for h in geoms if h.forcible(path)}, (g, path, ran)
            check(c, got, (g.id, path, 'refused', 'valid'))
    # all geometries of the chain length agree bit for bit, on both paths (launch.cpp relies on it when it picks the geometry of a
    # split launch; a result must not depend on the size of the batch it is part of), but for the block layout (15 / 16), which
    # sums S in another order (kernels.hip, at BILD_GEOMETRIES)
    same = {g.id for g in geoms if g.LAY != 1}
    for key, by_geom in results.items():
        ids = sorted(i for i in by_geom if i in same)
        for i in ids[1:]:
            assert np.array_equal(by_geom[i], by_geom[ids[0]]), (key, ids[0], i, np.max(np.abs(by_geom[i] - by_geom[ids[0]])))
    DONE.add(NP)
    _report(NP)


def _report(NP):
    ids = {g.id for g in GEOMS if g.NP == NP}
    print(f'\nNP = {NP}: worst |logL - oracle| per (geometry, path, launch kind, flavour)')
    for key in sorted(k for k in WORST if k[0] in ids):
        print('  %3d  %-5s  %-8s  %-6s  %.2e' % (key + (WORST[key],)))


def _report_family(name):
    print(f'\n{name}: worst |logL - oracle|')
    for key in sorted(k for k in WORST if k[0] == name):
        print('  ' + '  '.join(str(v) for v in key[1:]) + '  %.2e' % WORST[key])


def automatic_geometry(NP, path, ntasks, means):
    """
    geometry_for without BILD_GEOM, restated: of the geometries with room for `means` mean vectors that the path may pick (one
    column per lane: only the tightest fit), the first whose waves are all resident at once (1024 x OCC), else the one with the
    fewest rounds of resident waves x (columns per lane + per-frame overhead: 2 modal, 0 dense)
    """
    best, best_cost = None, 0
    for c in GEOMS:
        if c.NP != NP or c.mean_slots < means or not (c.MODES & (1 if path == 'dense' else 2)):
            continue
        if best is not None and best.CPL == 1 and c.CPL == 1:
            continue
        waves = -(-ntasks // c.tasks_per_wave)
        slots = 1024 * c.OCC
        if waves <= slots:
            return c.id
        cost = -(-waves // slots) * (c.CPL + (0 if path == 'dense' else 2))
        if best is None or cost < best_cost:
            best, best_cost = c, cost
    return best.id


def test_automatic_geometry_of_the_wrap_batches():
    """ (CPU) the restated rule picks a geometry with several columns per lane for one of the wrap batches (NP = 12) """
    picks = {NP: automatic_geometry(NP, 'modal', wrap_rows(NP), 1) for NP in NPS}
    assert any(next(g for g in GEOMS if g.id == i).CPL > 1 for i in picks.values()), picks


def wrap_rows(NP):
    """ a batch that wraps the grid-stride loop of an unsplit launch in any geometry of the chain length """
    return MAX_BLOCKS * max(4 * g.tasks_per_wave for g in GEOMS if g.NP == NP and g.MODES & 2) + 37


@pytest.mark.gpu
@pytest.mark.parametrize('NP', NPS)
def test_grid_stride_wrap(clean_switches, NP):
    """
    A batch too large for one grid of the unsplit launch (256 x 16 workgroups): the automatic choice, ~100 rows against the
    oracle, and a permutation of the batch gives the permuted results bit for bit.
    """
    from bild_amd import _lib
    from oracle import oracle
    n_rows = wrap_rows(NP)
    T, n = 40, smallest_n(NP)
    rng = np.random.default_rng(NP)
    c = make_case(n, 'd1', 'masked', T, rng=rng, rows=8)
    starts = np.sort(rng.integers(1, T, size=(n_rows, 3)), axis=1)
    c.seg_start = np.concatenate([np.zeros((n_rows, 1), int), starts], axis=1).astype(np.int32)
    c.seg_state = ((rng.integers(2, size=(n_rows, 1)) + np.arange(4)[None, :]) % 2).astype(np.int32)
    ts = c.trajset()
    got, ran = run(c, 'modal', ts=ts, split=False)
    assert ran == automatic_geometry(NP, 'modal', n_rows, 1), ran
    RAN.add(ran)
    print(f'\nNP = {NP}: {n_rows} rows ran in geometry {ran}')
    pick = rng.choice(n_rows, 100, replace=False)
    from bild_amd.profiles import states_from_segments
    want = oracle.logl_batch(c.a, c.w, c.err, c.x, states_from_segments(c.seg_start[pick], c.seg_state[pick], T))
    assert np.max(np.abs(got[pick] - want)) < TOL
    perm = rng.permutation(n_rows)
    c.seg_start, c.seg_state = c.seg_start[perm], c.seg_state[perm]
    again, ran2 = run(c, 'modal', ts=ts, split=False)
    assert ran2 == ran and np.array_equal(again, got[perm])


# ---- the other kernel families ------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('threads', [256, 512, 1024])
def test_lds_resident_kernel(clean_switches, threads):
    """ wide.hip at odd chain lengths and its edges (n = 128 at 256 lanes: one row slice per workgroup), each width """
    with switches(BILD_WIDE_THREADS=threads):
        for n in (41, 63, 69, 91, 101, 127, 128):
            c = case(n, 'd3x' if n % 2 else 'd2', 'masked' if n < 100 else 'force', 40, rows=8)
            for prefix in (False, True):
                got, ran = run(c, 'modal', prefix=prefix)
                assert ran == -1
                check(c, got, ('wide', threads, n, prefix))
    _report_family('wide')


@pytest.mark.gpu
@pytest.mark.parametrize('flavour', FLAVOURS)
def test_modal_tile_kernel(clean_switches, flavour):
    """ modal_mfma.hip (36 / 40 padded rows) on and off its padding rows """
    for n in (33, 35, 36, 37, 39, 40):
        c = case(n, 'd3', flavour, 150)
        for prefix in (False, True):
            got, ran = run(c, 'modal', prefix=prefix)
            assert ran == -1
            check(c, got, ('tiles', flavour, n, prefix))
    _report_family('tiles')


@pytest.mark.gpu
@pytest.mark.parametrize('flavour', FLAVOURS)
def test_dense_matrix_pipe(clean_switches, flavour):
    """ dense_mfma.hip from a single mode (NP = 4) on, across the padding rows of its 4 x 4 tiles """
    from bild_amd import _lib
    for n in (1, 4, 5, 9, 13, 17, 21, 24):
        c = case(n, 'd3' if n > 1 else 'd2', flavour, 150)
        assert c.handle().query(_lib.Q_NP) == padded_rows(n)
        got, ran = run(c, 'dense')
        assert ran == -1
        check(c, got, ('dense_mfma', flavour, n))
    _report_family('dense_mfma')


@pytest.mark.gpu
def test_every_geometry_ran(built_lib):
    """ all geometries of the table confirmed by BILD_Q_LAST_GEOMETRY (when the whole sweep ran in this process) """
    if DONE != set(NPS):
        pytest.skip('the geometry sweep did not run in full in this process')
    print('\n(geometry, path) pairs not run -- forcing refused by design:')
    for (gid, path), why in sorted(UNREACHABLE.items()):
        print(f'  {gid:3d}  {path:5s}  {why}')
    assert RAN == {g.id for g in GEOMS}, sorted({g.id for g in GEOMS} - RAN)
