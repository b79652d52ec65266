"""
CPU tests that hold the ctypes binding (bild_amd/_lib.py) to include/bild_amd.h: the ``bild_*_out`` structures field for
field, every prototype argument for argument, and the routing of the exact-inference wrappers' arguments into the positions
the header names.  The library is not called: the routing test replaces it by a recorder.
"""
import ctypes
import os
import re
import types

import numpy as np

from bild_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCALARS = {'int': ctypes.c_int, 'unsigned': ctypes.c_uint, 'double': ctypes.c_double, 'int32_t': ctypes.c_int32,
           'uint32_t': ctypes.c_uint32, 'int64_t': ctypes.c_int64, 'uint64_t': ctypes.c_uint64}
DTYPES = {'double': np.float64, 'int64_t': np.int64, 'int32_t': np.int32, 'int': np.int32, 'uint8_t': np.uint8}
N_OUT_STRUCTS, N_PROTOTYPES = 13, 107
EXACT_CALL = r'bild_(gauss_dwell_\w+|gauss_segment_\w+|(gauss_)?exact_evidence)$'


def _header():
    """ include/bild_amd.h without its comments """
    text = open(os.path.join(ROOT, 'include', 'bild_amd.h')).read()
    return re.sub(r'//[^\n]*', '', re.sub(r'/\*.*?\*/', '', text, flags=re.S))


def _declarations(text):
    """ 'const double *a, *b' or 'int64_t n' -> [(name, C type without const, is a pointer)] """
    base, rest = re.match(r'\s*((?:const\s+)?\w+)\s*(.*)$', text, flags=re.S).groups()
    out = []
    for d in rest.split(','):
        stars, name = re.match(r'\s*([\s*]*)(\w+)\s*$', d).groups()
        out.append((name, base.replace('const', '').strip(), '*' in stars))
    return out


def header_out_structs():
    """ {struct name: [(field, C element type, is a pointer)]} of every ``typedef struct bild_*_out`` """
    found = re.findall(r'typedef\s+struct\s+(bild_\w+_out)\s*\{(.*?)\}\s*(\w+)\s*;', _header(), flags=re.S)
    assert all(tag == name for tag, _, name in found)
    return {tag: [f for part in body.split(';') if part.strip() for f in _declarations(part)] for tag, body, _ in found}


def header_prototypes():
    """ {function: (return type, [(parameter, C type, is a pointer)])} of every prototype """
    text = re.sub(r'typedef\s+(struct|enum)\s*\w*\s*\{.*?\}\s*\w+\s*;', '', _header(), flags=re.S)
    text = '\n'.join(line for line in text.splitlines() if not line.lstrip().startswith('#'))
    out = {}
    for ret, name, args in re.findall(r'([\w\s*]+?)\b(bild_\w+)\s*\(([^()]*)\)\s*;', text):
        assert name not in out, name
        params = [] if args.strip() in ('', 'void') else [_declarations(a)[0] for a in args.split(',')]
        out[name] = (' '.join(ret.split()), params)
    return out


def _class_of(struct):
    """ bild_dwell_lengths_out -> _lib.DwellLengthsOut """
    return getattr(_lib, ''.join(part.capitalize() for part in struct.split('_')[1:]))


def _is_pointer(t):
    return t in (ctypes.c_void_p, ctypes.c_char_p) or (isinstance(t, type) and issubclass(t, ctypes._Pointer))


# ---------------------------------------------------------------- the 13 wrappers on a recorder in place of the library

S, T, L, K_MAX, P = 2, [1, 5], 5, 3, 2


class Recorder:
    """ stands for the loaded library: the exact-inference functions record their arguments and return BILD_OK """

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not re.match(EXACT_CALL, name):
            raise AttributeError(name)
        return lambda *args: self.calls.append((name, args)) or 0


def record_wrappers(monkeypatch):
    """
    every exact-inference wrapper called once or twice on stand-ins -> [(label, function, {parameter: value recorded}, the
    out structure, the dict returned, what the caller gave)]
    """
    rec = Recorder()
    monkeypatch.setattr(_lib, 'lib', lambda: rec)
    model = types.SimpleNamespace(_h=0x1000, S=S, d=1, Tmax=7)
    ts = types.SimpleNamespace(_h=0x2000, n_traj=len(T), T=np.array(T, dtype=np.int32))
    rng = np.random.default_rng(0)
    tables = (np.zeros(S), np.zeros((S, S)), np.zeros((S, L)), np.zeros((S, L)))
    trajs = [rng.normal(size=(t, 1)) for t in T]
    tr = np.ones((S, S), dtype=bool)
    derivs = dict(dmsd=np.ones((P, S, 1, 8)), dmsd_inf=np.ones((P, S, 1)), dmean=np.ones((P, S, 1)))
    draw_traj, draw_k = np.array([0, 1, 1], dtype=np.int32), np.array([0, 2, 1], dtype=np.int32)
    prior_k = np.zeros((len(T), K_MAX + 1))
    dwell = dict(L=L, T_max=max(T), log_init=tables[0], log_jump=tables[1], log_dwell=tables[2], log_surv=tables[3])
    cases = [
        ('exact_evidence', lambda: _lib.exact_evidence(model, ts, 2, tr, marginals=True, max_profiles=1e6, scratch_bytes=11, path='dense'),
         dict(k=2, max_profiles=1e6, scratch_bytes=11, T_max=max(T), flags=_lib.PATH_DENSE), ()),
        ('exact_evidence gauss', lambda: _lib.exact_evidence(model, ts, 1, tr, marginals=False, scratch_bytes=12, gauss=True),
         dict(k=1, max_profiles=2.0 ** 32, scratch_bytes=12, T_max=max(T)), ('log_post',)),
        ('segment_evidence', lambda: _lib.gauss_segment_evidence(model, ts, K_MAX, tr, marginals=True, omit=True, scratch_bytes=13),
         dict(k_max=K_MAX, T_max=max(T), flags=1, scratch_bytes=13), ()),
        ('segment_evidence no marginals', lambda: _lib.gauss_segment_evidence(model, ts, K_MAX, tr, marginals=False),
         dict(k_max=K_MAX, T_max=max(T), flags=0, scratch_bytes=0), ('log_post',)),
        ('segment_draw', lambda: _lib.gauss_segment_draw(model, ts, K_MAX, tr, draw_traj, draw_k, seed=2 ** 64 + 5, scratch_bytes=14),
         dict(k_max=K_MAX, T_max=max(T), scratch_bytes=14, n_draws=3, draw_traj=draw_traj, draw_k=draw_k, uniforms=None, seed=5), ()),
        ('segment_sensitivities', lambda: _lib.gauss_segment_sensitivities(model, ts, trajs, K_MAX, tr, log_k_prior=prior_k, P=P, omit=True,
                                                                             scratch_bytes=15, **derivs),
         dict(k_max=K_MAX, flags=1, log_k_prior=prior_k, P=P, scratch_bytes=15), ()),
        ('segment_sensitivities P = 0', lambda: _lib.gauss_segment_sensitivities(model, ts, trajs, K_MAX, tr, fisher=False),
         dict(k_max=K_MAX, flags=0, log_k_prior=None, P=0, scratch_bytes=0), ('grad', 'fisher')),
        ('segment_sensitivities P = 0 fisher', lambda: _lib.gauss_segment_sensitivities(model, ts, trajs, K_MAX, tr),
         dict(P=0), ('grad', 'fisher')),
        ('dwell_evidence', lambda: _lib.gauss_dwell_evidence(model, ts, *tables, marginals=True, omit=True, scratch_bytes=21),
         dict(dwell, flags=1, scratch_bytes=21), ()),
        ('dwell_evidence no marginals', lambda: _lib.gauss_dwell_evidence(model, ts, *tables, marginals=False),
         dict(dwell, flags=0, scratch_bytes=0), ('log_post', 'exp_jumps', 'exp_stay')),
        ('dwell_sensitivities', lambda: _lib.gauss_dwell_sensitivities(model, ts, trajs, *tables, P=P, omit=True, scratch_bytes=22, **derivs),
         dict({k: v for k, v in dwell.items() if k != 'T_max'}, flags=1, P=P, scratch_bytes=22), ()),
        ('dwell_sensitivities P = 0', lambda: _lib.gauss_dwell_sensitivities(model, ts, trajs, *tables, fisher=False),
         dict(L=L, flags=0, P=0, scratch_bytes=0), ('grad', 'fisher')),
        ('dwell_sensitivities P = 0 fisher', lambda: _lib.gauss_dwell_sensitivities(model, ts, trajs, *tables), dict(P=0), ('grad', 'fisher')),
        ('dwell_lengths', lambda: _lib.gauss_dwell_lengths(model, ts, *tables, omit=True, scratch_bytes=23),
         dict(dwell, flags=1, scratch_bytes=23), ()),
        ('dwell_switch_counts', lambda: _lib.gauss_dwell_switch_counts(model, ts, *tables, K_MAX, omit=False, scratch_bytes=24),
         dict(dwell, k_max=K_MAX, flags=0, scratch_bytes=24), ()),
        ('dwell_first_contact', lambda: _lib.gauss_dwell_first_contact(model, ts, *tables, 2, omit=True, scratch_bytes=25),
         dict(dwell, target=2, flags=1, scratch_bytes=25), ()),
        ('dwell_occupancy', lambda: _lib.gauss_dwell_occupancy(model, ts, *tables, 1, omit=False, scratch_bytes=26),
         dict(dwell, target=1, flags=0, scratch_bytes=26), ()),
        ('dwell_filter', lambda: _lib.gauss_dwell_filter(model, ts, *tables, run_max=4, omit=True, scratch_bytes=27),
         dict(dwell, run_max=4, flags=1, scratch_bytes=27), ()),
        ('dwell_filter run_max = 0', lambda: _lib.gauss_dwell_filter(model, ts, *tables),
         dict(dwell, run_max=0, flags=0, scratch_bytes=0), ('log_run',)),
        ('dwell_lag', lambda: _lib.gauss_dwell_lag(model, ts, *tables, 3, omit=True, scratch_bytes=28),
         dict(dwell, lag=3, flags=1, scratch_bytes=28), ()),
        ('dwell_draw', lambda: _lib.gauss_dwell_draw(model, ts, *tables, draw_traj, keep_uniforms=6, seed=7, scratch_bytes=29),
         dict(dwell, scratch_bytes=29, n_draws=3, draw_traj=draw_traj, draw_stream=None, U=6, uniforms=None, seed=7), ()),
        ('dwell_draw without uniforms', lambda: _lib.gauss_dwell_draw(model, ts, *tables, draw_traj),
         dict(dwell, scratch_bytes=0, n_draws=3, U=0, seed=0), ('uniforms_out',)),
        # an empty output is NULL in the sensitivity calls alone: elsewhere NULL means "not asked for"
        ('dwell_draw of no draw', lambda: _lib.gauss_dwell_draw(model, ts, *tables, draw_traj[:0], keep_uniforms=2),
         dict(dwell, n_draws=0, U=2), ()),
    ]
    prototypes = header_prototypes()
    out = []
    for label, call, given, null in cases:
        before = len(rec.calls)
        res = call()
        assert len(rec.calls) == before + 1, label
        name, args = rec.calls[-1]
        names = [p[0] for p in prototypes[name][1]]
        assert len(args) == len(names), label
        named = dict(zip(names, args))
        assert named['m'] == model._h and named['ts'] == ts._h, label
        out.append((label, name, named, named['out']._obj, res, given, set(null)))
    assert {name for _, name, *_ in out} == {n for n in prototypes if re.match(EXACT_CALL, n)}     # 14 functions, 13 wrappers
    return out


def test_out_structs_match_header(monkeypatch):
    """
    every pointer-only ``bild_*_out`` of the header has its ctypes class with the same fields in the same order, and the arrays
    the wrappers allocate for the fields have the C element type
    """
    structs = {tag: fields for tag, fields in header_out_structs().items() if all(f[2] for f in fields)}
    assert len(structs) == N_OUT_STRUCTS, sorted(structs)
    for tag, fields in structs.items():
        cls = _class_of(tag)
        assert [f[0] for f in cls._fields_] == [f[0] for f in fields], tag
        assert all(f[1] is ctypes.c_void_p for f in cls._fields_), tag
    assert [f[0] for f in _lib.KalmanOut._fields_] == [f[0] for f in header_out_structs()['bild_kalman_out']]
    seen = set()
    for label, name, named, spec, res, given, null in record_wrappers(monkeypatch):
        tag = next(t for t in structs if _class_of(t) is type(spec))
        seen.add(tag)
        for field, ctype, _ in structs[tag]:
            a = res[field[:-len('_out')] if field not in res else field]       # (uniforms_out is returned as 'uniforms')
            assert a is None or a.dtype == DTYPES[ctype], (label, field)
    assert seen == set(structs)


def test_signatures_match_header():
    """ every prototype of the header: the argument count, the C type of every scalar, a pointer at every pointer, the return type """
    prototypes = header_prototypes()
    assert len(prototypes) == N_PROTOTYPES
    assert set(prototypes) == set(_lib._SIGNATURES)
    returns = {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'const char *': ctypes.c_char_p, 'void': None}
    for name, (ret, params) in prototypes.items():
        restype, argtypes = _lib._SIGNATURES[name]
        assert restype is returns[ret], name
        assert len(argtypes) == len(params), name
        for (pname, ctype, pointer), t in zip(params, argtypes):
            if pointer:
                assert _is_pointer(t), (name, pname)
            else:
                assert t is SCALARS[ctype], (name, pname)


def test_wrappers_route_arguments(monkeypatch):
    """
    each wrapper puts every scalar and table it is given at the position the header names, and its out structure points at the
    arrays it returns, field by field, NULL exactly where an output is not asked for
    """
    for label, name, named, spec, res, given, null in record_wrappers(monkeypatch):
        for key, want in given.items():
            got = named[key]
            if isinstance(want, np.ndarray):
                assert got == want.ctypes.data, (label, key)
            else:
                assert got == want and type(got) is type(want), (label, key, got)
        fields = [f[0] for f in spec._fields_]
        assert {f for f in fields if getattr(spec, f) is None} == null, label
        assert len(res) == len(fields), label
        for f in fields:
            a = res[f[:-len('_out')] if f not in res else f]
            if f in null:
                assert a is None or a.size == 0, (label, f)
            else:
                assert a is not None and getattr(spec, f) == a.ctypes.data, (label, f)
