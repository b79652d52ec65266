"""
ctypes binding of ``libbild_amd.so`` (C ABI: include/bild_amd.h).

There is no CPU fallback: if the shared library is missing or no GPU is usable, every
evaluation raises.  (The reference's warn-and-fall-back shim, bild/cython_imports.py:3-7,
is deliberately *not* mirrored: a silent fallback would void the parity claims.)
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# BILD_AMD_LIB selects an alternative build of the same ABI (kernel A/B experiments, tools/ab.py)
LIB_PATH = os.environ.get('BILD_AMD_LIB') or os.path.join(_HERE, 'libbild_amd.so')

OK, ERR_INVALID, ERR_HIP, ERR_NO_DEVICE, ERR_UNSUPPORTED, ERR_NOMEM = range(6)

PATH_AUTO, PATH_DENSE, PATH_MODAL = 0, 1, 2
PATHS = {'auto': PATH_AUTO, 'dense': PATH_DENSE, 'modal': PATH_MODAL}
MODEL_NO_REDUCE = 1
VALIDATE_DEVICE = 0x10
NO_PREFIX = 0x20
NO_JUMP = 0x40
NO_SPLIT = 0x80
NO_STATES = 0x100
NO_TAIL = 0x200
NO_SWITCH_TAIL = 0x400

Q_N, Q_D, Q_S, Q_MODAL_OK, Q_NP, Q_NEFF, Q_HAS_G, Q_LAST_GEOMETRY = range(8)
X_LAMBDA, X_SIGMA, X_Q, X_WQ, X_R, X_C0Q, X_V = range(7)


class BildAmdError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"bild_amd error {code}: {message}")
        self.code = code


class NoDeviceError(BildAmdError):
    pass


# (double* / int32* parameters are declared as addresses: a NumPy buffer is then passed as a plain integer -- dptr / iptr below --,
# which costs a third of building a typed ctypes pointer per argument; byref(...) of an output scalar is accepted as before)
_dp = ctypes.c_void_p
_ip = ctypes.c_void_p
_vp = ctypes.c_void_p

_SIGNATURES = {
    'bild_abi_version': (ctypes.c_int, []),
    'bild_config_string': (ctypes.c_char_p, []),
    'bild_config_reload': (ctypes.c_int, []),
    'bild_last_error': (ctypes.c_char_p, []),
    'bild_set_last_error': (None, [ctypes.c_char_p]),
    'bild_comm_library': (ctypes.c_int, [ctypes.c_char_p]),
    'bild_comm_unique_id': (ctypes.c_int, [ctypes.c_char_p, ctypes.c_int]),
    'bild_comm_create': (ctypes.c_int, [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(_vp)]),
    'bild_comm_allgather': (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int64, _vp]),
    'bild_comm_destroy': (ctypes.c_int, [_vp]),
    'bild_device_alloc': (ctypes.c_int, [ctypes.c_int64, ctypes.POINTER(_vp)]),
    'bild_device_free': (ctypes.c_int, [_vp]),
    'bild_device_to_host': (ctypes.c_int, [_vp, _vp, ctypes.c_int64, _vp]),
    'bild_device_count': (ctypes.c_int, [ctypes.POINTER(ctypes.c_int)]),
    'bild_model_create': (ctypes.c_int, [ctypes.c_int] * 3 + [_dp] * 6 + [ctypes.c_uint, ctypes.POINTER(_vp)]),
    'bild_model_destroy': (ctypes.c_int, [_vp]),
    'bild_model_query': (ctypes.c_int, [_vp, ctypes.c_int, ctypes.POINTER(ctypes.c_int64)]),
    'bild_model_export': (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _dp, ctypes.c_int64]),
    'bild_trajset_create': (ctypes.c_int, [_vp, ctypes.c_int, _ip, _dp, _dp, ctypes.POINTER(_vp)]),
    'bild_trajset_destroy': (ctypes.c_int, [_vp]),
    'bild_trajset_expect': (ctypes.c_int, [_vp, ctypes.c_int64]),
    'bild_logl_segments': (ctypes.c_int, [_vp, _vp, ctypes.c_int64, ctypes.c_int, _ip, _ip, _ip, ctypes.c_uint, _dp]),
    'bild_logl_st': (ctypes.c_int, [_vp, _vp, ctypes.c_int64, ctypes.c_int, _dp, _vp, _ip, ctypes.c_uint, _dp]),
    'bild_logl_st_to_device': (ctypes.c_int, [_vp, _vp, ctypes.c_int64, ctypes.c_int, _dp, _vp, _ip, ctypes.c_uint, _vp, _vp]),
    'bild_logl_st_device': (ctypes.c_int, [_vp, _vp, ctypes.c_int64, ctypes.c_int, _vp, _vp, _vp, ctypes.c_uint, _vp, _vp, _vp]),
    'bild_segments_from_st': (ctypes.c_int, [ctypes.c_int64, ctypes.c_int, ctypes.c_int, _ip, ctypes.c_int64, _dp, _vp, _ip, _ip]),
    'bild_logl_profiles': (ctypes.c_int, [_vp, _vp, ctypes.c_int64, ctypes.c_int64, _ip, _ip, ctypes.c_uint, _dp]),
    'bild_logl_segments_device': (ctypes.c_int, [_vp, _vp, ctypes.c_int64, ctypes.c_int, _vp, _vp, _vp,
                                                 ctypes.c_uint, _vp, _vp]),
    'bild_schedule_segments': (ctypes.c_int, [_vp, _vp, ctypes.c_int64, ctypes.c_int, _ip, _ip, _ip, ctypes.c_uint, _ip]),
    'bild_logl_segments_device_ordered': (ctypes.c_int, [_vp, _vp, ctypes.c_int64, ctypes.c_int, _vp, _vp, _vp, _vp,
                                                         ctypes.c_uint, _vp, _vp]),
    'bild_frames_executed': (ctypes.c_int, [_vp, _vp, ctypes.c_int64, ctypes.c_int, _ip, _ip, _ip, ctypes.c_uint, _dp, _dp]),
    'bild_frames_run_read': (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_int64)]),
    'bild_debug_frames_per_task': (ctypes.c_int, [_vp]),
    'bild_prefix_info': (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_int64), _dp]),
    'bild_flop_count': (ctypes.c_int, [_vp, _vp, ctypes.c_int64, _ip, ctypes.c_uint, _dp, _dp]),
    'bild_kernel_timing': (ctypes.c_int, [ctypes.c_int]),
    'bild_kernel_timing_read': (ctypes.c_int, [_dp, ctypes.POINTER(ctypes.c_int64), ctypes.c_char_p, ctypes.c_int]),
    'bild_kernel_timing_read_walk': (ctypes.c_int, [_dp, ctypes.POINTER(ctypes.c_int64)]),
    'bild_logl_st_status': (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_int64)]),
    # host-side AMIS bookkeeping (amis_host.cpp)
    'bild_amis_create': (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _vp, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                        _dp, _dp, ctypes.POINTER(_vp)]),
    'bild_amis_destroy': (ctypes.c_int, [_vp]),
    'bild_amis_error': (ctypes.c_char_p, [_vp]),
    'bild_amis_pool_size': (ctypes.c_int64, [_vp]),
    'bild_amis_num_proposals': (ctypes.c_int64, [_vp]),
    'bild_amis_params': (ctypes.c_int, [_vp, ctypes.c_int64, _dp, _dp]),
    'bild_amis_pool': (ctypes.c_int, [_vp, ctypes.c_int, _dp]),
    'bild_amis_restore': (ctypes.c_int, [_vp, ctypes.c_int64, _dp, _dp, ctypes.c_int64, _dp, _vp, _dp, _dp, _dp, _dp]),
    'bild_amis_sample_traces': (ctypes.c_int, [_vp, ctypes.c_int64, _dp, _vp]),
    'bild_amis_step': (ctypes.c_int, [_vp, ctypes.c_int64, _dp, _vp, _dp, _dp]),
    'bild_amis_use_device': (ctypes.c_int, [_vp, ctypes.c_int]),
    'bild_amis_step_fused': (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int64, _dp, _vp, ctypes.c_uint, _dp]),
    'bild_amis_step_device_rng': (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int64, ctypes.c_uint64, ctypes.c_uint, _dp]),
    'bild_amis_pool_samples': (ctypes.c_int, [_vp, _dp, _vp]),
    'bild_interval_marginals': (ctypes.c_int, [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int64, _ip, _ip, _dp, _dp]),
    'bild_exchange_create': (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.POINTER(_vp)]),
    'bild_exchange_handle': (ctypes.c_int, [_vp, ctypes.c_char_p]),
    'bild_exchange_connect': (ctypes.c_int, [_vp, ctypes.c_char_p]),
    'bild_exchange_allgather': (ctypes.c_int, [_vp, _vp, ctypes.c_int64, _vp, _vp]),
    'bild_exchange_status': (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_int)]),
    'bild_exchange_set_step': (ctypes.c_int, [_vp, ctypes.c_uint32]),
    'bild_exchange_set_timeout': (ctypes.c_int, [_vp, ctypes.c_double]),
    'bild_exchange_destroy': (ctypes.c_int, [_vp]),
    # the inference driver (run_host.cpp)
    'bild_run_create': (ctypes.c_int, [ctypes.c_int, _ip, ctypes.c_int, _vp, _vp, ctypes.c_int, _dp, _dp, _dp, _vp, _ip,
                                       ctypes.POINTER(_vp)]),
    'bild_run_destroy': (ctypes.c_int, [_vp]),
    'bild_run_error': (ctypes.c_char_p, [_vp]),
    'bild_run_plan': (ctypes.c_int, [_vp, _vp, ctypes.POINTER(_vp)]),
    'bild_run_round': (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint, _dp, _dp, _dp]),
    'bild_run_stage': (ctypes.c_int, [_vp, _dp, _dp]),
    'bild_run_rows': (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(_vp),
                                     ctypes.POINTER(_vp), ctypes.POINTER(_vp)]),
    'bild_run_finish': (ctypes.c_int, [_vp, _dp, _dp]),
    'bild_run_traj_info': (ctypes.c_int, [_vp, ctypes.c_int, _vp, ctypes.POINTER(ctypes.c_char_p)]),
    'bild_run_traj_log': (ctypes.c_int, [_vp, ctypes.c_int, _ip, _ip, _dp, _dp, _dp]),
    'bild_run_sampler_info': (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, _vp]),
    'bild_run_sampler_data': (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, _dp, _dp, _vp, _dp]),
    'bild_run_take_core': (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(_vp)]),
    'bild_run_totals': (ctypes.c_int, [_vp, _vp]),
    # GenericGaussianModel (gauss.cpp)
    'bild_gauss_model_create': (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, _ip, _dp, _dp, _dp, ctypes.POINTER(_vp)]),
    'bild_gauss_model_destroy': (ctypes.c_int, [_vp]),
    'bild_gauss_trajset_create': (ctypes.c_int, [_vp, ctypes.c_int, _ip, _dp, ctypes.POINTER(_vp)]),
    'bild_gauss_trajset_destroy': (ctypes.c_int, [_vp]),
    'bild_gauss_trajset_info': (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)]),
    'bild_gauss_logl_segments': (ctypes.c_int, [_vp, _vp, ctypes.c_int64, ctypes.c_int, _ip, _ip, _ip, _dp]),
    'bild_gauss_logl_st': (ctypes.c_int, [_vp, _vp, ctypes.c_int64, ctypes.c_int, _dp, _vp, _ip, _dp]),
    # Rouse trajectory generator (sim.cpp)
    'bild_rouse_simulate': (ctypes.c_int, [ctypes.c_int] * 3 + [_dp] * 7 + [ctypes.c_int, _ip, ctypes.c_int, _ip, _ip, _vp, _dp, _dp,
                                           ctypes.c_uint64, ctypes.c_int64, _dp]),
    # GenericGaussianModel trajectory generator (gauss_sim.cpp)
    'bild_gauss_simulate': (ctypes.c_int, [_vp, ctypes.c_int, _ip, ctypes.c_int, _ip, _ip, _vp, _dp, ctypes.c_uint64, ctypes.c_int64, _dp]),
    # Kalman filter and smoother (kalman.cpp)
    'bild_kalman_segments': (ctypes.c_int, [_vp, _vp, ctypes.c_int64, ctypes.c_int, _ip, _ip, _ip, _vp, ctypes.c_int64]),
    'bild_kalman_mixture': (ctypes.c_int, [_vp, _vp, ctypes.c_int64, ctypes.c_int, _ip, _ip, _ip, _dp, _dp, _dp, ctypes.c_int64]),
    # log-likelihood sensitivities (sens.cpp)
    'bild_logl_sensitivities': (ctypes.c_int, [_vp, _vp, ctypes.c_int64, ctypes.c_int, _ip, _ip, _ip, ctypes.c_int, _vp, _dp,
                                               _dp, _dp, _dp, ctypes.c_int64]),
    # GenericGaussianModel log-likelihood sensitivities (gauss_sens.cpp)
    'bild_gauss_logl_sensitivities': (ctypes.c_int, [_vp, ctypes.c_int, _ip, _dp, ctypes.c_int64, ctypes.c_int, _ip, _ip, _ip,
                                                     ctypes.c_int, _vp, _dp, _dp, _dp, ctypes.c_int64]),
    # GenericGaussianModel per-frame moments (gauss_kalman.cpp)
    'bild_gauss_kalman_segments': (ctypes.c_int, [_vp, ctypes.c_int, _ip, _dp, ctypes.c_int64, ctypes.c_int, _ip, _ip, _ip, _vp,
                                                  ctypes.c_int64]),
    'bild_gauss_kalman_mixture': (ctypes.c_int, [_vp, ctypes.c_int, _ip, _dp, ctypes.c_int64, ctypes.c_int, _ip, _ip, _ip, _dp,
                                                 _dp, _dp, ctypes.c_int64]),
    # exact evidence by enumeration (exact.cpp)
    'bild_exact_count': (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, ctypes.POINTER(ctypes.c_double)]),
    'bild_exact_evidence': (ctypes.c_int, [_vp, _vp, ctypes.c_int, _vp, ctypes.c_double, ctypes.c_int64, ctypes.c_int, ctypes.c_uint,
                                           _vp]),
    'bild_gauss_exact_evidence': (ctypes.c_int, [_vp, _vp, ctypes.c_int, _vp, ctypes.c_double, ctypes.c_int64, ctypes.c_int, _vp]),
    # exact evidence of every k by the segment recursion (gauss_segdp.cpp)
    'bild_gauss_segment_evidence': (ctypes.c_int, [_vp, _vp, ctypes.c_int, _vp, ctypes.c_int, ctypes.c_uint, ctypes.c_int64, _vp]),
    # exact posterior draws from the segment recursion's backward tables (gauss_segdraw.cpp)
    'bild_gauss_segment_draw': (ctypes.c_int, [_vp, _vp, ctypes.c_int, _vp, ctypes.c_int, ctypes.c_int64, ctypes.c_int64, _ip, _ip, _dp,
                                               ctypes.c_uint64, _vp]),
    # gradient of the exact evidence with respect to model parameters (gauss_segsens.cpp)
    'bild_gauss_segment_sensitivities': (ctypes.c_int, [_vp, _vp, _dp, ctypes.c_int, _vp, ctypes.c_uint, _dp, ctypes.c_int, _vp,
                                                        ctypes.c_int64, _vp]),
    # exact inference under a dwell-time prior (gauss_dwell.cpp)
    'bild_gauss_dwell_evidence': (ctypes.c_int, [_vp, _vp, ctypes.c_int, _dp, _dp, _dp, _dp, ctypes.c_int, ctypes.c_uint, ctypes.c_int64,
                                                 _vp]),
    # exact posterior draws under a dwell-time prior (gauss_dwelldraw.cpp)
    'bild_gauss_dwell_draw': (ctypes.c_int, [_vp, _vp, ctypes.c_int, _dp, _dp, _dp, _dp, ctypes.c_int, ctypes.c_int64, ctypes.c_int64, _ip,
                                             _vp, ctypes.c_int, _dp, ctypes.c_uint64, _vp]),
    # gradient of the exact evidence under a dwell-time prior (gauss_dwellsens.cpp)
    'bild_gauss_dwell_sensitivities': (ctypes.c_int, [_vp, _vp, _dp, ctypes.c_int, _dp, _dp, _dp, _dp, ctypes.c_uint, ctypes.c_int, _vp,
                                                      ctypes.c_int64, _vp]),
    # expected segment-length counts under a dwell-time prior (gauss_dwelllen.cpp)
    'bild_gauss_dwell_lengths': (ctypes.c_int, [_vp, _vp, ctypes.c_int, _dp, _dp, _dp, _dp, ctypes.c_int, ctypes.c_uint, ctypes.c_int64,
                                                _vp]),
    # exact online filtering under a dwell-time prior (gauss_dwellfilt.cpp)
    'bild_gauss_dwell_filter': (ctypes.c_int, [_vp, _vp, ctypes.c_int, _dp, _dp, _dp, _dp, ctypes.c_int, ctypes.c_int, ctypes.c_uint,
                                               ctypes.c_int64, _vp]),
    'bild_gauss_dwell_lag': (ctypes.c_int, [_vp, _vp, ctypes.c_int, _dp, _dp, _dp, _dp, ctypes.c_int, ctypes.c_int, ctypes.c_uint,
                                            ctypes.c_int64, _vp]),
    # exact switch counts and first-contact times under a dwell-time prior (gauss_dwellevent.cpp)
    'bild_gauss_dwell_switch_counts': (ctypes.c_int, [_vp, _vp, ctypes.c_int, _dp, _dp, _dp, _dp, ctypes.c_int, ctypes.c_int, ctypes.c_uint,
                                                      ctypes.c_int64, _vp]),
    'bild_gauss_dwell_first_contact': (ctypes.c_int, [_vp, _vp, ctypes.c_int, _dp, _dp, _dp, _dp, ctypes.c_int, ctypes.c_uint, ctypes.c_uint,
                                                      ctypes.c_int64, _vp]),
    # exact posterior of the frames in a set of states under a dwell-time prior (gauss_dwellocc.cpp)
    'bild_gauss_dwell_occupancy': (ctypes.c_int, [_vp, _vp, ctypes.c_int, _dp, _dp, _dp, _dp, ctypes.c_int, ctypes.c_uint, ctypes.c_uint,
                                                  ctypes.c_int64, _vp]),
    'bild_choice_counts': (ctypes.c_int, [ctypes.c_int64, ctypes.c_int, _dp, _dp, _dp, ctypes.c_double, _vp, _vp, _vp, _vp]),
}

# the calls of include/bild_amd_windows.h: bound by `lib()` as the table above is, and no part of `exported_symbols()`, which
# lists include/bild_amd.h
_SIGNATURES_EXT = {
    # exact window support under a dwell-time prior (gauss_dwellwin.cpp)
    'bild_gauss_dwell_windows': (ctypes.c_int, [_vp, _vp, ctypes.c_int, _dp, _dp, _dp, _dp, ctypes.c_int, ctypes.c_int64, ctypes.c_int64,
                                                _ip, _ip, _ip, _ip, ctypes.c_uint, _vp]),
}

# the calls of include/bild_amd_visits.h: bound by `lib()` as the two tables above are, and no part of `exported_symbols()`
_SIGNATURES_VISITS = {
    # exact visit counts to a set of states under a dwell-time prior (gauss_dwellvis.cpp)
    'bild_gauss_dwell_visits': (ctypes.c_int, [_vp, _vp, ctypes.c_int, _dp, _dp, _dp, _dp, ctypes.c_int, ctypes.c_int, ctypes.c_uint,
                                               ctypes.c_uint, ctypes.c_int64, _vp]),
}

_lib = None
_torch_libdir = None     # set when the library was bound to the HIP runtime of an installed PyTorch
_rccl_chosen = False


def _share_hip_runtime_with_torch():
    """
    A PyTorch-ROCm wheel ships its own HIP runtime (same soname as the system one).  Two runtimes in one process do
    not coexist: if this library brings in the system runtime first, a later ``torch.cuda`` finds "No HIP GPUs".
    So when PyTorch is installed but not loaded yet, its runtime is loaded first and the library binds to it -- the
    same arrangement as when torch is imported before bild_amd.  ``BILD_AMD_HIP_RUNTIME=system`` skips this.
    """
    import importlib.util
    import sys
    if 'torch' in sys.modules or os.environ.get('BILD_AMD_HIP_RUNTIME') == 'system':
        return
    try:
        spec = importlib.util.find_spec('torch')
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    path = os.path.join(os.path.dirname(spec.origin), 'lib', 'libamdhip64.so')
    if os.path.exists(path):
        try:
            ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
            global _torch_libdir
            _torch_libdir = os.path.dirname(path)
        except OSError:
            pass


def lib():
    """ load libbild_amd.so (raises if it has not been built) """
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                              f"or `make -C bild_amd/csrc` (there is no CPU fallback)")
        _share_hip_runtime_with_torch()
        handle = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in {**_SIGNATURES, **_SIGNATURES_EXT, **_SIGNATURES_VISITS}.items():
            fn = getattr(handle, name)
            fn.restype = restype
            fn.argtypes = argtypes
        if handle.bild_abi_version() != 2:
            raise ImportError("libbild_amd.so ABI version mismatch")
        _lib = handle
    return _lib


def config_string():
    """ the BILD_* environment switches in force, as the library read them ("" = defaults) """
    return lib().bild_config_string().decode()


def config_reload():
    """ re-read the BILD_* environment switches (tests / tools; not while evaluations are running) """
    check(lib().bild_config_reload())


def exported_symbols():
    return list(_SIGNATURES)


def check(code):
    if code != OK:
        msg = lib().bild_last_error().decode()
        raise (NoDeviceError if code == ERR_NO_DEVICE else BildAmdError)(code, msg)


def device_count():
    c = ctypes.c_int(0)
    check(lib().bild_device_count(ctypes.byref(c)))
    return c.value


def f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


_addressof, _from_buffer = ctypes.addressof, ctypes.c_char.from_buffer


def _traj_block(trajs):
    """ a list of (T, d) arrays -> (T (n,) int32, their frames in one (sum T, d) float64 block) """
    arrs = [f64(t) for t in trajs]
    return i32([a.shape[0] for a in arrs]), f64(np.concatenate(arrs, axis=0))


def aptr(a):
    """
    address of a C-contiguous array of any element type; the CALLER keeps the array alive across the call (no temporaries
    here).  Through the buffer protocol where that works (0.4 us; writable, non-empty arrays), else through
    ``__array_interface__`` (1.2 us; building a typed ctypes pointer costs 2.3).
    """
    try:
        return _addressof(_from_buffer(a))
    except (TypeError, ValueError, BufferError):
        return a.__array_interface__['data'][0]


dptr = aptr   # float64 buffers


def iptr(a):
    """ address of a C-contiguous int32 array, or None; lifetime as for `aptr` """
    return None if a is None else aptr(a)


class ModelHandle:
    """ owns a ``bild_model*`` """

    def __init__(self, B, G, Sig, M0, C0, w, reduce=True):
        B, G, Sig, M0, C0, w = (f64(a) for a in (B, G, Sig, M0, C0, w))
        S, N, d = G.shape
        if B.shape != (S, N, N) or Sig.shape != (S, N, N) or C0.shape != (S, N, N) \
                or M0.shape != (S, N, d) or w.shape != (N,):
            raise AssertionError("inconsistent model array shapes")  # reference: pyx:165-166 asserts
        self.N, self.d, self.S = N, d, S
        self._h = _vp()
        check(lib().bild_model_create(N, d, S, dptr(B), dptr(G), dptr(Sig), dptr(M0), dptr(C0), dptr(w),
                                      0 if reduce else MODEL_NO_REDUCE, ctypes.byref(self._h)))

    def query(self, what):
        v = ctypes.c_int64(0)
        check(lib().bild_model_query(self._h, what, ctypes.byref(v)))
        return v.value

    def export(self, what, s=0, s2=0):
        n = self.query(Q_NEFF)
        shape = {X_LAMBDA: (n,), X_SIGMA: (n,), X_Q: (n, n), X_WQ: (n,), X_R: (n, n), X_C0Q: (n, n),
                 X_V: (self.N, n)}[what]
        buf = np.empty(shape, dtype=np.float64)
        check(lib().bild_model_export(self._h, what, s, s2, dptr(buf), buf.size))
        return buf

    def __del__(self):
        if getattr(self, '_h', None) and _lib is not None:
            _lib.bild_model_destroy(self._h)
            self._h = None


class TrajSetHandle:
    """ owns a ``bild_trajset*`` (device-resident trajectories) """

    def __init__(self, model, trajs, loc_errs):
        self.model = model  # keep alive
        arrs = [f64(t) for t in trajs]
        for a in arrs:
            if a.ndim != 2 or a.shape[1] != model.d:
                raise AssertionError(f"trajectory shape {a.shape} does not match model dimension d={model.d}")
        self.T, x = _traj_block(arrs)
        err = f64(loc_errs).reshape(len(arrs), model.d)
        self.n_traj = len(arrs)
        self._h = _vp()
        check(lib().bild_trajset_create(model._h, self.n_traj, iptr(self.T), dptr(x), dptr(err), ctypes.byref(self._h)))

    def expect(self, evaluations):
        """ declare, before the first evaluation, how many evaluations the set will see (bild_trajset_expect) """
        check(lib().bild_trajset_expect(self._h, int(evaluations)))

    def __del__(self):
        if getattr(self, '_h', None) and _lib is not None:
            _lib.bild_trajset_destroy(self._h)
            self._h = None


class GaussModelHandle:
    """ owns a ``bild_gauss_model*`` (GenericGaussianModel: host memory only) """

    def __init__(self, order, mean, msd, msd_inf):
        order, mean, msd, msd_inf = i32(order), f64(mean), f64(msd), f64(msd_inf)
        S, d, L1 = msd.shape
        assert order.shape == (S, d) and mean.shape == (S, d) and msd_inf.shape == (S, d)
        self.S, self.d, self.Tmax = S, d, L1 - 1
        self.order = order
        self._h = _vp()
        check(lib().bild_gauss_model_create(S, d, L1 - 1, iptr(order), dptr(mean), dptr(msd), dptr(msd_inf), ctypes.byref(self._h)))

    def __del__(self):
        if getattr(self, '_h', None) and _lib is not None:
            _lib.bild_gauss_model_destroy(self._h)
            self._h = None


class GaussTrajSetHandle:
    """ owns a ``bild_gauss_trajset*``: the trajectories and their interval tables on the device """

    def __init__(self, model, trajs):
        self.model = model  # keep alive
        arrs = [f64(t) for t in trajs]
        for a in arrs:
            if a.ndim != 2 or a.shape[1] != model.d:
                raise AssertionError(f"trajectory shape {a.shape} does not match model dimension d={model.d}")
        self.T, x = _traj_block(arrs)
        self.n_traj = len(arrs)
        self._h = _vp()
        check(lib().bild_gauss_trajset_create(model._h, self.n_traj, iptr(self.T), dptr(x), ctypes.byref(self._h)))

    def info(self):
        """ (table bytes, build ms) """
        b, ms = ctypes.c_int64(0), ctypes.c_double(0)
        check(lib().bild_gauss_trajset_info(self._h, ctypes.byref(b), ctypes.byref(ms)))
        return b.value, ms.value

    def __del__(self):
        if getattr(self, '_h', None) and _lib is not None:
            _lib.bild_gauss_trajset_destroy(self._h)
            self._h = None


def gauss_logl_segments(model, ts, seg_start, seg_state, traj_id=None):
    seg_start, seg_state = i32(seg_start), i32(seg_state)
    n, K1 = seg_start.shape
    assert seg_state.shape == (n, K1)
    tid = None if traj_id is None else i32(traj_id)
    assert tid is None or tid.shape == (n,)
    out = np.empty(n, dtype=np.float64)
    check(lib().bild_gauss_logl_segments(model._h, ts._h, n, K1, iptr(seg_start), iptr(seg_state), iptr(tid), dptr(out)))
    return out


def gauss_logl_st(model, ts, ss, thetas, traj_id=None):
    ss = f64(ss)
    thetas = np.ascontiguousarray(thetas, dtype=np.int64)
    if ss.ndim == 1:
        ss, thetas = ss[None, :], thetas[None, :]
    n, K1 = thetas.shape
    assert ss.shape == (n, K1)
    tid = None if traj_id is None else i32(traj_id)
    assert tid is None or tid.shape == (n,)
    out = np.empty(n, dtype=np.float64)
    check(lib().bild_gauss_logl_st(model._h, ts._h, n, K1, dptr(ss), aptr(thetas), iptr(tid), dptr(out)))
    return out


def rouse_simulate(V, b, sqrt_sig, sqrt_cinf, VtG, VtM0, w, T, seg_start, seg_state, missing, loc_err, normals=None, seed=0,
                   scratch_bytes=0):
    """
    Rouse trajectories in modal coordinates (bild_rouse_simulate): per state V (S, N, N), b, sqrt_sig, sqrt_cinf (S, N),
    VtG, VtM0 (S, N, d); w (N,); per trajectory T (n,), segments (n, K1), missing (sum T,) bool or None, loc_err (n, d);
    normals: the host-drawn normals of every trajectory in order (replay), or None (device mode, keyed by ``seed``).
    ``scratch_bytes`` bounds the upload chunks of the normals (0: the library's rule).  -> (sum T, d) float64
    """
    V, b, sqrt_sig, sqrt_cinf, VtG, VtM0, w = (f64(a) for a in (V, b, sqrt_sig, sqrt_cinf, VtG, VtM0, w))
    S, N, d = VtG.shape
    assert V.shape == (S, N, N) and b.shape == sqrt_sig.shape == sqrt_cinf.shape == (S, N) and VtM0.shape == (S, N, d)
    assert w.shape == (N,)
    T, seg_start, seg_state = i32(T), i32(seg_start), i32(seg_state)
    n = T.shape[0]
    K1 = seg_start.shape[1] if seg_start.ndim == 2 else 1
    assert seg_start.shape == seg_state.shape == (n, K1)
    rows = int(T.sum())
    miss = None if missing is None else np.ascontiguousarray(missing, dtype=np.uint8)
    assert miss is None or miss.shape == (rows,)
    err = f64(loc_err)
    assert err.shape == (n, d)
    z = None if normals is None else f64(normals)
    assert z is None or z.shape == (rows * (N + 1) * d,)
    out = np.empty((rows, d), dtype=np.float64)
    check(lib().bild_rouse_simulate(S, N, d, dptr(V), dptr(b), dptr(sqrt_sig), dptr(sqrt_cinf), dptr(VtG), dptr(VtM0), dptr(w),
                                    n, iptr(T), K1, iptr(seg_start), iptr(seg_state), None if miss is None else aptr(miss),
                                    dptr(err), None if z is None else dptr(z), int(seed), int(scratch_bytes),
                                    dptr(out) if rows else None))
    return out


def gauss_simulate(model, T, seg_start, seg_state, missing, normals=None, seed=0, scratch_bytes=0):
    """
    GenericGaussianModel trajectories (bild_gauss_simulate) of the model handle ``model``: per trajectory T (n,), segments
    (n, K1), missing (sum T,) bool or None; normals: every trajectory's normals in the loop's order, one trajectory after
    the other (replay), or None (device mode, keyed by ``seed``).  ``scratch_bytes`` bounds the chunks of normals (0: the
    library's rule).  A covariance that is not positive definite raises numpy.linalg.LinAlgError.  -> (sum T, d) float64
    """
    T, seg_start, seg_state = i32(T), i32(seg_start), i32(seg_state)
    n = T.shape[0]
    K1 = seg_start.shape[1] if seg_start.ndim == 2 else 1
    assert seg_start.shape == seg_state.shape == (n, K1)
    rows = int(T.sum())
    miss = None if missing is None else np.ascontiguousarray(missing, dtype=np.uint8)
    assert miss is None or miss.shape == (rows,)
    z = None if normals is None else f64(normals)
    assert z is None or (seg_state.min(initial=0) >= 0 and seg_state.max(initial=0) < model.S and
                         z.shape == (rows * model.d - int(model.order[seg_state[:, 0]].sum()),))
    out = np.empty((rows, model.d), dtype=np.float64)
    code = lib().bild_gauss_simulate(model._h, n, iptr(T), K1, iptr(seg_start), iptr(seg_state), None if miss is None else aptr(miss),
                                     None if z is None else dptr(z), int(seed), int(scratch_bytes), dptr(out) if rows else None)
    if code == ERR_INVALID:
        msg = lib().bild_last_error().decode()
        if 'not positive definite' in msg:
            raise np.linalg.LinAlgError(msg)
    check(code)
    return out


def logl_segments(model, ts, seg_start, seg_state, traj_id=None, path='auto', prefix=True, jump=True, split=True, states=True, tail=True,
                  switch_tail=True):
    seg_start, seg_state = i32(seg_start), i32(seg_state)
    n, K1 = seg_start.shape
    assert seg_state.shape == (n, K1)
    tid = None if traj_id is None else i32(traj_id)
    out = np.empty(n, dtype=np.float64)
    check(lib().bild_logl_segments(model._h, ts._h, n, K1, iptr(seg_start), iptr(seg_state), iptr(tid),
                                   _flags(path, prefix=prefix, jump=jump, split=split, states=states, tail=tail, switch_tail=switch_tail),
                                   dptr(out)))
    return out


def logl_st(model, ts, ss, thetas, traj_id=None, path='auto', prefix=True, jump=True, split=True, tail=True, switch_tail=True):
    """ the sampler's (s, theta) batch as it is: switch frames are computed natively (bild_logl_st) """
    ss = f64(ss)
    thetas = np.ascontiguousarray(thetas, dtype=np.int64)
    if ss.ndim == 1:
        ss, thetas = ss[None, :], thetas[None, :]
    n, K1 = thetas.shape
    assert ss.shape == (n, K1)
    tid = None if traj_id is None else i32(traj_id)
    out = np.empty(n, dtype=np.float64)
    check(lib().bild_logl_st(model._h, ts._h, n, K1, dptr(ss), aptr(thetas), iptr(tid),
                             _flags(path, prefix=prefix, jump=jump, split=split, tail=tail, switch_tail=switch_tail), dptr(out)))
    return out


def logl_st_to_device(model, ts, ss, thetas, d_out, traj_id=None, stream=0, path='auto'):
    """ host (s, theta) batch in, results left in HBM at the raw device pointer `d_out`; asynchronous on `stream` """
    ss = f64(ss)
    thetas = np.ascontiguousarray(thetas, dtype=np.int64)
    n, K1 = thetas.shape
    assert ss.shape == (n, K1)
    tid = None if traj_id is None else i32(traj_id)
    check(lib().bild_logl_st_to_device(model._h, ts._h, n, K1, dptr(ss), aptr(thetas), iptr(tid), PATHS[path],
                                       _vp(stream) if stream else None, _vp(d_out)))


def segments_from_st(ss, thetas, T, n_states):
    """ native (s, theta) -> run-length segments (bild_segments_from_st); T: one length or one per sample """
    ss = f64(ss)
    thetas = np.ascontiguousarray(thetas, dtype=np.int64)
    n, K1 = thetas.shape
    assert ss.shape == (n, K1)
    Ts = i32(np.atleast_1d(T))
    assert len(Ts) in (1, n)
    seg_start = np.empty((n, K1), dtype=np.int32)
    seg_state = np.empty((n, K1), dtype=np.int32)
    check(lib().bild_segments_from_st(n, K1, int(n_states), iptr(Ts), 0 if len(Ts) == 1 else 1, dptr(ss),
                                      aptr(thetas), iptr(seg_start), iptr(seg_state)))
    return seg_start, seg_state


def logl_profiles(model, ts, states, traj_id=None, path='auto'):
    states = i32(np.atleast_2d(states))
    n, ld = states.shape
    tid = None if traj_id is None else i32(traj_id)
    out = np.empty(n, dtype=np.float64)
    check(lib().bild_logl_profiles(model._h, ts._h, n, ld, iptr(states), iptr(tid), PATHS[path], dptr(out)))
    return out


def _flags(path, validate=False, prefix=True, jump=True, split=True, states=True, tail=True, switch_tail=True):
    return (PATHS[path] | (VALIDATE_DEVICE if validate else 0) | (0 if prefix else NO_PREFIX) | (0 if jump else NO_JUMP) |
            (0 if split else NO_SPLIT) | (0 if states else NO_STATES) | (0 if tail else NO_TAIL) |
            (0 if switch_tail else NO_SWITCH_TAIL))


def frames_run_read(model):
    """ frames the tasks ran themselves since the last call (kernel timing must be on); resets the counter """
    v = ctypes.c_int64(0)
    check(lib().bild_frames_run_read(model._h, ctypes.byref(v)))
    return v.value


def schedule_segments(model, ts, seg_start, seg_state, traj_id=None, path='auto', prefix=True, jump=True):
    """
    launch order for device-resident candidates (bild_schedule_segments): (n,) int32, order[slot] = sample.  The work
    estimate behind it uses the trajectory set's tables: evaluate something on the set once before asking.
    """
    seg_start, seg_state = i32(seg_start), i32(seg_state)
    n, K1 = seg_start.shape
    tid = None if traj_id is None else i32(traj_id)
    order = np.empty(n, dtype=np.int32)
    check(lib().bild_schedule_segments(model._h, ts._h, n, K1, iptr(seg_start), iptr(seg_state), iptr(tid),
                                       _flags(path, prefix=prefix, jump=jump), iptr(order)))
    return order


def frames_executed_fraction(model, ts, seg_start, traj_id=None, order=None, path='auto', prefix=True):
    """ share of the (task, frame) pairs of a batch that the launch runs itself (the rest comes out of the prefix table) """
    seg_start = i32(seg_start)
    n, K1 = seg_start.shape
    tid = None if traj_id is None else i32(traj_id)
    od = None if order is None else i32(order)
    tot, run = ctypes.c_double(0), ctypes.c_double(0)
    check(lib().bild_frames_executed(model._h, ts._h, n, K1, iptr(seg_start), iptr(tid), iptr(od), _flags(path, prefix=prefix),
                                     ctypes.byref(tot), ctypes.byref(run)))
    return run.value / tot.value if tot.value else 1.0


KALMAN_OUTPUTS = ('terms', 'pred_mean', 'pred_var', 'filt_mean', 'filt_var', 'smooth_mean', 'smooth_var', 'innov')


class KalmanOut(ctypes.Structure):
    _fields_ = [(name, ctypes.c_void_p) for name in KALMAN_OUTPUTS] + [('T_max', ctypes.c_int32)]


def kalman_segments(model, ts, seg_start, seg_state, traj_id=None, outputs=KALMAN_OUTPUTS, T_max=None, scratch_bytes=0):
    """
    per-frame filter and smoother moments of run-length encoded profiles (bild_kalman_segments): a dict of the requested
    outputs (names of KALMAN_OUTPUTS), each (n, T_max, d) float64; T_max defaults to the set's longest trajectory
    """
    seg_start, seg_state = i32(seg_start), i32(seg_state)
    n, K1 = seg_start.shape
    assert seg_state.shape == (n, K1)
    tid = None if traj_id is None else i32(traj_id)
    if T_max is None:
        T_max = int(np.max(ts.T))
    res = {}
    spec = KalmanOut(T_max=int(T_max))
    for name in outputs:
        if name not in KALMAN_OUTPUTS:
            raise ValueError(f"unknown output {name!r}")
        res[name] = np.empty((n, T_max, model.d), dtype=np.float64)
        setattr(spec, name, aptr(res[name]) if res[name].size else None)
    check(lib().bild_kalman_segments(model._h, ts._h, n, K1, iptr(seg_start), iptr(seg_state), iptr(tid), ctypes.byref(spec),
                                     int(scratch_bytes)))
    return res


def kalman_mixture(model, ts, seg_start, seg_state, log_weights, traj_id=None, scratch_bytes=0):
    """ posterior mixture of the smoothed y per trajectory of the set (bild_kalman_mixture): (mean, var), each (n_traj, Tmax, d) """
    seg_start, seg_state = i32(seg_start), i32(seg_state)
    n, K1 = seg_start.shape
    assert seg_state.shape == (n, K1)
    lw = f64(log_weights).reshape(-1)
    assert lw.shape == (n,)
    tid = None if traj_id is None else i32(traj_id)
    Tmax = int(np.max(ts.T))
    mean = np.empty((ts.n_traj, Tmax, model.d), dtype=np.float64)
    var = np.empty_like(mean)
    check(lib().bild_kalman_mixture(model._h, ts._h, n, K1, iptr(seg_start), iptr(seg_state), iptr(tid), dptr(lw), dptr(mean),
                                    dptr(var), int(scratch_bytes)))
    return mean, var


class ModelDerivs(ctypes.Structure):
    _fields_ = [(name, ctypes.c_void_p) for name in ('dB', 'dG', 'dSig', 'dM0', 'dC0')]


DERIV_NAMES = ('dB', 'dG', 'dSig', 'dM0', 'dC0')


def logl_sensitivities(model, ts, seg_start, seg_state, traj_id=None, derivs=None, ds2=None, P=None, grad=True, fisher=True,
                       scratch_bytes=0):
    """
    log-likelihood, gradient and Fisher information of run-length encoded profiles (bild_logl_sensitivities).
    derivs: dict of raw derivative arrays (DERIV_NAMES; each (P, S, N, N) or (P, S, N, d), absent = zero); ds2:
    (P, n_traj, d) or None.  -> (logl (n,), grad (n, P) or None, fisher (n, P, P) or None)
    """
    seg_start, seg_state = i32(seg_start), i32(seg_state)
    n, K1 = seg_start.shape
    assert seg_state.shape == (n, K1)
    tid = None if traj_id is None else i32(traj_id)
    derivs = {} if derivs is None else derivs
    unknown = set(derivs) - set(DERIV_NAMES)
    if unknown:
        raise ValueError(f"unknown derivative arrays {sorted(unknown)}; choose from {DERIV_NAMES}")
    arrs = {k: f64(v) for k, v in derivs.items() if v is not None}
    if P is None:
        P = next((len(a) for a in arrs.values()), len(ds2) if ds2 is not None else 0)
    S, N, d = model.S, model.N, model.d
    for k, a in arrs.items():
        want = (P, S, N, N) if k in ('dB', 'dSig', 'dC0') else (P, S, N, d)
        if a.shape != want:
            raise ValueError(f"{k} has shape {a.shape}, expected {want}")
    spec = ModelDerivs(**{k: aptr(a) if a.size else None for k, a in arrs.items()})
    if ds2 is not None:
        ds2 = f64(ds2)
        if ds2.shape != (P, ts.n_traj, d):
            raise ValueError(f"ds2 has shape {ds2.shape}, expected {(P, ts.n_traj, d)}")
    logl = np.empty(n, dtype=np.float64)
    g = np.empty((n, P), dtype=np.float64) if grad else None
    F = np.empty((n, P, P), dtype=np.float64) if fisher else None
    check(lib().bild_logl_sensitivities(model._h, ts._h, n, K1, iptr(seg_start), iptr(seg_state), iptr(tid), int(P),
                                        ctypes.byref(spec), None if ds2 is None or not ds2.size else dptr(ds2), dptr(logl),
                                        None if g is None or not g.size else dptr(g),
                                        None if F is None or not F.size else dptr(F), int(scratch_bytes)))
    return logl, g, F


class GaussDerivs(ctypes.Structure):
    _fields_ = [(name, ctypes.c_void_p) for name in ('dmsd', 'dmsd_inf', 'dmean')]


def _gauss_derivs(model, P, dmsd, dmsd_inf, dmean):
    """ dmsd (P, S, d, Tmax + 1), dmsd_inf and dmean (P, S, d), None = zero -> (GaussDerivs, the arrays it points into) """
    S, d, L1 = model.S, model.d, model.Tmax + 1
    keep = {}
    for name, a, shape in (('dmsd', dmsd, (P, S, d, L1)), ('dmsd_inf', dmsd_inf, (P, S, d)), ('dmean', dmean, (P, S, d))):
        if a is not None:
            a = f64(a)
            assert a.shape == shape, f"{name} has shape {a.shape}, expected {shape}"
            keep[name] = a
    return GaussDerivs(**{k: aptr(a) if a.size else None for k, a in keep.items()}), keep


def gauss_logl_sensitivities(model, trajs, seg_start, seg_state, traj_id=None, dmsd=None, dmsd_inf=None, dmean=None, P=0,
                             fisher=True, scratch_bytes=0):
    """
    log-likelihood, gradient and Fisher information of GenericGaussianModel candidates (bild_gauss_logl_sensitivities) of
    the model handle ``model``: trajs a list of (T, d) arrays, segments (n, K1); dmsd (P, S, d, Tmax + 1), dmsd_inf and
    dmean (P, S, d), None = zero.  -> (logl (n,), grad (n, P), fisher (n, P, P) or None)
    """
    seg_start, seg_state = i32(seg_start), i32(seg_state)
    n, K1 = seg_start.shape
    assert seg_state.shape == (n, K1)
    tid = None if traj_id is None else i32(traj_id)
    assert tid is None or tid.shape == (n,)
    T, x = _traj_block(trajs)
    spec, keep = _gauss_derivs(model, P, dmsd, dmsd_inf, dmean)
    logl = np.empty(n, dtype=np.float64)
    g = np.empty((n, P), dtype=np.float64)
    F = np.empty((n, P, P), dtype=np.float64) if fisher else None
    check(lib().bild_gauss_logl_sensitivities(model._h, len(T), iptr(T), dptr(x), n, K1, iptr(seg_start), iptr(seg_state),
                                              iptr(tid), int(P), ctypes.byref(spec), dptr(logl),
                                              dptr(g) if g.size else None, dptr(F) if F is not None and F.size else None,
                                              int(scratch_bytes)))
    return logl, g, F


GAUSS_KALMAN_OUTPUTS = ('terms', 'pred_mean', 'pred_var', 'smooth_mean', 'smooth_var', 'innov')


def gauss_kalman_segments(model, trajs, seg_start, seg_state, traj_id=None, outputs=GAUSS_KALMAN_OUTPUTS, T_max=None,
                          scratch_bytes=0):
    """
    per-frame moments of GenericGaussianModel candidates (bild_gauss_kalman_segments) of the model handle ``model``: trajs a
    list of (T, d) arrays, segments (n, K1); a dict of the requested outputs (names of KALMAN_OUTPUTS), each (n, T_max, d)
    float64, T_max defaulting to the longest trajectory
    """
    seg_start, seg_state = i32(seg_start), i32(seg_state)
    n, K1 = seg_start.shape
    assert seg_state.shape == (n, K1)
    tid = None if traj_id is None else i32(traj_id)
    assert tid is None or tid.shape == (n,)
    T, x = _traj_block(trajs)
    if T_max is None:
        T_max = int(np.max(T))
    res = {}
    spec = KalmanOut(T_max=int(T_max))
    for name in outputs:
        if name not in KALMAN_OUTPUTS:
            raise ValueError(f"unknown output {name!r}")
        res[name] = np.empty((n, T_max, model.d), dtype=np.float64)
        setattr(spec, name, aptr(res[name]) if res[name].size else None)
    check(lib().bild_gauss_kalman_segments(model._h, len(T), iptr(T), dptr(x), n, K1, iptr(seg_start), iptr(seg_state),
                                           iptr(tid), ctypes.byref(spec), int(scratch_bytes)))
    return res


def gauss_kalman_mixture(model, trajs, seg_start, seg_state, log_weights, traj_id=None, scratch_bytes=0):
    """
    posterior mixture of the smoothed coordinate per trajectory (bild_gauss_kalman_mixture): (mean, var), each
    (n_traj, T_max, d), T_max the longest trajectory
    """
    seg_start, seg_state = i32(seg_start), i32(seg_state)
    n, K1 = seg_start.shape
    assert seg_state.shape == (n, K1)
    lw = f64(log_weights).reshape(-1)
    assert lw.shape == (n,)
    tid = None if traj_id is None else i32(traj_id)
    T, x = _traj_block(trajs)
    mean = np.empty((len(T), int(np.max(T)), model.d), dtype=np.float64)
    var = np.empty_like(mean)
    check(lib().bild_gauss_kalman_mixture(model._h, len(T), iptr(T), dptr(x), n, K1, iptr(seg_start), iptr(seg_state),
                                          iptr(tid), dptr(lw), dptr(mean), dptr(var), int(scratch_bytes)))
    return mean, var


def prefix_info(ts):
    """ (bytes, build_ms) of the trajectory set's prefix table; (0, 0.0) when none has been built """
    b, ms = ctypes.c_int64(0), ctypes.c_double(0)
    check(lib().bild_prefix_info(ts._h, ctypes.byref(b), ctypes.byref(ms)))
    return b.value, ms.value


def logl_segments_device(model, ts, n, K1, d_seg_start, d_seg_state, d_traj_id, d_out, stream=0, path='auto', validate=False,
                         d_order=0, prefix=True, jump=True, split=True, states=True, tail=True, switch_tail=True):
    """
    raw device pointers (ints); asynchronous on `stream` (validate=True: descriptors checked on the device first);
    d_order: device pointer of the launch order from `schedule_segments`, 0 = the order of the arrays
    """
    check(lib().bild_logl_segments_device_ordered(model._h, ts._h, n, K1, _vp(d_seg_start), _vp(d_seg_state),
                                          _vp(d_traj_id) if d_traj_id else None, _vp(d_order) if d_order else None,
                                          _flags(path, validate, prefix, jump, split, states, tail, switch_tail),
                                          _vp(stream) if stream else None, _vp(d_out)))


def logl_st_device(model, ts, n, K1, d_ss, d_thetas, d_out, d_traj_id=0, stream=0, path='auto', d_status=0, split=True, states=True, tail=True):
    """
    the sampler's (s, theta) rows resident in HBM (raw device pointers: float64 n x K1, uint8 n x K1), results to d_out;
    asynchronous on `stream` (bild_logl_st_device)
    """
    check(lib().bild_logl_st_device(model._h, ts._h, n, K1, _vp(d_ss), _vp(d_thetas), _vp(d_traj_id) if d_traj_id else None,
                                    _flags(path, split=split, states=states, tail=tail), _vp(stream) if stream else None, _vp(d_out),
                                    _vp(d_status) if d_status else None))


def flop_count(model, ts, n, traj_id=None, path='auto'):
    can, exe = ctypes.c_double(0), ctypes.c_double(0)
    tid = None if traj_id is None else i32(traj_id)
    check(lib().bild_flop_count(model._h, ts._h, n, iptr(tid), PATHS[path], ctypes.byref(can), ctypes.byref(exe)))
    return can.value, exe.value


def kernel_timing(enable):
    """ False / 0: off; True / 1: events around every launch; p > 1: around every p-th launch """
    check(lib().bild_kernel_timing(int(enable)))


def kernel_timing_read():
    ms, cnt = ctypes.c_double(0), ctypes.c_int64(0)
    name = ctypes.create_string_buffer(128)
    check(lib().bild_kernel_timing_read(ctypes.byref(ms), ctypes.byref(cnt), name, 128))
    return ms.value, cnt.value, name.value.decode()


def kernel_timing_read_walk():
    """ device time and number of launches of the table-walk kernel (walk.hip) since the last call """
    ms, cnt = ctypes.c_double(0), ctypes.c_int64(0)
    check(lib().bild_kernel_timing_read_walk(ctypes.byref(ms), ctypes.byref(cnt)))
    return ms.value, cnt.value


def logl_st_status(model):
    """ waits for the model's pending to_device calls; raises if one of their rows was refused (bild_logl_st_status) """
    row = ctypes.c_int64(-1)
    check(lib().bild_logl_st_status(model._h, ctypes.byref(row)))


COMM_ID_BYTES = 128


def _choose_rccl():
    """
    The RCCL that matches the HIP runtime in the process: when the library was bound to PyTorch's runtime (see
    `_share_hip_runtime_with_torch`), PyTorch's own librccl.so beside it; else whatever the loader finds.
    """
    global _rccl_chosen
    if _rccl_chosen:
        return
    _rccl_chosen = True
    libdir = _torch_libdir
    if libdir is None and 'torch' in __import__('sys').modules:
        libdir = os.path.join(os.path.dirname(__import__('sys').modules['torch'].__file__), 'lib')
    if libdir and os.path.exists(os.path.join(libdir, 'librccl.so')) and not os.environ.get('BILD_AMD_RCCL'):
        lib().bild_comm_library(os.path.join(libdir, 'librccl.so').encode())


def comm_unique_id():
    """ 128 opaque bytes identifying a new communicator (rank 0 calls this and hands them to every rank) """
    _choose_rccl()
    buf = ctypes.create_string_buffer(COMM_ID_BYTES)
    check(lib().bild_comm_unique_id(buf, COMM_ID_BYTES))
    return buf.raw


class CommHandle:
    """ owns a ``bild_comm*`` (an RCCL communicator on the current device) """

    def __init__(self, unique_id, world, rank):
        assert len(unique_id) == COMM_ID_BYTES
        _choose_rccl()
        self.world, self.rank = int(world), int(rank)
        self._h = _vp()
        check(lib().bild_comm_create(unique_id, self.world, self.rank, ctypes.byref(self._h)))

    def allgather(self, d_send, d_recv, n_per_rank, stream=0):
        """ raw device pointers; asynchronous on `stream` """
        check(lib().bild_comm_allgather(self._h, _vp(d_send), _vp(d_recv), int(n_per_rank), _vp(stream) if stream else None))

    def __del__(self):
        if getattr(self, '_h', None) and _lib is not None:
            _lib.bild_comm_destroy(self._h)
            self._h = None


EXCHANGE_HANDLE_BYTES = 64


class ExchangeHandle:
    """ owns a ``bild_exchange*``: the direct all-gather of a multi-GPU step (include/bild_amd.h, "the direct exchange") """

    def __init__(self, world, rank, slot_doubles):
        self.world, self.rank = int(world), int(rank)
        self._h = _vp()
        check(lib().bild_exchange_create(self.world, self.rank, int(slot_doubles), ctypes.byref(self._h)))

    def handle(self):
        buf = ctypes.create_string_buffer(EXCHANGE_HANDLE_BYTES)
        check(lib().bild_exchange_handle(self._h, buf))
        return buf.raw

    def connect(self, handles):
        """ handles: the 64-byte handles of all ranks, in rank order """
        blob = b''.join(handles)
        assert len(blob) == self.world * EXCHANGE_HANDLE_BYTES
        check(lib().bild_exchange_connect(self._h, blob))

    def allgather(self, d_send, d_recv, n_per_rank, stream=0):
        check(lib().bild_exchange_allgather(self._h, int(d_send), int(n_per_rank), int(stream) if stream else None, int(d_recv)))

    def status(self):
        """ after the stream has been waited for: raises when a peer did not deliver within the timeout """
        peer = ctypes.c_int(-1)
        check(lib().bild_exchange_status(self._h, ctypes.byref(peer)))

    def set_step(self, step):
        check(lib().bild_exchange_set_step(self._h, int(step) & 0xffffffff))

    def set_timeout(self, seconds):
        check(lib().bild_exchange_set_timeout(self._h, float(seconds)))

    def __del__(self):
        h, self._h = getattr(self, '_h', None), None
        if h:
            try:
                lib().bild_exchange_destroy(h)
            except Exception:  # pragma: no cover  (interpreter shutdown)
                pass


class DeviceBuffer:
    """ a plain device allocation of `n` float64 (for host programs without a GPU framework) """

    def __init__(self, n):
        self.n = int(n)
        self._p = _vp()
        check(lib().bild_device_alloc(8 * self.n, ctypes.byref(self._p)))

    @property
    def ptr(self):
        return self._p.value or 0

    def to_host(self, n=None, stream=0):
        out = np.empty(self.n if n is None else int(n), dtype=np.float64)
        check(lib().bild_device_to_host(aptr(out), self._p, 8 * out.size, _vp(stream) if stream else None))
        return out

    def __del__(self):
        if getattr(self, '_p', None) and _lib is not None:
            _lib.bild_device_free(self._p)
            self._p = None


class AmisCore:
    """
    Host-side bookkeeping of one fixed-k AMIS sampler in native code (include/bild_amd.h, "host-side AMIS
    bookkeeping"; csrc/amis_host.cpp).  No GPU involved.  `bild_amd.amis.FixedkSampler` drives it; the NumPy
    formulation of the same bookkeeping lives there as the specification.
    """
    POOL = {'logLs': 0, 'logδs': 1, 'cur_log_proposal': 2, 'log_weights': 3}

    def __init__(self, transitions, a0, logp0, concentration_brake, polarization_brake, logprior):
        trans = np.ascontiguousarray(np.asarray(transitions) != 0, dtype=np.uint8)
        self.n = trans.shape[0]
        self.k1 = len(a0)
        logp0, a0 = f64(logp0), f64(a0)
        assert logp0.shape == (self.n, self.k1)
        self._h = _vp()
        code = lib().bild_amis_create(self.k1, self.n, aptr(trans), float(concentration_brake),
                                      float(polarization_brake), float(logprior), dptr(a0), dptr(logp0),
                                      ctypes.byref(self._h))
        if code != OK:
            raise BildAmdError(code, "bild_amis_create failed")

    def __del__(self):
        h, self._h = getattr(self, '_h', None), None
        if h:
            try:
                lib().bild_amis_destroy(h)
            except Exception:  # pragma: no cover  (interpreter shutdown)
                pass

    def __len__(self):
        return int(lib().bild_amis_pool_size(self._h))

    def params(self, which=-1):
        a, logp = np.empty(self.k1), np.empty((self.n, self.k1))
        if lib().bild_amis_params(self._h, which, dptr(a), dptr(logp)) != OK:
            raise IndexError(which)
        return a, logp

    def pool(self, key):
        out = np.empty(len(self))
        if lib().bild_amis_pool(self._h, self.POOL[key], dptr(out)) != OK:
            raise KeyError(key)
        return out

    def restore(self, parameters, ss, thetas, arrays):
        """ load saved state into a freshly created core: further proposals [(a, logp), ...] and the pooled samples """
        Q = len(parameters)
        a = f64(np.array([p[0] for p in parameters]).reshape(Q, self.k1))
        logp = f64(np.array([p[1] for p in parameters]).reshape(Q, self.n, self.k1))
        ss = f64(np.asarray(ss).reshape(-1, self.k1))
        thetas = np.ascontiguousarray(np.asarray(thetas).reshape(-1, self.k1), dtype=np.int64)
        cols = [f64(arrays[key]) for key in ('logLs', 'logδs', 'cur_log_proposal', 'log_weights')] if len(ss) else [f64([])] * 4
        code = lib().bild_amis_restore(self._h, Q, dptr(a), dptr(logp), len(ss), dptr(ss), aptr(thetas),
                                       *(dptr(c) for c in cols))
        if code != OK:
            raise BildAmdError(code, "bild_amis_restore failed")

    def sample_traces(self, u):
        """ u: (k1, N) uniform random numbers -> (N, k1) int traces from the current proposal """
        u = f64(u)
        assert u.ndim == 2 and u.shape[0] == self.k1
        thetas = np.empty((u.shape[1], self.k1), dtype=np.int64)
        code = lib().bild_amis_sample_traces(self._h, u.shape[1], dptr(u), aptr(thetas))
        if code != OK:
            raise BildAmdError(code, "bild_amis_sample_traces failed")
        return thetas

    def use_device(self, enable=True):
        """ pooled samples in HBM, the passes of `step` on the GPU (bild_amis_use_device); for large batches per step """
        code = lib().bild_amis_use_device(self._h, 1 if enable else 0)
        if code == ERR_NO_DEVICE:
            raise NoDeviceError(code, lib().bild_amis_error(self._h).decode())
        if code != OK:
            raise BildAmdError(code, lib().bild_amis_error(self._h).decode())
        self.on_device = bool(enable)

    def step(self, ss, thetas, logLs):
        """ -> (logev, dlogev, KL); RuntimeError("Iteration did not converge") as the reference raises it """
        ss, logLs = f64(ss), f64(logLs)
        thetas = np.ascontiguousarray(thetas, dtype=np.int64)
        assert ss.shape == thetas.shape == (len(logLs), self.k1)
        ev = np.empty(3)
        code = lib().bild_amis_step(self._h, len(logLs), dptr(ss), aptr(thetas), dptr(logLs), dptr(ev))
        if code != OK:
            msg = lib().bild_amis_error(self._h).decode()
            raise RuntimeError(msg) if 'converge' in msg else BildAmdError(code, msg)
        return tuple(ev)


def _amis_step_fused(self, model, ts, ss, thetas, path='auto'):
    """
    the likelihood of the new batch and the bookkeeping of the step in one native call (bild_amis_step_fused): the samples
    go up once, nothing but partial sums comes down -> (logev, dlogev, KL)
    """
    ss = f64(ss)
    thetas = np.ascontiguousarray(thetas, dtype=np.int64)
    assert ss.shape == thetas.shape and ss.shape[1] == self.k1
    ev = np.empty(3)
    code = lib().bild_amis_step_fused(self._h, model._h, ts._h, len(ss), dptr(ss), aptr(thetas), PATHS[path], dptr(ev))
    if code != OK:
        msg = lib().bild_amis_error(self._h).decode()
        raise RuntimeError(msg) if 'converge' in msg else BildAmdError(code, msg)
    return tuple(ev)


AmisCore.step_fused = _amis_step_fused


def _amis_step_device_rng(self, model, ts, N, seed, path='auto'):
    """ a fused step whose samples are drawn on the device (bild_amis_step_device_rng) -> (logev, dlogev, KL) """
    ev = np.empty(3)
    code = lib().bild_amis_step_device_rng(self._h, model._h, ts._h, int(N), ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), PATHS[path], dptr(ev))
    if code != OK:
        msg = lib().bild_amis_error(self._h).decode()
        raise RuntimeError(msg) if 'converge' in msg else BildAmdError(code, msg)
    return tuple(ev)


def _amis_pool_samples(self):
    """ (ss, thetas) of all pooled samples, fetched from the device where fused steps left them """
    P = len(self)
    ss, thetas = np.empty((P, self.k1)), np.empty((P, self.k1), dtype=np.int64)
    if lib().bild_amis_pool_samples(self._h, dptr(ss), aptr(thetas)) != OK:
        raise BildAmdError(ERR_HIP, lib().bild_amis_error(self._h).decode())
    return ss, thetas


AmisCore.step_device_rng = _amis_step_device_rng
AmisCore.pool_samples = _amis_pool_samples


def _adopt_amis_core(handle, n, k1):
    """ an `AmisCore` around native bookkeeping that already exists (bild_run_take_core); the wrapper owns it from now on """
    core = AmisCore.__new__(AmisCore)
    core._h = handle
    core.n = n
    core.k1 = k1
    return core


class RunSettings(ctypes.Structure):
    """ bild_run_settings (include/bild_amd.h) """
    _fields_ = [('init_runs', ctypes.c_int32), ('k_lookahead', ctypes.c_int32), ('k_max', ctypes.c_int32), ('reserved', ctypes.c_int32),
                ('certainty_in_k', ctypes.c_double), ('dE', ctypes.c_double), ('N', ctypes.c_int64),
                ('concentration_brake', ctypes.c_double), ('polarization_brake', ctypes.c_double), ('max_fev', ctypes.c_int64),
                ('max_fcomplete', ctypes.c_int64), ('choice_samplesize', ctypes.c_int64)]


class RunHandle:
    """
    The inference driver (include/bild_amd.h, "the inference driver"; csrc/run_host.cpp): the adaptive-k loops of many
    trajectories, one round at a time.  `bild_amd.core.sample_many` drives it.
    """

    def __init__(self, T, transitions, settings, per_k):
        """
        T : trajectory lengths; transitions : (n, n) bool; settings : dict of the fields of `RunSettings`;
        per_k : for k = 0, 1, ...: (logp0 (n, k+1), logprior, n_total, traces (m, k+1) int or None)
        """
        trans = np.ascontiguousarray(np.asarray(transitions) != 0, dtype=np.uint8)
        self.n = trans.shape[0]
        self.n_traj = len(T)
        Ts = i32(np.asarray(T))
        st = RunSettings(**settings)
        logp0 = f64(np.concatenate([np.asarray(p[0], dtype=np.float64).reshape(-1) for p in per_k]))
        logprior = f64([p[1] for p in per_k])
        n_total = f64([p[2] for p in per_k])
        n_traces = np.array([0 if p[3] is None else len(p[3]) for p in per_k], dtype=np.int64)
        given = [np.asarray(p[3], dtype=np.int32).reshape(-1) for p in per_k if p[3] is not None and len(p[3])]
        traces = np.ascontiguousarray(np.concatenate(given) if given else np.zeros(1, dtype=np.int32), dtype=np.int32)
        self._h = _vp()
        check(lib().bild_run_create(self.n_traj, iptr(Ts), self.n, aptr(trans), ctypes.addressof(st), len(per_k), dptr(logp0),
                                    dptr(logprior), dptr(n_total), aptr(n_traces), iptr(traces), ctypes.byref(self._h)))
        self._counts = np.zeros(8, dtype=np.int64)

    def __del__(self):
        h, self._h = getattr(self, '_h', None), None
        if h:
            try:
                lib().bild_run_destroy(h)
            except Exception:  # pragma: no cover  (interpreter shutdown)
                pass

    def _check(self, code):
        if code != OK:
            msg = lib().bild_run_error(self._h).decode() or lib().bild_last_error().decode()
            raise (NoDeviceError if code == ERR_NO_DEVICE else BildAmdError)(code, msg)

    def plan(self):
        """
        plan the next round -> (counts, shapes): counts = (gammas, uniforms, normals, rows, trajectories running, AMIS steps,
        trajectories failed so far),
        shapes = the gamma shape parameters (a view of the driver's buffer, valid until the next call)
        """
        ptr = _vp()
        self._check(lib().bild_run_plan(self._h, aptr(self._counts), ctypes.byref(ptr)))
        n = int(self._counts[0])
        shapes = np.frombuffer((ctypes.c_double * n).from_address(ptr.value), dtype=np.float64) if n else np.empty(0)
        return self._counts, shapes

    def round(self, model, ts, gammas, uniforms, normals, path='auto'):
        """ the planned round on the GPU: rows, ONE likelihood call over all of them, bookkeeping (bild_run_round) """
        self._check(lib().bild_run_round(self._h, model._h, ts._h, PATHS[path], dptr(gammas), dptr(uniforms), dptr(normals)))

    def stage(self, gammas, uniforms):
        """ -> (ss (n, K1), thetas (n, K1) int64, traj_id (n,)): the round's candidate rows, for a caller that evaluates them itself """
        self._check(lib().bild_run_stage(self._h, dptr(gammas), dptr(uniforms)))
        n, K1 = ctypes.c_int64(0), ctypes.c_int(0)
        p_ss, p_th, p_id = _vp(), _vp(), _vp()
        self._check(lib().bild_run_rows(self._h, ctypes.byref(n), ctypes.byref(K1), ctypes.byref(p_ss), ctypes.byref(p_th), ctypes.byref(p_id)))
        n, K1 = n.value, K1.value
        if n == 0:
            return np.empty((0, K1)), np.empty((0, K1), dtype=np.int64), np.empty(0, dtype=np.int32)
        ss = np.frombuffer((ctypes.c_double * (n * K1)).from_address(p_ss.value), dtype=np.float64).reshape(n, K1)
        thetas = np.frombuffer((ctypes.c_int64 * (n * K1)).from_address(p_th.value), dtype=np.int64).reshape(n, K1)
        traj_id = np.frombuffer((ctypes.c_int32 * n).from_address(p_id.value), dtype=np.int32)
        return ss, thetas, traj_id

    def finish(self, logLs, normals):
        logLs = f64(logLs)
        self._check(lib().bild_run_finish(self._h, dptr(logLs), dptr(normals)))

    # -- results ---------------------------------------------------------------------------------------------
    def traj_info(self, j):
        """ -> (state, kind of failure, samplers, log rows, width, message) """
        info = np.zeros(5, dtype=np.int64)
        msg = ctypes.c_char_p()
        self._check(lib().bild_run_traj_info(self._h, j, aptr(info), ctypes.byref(msg)))
        return int(info[0]), int(info[1]), int(info[2]), int(info[3]), int(info[4]), (msg.value or b'').decode()

    def traj_log(self, j, rows, width):
        k, flags = np.zeros(rows, dtype=np.int32), np.zeros(rows, dtype=np.int32)
        i_la, pk, kld = np.zeros(rows), np.zeros((rows, width)), np.zeros((rows, width))
        self._check(lib().bild_run_traj_log(self._h, j, iptr(k), iptr(flags), dptr(i_la), dptr(pk), dptr(kld)))
        return k, flags, i_la, pk, kld

    def sampler_info(self, j, k):
        """ -> (kind, exhausted, steps, evidences, enumerated rows) """
        info = np.zeros(5, dtype=np.int64)
        self._check(lib().bild_run_sampler_info(self._h, j, k, aptr(info)))
        return int(info[0]), bool(info[1]), int(info[2]), int(info[3]), int(info[4])

    def sampler_data(self, j, k, n_ev, rows):
        ev = np.zeros((n_ev, 3))
        ss, th, logL = np.zeros((rows, k + 1)), np.zeros((rows, k + 1), dtype=np.int64), np.zeros(rows)
        self._check(lib().bild_run_sampler_data(self._h, j, k, dptr(ev), dptr(ss), aptr(th), dptr(logL)))
        return ev, ss, th, logL

    def take_core(self, j, k):
        h = _vp()
        self._check(lib().bild_run_take_core(self._h, j, k, ctypes.byref(h)))
        return _adopt_amis_core(h, self.n, k + 1) if h.value else None

    def totals(self):
        """ -> (rounds, likelihood evaluations, host threads) """
        t = np.zeros(3, dtype=np.int64)
        self._check(lib().bild_run_totals(self._h, aptr(t)))
        return int(t[0]), int(t[1]), int(t[2])


def choice_counts(rvs, mu, dmu, dE, omit=None, want_dn=True):
    """
    histograms of the "best k" over the rows of the common random sample (bild_choice_counts):
    (n0, Dn or None, n_omit or None)
    """
    rvs, mu, dmu = f64(rvs), f64(mu), f64(dmu)
    samplesize, kmax = rvs.shape
    n0 = np.zeros(kmax, dtype=np.int64)
    dn = np.zeros((kmax, kmax), dtype=np.int64) if want_dn else None
    flags = n_omit = None
    if omit is not None:
        flags = np.zeros(kmax, dtype=np.uint8)
        flags[omit] = 1
        n_omit = np.zeros(kmax, dtype=np.int64)
    vp = lambda a: None if a is None else aptr(a)
    code = lib().bild_choice_counts(samplesize, kmax, dptr(rvs), dptr(mu), dptr(dmu), float(dE), vp(flags), vp(n0), vp(dn), vp(n_omit))
    if code != OK:
        raise BildAmdError(code, "bild_choice_counts failed")
    return n0, dn, n_omit


def interval_marginals(seg_start, seg_state, w, n, T):
    """ (n, T) weighted state occupancy per frame of the profiles (seg_start, seg_state) with weights w """
    seg_start, seg_state, w = i32(seg_start), i32(seg_state), f64(w)
    P, k1 = seg_state.shape
    post = np.empty((n, T), dtype=np.float64)
    code = lib().bild_interval_marginals(P, k1, n, T, iptr(seg_start), iptr(seg_state), dptr(w), dptr(post))
    if code != OK:
        raise BildAmdError(code, "bild_interval_marginals failed")
    return post


# ---------------------------------------------------------------- the exact-inference calls
# Each call fills the arrays of a ``bild_*_out`` structure of pointers.  A wrapper allocates them as a dict whose keys are the
# structure's fields, in the header's order; `_out` turns the dict into the structure.  The dwell-time calls that share one
# argument order go through `_dwell_call`.  (tests/test_abi_header.py holds the structures, `_SIGNATURES` and the positions of
# the wrappers' arguments to include/bild_amd.h without a device.)

def _out(cls, res, null_empty=False, rename={}):
    """
    the ``bild_*_out`` structure ``cls`` of a call from its dict of output arrays, key = field (``rename``: keys that differ).
    None becomes NULL: not written.  ``null_empty`` is the rule of the sensitivity calls, which pass an empty array (grad and
    fisher at P = 0) as NULL too.  Elsewhere an empty array keeps its address: NULL means "not asked for" there (a NULL
    log_post is the forward pass alone), also at T_max = 0.
    """
    return cls(**{rename.get(name, name): (None if a is None or (null_empty and not a.size) else aptr(a)) for name, a in res.items()})


class ExactOut(ctypes.Structure):
    _fields_ = [(name, ctypes.c_void_p) for name in ('logev', 'kl', 'map_logl', 'map_seg_start', 'map_seg_state', 'n_nan',
                                                      'log_post')]


def _transitions_u8(transitions, S):
    tr = np.ascontiguousarray(np.asarray(transitions, dtype=bool), dtype=np.uint8)
    if tr.shape != (S, S):
        raise ValueError(f"transitions of shape {tr.shape}; the model has {S} states: ({S}, {S}) expected")
    return tr


def exact_count(T, k, transitions):
    """ number of profiles of k switches on a trajectory of T frames (bild_exact_count; host only) """
    tr = _transitions_u8(transitions, np.asarray(transitions).shape[0])
    n = ctypes.c_double(0)
    check(lib().bild_exact_count(int(T), int(k), tr.shape[0], aptr(tr), ctypes.byref(n)))
    return n.value


def exact_evidence(model, ts, k, transitions, marginals=True, max_profiles=2 ** 32, scratch_bytes=0, gauss=False, path='auto'):
    """
    exact evidence of every trajectory of the set (bild_exact_evidence / bild_gauss_exact_evidence): a dict of
    logev, kl, map_logl (n_traj,), map_seg_start, map_seg_state (n_traj, k + 1) int32, n_nan (n_traj,) int64 and
    log_post (n_traj, S, T_max) or None; T_max is the set's longest trajectory
    """
    tr = _transitions_u8(transitions, model.S)
    n, K1 = ts.n_traj, int(k) + 1
    T_max = int(np.max(ts.T))
    res = {'logev': np.empty(n), 'kl': np.empty(n), 'map_logl': np.empty(n),
           'map_seg_start': np.empty((n, K1), dtype=np.int32), 'map_seg_state': np.empty((n, K1), dtype=np.int32),
           'n_nan': np.empty(n, dtype=np.int64),
           'log_post': np.empty((n, model.S, T_max)) if marginals else None}
    spec = _out(ExactOut, res)
    if gauss:
        check(lib().bild_gauss_exact_evidence(model._h, ts._h, int(k), aptr(tr), float(max_profiles), int(scratch_bytes), T_max,
                                              ctypes.byref(spec)))
    else:
        check(lib().bild_exact_evidence(model._h, ts._h, int(k), aptr(tr), float(max_profiles), int(scratch_bytes), T_max,
                                        _flags(path), ctypes.byref(spec)))
    return res


class SegdpOut(ctypes.Structure):
    _fields_ = [(name, ctypes.c_void_p) for name in ('logev', 'kl', 'map_logl', 'n_profiles', 'n_omitted', 'map_seg_start',
                                                      'map_seg_state', 'log_post')]


SEGDP_NAN_PROPAGATE, SEGDP_NAN_OMIT = 0, 1


def gauss_segment_evidence(model, ts, k_max, transitions, marginals=True, omit=False, scratch_bytes=0):
    """
    exact evidence of every k <= k_max of every trajectory of the set (bild_gauss_segment_evidence): a dict of logev, kl,
    map_logl, n_profiles, n_omitted (n_traj, K), map_seg_start, map_seg_state (n_traj, K, K) int32 and log_post
    (n_traj, K, S, T_max) or None; K = k_max + 1, T_max the set's longest trajectory
    """
    tr = _transitions_u8(transitions, model.S)
    n, K = ts.n_traj, int(k_max) + 1
    T_max = int(np.max(ts.T))
    res = {'logev': np.empty((n, K)), 'kl': np.empty((n, K)), 'map_logl': np.empty((n, K)),
           'n_profiles': np.empty((n, K)), 'n_omitted': np.empty((n, K)),
           'map_seg_start': np.empty((n, K, K), dtype=np.int32), 'map_seg_state': np.empty((n, K, K), dtype=np.int32),
           'log_post': np.empty((n, K, model.S, T_max)) if marginals else None}
    spec = _out(SegdpOut, res)
    check(lib().bild_gauss_segment_evidence(model._h, ts._h, int(k_max), aptr(tr), T_max, SEGDP_NAN_OMIT if omit else SEGDP_NAN_PROPAGATE,
                                            int(scratch_bytes), ctypes.byref(spec)))
    return res


class SegdrawOut(ctypes.Structure):
    _fields_ = [(name, ctypes.c_void_p) for name in ('seg_start', 'seg_state', 'logl', 'uniforms_out')]


def gauss_segment_draw(model, ts, k_max, transitions, draw_traj, draw_k, uniforms=None, seed=0, scratch_bytes=0):
    """
    exact posterior draws of profiles (bild_gauss_segment_draw): draw r on trajectory draw_traj[r] of the set with draw_k[r]
    switches, from its row of ``uniforms`` (n, max(1, 2 k_max)) or, without them, from Philox stream r of ``seed``.  A dict of
    seg_start, seg_state (n, K) int32, logl (n,) and uniforms (n, max(1, 2 k_max)): those consumed; K = k_max + 1
    """
    tr = _transitions_u8(transitions, model.S)
    draw_traj, draw_k = i32(draw_traj), i32(draw_k)
    n, K, U = len(draw_traj), int(k_max) + 1, max(1, 2 * int(k_max))
    assert draw_traj.shape == (n,) and draw_k.shape == (n,)
    if uniforms is not None:
        uniforms = f64(uniforms)
        assert uniforms.shape == (n, U)
    res = {'seg_start': np.empty((n, K), dtype=np.int32), 'seg_state': np.empty((n, K), dtype=np.int32), 'logl': np.empty(n),
           'uniforms': np.zeros((n, U))}
    spec = _out(SegdrawOut, res, rename={'uniforms': 'uniforms_out'})
    check(lib().bild_gauss_segment_draw(model._h, ts._h, int(k_max), aptr(tr), int(np.max(ts.T)), int(scratch_bytes), n, iptr(draw_traj),
                                        iptr(draw_k), None if uniforms is None else aptr(uniforms), int(seed) & (2 ** 64 - 1),
                                        ctypes.byref(spec)))
    return res


class SegsensOut(ctypes.Structure):
    _fields_ = [(name, ctypes.c_void_p) for name in ('logev', 'log_marginal', 'k_post', 'grad', 'exp_logl', 'fisher')]


def gauss_segment_sensitivities(model, ts, trajs, k_max, transitions, log_k_prior=None, dmsd=None, dmsd_inf=None, dmean=None, P=0,
                                omit=False, fisher=True, scratch_bytes=0):
    """
    gradient of the exact evidence of every trajectory of the set (bild_gauss_segment_sensitivities): trajs the (T, d) arrays
    the set was built from, log_k_prior None or (n_traj, K), derivatives as for `gauss_logl_sensitivities`.  A dict of logev,
    k_post (n_traj, K), log_marginal, exp_logl (n_traj,), grad (n_traj, P) and fisher (n_traj, P, P) or None; K = k_max + 1
    """
    tr = _transitions_u8(transitions, model.S)
    n, K = ts.n_traj, int(k_max) + 1
    T, x = _traj_block(trajs)
    assert np.array_equal(T, ts.T)
    prior = None
    if log_k_prior is not None:
        prior = f64(log_k_prior)
        assert prior.shape == (n, K)
    derivs, keep = _gauss_derivs(model, P, dmsd, dmsd_inf, dmean)
    res = {'logev': np.empty((n, K)), 'log_marginal': np.empty(n), 'k_post': np.empty((n, K)), 'grad': np.empty((n, P)),
           'exp_logl': np.empty(n), 'fisher': np.empty((n, P, P)) if fisher else None}
    spec = _out(SegsensOut, res, null_empty=True)
    check(lib().bild_gauss_segment_sensitivities(model._h, ts._h, dptr(x), int(k_max), aptr(tr), SEGDP_NAN_OMIT if omit else SEGDP_NAN_PROPAGATE,
                                                 None if prior is None else dptr(prior), int(P), ctypes.byref(derivs),
                                                 int(scratch_bytes), ctypes.byref(spec)))
    return res


class DwellOut(ctypes.Structure):
    _fields_ = [(name, ctypes.c_void_p) for name in ('logev', 'map_logjoint', 'map_states', 'n_nan_windows', 'log_post', 'exp_jumps',
                                                      'exp_stay')]


DWELL_NAN_PROPAGATE, DWELL_NAN_OMIT = 0, 1


def _dwell_tables(model, log_init, log_jump, log_dwell, log_surv):
    """ the four tables of a dwell-time prior as float64, shapes checked -> ((log_init, log_jump, log_dwell, log_surv), L) """
    S = model.S
    log_init, log_jump, log_dwell, log_surv = f64(log_init), f64(log_jump), f64(log_dwell), f64(log_surv)
    L = log_dwell.shape[1]
    assert log_init.shape == (S,) and log_jump.shape == (S, S) and log_dwell.shape == (S, L) and log_surv.shape == (S, L)
    return (log_init, log_jump, log_dwell, log_surv), L


def _dwell_call(name, out_cls, model, ts, tables, outputs, scalars=(), omit=False, scratch_bytes=0):
    """
    the path of the dwell-time calls with the argument order (m, ts, L, the four tables, T_max, the call's own integer scalars,
    flags, scratch_bytes, out): ``name`` the library's function, ``tables`` as `_dwell_tables` takes them, ``outputs(n, S,
    T_max)`` the dict of the output arrays (keys: the fields of ``out_cls``; None: not computed), which is returned
    """
    tables, L = _dwell_tables(model, *tables)
    T_max = int(np.max(ts.T))
    res = outputs(ts.n_traj, model.S, T_max)
    spec = _out(out_cls, res)
    check(getattr(lib(), name)(model._h, ts._h, L, *[dptr(a) for a in tables], T_max, *[int(v) for v in scalars],
                               DWELL_NAN_OMIT if omit else DWELL_NAN_PROPAGATE, int(scratch_bytes), ctypes.byref(spec)))
    return res


def gauss_dwell_evidence(model, ts, log_init, log_jump, log_dwell, log_surv, marginals=True, omit=False, scratch_bytes=0):
    """
    exact inference under a dwell-time prior for every trajectory of the set (bild_gauss_dwell_evidence): a dict of logev,
    map_logjoint (n_traj,), map_states (n_traj, T_max) uint8, n_nan_windows (n_traj,) int64 and, with marginals, log_post
    (n_traj, S, T_max), exp_jumps (n_traj, S, S) and exp_stay (n_traj, S) (None without); T_max the set's longest trajectory
    """
    outputs = lambda n, S, T_max: {
        'logev': np.empty(n), 'map_logjoint': np.empty(n), 'map_states': np.empty((n, T_max), dtype=np.uint8),
        'n_nan_windows': np.empty(n, dtype=np.int64),
        'log_post': np.empty((n, S, T_max)) if marginals else None,
        'exp_jumps': np.empty((n, S, S)) if marginals else None, 'exp_stay': np.empty((n, S)) if marginals else None}
    return _dwell_call('bild_gauss_dwell_evidence', DwellOut, model, ts, (log_init, log_jump, log_dwell, log_surv), outputs,
                       omit=omit, scratch_bytes=scratch_bytes)


class DwellsensOut(ctypes.Structure):
    _fields_ = [(name, ctypes.c_void_p) for name in ('logev', 'n_nan_windows', 'grad', 'exp_logl', 'fisher')]


def gauss_dwell_sensitivities(model, ts, trajs, log_init, log_jump, log_dwell, log_surv, dmsd=None, dmsd_inf=None, dmean=None, P=0,
                              omit=False, fisher=True, scratch_bytes=0):
    """
    gradient of the exact evidence under a dwell-time prior of every trajectory of the set (bild_gauss_dwell_sensitivities):
    trajs the (T, d) arrays the set was built from, the prior's tables as for `gauss_dwell_evidence`, derivatives as for
    `gauss_logl_sensitivities`.  A dict of logev, exp_logl (n_traj,), n_nan_windows (n_traj,) int64, grad (n_traj, P) and
    fisher (n_traj, P, P) or None
    """
    (log_init, log_jump, log_dwell, log_surv), L = _dwell_tables(model, log_init, log_jump, log_dwell, log_surv)
    n = ts.n_traj
    T, x = _traj_block(trajs)
    assert np.array_equal(T, ts.T)
    derivs, keep = _gauss_derivs(model, P, dmsd, dmsd_inf, dmean)
    res = {'logev': np.empty(n), 'n_nan_windows': np.empty(n, dtype=np.int64), 'grad': np.empty((n, P)), 'exp_logl': np.empty(n),
           'fisher': np.empty((n, P, P)) if fisher else None}
    spec = _out(DwellsensOut, res, null_empty=True)
    check(lib().bild_gauss_dwell_sensitivities(model._h, ts._h, dptr(x), L, dptr(log_init), dptr(log_jump), dptr(log_dwell),
                                               dptr(log_surv), DWELL_NAN_OMIT if omit else DWELL_NAN_PROPAGATE, int(P),
                                               ctypes.byref(derivs), int(scratch_bytes), ctypes.byref(spec)))
    return res


class DwellLengthsOut(ctypes.Structure):
    _fields_ = [(name, ctypes.c_void_p) for name in ('logev', 'n_nan_windows', 'exp_jumps', 'exp_init', 'exp_dwell', 'exp_cens')]


def gauss_dwell_lengths(model, ts, log_init, log_jump, log_dwell, log_surv, omit=False, scratch_bytes=0):
    """
    expected segment-length counts under a dwell-time prior for every trajectory of the set (bild_gauss_dwell_lengths): a dict
    of logev (n_traj,), n_nan_windows (n_traj,) int64, exp_jumps (n_traj, S, S), exp_init (n_traj, S), exp_dwell and exp_cens
    (n_traj, S, T_max), length l at column l - 1, 0 behind a trajectory's T; T_max the set's longest trajectory
    """
    outputs = lambda n, S, T_max: {
        'logev': np.empty(n), 'n_nan_windows': np.empty(n, dtype=np.int64), 'exp_jumps': np.empty((n, S, S)),
        'exp_init': np.empty((n, S)), 'exp_dwell': np.empty((n, S, T_max)), 'exp_cens': np.empty((n, S, T_max))}
    return _dwell_call('bild_gauss_dwell_lengths', DwellLengthsOut, model, ts, (log_init, log_jump, log_dwell, log_surv), outputs,
                       omit=omit, scratch_bytes=scratch_bytes)


class DwellSwitchCountsOut(ctypes.Structure):
    _fields_ = [(name, ctypes.c_void_p) for name in ('logev', 'n_nan_windows', 'log_count', 'log_tail')]


def gauss_dwell_switch_counts(model, ts, log_init, log_jump, log_dwell, log_surv, k_max, omit=False, scratch_bytes=0):
    """
    exact posterior switch counts under a dwell-time prior for every trajectory of the set (bild_gauss_dwell_switch_counts): a
    dict of logev, log_tail (n_traj,), n_nan_windows (n_traj,) int64 and log_count (n_traj, k_max + 1, S)
    """
    outputs = lambda n, S, T_max: {
        'logev': np.empty(n), 'n_nan_windows': np.empty(n, dtype=np.int64), 'log_count': np.empty((n, max(int(k_max), -1) + 1, S)),
        'log_tail': np.empty(n)}        # (a negative k_max: no column, and the call refuses it)
    return _dwell_call('bild_gauss_dwell_switch_counts', DwellSwitchCountsOut, model, ts, (log_init, log_jump, log_dwell, log_surv),
                       outputs, scalars=(k_max,), omit=omit, scratch_bytes=scratch_bytes)


class DwellFirstContactOut(ctypes.Structure):
    _fields_ = [(name, ctypes.c_void_p) for name in ('logev', 'n_nan_windows', 'log_first', 'log_never')]


def gauss_dwell_first_contact(model, ts, log_init, log_jump, log_dwell, log_surv, target, omit=False, scratch_bytes=0):
    """
    exact posterior first-contact times under a dwell-time prior for every trajectory of the set (bild_gauss_dwell_first_contact),
    target the bit mask of the states of the set: a dict of logev, log_never (n_traj,), n_nan_windows (n_traj,) int64 and
    log_first (n_traj, T_max), NaN behind a trajectory's T; T_max the set's longest trajectory
    """
    outputs = lambda n, S, T_max: {
        'logev': np.empty(n), 'n_nan_windows': np.empty(n, dtype=np.int64), 'log_first': np.empty((n, T_max)), 'log_never': np.empty(n)}
    return _dwell_call('bild_gauss_dwell_first_contact', DwellFirstContactOut, model, ts, (log_init, log_jump, log_dwell, log_surv),
                       outputs, scalars=(target,), omit=omit, scratch_bytes=scratch_bytes)


class DwellOccupancyOut(ctypes.Structure):
    _fields_ = [(name, ctypes.c_void_p) for name in ('logev', 'n_nan_windows', 'log_occ')]


def gauss_dwell_occupancy(model, ts, log_init, log_jump, log_dwell, log_surv, target, omit=False, scratch_bytes=0):
    """
    exact posterior of the number of frames in a set of states under a dwell-time prior for every trajectory of the set
    (bild_gauss_dwell_occupancy), target the bit mask of the states of the set: a dict of logev (n_traj,), n_nan_windows
    (n_traj,) int64 and log_occ (n_traj, T_max + 1, S), -inf behind a trajectory's T; T_max the set's longest trajectory
    """
    outputs = lambda n, S, T_max: {
        'logev': np.empty(n), 'n_nan_windows': np.empty(n, dtype=np.int64), 'log_occ': np.empty((n, T_max + 1, S))}
    return _dwell_call('bild_gauss_dwell_occupancy', DwellOccupancyOut, model, ts, (log_init, log_jump, log_dwell, log_surv), outputs,
                       scalars=(target,), omit=omit, scratch_bytes=scratch_bytes)


class DwellVisitsOut(ctypes.Structure):
    _fields_ = [(name, ctypes.c_void_p) for name in ('logev', 'n_nan_windows', 'log_visits', 'log_tail')]


def gauss_dwell_visits(model, ts, log_init, log_jump, log_dwell, log_surv, target, n_max, omit=False, scratch_bytes=0):
    """
    exact posterior of the number of visits to a set of states under a dwell-time prior for every trajectory of the set
    (bild_gauss_dwell_visits, include/bild_amd_visits.h), target the bit mask of the states of the set: a dict of logev,
    log_tail (n_traj,), n_nan_windows (n_traj,) int64 and log_visits (n_traj, n_max + 1, S), -inf behind a trajectory's
    (T + 1) // 2
    """
    outputs = lambda n, S, T_max: {
        'logev': np.empty(n), 'n_nan_windows': np.empty(n, dtype=np.int64), 'log_visits': np.empty((n, max(int(n_max), -1) + 1, S)),
        'log_tail': np.empty(n)}        # (a negative n_max: no row, and the call refuses it)
    return _dwell_call('bild_gauss_dwell_visits', DwellVisitsOut, model, ts, (log_init, log_jump, log_dwell, log_surv), outputs,
                       scalars=(n_max, target), omit=omit, scratch_bytes=scratch_bytes)


class DwellWindowsOut(ctypes.Structure):
    _fields_ = [(name, ctypes.c_void_p) for name in ('logev', 'log_all', 'n_nan_windows')]


def gauss_dwell_windows(model, ts, log_init, log_jump, log_dwell, log_surv, win_traj, win_u, win_v, win_target, omit=False,
                        scratch_bytes=0):
    """
    exact window support under a dwell-time prior (bild_gauss_dwell_windows, include/bild_amd_windows.h): query i asks for
    log P(every frame of [win_u[i], win_v[i]) is in the states of the bit mask win_target[i] | data) on trajectory win_traj[i] of
    the set, win_traj not decreasing.  A dict of logev (n_traj,), log_all (n_win,) and n_nan_windows (n_traj,) int64
    """
    (log_init, log_jump, log_dwell, log_surv), L = _dwell_tables(model, log_init, log_jump, log_dwell, log_surv)
    win_traj, win_u, win_v = i32(win_traj), i32(win_u), i32(win_v)
    win_target = np.ascontiguousarray(win_target, dtype=np.uint32)
    n = len(win_traj)
    assert win_traj.shape == win_u.shape == win_v.shape == win_target.shape == (n,)
    T_max = int(np.max(ts.T))
    res = {'logev': np.empty(ts.n_traj), 'log_all': np.empty(n), 'n_nan_windows': np.empty(ts.n_traj, dtype=np.int64)}
    spec = _out(DwellWindowsOut, res)
    check(lib().bild_gauss_dwell_windows(model._h, ts._h, L, dptr(log_init), dptr(log_jump), dptr(log_dwell), dptr(log_surv), T_max,
                                         int(scratch_bytes), n, iptr(win_traj), iptr(win_u), iptr(win_v), aptr(win_target),
                                         DWELL_NAN_OMIT if omit else DWELL_NAN_PROPAGATE, ctypes.byref(spec)))
    return res


class DwellFilterOut(ctypes.Structure):
    _fields_ = [(name, ctypes.c_void_p) for name in ('logev', 'prefix_logev', 'log_filtered', 'run_mean', 'log_run', 'n_nan_windows')]


def gauss_dwell_filter(model, ts, log_init, log_jump, log_dwell, log_surv, run_max=0, omit=False, scratch_bytes=0):
    """
    exact online filtering under a dwell-time prior for every trajectory of the set (bild_gauss_dwell_filter): a dict of logev
    (n_traj,), prefix_logev and run_mean (n_traj, T_max), log_filtered (n_traj, S, T_max), n_nan_windows (n_traj, T_max) int64
    and, with run_max > 0, log_run (n_traj, S, T_max, run_max) (None without); T_max the set's longest trajectory
    """
    outputs = lambda n, S, T_max: {
        'logev': np.empty(n), 'prefix_logev': np.empty((n, T_max)), 'log_filtered': np.empty((n, S, T_max)),
        'run_mean': np.empty((n, T_max)), 'log_run': np.empty((n, S, T_max, int(run_max))) if int(run_max) > 0 else None,
        'n_nan_windows': np.empty((n, T_max), dtype=np.int64)}
    return _dwell_call('bild_gauss_dwell_filter', DwellFilterOut, model, ts, (log_init, log_jump, log_dwell, log_surv), outputs,
                       scalars=(run_max,), omit=omit, scratch_bytes=scratch_bytes)


DWELL_LAG_MAX = 63      # BILD_DWELL_LAG_MAX: a window of lag + 1 frames is one wavefront


class DwellLagOut(ctypes.Structure):
    _fields_ = [(name, ctypes.c_void_p) for name in ('logev', 'log_lagged', 'n_nan_windows')]


def gauss_dwell_lag(model, ts, log_init, log_jump, log_dwell, log_surv, lag, omit=False, scratch_bytes=0):
    """
    exact fixed-lag smoothing under a dwell-time prior for every trajectory of the set (bild_gauss_dwell_lag): a dict of logev
    (n_traj,), log_lagged (n_traj, S, T_max, lag + 1) and n_nan_windows (n_traj, T_max) int64; T_max the set's longest trajectory
    """
    outputs = lambda n, S, T_max: {
        'logev': np.empty(n), 'log_lagged': np.empty((n, S, T_max, max(int(lag), 0) + 1)),
        'n_nan_windows': np.empty((n, T_max), dtype=np.int64)}
    return _dwell_call('bild_gauss_dwell_lag', DwellLagOut, model, ts, (log_init, log_jump, log_dwell, log_surv), outputs,
                       scalars=(lag,), omit=omit, scratch_bytes=scratch_bytes)


class DwelldrawOut(ctypes.Structure):
    _fields_ = [(name, ctypes.c_void_p) for name in ('states', 'n_switches', 'logl', 'log_prior', 'n_uniforms', 'uniforms_out')]


def gauss_dwell_draw(model, ts, log_init, log_jump, log_dwell, log_surv, draw_traj, draw_stream=None, uniforms=None, keep_uniforms=0,
                     seed=0, scratch_bytes=0):
    """
    exact posterior draws of profiles under a dwell-time prior (bild_gauss_dwell_draw): draw r on trajectory draw_traj[r] of
    the set, from its row of ``uniforms`` (n, U) or, without them, from Philox stream draw_stream[r] (None: r) of ``seed``.  A
    dict of states (n, T_max) uint8, n_switches, n_uniforms (n,) int32, logl, log_prior (n,) and uniforms (n, U): the first U
    consumed, U = ``keep_uniforms`` in device mode (None where U = 0); T_max the set's longest trajectory
    """
    S = model.S
    (log_init, log_jump, log_dwell, log_surv), L = _dwell_tables(model, log_init, log_jump, log_dwell, log_surv)
    draw_traj = i32(draw_traj)
    n, U = len(draw_traj), int(keep_uniforms)
    assert draw_traj.shape == (n,)
    if draw_stream is not None:
        draw_stream = np.ascontiguousarray(draw_stream, dtype=np.int64)
        assert draw_stream.shape == (n,)
    if uniforms is not None:
        uniforms = f64(uniforms)
        assert uniforms.ndim == 2 and len(uniforms) == n
        U = uniforms.shape[1]
    T_max = int(np.max(ts.T))
    res = {'states': np.empty((n, T_max), dtype=np.uint8), 'n_switches': np.empty(n, dtype=np.int32), 'logl': np.empty(n),
           'log_prior': np.empty(n), 'n_uniforms': np.empty(n, dtype=np.int32), 'uniforms': np.zeros((n, U)) if U > 0 else None}
    spec = _out(DwelldrawOut, res, rename={'uniforms': 'uniforms_out'})
    check(lib().bild_gauss_dwell_draw(model._h, ts._h, L, dptr(log_init), dptr(log_jump), dptr(log_dwell), dptr(log_surv), T_max,
                                      int(scratch_bytes), n, iptr(draw_traj), None if draw_stream is None else aptr(draw_stream), U,
                                      None if uniforms is None else aptr(uniforms), int(seed) & (2 ** 64 - 1), ctypes.byref(spec)))
    return res
