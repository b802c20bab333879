"""ctypes binding of libsfmcore.so (include/sfmcore.h) for the drop-in modules.

This is the only route to compute: there is no CPU fallback.  Importing this
module fails loudly if the HIP library has not been built, and every compute
call raises ``SfmCoreError`` if no MI355X is visible.

The device is ``$SFM_DEVICE`` (default 0).
"""
import array
import ctypes
import os
import random

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsfmcore.so")


class SfmCoreError(RuntimeError):
    pass


if not os.path.exists(LIB_PATH):
    raise ImportError(f"libsfmcore.so not built at {LIB_PATH}: run `make -C {_HERE}` "
                      "(or __graft_entry__.build()); there is no CPU fallback")

_lib = ctypes.CDLL(LIB_PATH)

_d = ctypes.POINTER(ctypes.c_double)
_i32 = ctypes.POINTER(ctypes.c_int32)
_u32 = ctypes.POINTER(ctypes.c_uint32)
_i64 = ctypes.POINTER(ctypes.c_int64)
_u8 = ctypes.POINTER(ctypes.c_uint8)
_u64 = ctypes.POINTER(ctypes.c_uint64)
_f32 = ctypes.POINTER(ctypes.c_float)
_c = ctypes.c_int
_i = ctypes.c_int64
_v = ctypes.c_void_p


class BAOpts(ctypes.Structure):
    _fields_ = [("max_iterations", ctypes.c_int32), ("fixed_iterations", ctypes.c_int32),
                ("function_tolerance", ctypes.c_double), ("gradient_tolerance", ctypes.c_double),
                ("parameter_tolerance", ctypes.c_double), ("initial_lambda", ctypes.c_double)]


class BAReport(ctypes.Structure):
    _fields_ = [("iterations", ctypes.c_int32), ("accepted", ctypes.c_int32), ("status", ctypes.c_int32),
                ("n_ranks", ctypes.c_int32), ("cost0", ctypes.c_double), ("cost", ctypes.c_double),
                ("t_setup_ms", ctypes.c_double), ("t_loop_ms", ctypes.c_double),
                ("t_download_ms", ctypes.c_double), ("lambda_", ctypes.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


# (name, restype, argtypes) -- every symbol include/sfmcore.h declares
SIGNATURES = [
    ("sfm_version", _c, []),
    ("sfm_last_error", ctypes.c_char_p, []),
    ("sfm_device_count", _c, []),
    ("sfm_last_timings", _c, [_d, _c]),
    ("sfm_set_call_timing", _c, [_c]),
    ("sfm_pyrandom_sample_table", _c, [_u32, _i, ctypes.c_int32, _i, _i32]),
    ("sfm_f8_batch", _c, [_d, _d, _i, _d, _c]),
    ("sfm_f8_general", _c, [_d, _d, _i, _d, _c]),
    ("sfm_ransac_f8", _c, [_d, _d, _i, _i32, _i, ctypes.c_double, _i32, _i64, _d, _u8, _c]),
    # the in-call-sampling entries take raw addresses (c_void_p): the drop-in
    # calls them once per image pair and .ctypes.data_as costs ~4 us a pointer
    ("sfm_ransac_f8_pyrandom", _c, [_v, _v, _i, _v, _i, ctypes.c_double, _v, _v, _v, _v, _v, _c]),
    ("sfm_ransac_f8_dropin", _c, [_v, _v, _i, _v, _i, ctypes.c_double, _v, _v, _v, _v, _c]),
    ("sfm_ransac_f8_range", _c, [_d, _d, _i, _i32, _i, _i, _i, ctypes.c_double, _i32, _u64, _d, _c]),
    ("sfm_ransac_f8_pyrandom_range", _c, [_d, _d, _i, _u32, _i, _i, _i, ctypes.c_double, _i32, _u64, _d, _c]),
    ("sfm_ransac_f8_mask", _c, [_d, _d, _i, _d, ctypes.c_double, _u8, _c]),
    ("sfm_ransac_h4_pyrandom_range", _c, [_d, _d, _i, _u32, _i, _i, _i, ctypes.c_double, _i32, _u64, _d, _c]),
    ("sfm_ransac_h4_mask", _c, [_d, _d, _i, _d, ctypes.c_double, _u8, _c]),
    ("sfm_ransac_combine", _c, [ctypes.c_void_p, _u64, _d]),
    ("sfm_h4_batch", _c, [_d, _d, _i, _d, _c]),
    ("sfm_homography_general", _c, [_d, _d, _i, _d, _c]),
    ("sfm_ransac_h4", _c, [_d, _d, _i, _i32, _i, ctypes.c_double, _i32, _i64, _d, _u8, _c]),
    ("sfm_ransac_h4_pyrandom", _c, [_v, _v, _i, _v, _i, ctypes.c_double, _v, _v, _v, _v, _v, _c]),
    ("sfm_linear_pnp", _c, [_d, _d, _i, _d, _d, _d, _i32, _c]),
    ("sfm_pnp_ransac", _c, [_d, _d, _i, _d, _i32, _i, ctypes.c_double, _i32, _i32, _i64, _i64, _d, _d, _c]),
    ("sfm_nonlinear_pnp", _c, [_d, _d, _i, _d, _d, _d, ctypes.c_int32, _d, _d, _i32, _c]),
    ("sfm_matching_parse", _c, [ctypes.c_char_p, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_void_p),
                                _i64, _i64]),
    ("sfm_matching_read", _c, [ctypes.c_void_p, _i32, _i32, _d, _d]),
    ("sfm_matching_free", _c, [ctypes.c_void_p]),
    ("sfm_dense_obs_scan", _c, [ctypes.c_void_p, ctypes.c_int32, _i, _i, _i64, _i, ctypes.c_int32, _d, _d, _i,
                                ctypes.c_int32, ctypes.POINTER(ctypes.c_void_p), _i64]),
    ("sfm_dense_obs_read", _c, [ctypes.c_void_p, _i32, _i32, _d]),
    ("sfm_dense_obs_free", _c, [ctypes.c_void_p]),
    ("sfm_gather_rows3", _c, [_d, _i, _i64, _i, _d]),
    ("sfm_matrix_to_rotvec", ctypes.c_int64, [_d, _i, _d]),
    ("sfm_rotvec_to_matrix", _c, [_d, _i, _d]),
    ("sfm_triangulate_dlt", _c, [_d, _d, _d, _d, _i, _d, _c]),
    ("sfm_two_view_select", _c, [_d, _d, _d, _d, _d, _d, ctypes.c_int32, _d, _d, _i, _i64, _i32, _d, _d, _c]),
    ("sfm_cheirality_count", _c, [_d, _d, _d, _d, ctypes.c_int32, _d, _i, _i64, _i32, _c]),
    ("sfm_triangulate_nonlinear", _c, [_d, _d, _d, _d, _d, _i, ctypes.c_int32, _d, _i32, _c]),
    ("sfm_triangulate_tracks", _c, [_d, ctypes.c_int32, _i64, _i, _i32, _d, _i, _d, ctypes.c_int32, ctypes.c_int32,
                                    _d, _d, _u8, _i32, _c]),
    ("sfm_triangulate_tracks_robust", _c, [_d, ctypes.c_int32, _d, _i64, _i, _i32, _d, _i, ctypes.c_double,
                                           ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _d, _d,
                                           _i32, _u8, _i32, _i32, _i32, _d, _c]),
    ("sfm_register_views", _c, [_d, _d, _i, _i64, _i, _i32, _d, _i, _i32, _i, ctypes.c_double, ctypes.c_int32,
                                ctypes.c_int32, ctypes.c_int32, _d, _d, _d, _i32, _i32, _i32, _i32, _u8, _i32, _d,
                                _c]),
    ("sfm_register_views_p3p", _c, [_d, _d, _i, _i64, _i, _i32, _d, _i, _i32, _i, ctypes.c_double, ctypes.c_int32,
                                    ctypes.c_int32, ctypes.c_int32, _d, _d, _d, _i32, _i32, _i32, _i32, _u8, _i32,
                                    _i32, _d, _c]),
    ("sfm_verify_pairs", _c, [_i64, _i, _d, _d, _i, _i32, _i, ctypes.c_double, ctypes.c_int32, ctypes.c_int32, _d,
                              _d, _i32, _i32, _i32, _i32, _u8, _i32, _d, _c]),
    ("sfm_essential_pairs", _c, [_d, _i64, _i, _d, _d, _i, _i32, _i, ctypes.c_double, ctypes.c_int32, ctypes.c_int32,
                                 ctypes.c_int32, _d, _d, _d, _i32, _i32, _i32, _i32, _u8, _i32, _i32, _d, _c]),
    ("sfm_init_pairs", _c, [_d, _i64, _i, _d, _d, _i, _d, _i32, _i, ctypes.c_double, ctypes.c_double, _d, _d, _i64,
                            _i32, _i32, _d, _i32, _i32, _d, _i32, _d, _u8, _d, _d, _i32, _d, _c]),
    ("sfm_average_rotations", _c, [ctypes.c_int32, _i32, _d, _d, _i, ctypes.c_uint64, ctypes.c_double, ctypes.c_int32,
                                   ctypes.c_int32, ctypes.c_double, _d, _d, _u8, _i32, _i32, _i32, _i32, _i32, _c]),
    ("sfm_average_rotations_cg", _c, [ctypes.c_int32, _i32, _d, _d, _i, ctypes.c_uint64, ctypes.c_double,
                                      ctypes.c_int32, ctypes.c_int32, ctypes.c_double, ctypes.c_double, ctypes.c_int32,
                                      _d, _d, _u8, _i32, _i32, _i32, _i32, _i32, _i32, _d, _d, _c]),
    ("sfm_average_positions", _c, [ctypes.c_int32, _i32, _d, _d, _i, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                   ctypes.c_int32, ctypes.c_double, ctypes.c_int32, ctypes.c_int32, _d, _d, _u8, _d,
                                   _i32, _i32, _d, _i32, _i32, _c]),
    ("sfm_merge_tracks", _c, [_i64, _i, _i32, _d, _d, _i, ctypes.c_int32, ctypes.c_int32, _i32, _i32, _u8, _i32, _i64,
                              _i32, _i64, _i32, _i32, _c]),
    ("sfm_match_descriptors", _c, [_u8, _i, _i64, ctypes.c_int32, ctypes.c_int32, _i32, _i, ctypes.c_double,
                                   ctypes.c_int32, ctypes.c_int32, _i, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32,
                                   _c]),
    ("sfm_match_descriptors_guided", _c, [_u8, _d, _i, _i64, ctypes.c_int32, ctypes.c_int32, _i32, _d, _i,
                                          ctypes.c_double, ctypes.c_double, ctypes.c_int32, ctypes.c_int32, _i, _i64,
                                          _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _c]),
    ("sfm_extract_features", _c, [_u8, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                  ctypes.c_double, ctypes.c_double, ctypes.c_double, _i, _i64, _d, _f32, _f32, _f32,
                                  _u8, _i32, _f32, _i, _i64, _i32, _u8, _i32, _f32, _c]),
    ("sfm_vocab_train", _c, [_u8, _i, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _u8, _i32, _i64, _i64, _i32, _c]),
    ("sfm_select_pairs", _c, [_i32, _i, _i64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _i32, _d, _i64, _i64,
                              _i32, _c]),
    ("sfm_project_points", _c, [_d, _d, _i, _d, _c]),
    ("sfm_reduced_solve", _c, [_d, _d, ctypes.c_int32, _d, _c]),
    ("sfm_ba_residuals", _c, [ctypes.c_int32, _i, _i, _i32, _i32, _d, _d, _d, _d, _d, _c]),
    ("sfm_ba_lm", _c, [ctypes.c_int32, _i, _i, _i32, _i32, _d, _d, _d, _d, ctypes.POINTER(BAOpts),
                       ctypes.POINTER(BAReport), _c]),
    ("sfm_ba_lm_dense", _c, [ctypes.c_void_p, ctypes.c_int32, _i, _d, _d, _d, ctypes.POINTER(BAOpts),
                             ctypes.POINTER(BAReport), _c]),
    ("sfm_comm_unique_id", _c, [ctypes.c_char_p]),
    ("sfm_comm_init", _c, [ctypes.c_char_p, _c, _c, _c, ctypes.POINTER(ctypes.c_void_p)]),
    ("sfm_comm_init_local", _c, [_c, ctypes.POINTER(ctypes.c_void_p)]),
    ("sfm_comm_destroy", _c, [ctypes.c_void_p]),
    ("sfm_ba_create", _c, [ctypes.c_int32, _i, _i, _i32, _i32, _d, _d, _d, _d, _c, ctypes.c_void_p,
                           ctypes.POINTER(ctypes.c_void_p)]),
    ("sfm_ba_solve", _c, [ctypes.c_void_p, ctypes.POINTER(BAOpts), ctypes.POINTER(BAReport)]),
    ("sfm_ba_reset", _c, [ctypes.c_void_p]),
    ("sfm_ba_plan_digest", _c, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]),
    ("sfm_ba_spec_plan", _c, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32)]),
    ("sfm_ba_download", _c, [ctypes.c_void_p, _d, _d]),
    ("sfm_ba_kernel_times", _c, [ctypes.c_void_p, _d, _c, ctypes.c_char_p, _c]),
    ("sfm_ba_set_timing", _c, [ctypes.c_void_p, _c]),
    ("sfm_ba_destroy", _c, [ctypes.c_void_p]),
    ("sfm_ba_lm_multi", _c, [ctypes.c_int32, _i, _i, _i32, _i32, _d, _d, _d, _d, ctypes.POINTER(BAOpts),
                             ctypes.POINTER(BAReport), ctypes.POINTER(ctypes.c_int), _c]),
]
for _name, _res, _args in SIGNATURES:
    _f = getattr(_lib, _name)
    _f.restype = _res
    _f.argtypes = _args

DEVICE = int(os.environ.get("SFM_DEVICE", "0"))


def version():
    return _lib.sfm_version()


def device_count():
    return _lib.sfm_device_count()


_DEVICE_SEEN = False


def require_device():
    """Fail loudly without a HIP device (no CPU fallback); once a device has
    been seen the check is skipped (~2 us of a 0.19-ms RANSAC call)."""
    global _DEVICE_SEEN
    if _DEVICE_SEEN:
        return
    if _lib.sfm_device_count() <= 0:
        raise SfmCoreError("libsfmcore: no HIP device visible (the MI355X path has no CPU fallback)")
    _DEVICE_SEEN = True


def _check(rc):
    if rc != 0:
        raise SfmCoreError(f"libsfmcore error {rc}: {_lib.sfm_last_error().decode(errors='replace')}")


def _p(a, t=_d):
    return a.ctypes.data_as(t)


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None:
        a = a.reshape(shape)
    return a


def set_call_timing(on=True):
    """Device-side timings (HIP events) in the drop-in RANSAC calls."""
    _check(_lib.sfm_set_call_timing(int(bool(on))))


def last_timings():
    out = np.zeros(12)
    n = _lib.sfm_last_timings(_p(out), 12)
    return out[:n]


# ------------------------------------------------------------------ random
assert array.array("I").itemsize == 4

# The global generator's MT19937 state crosses the C-ABI as uint32[625] (624
# key words + position).  CPython keeps it inside the _random.Random object
# as {PyObject_HEAD; int index; uint32_t state[624]}; when import verifies
# that layout against random.getstate() (at three positions, one across a
# twist, and a write-back), the state is copied out of and back into the
# object with two memmoves -- random.getstate / setstate build and parse a
# 625-int tuple, ~25 us of every RANSAC drop-in call.  Otherwise (another
# interpreter, another layout) getstate / setstate.
_MT_INDEX = ctypes.sizeof(ctypes.c_ssize_t) + ctypes.sizeof(ctypes.c_void_p)  # after PyObject_HEAD
_MT_KEY = _MT_INDEX + 4
_MT_ZERO = bytes(625 * 4)


def _mt_layout_ok():
    import sys
    try:
        import _random
        inst = random.sample.__self__
        if (sys.implementation.name != "cpython" or not isinstance(inst, _random.Random)
                or _random.Random.__basicsize__ < _MT_KEY + 624 * 4):
            return False
    except (AttributeError, ImportError):
        return False
    saved = random.getstate()
    try:
        v, st, g = saved
        random.setstate((v, st[:624] + (623,), g))
        base = id(inst)
        for _ in range(3):  # positions 623, 624, then 1 after the twist
            _, cur, _ = random.getstate()
            raw = (ctypes.c_uint32 * 624).from_address(base + _MT_KEY)
            if tuple(raw) != cur[:624] or ctypes.c_int.from_address(base + _MT_INDEX).value != cur[624]:
                return False
            random.getrandbits(32)
        ctypes.c_int.from_address(base + _MT_INDEX).value = 5  # write-back
        return random.getstate()[1][624] == 5
    finally:
        random.setstate(saved)


_MT_DIRECT = _mt_layout_ok()


def _mt_state():
    """The global MT19937 state as a C uint32[625] (key + position) plus what
    _mt_restore needs to put it back (array.array: ~3x cheaper than numpy
    for the 625-int round trip of the getstate path)."""
    if _MT_DIRECT:
        base = id(random.sample.__self__)
        st = array.array("I", _MT_ZERO)
        ctypes.memmove(st.buffer_info()[0], base + _MT_KEY, 624 * 4)
        st[624] = ctypes.c_int.from_address(base + _MT_INDEX).value
        return base, st, None
    version_, internal, gauss = random.getstate()
    return version_, array.array("I", internal), gauss


def _mt_ptr(st):
    return ctypes.cast(st.buffer_info()[0], _u32)


def _mt_restore(h, st, gauss):
    if _MT_DIRECT:
        ctypes.memmove(h + _MT_KEY, st.buffer_info()[0], 624 * 4)
        ctypes.c_int.from_address(h + _MT_INDEX).value = st[624]
        return
    random.setstate((h, tuple(st), gauss))


def sample_table(n, k, H):
    """H draws of random.sample(range(n), k) on the GLOBAL random instance,
    replayed natively; the global state is advanced exactly as the
    reference's loop (GetInliersRANSAC.py:53-55) would advance it."""
    version_, st, gauss = _mt_state()
    out = np.empty((H, k), dtype=np.int32)
    _check(_lib.sfm_pyrandom_sample_table(_mt_ptr(st), int(n), int(k), int(H), _p(out, _i32)))
    _mt_restore(version_, st, gauss)
    return out


# --------------------------------------------------------------- geometry
def f8_batch(x1s, x2s):
    """H independent 8-point F estimates; x1s, x2s: (H, 8, 2)."""
    require_device()
    x1s, x2s = _f64(x1s), _f64(x2s)
    H = x1s.shape[0]
    F = np.zeros((H, 9))
    _check(_lib.sfm_f8_batch(_p(x1s), _p(x2s), H, _p(F), DEVICE))
    return F.reshape(H, 3, 3)


def f8_general(x1, x2):
    require_device()
    x1, x2 = _f64(x1), _f64(x2)
    F = np.zeros(9)
    _check(_lib.sfm_f8_general(_p(x1), _p(x2), len(x1), _p(F), DEVICE))
    return F.reshape(3, 3)


def ransac_f8(x1, x2, samples, thr, want_counts=False, device=None):
    """Returns (best_iter or -1, F_best (3,3) or None, mask (N,) bool, counts or None)."""
    require_device()
    x1, x2 = _f64(x1), _f64(x2)
    samples = np.ascontiguousarray(samples, dtype=np.int32)
    N, H = len(x1), len(samples)
    counts = np.zeros(H, dtype=np.int32) if want_counts else None
    best = np.zeros(1, dtype=np.int64)
    F = np.zeros(9)
    mask = np.zeros(N, dtype=np.uint8)
    _check(_lib.sfm_ransac_f8(_p(x1), _p(x2), N, _p(samples, _i32), H, float(thr),
                              _p(counts, _i32) if want_counts else None, _p(best, _i64), _p(F),
                              _p(mask, _u8), DEVICE if device is None else device))
    b = int(best[0])
    if b < 0:
        return -1, None, np.zeros(N, dtype=bool), counts
    return b, F.reshape(3, 3), mask.astype(bool), counts


def _ransac_pyrandom(fn, x1, x2, H, thr, want_counts, want_samples, device):
    """Shared body of the in-call-sampling RANSAC entries: the GLOBAL random
    state goes in, comes back advanced as H random.sample draws would."""
    require_device()
    x1, x2 = _f64(x1), _f64(x2)
    N = len(x1)
    version_, st, gauss = _mt_state()
    counts = np.zeros(H, dtype=np.int32) if want_counts else None
    samples = np.zeros((H, fn[1]), dtype=np.int32) if want_samples else None
    best = np.zeros(1, dtype=np.int64)
    M = np.zeros(9)
    mask = np.zeros(N, dtype=bool)  # written as 0/1 bytes by the library
    _check(fn[0](x1.ctypes.data, x2.ctypes.data, N, st.buffer_info()[0], int(H), float(thr),
                 counts.ctypes.data if want_counts else None, best.ctypes.data, M.ctypes.data, mask.ctypes.data,
                 samples.ctypes.data if want_samples else None, DEVICE if device is None else device))
    _mt_restore(version_, st, gauss)
    b = int(best[0])
    if b < 0:
        return -1, None, np.zeros(N, dtype=bool), counts, samples
    return b, M.reshape(3, 3), mask, counts, samples


def ransac_f8_pyrandom(x1, x2, H, thr, want_counts=False, want_samples=False, device=None):
    """GetInliersRANSAC's whole loop with the H 8-point samples drawn inside
    the call from the global random stream (sfm_ransac_f8_pyrandom).
    Returns (best_iter or -1, F_best or None, mask, counts or None, samples or None)."""
    return _ransac_pyrandom((_lib.sfm_ransac_f8_pyrandom, 8), x1, x2, H, thr, want_counts, want_samples, device)


def ransac_f8_dropin(x1, x2, H, thr, device=None):
    """GetInliersRANSAC's loop as its drop-in needs it (sfm_ransac_f8_dropin):
    (best_iter or -1, F_best or None, split, n_inliers) -- split[:n_inliers]
    the winner's inlier positions, split[n_inliers:] the outliers'."""
    require_device()
    x1, x2 = _f64(x1), _f64(x2)
    N = len(x1)
    h, st, gauss = _mt_state()
    out = np.zeros(2, dtype=np.int64)  # best_iter, n_inliers
    M = np.empty(9)
    split = np.empty(N, dtype=np.int64)
    oa = out.ctypes.data
    _check(_lib.sfm_ransac_f8_dropin(x1.ctypes.data, x2.ctypes.data, N, st.buffer_info()[0], int(H), float(thr), oa,
                                     M.ctypes.data, split.ctypes.data, oa + 8, DEVICE if device is None else device))
    _mt_restore(h, st, gauss)
    b = int(out[0])
    if b < 0:
        return -1, None, split[:0], 0
    return b, M.reshape(3, 3), split, int(out[1])


def ransac_h4_pyrandom(x1, x2, H, thr, want_counts=False, want_samples=False, device=None):
    """get_homography_inliers' loop with in-call sampling (sfm_ransac_h4_pyrandom)."""
    return _ransac_pyrandom((_lib.sfm_ransac_h4_pyrandom, 4), x1, x2, H, thr, want_counts, want_samples, device)


# ------------------------------------------- hypothesis-sharded RANSAC (§8(e))
def _ransac_range(model, x1, x2, H, h0, h1, thr, samples=None, want_counts=False, device=None):
    require_device()
    x1, x2 = _f64(x1), _f64(x2)
    N = len(x1)
    counts = np.zeros(max(h1 - h0, 0), dtype=np.int32) if want_counts else None
    key = np.zeros(1, dtype=np.uint64)
    M = np.zeros(9)
    dev = DEVICE if device is None else device
    cp = _p(counts, _i32) if want_counts else None
    if samples is not None:
        assert model == 8, "a given sample table is supported for the F model"
        samples = np.ascontiguousarray(samples, dtype=np.int32)
        assert samples.shape == (H, 8)
        _check(_lib.sfm_ransac_f8_range(_p(x1), _p(x2), N, _p(samples, _i32), int(H), int(h0), int(h1), float(thr),
                                        cp, _p(key, _u64), _p(M), dev))
    else:
        fn = _lib.sfm_ransac_f8_pyrandom_range if model == 8 else _lib.sfm_ransac_h4_pyrandom_range
        version_, st, gauss = _mt_state()
        _check(fn(_p(x1), _p(x2), N, _mt_ptr(st), int(H), int(h0), int(h1), float(thr), cp, _p(key, _u64), _p(M), dev))
        _mt_restore(version_, st, gauss)
    return int(key[0]), M.reshape(3, 3), counts


def ransac_f8_range(x1, x2, H, h0, h1, thr, samples=None, want_counts=False, device=None):
    """One hypothesis shard [h0, h1) of an H-hypothesis F-RANSAC.  Without
    `samples` the whole table is drawn from the GLOBAL random stream (which
    ends where the unsharded call leaves it) and only the shard is scored.
    Returns (key, F of the shard winner, counts or None); key = count << 32 |
    (0xFFFFFFFF - iteration), 0 if no hypothesis has an inlier."""
    return _ransac_range(8, x1, x2, H, h0, h1, thr, samples, want_counts, device)


def ransac_h4_range(x1, x2, H, h0, h1, thr, want_counts=False, device=None):
    """Homography counterpart of ransac_f8_range (in-call sampling)."""
    return _ransac_range(4, x1, x2, H, h0, h1, thr, None, want_counts, device)


def ransac_mask(x1, x2, M, thr, model=8, device=None):
    """Inlier mask of one model (the winner's emit after the combine)."""
    require_device()
    x1, x2, M = _f64(x1), _f64(x2), _f64(M)
    mask = np.zeros(len(x1), dtype=np.uint8)
    fn = _lib.sfm_ransac_f8_mask if model == 8 else _lib.sfm_ransac_h4_mask
    _check(fn(_p(x1), _p(x2), len(x1), _p(M), float(thr), _p(mask, _u8), DEVICE if device is None else device))
    return mask.astype(bool)


def ransac_combine(comm, key, M):
    """Max of the ranks' keys over `comm` (RCCL or an in-process group) and
    the winner's model.  Returns (key, model)."""
    k = np.array([key], dtype=np.uint64)
    M = np.array(M, dtype=np.float64).reshape(9).copy()
    _check(_lib.sfm_ransac_combine(comm.h if hasattr(comm, "h") else comm, _p(k, _u64), _p(M)))
    return int(k[0]), M.reshape(3, 3)


def local_group(nranks):
    """An in-process rank group (sfm_comm_init_local): one handle per rank,
    for N host threads sharing one process (and possibly one GPU)."""
    hs = (ctypes.c_void_p * nranks)()
    _check(_lib.sfm_comm_init_local(nranks, hs))
    return [LocalComm(h, nranks, r) for r, h in enumerate(hs)]


class LocalComm:
    def __init__(self, h, nranks, rank):
        self.h = ctypes.c_void_p(h)
        self.nranks, self.rank = nranks, rank

    def close(self):
        if self.h:
            _lib.sfm_comm_destroy(self.h)
            self.h = ctypes.c_void_p()


def h4_batch(x1s, x2s):
    """H independent 4-point homographies; x1s, x2s: (H, 4, 2)."""
    require_device()
    x1s, x2s = _f64(x1s), _f64(x2s)
    H = x1s.shape[0]
    out = np.zeros((H, 9))
    _check(_lib.sfm_h4_batch(_p(x1s), _p(x2s), H, _p(out), DEVICE))
    return out.reshape(H, 3, 3)


def homography_general(x1, x2):
    require_device()
    x1, x2 = _f64(x1), _f64(x2)
    out = np.zeros(9)
    _check(_lib.sfm_homography_general(_p(x1), _p(x2), len(x1), _p(out), DEVICE))
    return out.reshape(3, 3)


def ransac_h4(x1, x2, samples, thr, want_counts=False, device=None):
    """Returns (best_iter or -1, H_best (3,3) or None, mask (N,) bool, counts or None)."""
    require_device()
    x1, x2 = _f64(x1), _f64(x2)
    samples = np.ascontiguousarray(samples, dtype=np.int32)
    N, H = len(x1), len(samples)
    counts = np.zeros(H, dtype=np.int32) if want_counts else None
    best = np.zeros(1, dtype=np.int64)
    Hb = np.zeros(9)
    mask = np.zeros(N, dtype=np.uint8)
    _check(_lib.sfm_ransac_h4(_p(x1), _p(x2), N, _p(samples, _i32), H, float(thr),
                              _p(counts, _i32) if want_counts else None, _p(best, _i64), _p(Hb),
                              _p(mask, _u8), DEVICE if device is None else device))
    b = int(best[0])
    if b < 0:
        return -1, None, np.zeros(N, dtype=bool), counts
    return b, Hb.reshape(3, 3), mask.astype(bool), counts


def linear_pnp(X, x, K):
    """Returns (C (3,), R (3,3), branch)."""
    require_device()
    X, x, K = _f64(np.reshape(X, (-1, 3))), _f64(np.reshape(x, (-1, 2))), _f64(K)
    C, R, br = np.zeros(3), np.zeros(9), np.zeros(1, dtype=np.int32)
    _check(_lib.sfm_linear_pnp(_p(X), _p(x), len(X), _p(K), _p(C), _p(R), _p(br, _i32), DEVICE))
    return C, R.reshape(3, 3), int(br[0])


def pnp_ransac(X, x, K, samples, thr, want_counts=False):
    """Returns (best_iter or -1, best_count, C, R, counts or None, branches or None)."""
    require_device()
    X, x, K = _f64(np.reshape(X, (-1, 3))), _f64(np.reshape(x, (-1, 2))), _f64(K)
    samples = np.ascontiguousarray(samples, dtype=np.int32)
    H = len(samples)
    counts = np.zeros(H, dtype=np.int32) if want_counts else None
    branches = np.zeros(H, dtype=np.int32) if want_counts else None
    best, bc = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64)
    C, R = np.zeros(3), np.zeros(9)
    _check(_lib.sfm_pnp_ransac(_p(X), _p(x), len(X), _p(K), _p(samples, _i32), H, float(thr),
                               _p(counts, _i32) if want_counts else None,
                               _p(branches, _i32) if want_counts else None, _p(best, _i64), _p(bc, _i64),
                               _p(C), _p(R), DEVICE))
    return int(best[0]), int(bc[0]), C, R.reshape(3, 3), counts, branches


def nonlinear_pnp(X, x, K, C0, R0, max_nfev=100, want_flags=False):
    """Returns (C (3,), R (3,3), info) -- info MINPACK's code (-1: the
    reference's except path) -- and with want_flags the CholeskyQR flags
    (1: shifted pass-1 factor, a third pass ran; 2: a Gram factor failed)."""
    require_device()
    X, x, K = _f64(np.reshape(X, (-1, 3))), _f64(np.reshape(x, (-1, 2))), _f64(K)
    C0, R0 = _f64(np.reshape(C0, 3)), _f64(np.reshape(R0, (3, 3)))
    C, R, info = np.zeros(3), np.zeros(9), np.zeros(1, dtype=np.int32)
    _check(_lib.sfm_nonlinear_pnp(_p(X), _p(x), len(X), _p(K), _p(C0), _p(R0), int(max_nfev), _p(C), _p(R),
                                  _p(info, _i32), DEVICE))
    v = int(info[0])
    code, flags = (v & 0xff, v >> 8) if v >= 0 else (v, 0)
    return (C, R.reshape(3, 3), code, flags) if want_flags else (C, R.reshape(3, 3), code)


def parse_matching(data_path, no_of_images, n_threads=0):
    """Native matching-file reader (host threads, no device needed).
    Returns (n_features, feature, image, x, y) -- COO, feature-major."""
    h = ctypes.c_void_p()
    nf, no = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64)
    _check(_lib.sfm_matching_parse(os.fsencode(str(data_path)), int(no_of_images), int(n_threads), ctypes.byref(h),
                                   _p(nf, _i64), _p(no, _i64)))
    try:
        n = int(no[0])
        feat, img = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
        x, y = np.empty(n), np.empty(n)
        _check(_lib.sfm_matching_read(h, _p(feat, _i32), _p(img, _i32), _p(x), _p(y)))
    finally:
        _lib.sfm_matching_free(h)
    return int(nf[0]), feat, img, x, y


_DENSE_DTYPES = {np.dtype(np.float64): 0, np.dtype(np.float32): 1, np.dtype(np.int64): 2, np.dtype(np.int32): 3,
                 np.dtype(np.uint8): 4, np.dtype(np.bool_): 4}


class DenseScan:
    """The native dense -> COO scan kept in the library (sfm_dense_obs_scan):
    len() observations, .arrays() copies them out as (camera_indices,
    point_indices, points_2d), ba_lm_dense() solves from it without the
    arrays.  close() (or the context manager) hands the pieces back."""

    def __init__(self, handle, n):
        self.h, self.n = handle, n

    def __len__(self):
        return self.n

    def arrays(self):
        n = self.n
        cam, pt, obs = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32), np.empty((n, 2))
        _check(_lib.sfm_dense_obs_read(self.h, _p(cam, _i32), _p(pt, _i32), _p(obs)))
        return cam, pt, obs

    def close(self):
        if self.h:
            _lib.sfm_dense_obs_free(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()


def dense_scan(flags, feature_x, feature_y, rows, n_cams, n_threads=0):
    """np.where(flags[rows][:, :n_cams] == 1) and the coordinates at the hits,
    scanned natively (host threads, no device): a DenseScan, or None when the
    matrices' layout or dtype is not one the scanner reads (the caller then
    takes the numpy expression).  n_threads: row jobs (0: the library's)."""
    f, fx, fy = np.asarray(flags), np.asarray(feature_x), np.asarray(feature_y)
    if (f.ndim != 2 or fx.ndim != 2 or fx.shape != fy.shape or f.shape[0] != fx.shape[0]
            or f.dtype not in _DENSE_DTYPES or fx.dtype != np.float64 or fy.dtype != np.float64
            or f.strides[1] != f.itemsize or fx.strides != fy.strides or fx.strides[1] != 8
            or min(f.shape[1], fx.shape[1]) < n_cams):
        return None
    rows = np.ascontiguousarray(rows, dtype=np.int64)
    h = ctypes.c_void_p()
    no = np.zeros(1, dtype=np.int64)
    _check(_lib.sfm_dense_obs_scan(f.ctypes.data, _DENSE_DTYPES[f.dtype], f.strides[0], f.shape[0],
                                   _p(rows, _i64), len(rows),
                                   int(n_cams), fx.ctypes.data_as(_d), fy.ctypes.data_as(_d), fx.strides[0],
                                   int(n_threads), ctypes.byref(h), _p(no, _i64)))
    return DenseScan(h, int(no[0]))


def dense_observations(flags, feature_x, feature_y, rows, n_cams, n_threads=0):
    """Native dense -> COO scan (host threads, no device needed): the
    observations np.where(flags[rows][:, :n_cams] == 1) gives, in its order,
    with feature_x / feature_y at the hits.  Returns (camera_indices,
    point_indices, points_2d), or None when the matrices' layout or dtype is
    not one the scanner reads (the caller then takes the numpy expression)."""
    scan = dense_scan(flags, feature_x, feature_y, rows, n_cams, n_threads)
    if scan is None:
        return None
    with scan:
        return scan.arrays()


def gather_points(all_world_coords, rows):
    """np.asarray(all_world_coords, dtype=float64)[rows] for the BA drop-in's
    x0 (BundleAdjustment.py:196-197), gathered by the host pool when the array
    is a C-ordered float64 n x 3 one and every row is in range; otherwise the
    numpy expression (its conversions and its IndexError)."""
    a = np.asarray(all_world_coords)
    rows = np.asarray(rows)
    if (a.dtype != np.float64 or a.ndim != 2 or a.shape[1] != 3 or not a.flags.c_contiguous
            or rows.dtype != np.int64 or rows.ndim != 1 or not rows.flags.c_contiguous):
        return np.asarray(all_world_coords, dtype=np.float64)[rows]
    out = np.empty((len(rows), 3))
    if _lib.sfm_gather_rows3(a.ctypes.data_as(_d), a.shape[0], _p(rows, _i64), len(rows), _p(out)) != 0:
        return a[rows]  # an index out of range: numpy's IndexError
    return out


def matrix_to_rotvec(Rs):
    """Rotation.from_matrix(Rs).as_rotvec() for an (n, 3, 3) stack, with
    scipy's bits (csrc/rotations.cpp); scipy itself when a matrix is not
    orthogonal to within 1e-13 (scipy orthogonalises it first) or the input
    is not a C-ordered float64 stack."""
    R = np.asarray(Rs)
    if R.dtype == np.float64 and R.ndim == 3 and R.shape[1:] == (3, 3) and R.flags.c_contiguous:
        w = np.empty((len(R), 3))
        if _lib.sfm_matrix_to_rotvec(R.ctypes.data_as(_d), len(R), _p(w)) == 0:
            return w
    from scipy.spatial.transform import Rotation
    return Rotation.from_matrix(Rs).as_rotvec()


def rotvec_to_matrix(w):
    """Rotation.from_rotvec(w).as_matrix() for an (n, 3) array, with scipy's
    bits (csrc/rotations.cpp)."""
    w = np.ascontiguousarray(w, dtype=np.float64)
    if w.ndim != 2 or w.shape[1] != 3:
        from scipy.spatial.transform import Rotation
        return Rotation.from_rotvec(w).as_matrix()
    R = np.empty((len(w), 3, 3))
    _check(_lib.sfm_rotvec_to_matrix(_p(w), len(w), _p(R)))
    return R


def triangulate(P1, P2, x1, x2):
    require_device()
    P1, P2, x1, x2 = _f64(P1), _f64(P2), _f64(x1), _f64(x2)
    X = np.zeros((len(x1), 3))
    _check(_lib.sfm_triangulate_dlt(_p(P1), _p(P2), _p(x1), _p(x2), len(x1), _p(X), DEVICE))
    return X


def two_view_select(P1, P2s, R1, C1, Rs, Cs, x1, x2, return_all=False):
    """Every pose candidate triangulated and its cheirality count taken in one
    launch (sfm_two_view_select); P2s (M, 3, 4), Rs (M, 3, 3), Cs (M, 3).
    Returns (counts (M,) int64, best, X_best (N, 3), X_all (M, N, 3) or None)."""
    require_device()
    P1, R1, C1 = _f64(P1, (3, 4)), _f64(R1, (3, 3)), _f64(C1, (3,))
    M, N = len(P2s), len(x1)
    if len(Rs) != M or len(Cs) != M or len(x2) != N:
        raise ValueError("two_view_select: P2s, Rs, Cs need one entry per candidate and x1, x2 one row per point")
    P2s, Rs, Cs = _f64(P2s, (M, 3, 4)), _f64(Rs, (M, 3, 3)), _f64(Cs, (M, 3))
    x1, x2 = _f64(x1, (N, 2)), _f64(x2, (N, 2))
    counts = np.zeros(M, dtype=np.int64)
    best = np.zeros(1, dtype=np.int32)
    X_best = np.zeros((N, 3))
    X_all = np.zeros((M, N, 3)) if return_all else None
    _check(_lib.sfm_two_view_select(_p(P1), _p(P2s), _p(R1), _p(C1), _p(Rs), _p(Cs), M, _p(x1), _p(x2), N,
                                    _p(counts, _i64), _p(best, _i32), _p(X_best),
                                    _p(X_all) if return_all else None, DEVICE))
    return counts, int(best[0]), X_best, X_all


def cheirality_count(R1, C1, Rs, Cs, Xset):
    """Points in front of both cameras per candidate (sfm_cheirality_count);
    Xset (M, N, 3).  Returns (counts (M,) int64, best)."""
    require_device()
    R1, C1 = _f64(R1, (3, 3)), _f64(C1, (3,))
    Xset = _f64(Xset)
    if Xset.ndim != 3 or Xset.shape[2] != 3 or len(Rs) != len(Xset) or len(Cs) != len(Xset):
        raise ValueError("cheirality_count: Xset must be (M, N, 3) with one R and one C per candidate")
    M, N = Xset.shape[:2]
    Rs, Cs = _f64(Rs, (M, 3, 3)), _f64(Cs, (M, 3))
    counts = np.zeros(M, dtype=np.int64)
    best = np.zeros(1, dtype=np.int32)
    _check(_lib.sfm_cheirality_count(_p(R1), _p(C1), _p(Rs), _p(Cs), M, _p(Xset), N, _p(counts, _i64),
                                     _p(best, _i32), DEVICE))
    return counts, int(best[0])


def triangulate_nonlinear(P1, P2, x1, x2, X0, max_nfev=50):
    """Returns (X (N,3), info (N,) int32): MINPACK info, -1 = x0 kept."""
    require_device()
    P1, P2 = _f64(P1), _f64(P2)
    x1, x2 = _f64(np.reshape(x1, (-1, 2))), _f64(np.reshape(x2, (-1, 2)))
    X0 = _f64(np.reshape(X0, (-1, 3)))
    X = np.zeros((len(x1), 3))
    info = np.zeros(len(x1), dtype=np.int32)
    _check(_lib.sfm_triangulate_nonlinear(_p(P1), _p(P2), _p(x1), _p(x2), _p(X0), len(x1), int(max_nfev), _p(X),
                                          _p(info, _i32), DEVICE))
    return X, info


TRACKS_LINEAR, TRACKS_REFINE, TRACKS_BOTH = 0, 1, 2  # sfmcore.h SFM_TRACKS_*


def _csr_ok(start, idx, n_targets):
    """The library's CSR checks.  It makes them itself and reports what is
    wrong; only a call that would reach the device asks for one first."""
    return bool(start[0] == 0 and not np.any(np.diff(start) < 0) and start[-1] == len(idx)
                and (not len(idx) or (idx.min() >= 0 and idx.max() < n_targets)))


def triangulate_tracks(P, track_start, obs_cam, obs_xy, X0=None, refine=True, max_nfev=50):
    """One point per track from all of its views in one launch
    (sfm_triangulate_tracks).  P (n_cams, 3, 4); the tracks are CSR rows:
    track t owns obs_cam / obs_xy[track_start[t]:track_start[t + 1]], cameras
    ascending.  refine=False: the N-view DLT.  refine=True: the DLT, then
    Levenberg-Marquardt on all 2n residuals -- or, with X0 (T, 3), the
    refinement alone from X0.  refine="only" is the latter and an error
    without X0.  Returns (X (T, 3), cost (T,) sum of squared residuals at X,
    front (T,) bool: X in front of every camera of the track, info (T,) int32:
    >= 1 stop code, 0 not refined, -1 start kept, -2 fewer than two views).
    The arguments are checked before a device is looked for, and T = 0
    returns empty arrays without one."""
    P = _f64(P).reshape(-1, 12)
    ts = np.ascontiguousarray(track_start, dtype=np.int64).reshape(-1)
    cam = np.ascontiguousarray(obs_cam, dtype=np.int32).reshape(-1)
    xy = _f64(obs_xy).reshape(-1, 2)
    if len(ts) < 1 or len(xy) != len(cam):
        raise ValueError("triangulate_tracks: track_start needs T + 1 entries and obs_cam, obs_xy one row per "
                         "observation")
    T = len(ts) - 1
    if X0 is not None:
        X0 = _f64(X0).reshape(-1, 3)
        if len(X0) != T:
            raise ValueError("triangulate_tracks: X0 must be (T, 3)")
    if refine is False:
        mode = TRACKS_LINEAR
    elif refine is True:
        mode = TRACKS_BOTH if X0 is None else TRACKS_REFINE
    elif refine == "only":
        mode = TRACKS_REFINE
    else:
        raise ValueError('triangulate_tracks: refine is True, False or "only"')
    bad = int(max_nfev) <= 0 or (mode == TRACKS_REFINE and X0 is None) or not _csr_ok(ts, cam, len(P))
    if T and not bad:
        require_device()
    X, cost = np.zeros((T, 3)), np.zeros(T)
    front, info = np.zeros(T, dtype=np.uint8), np.zeros(T, dtype=np.int32)
    _check(_lib.sfm_triangulate_tracks(_p(P), len(P), _p(ts, _i64), T, _p(cam, _i32), _p(xy), len(cam),
                                       _p(X0) if X0 is not None else None, mode, int(max_nfev), _p(X), _p(cost),
                                       _p(front, _u8), _p(info, _i32), DEVICE))
    return X, cost, front.astype(bool), info


def triangulate_tracks_robust(P, track_start, obs_cam, obs_xy, threshold=4.0, max_pairs=120, min_inliers=2,
                              max_nfev=50, centres=None, lanes_per_track=0):
    """Robust triangulate_tracks (sfm_triangulate_tracks_robust): per track,
    view-pair hypotheses (widest index gap first, at most max_pairs) scored by
    their inliers within ``threshold`` pixels, the winner's inliers refitted
    as triangulate_tracks fits them alone, and the mask recomputed against the
    refitted point.  P, track_start, obs_cam, obs_xy as triangulate_tracks;
    centres (n_cams, 3) are the camera centres, needed for ``angle`` only.
    Returns (X (T, 3), cost (T,) sum of the final inliers' squared errors,
    n_inliers (T,) int32, inlier (n_obs,) bool, best_pair (T,) int32 the
    winner's place in the enumeration or -1, best_count (T,) int32, info (T,)
    int32: >= 1 stop code, -1 start kept, -2 fewer than two views, -3 no
    hypothesis with min_inliers, angle (T,) the largest angle in radians
    between the final inliers' rays, or None without centres).
    lanes_per_track forces the kernel's lanes per track (0: chosen from the
    tracks); the results do not depend on it.  The arguments are checked
    before a device is looked for, and T = 0 returns empty arrays without one."""
    P = _f64(P).reshape(-1, 12)
    ts = np.ascontiguousarray(track_start, dtype=np.int64).reshape(-1)
    cam = np.ascontiguousarray(obs_cam, dtype=np.int32).reshape(-1)
    xy = _f64(obs_xy).reshape(-1, 2)
    if len(ts) < 1 or len(xy) != len(cam):
        raise ValueError("triangulate_tracks_robust: track_start needs T + 1 entries and obs_cam, obs_xy one row "
                         "per observation")
    T = len(ts) - 1
    if centres is not None:
        centres = _f64(centres).reshape(-1, 3)
        if len(centres) != len(P):
            raise ValueError("triangulate_tracks_robust: centres must be (n_cams, 3)")
    threshold, lanes = float(threshold), int(lanes_per_track)
    bad = (not (np.isfinite(threshold) and threshold > 0) or int(max_pairs) < 1 or int(min_inliers) < 2
           or int(max_nfev) <= 0 or lanes < 0 or lanes > 64 or lanes & (lanes - 1) or not _csr_ok(ts, cam, len(P)))
    if T and not bad:
        require_device()
    X, cost = np.zeros((T, 3)), np.zeros(T)
    n_inl, pair, count, info = (np.zeros(T, dtype=np.int32) for _ in range(4))
    inlier = np.zeros(len(cam), dtype=np.uint8)
    angle = np.zeros(T) if centres is not None else None
    _check(_lib.sfm_triangulate_tracks_robust(
        _p(P), len(P), _p(centres) if centres is not None else None, _p(ts, _i64), T, _p(cam, _i32), _p(xy), len(cam),
        threshold, int(max_pairs), int(min_inliers), int(max_nfev), lanes, _p(X), _p(cost), _p(n_inl, _i32),
        _p(inlier, _u8), _p(pair, _i32), _p(count, _i32), _p(info, _i32), _p(angle) if angle is not None else None,
        DEVICE))
    return X, cost, n_inl, inlier.astype(bool), pair, count, info, angle


def track_pairs(n, max_pairs=120):
    """The hypotheses of a track of n views in the kernel's order: pairs
    (i, j), i < j, by decreasing index gap and for each gap i ascending, the
    first max_pairs of them; (m, 2) int64."""
    out = [(i, i + g) for g in range(n - 1, 0, -1) for i in range(n - g)]
    return np.array(out[:max_pairs], dtype=np.int64).reshape(-1, 2)


def register_samples(counts, H, seed):
    """The 6-point sample table of register_views for views of ``counts``
    correspondences: (V, H, 6) int32, each entry a position inside its view,
    the six of a hypothesis distinct.  View v draws from child v of
    numpy.random.default_rng(seed) -- integers(0, n_v, (H, 6)), the rows that
    hold a duplicate redrawn until none do -- so its table does not depend on
    the other views; a view of n_v < 6 gets zeros."""
    return _sample_tables(counts, H, seed, 6, "register_samples")


def p3p_samples(counts, H, seed):
    """The 3-point sample table of register_views_p3p: (V, H, 3) int32, drawn
    as register_samples draws (_sample_tables); a view of n_v < 3 gets zeros."""
    return _sample_tables(counts, H, seed, 3, "p3p_samples")


def _sample_tables(counts, H, seed, k, who):
    """(len(counts), H, k) int32: row v from child v of the seed, k distinct
    positions in [0, counts[v]) per hypothesis, zeros where counts[v] < k"""
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    H = int(H)
    if H < 1:
        raise ValueError(f"{who}: H must be at least 1")
    out = np.zeros((len(counts), H, k), dtype=np.int32)
    root = np.random.SeedSequence(seed)
    for v, n in enumerate(counts):
        if n < k:
            continue
        # child v of the seed, whatever the number of views
        rng = np.random.default_rng(np.random.SeedSequence(root.entropy, spawn_key=(v,)))
        t = rng.integers(0, n, (H, k))
        while True:
            s = np.sort(t, axis=1)
            dup = np.where((s[:, 1:] == s[:, :-1]).any(axis=1))[0]
            if not len(dup):
                break
            t[dup] = rng.integers(0, n, (len(dup), k))
        out[v] = t
    return out


def _rows_rejected(bad, start, n_items, samples=None, min_n=0, live_n=None):
    """Whether the C call of a hypothesis-batch entry point will reject its
    arguments: ``bad`` (what the caller found already), CSR row starts that do
    not run from 0 to ``n_items``, or ``samples`` (rows, H, k) that leave [0, n)
    or repeat an entry in a row of at least ``min_n`` items.  Where it will not
    and some row has ``live_n`` (default ``min_n``) items: require_device()."""
    if bad or start[0] != 0 or bool(np.any(np.diff(start) < 0)) or start[-1] != n_items:
        return True
    n = np.diff(start)
    rows = n >= min_n
    if samples is not None and rows.any():
        s = samples[rows]
        srt = np.sort(s, axis=2)
        if ((s.min(axis=(1, 2)) < 0).any() or (s.max(axis=(1, 2)) >= n[rows]).any()
                or (srt[:, :, 1:] == srt[:, :, :-1]).any()):
            return True
    if (n >= (min_n if live_n is None else live_n)).any():
        require_device()
    return False


def pair_samples(counts, H, seed):
    """The 8-point sample table of verify_pairs for pairs of ``counts``
    correspondences: (P, H, 8) int32, drawn as register_samples draws
    (_sample_tables); a pair of n_p < 8 gets zeros."""
    return _sample_tables(counts, H, seed, 8, "pair_samples")


def verify_pairs(pair_start, x1, x2, samples, threshold=2.5, min_inliers=8, refit_rounds=3, want_counts=False,
                 want_models=False):
    """Batched pair verification (sfm_verify_pairs): for every image pair,
    8-point F-RANSAC over the host-drawn ``samples`` (P, H, 8; pair_samples)
    under x2^T F x1 = 0 with the Sampson distance as the inlier rule, the
    winner refitted to its consensus set by normalised least squares in up to
    ``refit_rounds`` rounds, and the inlier mask of the pair's correspondences.
    The pairs are CSR rows: pair p owns x1 / x2[pair_start[p]:pair_start[p + 1]],
    pixel coordinates in its first and second image.
    Returns (F (P, 3, 3) of unit Frobenius norm, cost (P,) sum of the final
    inliers' squared Sampson distances, n_inliers (P,) int32, inlier (n_corr,)
    bool, best_hyp (P,) int32, best_count (P,) int32, info (P,) int32: 1 the
    refit ended on an unchanged mask, 2 on a worse state or out of rounds, 0 no
    refit asked for, -1 fewer than eight correspondences, -2 no finite
    hypothesis, -3 best_count < min_inliers), then counts (P, H) int32 with
    want_counts and models (P, H, 3, 3) with want_models.  The arguments are
    checked before a device is looked for; P = 0, or no pair of eight
    correspondences, returns without one."""
    ps = np.ascontiguousarray(pair_start, dtype=np.int64).reshape(-1)
    x1 = _f64(x1).reshape(-1, 2)
    x2 = _f64(x2).reshape(-1, 2)
    samples = np.ascontiguousarray(samples, dtype=np.int32)
    if len(ps) < 1 or len(x1) != len(x2):
        raise ValueError("verify_pairs: pair_start needs P + 1 entries and x1, x2 one row per correspondence")
    P = len(ps) - 1
    if samples.ndim != 3 or samples.shape[0] != P or samples.shape[2] != 8 or samples.shape[1] < 1:
        raise ValueError("verify_pairs: samples must be (P, H, 8) with H >= 1")
    H = samples.shape[1]
    threshold = float(threshold)
    _rows_rejected(not (np.isfinite(threshold) and threshold > 0) or int(min_inliers) < 8 or int(refit_rounds) < 0,
                   ps, len(x1), samples, 8)
    F, cost = np.zeros((P, 9)), np.zeros(P)
    n_inl, hyp, count, info = (np.zeros(P, dtype=np.int32) for _ in range(4))
    inlier = np.zeros(len(x1), dtype=np.uint8)
    counts = np.zeros((P, H), dtype=np.int32) if want_counts else None
    models = np.zeros((P, H, 9)) if want_models else None
    _check(_lib.sfm_verify_pairs(
        _p(ps, _i64), P, _p(x1), _p(x2), len(x1), _p(samples, _i32), H, threshold, int(min_inliers),
        int(refit_rounds), _p(F), _p(cost), _p(n_inl, _i32), _p(hyp, _i32), _p(count, _i32), _p(info, _i32),
        _p(inlier, _u8), _p(counts, _i32) if want_counts else None, _p(models) if want_models else None, DEVICE))
    out = (F.reshape(P, 3, 3), cost, n_inl, inlier.astype(bool), hyp, count, info)
    if want_counts:
        out += (counts,)
    if want_models:
        out += (models.reshape(P, H, 3, 3),)
    return out


def essential_samples(counts, H, seed):
    """The 5-point sample table of essential_pairs for pairs of ``counts``
    correspondences: (P, H, 5) int32, drawn as register_samples draws
    (_sample_tables); a pair of n_p < 5 gets zeros."""
    return _sample_tables(counts, H, seed, 5, "essential_samples")


def essential_pairs(K, pair_start, x1, x2, samples, threshold=2.5, min_inliers=5, refit_rounds=3, max_nfev=50,
                    want_counts=False, want_models=False):
    """Batched calibrated pair verification (sfm_essential_pairs): for every
    image pair, 5-point essential-matrix RANSAC over the host-drawn ``samples``
    (P, H, 5; essential_samples) -- up to ten solutions per hypothesis, each
    scored in pixels by the Sampson distance of F = K^-T E K^-1 --, the winner
    (most inliers, then the smaller cost, then the earliest hypothesis)
    refitted as E = [t]x R by Levenberg-Marquardt over its consensus set in up
    to ``refit_rounds`` rounds, and the inlier mask of the pair's
    correspondences.  The pairs are CSR rows as for verify_pairs.
    Returns (F (P, 3, 3) and, at position 7, E (P, 3, 3), both of unit
    Frobenius norm, cost (P,) sum of the final inliers' squared Sampson
    distances, n_inliers (P,) int32, inlier (n_corr,) bool, best_hyp (P,) int32,
    best_count (P,) int32, info (P,) int32: 1..5 the last refit's stop code, 0
    no refit asked for, -1 fewer than five correspondences, -2 no finite
    solution, -3 best_count < min_inliers, -4 refit could not start, E), then
    n_sol (P, H) int32 and counts (P, H, 10) int32 with want_counts and models
    (P, H, 10, 3, 3) with want_models: positions 0-6 are verify_pairs' tuple.
    The arguments are checked before a device is looked for; P = 0, or no pair
    of five correspondences, returns without one."""
    K = _f64(K)
    ps = np.ascontiguousarray(pair_start, dtype=np.int64).reshape(-1)
    x1 = _f64(x1).reshape(-1, 2)
    x2 = _f64(x2).reshape(-1, 2)
    samples = np.ascontiguousarray(samples, dtype=np.int32)
    if K.size != 9:
        raise ValueError("essential_pairs: K must be 3 x 3")
    if len(ps) < 1 or len(x1) != len(x2):
        raise ValueError("essential_pairs: pair_start needs P + 1 entries and x1, x2 one row per correspondence")
    P = len(ps) - 1
    if samples.ndim != 3 or samples.shape[0] != P or samples.shape[2] != 5 or samples.shape[1] < 1:
        raise ValueError("essential_pairs: samples must be (P, H, 5) with H >= 1")
    H = samples.shape[1]
    threshold = float(threshold)
    with np.errstate(all="ignore"):
        bad = (not (np.isfinite(threshold) and threshold > 0) or int(min_inliers) < 5 or int(refit_rounds) < 0
               or int(max_nfev) <= 0 or not np.all(np.isfinite(K)) or not np.linalg.det(K.reshape(3, 3)) != 0)
    _rows_rejected(bad, ps, len(x1), samples, 5)
    E, F, cost = np.zeros((P, 9)), np.zeros((P, 9)), np.zeros(P)
    n_inl, hyp, count, info = (np.zeros(P, dtype=np.int32) for _ in range(4))
    inlier = np.zeros(len(x1), dtype=np.uint8)
    n_sol = np.zeros((P, H), dtype=np.int32) if want_counts else None
    counts = np.zeros((P, H, 10), dtype=np.int32) if want_counts else None
    models = np.zeros((P, H, 10, 9)) if want_models else None
    _check(_lib.sfm_essential_pairs(
        _p(K), _p(ps, _i64), P, _p(x1), _p(x2), len(x1), _p(samples, _i32), H, threshold, int(min_inliers),
        int(refit_rounds), int(max_nfev), _p(E), _p(F), _p(cost), _p(n_inl, _i32), _p(hyp, _i32), _p(count, _i32),
        _p(info, _i32), _p(inlier, _u8), _p(n_sol, _i32) if want_counts else None,
        _p(counts, _i32) if want_counts else None, _p(models) if want_models else None, DEVICE))
    out = (F.reshape(P, 3, 3), cost, n_inl, inlier.astype(bool), hyp, count, info, E.reshape(P, 3, 3))
    if want_counts:
        out += (n_sol, counts)
    if want_models:
        out += (models.reshape(P, H, 10, 3, 3),)
    return out


def homography_samples(counts, H, seed):
    """The 4-point sample table of init_pairs for pairs of ``counts``
    correspondences: (P, H, 4) int32, drawn as register_samples draws
    (_sample_tables); a pair of n_p < 4 gets zeros."""
    return _sample_tables(counts, H, seed, 4, "homography_samples")


def init_pairs(K, pair_start, x1, x2, F, hsamples=None, h_threshold=4.0, max_reproj=4.0, want_cands=False,
               want_hcounts=False, want_hmodels=False):
    """Batched initial-pair selection (sfm_init_pairs): for every pair, the
    four pose candidates of E = K^T F K, their cheirality counts over the
    pair's correspondences, the winner's pose and points with their parallax
    angles and, with ``hsamples`` (P, Hh, 4; homography_samples), the inlier
    count of the best 4-point homography.  The pairs are CSR rows: pair p owns
    x1 / x2[pair_start[p]:pair_start[p + 1]], every row is used (pass the
    verified inliers); F (P, 3, 3) under x2^T F x1 = 0, as verify_pairs
    returns it.
    Returns (R (P, 3, 3), C (P, 3), counts (P, 4) int64, best (P,) int32, n_good
    (P,) int32, median_angle (P,) the lower median of the good angles in
    radians, h_count (P,) int32, h_best (P,) int32 (-1 without one), Hbest (P,
    3, 3), info (P,) int32: 0 done, -1 fewer than eight correspondences, -2 F or
    E not finite or of rank below 2; X (n_corr, 3), good (n_corr,) bool, angle
    (n_corr,)), then cands (P, 4, 12: R row-major, then t) with want_cands,
    hcounts (P, Hh) int32 with want_hcounts and hmodels (P, Hh, 3, 3) with
    want_hmodels.  The arguments are checked before a device is looked for;
    P = 0, or no pair of eight correspondences, returns without one."""
    K = _f64(K)
    ps = np.ascontiguousarray(pair_start, dtype=np.int64).reshape(-1)
    x1 = _f64(x1).reshape(-1, 2)
    x2 = _f64(x2).reshape(-1, 2)
    F = _f64(F)
    if K.size != 9:
        raise ValueError("init_pairs: K must be 3 x 3")
    if len(ps) < 1 or len(x1) != len(x2):
        raise ValueError("init_pairs: pair_start needs P + 1 entries and x1, x2 one row per correspondence")
    P = len(ps) - 1
    if F.size != 9 * P:
        raise ValueError("init_pairs: F must be (P, 3, 3)")
    F = F.reshape(P, 9)
    Hh = 0
    if hsamples is not None:
        hsamples = np.ascontiguousarray(hsamples, dtype=np.int32)
        if hsamples.ndim != 3 or hsamples.shape[0] != P or hsamples.shape[2] != 4:
            raise ValueError("init_pairs: hsamples must be (P, Hh, 4)")
        Hh = hsamples.shape[1]
        if Hh == 0:
            hsamples = None
    h_threshold, max_reproj = float(h_threshold), float(max_reproj)
    bad = (not (np.isfinite(h_threshold) and h_threshold > 0) or not (np.isfinite(max_reproj) and max_reproj > 0)
           or Hh > 1 << 20)
    # a pair of four is sampled, a pair of eight is live
    _rows_rejected(bad, ps, len(x1), hsamples if Hh else None, 4, live_n=8)
    R, C, med, Hbest = np.zeros((P, 9)), np.zeros((P, 3)), np.zeros(P), np.zeros((P, 9))
    counts = np.zeros((P, 4), dtype=np.int64)
    best, n_good, h_count, h_best, info = (np.zeros(P, dtype=np.int32) for _ in range(5))
    X, good, angle = np.zeros((len(x1), 3)), np.zeros(len(x1), dtype=np.uint8), np.zeros(len(x1))
    cands = np.zeros((P, 4, 12)) if want_cands else None
    hcounts = np.zeros((P, Hh), dtype=np.int32) if want_hcounts else None
    hmodels = np.zeros((P, Hh, 9)) if want_hmodels else None
    _check(_lib.sfm_init_pairs(
        _p(K), _p(ps, _i64), P, _p(x1), _p(x2), len(x1), _p(F), _p(hsamples, _i32) if Hh else None, Hh, h_threshold,
        max_reproj, _p(R), _p(C), _p(counts, _i64), _p(best, _i32), _p(n_good, _i32), _p(med), _p(h_count, _i32),
        _p(h_best, _i32), _p(Hbest), _p(info, _i32), _p(X), _p(good, _u8), _p(angle),
        _p(cands) if want_cands else None, _p(hcounts, _i32) if want_hcounts else None,
        _p(hmodels) if want_hmodels else None, DEVICE))
    out = (R.reshape(P, 3, 3), C, counts, best, n_good, med, h_count, h_best, Hbest.reshape(P, 3, 3), info, X,
           good.astype(bool), angle)
    if want_cands:
        out += (cands,)
    if want_hcounts:
        out += (hcounts,)
    if want_hmodels:
        out += (hmodels.reshape(P, Hh, 3, 3),)
    return out


def average_rotations(n_images, pair_ij, R_rel, weight=None, seed=0, threshold=np.deg2rad(5), consensus_sweeps=3,
                      max_sweeps=200, tol=1e-9, refit="jacobi", rounds=10, cg_tol=1e-10, cg_max_iters=500):
    """Global rotation averaging (sfm_average_rotations): the rotation of every
    one of ``n_images`` cameras from the relative rotations of the pairs, in one
    device call.  ``pair_ij`` (E, 2): i != j, duplicates and both orientations
    allowed; ``R_rel`` (E, 3, 3) under R_j ~ R_rel R_i with x_cam = R (X - C),
    init_pairs' out[0][b] for pair_ij[b] = (i, j); ``weight`` (E,) finite and
    > 0, or None for 1.  One spanning tree per component from its node of
    highest degree (edge priorities from ``seed``), ``consensus_sweeps`` sweeps
    in which every node takes the prediction that most of its other predictions
    agree with to within ``threshold`` radians, then up to ``max_sweeps``
    weighted refit sweeps over the agreeing entries, ended by the first whose
    largest update is <= ``tol`` radians (tol = 0: exactly max_sweeps).
    Returns (R (N, 3, 3), edge_angle (E,) radians, edge_inlier (E,) bool,
    n_inlier_edges (N,) int32, group (N,) int32 the component of the inlier
    graph labelled by its lowest node, info (N,) int32: 1 root, 0 has an inlier
    edge, -1 none; level (N,) int32, sweeps int).  Gauge: the root of every
    component of the input graph is I; rotations are mutually consistent inside
    a group, and a group cut off from its root keeps an arbitrary offset, so use
    one group.  The arguments are checked before a device is looked for
    (SfmCoreError on a violation, with no output of the C call written);
    n_images = 0 or no edge returns without one.  The threshold and the sweep
    counts are policy defaults to override, not measured quantities.
    ``refit="cg"`` (sfm_average_rotations_cg) replaces the refit sweeps, which
    remove an error common to all cameras by about 1 / (N - 1) per sweep and so
    reach ``tol`` within ``max_sweeps`` only on about a dozen images, by up to
    ``rounds`` Gauss-Newton rounds with the same stationary point: each solves
    the linearised cost over the agreeing edges by conjugate gradients (ended
    at a relative residual of ``cg_tol`` or after ``cg_max_iters`` iterations)
    and ends the refit when its largest update is <= ``tol`` (tol = 0: exactly
    ``rounds``); ``max_sweeps`` is then not used.  Measured: ``tol`` is reached
    in 4 to 5 rounds on graphs of up to 300 images; at 10,000 images x 500,000
    pairs the default 10 rounds end at a step of 7.8e-8 (raise ``rounds``).  The tuple gains, after
    ``sweeps`` (the rounds run): cg_iters (rounds,) int32, cg_residual
    (rounds,) and step (rounds,) radians, each 0 past the rounds run.  Any
    other ``refit`` raises ValueError."""
    if refit not in ("jacobi", "cg"):
        raise ValueError("average_rotations: refit must be 'jacobi' or 'cg'")
    N = int(n_images)
    ij = np.ascontiguousarray(pair_ij, dtype=np.int32).reshape(-1, 2)
    E = len(ij)
    Rr = _f64(R_rel)
    if Rr.size != 9 * E:
        raise ValueError("average_rotations: R_rel must be (E, 3, 3)")
    Rr = Rr.reshape(E, 9)
    w = None
    if weight is not None:
        w = _f64(weight).reshape(-1)
        if len(w) != E:
            raise ValueError("average_rotations: weight must be (E,)")
    threshold, tol = float(threshold), float(tol)
    consensus_sweeps, max_sweeps = int(consensus_sweeps), int(max_sweeps)
    cg = refit == "cg"
    rounds, cg_tol, cg_max_iters = int(rounds), float(cg_tol), int(cg_max_iters)
    bad = (N < 0 or E > 1 << 30 or not (np.isfinite(threshold) and 0 < threshold < np.pi) or consensus_sweeps < 0
           or (max_sweeps < 0 and not cg) or not tol >= 0
           or (cg and (rounds < 0 or not (np.isfinite(cg_tol) and cg_tol >= 0) or cg_max_iters < 1))
           or bool(E and (ij.min() < 0 or ij.max() >= N or (ij[:, 0] == ij[:, 1]).any()))
           or not bool(np.isfinite(Rr).all()) or (w is not None and not bool((np.isfinite(w) & (w > 0)).all())))
    if not bad and N and E:
        require_device()
    n = max(N, 0)
    R, angle, inlier = np.zeros((n, 9)), np.zeros(E), np.zeros(E, dtype=np.uint8)
    n_inl, group, info, level = (np.zeros(n, dtype=np.int32) for _ in range(4))
    sweeps = np.zeros(1, dtype=np.int32)
    if cg:
        nr = max(rounds, 0)
        iters, resid, step = np.zeros(nr, dtype=np.int32), np.zeros(nr), np.zeros(nr)
        _check(_lib.sfm_average_rotations_cg(N, _p(ij, _i32), _p(Rr), _p(w) if w is not None else None, E,
                                             int(seed) & (2 ** 64 - 1), threshold, consensus_sweeps, rounds, tol,
                                             cg_tol, cg_max_iters, _p(R), _p(angle), _p(inlier, _u8), _p(n_inl, _i32),
                                             _p(group, _i32), _p(info, _i32), _p(level, _i32), _p(sweeps, _i32),
                                             _p(iters, _i32), _p(resid), _p(step), DEVICE))
        return (R.reshape(n, 3, 3), angle, inlier.astype(bool), n_inl, group, info, level, int(sweeps[0]), iters,
                resid, step)
    _check(_lib.sfm_average_rotations(N, _p(ij, _i32), _p(Rr), _p(w) if w is not None else None, E,
                                      int(seed) & (2 ** 64 - 1), threshold, consensus_sweeps, max_sweeps, tol, _p(R),
                                      _p(angle), _p(inlier, _u8), _p(n_inl, _i32), _p(group, _i32), _p(info, _i32),
                                      _p(level, _i32), _p(sweeps, _i32), DEVICE))
    return R.reshape(n, 3, 3), angle, inlier.astype(bool), n_inl, group, info, level, int(sweeps[0])


POSITIONS_PATH1_MAX_NODES = 512  # SFM_POSITIONS_PATH1_MAX_NODES


def average_positions(n_images, pair_ij, dir, weight=None, mu=0.01, sigma=np.deg2rad(3), threshold=np.deg2rad(5),
                      rounds=12, cg_tol=1e-12, cg_max_iters=2000, path=0):
    """Global position averaging (sfm_average_positions): the centre of every
    one of ``n_images`` cameras from the directions between the cameras of the
    pairs, in one device call.  ``pair_ij`` (E, 2): i != j, duplicates and both
    orientations allowed; ``dir`` (E, 3): the direction from C_i towards C_j in
    world coordinates, finite and not zero (normalised by the call); ``weight``
    (E,) finite and > 0, or None for 1.  Nodes with fewer than two distinct
    neighbours are pruned repeatedly and the largest component of the rest is
    solved.  ``rounds`` rounds, each a conjugate-gradient solve (preconditioned
    by the 3 x 3 diagonal blocks, ended at a relative residual of ``cg_tol`` or
    after ``cg_max_iters`` iterations) of the chordal cost with the term
    ``mu`` (d.v - s)^2 that pins the lengths, a division by the weighted mean
    baseline, and new weights weight / ((1 + (theta / ``sigma``)^2) |v|^2).
    ``path``: 1 the single-workgroup kernel (at most POSITIONS_PATH1_MAX_NODES
    solved nodes), 2 the multi-launch one, 0 whichever fits.
    Returns (C (N, 3), edge_angle (E,) radians, edge_inlier (E,) bool: angle <=
    ``threshold``, edge_length (E,) = d.(C_j - C_i), info (N,) int32: 1 root, 0
    solved, -1 not solved; cg_iters (rounds,) int32, cg_residual (rounds,),
    n_solved int, path_used int).  C and the edge outputs are 0 for what was not
    solved.  Gauge: the root at 0, the weighted mean of d.(C_j - C_i) equal to 1;
    the scale is arbitrary.  A solve that ends at cg_max_iters is reported in
    cg_iters, not raised: a graph that is not rigid shows there.  The arguments
    are checked before a device is looked for (SfmCoreError on a violation, with
    no output of the C call written); nothing to solve returns without one.
    The parameters are policy defaults to override, not measured optima."""
    N = int(n_images)
    ij = np.ascontiguousarray(pair_ij, dtype=np.int32).reshape(-1, 2)
    E = len(ij)
    d = _f64(dir)
    if d.size != 3 * E:
        raise ValueError("average_positions: dir must be (E, 3)")
    d = d.reshape(E, 3)
    w = None
    if weight is not None:
        w = _f64(weight).reshape(-1)
        if len(w) != E:
            raise ValueError("average_positions: weight must be (E,)")
    mu, sigma, threshold, cg_tol = float(mu), float(sigma), float(threshold), float(cg_tol)
    rounds, cg_max_iters, path = int(rounds), int(cg_max_iters), int(path)
    n, nr = max(N, 0), max(rounds, 0)
    C, angle, inlier, length = np.zeros((n, 3)), np.zeros(E), np.zeros(E, dtype=np.uint8), np.zeros(E)
    info, iters, resid = np.zeros(n, dtype=np.int32), np.zeros(nr, dtype=np.int32), np.zeros(nr)
    n_solved, path_used = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)

    # the library checks the arguments and prunes the graph before it looks for a device: only a call that passes
    # both and has something to solve needs one, and fails loudly without it (no CPU fallback)
    _check(_lib.sfm_average_positions(N, _p(ij, _i32), _p(d), _p(w) if w is not None else None, E, mu, sigma,
                                      threshold, rounds, cg_tol, cg_max_iters, path, _p(C), _p(angle), _p(inlier, _u8),
                                      _p(length), _p(info, _i32), _p(iters, _i32), _p(resid), _p(n_solved, _i32),
                                      _p(path_used, _i32), DEVICE))
    return (C, angle, inlier.astype(bool), length, info, iters, resid, int(n_solved[0]), int(path_used[0]))


MERGE_DROP, MERGE_KEEP_ROWS = 0, 1


def merge_tracks(row_start, image, x, y, n_images, policy=MERGE_DROP):
    """Track merging (sfm_merge_tracks): the rows of a feature-major store that
    share a keypoint joined into tracks on the device.  Row r owns image / x /
    y[row_start[r]:row_start[r + 1]].  An observation's keypoint is the
    smallest observation index with its image and coordinates, a row's
    component the smallest row index reachable through shared keypoints; a
    component with two different keypoints of one image is conflicting, and its
    rows get the label -1 (MERGE_DROP) or their own index (MERGE_KEEP_ROWS).
    Returns a dict: keypoint (n_obs,) int32, component (n_rows,) int32,
    conflict (n_rows,) bool, label (n_rows,) int32, track_label (n_tracks,)
    int32 the distinct labels >= 0 ascending, track_start (n_tracks + 1,) int64,
    track_obs (track_start[-1],) int32 each track's distinct keypoints ordered
    by (image, keypoint), obs_slot (n_obs,) int32 the place of each
    observation's keypoint in track_obs or -1.  The arguments are checked
    before a device is looked for (SfmCoreError on a violation, with no output
    of the C call written); no rows, or no observations, returns without one."""
    rs = np.ascontiguousarray(row_start, dtype=np.int64).reshape(-1)
    image = np.ascontiguousarray(image, dtype=np.int32).reshape(-1)
    x, y = _f64(x).reshape(-1), _f64(y).reshape(-1)
    if len(rs) < 1 or len(x) != len(image) or len(y) != len(image):
        raise ValueError("merge_tracks: row_start needs n_rows + 1 entries and image, x, y one entry per observation")
    n_rows, n_obs, n_images, policy = len(rs) - 1, len(image), int(n_images), int(policy)
    bad = (policy not in (MERGE_DROP, MERGE_KEEP_ROWS) or n_images < 0 or rs[0] != 0 or bool(np.any(np.diff(rs) < 0))
           or rs[-1] != n_obs or bool(n_obs and (image.min() < 0 or image.max() >= n_images))
           or not bool(np.isfinite(x).all() and np.isfinite(y).all()))
    if not bad and n_rows and n_obs:
        require_device()
    keypoint, obs_slot, track_obs = (np.full(n_obs, -1, dtype=np.int32) for _ in range(3))
    component, label, track_label = (np.full(n_rows, -1, dtype=np.int32) for _ in range(3))
    conflict = np.zeros(n_rows, dtype=np.uint8)
    track_start = np.zeros(n_rows + 1, dtype=np.int64)
    n_tracks = np.zeros(1, dtype=np.int64)
    _check(_lib.sfm_merge_tracks(_p(rs, _i64), n_rows, _p(image, _i32), _p(x), _p(y), n_obs, n_images, policy,
                                 _p(keypoint, _i32), _p(component, _i32), _p(conflict, _u8), _p(label, _i32),
                                 _p(n_tracks, _i64), _p(track_label, _i32), _p(track_start, _i64),
                                 _p(track_obs, _i32), _p(obs_slot, _i32), DEVICE))
    nt = int(n_tracks[0])
    track_start = track_start[:nt + 1].copy()
    return dict(keypoint=keypoint, component=component, conflict=conflict.astype(bool), label=label,
                track_label=track_label[:nt].copy(), track_start=track_start,
                track_obs=track_obs[:int(track_start[-1])].copy(), obs_slot=obs_slot)


INT32_MAX = 2 ** 31 - 1


def match_descriptors(desc, img_start, pairs, ratio=0.8, max_dsq=INT32_MAX, cross_check=True, capacity=None,
                      want_diagnostics=False):
    """Descriptor matching (sfm_match_descriptors): for every image pair (i, j)
    of ``pairs`` (P, 2) the matches of image i's keypoints in image j, on the
    device.  desc (n_kp, dim) uint8 with dim 64, 128 or 256; image k owns rows
    img_start[k]:img_start[k + 1].  dsq is the exact integer squared distance;
    the keypoints of j are ordered by (dsq, index): nn is the first, d1 its dsq,
    d2 the second's (INT32_MAX without one; nn = -1, d1 = INT32_MAX with no
    keypoint in j).  a is matched to nn when nn >= 0, d1 <= max_dsq,
    d2 == INT32_MAX or float(d1) < (ratio * ratio) * float(d2), and, with
    cross_check, the first of i's keypoints in nn's order is a.  The ratio test
    is on the forward direction only.  ``capacity`` (default the bound: the sum
    of N_i, or of min(N_i, N_j) with cross_check) sizes the match arrays.
    Returns a dict: match_start (P + 1,) int64, a, b, dsq (match_start[-1],)
    int32 -- pair p owns [match_start[p], match_start[p + 1]), ascending a --
    and, with want_diagnostics, nn, d1, d2 (sum of N_i,) and nn_rev (sum of
    N_j,) int32, pair-major.  The arguments are checked before a device is
    looked for (SfmCoreError, nothing written); P == 0 needs no device."""
    desc, st, pairs, capacity, outs, diag = _match_arrays("match_descriptors", desc, img_start, pairs, cross_check,
                                                          capacity, want_diagnostics, "iiij")
    _check(_lib.sfm_match_descriptors(_p(desc, _u8), len(desc), _p(st, _i64), len(st) - 1, desc.shape[1],
                                      _p(pairs, _i32), len(pairs), float(ratio), int(max_dsq), int(bool(cross_check)),
                                      capacity, _p(outs[0], _i64), *(_p(o, _i32) for o in outs[1:]),
                                      *(None if d is None else _p(d, _i32) for d in diag), DEVICE))
    return _match_result(outs, diag, ("nn", "d1", "d2", "nn_rev"), want_diagnostics)


def _match_arrays(name, desc, img_start, pairs, cross_check, capacity, want_diagnostics, diag_sides):
    """The inputs of a matching call as contiguous arrays, the capacity (default
    the bound) and the caller-allocated outputs: (match_start, a, b, dsq) and one
    diagnostic per letter of ``diag_sides`` -- "i": sum of N_i entries, "j": sum
    of N_j -- or None without want_diagnostics."""
    desc = np.ascontiguousarray(desc, dtype=np.uint8)
    if desc.ndim != 2:
        raise ValueError(f"{name}: desc must be (n_kp, dim)")
    st = np.ascontiguousarray(img_start, dtype=np.int64).reshape(-1)
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    if len(st) < 1:
        raise ValueError(f"{name}: img_start needs n_images + 1 entries")
    n_images, P = len(st) - 1, len(pairs)
    n = np.diff(st)
    inside = bool(P == 0 or (pairs.min() >= 0 and pairs.max() < n_images))
    ni = n[pairs[:, 0]] if inside else np.zeros(0, dtype=np.int64)
    nj = n[pairs[:, 1]] if inside else np.zeros(0, dtype=np.int64)
    bound = int(np.minimum(ni, nj).sum() if cross_check else ni.sum())
    capacity = max(bound, 0) if capacity is None else int(capacity)
    match_start = np.zeros(P + 1, dtype=np.int64)
    a, b, dsq = (np.full(max(capacity, 0), -1, dtype=np.int32) for _ in range(3))
    diag = [None] * len(diag_sides)
    if want_diagnostics:
        diag = [np.full(max(int((ni if k == "i" else nj).sum()), 0), -1, dtype=np.int32) for k in diag_sides]
    return desc, st, pairs, capacity, (match_start, a, b, dsq), diag


def _match_result(outs, diag, names, want_diagnostics):
    match_start, a, b, dsq = outs
    m = int(match_start[-1])
    out = dict(match_start=match_start, a=a[:m].copy(), b=b[:m].copy(), dsq=dsq[:m].copy())
    if want_diagnostics:
        out.update(zip(names, diag))
    return out


def match_descriptors_guided(desc, xy, img_start, pairs, F, gate, ratio=0.8, max_dsq=INT32_MAX, cross_check=True,
                             capacity=None, want_diagnostics=False):
    """Guided descriptor matching (sfm_match_descriptors_guided):
    ``match_descriptors`` with the candidates of keypoint a of image i
    restricted to the keypoints b of j inside the band of half-width ``gate``
    pixels around a's epipolar line.  xy (n_kp, 2) are the keypoints in desc's
    row order; F (P, 3, 3), one matrix per pair with x_j^T F x_i = 0 for the
    pair (i, j) -- verify_pairs' convention; a pair listed as (j, i) takes
    F^T.  A pair of keypoints is a candidate when den > 0 and
    e^2 < (gate * gate) den, the squared Sampson distance of verify_pairs'
    inlier rule, bit for bit (include/sfmcore.h has the operation order); it is
    the same decision in the reverse pass of the cross-check.  An F with a NaN
    gives a pair without candidates and without matches.  nn, d1, d2 and nn_rev
    are taken over the candidates only (nn = -1 and d1 = INT32_MAX without one,
    d2 = INT32_MAX with fewer than two); the tests, the capacity and the layout
    are ``match_descriptors``'s.  Returns its dict; with want_diagnostics also
    n_cand (sum of N_i,) int32, the number of candidates of each keypoint.
    The arguments are checked before a device is looked for; P == 0 needs no
    device."""
    desc, st, pairs, capacity, outs, diag = _match_arrays("match_descriptors_guided", desc, img_start, pairs,
                                                          cross_check, capacity, want_diagnostics, "iiiji")
    xy = _f64(xy)
    if xy.shape != (len(desc), 2):
        raise ValueError("match_descriptors_guided: xy must be (n_kp, 2)")
    F = _f64(F)
    if F.shape != (len(pairs), 3, 3):
        raise ValueError("match_descriptors_guided: F must be (P, 3, 3)")
    _check(_lib.sfm_match_descriptors_guided(_p(desc, _u8), _p(xy), len(desc), _p(st, _i64), len(st) - 1,
                                             desc.shape[1], _p(pairs, _i32), _p(F), len(pairs), float(gate),
                                             float(ratio), int(max_dsq), int(bool(cross_check)), capacity,
                                             _p(outs[0], _i64), *(_p(o, _i32) for o in outs[1:]),
                                             *(None if d is None else _p(d, _i32) for d in diag), DEVICE))
    return _match_result(outs, diag, ("nn", "d1", "d2", "nn_rev", "n_cand"), want_diagnostics)


EXTRACT_DEFAULT_CAPACITY = 32768


def extract_octaves(H, W):
    """the octaves that keep the smaller side of an H x W image >= 16, each taking every second pixel"""
    n = 0
    while min(H, W) >= 16:
        n, H, W = n + 1, (H + 1) // 2, (W + 1) // 2
    return n


def extract_features(images, n_octaves=0, max_keypoints=0, contrast_threshold=0.04, edge_threshold=10.0, sigma=1.6,
                     capacity=None, want_diagnostics=False, cand_capacity=None):
    """Feature extraction (sfm_extract_features): difference-of-Gaussians
    keypoints with 128-byte gradient-histogram descriptors of ``images``
    (n, H, W) uint8, on the device; include/sfmcore.h has the definitions.
    n_octaves 0 means as many as keep the smaller side >= 16.  ``capacity`` is
    the rows per image of the outputs, which are allocated here as n x
    capacity rows of 172 bytes (default: max_keypoints, or without a cap
    EXTRACT_DEFAULT_CAPACITY = 32768 or the bound on an image's candidates if
    that is smaller; an image with more keypoints ends the call with an
    SfmCoreError that names the image and its count).  Returns a dict: kp_start (n + 1,) int64 -- image k owns
    rows kp_start[k]:kp_start[k + 1] -- xy (N, 2) fp64, scale, angle, response
    (N,) fp32, desc (N, 128) uint8; with want_diagnostics also kp_site (N, 4)
    int32 (octave, layer, row, col), pyramid (n, floats per image) fp32,
    cand_start (n + 1,), cand (C, 5) int32 (image, octave, layer, row, col),
    ref_ok (C,) bool, ref_site (C, 3) int32 and ref_val (C, 4) fp32 (xc, xr,
    xs, |D^|).  The arguments are checked before a device is looked for;
    no images need no device."""
    images = np.ascontiguousarray(images, dtype=np.uint8)
    if images.ndim != 3:
        raise ValueError("extract_features: images must be (n, H, W)")
    n, H, W = images.shape
    n_oct = int(n_octaves) if n_octaves else extract_octaves(H, W)
    per_image = bound = 0
    h, w = H, W
    for _ in range(max(min(n_oct, 16), 0)):
        per_image += 6 * h * w
        bound += 6 * ((h + 1) // 2) * ((w + 1) // 2)
        h, w = (h + 1) // 2, (w + 1) // 2
    if capacity is None:
        capacity = int(max_keypoints) if max_keypoints > 0 else min(bound, EXTRACT_DEFAULT_CAPACITY)
    capacity = int(capacity)
    rows = n * max(capacity, 0)
    kp_start = np.zeros(n + 1, dtype=np.int64)
    xy = np.zeros((rows, 2), dtype=np.float64)
    scale, angle, response = (np.zeros(rows, dtype=np.float32) for _ in range(3))
    desc = np.zeros((rows, 128), dtype=np.uint8)
    site = pyramid = cand_start = cand = ref_ok = ref_site = ref_val = None
    cc = 0
    if want_diagnostics:
        cc = n * bound if cand_capacity is None else int(cand_capacity)
        site = np.zeros((rows, 4), dtype=np.int32)
        pyramid = np.zeros((n, per_image), dtype=np.float32)
        cand_start = np.zeros(n + 1, dtype=np.int64)
        cand = np.zeros((cc, 5), dtype=np.int32)
        ref_ok = np.zeros(cc, dtype=np.uint8)
        ref_site = np.zeros((cc, 3), dtype=np.int32)
        ref_val = np.zeros((cc, 4), dtype=np.float32)

    def ptr(a, t):
        return None if a is None else _p(a, t)
    _check(_lib.sfm_extract_features(_p(images, _u8), n, H, W, int(n_octaves), int(max_keypoints),
                                     float(contrast_threshold), float(edge_threshold), float(sigma), capacity,
                                     _p(kp_start, _i64), _p(xy), _p(scale, _f32), _p(angle, _f32), _p(response, _f32),
                                     _p(desc, _u8), ptr(site, _i32), ptr(pyramid, _f32), cc, ptr(cand_start, _i64),
                                     ptr(cand, _i32), ptr(ref_ok, _u8), ptr(ref_site, _i32), ptr(ref_val, _f32),
                                     DEVICE))
    N = int(kp_start[-1])
    out = dict(kp_start=kp_start, xy=xy[:N].copy(), scale=scale[:N].copy(), angle=angle[:N].copy(),
               response=response[:N].copy(), desc=desc[:N].copy())
    if want_diagnostics:
        C = int(cand_start[-1])
        out.update(kp_site=site[:N].copy(), pyramid=pyramid, cand_start=cand_start, cand=cand[:C].copy(),
                   ref_ok=ref_ok[:C].astype(bool), ref_site=ref_site[:C].copy(), ref_val=ref_val[:C].copy())
    return out


def vocab_train(desc, centres, max_iterations=10):
    """Visual vocabulary (sfm_vocab_train): k-means on the uint8 descriptors
    desc (n, dim), dim 64, 128 or 256, from the initial ``centres``
    (n_words, dim) uint8, on the device; max_iterations = 0 is the quantisation
    of desc against centres.  Exact integer work (include/sfmcore.h): a
    descriptor goes to the first centre of the (dsq, index) order, a centre
    becomes the mean of its members rounded half up, an empty cluster keeps its
    centre, and the loop stops after update T when T == max_iterations or
    nothing changed.  Returns a dict: centres (n_words, dim) uint8, word (n,)
    int32, count (n_words,) int64, inertia (T + 1,) int64 and iterations = T.
    The arguments are checked before a device is looked for."""
    desc = np.ascontiguousarray(desc, dtype=np.uint8)
    centres = np.array(centres, dtype=np.uint8, order="C")  # a copy: the call writes it
    if desc.ndim != 2 or centres.ndim != 2 or centres.shape[1] != desc.shape[1]:
        raise ValueError("vocab_train: desc must be (n, dim) and centres (n_words, dim)")
    n, n_words, its = len(desc), len(centres), int(max_iterations)
    word = np.full(n, -1, dtype=np.int32)
    count = np.zeros(n_words, dtype=np.int64)
    inertia = np.zeros(max(its, 0) + 1, dtype=np.int64)
    T = np.zeros(1, dtype=np.int32)
    _check(_lib.sfm_vocab_train(_p(desc, _u8), n, desc.shape[1], n_words, its, _p(centres, _u8), _p(word, _i32),
                                _p(count, _i64), _p(inertia, _i64), _p(T, _i32), DEVICE))
    return dict(centres=centres, word=word, count=count, inertia=inertia[:int(T[0]) + 1].copy(), iterations=int(T[0]))


def select_pairs(word, img_start, n_words, top_k=20):
    """Pair selection (sfm_select_pairs): tf-idf retrieval over the words
    (n_kp,) int32 in [0, n_words) of the images' keypoints -- image k owns
    img_start[k]:img_start[k + 1] -- on the device.  With h the word counts of
    an image, df the images per word and q[d] = floor(256 log(n_images / d) +
    0.5), v = h q[df]; norm2 and dot are exact int64, score = dot /
    (sqrt(norm2_i) sqrt(norm2_j)), and the neighbours of i are the j != i with
    dot > 0 by (score descending, j ascending).  Returns a dict: neighbour
    (n_images, top_k) int32 padded with -1, score (n_images, top_k) fp64 padded
    with 0, dot (n_images, top_k) int64 padded with 0, norm2 (n_images,) int64
    and df (n_words,) int32.  The arguments are checked before a device is
    looked for; no images, or top_k == 0, need no device."""
    word = np.ascontiguousarray(word, dtype=np.int32).reshape(-1)
    st = np.ascontiguousarray(img_start, dtype=np.int64).reshape(-1)
    if len(st) < 1:
        raise ValueError("select_pairs: img_start needs n_images + 1 entries")
    n_images, k = len(st) - 1, int(top_k)
    neighbour = np.full((n_images, max(k, 0)), -1, dtype=np.int32)
    score = np.zeros((n_images, max(k, 0)), dtype=np.float64)
    dot = np.zeros((n_images, max(k, 0)), dtype=np.int64)
    norm2 = np.zeros(n_images, dtype=np.int64)
    df = np.zeros(max(int(n_words), 0), dtype=np.int32)
    _check(_lib.sfm_select_pairs(_p(word, _i32), len(word), _p(st, _i64), n_images, int(n_words), k,
                                 _p(neighbour, _i32), _p(score), _p(dot, _i64), _p(norm2, _i64), _p(df, _i32), DEVICE))
    return dict(neighbour=neighbour, score=score, dot=dot, norm2=norm2, df=df)


def _register(name, k, min_n, slots, K, X, view_start, pt_idx, xy, samples, threshold, min_inliers, refit_rounds,
              max_nfev, want_counts, want_models):
    """register_views (k = 6, slots = 1) and register_views_p3p (k = 3, slots
    = 4): the coercions, the checks before a device is looked for, the call and
    the output tuple.  ``slots`` > 1 brings the n_sol table and a slot axis."""
    K = _f64(K).reshape(3, 3)
    X = _f64(X).reshape(-1, 3)
    vs = np.ascontiguousarray(view_start, dtype=np.int64).reshape(-1)
    pt = np.ascontiguousarray(pt_idx, dtype=np.int32).reshape(-1)
    xy = _f64(xy).reshape(-1, 2)
    samples = np.ascontiguousarray(samples, dtype=np.int32)
    if len(vs) < 1 or len(xy) != len(pt):
        raise ValueError(f"{name}: view_start needs V + 1 entries and pt_idx, xy one row per correspondence")
    V = len(vs) - 1
    if samples.ndim != 3 or samples.shape[0] != V or samples.shape[2] != k or samples.shape[1] < 1:
        raise ValueError(f"{name}: samples must be (V, H, {k}) with H >= 1")
    H = samples.shape[1]
    threshold = float(threshold)
    bad = (not (np.isfinite(threshold) and threshold > 0) or int(min_inliers) < min_n or int(refit_rounds) < 0
           or int(max_nfev) <= 0 or H > 1 << 20 or not _csr_ok(vs, pt, len(X)))
    _rows_rejected(bad, vs, len(pt), samples, min_n)
    multi = slots > 1
    per = (H, slots) if multi else (H,)
    C, R, cost = np.zeros((V, 3)), np.zeros((V, 9)), np.zeros(V)
    n_inl, hyp, count, info = (np.zeros(V, dtype=np.int32) for _ in range(4))
    inlier = np.zeros(len(pt), dtype=np.uint8)
    n_sol = np.zeros((V, H), dtype=np.int32) if want_counts and multi else None
    counts = np.zeros((V,) + per, dtype=np.int32) if want_counts else None
    models = np.zeros((V,) + per + (12,)) if want_models else None
    tables = [(n_sol, _i32)] * multi + [(counts, _i32), (models, _d)]  # the optional arrays, in the C order
    tables = [None if a is None else _p(a, t) for a, t in tables]
    _check(getattr(_lib, "sfm_" + name)(
        _p(K), _p(X), len(X), _p(vs, _i64), V, _p(pt, _i32), _p(xy), len(pt), _p(samples, _i32), H, threshold,
        int(min_inliers), int(refit_rounds), int(max_nfev), _p(C), _p(R), _p(cost), _p(n_inl, _i32), _p(hyp, _i32),
        _p(count, _i32), _p(info, _i32), _p(inlier, _u8), *tables, DEVICE))
    out = (C, R.reshape(V, 3, 3), cost, n_inl, inlier.astype(bool), hyp, count, info)
    if want_counts:
        out += (n_sol, counts) if multi else (counts,)
    if want_models:
        out += (models.reshape((V,) + per + (3, 4)),)
    return out


def register_views(K, X, view_start, pt_idx, xy, samples, threshold=4.0, min_inliers=6, refit_rounds=3, max_nfev=50,
                   want_counts=False, want_models=False):
    """Batched view registration (sfm_register_views): for every view, 6-point
    PnP RANSAC over the host-drawn ``samples`` (V, H, 6; register_samples), the
    winner's pose refitted to its consensus set by Levenberg-Marquardt in up
    to ``refit_rounds`` rounds, and the inlier mask of the view's
    correspondences.  X (n_pts, 3); the views are CSR rows: view v owns
    pt_idx / xy[view_start[v]:view_start[v + 1]], pt_idx an index into X.
    Returns (C (V, 3), R (V, 3, 3), cost (V,) sum of the final inliers' squared
    errors, n_inliers (V,) int32, inlier (n_corr,) bool, best_hyp (V,) int32,
    best_count (V,) int32, info (V,) int32: 1..5 the last refit's stop code, 0
    no refit asked for, -1 fewer than six correspondences, -2 no finite
    hypothesis, -3 best_count < min_inliers, -4 refit could not start), then
    counts (V, H) int32 with want_counts and models (V, H, 3, 4) with
    want_models.  The arguments are checked before a device is looked for;
    V = 0, or no view of six correspondences, returns without one."""
    return _register("register_views", 6, 6, 1, K, X, view_start, pt_idx, xy, samples, threshold, min_inliers,
                     refit_rounds, max_nfev, want_counts, want_models)


def register_views_p3p(K, X, view_start, pt_idx, xy, samples, threshold=4.0, min_inliers=4, refit_rounds=3,
                       max_nfev=50, want_counts=False, want_models=False):
    """Calibrated batched view registration (sfm_register_views_p3p): for every
    view, P3P RANSAC over the host-drawn ``samples`` (V, H, 3; p3p_samples) --
    up to four poses per sample, each scored as P = K [R | -R C] -- then
    register_views' refit from the winning pose.  Unlike register_views it
    registers views of points on one plane.  X, view_start, pt_idx, xy as
    register_views.  Returns register_views' eight outputs in the same places
    (C, R, cost, n_inliers, inlier, best_hyp, best_count, info; info -1 is
    fewer than four correspondences, -2 no solution in any hypothesis), then
    n_sol (V, H) and counts (V, H, 4) int32 with want_counts and models (V, H,
    4, 3, 4) with want_models, zero past n_sol.  The arguments are checked
    before a device is looked for; V = 0, or no view of four correspondences,
    returns without one."""
    return _register("register_views_p3p", 3, 4, 4, K, X, view_start, pt_idx, xy, samples, threshold, min_inliers,
                     refit_rounds, max_nfev, want_counts, want_models)


def reduced_solve(S, rhs):
    """Diagnostic: x = S^-1 rhs with the bundle adjuster's reduced-camera
    solver (k_assemble + tiled Cholesky + substitutions)."""
    require_device()
    S = _f64(np.asarray(S))
    rhs = _f64(np.asarray(rhs).reshape(-1))
    n = len(rhs)
    if S.shape != (n, n):
        raise ValueError("S must be n x n")
    x = np.zeros(n)
    _check(_lib.sfm_reduced_solve(_p(S), _p(rhs), n, _p(x), DEVICE))
    return x


def project(P, X):
    require_device()
    P, X = _f64(P), _f64(X)
    out = np.zeros((len(X), 2))
    _check(_lib.sfm_project_points(_p(P), _p(X), len(X), _p(out), DEVICE))
    return out


def ba_residuals(cams, pts, cam_idx, pt_idx, obs, K):
    require_device()
    cams, pts, obs, K = _f64(cams), _f64(pts), _f64(obs), _f64(K)
    ci = np.ascontiguousarray(cam_idx, dtype=np.int32)
    pi = np.ascontiguousarray(pt_idx, dtype=np.int32)
    r = np.zeros(2 * len(ci))
    _check(_lib.sfm_ba_residuals(len(cams), len(pts), len(ci), _p(ci, _i32), _p(pi, _i32), _p(obs), _p(K),
                                 _p(cams), _p(pts), _p(r), DEVICE))
    return r


def ba_opts(max_iterations=100, fixed_iterations=False, function_tolerance=1e-10, gradient_tolerance=0.0,
            parameter_tolerance=1e-12, initial_lambda=1e-4):
    return BAOpts(int(max_iterations), int(bool(fixed_iterations)), function_tolerance, gradient_tolerance,
                  parameter_tolerance, initial_lambda)


def _own(a, own):
    """a as a C-order float64 array the solve may overwrite: a itself when
    the caller hands it over (own=True and already that layout), else a copy."""
    b = _f64(a)
    return b if own and b is a else b.copy()


def ba_lm(cams, pts, cam_idx, pt_idx, obs, K, own=False, **opts):
    """Schur-complement LM on the GPU. Returns (cams, pts, report dict);
    own=True: cams / pts are the caller's to overwrite (no copies)."""
    require_device()
    cams, pts = _own(cams, own), _own(pts, own)
    obs, K = _f64(obs), _f64(K)
    ci = np.ascontiguousarray(cam_idx, dtype=np.int32)
    pi = np.ascontiguousarray(pt_idx, dtype=np.int32)
    o, rep = ba_opts(**opts), BAReport()
    _check(_lib.sfm_ba_lm(len(cams), len(pts), len(ci), _p(ci, _i32), _p(pi, _i32), _p(obs), _p(K), _p(cams),
                          _p(pts), ctypes.byref(o), ctypes.byref(rep), DEVICE))
    return cams, pts, rep.as_dict()


def ba_lm_dense(cams, pts, scan, K, own=False, **opts):
    """ba_lm with the observations of a DenseScan (sfm_ba_lm_dense): they go
    from the scan's pieces into the upload buffer, no COO arrays."""
    require_device()
    cams, pts = _own(cams, own), _own(pts, own)
    o, rep = ba_opts(**opts), BAReport()
    _check(_lib.sfm_ba_lm_dense(scan.h, len(cams), len(pts), _p(_f64(K)), _p(cams), _p(pts), ctypes.byref(o),
                                ctypes.byref(rep), DEVICE))
    return cams, pts, rep.as_dict()


def ba_lm_multi(cams, pts, cam_idx, pt_idx, obs, K, devices, **opts):
    """Single-process multi-GPU LM: points split over `devices` (repeats allowed)."""
    require_device()
    cams, pts = _f64(cams).copy(), _f64(pts).copy()
    obs, K = _f64(obs), _f64(K)
    ci = np.ascontiguousarray(cam_idx, dtype=np.int32)
    pi = np.ascontiguousarray(pt_idx, dtype=np.int32)
    dev = (ctypes.c_int * len(devices))(*devices)
    o, rep = ba_opts(**opts), BAReport()
    _check(_lib.sfm_ba_lm_multi(len(cams), len(pts), len(ci), _p(ci, _i32), _p(pi, _i32), _p(obs), _p(K), _p(cams),
                                _p(pts), ctypes.byref(o), ctypes.byref(rep), dev, len(devices)))
    return cams, pts, rep.as_dict()


class Comm:
    """RCCL communicator for the multi-GPU BA (one process per GPU)."""

    @staticmethod
    def unique_id():
        buf = ctypes.create_string_buffer(128)
        _check(_lib.sfm_comm_unique_id(buf))
        return buf.raw

    def __init__(self, uid, nranks, rank, device=None):
        require_device()
        self.h = ctypes.c_void_p()
        dev = DEVICE if device is None else device
        _check(_lib.sfm_comm_init(ctypes.c_char_p(bytes(uid)), nranks, rank, dev, ctypes.byref(self.h)))

    def close(self):
        if self.h:
            _lib.sfm_comm_destroy(self.h)
            self.h = ctypes.c_void_p()


class BAProblem:
    """Device-resident BA problem (uploaded once, iterated many times)."""

    def __init__(self, cams, pts, cam_idx, pt_idx, obs, K, comm=None, device=None):
        require_device()
        self.n_cams, self.n_pts = len(cams), len(pts)
        cams, pts, obs, K = _f64(cams), _f64(pts), _f64(obs), _f64(K)
        ci = np.ascontiguousarray(cam_idx, dtype=np.int32)
        pi = np.ascontiguousarray(pt_idx, dtype=np.int32)
        self.n_obs = len(ci)
        self.h = ctypes.c_void_p()
        dev = DEVICE if device is None else device
        _check(_lib.sfm_ba_create(self.n_cams, self.n_pts, self.n_obs, _p(ci, _i32), _p(pi, _i32), _p(obs),
                                  _p(K), _p(cams), _p(pts), dev, comm.h if comm is not None else None,
                                  ctypes.byref(self.h)))

    def solve(self, **opts):
        o, rep = ba_opts(**opts), BAReport()
        _check(_lib.sfm_ba_solve(self.h, ctypes.byref(o), ctypes.byref(rep)))
        return rep.as_dict()

    def reset(self):
        _check(_lib.sfm_ba_reset(self.h))

    def plan_digest(self):
        """Digest of the Schur sweep plan (create with SFM_PLAN_DIGEST=1; else 0)."""
        d = ctypes.c_uint64()
        _check(_lib.sfm_ba_plan_digest(self.h, ctypes.byref(d)))
        return d.value

    def spec_plan(self):
        """The speculative sweep's dispatch (sfm_ba_spec_plan): free CUs, whole
        items, split specs, sub-ranges per split item."""
        out = (ctypes.c_int32 * 4)()
        _check(_lib.sfm_ba_spec_plan(self.h, out))
        return dict(zip(("free_cus", "whole_items", "split_specs", "sub_ranges"), out))

    def download(self):
        cams = np.zeros((self.n_cams, 6))
        pts = np.zeros((self.n_pts, 3))
        _check(_lib.sfm_ba_download(self.h, _p(cams), _p(pts)))
        return cams, pts

    def set_timing(self, on=True):
        """Per-phase HIP events in the following solves (kernel_times)."""
        _check(_lib.sfm_ba_set_timing(self.h, int(bool(on))))

    def kernel_times(self):
        ms = np.zeros(16)
        names = ctypes.create_string_buffer(512)
        n = _lib.sfm_ba_kernel_times(self.h, _p(ms), 16, names, 512)
        return dict(zip(names.value.decode().split(";"), ms[:n].tolist()))

    def close(self):
        if self.h:
            _lib.sfm_ba_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
