"""
ctypes binding of libtltrace.so (C ABI in include/tl_trace.h).

There is NO fallback: if the library is missing or a call fails, a RuntimeError is raised.
The product path never computes the trace any other way.
"""
import ctypes as C
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
# TORCHOPTICS_AMD_LIB: another build of the same library (an A/B variant written by build.build_library(tag=...))
LIB_PATH = os.environ.get("TORCHOPTICS_AMD_LIB") or os.path.join(_HERE, "libtltrace.so")

TL_ABI_VERSION = 15
TL_NMOM = 10
TL_MAX_SURFACES = 32
TL_MAX_POLY = 4
TL_MAX_HIT_SLOTS = 8
TL_MAX_AIM_ITER = 16
MODE_STRICT, MODE_FAST = 0, 1
# tl_bwd_route: what tl_trace_bwd_from_outputs enqueues for a problem
ROUTE_CHECKPOINT, ROUTE_WALK_ROLLED, ROUTE_WALK_UNROLLED, ROUTE_EMPTY = 0, 1, 2, 3


class tl_problem(C.Structure):
    _fields_ = [
        ("F", C.c_int32), ("P", C.c_int32), ("W", C.c_int32), ("S", C.c_int32),
        ("device", C.c_int32), ("mode", C.c_int32), ("allow_backward", C.c_int32), ("aggregate", C.c_int32),
        ("x_in", C.c_void_p), ("y_in", C.c_void_p),
        ("xs_f", C.c_int64), ("xs_p", C.c_int64), ("xs_w", C.c_int64),
        ("ys_f", C.c_int64), ("ys_p", C.c_int64), ("ys_w", C.c_int64),
        ("z", C.c_void_p), ("cx", C.c_void_p), ("cy", C.c_void_p),
        ("cx_stride", C.c_int32), ("cy_stride", C.c_int32),
        ("c", C.c_void_p), ("t", C.c_void_p), ("mu", C.c_void_p), ("mask", C.c_void_p),
        ("kappa", C.c_void_p), ("poly", C.c_void_p), ("surf_kind", C.c_void_p), ("n_index", C.c_void_p),
        ("B", C.c_int32), ("cx_stride_b", C.c_int32), ("cy_stride_b", C.c_int32),
        ("xs_b", C.c_int64), ("ys_b", C.c_int64),
        ("asph_hits", C.c_void_p), ("asph_hit_slots", C.c_int32), ("moments_x", C.c_int32), ("cond_flags", C.c_void_p),
    ]


_VP = C.c_void_p


# the trace calls' buffers as blocks of named device pointers (tl_trace.h); member order is the header's
class tl_rays(C.Structure):
    _fields_ = [(n, _VP) for n in ("x", "y", "cx", "cy", "ok", "back", "opd", "stacks", "moments")]


class tl_seeds(C.Structure):
    _fields_ = [(n, _VP) for n in ("gx", "gy", "gcx", "gcy", "g_moments", "g_opd", "g_stacks")]


class tl_grads(C.Structure):
    _fields_ = [(n, _VP) for n in ("g_c", "g_t", "g_mu", "g_z", "g_cx", "g_cy", "g_kappa", "g_poly", "g_n_index",
                                   "g_x_in", "g_y_in")]


def _from_tensors(cls):
    def make(**tensors):
        """A block whose named members point at the given tensors (None / unnamed -> NULL).  It holds no reference:
        the caller keeps the tensors alive until the call has returned."""
        unknown = set(tensors) - {n for n, _ in cls._fields_}
        if unknown:
            raise TypeError(f"{cls.__name__} has no member {sorted(unknown)}")
        return cls(**{n: t.data_ptr() for n, t in tensors.items() if t is not None})
    return make


rays, seeds, grads = _from_tensors(tl_rays), _from_tensors(tl_seeds), _from_tensors(tl_grads)

class tl_svola_geom(C.Structure):
    _fields_ = [("device", C.c_int32), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32),
                ("psf_batch", C.c_int32), ("gh", C.c_int32), ("gw", C.c_int32), ("kh", C.c_int32), ("kw", C.c_int32),
                ("oh", C.c_int32), ("ow", C.c_int32),
                ("image_stride", C.c_int64 * 4), ("psfs_stride", C.c_int64 * 5), ("g_psfs_stride", C.c_int64 * 5)]


class tl_warp_geom(C.Structure):
    _fields_ = [("device", C.c_int32), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32),
                ("Ho", C.c_int32), ("Wo", C.c_int32), ("coord_batch", C.c_int32), ("gain_batch", C.c_int32),
                ("gain_channels", C.c_int32),
                ("image_stride", C.c_int64 * 4), ("x_stride", C.c_int64 * 3), ("y_stride", C.c_int64 * 3),
                ("gain_stride", C.c_int64 * 4), ("g_x_stride", C.c_int64 * 3), ("g_y_stride", C.c_int64 * 3),
                ("g_gain_stride", C.c_int64 * 4)]


class tl_ssim_geom(C.Structure):
    _fields_ = [("device", C.c_int32), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32),
                ("K", C.c_int32), ("window", C.c_float * 11), ("C1", C.c_float), ("C2", C.c_float), ("flags", C.c_int32),
                ("a_stride", C.c_int64 * 4), ("b_stride", C.c_int64 * 4), ("g_stride", C.c_int64 * 4)]


class tl_ms_ssim_geom(C.Structure):
    _fields_ = [("device", C.c_int32), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32),
                ("K", C.c_int32), ("window", C.c_float * 11), ("C1", C.c_float), ("C2", C.c_float), ("levels", C.c_int32),
                ("power", C.c_float * 8), ("flags", C.c_int32),
                ("a_stride", C.c_int64 * 4), ("b_stride", C.c_int64 * 4), ("g_stride", C.c_int64 * 4)]


_lock = threading.Lock()
_lib = None

_P, _R, _S, _G = C.POINTER(tl_problem), C.POINTER(tl_rays), C.POINTER(tl_seeds), C.POINTER(tl_grads)
_WS = [_VP, C.c_size_t, _VP]        # workspace, workspace_bytes, stream
_SV = C.POINTER(tl_svola_geom)
_SIGNATURES = {
    "tl_version": (C.c_int, []),
    "tl_last_error": (C.c_char_p, []),
    "tl_problem_size": (C.c_size_t, []),
    "tl_workspace_bytes": (C.c_size_t, [_P]),
    "tl_trace_fwd": (C.c_int, [_P, _R] + _WS),
    "tl_trace_bwd": (C.c_int, [_P, _S, _G] + _WS),
    "tl_trace_bwd_from_outputs": (C.c_int, [_P, _S, _R, _G] + _WS),
    "tl_bwd_route": (C.c_int, [_P]),
    "tl_spot_moments": (C.c_int, [C.c_int32] * 4 + [_VP] * 3 + [C.c_int64] * 3 + [_VP, _VP, C.c_size_t, _VP]),
    "tl_spot_rms": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_double, _VP, _VP, _VP, _VP]),
    "tl_unsup_loss": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_double, _VP, _VP, C.c_double, C.c_float, _VP, _VP, _VP, _VP, _VP]),
    "tl_unsup_loss_bwd": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _VP, _VP, _VP, _VP, C.c_int32, _VP, C.c_double, C.c_float,
                                    _VP, _VP]),
    "tl_aim_fan": (C.c_int, [C.c_int32] * 5 + [_VP] * 9),
    "tl_spot_seed": (C.c_int, [C.c_int32] * 4 + [_VP] * 3 + [C.c_int64] * 3 + [_VP] * 4),
    "tl_pupil_position": (C.c_int, [C.c_int32] * 3 + [_VP] * 8 + [C.c_int32, _VP]),
    "tl_workspace_bytes_f64": (C.c_size_t, [_P]),
    "tl_trace_fwd_f64": (C.c_int, [_P, _R] + _WS),
    "tl_trace_bwd_f64": (C.c_int, [_P, _S, _G] + _WS),
    "tl_selftest_arith": (C.c_int, [C.c_int32, C.c_int32, _VP, _VP, C.c_int64, _VP, _VP, _VP]),
    "tl_ray_aim": (C.c_int, [C.c_int32] * 5 + [_VP] * 12 + [C.c_int32] + [_VP] * 4),
    "tl_ray_aim_iter": (C.c_int, [C.c_int32] * 5 + [_VP] * 12 + [C.c_int32] * 2 + [_VP] * 6),
    "tl_psf_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32]),
    # device, G, W, R | x, y, weight, ok | s_g, s_w | x_pitch, y_pitch, y_centre | nxh, ny | x_first, y_first | ...
    "tl_psf_accumulate": (C.c_int, [C.c_int32] * 3 + [C.c_int64] + [_VP] * 4 + [C.c_int64] * 2 + [_VP] * 3 + [C.c_int32] * 2
                          + [C.c_float] * 2 + [_VP] + _WS),
    "tl_psf_accumulate_bwd": (C.c_int, [C.c_int32] * 3 + [C.c_int64] + [_VP] * 4 + [C.c_int64] * 2 + [_VP] * 3 + [C.c_int32] * 2
                              + [C.c_float] * 2 + [_VP] * 6 + _WS),
    "tl_psf_rot_workspace_bytes": (C.c_size_t, [C.c_int32] * 3 + [C.c_int64] + [C.c_int32] * 2),
    # device, G, K, W, R | x, y, weight, ok | s_g, s_w | src, c, s | x_pitch, y_pitch, y_centre | nx, ny | x_first, y_first | ...
    "tl_psf_rot_accumulate": (C.c_int, [C.c_int32] * 4 + [C.c_int64] + [_VP] * 4 + [C.c_int64] * 2 + [_VP] * 6 + [C.c_int32] * 2
                              + [C.c_float] * 2 + [_VP] + _WS),
    # ... | field_start, field_grids | g_hist | gx, gy, g_y_centre | ...
    "tl_psf_rot_accumulate_bwd": (C.c_int, [C.c_int32] * 4 + [C.c_int64] + [_VP] * 4 + [C.c_int64] * 2 + [_VP] * 6
                                  + [C.c_int32] * 2 + [C.c_float] * 2 + [_VP] * 6 + _WS),
    # geom, r0, r1, c0, c1 (host ints) | wr, wc (device doubles) | ...
    "tl_svola_workspace_bytes": (C.c_size_t, [_SV] + [_VP] * 4),
    "tl_svola_fwd": (C.c_int, [_SV] + [_VP] * 4 + [_VP] * 2 + [_VP] * 3 + [_VP]),
    "tl_svola_bwd_psf": (C.c_int, [_SV] + [_VP] * 4 + [_VP] * 2 + [_VP] * 3 + _WS),
    "tl_svola_bwd_image": (C.c_int, [_SV] + [_VP] * 4 + [_VP] * 2 + [_VP] * 3 + _WS),
    # geom | image, x, y, gain | out | stream          and          geom | image, x, y, gain | g_out | g_x, g_y, g_gain | stream
    "tl_warp_fwd": (C.c_int, [C.POINTER(tl_warp_geom)] + [_VP] * 4 + [_VP] + [_VP]),
    "tl_warp_bwd": (C.c_int, [C.POINTER(tl_warp_geom)] + [_VP] * 4 + [_VP] + [_VP] * 3 + [_VP]),
    # geom | x, y, gain | g_out | g_image | work, work_bytes | flags (bit 0: direct atomics, no LDS box) | stream
    "tl_warp_bwd_image_work_bytes": (C.c_size_t, [C.POINTER(tl_warp_geom)]),
    "tl_warp_bwd_image": (C.c_int, [C.POINTER(tl_warp_geom)] + [_VP] * 3 + [_VP] + [_VP] + [_VP, C.c_size_t] + [C.c_int] + [_VP]),
    "tl_ssim_work_bytes": (C.c_size_t, [C.POINTER(tl_ssim_geom)]),
    "tl_ssim_maps_elems": (C.c_size_t, [C.POINTER(tl_ssim_geom)]),
    # geom | a, b | value | dm_a, ds_a, dm_b, ds_b, dc | work, work_bytes | stream
    "tl_ssim_fwd": (C.c_int, [C.POINTER(tl_ssim_geom)] + [_VP] * 2 + [_VP] + [_VP] * 5 + [_VP, C.c_size_t] + [_VP]),
    # geom | p, q | dm, ds, dc | g_value | g_p | stream
    "tl_ssim_bwd": (C.c_int, [C.POINTER(tl_ssim_geom)] + [_VP] * 2 + [_VP] * 3 + [_VP] + [_VP] + [_VP]),
    "tl_ms_ssim_work_bytes": (C.c_size_t, [C.POINTER(tl_ms_ssim_geom)]),
    "tl_ms_ssim_keep_elems": (C.c_size_t, [C.POINTER(tl_ms_ssim_geom)]),
    # geom | a, b | value, terms | keep, keep_elems | work, work_bytes | stream
    "tl_ms_ssim_fwd": (C.c_int, [C.POINTER(tl_ms_ssim_geom)] + [_VP] * 2 + [_VP] * 2 + [_VP, C.c_size_t] + [_VP, C.c_size_t] + [_VP]),
    # geom | p, q | keep, keep_elems | g_value | g_p | which | work, work_bytes | stream
    "tl_ms_ssim_bwd": (C.c_int, [C.POINTER(tl_ms_ssim_geom)] + [_VP] * 2 + [_VP, C.c_size_t] + [_VP] + [_VP] + [C.c_int]
                       + [_VP, C.c_size_t] + [_VP]),
    "tl_focus_workspace_bytes": (C.c_size_t, [C.c_int64] * 3),
    # device, F, P, W | x, y, cx, cy, ok | s_f, s_p, s_w | moments | workspace, bytes | stream
    "tl_focus_moments": (C.c_int, [C.c_int32] + [C.c_int64] * 3 + [_VP] * 5 + [C.c_int64] * 3 + [_VP] + _WS),
    # ... | g_moments | gx, gy, gcx, gcy | stream
    "tl_focus_seed": (C.c_int, [C.c_int32] + [C.c_int64] * 3 + [_VP] * 5 + [C.c_int64] * 3 + [_VP] + [_VP] * 4 + [_VP]),
    "tl_enclosed_workspace_bytes": (C.c_size_t, [C.c_int64] * 3 + [C.c_int]),
    # device, F, P, W | x, y, ok | s_f, s_p, s_w | S | workspace, bytes | stream
    "tl_enclosed_centroid": (C.c_int, [C.c_int32] + [C.c_int64] * 3 + [_VP] * 3 + [C.c_int64] * 3 + [_VP] + _WS),
    # ... | centre | radii, inv_soft (host doubles), K, shape | sums | workspace, bytes | stream
    "tl_enclosed_sums": (C.c_int, [C.c_int32] + [C.c_int64] * 3 + [_VP] * 3 + [C.c_int64] * 3 + [_VP] + [_VP, _VP, C.c_int, C.c_int]
                         + [_VP] + _WS),
    # ... | centre | radii, inv_soft, K, shape | g_sums, g_lin | gx, gy, g_centre | workspace, bytes | stream
    "tl_enclosed_seed": (C.c_int, [C.c_int32] + [C.c_int64] * 3 + [_VP] * 3 + [C.c_int64] * 3 + [_VP] + [_VP, _VP, C.c_int, C.c_int]
                         + [_VP] * 2 + [_VP] * 3 + _WS),
    "tl_zfit_workspace_bytes": (C.c_size_t, [C.c_int64] * 3 + [C.c_int]),
    # device, F, P, W, order | x, y, ok | s_f, s_p, s_w | px, py | ps_f, ps_p, ps_w | moments | workspace, bytes | stream
    "tl_zfit_moments": (C.c_int, [C.c_int32] + [C.c_int64] * 3 + [C.c_int] + [_VP] * 3 + [C.c_int64] * 3 + [_VP] * 2
                        + [C.c_int64] * 3 + [_VP] + _WS),
    # device, rows, order | moments (NULL: the adjoint) | g_a, g_q | a, q, valid, factor | coef | stream
    "tl_zfit_solve": (C.c_int, [C.c_int32, C.c_int64, C.c_int] + [_VP] + [_VP] * 2 + [_VP] * 4 + [_VP] + [_VP]),
    # ... | px, py | ps_f, ps_p, ps_w | coef | gx, gy | stream
    "tl_zfit_seed": (C.c_int, [C.c_int32] + [C.c_int64] * 3 + [C.c_int] + [_VP] * 3 + [C.c_int64] * 3 + [_VP] * 2
                     + [C.c_int64] * 3 + [_VP] + [_VP] * 2 + [_VP]),
    "tl_mtf_workspace_bytes": (C.c_size_t, [C.c_int64] * 3 + [C.c_int]),
    # device, F, P, W | x, y, ok | s_f, s_p, s_w | origin | nu_x, nu_y (host doubles), J | sums | workspace, bytes | stream
    "tl_mtf_sums": (C.c_int, [C.c_int32] + [C.c_int64] * 3 + [_VP] * 3 + [C.c_int64] * 3 + [_VP] + [_VP, _VP, C.c_int] + [_VP] + _WS),
    # ... | origin | nu_x, nu_y, J | g_sums | gx, gy | workspace, bytes | stream
    "tl_mtf_seed": (C.c_int, [C.c_int32] + [C.c_int64] * 3 + [_VP] * 3 + [C.c_int64] * 3 + [_VP] + [_VP, _VP, C.c_int] + [_VP]
                    + [_VP] * 2 + _WS),
    "tl_tfmtf_workspace_bytes": (C.c_size_t, [C.c_int64] * 3 + [C.c_int] * 2),
    # device, F, P, W | x, y, cx, cy, ok | s_f, s_p, s_w | origin | nu_x, nu_y (host doubles), J | shift_first, shift_step, Z | sums
    # | workspace, bytes | stream
    "tl_tfmtf_sums": (C.c_int, [C.c_int32] + [C.c_int64] * 3 + [_VP] * 5 + [C.c_int64] * 3 + [_VP] + [_VP, _VP, C.c_int]
                      + [C.c_double, C.c_double, C.c_int] + [_VP] + _WS),
    # ... | shift_first, shift_step, Z | g_sums | gx, gy, gcx, gcy | workspace, bytes | stream
    "tl_tfmtf_seed": (C.c_int, [C.c_int32] + [C.c_int64] * 3 + [_VP] * 5 + [C.c_int64] * 3 + [_VP] + [_VP, _VP, C.c_int]
                      + [C.c_double, C.c_double, C.c_int] + [_VP] + [_VP] * 4 + _WS),
}
EXPORTS = tuple(_SIGNATURES)


def lib():
    """Load (once) and return the CDLL; raises RuntimeError when it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise RuntimeError(
                    f"{LIB_PATH} is missing: the HIP ray-trace library has not been built. "
                    "Run `python -m torchoptics_amd.build` (needs hipcc); there is no CPU fallback.")
            try:
                dll = C.CDLL(LIB_PATH)
            except OSError as e:
                raise RuntimeError(f"cannot load {LIB_PATH}: {e}") from e
            for name, (res, args) in _SIGNATURES.items():
                fn = getattr(dll, name)
                fn.restype, fn.argtypes = res, args
            got = dll.tl_version()
            if got != TL_ABI_VERSION:
                raise RuntimeError(f"libtltrace.so ABI {got} != expected {TL_ABI_VERSION}; rebuild it")
            if dll.tl_problem_size() != C.sizeof(tl_problem):
                raise RuntimeError("tl_problem layout mismatch between _lib.py and libtltrace.so; rebuild it")
            _lib = dll
    return _lib


def check(rc, what):
    if rc != 0:
        msg = lib().tl_last_error().decode(errors="replace")
        raise RuntimeError(f"{what} failed (code {rc}): {msg}")


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    return None if t is None else C.c_void_p(t.data_ptr())
