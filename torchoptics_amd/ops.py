"""
autograd.Function wrappers around the C ABI (include/tl_trace.h).

`TraceFunction` stands where PyTorch autograd's recorded graph of the reference's
`trace_skew` stood (ray_tracing_lite.py:594-675): forward = one fused HIP kernel,
backward = one recompute-and-reverse HIP kernel.  It is the one trace node of both precisions:
float64 rays select the `_f64` entry points and element type through a `_Precision` record.
`SpotMomentsFunction` is the reduction of `compute_rms2d` (ray_tracing_lite.py:678-702) for
tensors that did not come from the trace.

Every launching entry point of the C ABI is reached through `_call`: device guard, optional
timing events, tensors -> device pointers, the current stream as the last argument, the return
code checked under the entry point's own name.  Only the sizing entries (`tl_*workspace_bytes*`:
no stream, no return code) are called directly.

Per-ray buffers are allocated [B, F, W, P] (pupil index contiguous) and handed
out as [B, F, P, W] permuted views, which is the reference's logical shape.  A batch of B padded
lenses is ONE launch (tl_problem.B); B = 1 is the reference's callers' case.
"""
import ctypes as C
import os
from types import SimpleNamespace
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from ._lib import TL_NMOM, tl_problem

_MODES = {"strict": _lib.MODE_STRICT, "fast": _lib.MODE_FAST}
_default_mode = os.environ.get("TORCHOPTICS_AMD_MODE", "strict")
# backward algorithm: "checkpoint" = re-trace forwards keeping the per-surface states in registers;
# "inverse" = walk back from the forward kernel's outputs (tl_trace_bwd_from_outputs), used whenever the
# problem allows it (allow_backward_rays, no penalty term, per-ray outputs were produced)
_bwd_algo = os.environ.get("TORCHOPTICS_AMD_BWD", "inverse")


# host chain: "cpp" = the C++ autograd functions of _tlx.so (csrc/tl_torch.cpp: argument normalisation, allocation,
# the C-ABI calls and the autograd nodes in C++; the default when the extension is built), "python" = the ctypes
# wrappers below (same kernels, same numbers; ~2x the host time per step)
_host = os.environ.get("TORCHOPTICS_AMD_HOST", "cpp")
_ext_mod = None


def set_host_chain(name: str) -> None:
    global _host
    if name not in ("cpp", "python"):
        raise ValueError("host chain must be 'cpp' or 'python'")
    _host = name


def _ext():
    """The C++ host extension, or None (not built / another ABI / host chain 'python')."""
    global _ext_mod
    if _host != "cpp":
        return None
    if _ext_mod is None:
        try:
            _lib.lib()                                  # libtltrace.so first: clear error when THAT is missing
            from . import _tlx
            _ext_mod = _tlx if _tlx.abi_version() == _lib.TL_ABI_VERSION else False
        except ImportError:
            _ext_mod = False
    return _ext_mod or None


def host_chain() -> str:
    """Which host chain trace_skew / compute_rms2d use right now: 'cpp' or 'python'."""
    return "cpp" if _ext() is not None else "python"


def used_walk_back(t: torch.Tensor) -> bool:
    """Whether the backward of the trace that produced `t` (the x returned by trace_skew) will CALL
    tl_trace_bwd_from_outputs rather than tl_trace_bwd: the host chain's choice of entry point (backward algorithm
    'inverse', allow_backward_rays, no OPD gradient, no per-ray input gradients, fp32).  It does not say that a walk-back
    kernel runs: tl_trace_bwd_from_outputs hands the penalty term of some lenses to tl_trace_bwd as a whole --
    `backward_route(t)` names the kernels.  A batch traced in lens chunks reports its chunks' (common) answer; a tensor
    that no trace produced: False."""
    return bool(getattr(t, "_tl_use_inv", False))


BACKWARD_ROUTES = {_lib.ROUTE_CHECKPOINT: "checkpoint", _lib.ROUTE_WALK_ROLLED: "walk_rolled",
                   _lib.ROUTE_WALK_UNROLLED: "walk_unrolled", _lib.ROUTE_EMPTY: "empty"}


def backward_route(t: torch.Tensor) -> str:
    """Which kernels the backward of the trace that produced `t` (the x returned by trace_skew) enqueues: 'checkpoint'
    (trace_bwd_kernel for every ray: tl_trace_bwd), 'walk_rolled' (trace_bwd_inv_kernel), 'walk_unrolled'
    (trace_bwd_inv_unrolled_kernel) or 'empty' (no rays) -- tl_bwd_route of the trace's own tl_problem (include/tl_trace.h),
    the decision tl_trace_bwd_from_outputs takes on the host.  A trace whose backward calls tl_trace_bwd by the host
    chain's own choice (`used_walk_back(t)` False: 'checkpoint' algorithm, OPD gradient, per-ray input gradients, fp64)
    reports 'checkpoint'.  Either host chain; a batch traced in lens chunks reports the route of its chunks (the last,
    shorter chunk has the same S, P, aggregate and hit slots: the same route)."""
    route = getattr(t, "_tl_route", None)
    if route is None:
        raise ValueError("backward_route: not the x of a trace_skew call")
    return BACKWARD_ROUTES[route]


_last_use_inv = False
_last_route = _lib.ROUTE_CHECKPOINT


def set_backward_algorithm(name: str) -> None:
    global _bwd_algo
    if name not in ("checkpoint", "inverse"):
        raise ValueError("backward algorithm must be 'checkpoint' or 'inverse'")
    _bwd_algo = name


def get_backward_algorithm() -> str:
    return _bwd_algo


def set_default_mode(mode: str) -> None:
    """'strict' (bit-faithful fp32 op order) or 'fast' (FMA contraction, hardware rcp/sqrt)."""
    global _default_mode
    if mode not in _MODES:
        raise ValueError(f"mode must be one of {tuple(_MODES)}")
    _default_mode = mode


def get_default_mode() -> str:
    return _default_mode


def _require_device(t: torch.Tensor, name: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(
            f"torchoptics_amd: `{name}` lives on {t.device}; the ray tracer runs only as HIP kernels on an "
            "AMD GPU (there is no CPU fallback).  Move the lens and rays to device='cuda'.")


def _stream_ptr(device) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


_ws_cache = {}

# optional live timing of the C-ABI calls with events on the launch stream (bench.py)
_timing = None
_timing_named = None       # the same for calls that are not the trace's, under their entry point's name (named_timing_ms)


def enable_timing(on: bool = True) -> None:
    """Record a (start, stop) event pair around every tl_trace_fwd / tl_trace_bwd call."""
    global _timing, _timing_named
    _timing = {"fwd": [], "bwd": []} if on else None
    _timing_named = {} if on else None
    if _ext() is not None:
        _ext().enable_timing(bool(on))


def timing_counts() -> dict:
    """C-ABI trace calls recorded since enable_timing(True): {'fwd': n, 'bwd': n} (either host chain)."""
    out = {k: len(v) for k, v in (_timing or {}).items()}
    if _ext() is not None and _timing is not None:
        f, b = _ext().timing_counts()
        out = {"fwd": out.get("fwd", 0) + f, "bwd": out.get("bwd", 0) + b}
    return out


def timing_ms() -> dict:
    """Mean GPU milliseconds per call since enable_timing(); synchronises the device."""
    torch.cuda.synchronize()
    out = {k: (sum(a.elapsed_time(b) for a, b in v) / len(v) if v else None) for k, v in (_timing or {}).items()}
    if _ext() is not None and _timing is not None:
        f, b = _ext().timing_ms()
        out = {"fwd": f if f >= 0 else out.get("fwd"), "bwd": b if b >= 0 else out.get("bwd")}
    return out


def named_timing_ms() -> dict:
    """Mean GPU milliseconds per call, by entry point, of the timed calls outside the trace (tl_focus_moments, tl_focus_seed,
    tl_enclosed_centroid, tl_enclosed_sums, tl_enclosed_seed, tl_zfit_moments, tl_zfit_solve, tl_zfit_seed, tl_mtf_sums, tl_mtf_seed, tl_tfmtf_sums, tl_tfmtf_seed) since enable_timing();
    synchronises the device."""
    torch.cuda.synchronize()
    return {k: sum(a.elapsed_time(b) for a, b in v) / len(v) for k, v in (_timing_named or {}).items()}


class _Timed:
    def __init__(self, key, dev):
        self.key, self.dev = key, dev

    def __enter__(self):
        if _timing is not None:
            self.a = torch.cuda.Event(enable_timing=True)
            self.b = torch.cuda.Event(enable_timing=True)
            self.a.record(torch.cuda.current_stream(self.dev))

    def __exit__(self, *exc):
        if _timing is not None:
            self.b.record(torch.cuda.current_stream(self.dev))
            (_timing[self.key] if self.key in _timing else _timing_named.setdefault(self.key, [])).append((self.a, self.b))


class _NoCtx:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_NO_CTX = _NoCtx()


def _on_device(dev):
    """`with torch.cuda.device(dev)` only when dev is not the current device already (the usual case: ~6 us saved)."""
    return _NO_CTX if torch.cuda.current_device() == dev.index else torch.cuda.device(dev)


def _call(name, dev, *args, timed=None):
    """Call the launching C-ABI entry `name` on the current stream of `dev`: tensors go as their device pointers (None ->
    NULL), everything else (ints, floats, byref structs, pointer blocks) as it is, the stream last.  `timed`: 'fwd' /
    'bwd' records the call for timing_ms() while enable_timing() is on, any other name for named_timing_ms().  A non-zero
    return code raises."""
    with _on_device(dev), (_Timed(timed, dev) if timed is not None else _NO_CTX):
        rc = getattr(_lib.lib(), name)(*[_lib.ptr(a) if isinstance(a, torch.Tensor) else a for a in args],
                                       _stream_ptr(dev))
    if rc != 0:
        _lib.check(rc, name)


def workspace_of(device, stream=None) -> tuple:
    """The scratch tensors the kernels launched on `stream` of `device` (default: its current stream) write to right now:
    this module's and the C++ host chain's, as far as either has been needed there yet.  A HIP graph recorded on that stream
    holds their raw pointers: whoever owns the graph keeps the tensors (graphs.capture_step does), because both caches drop
    their own reference when a later call on a stream with the same handle needs a larger one."""
    device = torch.device(device)
    index = torch.cuda.current_device() if device.index is None else device.index
    stream = torch.cuda.current_stream(device) if stream is None else stream
    held = [_ws_cache.get((index, stream.cuda_stream))]
    if _ext() is not None and hasattr(_ext(), "workspace_of"):
        held.append(_ext().workspace_of(index, stream.cuda_stream))
    return tuple(t for t in held if t is not None)


def _workspace(nbytes: int, device) -> torch.Tensor:
    """Per-(device, stream) scratch for the block partials; grows monotonically.  Replacing it only drops the cache's
    reference: a captured graph that still writes to the old tensor holds its own (workspace_of)."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        _ws_cache[key] = ws
    return ws


# hit-point slots handed to the walk-back kernel per lens (tl_problem.asph_hits): lenses with more aspheric rows than
# this still get the right gradient, from the checkpoint kernel (decided on the device, no host sync on the row kinds)
ASPH_HIT_SLOTS = 4


def set_asph_hit_slots(n: int) -> None:
    """Hit-point slots per lens for the walk-back over aspheric rows (0.._lib.TL_MAX_HIT_SLOTS); 0 = no stored hits:
    Newton iteration on the reversed ray (trace_bwd_inv_kernel<true>)."""
    global ASPH_HIT_SLOTS
    if not 0 <= int(n) <= _lib.TL_MAX_HIT_SLOTS:
        raise ValueError(f"hit slots must be 0..{_lib.TL_MAX_HIT_SLOTS}")
    ASPH_HIT_SLOTS = int(n)


def _problem(x_e, y_e, z, cx, cy, c, t, mu, mask_u8, allow_back, mode, kappa=None, poly=None, kind_u8=None,
             n_index=None, aggregate=False, hits=None, moments_x=False, cond=None):
    B, F, P, W = x_e.shape
    p = tl_problem()
    p.F, p.P, p.W, p.S = F, P, W, c.shape[-1]
    p.B = B
    p.xs_b, p.ys_b = x_e.stride(0), y_e.stride(0)
    p.device = x_e.device.index
    p.mode = _MODES[mode]
    p.allow_backward = 1 if allow_back else 0
    p.aggregate = 1 if aggregate else 0
    p.x_in, p.y_in = x_e.data_ptr(), y_e.data_ptr()
    p.xs_f, p.xs_p, p.xs_w = x_e.stride(1), x_e.stride(2), x_e.stride(3)
    p.ys_f, p.ys_p, p.ys_w = y_e.stride(1), y_e.stride(2), y_e.stride(3)
    p.z, p.cx, p.cy = z.data_ptr(), cx.data_ptr(), cy.data_ptr()
    # cx, cy: [1|B, 1|F] contiguous (a 1-D [1|F] is read as one lens)
    cx, cy = (a.reshape(1, -1) if a.dim() == 1 else a for a in (cx, cy))
    p.cx_stride, p.cx_stride_b = (0 if cx.shape[1] == 1 else 1), (0 if cx.shape[0] == 1 else cx.shape[1])
    p.cy_stride, p.cy_stride_b = (0 if cy.shape[1] == 1 else 1), (0 if cy.shape[0] == 1 else cy.shape[1])
    p.c, p.t, p.mu, p.mask = c.data_ptr(), t.data_ptr(), mu.data_ptr(), mask_u8.data_ptr()
    asph = kind_u8 is not None
    p.kappa = kappa.data_ptr() if asph else None
    p.poly = poly.data_ptr() if asph else None
    p.surf_kind = kind_u8.data_ptr() if asph else None
    p.n_index = n_index.data_ptr() if n_index is not None else None
    p.asph_hits = hits.data_ptr() if hits is not None else None
    p.asph_hit_slots = hits.shape[0] if hits is not None else 0
    p.moments_x = 1 if moments_x else 0
    p.cond_flags = cond.data_ptr() if cond is not None else None
    return p


def _fwp(t):
    """[B,F,P,W] logical tensor -> memory laid out [B,F,W,P] contiguous (no copy if it already is)."""
    return t.permute(0, 1, 3, 2).contiguous()


class _Precision(NamedTuple):
    """What the trace node takes from the element type of its rays."""
    dtype: torch.dtype        # every float allocation, and the cast of the backward's seeds
    ws_bytes: str             # the C-ABI entries: workspace size, forward, checkpoint backward
    fwd: str
    bwd: str
    walk_back: bool           # tl_trace_bwd_from_outputs (with its hit-point and conditioning buffers) exists
    timed: bool               # the calls are recorded by enable_timing()


_F32 = _Precision(torch.float32, "tl_workspace_bytes", "tl_trace_fwd", "tl_trace_bwd", True, True)
# RayTracer(double_precision=True): generic, untuned fp64 kernels, checkpoint backward; no penalty term, no optical path length
_F64 = _Precision(torch.float64, "tl_workspace_bytes_f64", "tl_trace_fwd_f64", "tl_trace_bwd_f64", False, False)


class TraceFunction(torch.autograd.Function):
    """(x, y, cx, cy, ok, back, moments, opd, stacks) = trace(x_in, y_in, z, cx, cy, c, t, mu[, kappa, poly]).

    Shapes: x_in, y_in [B,F,P,W] (expanded views welcome), z [B], cx, cy [1|B, 1|F], c, t [B,S], mu [B,W,S],
    mask_u8 [B,S]; kappa [B,S], poly [B,S,4], kind_u8 [B,S] are None for an all-spherical lens (the reference's
    case); n_index [B,W,S+1] is only needed for the optical path length output (`want_opd`).  moments [B*F, TL_NMOM].
    float64 rays run the double-precision kernels: every float argument float64, mode 'strict', no `want_opd`, no
    `aggregate` (trace_skew refuses them), and the x-moments are always filled."""

    @staticmethod
    def forward(ctx, x_e, y_e, z, cx, cy, c, t, mu, kappa, poly, mask_u8, kind_u8, n_index, allow_back, mode,
                want_rays, want_opd, aggregate, want_stacks, moments_x=False):
        prec = _F64 if x_e.dtype == torch.float64 else _F32
        for name, ten in (("x", x_e), ("y", y_e), ("z", z), ("cx", cx), ("cy", cy), ("c", c), ("t", t),
                          ("mu", mu), ("mask", mask_u8)):
            _require_device(ten, name)
            if prec is _F64 and name != "mask" and ten.dtype != torch.float64:
                raise TypeError(f"double-precision trace: `{name}` is {ten.dtype}")
        dev = x_e.device
        B, F, P, W = x_e.shape
        S = c.shape[-1]
        if S > _lib.TL_MAX_SURFACES:
            raise RuntimeError(f"lens has {S} rows; this build supports at most {_lib.TL_MAX_SURFACES}")
        # per-ray input gradients (ray aiming: a handful of rays) keep the checkpoint algorithm: extreme rays
        # amplify the reconstruction rounding of the walk-back to ~1e-4 in d/dx_in, d/dy_in
        # ... and so does the gradient through the optical path length (only the checkpoint kernel carries it)
        use_inv = (prec.walk_back and _bwd_algo == "inverse" and want_rays and allow_back and not want_opd
                   and not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]))
        # aspheric rows: the forward leaves their hit points for the walk-back (8 B per ray and slot actually used)
        hits = None
        if use_inv and kind_u8 is not None and ASPH_HIT_SLOTS > 0 and any(ctx.needs_input_grad[2:10]):
            hits = torch.empty((min(ASPH_HIT_SLOTS, S), 2, B, F, W, P), dtype=torch.float32, device=dev)
        # one byte per ray: the forward flags the ill-conditioned live rays, so that the backward can leave exactly those
        # to the checkpoint kernel and walk back the rest (without it, one such ray costs the whole launch the walk-back)
        cond = (torch.empty((B, F, W, P), dtype=torch.uint8, device=dev)
                if use_inv and any(ctx.needs_input_grad[2:10]) else None)
        prob = _problem(x_e, y_e, z, cx, cy, c, t, mu, mask_u8, allow_back, mode, kappa, poly, kind_u8, n_index, aggregate,
                        hits, moments_x, cond)
        nbytes = getattr(_lib.lib(), prec.ws_bytes)(C.byref(prob))
        ws = _workspace(nbytes, dev)
        if want_rays:
            fp = [torch.empty((B, F, W, P), dtype=prec.dtype, device=dev) for _ in range(4)]
            bp = [torch.empty((B, F, W, P), dtype=torch.uint8, device=dev) for _ in range(2)]
        else:
            fp, bp = [None] * 4, [None] * 2
        opd = torch.empty((B, F, W, P), dtype=prec.dtype, device=dev) if want_opd else None
        stacks = torch.empty((3, S, B, F, W, P), dtype=prec.dtype, device=dev) if (aggregate and want_stacks) else None
        moments = torch.empty((B * F, TL_NMOM), dtype=torch.float64, device=dev)
        out = _lib.rays(x=fp[0], y=fp[1], cx=fp[2], cy=fp[3], ok=bp[0], back=bp[1], opd=opd, stacks=stacks, moments=moments)
        _call(prec.fwd, dev, C.byref(prob), out, ws, ws.numel(), timed="fwd" if prec.timed else None)
        global _last_use_inv, _last_route
        _last_use_inv = use_inv
        # (tl_bwd_route reads the problem's sizes and hit-slot members only: the same answer in backward)
        _last_route = _lib.lib().tl_bwd_route(C.byref(prob)) if use_inv else _lib.ROUTE_CHECKPOINT
        fwd_out = (fp[0], fp[1], fp[2], fp[3], bp[0], moments) if use_inv else (None,) * 6
        ctx.save_for_backward(x_e, y_e, z, cx, cy, c, t, mu, mask_u8, kappa, poly, kind_u8, *fwd_out,
                              n_index if want_opd else None, hits, cond)
        ctx.allow_back, ctx.mode, ctx.aggregate, ctx.use_inv = allow_back, mode, aggregate, use_inv
        ctx.prob, ctx.ws_bytes = prob, nbytes      # same tensors, same pointers in backward: no need to fill it again
        ctx.set_materialize_grads(False)
        if want_rays:
            outs = [b.permute(0, 1, 3, 2) for b in fp]
            flags = [b.view(torch.bool).permute(0, 1, 3, 2) for b in bp]
        else:
            outs = [torch.empty(0, dtype=prec.dtype, device=dev) for _ in range(4)]
            flags = [torch.empty(0, dtype=torch.bool, device=dev) for _ in range(2)]
        opd_out = opd.permute(0, 1, 3, 2) if want_opd else torch.empty(0, dtype=prec.dtype, device=dev)
        stk_out = stacks.permute(0, 1, 2, 3, 5, 4) if stacks is not None else torch.empty(0, dtype=prec.dtype, device=dev)
        # the stacks are differentiable (their gradient reaches the backward calls as tl_seeds.g_stacks); the placeholders are not
        ctx.mark_non_differentiable(*flags)
        if not want_opd:
            ctx.mark_non_differentiable(opd_out)
        if stacks is None:
            ctx.mark_non_differentiable(stk_out)
        return (*outs, *flags, moments, opd_out, stk_out)

    @staticmethod
    def backward(ctx, gx, gy, gcx, gcy, _gok, _gback, gmom, gopd, gstk):
        (x_e, y_e, z, cx, cy, c, t, mu, mask_u8, kappa, poly, kind_u8, fx, fy, fcx, fcy, fok, fmom,
         n_index, hits, cond) = ctx.saved_tensors
        dev = x_e.device
        B, F, P, W = x_e.shape
        S = c.shape[-1]
        prec = _F64 if x_e.dtype == torch.float64 else _F32
        if gopd is not None and (n_index is None or gopd.numel() == 0):
            gopd = None
        # gradient of the per-surface stacks [3,S,B,F,P,W] -> g_stacks [3][S][B,F,W,P], the layout of the forward's output
        gstkd = None
        if ctx.aggregate and gstk is not None and gstk.numel() > 0:
            gstkd = gstk.to(prec.dtype).permute(0, 1, 2, 3, 5, 4).contiguous()
        if (gx is None and gy is None and gcx is None and gcy is None and gmom is None and gopd is None
                and gstkd is None):
            return (None,) * 20
        asph = kind_u8 is not None
        prob = ctx.prob
        # saved-tensor hooks (save_on_cpu, checkpointing) hand back tensors in other storage than the forward saw
        if (prob.x_in != (x_e.data_ptr() or None) or prob.c != c.data_ptr() or prob.mu != mu.data_ptr()
                or prob.asph_hits != (hits.data_ptr() if hits is not None else None)
                or prob.cond_flags != (cond.data_ptr() if cond is not None else None)):
            prob = _problem(x_e, y_e, z, cx, cy, c, t, mu, mask_u8, ctx.allow_back, ctx.mode, kappa, poly, kind_u8, None,
                            ctx.aggregate, hits, False, cond)
        prob.n_index = n_index.data_ptr() if gopd is not None else None
        ws = _workspace(ctx.ws_bytes, dev)

        def dense(g):
            if g is None or g.numel() == 0:
                return None
            return _fwp(g.to(prec.dtype))
        gxd, gyd, gcxd, gcyd, gopdd = dense(gx), dense(gy), dense(gcx), dense(gcy), dense(gopd)
        gmd = None if gmom is None else gmom.to(torch.float64).contiguous()
        need = ctx.needs_input_grad
        # one tensor per parameter group in the rays' element type, written by the reduction kernel (fp64 sums rounded
        # once): autograd can take them as the leaves' .grad without a cast or a clone
        new = lambda *shape: torch.empty(shape, dtype=prec.dtype, device=dev)     # noqa: E731
        gxin = new(B, F, W, P) if need[0] else None
        gyin = new(B, F, W, P) if need[1] else None
        g_c, g_t, g_mu, g_z, g_cx, g_cy = new(B, S), new(B, S), new(B, W, S), new(B), new(B, F), new(B, F)
        g_kappa, g_poly = (new(B, S), new(B, S, 4)) if asph else (None, None)
        g_n = new(B, W, S + 1) if gopdd is not None else None
        g = _lib.seeds(gx=gxd, gy=gyd, gcx=gcxd, gcy=gcyd, g_moments=gmd, g_opd=gopdd, g_stacks=gstkd)
        out = _lib.grads(g_c=g_c, g_t=g_t, g_mu=g_mu, g_z=g_z, g_cx=g_cx, g_cy=g_cy, g_kappa=g_kappa, g_poly=g_poly,
                         g_n_index=g_n, g_x_in=gxin, g_y_in=gyin)
        timed = "bwd" if prec.timed else None
        if ctx.use_inv:
            fwd = _lib.rays(x=fx, y=fy, cx=fcx, cy=fcy, ok=fok, moments=fmom)
            _call("tl_trace_bwd_from_outputs", dev, C.byref(prob), g, fwd, out, ws, ws.numel(), timed=timed)
        else:
            _call(prec.bwd, dev, C.byref(prob), g, out, ws, ws.numel(), timed=timed)

        def fold(g, like):          # [B,F] -> the (possibly broadcast) shape [1|B, 1|F] of cx / cy
            if like.shape[0] == 1 and B > 1:
                g = g.sum(dim=0, keepdim=True)
            if like.shape[1] == 1 and F > 1:
                g = g.sum(dim=1, keepdim=True)
            return g.reshape(like.shape)
        return (gxin.permute(0, 1, 3, 2) if need[0] else None, gyin.permute(0, 1, 3, 2) if need[1] else None,
                g_z.reshape(z.shape) if need[2] else None, fold(g_cx, cx) if need[3] else None,
                fold(g_cy, cy) if need[4] else None,
                g_c.reshape(c.shape), g_t.reshape(t.shape), g_mu.reshape(mu.shape),
                g_kappa.reshape(kappa.shape) if asph else None, g_poly.reshape(poly.shape) if asph else None,
                None, None, g_n.reshape(n_index.shape) if g_n is not None else None, None, None, None, None, None, None,
                None)


class SpotRmsFunction(torch.autograd.Function):
    """rms = compute_rms2d on the [F, TL_NMOM] moments (closed form) with its derivative, one tiny
    kernel each way instead of the ~25 elementwise kernels of the eager formula and its autograd.
    n_lens > 1: moments [n_lens * F, TL_NMOM] of a lens batch -> rms [n_lens], one value per lens."""

    @staticmethod
    def forward(ctx, moments, n_per_field, n_lens=1):
        _require_device(moments, "moments")
        dev = moments.device
        m = moments.to(torch.float64).contiguous()
        rms = torch.empty(() if n_lens == 1 else (n_lens,), dtype=torch.float32, device=dev)
        dm = torch.empty_like(m)
        _call("tl_spot_rms", dev, dev.index, n_lens, m.shape[0] // n_lens, float(n_per_field), m, rms, dm)
        ctx.save_for_backward(dm)
        ctx.n_lens = n_lens
        return rms

    @staticmethod
    def backward(ctx, g):
        (dm,) = ctx.saved_tensors
        if ctx.n_lens == 1:
            return dm * g, None, None          # [F,10] fp64 * 0-dim fp32 -> fp64 in one launch (no separate cast)
        return (dm.view(ctx.n_lens, -1, TL_NMOM) * g.view(-1, 1, 1)).view_as(dm), None, None


class SpotMomentsFunction(torch.autograd.Function):
    """moments[F, TL_NMOM] of arbitrary per-ray tensors x, y, ok shaped [1, F, P, W]."""

    @staticmethod
    def forward(ctx, x, y, ok):
        _require_device(y, "y")
        dev = y.device
        _, F, P, W = y.shape
        if y.dtype != torch.float32 or any(s == 0 for s in y.stride()[1:]):
            y = y.to(torch.float32).contiguous()
        xs = None
        if x is not None:
            xs = x.to(torch.float32)
            if xs.stride() != y.stride():
                xs = torch.empty_strided(y.shape, y.stride(), dtype=torch.float32, device=dev).copy_(xs)
        oks = ok.view(torch.uint8) if ok.dtype == torch.bool else ok.to(torch.uint8)
        if oks.stride() != y.stride():
            oks = torch.empty_strided(y.shape, y.stride(), dtype=torch.uint8, device=dev).copy_(oks)
        moments = torch.empty((F, TL_NMOM), dtype=torch.float64, device=dev)
        ws = _workspace(F * W * ((P + 255) // 256) * TL_NMOM * 8 + 256, dev)
        _call("tl_spot_moments", dev, dev.index, F, P, W, xs, y, oks, y.stride(1), y.stride(2), y.stride(3), moments,
              ws, ws.numel())
        ctx.save_for_backward(xs if xs is not None else y, y, oks)
        ctx.has_x = xs is not None
        return moments

    @staticmethod
    def backward(ctx, gmom):
        xs, y, oks = ctx.saved_tensors
        dev = y.device
        _, F, P, W = y.shape
        gm = gmom.to(torch.float64).contiguous()
        gy = torch.empty_strided(y.shape, y.stride(), dtype=torch.float32, device=dev)
        need_x = ctx.has_x and ctx.needs_input_grad[0]
        gx = torch.empty_strided(y.shape, y.stride(), dtype=torch.float32, device=dev) if need_x else None
        _call("tl_spot_seed", dev, dev.index, F, P, W, xs if ctx.has_x else None, y, oks, y.stride(1), y.stride(2),
              y.stride(3), gm, gx, gy)
        return gx, gy, None


FOCUS_NMOM = 11            # per (field, wavelength): sums of 1, x, y, u, v, x^2, y^2, u^2, v^2, x u, y v over the live rays


def _same_layout(t, shape, stride):
    """Whether t's elements sit at the given strides (the stride of a dimension of size 1 addresses nothing)."""
    return all(n == 1 or a == b for n, a, b in zip(shape, t.stride(), stride))


def _focus_layout(tensors):
    """The stride quadruple [B,F,P,W] the focus kernels read all five arrays with: that of the first float32 tensor that is
    not expanded and whose lenses fold into its fields (B = 1, F = 1, or stride(0) = F stride(1)) -- the tracer's [1,F,P,W]
    views of [F,W,P] memory are -- or the tracer's own layout."""
    shape = tensors[0].shape
    B, F = shape[0], shape[1]
    for t in tensors:
        st = t.stride()
        if (t.dtype == torch.float32 and all(n == 1 or s > 0 for n, s in zip(shape, st))
                and (B == 1 or F == 1 or st[0] == F * st[1])):
            return st
    B, F, P, W = shape
    return (F * W * P, W * P, 1, P)


def _row_rays(rays, ok, noun, what="tensors"):
    """The float32 ray tensors `rays` (name -> tensor, all of ONE shape [B,F,P,W]) and `ok` as the row kernels read them:
    (the tensors placed, oks, st, s_f) -- all at the one stride quadruple st of _focus_layout (only what is expanded or strided
    differently is copied), ok as uint8, and s_f the field stride once B is folded into F.  The device and dtype checks of the
    rays come first and raise before anything is copied; a caller's further argument checks (MTFSumsFunction: J and origin,
    ZernikeFitFunction: the devices of px, py) run after the copies, in the order and with the texts they always had, so only an
    error path does work it then throws away."""
    for name, t in rays.items():
        _require_device(t, name)
        if t.dtype != torch.float32:
            raise RuntimeError(f"torchoptics_amd: the {noun} kernels take float32 {what}; `{name}` is {t.dtype} "
                               "(there is no CPU fallback and no fp64 kernel: use fused=False)")
    _require_device(ok, "ray_ok")
    tensors = tuple(rays.values())
    dev, shape = tensors[0].device, tensors[0].shape
    st = _focus_layout(tensors)

    def placed(t):
        return t if _same_layout(t, shape, st) else torch.empty_strided(shape, st, dtype=t.dtype, device=dev).copy_(t)
    tensors = [placed(t) for t in tensors]
    oks = placed(ok.view(torch.uint8) if ok.dtype == torch.bool else ok if ok.dtype == torch.uint8 else (ok != 0).view(torch.uint8))
    s_f = st[1] if shape[0] == 1 else st[0] if shape[1] == 1 else st[1]
    return tensors, oks, st, s_f


def _ray_grads(ctx, n, like, st):
    """The seeds of the first n inputs, laid out as the rays `like` are: None where needs_input_grad says so."""
    return [torch.empty_strided(like.shape, st, dtype=torch.float32, device=like.device) if need else None
            for need in ctx.needs_input_grad[:n]]


class FocusMomentsFunction(torch.autograd.Function):
    """moments [B, F, W, FOCUS_NMOM] (float64) of per-ray tensors x, y, cx, cy, ok, all of ONE shape [B, F, P, W] (the caller
    broadcasts, under autograd): tl_focus_moments forward, tl_focus_seed backward.  The five arrays are brought to one common
    stride quadruple -- the tracer's [1,F,P,W] views of [F,W,P] memory are read in place, only what is expanded or strided
    differently is copied -- and B is folded into F."""

    @staticmethod
    def forward(ctx, x, y, cx, cy, ok):
        (x, y, cx, cy), oks, st, s_f = _row_rays({"x": x, "y": y, "cx": cx, "cy": cy}, ok, "focus")
        dev = x.device
        B, F, P, W = x.shape
        moments = torch.empty((B, F, W, FOCUS_NMOM), dtype=torch.float64, device=dev)
        ws = _workspace(_lib.lib().tl_focus_workspace_bytes(B * F, P, W), dev)
        _call("tl_focus_moments", dev, dev.index, B * F, P, W, x, y, cx, cy, oks, s_f, st[2], st[3], moments, ws, ws.numel(),
              timed="tl_focus_moments")
        ctx.save_for_backward(x, y, cx, cy, oks)
        ctx.layout = (st, s_f)
        return moments

    @staticmethod
    def backward(ctx, gmom):
        x, y, cx, cy, oks = ctx.saved_tensors
        dev, shape = x.device, x.shape
        B, F, P, W = shape
        st, s_f = ctx.layout
        gm = gmom.to(torch.float64).contiguous()
        outs = _ray_grads(ctx, 4, x, st)
        if all(o is None for o in outs):
            return (None,) * 5
        _call("tl_focus_seed", dev, dev.index, B * F, P, W, x, y, cx, cy, oks, s_f, st[2], st[3], gm, *outs,
              timed="tl_focus_seed")
        return (*outs, None)


ENCLOSED_MAX_K = 32        # radii per tl_enclosed_sums / tl_enclosed_seed call (the largest register bucket)
ENCLOSED_SHAPES = {"circle": 0, "square": 1}


def _host_doubles(values):
    return (C.c_double * len(values))(*values)


class EnclosedEnergyFunction(torch.autograd.Function):
    """(S [B, F, W, 3], sums [B, F, W, K]), both float64, of per-ray tensors x, y, ok of ONE shape [B, F, P, W]: S = (n, sum x,
    sum y) over the live rays (tl_enclosed_centroid), sums[.., k] = the live rays' edge terms about the centre
    (tl_enclosed_sums); backward is tl_enclosed_seed.  `centre`: a tensor broadcastable to [B, F, W, 2] (differentiable), or
    "row" / "field": the centroid S[.., 1:3] / n of the row, or of the field's rows together, formed here from S and
    differentiated through.  radii, inv_soft: K <= ENCLOSED_MAX_K host floats; shape: "circle" / "square".  The three arrays
    are brought to one layout exactly as FocusMomentsFunction does, and B is folded into F.  Nothing of size rays x K is stored."""

    @staticmethod
    def _centre_of(S, mode):
        if mode == "field":
            S = S.sum(dim=2, keepdim=True).expand_as(S)
        return S[..., 1:3] / S[..., :1].clamp(min=1.0), S[..., :1].clamp(min=1.0)

    @staticmethod
    def forward(ctx, x, y, ok, centre, radii, inv_soft, shape):
        (x, y), oks, st, s_f = _row_rays({"x": x, "y": y}, ok, "enclosed-energy")
        dev = x.device
        B, F, P, W = x.shape
        K = len(radii)
        rays = (dev.index, B * F, P, W, x, y, oks, s_f, st[2], st[3])
        # (no radii: S alone, metrics.spot_centroid; the seed call then runs on one radius whose seed is 0)
        edge = (_host_doubles(radii or (1.0,)), _host_doubles(inv_soft or (1.0,)), max(K, 1), ENCLOSED_SHAPES[shape])
        S = torch.empty((B, F, W, 3), dtype=torch.float64, device=dev)
        sums = torch.empty((B, F, W, K), dtype=torch.float64, device=dev)
        ws = _workspace(_lib.lib().tl_enclosed_workspace_bytes(B * F, P, W, max(K, 1)), dev)
        _call("tl_enclosed_centroid", dev, *rays, S, ws, ws.numel(), timed="tl_enclosed_centroid")
        if isinstance(centre, str):
            c = EnclosedEnergyFunction._centre_of(S, centre)[0]
        else:
            _require_device(centre, "centre")
            c = centre
        c64 = torch.empty((B, F, W, 2), dtype=torch.float64, device=dev).copy_(c)
        if K:
            _call("tl_enclosed_sums", dev, *rays, c64, *edge, sums, ws, ws.numel(), timed="tl_enclosed_sums")
        ctx.save_for_backward(x, y, oks, c64, S)
        ctx.plan = (st, s_f, edge, centre if isinstance(centre, str) else (centre.shape, centre.dtype))
        return S, sums

    @staticmethod
    def backward(ctx, g_S, g_sums):
        x, y, oks, c64, S = ctx.saved_tensors
        dev, full = x.device, x.shape
        B, F, P, W = full
        st, s_f, edge, centre = ctx.plan
        rays = (dev.index, B * F, P, W, x, y, oks, s_f, st[2], st[3])
        if g_sums.shape[-1]:
            gs = torch.empty(g_sums.shape, dtype=torch.float64, device=dev).copy_(g_sums)
        else:
            gs = torch.empty((B, F, W, 1), dtype=torch.float64, device=dev).zero_()
        g_lin = torch.empty((B, F, W, 2), dtype=torch.float64, device=dev).copy_(g_S[..., 1:3])
        outs = _ray_grads(ctx, 2, x, st)
        ws = _workspace(_lib.lib().tl_enclosed_workspace_bytes(B * F, P, W, edge[2]), dev)
        g_centre = None
        if isinstance(centre, str):
            if all(o is None for o in outs):
                return (None,) * 7
            # the centroid's share: the centre's gradient alone first, then spread over the live rays it is the mean of
            g_c = torch.empty((B, F, W, 2), dtype=torch.float64, device=dev)
            _call("tl_enclosed_seed", dev, *rays, c64, *edge, gs, None, None, None, g_c, ws, ws.numel(), timed="tl_enclosed_seed")
            n1 = EnclosedEnergyFunction._centre_of(S, centre)[1]
            if centre == "field":
                g_c = g_c.sum(dim=2, keepdim=True).expand_as(g_lin)
            g_lin = (g_lin + g_c / n1).contiguous()
            _call("tl_enclosed_seed", dev, *rays, c64, *edge, gs, g_lin, *outs, None, ws, ws.numel(), timed="tl_enclosed_seed")
        else:
            want_c = ctx.needs_input_grad[3]
            if all(o is None for o in outs) and not want_c:
                return (None,) * 7
            g_c = torch.empty((B, F, W, 2), dtype=torch.float64, device=dev) if want_c else None
            _call("tl_enclosed_seed", dev, *rays, c64, *edge, gs, g_lin, *outs, g_c, ws, ws.numel(), timed="tl_enclosed_seed")
            if want_c:
                g_centre = g_c.sum_to_size(centre[0]).to(centre[1])
        return (*outs, None, g_centre, None, None, None)


MTF_MAX_J = 16             # frequency vectors per tl_mtf_sums / tl_mtf_seed call (the largest register bucket)


class MTFSumsFunction(torch.autograd.Function):
    """sums [B, F, W, J, 2] (float64) = (C_j, S_j), the sums of cos / sin(2 pi nu_j . (r - origin)) over the live rays, of per-ray
    tensors x, y, ok of ONE shape [B, F, P, W]: tl_mtf_sums forward, tl_mtf_seed backward.  `origin`: a float64 tensor [B, F, W, 2],
    possibly expanded; a constant of the calculation (the modulus does not depend on it): no gradient.  It is read in place where it
    is contiguous and copied otherwise, as EnclosedEnergyFunction's centre is.  nu_x, nu_y: J <= MTF_MAX_J host floats (cycles per
    unit of x).  The three ray arrays are brought to one layout exactly as FocusMomentsFunction does, and B is folded into F.
    Nothing of size rays x J is stored."""

    @staticmethod
    def forward(ctx, x, y, ok, origin, nu_x, nu_y):
        (x, y), oks, st, s_f = _row_rays({"x": x, "y": y}, ok, "MTF")
        _require_device(origin, "origin")
        dev, full = x.device, x.shape
        B, F, P, W = full
        J = len(nu_x)
        if not 1 <= J <= MTF_MAX_J or len(nu_y) != J:
            raise ValueError(f"nu_x and nu_y must hold the same 1 .. {MTF_MAX_J} frequencies, got {J} and {len(nu_y)}")
        if origin.dtype != torch.float64 or tuple(origin.shape) != (B, F, W, 2):
            raise ValueError(f"origin must be a float64 tensor [B, F, W, 2] = {(B, F, W, 2)}, got {origin.dtype} {tuple(origin.shape)}")
        o64 = origin.detach()
        if not o64.is_contiguous():
            o64 = torch.empty((B, F, W, 2), dtype=torch.float64, device=dev).copy_(o64)
        sums = torch.empty((B, F, W, J, 2), dtype=torch.float64, device=dev)
        ctx.save_for_backward(x, y, oks, o64)
        ctx.plan = (st, s_f, (_host_doubles(nu_x), _host_doubles(nu_y), J))
        if P == 0 or sums.numel() == 0:                     # an empty fan: every sum is 0
            return sums.zero_()
        ws = _workspace(_lib.lib().tl_mtf_workspace_bytes(B * F, P, W, J), dev)
        _call("tl_mtf_sums", dev, dev.index, B * F, P, W, x, y, oks, s_f, st[2], st[3], o64, *ctx.plan[2], sums, ws, ws.numel(),
              timed="tl_mtf_sums")
        return sums

    @staticmethod
    def backward(ctx, g_sums):
        x, y, oks, o64 = ctx.saved_tensors
        dev, full = x.device, x.shape
        B, F, P, W = full
        st, s_f, freq = ctx.plan
        outs = _ray_grads(ctx, 2, x, st)
        if all(o is None for o in outs) or x.numel() == 0:
            return (*outs, None, None, None, None)
        gs = torch.empty(g_sums.shape, dtype=torch.float64, device=dev).copy_(g_sums)
        ws = _workspace(_lib.lib().tl_mtf_workspace_bytes(B * F, P, W, freq[2]), dev)
        _call("tl_mtf_seed", dev, dev.index, B * F, P, W, x, y, oks, s_f, st[2], st[3], o64, *freq, gs, *outs, ws, ws.numel(),
              timed="tl_mtf_seed")
        return (*outs, None, None, None, None)


TFMTF_MAX_J = 16           # frequency vectors per tl_tfmtf_sums / tl_tfmtf_seed call
TFMTF_MAX_Z = 16           # focal planes per call


class TFMTFSumsFunction(torch.autograd.Function):
    """sums [B, F, W, J, Z, 2] (float64) = (C_jz, S_jz), the Fourier sums of the live rays at the Z focal planes first + z step, of
    per-ray tensors x, y, cx, cy, ok of ONE shape [B, F, P, W]: tl_tfmtf_sums forward, tl_tfmtf_seed backward (include/tl_trace.h
    states the definition).  `origin`, nu_x, nu_y as for MTFSumsFunction; first, step: host floats, Z <= TFMTF_MAX_Z planes.  The
    five ray arrays are brought to one layout exactly as FocusMomentsFunction does, and B is folded into F.  Nothing of size rays x
    J or rays x Z is stored, and only the gradients that are asked for are computed."""

    @staticmethod
    def forward(ctx, x, y, cx, cy, ok, origin, nu_x, nu_y, first, step, Z):
        (x, y, cx, cy), oks, st, s_f = _row_rays({"x": x, "y": y, "cx": cx, "cy": cy}, ok, "through-focus MTF")
        _require_device(origin, "origin")
        dev, full = x.device, x.shape
        B, F, P, W = full
        J = len(nu_x)
        if not 1 <= J <= TFMTF_MAX_J or len(nu_y) != J:
            raise ValueError(f"nu_x and nu_y must hold the same 1 .. {TFMTF_MAX_J} frequencies, got {J} and {len(nu_y)}")
        if not 1 <= Z <= TFMTF_MAX_Z:
            raise ValueError(f"a call takes 1 .. {TFMTF_MAX_Z} planes, got {Z}")
        if origin.dtype != torch.float64 or tuple(origin.shape) != (B, F, W, 2):
            raise ValueError(f"origin must be a float64 tensor [B, F, W, 2] = {(B, F, W, 2)}, got {origin.dtype} {tuple(origin.shape)}")
        o64 = origin.detach()
        if not o64.is_contiguous():
            o64 = torch.empty((B, F, W, 2), dtype=torch.float64, device=dev).copy_(o64)
        sums = torch.empty((B, F, W, J, Z, 2), dtype=torch.float64, device=dev)
        ctx.save_for_backward(x, y, cx, cy, oks, o64)
        ctx.plan = (st, s_f, (_host_doubles(nu_x), _host_doubles(nu_y), J, float(first), float(step), Z))
        if P == 0 or sums.numel() == 0:                     # an empty fan: every sum is 0
            return sums.zero_()
        ws = _workspace(_lib.lib().tl_tfmtf_workspace_bytes(B * F, P, W, J, Z), dev)
        _call("tl_tfmtf_sums", dev, dev.index, B * F, P, W, x, y, cx, cy, oks, s_f, st[2], st[3], o64, *ctx.plan[2], sums, ws,
              ws.numel(), timed="tl_tfmtf_sums")
        return sums

    @staticmethod
    def backward(ctx, g_sums):
        x, y, cx, cy, oks, o64 = ctx.saved_tensors
        dev, full = x.device, x.shape
        B, F, P, W = full
        st, s_f, planes = ctx.plan
        outs = _ray_grads(ctx, 4, x, st)
        if all(o is None for o in outs) or x.numel() == 0:
            return (*outs, None, None, None, None, None, None, None)
        gs = torch.empty(g_sums.shape, dtype=torch.float64, device=dev).copy_(g_sums)
        ws = _workspace(_lib.lib().tl_tfmtf_workspace_bytes(B * F, P, W, planes[2], planes[5]), dev)
        _call("tl_tfmtf_seed", dev, dev.index, B * F, P, W, x, y, cx, cy, oks, s_f, st[2], st[3], o64, *planes, gs, *outs, ws,
              ws.numel(), timed="tl_tfmtf_seed")
        return (*outs, None, None, None, None, None, None, None)


ZFIT_ORDERS = (2, 3, 4, 5, 6)     # radial orders the tl_zfit_* kernels are instantiated for


def zfit_sizes(order):
    """(J, K) of a Zernike fit of radial order `order`: coefficients Z_2 .. Z_{J+1}, monomial sums per row (include/tl_trace.h)."""
    if order not in ZFIT_ORDERS:
        raise ValueError(f"max_order must be one of {ZFIT_ORDERS}, got {order!r}")
    return (order + 1) * (order + 2) // 2 - 1, 3 * order * order + 2


def _pupil_layout(px, py, shape, dev):
    """px, py [B,F,P,W] as the zfit kernels read them: one stride quadruple for both whose lenses fold into its fields.  The
    kernels only read them, so an expanded pupil (stride 0 over lenses, fields and wavelengths) goes as it is; what is not
    float32 on `dev`, or strided otherwise, is copied into the tracer's [B,F,W,P] memory."""
    B, F, P, W = shape
    st = px.stride()

    def folds(t):
        s = t.stride()
        return B == 1 or F == 1 or s[0] == F * s[1]
    if not (px.dtype == py.dtype == torch.float32 and px.device == py.device == dev and folds(px) and _same_layout(py, shape, st)):
        st = (F * W * P, W * P, 1, P)
        px, py = (torch.empty_strided(shape, st, dtype=torch.float32, device=dev).copy_(t) for t in (px, py))
    return px, py, (st[1] if B == 1 else st[0] if F == 1 else st[1], st[2], st[3])


class ZernikeFitFunction(torch.autograd.Function):
    """(moments [B, F, W, K], a [B, F, W, J], q [B, F, W], valid [B, F, W]) of per-ray tensors x, y, ok, px, py of ONE shape
    [B, F, P, W] (the caller broadcasts): the monomial sums of tl_zfit_moments, the coefficients a of the least-squares fit of
    (x, y) against the gradients of the Noll Zernike polynomials Z_2 .. Z_{J+1} at the pupil coordinates (px, py), the residual
    sum q = sum (x^2 + y^2) - b . a and the validity flag (tl_zfit_solve); float64, uint8 the flag.  An invalid row has a = 0,
    q = 0.  Backward: tl_zfit_solve's adjoint and tl_zfit_seed, to x and y only; the moments are an intermediate and carry no
    gradient.  x, y, ok are brought to one layout exactly as FocusMomentsFunction does, px and py are read with strides of their
    own (_pupil_layout), and B is folded into F."""

    @staticmethod
    def forward(ctx, x, y, ok, px, py, order):
        J, K = zfit_sizes(order)
        (x, y), oks, st, s_f = _row_rays({"x": x, "y": y}, ok, "Zernike-fit", "rays")
        for name, t in (("px", px), ("py", py)):
            _require_device(t, name)
        dev, shape = x.device, x.shape
        B, F, P, W = shape
        px, py, pst = _pupil_layout(px, py, shape, dev)
        rays = (dev.index, B * F, P, W, order, x, y, oks, s_f, st[2], st[3], px, py, *pst)
        moments = torch.empty((B, F, W, K), dtype=torch.float64, device=dev)
        a = torch.empty((B, F, W, J), dtype=torch.float64, device=dev)
        q = torch.empty((B, F, W), dtype=torch.float64, device=dev)
        valid = torch.empty((B, F, W), dtype=torch.uint8, device=dev)
        factor = torch.empty((B, F, W, J * J + J), dtype=torch.float64, device=dev)
        ws = _workspace(_lib.lib().tl_zfit_workspace_bytes(B * F, P, W, order), dev)
        _call("tl_zfit_moments", dev, *rays, moments, ws, ws.numel(), timed="tl_zfit_moments")
        _call("tl_zfit_solve", dev, dev.index, B * F * W, order, moments, None, None, a, q, valid, factor, None, timed="tl_zfit_solve")
        ctx.save_for_backward(x, y, oks, px, py, a, valid, factor)
        ctx.plan = (order, st, s_f, pst)
        ctx.mark_non_differentiable(moments, valid)
        return moments, a, q, valid

    @staticmethod
    def backward(ctx, _g_moments, g_a, g_q, _g_valid):
        x, y, oks, px, py, a, valid, factor = ctx.saved_tensors
        dev, shape = x.device, x.shape
        B, F, P, W = shape
        order, st, s_f, pst = ctx.plan
        J, _ = zfit_sizes(order)
        outs = _ray_grads(ctx, 2, x, st)
        if all(o is None for o in outs):
            return (None,) * 6
        ga = torch.empty((B, F, W, J), dtype=torch.float64, device=dev).copy_(g_a)
        gq = torch.empty((B, F, W), dtype=torch.float64, device=dev).copy_(g_q)
        coef = torch.empty((B, F, W, J + 1), dtype=torch.float64, device=dev)
        _call("tl_zfit_solve", dev, dev.index, B * F * W, order, None, ga, gq, a, None, valid, factor, coef, timed="tl_zfit_solve")
        _call("tl_zfit_seed", dev, dev.index, B * F, P, W, order, x, y, oks, s_f, st[2], st[3], px, py, *pst, coef, *outs,
              timed="tl_zfit_seed")
        return (*outs, None, None, None, None)


PSF_MAX_BINS = 32          # rows / columns of the half kernel tl_psf_accumulate takes (one 32x32 MFMA tile)


def _psf_float32(**tensors):
    """The device and dtype check of the fused PSF's tensor arguments, in the order given."""
    for name, ten in tensors.items():
        _require_device(ten, name)
        if ten.dtype != torch.float32:
            raise RuntimeError(f"torchoptics_amd: the fused PSF takes float32 tensors; `{name}` is {ten.dtype} "
                               "(there is no CPU fallback and no fp64 kernel: use fused=False)")


def _psf_rays(x, y, weight):
    """x, y [.., W, R] and the weights as tl_psf_accumulate and tl_psf_rot_accumulate take them: (x, y, wf, wb), rays
    contiguous and one set of strides for all.  A strided view of x goes through in place, an expanded one is copied; y and
    the weights are copied only where their strides differ from x's.  wf: float weights, wb: ok bytes, at most one of them."""
    dev = x.device
    if x.stride(2) != 1 or any(s == 0 for s in x.stride()[:2]):
        x = x.contiguous()
    if y.stride() != x.stride():
        y = torch.empty_strided(x.shape, x.stride(), dtype=torch.float32, device=dev).copy_(y)
    if weight is None:
        return x, y, None, None
    _require_device(weight, "weight")
    as_bytes = weight.dtype in (torch.bool, torch.uint8)
    if as_bytes:
        wt = weight.view(torch.uint8) if weight.dtype == torch.bool else weight
    else:
        wt = weight.detach().to(torch.float32)
    if wt.shape != x.shape:
        raise ValueError("the fused PSF: weights must have the shape of x")
    if wt.stride() != x.stride():
        wt = torch.empty_strided(x.shape, x.stride(), dtype=wt.dtype, device=dev).copy_(wt)
    return (x, y, None, wt) if as_bytes else (x, y, wt, None)


class PsfAccumulateFunction(torch.autograd.Function):
    """hist [G,W,ny,nxh] = sum_r wt_r Gy_i(r) Gx_j(r): the un-mirrored, un-normalised half kernel of the soft-histogram PSF
    (tl_psf_accumulate / tl_psf_accumulate_bwd; metrics.compute_psf(fused=True)).

    x, y [G,W,R] float32 on the GPU (rays contiguous; a [F,W,P] view of the tracer's outputs is taken as it is);
    weight: None, a float tensor (per-ray weights) or a bool / uint8 tensor (the tracer's ray_ok, passed as bytes), same
    shape; x_pitch, y_pitch, y_centre [G]; the pixel centres are x_pitch (x_first + j), y_centre + y_pitch (y_first + i).
    Differentiable in x, y, x_pitch, y_pitch and y_centre; the weights carry NO gradient."""

    @staticmethod
    def forward(ctx, x, y, weight, x_pitch, y_pitch, y_centre, nxh, ny, x_first, y_first):
        _psf_float32(x=x, y=y, x_pitch=x_pitch, y_pitch=y_pitch, y_centre=y_centre)
        if not (1 <= nxh <= PSF_MAX_BINS and 1 <= ny <= PSF_MAX_BINS):
            raise ValueError(f"the fused PSF takes 1..{PSF_MAX_BINS} bins per axis of the half kernel (got {ny} x {nxh})")
        dev = x.device
        G, W, R = x.shape
        x, y, wf, wb = _psf_rays(x, y, weight)
        xp, yp, yc = (a.detach().reshape(G).contiguous() for a in (x_pitch, y_pitch, y_centre))
        nbytes = _lib.lib().tl_psf_workspace_bytes(G, W, R, nxh, ny)
        ws = _workspace(nbytes, dev)
        hist = torch.empty((G, W, ny, nxh), dtype=torch.float32, device=dev)
        _call("tl_psf_accumulate", dev, dev.index, G, W, R, x, y, wf, wb, x.stride(0), x.stride(1), xp, yp, yc, nxh, ny,
              float(x_first), float(y_first), hist, ws, ws.numel())
        ctx.save_for_backward(x, y, wf, wb, xp, yp, yc)
        ctx.geom = (nxh, ny, float(x_first), float(y_first), nbytes)
        ctx.shapes = (x_pitch.shape, y_pitch.shape, y_centre.shape)
        return hist

    @staticmethod
    def backward(ctx, g_hist):
        x, y, wf, wb, xp, yp, yc = ctx.saved_tensors
        nxh, ny, x_first, y_first, nbytes = ctx.geom
        dev = x.device
        G, W, R = x.shape
        gh = g_hist.to(torch.float32).contiguous()
        gx = torch.empty_strided(x.shape, x.stride(), dtype=torch.float32, device=dev)
        gy = torch.empty_strided(x.shape, x.stride(), dtype=torch.float32, device=dev)
        need = ctx.needs_input_grad
        g_xp, g_yp, g_yc = (torch.empty(G, dtype=torch.float32, device=dev) if need[k] else None for k in (3, 4, 5))
        ws = _workspace(nbytes, dev)
        _call("tl_psf_accumulate_bwd", dev, dev.index, G, W, R, x, y, wf, wb, x.stride(0), x.stride(1), xp, yp, yc, nxh, ny,
              x_first, y_first, gh, gx, gy, g_xp, g_yp, g_yc, ws, ws.numel())
        g_xp, g_yp, g_yc = (g if g is None else g.reshape(s) for g, s in zip((g_xp, g_yp, g_yc), ctx.shapes))
        return (gx if need[0] else None, gy if need[1] else None, None, g_xp, g_yp, g_yc, None, None, None, None)


PSF_ROT_MAX_ROWS = 1 << 20          # G W and K W of tl_psf_rot_accumulate (include/tl_trace.h)


def psf_rot_grid(src, c, s, n_sources):
    """The host side of G rotated grids over K = n_sources fans, checked here because the kernels cannot: src [G] (the fan
    of every grid, 0 <= src < K), c, s [G] (cos and sin of its angle).  Returns a namespace of G, K, the arrays as the C ABI
    takes them (int32 / float32) and the CSR inverse of src -- field_grids[field_start[k] : field_start[k+1]] are the grids
    that read fan k, ascending -- with a cache of their device copies (uploaded once per device)."""
    src = np.asarray(src).reshape(-1)
    G, K = src.size, int(n_sources)
    if G < 1 or K < 1:
        raise ValueError(f"psf_rot_grid: at least one grid and one source fan are needed, got {G} and {K}")
    if not np.issubdtype(src.dtype, np.integer) or int(src.min()) < 0 or int(src.max()) >= K:
        raise ValueError(f"psf_rot_grid: src must hold integers in 0..{K - 1}")
    c, s = (np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(-1)) for a in (c, s))
    if c.size != G or s.size != G:
        raise ValueError(f"psf_rot_grid: c and s must hold {G} entries, one per grid")
    field_start = np.concatenate(([0], np.cumsum(np.bincount(src, minlength=K)))).astype(np.int32)
    field_grids = np.argsort(src, kind="stable").astype(np.int32)
    return SimpleNamespace(G=G, K=K, src=src.astype(np.int32), c=c, s=s, field_start=field_start, field_grids=field_grids,
                           device_tables={})


def _rot_tables(grid, dev):
    key = (dev.type, dev.index)
    if key not in grid.device_tables:
        grid.device_tables[key] = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in
                                        (grid.src, grid.c, grid.s, grid.field_start, grid.field_grids))
    return grid.device_tables[key]


class PsfRotAccumulateFunction(torch.autograd.Function):
    """hist [G,W,ny,nx] = sum_r wt_r Gy_i(r) Gx_j(r) of G full (un-mirrored) grids that each read one of K fans, rotated by
    the grid's (c, s) about the fan's centre (tl_psf_rot_accumulate / tl_psf_rot_accumulate_bwd;
    imaging.psf_grid_from_trace(fused=True)).

    x, y [K,W,R] float32 on the GPU, taken as PsfAccumulateFunction takes them; weight likewise; grid: psf_rot_grid(...);
    x_pitch, y_pitch: a float or a [G] tensor, explicit and WITHOUT gradient; y_centre [K], per source fan.  Differentiable
    in x, y (source coordinates: the sum over the grids that read the fan) and y_centre; the weights carry NO gradient."""

    @staticmethod
    def forward(ctx, x, y, weight, grid, x_pitch, y_pitch, y_centre, nx, ny, x_first, y_first):
        _psf_float32(x=x, y=y, y_centre=y_centre)
        if not (1 <= nx <= PSF_MAX_BINS and 1 <= ny <= PSF_MAX_BINS):
            raise ValueError(f"the fused PSF takes 1..{PSF_MAX_BINS} bins per axis (got {ny} x {nx})")
        dev = x.device
        K, W, R = x.shape
        G = grid.G
        if grid.K != K:
            raise ValueError(f"the fused PSF grid was laid out for {grid.K} source fans, x holds {K}")
        if G * W > PSF_ROT_MAX_ROWS or K * W > PSF_ROT_MAX_ROWS:
            raise ValueError(f"the fused PSF grid takes at most {PSF_ROT_MAX_ROWS} (grid, channel) rows, got {G} x {W}")
        x, y, wf, wb = _psf_rays(x, y, weight)
        pitch = lambda p: (p.detach().to(device=dev, dtype=torch.float32).reshape(G).contiguous() if torch.is_tensor(p)  # noqa: E731
                           else torch.full((G,), float(p), dtype=torch.float32, device=dev))
        xp, yp = pitch(x_pitch), pitch(y_pitch)
        yc = y_centre.detach().reshape(K).contiguous()
        src, c, s, fstart, fgrids = _rot_tables(grid, dev)
        nbytes = _lib.lib().tl_psf_rot_workspace_bytes(G, K, W, R, nx, ny)
        ws = _workspace(nbytes, dev)
        hist = torch.empty((G, W, ny, nx), dtype=torch.float32, device=dev)
        _call("tl_psf_rot_accumulate", dev, dev.index, G, K, W, R, x, y, wf, wb, x.stride(0), x.stride(1), src, c, s, xp, yp, yc,
              nx, ny, float(x_first), float(y_first), hist, ws, ws.numel())
        ctx.save_for_backward(x, y, wf, wb, xp, yp, yc)
        ctx.grid = grid
        ctx.geom = (nx, ny, float(x_first), float(y_first), nbytes)
        ctx.yc_shape = y_centre.shape
        return hist

    @staticmethod
    def backward(ctx, g_hist):
        x, y, wf, wb, xp, yp, yc = ctx.saved_tensors
        nx, ny, x_first, y_first, nbytes = ctx.geom
        dev = x.device
        K, W, R = x.shape
        src, c, s, fstart, fgrids = _rot_tables(ctx.grid, dev)
        gh = g_hist.to(torch.float32).contiguous()
        gx = torch.empty_strided(x.shape, x.stride(), dtype=torch.float32, device=dev)
        gy = torch.empty_strided(x.shape, x.stride(), dtype=torch.float32, device=dev)
        need = ctx.needs_input_grad
        g_yc = torch.empty(K, dtype=torch.float32, device=dev) if need[6] else None
        ws = _workspace(nbytes, dev)
        _call("tl_psf_rot_accumulate_bwd", dev, dev.index, ctx.grid.G, K, W, R, x, y, wf, wb, x.stride(0), x.stride(1), src, c, s,
              xp, yp, yc, nx, ny, x_first, y_first, fstart, fgrids, gh, gx, gy, g_yc, ws, ws.numel())
        return (gx if need[0] else None, gy if need[1] else None, None, None, None, None,
                None if g_yc is None else g_yc.reshape(ctx.yc_shape), None, None, None, None)


SVOLA_MAX_TAPS = 31       # rows / columns of a PSF the tl_svola_* kernels take (tile plus halo in LDS)
SVOLA_MAX_GRID = 128      # patches per axis

# C-ABI calls of SvolaFunction since import (tests: the image backward runs only when the image needs a gradient), and the
# psfs pointer the last forward handed to the kernel (a strided view goes through as it is: no copy)
_svola_calls = {"fwd": 0, "bwd_psf": 0, "bwd_image": 0, "psfs_ptr": None}


def svola_counts() -> dict:
    """{'fwd': n, 'bwd_psf': n, 'bwd_image': n, 'psfs_ptr': data pointer of the last forward's psfs}."""
    return dict(_svola_calls)


class SvolaFunction(torch.autograd.Function):
    """out [B,H,W,C] = the spatially varying overlap-add convolution of image [B,H,W,C] with psfs [B or 1,N,kh,kw,C]
    (tl_svola_fwd / tl_svola_bwd_psf / tl_svola_bwd_image; imaging.svola_convolution(fused=True), which checks the arguments).

    float32 on one GPU; both tensors are taken with the strides they have.  `geo` is imaging.svola_geometry(...): the patch
    bounds as host ints and the normalised per-axis window tables, uploaded once per device as doubles.  Differentiable in
    image and psfs; the image backward is launched only when the image needs a gradient."""

    @staticmethod
    def _geom(geo, image, psfs, g_psfs=None):
        B, H, W, Cc = image.shape
        q = _lib.tl_svola_geom(device=image.device.index, B=B, H=H, W=W, C=Cc, psf_batch=psfs.shape[0], gh=geo.gh, gw=geo.gw,
                               kh=psfs.shape[2], kw=psfs.shape[3], oh=geo.oh, ow=geo.ow)
        q.image_stride[:] = image.stride()
        q.psfs_stride[:] = psfs.stride()
        q.g_psfs_stride[:] = (g_psfs if g_psfs is not None else psfs).stride()
        return q

    @staticmethod
    def _tables(geo, dev):
        tabs = geo.device_tables.get(dev)
        if tabs is None:
            tabs = geo.device_tables[dev] = (torch.from_numpy(geo.tab_r).to(dev), torch.from_numpy(geo.tab_c).to(dev))
        return tabs

    @staticmethod
    def forward(ctx, image, psfs, geo):
        ctx.set_materialize_grads(False)
        dev = image.device
        wr, wc = SvolaFunction._tables(geo, dev)
        out = torch.empty(image.shape, dtype=torch.float32, device=dev)
        q = SvolaFunction._geom(geo, image, psfs)
        _call("tl_svola_fwd", dev, C.byref(q), *geo.bounds, wr, wc, image, psfs, out)
        _svola_calls["fwd"] += 1
        _svola_calls["psfs_ptr"] = psfs.data_ptr()
        ctx.save_for_backward(image, psfs)
        ctx.geo = geo
        return out

    @staticmethod
    def backward(ctx, g_out):
        need_image, need_psfs = ctx.needs_input_grad[:2]
        if g_out is None or not (need_image or need_psfs):
            return None, None, None
        image, psfs = ctx.saved_tensors
        geo, dev = ctx.geo, image.device
        wr, wc = SvolaFunction._tables(geo, dev)
        g_out = g_out.to(torch.float32).contiguous()
        g_image = g_psfs = None
        if need_psfs:
            g_psfs = torch.empty(psfs.shape, dtype=torch.float32, device=dev)
        q = SvolaFunction._geom(geo, image, psfs, g_psfs)
        nbytes = _lib.lib().tl_svola_workspace_bytes(C.byref(q), *geo.bounds)
        ws = _workspace(nbytes, dev)
        if need_psfs:
            _call("tl_svola_bwd_psf", dev, C.byref(q), *geo.bounds, wr, wc, image, g_out, g_psfs, ws, ws.numel())
            _svola_calls["bwd_psf"] += 1
        if need_image:
            g_image = torch.empty(image.shape, dtype=torch.float32, device=dev)
            _call("tl_svola_bwd_image", dev, C.byref(q), *geo.bounds, wr, wc, psfs, g_out, g_image, ws, ws.numel())
            _svola_calls["bwd_image"] += 1
        return g_image, g_psfs, None


# C-ABI calls of WarpFunction since import (tests: the backward runs only when a coordinate or the gain needs a gradient, the
# image backward only when the image does), and the pointers the last forward handed to the kernel (strided views go through
# as they are: no copy)
_warp_calls = {"fwd": 0, "bwd": 0, "bwd_image": 0, "image_ptr": None, "x_ptr": None, "y_ptr": None, "gain_ptr": None}
_WARP_IMAGE_PATHS = {"auto": 0, "direct": 1}      # tl_warp_bwd_image's flags
_warp_image_path = "auto"


def warp_counts() -> dict:
    """{'fwd': n, 'bwd': n, 'bwd_image': n, 'image_ptr', 'x_ptr', 'y_ptr', 'gain_ptr': data pointers of the last forward's
    arguments}."""
    return dict(_warp_calls)


def set_warp_image_grad_path(path: str) -> None:
    """How tl_warp_bwd_image adds up: 'auto' (default) privatises a box of the source image in LDS per tile of output pixels,
    'direct' sends every contribution to the global accumulator.  The same bits either way (64-bit integer sums); 'direct'
    is the A/B switch and the cross-check of the two paths."""
    global _warp_image_path
    if path not in _WARP_IMAGE_PATHS:
        raise ValueError(f"set_warp_image_grad_path: path must be one of {sorted(_WARP_IMAGE_PATHS)}, got {path!r}")
    _warp_image_path = path


class WarpFunction(torch.autograd.Function):
    """out [B,Ho,Wo,C] = gain x the bicubic resampling of image [B,H,W,C] at the normalised coordinates x, y [B or 1,Ho,Wo]
    (tl_warp_fwd / tl_warp_bwd / tl_warp_bwd_image; imaging.warp_bicubic(fused=True), which checks the arguments).  gain
    [B or 1,Ho,Wo,C or 1] or None.  An optional fifth argument, True, allows the gradient to the image.

    float32 on one GPU; every tensor is taken with the strides it has.  Differentiable in x, y and gain: one backward launch,
    and only when one of them needs a gradient.  The image gradient is a scatter in 64-bit fixed point (tl_warp_bwd_image:
    bit-reproducible, error absolute on the scale of the largest seed); it runs once, only when the image needs a gradient,
    and only when the fifth argument allowed it: otherwise asking for it raises."""

    @staticmethod
    def _geom(image, x, y, gain, g_x=None, g_y=None, g_gain=None):
        B, H, W, Cc = image.shape
        q = _lib.tl_warp_geom(device=image.device.index, B=B, H=H, W=W, C=Cc, Ho=x.shape[1], Wo=x.shape[2], coord_batch=x.shape[0],
                              gain_batch=1 if gain is None else gain.shape[0], gain_channels=1 if gain is None else gain.shape[3])
        q.image_stride[:] = image.stride()
        q.x_stride[:] = x.stride()
        q.y_stride[:] = y.stride()
        q.g_x_stride[:] = (g_x if g_x is not None else x).stride()
        q.g_y_stride[:] = (g_y if g_y is not None else y).stride()
        if gain is not None:
            q.gain_stride[:] = gain.stride()
            q.g_gain_stride[:] = (g_gain if g_gain is not None else gain).stride()
        return q

    @staticmethod
    def forward(ctx, image, x, y, gain, *allow_image_grad):
        ctx.set_materialize_grads(False)
        ctx.image_grad = bool(allow_image_grad and allow_image_grad[0])
        ctx.n_in = 4 + len(allow_image_grad)
        dev = image.device
        out = torch.empty((image.shape[0], x.shape[1], x.shape[2], image.shape[3]), dtype=torch.float32, device=dev)
        q = WarpFunction._geom(image, x, y, gain)
        _call("tl_warp_fwd", dev, C.byref(q), image, x, y, gain, out)
        _warp_calls["fwd"] += 1
        _warp_calls.update(image_ptr=image.data_ptr(), x_ptr=x.data_ptr(), y_ptr=y.data_ptr(),
                           gain_ptr=None if gain is None else gain.data_ptr())
        ctx.save_for_backward(image, x, y, gain)
        return out

    @staticmethod
    def backward(ctx, g_out):
        need_image, need_x, need_y, need_gain = ctx.needs_input_grad[:4]
        if need_image and not ctx.image_grad:
            raise RuntimeError("WarpFunction: the gradient to the image is a scatter and is not a kernel; use "
                               "imaging.warp_bicubic(fused=False) when the image needs a gradient")
        none = (None,) * (ctx.n_in - 4)
        if g_out is None or not (need_image or need_x or need_y or need_gain):
            return (None, None, None, None) + none
        image, x, y, gain = ctx.saved_tensors
        dev = image.device
        g_out = g_out.to(torch.float32).contiguous()
        g_image = g_x = g_y = g_gain = None
        if need_x or need_y or need_gain:
            if need_x or need_y:
                g_x = torch.empty(x.shape, dtype=torch.float32, device=dev)
                g_y = torch.empty(y.shape, dtype=torch.float32, device=dev)
            if need_gain:
                g_gain = torch.empty(gain.shape, dtype=torch.float32, device=dev)
            q = WarpFunction._geom(image, x, y, gain, g_x, g_y, g_gain)
            _call("tl_warp_bwd", dev, C.byref(q), image, x, y, gain, g_out, g_x, g_y, g_gain)
            _warp_calls["bwd"] += 1
        if need_image:
            g_image = torch.empty(image.shape, dtype=torch.float32, device=dev)
            q = WarpFunction._geom(image, x, y, gain)
            nbytes = _lib.lib().tl_warp_bwd_image_work_bytes(C.byref(q))
            ws = _workspace(nbytes, dev)
            _call("tl_warp_bwd_image", dev, C.byref(q), x, y, gain, g_out, g_image, ws, ws.numel(),
                  _WARP_IMAGE_PATHS[_warp_image_path])
            _warp_calls["bwd_image"] += 1
        return (g_image, g_x if need_x else None, g_y if need_y else None, g_gain) + none


SSIM_MAX_TAPS = 11        # the window of the tl_ssim_* kernels: odd, 3 .. 11 taps per axis
MS_SSIM_MAX_LEVELS = 8    # the levels of the tl_ms_ssim_* pyramid

# C-ABI calls of SsimFunction / of MsSsimFunction since import (tests: the backward runs once per image that needs a gradient;
# neither moves under the other function), and the pointers the last forward handed to the kernel (strided views go through
# as they are: no copy)
_ssim_calls = {"fwd": 0, "bwd": 0, "a_ptr": None, "b_ptr": None}
_ms_ssim_calls = dict(_ssim_calls)


def ssim_counts() -> dict:
    """{'fwd': n, 'bwd': n, 'a_ptr', 'b_ptr': data pointers of the last forward's images}."""
    return dict(_ssim_calls)


def ms_ssim_counts() -> dict:
    """{'fwd': n, 'bwd': n, 'a_ptr', 'b_ptr': data pointers of the last forward's images}."""
    return dict(_ms_ssim_calls)


def _ssim_geom(struct, a, b, window, c1, c2, flags, g, **more):
    """tl_ssim_geom or tl_ms_ssim_geom (`struct`; `more`: the members only the latter has) of a and b with the strides they
    have; g: the tensor the gradient is written to (a's strides without one)."""
    B, H, W, Cc = a.shape
    q = struct(device=a.device.index, B=B, H=H, W=W, C=Cc, K=len(window), C1=c1, C2=c2, flags=flags, **more)
    q.window[:len(window)] = window
    q.a_stride[:] = a.stride()
    q.b_stride[:] = b.stride()
    q.g_stride[:] = (g if g is not None else a).stride()
    return q


def _ssim_backward(fn, calls, ctx, g_value):
    """The backward of SsimFunction and MsSsimFunction (`fn`, counting in `calls`): per image that needs a gradient, with the
    roles and strides swapped (p the image, q_ the other one), fn._bwd(which, geometry, p, q_, kept, g_value, g_p) fills g_p
    from `kept`, what the forward saved after the images."""
    need_a, need_b = ctx.needs_input_grad[:2]
    rest = (None,) * (len(ctx.needs_input_grad) - 2)
    if g_value is None or not (need_a or need_b):
        return (None, None) + rest
    a, b, *kept = ctx.saved_tensors
    g_value = g_value.to(torch.float32).contiguous()
    grads = []
    for which, (need, p, q_) in enumerate(((need_a, a, b), (need_b, b, a))):
        if not need:
            grads.append(None)
            continue
        g_p = torch.empty(p.shape, dtype=torch.float32, device=a.device)
        fn._bwd(which, fn._geom(p, q_, *ctx.args, g=g_p), p, q_, kept, g_value, g_p)
        calls["bwd"] += 1
        grads.append(g_p)
    return (grads[0], grads[1]) + rest


class SsimFunction(torch.autograd.Function):
    """ssim [B] = the mean structural similarity of a and b [B,H,W,C] under the separable window `window` (K floats, odd K in
    3..11, already normalised) with the constants c1 = (k1 L)^2, c2 = (k2 L)^2 (tl_ssim_fwd / tl_ssim_bwd; imaging.ssim(fused=True),
    which checks the arguments).

    float32 on one GPU; both images are taken with the strides they have.  The forward stores the partial maps only of the
    images that need a gradient (4 bytes per map element each: three maps for one gradient, five for both, none without);
    the backward is one launch per image that needs a gradient."""

    @staticmethod
    def _geom(a, b, window, c1, c2, flags=0, g=None):
        return _ssim_geom(_lib.tl_ssim_geom, a, b, window, c1, c2, flags, g)

    @staticmethod
    def forward(ctx, a, b, window, c1, c2):
        ctx.set_materialize_grads(False)
        dev = a.device
        need_a, need_b = ctx.needs_input_grad[:2]
        q = SsimFunction._geom(a, b, window, c1, c2, flags=int(need_a) | 2 * int(need_b))
        n = _lib.lib().tl_ssim_maps_elems(C.byref(q))
        nbytes = _lib.lib().tl_ssim_work_bytes(C.byref(q))
        maps = [torch.empty(n, dtype=torch.float32, device=dev) if want else None
                for want in (need_a, need_a, need_b, need_b, need_a or need_b)]
        value = torch.empty(a.shape[0], dtype=torch.float32, device=dev)
        ws = _workspace(nbytes, dev)
        _call("tl_ssim_fwd", dev, C.byref(q), a, b, value, *maps, ws, ws.numel())
        _ssim_calls["fwd"] += 1
        _ssim_calls.update(a_ptr=a.data_ptr(), b_ptr=b.data_ptr())
        ctx.save_for_backward(a, b, *[m for m in maps if m is not None])
        ctx.args = (window, c1, c2)
        return value

    @staticmethod
    def _bwd(which, q, p, q_, kept, g_value, g_p):
        dm, ds = kept[-3:-1] if which else kept[:2]         # kept: (dm, ds) of a, then of b, as far as stored, then dc
        _call("tl_ssim_bwd", p.device, C.byref(q), p, q_, dm, ds, kept[-1], g_value, g_p)

    @staticmethod
    def backward(ctx, g_value):
        return _ssim_backward(SsimFunction, _ssim_calls, ctx, g_value)


class MsSsimFunction(torch.autograd.Function):
    """(ms_ssim [B], terms [B,C,M]) of a and b [B,H,W,C]: the multi-scale structural similarity over M = len(power) levels of
    2 x 2 mean pooling (tl_ms_ssim_fwd / tl_ms_ssim_bwd; imaging.ms_ssim(fused=True), which checks the arguments).  `terms`
    (cs of the levels below the top, ssim of the top one, per lens and channel) is a diagnostic and carries no gradient.

    float32 on one GPU; both images are taken with the strides they have.  One C-ABI call forward for the whole pyramid and
    one backward per image that needs a gradient; the forward allocates one workspace and one keep buffer (the pooled levels
    of both images and, per level, three partial maps for one gradient, four for both)."""

    @staticmethod
    def _geom(a, b, window, c1, c2, power, flags, g=None):
        q = _ssim_geom(_lib.tl_ms_ssim_geom, a, b, window, c1, c2, flags, g, levels=len(power))
        q.power[:len(power)] = power
        return q

    @staticmethod
    def forward(ctx, a, b, window, c1, c2, power):
        ctx.set_materialize_grads(False)
        dev = a.device
        need_a, need_b = ctx.needs_input_grad[:2]
        flags = int(need_a) | 2 * int(need_b)
        q = MsSsimFunction._geom(a, b, window, c1, c2, power, flags)
        keep = torch.empty(_lib.lib().tl_ms_ssim_keep_elems(C.byref(q)), dtype=torch.float32, device=dev)
        ws = _workspace(_lib.lib().tl_ms_ssim_work_bytes(C.byref(q)), dev)
        value = torch.empty(a.shape[0], dtype=torch.float32, device=dev)
        terms = torch.empty((a.shape[0], a.shape[3], len(power)), dtype=torch.float32, device=dev)
        _call("tl_ms_ssim_fwd", dev, C.byref(q), a, b, value, terms, keep, keep.numel(), ws, ws.numel())
        _ms_ssim_calls["fwd"] += 1
        _ms_ssim_calls.update(a_ptr=a.data_ptr(), b_ptr=b.data_ptr())
        ctx.save_for_backward(a, b, keep)
        ctx.args = (window, c1, c2, power, flags)
        ctx.mark_non_differentiable(terms)
        return value, terms

    @staticmethod
    def _bwd(which, q, p, q_, kept, g_value, g_p):
        keep, = kept
        ws = _workspace(_lib.lib().tl_ms_ssim_work_bytes(C.byref(q)), p.device)
        _call("tl_ms_ssim_bwd", p.device, C.byref(q), p, q_, keep, keep.numel(), g_value, g_p, which, ws, ws.numel())

    @staticmethod
    def backward(ctx, g_value, _g_terms):
        return _ssim_backward(MsSsimFunction, _ms_ssim_calls, ctx, g_value)


class PupilPositionFunction(torch.autograd.Function):
    """z [B] = paraxial entrance-pupil position from the rows in front of the stop: c, t [B,K], n [B,K+1]
    (tl_pupil_position: one tiny kernel forward, one backward, one thread per lens; mode 'strict': the value is the
    reference's fp32 product tree bit for bit, 'fast': fp64 inside, rounded once; default ops.get_default_mode())."""

    @staticmethod
    def forward(ctx, c, t, n, mode=None):
        ctx.mode = _MODES[mode or _default_mode]
        for name, ten in (("c", c), ("t", t), ("n", n)):
            _require_device(ten, name)
        B, K = c.shape
        c, t, n = (a.detach().to(torch.float32).contiguous() for a in (c, t, n))
        if t.shape != (B, K) or n.shape != (B, K + 1):
            raise ValueError("pupil position: c, t must hold [B,K] rows and n [B,K+1] indices")
        z = torch.empty(B, dtype=torch.float32, device=c.device)
        _call("tl_pupil_position", c.device, c.device.index, B, K, c, t, n, z, None, None, None, None, ctx.mode)
        ctx.save_for_backward(c, t, n)
        return z

    @staticmethod
    def backward(ctx, g_z):
        c, t, n = ctx.saved_tensors
        B, K = c.shape
        g_z = g_z.to(torch.float32).reshape(B).contiguous()
        g_c, g_t, g_n = torch.empty_like(c), torch.empty_like(t), torch.empty_like(n)
        _call("tl_pupil_position", c.device, c.device.index, B, K, c, t, n, None, g_z, g_c, g_t, g_n, ctx.mode)
        return g_c, g_t, g_n, None


# ------------------------------------------------------------------------------------------ entry points of the host chain
def _dist_initialized() -> bool:
    return torch.distributed.is_available() and torch.distributed.is_initialized()


def trace_cpp(ext, x, y, z, cx, cy, c, t, mu, mask, kappa, poly, kind, n_index, allow_back, mode, want_rays, want_opd,
              aggregate, want_stacks, moments_x):
    """The trace through the C++ host extension: the arguments exactly as trace_skew received them (their broadcast
    shapes are normalised in C++).  Returns (the nine outputs of TraceFunction, use_inv, the tl_bwd_route value of the
    backward: used_walk_back / backward_route)."""
    flags = ((ext.ALLOW_BACK if allow_back else 0) | (ext.WANT_RAYS if want_rays else 0) | (ext.WANT_OPD if want_opd else 0)
             | (ext.AGGREGATE if aggregate else 0) | (ext.WANT_STACKS if want_stacks else 0)
             | (ext.MOMENTS_X if moments_x else 0) | (ext.INVERSE if _bwd_algo == "inverse" else 0)
             # the spot metric of the traced rays as an output of the same node (ray_tracing.compute_rms2d picks it up);
             # not when the pupil is sharded over ranks: the moments are summed across them first
             # (nor with the penalty term: those callers take the whole loss_dict from the moments, unsup_loss below)
             | (ext.FUSE_RMS if (want_rays and not aggregate and hasattr(ext, "FUSE_RMS") and not _dist_initialized()) else 0))
    out = ext.trace(x, y, z, cx, cy, c, t, mu, mask, kappa, poly, kind, n_index, flags, _MODES[mode], ASPH_HIT_SLOTS)
    return out, ext.last_use_inv(), ext.last_route()


def pupil_position(c, t, n, mode=None):
    """PupilPositionFunction, through the C++ host extension when it is there."""
    ext = _ext()
    if ext is not None and c.is_cuda and hasattr(ext, "pupil_position"):
        return ext.pupil_position(c, t, n, _MODES[mode or _default_mode])
    return PupilPositionFunction.apply(c, t, n, mode)


def unsup_loss(moments, n_per_field, n_lens, n_sequence, penalty_rate):
    """(loss_unsup, rms, penalty) per lens from the moments of an aggregate trace in one launch (tl_unsup_loss), or None
    when the C++ host chain is not active (the callers then compose the same values from tensor ops)."""
    ext = _ext()
    if ext is None or not moments.is_cuda or not hasattr(ext, "unsup_loss"):
        return None
    if isinstance(n_sequence, (int, float)):
        return ext.unsup_loss(moments, float(n_per_field), int(n_lens), None, float(n_sequence), float(penalty_rate))
    return ext.unsup_loss(moments, float(n_per_field), int(n_lens), torch.as_tensor(n_sequence), 0.0, float(penalty_rate))


def spot_rms(moments, n_per_field, n_lens=1):
    """compute_rms2d on the moments (SpotRmsFunction), through the C++ host extension when it is there."""
    ext = _ext()
    if ext is not None and moments.is_cuda:
        return ext.spot_rms(moments, float(n_per_field), int(n_lens))
    return SpotRmsFunction.apply(moments, n_per_field, n_lens)
