"""
Image-quality metrics computed from a handful of traced rays: the step AFTER the hot path.

In the reference these exist only as commented-out TensorFlow code (ray_tracing_lite.py:848-934;
originals in ray_tracing.py:815-901) and are unreachable in its PyTorch port.  Written here from their
stated intent on top of RayTracer.trace_rays (i.e. the HIP kernels).  The reference cannot pin them; distortion,
relative illumination and the aiming error are held, values and leaf gradients, to the fp64 restatement of their
definitions in tests/metrics_ref.py (cases and gates: tests/metrics_cases.py, tests/test_gpu_metrics_matrix.py).
"""
from __future__ import annotations

import math
from typing import NamedTuple

import torch

from . import ops, paraxial
from .lens_modeling import const_tensor
from .ray_tracing import RayTracer, _root_of_variance, apply_vignetting


def compute_distortion(specs, lens, relative_fields, default_device="cuda"):
    """Relative distortion (y_chief - y_ref) / y_ref per field, d line.

    y_ref = EFL tan(field) corrected for the defocus of the image plane from the paraxial focus
    (last gap - BFL) along the traced chief-ray direction.  Field 0 gives 0/0 = NaN; pass fields > 0.

    Accuracy: d is a difference of two heights that agree to 1e-5 .. 1e-1 of their size, so its error is ABSOLUTE, whatever
    its value: measured 3.0e-7 at most from the fp64 restatement of this definition (tests/metrics_ref.py) in strict and
    in fast mode, over singlet, doublet, Cooke triplet, Tessar, an aspheric double Gauss and a padded batch at 10 .. 25
    degrees -- the fp32 evaluation of the same formulas on the CPU is 3.7e-7 off (profiles/metrics_accuracy.txt).  A
    distortion of 1e-5 therefore carries about two digits, one of 1e-2 five.  EFL, BFL and y_ref come from the fp32 ABCD
    product; nothing is gained by forming them in fp64 while y itself is an fp32 trace.
    """
    tr = RayTracer(mode='chief', n_rays=1, rel_fields=relative_fields, wavelengths=['d'], vig_fn=None,
                   default_device=default_device)
    # The chief ray's backward is the checkpoint kernel: with one ray per field the walk-back from the forward's outputs
    # saves nothing, and d's gradient is a small difference of the gradients of y and y_ref, which amplifies the rounding
    # of the walk-back's reconstructed states (strict mode, aspheric double Gauss: d/d poly 1.0e-5 rel-L2 from fp64 with
    # the walk-back, 1.9e-6 with the checkpoint kernel; the choice is made at the forward and kept by its node).
    algo = ops.get_backward_algorithm()
    ops.set_backward_algorithm("checkpoint")
    try:
        _, y, _, cy, *_ = tr.trace_rays(specs, lens)
    finally:
        ops.set_backward_algorithm(algo)
    n_lens = len(specs)
    y, cy = y.reshape(n_lens, -1), cy.reshape(n_lens, -1)
    fields = const_tensor([float(v) for v in relative_fields], y.dtype, y.device)        # cached: a captured step uploads nothing
    efl, bfl = paraxial.get_first_order(lens)
    ideal = torch.tan(fields[None, :] * specs.hfov[:, None]) * efl[:, None]
    rows = torch.arange(n_lens, device=y.device)
    last = lens.structure.mask_torch.sum(dim=1) - 1
    defocus = lens.t[rows, last] - bfl
    ref_y = ideal + defocus[:, None] * cy / torch.sqrt(1 - cy * cy)
    return (y - ref_y) / ref_y


def compute_relative_illumination(specs, lens, relative_fields, vig_fn=None, n_ray_aiming_iter=1,
                                  wavelengths=('d',), default_device="cuda"):
    """Relative illumination per field and wavelength from the image-space solid angle of three rays
    (upper / lower marginal and one sagittal ray; Rimmer, doi 10.1117/12.938414), normalised to the
    on-axis field (relative_fields[0] must be 0).  Fields with a failed ray report 1."""
    assert relative_fields[0] == 0., "the first field must be the axis"
    tr = RayTracer(mode='tee', rel_fields=relative_fields, vig_fn=vig_fn, n_ray_aiming_iter=n_ray_aiming_iter,
                   wavelengths=wavelengths, default_device=default_device)
    x = const_tensor([0., 0., 1.], torch.float32, default_device, (1, 1, 3, 1))      # cached: no upload per call
    y = const_tensor([1., -1., 0.], torch.float32, default_device, (1, 1, 3, 1))
    _, _, cx, cy, ray_ok, _ = tr.trace_rays(specs, lens, xy=(x, y))
    axis = torch.clamp(2 * cy[:, 0, 0, 0] ** 2, min=1e-6)
    ri = (cy[..., 0, :] - cy[..., 1, :]) * cx[..., 2, :] / axis[:, None, None]
    valid = ray_ok.all(dim=2)                                   # [lens, field, wavelength]
    valid = valid & valid[:, :1, :]
    return torch.where(valid, ri, torch.ones_like(ri))


def compute_ray_aiming_error(specs, lens, rel_fields, vig_fn=None, n_ray_aiming_iter=1, ray_aiming_mode='real',
                             default_device="cuda"):
    """Relative error, at the aperture stop, of the upper and lower meridional rays after ray aiming:
    y_stop / r_stop - y_pupil (0 for a lens whose stop is its first row)."""
    specs2, lens2 = specs.up_to_stop(), lens.up_to_stop()
    if (lens2.structure.stop_idx == 0).all():
        return 0
    if ray_aiming_mode == 'paraxial':
        rs = (paraxial.compute_magnification(lens2) * specs2.epd / 2).reshape(-1, 1, 1, 1)
    elif ray_aiming_mode == 'real':
        rs = paraxial.compute_pupil_radius(specs2, lens2, default_device=default_device).reshape(-1, 1, 1, 1)
    else:
        raise ValueError("ray_aiming_mode must be 'real' or 'paraxial'")
    y = const_tensor([-1., 1.], torch.float32, default_device, (1, 1, 2, 1))         # cached: no upload per call
    x = const_tensor([0., 0.], torch.float32, default_device, (1, 1, 2, 1))
    tr = RayTracer(mode='tee', rel_fields=rel_fields, vig_fn=vig_fn, wavelengths=['d'],
                   n_ray_aiming_iter=n_ray_aiming_iter, ray_aiming_mode=ray_aiming_mode, default_device=default_device)
    # the truncated lens ends at the stop: its "image plane" is the stop plane, and ray aiming (computed on
    # the same rows) is applied by trace_rays itself
    _, ys, *_ = tr.trace_rays(specs2, lens2, xy=(x, y), use_vig=True)
    if vig_fn is not None:
        fields = const_tensor([float(v) for v in rel_fields], torch.float32, default_device)[None, :]
        y = apply_vignetting(y, vig_fn(fields, specs.vig_up), vig_fn(fields, specs.vig_down))
    return ys / rs - y


def compute_psf(x, y, n_bins=(21, 21), increment=None, y_target=None, weights=None, y_extent="reference", fused=False):
    """Soft-histogram PSF of a ray fan on a per-field pixel grid (the reference's TensorFlow
    `compute_psf`, ray_tracing.py:206-270; unreachable in its PyTorch port, PARITY UNPINNED).

    x, y: [n_lens, n_fields, n_channels, n_rays] image-plane coordinates (`psf_from_trace` brings the
    tracer's [1,F,P,W] outputs into this layout).  One grid per (lens, field), centred at x = 0 and
    y = y_target (default: the mean y of the field); pixel size `increment`, or the fan's extent / n_bins.
    Every ray adds a Gaussian of sigma = half a pixel to each pixel centre; as in the reference only the
    x >= 0 half of the grid is evaluated and mirrored (the pupil is sampled symmetrically in x), and each
    channel's kernel is normalised to unit sum.
    `weights` (extension; same shape as x): per-ray weights, e.g. ray_ok as float to leave failed rays out.
    `y_extent` (increment=None only): "reference" (default) sizes the grid exactly as the reference text does --
    y_size = 2 max(y_max - y_target, y_target - y_min) with y_min, y_max taken AFTER y was centred on y_target
    (ray_tracing.py:220-231), i.e. y_target is subtracted twice (sic): for an off-axis field (y_target = 3 mm, spot
    +-0.06 mm) the grid spans 6.12 mm, not 0.12 mm, and the spot fills one pixel.  Kept because this function stands in
    for that text number for number; "centred" is the evident intent, y_size = 2 max(y_max, -y_min) of the centred y
    (a deviation from the reference, off by default; `psf_from_trace`, an extension, uses it).

    Returns (x_size, y_size, y_target, kernels [n_grids, n_channels, n_y_bins, n_x_bins],
    accounted_ray_proportion [n_grids]).

    The double sum over rays and pixels is a contraction over the ray index, so it is evaluated as one batched
    GEMM  G_y [ny, R] @ G_x^T [R, nx]  per (grid, channel) instead of the reference's [.., ny, nx, R] tensor.

    `fused=True` (opt-in; float32 tensors on the GPU only, at most 32 bins per axis): that GEMM and its two operands
    [g, w, bins, r] -- 128 B per ray at 21 x 21, kept by autograd -- are replaced by one HIP kernel that holds them in
    registers (ops.PsfAccumulateFunction: fp32 MFMA forward, per-ray backward; differentiable in x, y and through a grid
    sized from the data; `weights` carry no gradient there and may be bool / uint8: the tracer's ray_ok as it is).  The
    rest -- y_target, grid sizing, mirroring, normalisation, accounted_ray_proportion -- is the same code below.  The
    default (`fused=False`) is unchanged: any device, any float dtype.
    """
    nw, nr = x.shape[-2], x.shape[-1]
    n_grids = x.shape[0] * x.shape[1]
    n_x_bins, n_y_bins = n_bins
    if fused:
        if n_x_bins > ops.PSF_MAX_BINS or n_y_bins > ops.PSF_MAX_BINS:
            raise ValueError(f"compute_psf(fused=True) takes at most {ops.PSF_MAX_BINS} bins per axis, got {tuple(n_bins)}")
        if not (x.is_cuda and y.is_cuda) or x.dtype != torch.float32 or y.dtype != torch.float32:
            raise RuntimeError(f"compute_psf(fused=True): x is {x.dtype} on {x.device}; the fused PSF runs only as a HIP "
                               "kernel on float32 tensors on an AMD GPU (there is no CPU fallback): use fused=False")
    x = x.reshape(n_grids, nw, nr)
    y = y.reshape(n_grids, nw, nr)
    if y_target is None:
        y_target = y.reshape(n_grids, -1).mean(dim=1)
    y_rays = y                                          # the fused kernel centres y itself (y_target's gradient comes from it)
    y = y - y_target[:, None, None]
    if increment is not None:
        x_incr = y_incr = torch.ones(n_grids, dtype=x.dtype, device=x.device) * increment
        x_size = increment * n_x_bins
        y_size = increment * n_x_bins                  # (sic: the reference uses n_x_bins for both)
    else:
        flat_y = y.reshape(n_grids, -1)
        y_c_min, y_c_max = flat_y.min(dim=1).values, flat_y.max(dim=1).values      # y is centred already
        x_size = x.reshape(n_grids, -1).max(dim=1).values
        if y_extent == "reference":
            y_size = 2 * torch.maximum(y_c_max - y_target, y_target - y_c_min)     # (sic) ray_tracing.py:231
        elif y_extent == "centred":
            y_size = 2 * torch.maximum(y_c_max, -y_c_min)
        else:
            raise ValueError("y_extent must be 'reference' or 'centred'")
        x_incr = x_size / n_x_bins
        y_incr = y_size / n_y_bins
    if fused:
        # pixel centres x_incr (x_first + j), y_target + y_incr (y_first + i): the grids below, in pitch units
        nxh, x_first = (n_x_bins // 2 + 1, 0.0) if n_x_bins % 2 == 1 else (n_x_bins // 2, 0.5)
        wts = None if weights is None else weights.reshape(n_grids, nw, nr)
        pitch = lambda p: p.to(torch.float32) if torch.is_tensor(p) else torch.full((n_grids,), float(p), dtype=x.dtype, device=x.device)  # noqa: E731
        kernels = ops.PsfAccumulateFunction.apply(x, y_rays, wts, pitch(x_incr), pitch(y_incr), y_target.to(torch.float32),
                                                  nxh, n_y_bins, x_first, 0.5 - n_y_bins / 2)
        return _finish_psf(kernels, n_x_bins, x, y, x_size, y_size, y_target, n_grids)
    rng = lambda n: torch.arange(n, dtype=x.dtype, device=x.device)                 # noqa: E731
    if n_x_bins % 2 == 1:
        gx = rng(n_x_bins // 2 + 1)[None, :] * x_incr[:, None]
    else:
        gx = (rng(n_x_bins // 2) + 0.5)[None, :] * x_incr[:, None]
    gy = (rng(n_y_bins) + 0.5 - n_y_bins / 2)[None, :] * y_incr[:, None]
    sig_x, sig_y = (x_incr / 2)[:, None, None, None], (y_incr / 2)[:, None, None, None]
    g_x = torch.exp(-((x[:, :, None, :] - gx[:, None, :, None]) / sig_x) ** 2 / 2)   # [g, w, nx_half, r]
    g_y = torch.exp(-((y[:, :, None, :] - gy[:, None, :, None]) / sig_y) ** 2 / 2)   # [g, w, ny, r]
    if weights is not None:
        g_y = g_y * weights.reshape(n_grids, nw, 1, nr).to(g_y.dtype)
    kernels = torch.matmul(g_y, g_x.transpose(-1, -2))                               # [g, w, ny, nx_half]
    return _finish_psf(kernels, n_x_bins, x, y, x_size, y_size, y_target, n_grids)


def _finish_psf(kernels, n_x_bins, x, y, x_size, y_size, y_target, n_grids):
    """Mirror the half kernel [g, w, ny, nx_half] in x, normalise each channel, count the rays inside the grid (y centred)."""
    if n_x_bins % 2 == 1:
        kernels = torch.cat((torch.flip(kernels[..., 1:], dims=(-1,)), kernels), dim=-1)
    else:
        kernels = torch.cat((torch.flip(kernels, dims=(-1,)), kernels), dim=-1)
    kernels = kernels / kernels.sum(dim=(-1, -2), keepdim=True)
    xs = x_size if torch.is_tensor(x_size) else torch.full((n_grids,), float(x_size), dtype=x.dtype, device=x.device)
    ys = y_size if torch.is_tensor(y_size) else torch.full((n_grids,), float(y_size), dtype=x.dtype, device=x.device)
    accounted = (y.abs() < ys[:, None, None] / 2) & (x.abs() < xs[:, None, None] / 2)
    return x_size, y_size, y_target, kernels, accounted.to(x.dtype).mean(dim=(-1, -2))


def psf_from_trace(x, y, ray_ok=None, n_bins=(21, 21), increment=None, y_target=None, y_extent="centred", fused=False):
    """compute_psf on the outputs of RayTracer.trace_rays / trace_skew ([1, F, P, W]; their memory is already
    [F, W, P], so the permutation below is free).  With `ray_ok` failed rays are left out of the histogram and of
    the default y_target (the reference counts them as rays at the origin).  An extension with no counterpart in the
    reference: the automatic grid is sized on the centred spot (`y_extent="centred"`, see compute_psf).
    `fused=True`: compute_psf's HIP kernel; it reads x, y in the tracer's memory layout and ray_ok as its bytes (no float
    copy of the flags goes to the kernel; the weighted default y_target is computed as before)."""
    xt, yt = x.permute(0, 1, 3, 2), y.permute(0, 1, 3, 2)
    w = None
    if ray_ok is not None:
        w = ray_ok.permute(0, 1, 3, 2).to(y.dtype)
        if y_target is None:
            n_g = yt.shape[0] * yt.shape[1]
            y_target = (yt * w).reshape(n_g, -1).sum(dim=1) / w.reshape(n_g, -1).sum(dim=1).clamp_min(1)
    if fused and ray_ok is not None:
        w = ray_ok.permute(0, 1, 3, 2)
    return compute_psf(xt, yt, n_bins=n_bins, increment=increment, y_target=y_target, weights=w, y_extent=y_extent,
                       fused=fused)


# ---------------------------------------------------------------------------- through-focus spot moments
class ThroughFocus(NamedTuple):
    """What through_focus returns; every member is [B, F, W] less the pooled dimensions."""
    n: torch.Tensor                 # live rays
    rms: torch.Tensor               # RMS spot radius at the plane the rays were traced to
    best_focus: torch.Tensor        # shift of the image plane along +z that minimises it
    rms_best: torch.Tensor          # RMS spot radius there
    focus_t: torch.Tensor           # tangential focus: the shift that minimises the y extent
    focus_s: torch.Tensor           # sagittal focus: the shift that minimises the x extent
    a: torch.Tensor                 # R^2(d) = a + 2 b d + c d^2
    b: torch.Tensor
    c: torch.Tensor


FOCUS_SLOPE_FLOOR = 2.0 ** -40      # a centred slope sum at or below this share of its raw sum is rounding noise: no focus


def _uses_kernels(fused, tensors, n_float32, noun, where, what="tensors"):
    """Whether the fused path is taken: the `noun` kernels apply where every tensor sits on one AMD GPU and the first n_float32
    of them are float32; fused=True where they do not apply raises."""
    applies = (all(t.is_cuda and t.device == tensors[0].device for t in tensors)
               and all(t.dtype == torch.float32 for t in tensors[:n_float32]))
    if fused and not applies:
        raise RuntimeError(f"{where}(fused=True): x is {tensors[0].dtype} on {tensors[0].device}; the {noun} kernels run only "
                           f"on float32 {what} on one AMD GPU (there is no CPU fallback): use fused=False")
    return applies if fused is None else bool(fused)


def _rays_4d(where, *tensors):
    """The tensors broadcast against each other (under autograd); they must come out [B, F, P, W]."""
    tensors = torch.broadcast_tensors(*tensors)
    if tensors[0].dim() != 4:
        raise ValueError(f"{where} takes [B, F, P, W] tensors, got {tuple(tensors[0].shape)}")
    return tensors


def _focus_moments_torch(x, y, cx, cy, ray_ok):
    """The definition of focus_moments in torch ops, in float64."""
    x, y, cx, cy = (t.to(torch.float64) for t in (x, y, cx, cy))
    live = (ray_ok != 0) & (1 - cx * cx - cy * cy > 0)                # (NaN > 0 is false)
    zero = x.new_zeros(())
    # a dead ray is the ray (0, 0, 0, 0) that is not counted: nothing of what it holds reaches a sum or a gradient
    x, y, cx, cy = (torch.where(live, t, zero) for t in (x, y, cx, cy))
    cz = torch.sqrt(1 - cx * cx - cy * cy)
    u, v = cx / cz, cy / cz
    terms = (live.to(torch.float64), x, y, u, v, x * x, y * y, u * u, v * v, x * u, y * v)
    return torch.stack([t.sum(dim=2) for t in terms], dim=-1)


def focus_moments(x, y, cx, cy, ray_ok, fused=None):
    """The eleven through-focus moments M [B, F, W, 11] (float64) of a traced fan: per row (lens, field, wavelength)

        M[row, 0..10] = sum over the live rays of (1, x, y, u, v, x^2, y^2, u^2, v^2, x u, y v),   u = cx / cz, v = cy / cz.

    x, y, cx, cy, ray_ok: [B, F, P, W] as RayTracer.trace_rays returns them, broadcastable.  A ray is live iff ray_ok != 0 and
    s = 1 - cx^2 - cy^2 > 0; then cz = sqrt(s).  A dead ray adds exactly 0 to every moment and receives exactly 0 gradient,
    whatever its coordinates hold (NaN, +-inf, 1e30, cx^2 + cy^2 >= 1).  Differentiable in x, y, cx, cy.
    `fused`: False -- these sums in torch ops, upcast to float64, on any device and float dtype; True -- the HIP kernels
    (ops.FocusMomentsFunction: float32 tensors on one AMD GPU, anything else raises); None -- the kernels where they apply.
    Either way every product and sum is in float64: the raw second moment of y is ~4e5 times the variance taken from it."""
    use = _uses_kernels(fused, (x, y, cx, cy, ray_ok), 4, "focus", "focus_moments")
    x, y, cx, cy, ray_ok = _rays_4d("focus_moments", x, y, cx, cy, ray_ok)
    if use:
        return ops.FocusMomentsFunction.apply(x, y, cx, cy, ray_ok)
    return _focus_moments_torch(x, y, cx, cy, ray_ok)


def _quotient(num, den, raw):
    """num / den where den > 2^-40 raw, else 0 with zero gradient (the rule of _root_of_variance for a quotient)."""
    good = den > FOCUS_SLOPE_FLOOR * raw
    return torch.where(good, num / torch.where(good, den, torch.ones_like(den)), torch.zeros_like(den))


def through_focus_from_moments(M, common=("wavelength",), centroid="row", dtype=None):
    """The finish of through_focus on the moments M [B, F, W, 11] of focus_moments: plain torch in float64, differentiable."""
    common = tuple(common)
    if any(c not in ("field", "wavelength") for c in common):
        raise ValueError("common must be a subset of ('field', 'wavelength')")
    if centroid not in ("row", "field"):
        raise ValueError("centroid must be 'row' or 'field'")
    if centroid == "field" and "wavelength" not in common:
        raise ValueError("centroid='field' sums the moments over wavelengths first: 'wavelength' must be in common")
    dtype = dtype or M.dtype
    M = M.to(torch.float64)
    if centroid == "field":
        M = M.sum(dim=2, keepdim=True)
    n = M[..., 0]
    n1 = n.clamp(min=1.0)                       # (a row with n = 0 has M = 0: it adds nothing)

    def centred(q, s, qq, ss, qs):
        return (M[..., qq] - M[..., q] * M[..., q] / n1, M[..., qs] - M[..., q] * M[..., s] / n1,
                M[..., ss] - M[..., s] * M[..., s] / n1)
    Ax, Bx, Cx = centred(1, 3, 5, 7, 9)
    Ay, By, Cy = centred(2, 4, 6, 8, 10)
    raw_x, raw_y = M[..., 7], M[..., 8]
    dims = [d for d, name in ((1, "field"), (2, "wavelength")) if name in common]
    if dims:
        n, Ax, Ay, Bx, By, Cx, Cy, raw_x, raw_y = (t.sum(dim=dims) for t in (n, Ax, Ay, Bx, By, Cx, Cy, raw_x, raw_y))
    A, B, C = Ax + Ay, Bx + By, Cx + Cy
    n1 = n.clamp(min=1.0)
    q = _quotient(B, C, raw_x + raw_y)
    out = ThroughFocus(n=n, rms=_root_of_variance(A / n1), best_focus=-q, rms_best=_root_of_variance((A - B * q) / n1),
                       focus_t=-_quotient(By, Cy, raw_y), focus_s=-_quotient(Bx, Cx, raw_x), a=A / n1, b=B / n1, c=C / n1)
    return ThroughFocus(*(t.to(dtype) for t in out))


def through_focus(x, y, cx, cy, ray_ok, common=("wavelength",), centroid="row", fused=None):
    """Best focus, tangential / sagittal foci and the RMS spot radius through focus, from the rays as they stand.

    Behind the last surface a ray is a straight line: at an image plane shifted by d along +z (the sign of adding d to the
    last thickness) it lands at (x + d u, y + d v), u = cx / cz, v = cy / cz.  The mean square radius of a spot about its
    centroid is therefore a parabola R^2(d) = a + 2 b d + c d^2 whose coefficients are second moments of (x, y, u, v).

    x, y, cx, cy, ray_ok: [B, F, P, W] as RayTracer.trace_rays returns them, broadcastable.  A ROW is one (lens, field,
    wavelength); its eleven moments M (focus_moments; live rays only) give, for n = M0 > 0, the centred sums
        Ax = M5 - M1^2 / n,   Bx = M9 - M1 M3 / n,   Cx = M7 - M3^2 / n,      Ay, By, Cy likewise from columns 2, 4, 6, 8, 10.
    Rows are pooled over the dimensions named in `common` (a subset of ("field", "wavelength"), possibly empty) by adding
    n, Ax, Ay, Bx, By, Cx, Cy: ONE focal plane for the pooled rays, each row about its own centroid.  centroid="field" sums
    the raw M over wavelengths first -- one centroid per field, so lateral colour counts as spot size (needs "wavelength" in
    `common`).  Over a pooled set, with A = Ax + Ay, B = Bx + By, C = Cx + Cy:
        a = A / n, b = B / n, c = C / n          rms = sqrt(a)                    best_focus = -B / C
        rms_best = sqrt((A - B^2 / C) / n)       focus_t = -By / Cy               focus_s = -Bx / Cx
    Degenerate cases: the square root of a value <= 0 is 0 with zero gradient; a quotient whose denominator D (C, Cx, Cy) is
    <= 2^-40 times its raw second moment (M7 + M8, M7, M8) is 0 with zero gradient, and then rms_best = rms.  fp32 slopes
    carry relative errors of 2^-24, so a relative slope variance near 2^-48 is the inputs' rounding noise; 2^-40 is that with a
    margin of 256.  This covers n <= 1, a collimated bundle and a purely meridional fan (no sagittal focus).

    Returns ThroughFocus(n, rms, best_focus, rms_best, focus_t, focus_s, a, b, c), each [B, F, W] with the pooled dimensions
    removed, in the dtype of x; differentiable in x, y, cx, cy.  `fused`: as for focus_moments (the kernels form M; this
    finish is plain float64 torch on tiny tensors either way)."""
    M = focus_moments(x, y, cx, cy, ray_ok, fused=fused)
    return through_focus_from_moments(M, common, centroid, dtype=x.dtype)


# ---------------------------------------------------------------------------- encircled / ensquared energy
class EnclosedEnergy(NamedTuple):
    """What enclosed_energy returns."""
    n: torch.Tensor                 # live rays, [B, F, W] less the pooled dimensions
    energy: torch.Tensor            # share of them inside each radius, [..., K]
    centre: torch.Tensor            # the centre every row was measured about, [B, F, W, 2]


def _enclosed_edge(radii, softness, shape):
    """(radii, 1 / softness) as tuples of K Python floats, checked against the definition."""
    radii = tuple(float(r) for r in radii)
    soft = tuple(float(s) for s in softness) if isinstance(softness, (tuple, list)) else (float(softness),) * len(radii)
    if shape not in ops.ENCLOSED_SHAPES:
        raise ValueError("shape must be 'circle' or 'square'")
    if not radii or len(soft) != len(radii):
        raise ValueError("radii must hold at least one radius, softness one float or one per radius")
    inv = tuple(1.0 / s if s > 0 else 0.0 for s in soft)
    ok = all(0 < v < float("inf") for v in radii + soft + inv) and all(a < b for a, b in zip(radii, radii[1:]))
    if not ok:
        raise ValueError("radii must be finite, positive and strictly increasing, softness finite and positive")
    return radii, inv


def _enclosed_centre(S, centre):
    """[B, F, W, 2] float64: the centroid of every row ("row"), of every field's rows together ("field"), or the given tensor."""
    if isinstance(centre, str):
        if centre not in ("row", "field"):
            raise ValueError("centre must be 'row', 'field' or a tensor broadcastable to [B, F, W, 2]")
        return ops.EnclosedEnergyFunction._centre_of(S, centre)[0]
    return centre.to(torch.float64).expand(*S.shape[:3], 2)


def _enclosed_torch(x, y, ray_ok, radii, inv_soft, shape, centre):
    """The definition of enclosed_energy in torch ops, in float64, on any device: (S [B, F, W, 3], sums [B, F, W, K], centre
    [B, F, W, 2]).  It holds the ray x radius tensor the kernels never form."""
    x, y = x.to(torch.float64), y.to(torch.float64)
    live = ray_ok != 0
    zero = x.new_zeros(())
    # a dead ray is the ray at the origin that is not counted: nothing of what it holds reaches a sum or a gradient
    x, y = torch.where(live, x, zero), torch.where(live, y, zero)
    S = torch.stack([live.to(torch.float64).sum(dim=2), x.sum(dim=2), y.sum(dim=2)], dim=-1)
    c = _enclosed_centre(S, centre)
    dx, dy = x - c[:, :, None, :, 0], y - c[:, :, None, :, 1]
    R, inv = const_tensor(radii, torch.float64, x.device), const_tensor(inv_soft, torch.float64, x.device)   # cached: no upload per call

    def sigma(a):                                           # a [B, F, P, W] -> [B, F, P, W, K]
        t = (((R - a[..., None]) * inv + 1.0) * 0.5).clamp(0.0, 1.0)
        return t * t * (3.0 - 2.0 * t)
    if shape == "circle":
        r2 = dx * dx + dy * dy
        some = r2 > 0                                       # (the root has no gradient at 0: the definition says 0 there)
        e = sigma(torch.where(some, torch.sqrt(torch.where(some, r2, torch.ones_like(r2))), zero))
    else:
        e = sigma(dx.abs()) * sigma(dy.abs())
    sums = torch.where(live[..., None], e, zero).sum(dim=2)
    return S, sums, c


def enclosed_energy(x, y, ray_ok, radii, softness, shape="circle", common=("wavelength",), centre="row", fused=None):
    """Encircled (shape="circle") or ensquared ("square") energy of a traced fan: the share of the live rays inside a circle
    of radius R_k, or a square of half side R_k, about a centre, under a smooth edge of half width `softness`.

    x, y, ray_ok: [B, F, P, W] as RayTracer.trace_rays returns them, broadcastable.  A ROW is one (lens, field, wavelength); a
    ray is LIVE iff ray_ok != 0.  A dead ray adds exactly 0 to every sum and receives exactly 0 gradient, whatever its
    coordinates hold (NaN, +-inf, 1e30); live rays must be finite.  Per row S = (n, sum x, sum y) over the live rays.
    `centre`: "row" -- (sum x / n, sum y / n) of the row, 0 for an empty row; "field" -- S summed over the wavelengths first:
    one polychromatic centroid per field, so lateral colour counts as spread; or a tensor broadcastable to [B, F, W, 2] (the
    chief ray, an ideal image point), differentiable.
    The edge is sigma(u) = 0 for u <= -1, 1 for u >= 1, else t^2 (3 - 2 t) with t = (u + 1) / 2, so sigma'(u) = 3 t (1 - t)
    inside the band: C1, of compact support (a ray farther than the softness from the edge counts exactly 0 or 1), a
    polynomial.  It is part of the definition: a hard count has zero gradient everywhere.  With dx = x - c_x, dy = y - c_y,
    radii R_1 < ... < R_K (Python floats > 0) and softness tau_k > 0 (one float, or K of them),
        circle   e_ik = sigma((R_k - rho_i) / tau_k),   rho_i = sqrt(dx^2 + dy^2)
        square   e_ik = sigma((R_k - |dx_i|) / tau_k) sigma((R_k - |dy_i|) / tau_k)
    (the quotient formed as a product with 1 / tau_k), sums[row, k] = sum over live rays of e_ik, and energy = pooled sums /
    pooled n: `common`, a subset of ("field", "wavelength"), adds sums and n over the named dimensions before the division, as
    through_focus does; a pooled set with n = 0 gives energy 0 with zero gradient.
    Gradients: circle d e_ik / dx_i = -sigma'(u) / tau_k dx / rho (0 at rho = 0); square -sigma'(u_x) sigma(u_y) / tau_k sgn(dx)
    with sgn(0) = 0; y likewise; d / dc = -sum_i d / dx_i; through an internal centroid dc_x / dx_i = 1 / n on live rays.  Radii
    and softness are host numbers, not differentiable.

    Returns EnclosedEnergy(n, energy [..., K], centre [B, F, W, 2]) in the dtype of x.  `fused`: False -- the definition in
    torch ops in float64 on any device (it holds a ray x radius tensor several times over); True -- the HIP kernels
    (ops.EnclosedEnergyFunction: float32 x, y on one AMD GPU, anything else raises; at most 32 radii per launch, longer lists
    go in several); None -- the kernels where they apply.  Either way every difference, product, root and sum is in float64."""
    common = tuple(common)
    if any(c not in ("field", "wavelength") for c in common):
        raise ValueError("common must be a subset of ('field', 'wavelength')")
    radii, inv = _enclosed_edge(radii, softness, shape)
    tensors = (x, y, ray_ok) + (() if isinstance(centre, str) else (centre,))
    use = _uses_kernels(fused, tensors, 2, "enclosed-energy", "enclosed_energy")
    x, y, ray_ok = _rays_4d("enclosed_energy", x, y, ray_ok)
    if isinstance(centre, str) and centre not in ("row", "field"):
        raise ValueError("centre must be 'row', 'field' or a tensor broadcastable to [B, F, W, 2]")
    if use:
        parts = []
        for k in range(0, len(radii), ops.ENCLOSED_MAX_K):
            S, sums = ops.EnclosedEnergyFunction.apply(x, y, ray_ok, centre, radii[k:k + ops.ENCLOSED_MAX_K],
                                                       inv[k:k + ops.ENCLOSED_MAX_K], shape)
            parts.append(sums)
        sums = parts[0] if len(parts) == 1 else torch.cat(parts, dim=-1)
        c = _enclosed_centre(S, centre)
    else:
        S, sums, c = _enclosed_torch(x, y, ray_ok, radii, inv, shape, centre)
    n = S[..., 0]
    dims = [d for d, name in ((1, "field"), (2, "wavelength")) if name in common]
    if dims:
        n, sums = n.sum(dim=dims), sums.sum(dim=dims)
    energy = sums / n.clamp(min=1.0)[..., None]             # (n = 0: the sums are 0 and depend on nothing)
    return EnclosedEnergy(n.detach().to(x.dtype), energy.to(x.dtype), c.to(x.dtype))        # (a count carries no gradient)


def enclosed_radius(energy, radii, fraction):
    """The radius that holds `fraction` of the energy, on the piecewise-linear curve through (0, 0), (R_1, E_1), ..., (R_K, E_K):
    at the first k with E_k >= fraction,  R_{k-1} + (fraction - E_{k-1}) / (E_k - E_{k-1}) (R_k - R_{k-1}).

    energy: [..., K] (enclosed_energy's); radii: the K Python floats it was computed at.  Returns (radius, reached), both of
    energy's shape less its last dimension: float64 torch on tiny tensors, differentiable through E.  Where the curve never
    reaches `fraction` the radius is R_K with zero gradient and reached is False.  No host synchronisation."""
    radii = tuple(float(r) for r in radii)
    K = len(radii)
    if energy.shape[-1] != K:
        raise ValueError(f"energy holds {energy.shape[-1]} radii, {K} were given")
    E = energy.to(torch.float64)
    R0 = const_tensor((0.0,) + radii, torch.float64, E.device)
    E0 = torch.cat((torch.zeros_like(E[..., :1]), E), dim=-1)
    hit = E >= fraction
    reached = hit.any(dim=-1)
    k = (torch.cumsum(hit.to(torch.int64), dim=-1) == 0).sum(dim=-1).clamp(max=K - 1)      # the first hit (K - 1 where none)
    lo, hi = torch.gather(E0, -1, k[..., None])[..., 0], torch.gather(E0, -1, k[..., None] + 1)[..., 0]
    r_lo, r_hi = R0[k], R0[k + 1]
    good = reached & (hi > lo)
    at = r_lo + (fraction - lo) / torch.where(good, hi - lo, torch.ones_like(hi)) * (r_hi - r_lo)
    return torch.where(good, at, torch.where(reached, r_lo, r_hi)), reached


def spot_centroid(x, y, ray_ok, fused=None):
    """(n [B, F, W], centroid [B, F, W, 2]) of the live rays of every row (lens, field, wavelength), in the dtype of x: the
    per-wavelength centroids are the lateral colour through_focus does not give.  An empty row gets centroid 0.  Sums in
    float64; differentiable in x, y; `fused` as for enclosed_energy (tl_enclosed_centroid forward, tl_enclosed_seed backward)."""
    use = _uses_kernels(fused, (x, y, ray_ok), 2, "enclosed-energy", "spot_centroid")
    x, y, ray_ok = _rays_4d("spot_centroid", x, y, ray_ok)
    if use:
        S, _ = ops.EnclosedEnergyFunction.apply(x, y, ray_ok, "row", (), (), "circle")
    else:
        live = ray_ok != 0
        x64, y64 = (torch.where(live, t.to(torch.float64), t.new_zeros((), dtype=torch.float64)) for t in (x, y))
        S = torch.stack([live.to(torch.float64).sum(dim=2), x64.sum(dim=2), y64.sum(dim=2)], dim=-1)
    return S[..., 0].detach().to(x.dtype), _enclosed_centre(S, "row").to(x.dtype)


# ---------------------------------------------------------------------------- Zernike wavefront fit from the ray errors
class ZernikeFit(NamedTuple):
    """What zernike_fit returns; every member is [B, F, W], coeffs [B, F, W, J]."""
    n: torch.Tensor                 # live rays
    valid: torch.Tensor             # bool: the row's fit is determined (the validity rule)
    coeffs: torch.Tensor            # scale a_j for Z_2 .. Z_{J+1} (Noll): coeffs[..., j - 2]
    rms: torch.Tensor               # sqrt(sum_{j >= 4} coeffs_j^2): RMS wavefront error, tilt removed
    rms_focus: torch.Tensor         # sqrt(sum_{j >= 5} coeffs_j^2): tilt and defocus removed
    residual: torch.Tensor          # the transverse RMS ray error the polynomial does not explain


class ZernikeBasis(NamedTuple):
    """What zernike_basis returns."""
    T: torch.Tensor                 # [J, J] float64: Z_{j+2}(p, q) = sum_m T[m, j] p^a_m q^b_m (+ a constant the fit never sees)
    exponents: tuple                # ((a_m, b_m), ...): the monomials of degree 1 .. N, by degree, b ascending
    noll: tuple                     # ((j, n, m), ...): Noll index, radial order, azimuthal frequency (m < 0: the sine term)


ZFIT_PIVOT_FLOOR = 2.0 ** -30       # a pivot of the scaled normal equations at or below this: the row's fit is not determined
_ZBASIS = {}


def zernike_basis(max_order):
    """The Noll-indexed Zernike polynomials Z_2 .. Z_{J+1} of radial order <= max_order in {2, .., 6}, J = (N+1)(N+2)/2 - 1,
    orthonormal over the unit disc (their mean square is 1), with p = rho cos(theta) along x and q = rho sin(theta) along y:
    Z_j = N_nm R_n^m(rho) cos(m theta) for even j, sin for odd j, N_n0 = sqrt(n + 1), N_nm = sqrt(2 (n + 1)); so Z2 = 2 p,
    Z3 = 2 q, Z4 = sqrt(3) (2 rho^2 - 1), Z11 = sqrt(5) (6 rho^4 - 6 rho^2 + 1).  Returns ZernikeBasis(T, exponents, noll): the
    monomial coefficients from the closed form (a host tensor; the constant terms, which have no gradient, are left out)."""
    from math import comb, factorial, sqrt
    J, _ = ops.zfit_sizes(max_order)
    if max_order not in _ZBASIS:
        expo = tuple((d - b, b) for d in range(1, max_order + 1) for b in range(d + 1))
        at = {e: i for i, e in enumerate(expo)}
        T = torch.zeros((J, J), dtype=torch.float64)
        noll = []
        for j in range(2, J + 2):
            n = 0
            while (n + 1) * (n + 2) // 2 < j:
                n += 1
            k = j - n * (n + 1) // 2
            m = 2 * (k // 2) if n % 2 == 0 else 2 * ((k - 1) // 2) + 1
            sine = m != 0 and j % 2 == 1
            noll.append((j, n, -m if sine else m))
            norm = sqrt(n + 1) if m == 0 else sqrt(2 * (n + 1))
            for s in range((n - m) // 2 + 1):
                rc = (-1) ** s * factorial(n - s) // (factorial(s) * factorial((n + m) // 2 - s) * factorial((n - m) // 2 - s))
                t = (n - m) // 2 - s            # rho^(m + 2 t) cos / sin (m theta) = (p^2 + q^2)^t Re / Im (p + i q)^m
                for u in range(t + 1):
                    for h in range(1 if sine else 0, m + 1, 2):
                        e = (2 * (t - u) + m - h, 2 * u + h)
                        if e != (0, 0):
                            T[at[e], j - 2] += norm * rc * comb(t, u) * comb(m, h) * (-1) ** (h // 2)
        _ZBASIS[max_order] = ZernikeBasis(T, expo, tuple(noll))
    return _ZBASIS[max_order]


def _zfit_powers(p, q, top):
    """p^k, q^k for k = 0 .. top as lists: p^0 = 1, p^k = p^(k-1) p."""
    pp, qq = [torch.ones_like(p)], [torch.ones_like(q)]
    for _ in range(top):
        pp.append(pp[-1] * p)
        qq.append(qq[-1] * q)
    return pp, qq


def _zfit_live(x, y, ray_ok, px, py):
    """The rays in float64 with the dead ones at the origin of the spot and of the pupil, and the live mask."""
    live = ray_ok != 0
    zero = x.new_zeros((), dtype=torch.float64)
    return tuple(torch.where(live, t.to(torch.float64), zero) for t in (x, y, px, py)) + (live,)


def _zernike_moments_torch(x, y, ray_ok, px, py, order):
    x, y, p, q, live = _zfit_live(x, y, ray_ok, px, py)
    pp, qq = _zfit_powers(p, q, 2 * order - 2)
    mono = lambda top: [(d - b, b) for d in range(top + 1) for b in range(d + 1)]                       # noqa: E731
    terms = [live.to(torch.float64) if (a, b) == (0, 0) else pp[a] * qq[b] for a, b in mono(2 * order - 2)]
    terms += [(pp[a] * qq[b]) * x for a, b in mono(order - 1)] + [(pp[a] * qq[b]) * y for a, b in mono(order - 1)] + [x * x, y * y]
    return torch.stack([t.sum(dim=2) for t in terms], dim=-1)


def zernike_moments(x, y, ray_ok, px, py, max_order=4, fused=None):
    """The K = 3 N^2 + 2 monomial sums [B, F, W, K] (float64) the Zernike fit of order N = max_order is formed from: per row,
    over the live rays (ray_ok != 0), with tri(a, b) = (a + b)(a + b + 1) / 2 + b,
        M[tri(a, b)] = sum p^a q^b (a + b <= 2N - 2; M[0] = n),   then sum x p^a q^b and sum y p^a q^b (a + b <= N - 1, each by tri),
        then sum x^2, sum y^2,
    p^0 = 1, p^k = p^(k-1) p, a term (p^a q^b) and then times x, all in float64.  A dead ray adds exactly 0 whatever it holds.
    An intermediate: it carries no gradient (zernike_fit does).  `fused` as for zernike_fit."""
    ops.zfit_sizes(max_order)
    use = _uses_kernels(fused, (x, y, ray_ok, px, py), 2, "Zernike-fit", "zernike_moments", "rays")
    x, y, ray_ok, px, py = _rays_4d("zernike_moments", x, y, ray_ok, px, py)
    if use:
        return ops.ZernikeFitFunction.apply(x, y, ray_ok, px, py, max_order)[0]
    return _zernike_moments_torch(x, y, ray_ok, px, py, max_order).detach()


def _zernike_fit_torch(x, y, ray_ok, px, py, order):
    """The definition of zernike_fit in torch ops, in float64, design-matrix form: (n, a, q, valid)."""
    basis = zernike_basis(order)
    J = len(basis.noll)
    x, y, p, q, live = _zfit_live(x, y, ray_ok, px, py)
    pp, qq = _zfit_powers(p, q, order)
    zero = torch.zeros_like(p)
    dp = torch.stack([a * pp[a - 1] * qq[b] if a else zero for a, b in basis.exponents], dim=-1)       # [B,F,P,W,J] monomials
    dq = torch.stack([b * pp[a] * qq[b - 1] if b else zero for a, b in basis.exponents], dim=-1)
    T = const_tensor(basis.T.tolist(), torch.float64, x.device)
    lv = live[..., None]
    # [B,F,W,P,J]: dZ_j/dp, dZ_j/dq (the pupil has no gradient)
    Ap = torch.where(lv, dp @ T, zero[..., None]).permute(0, 1, 3, 2, 4).detach()
    Aq = torch.where(lv, dq @ T, zero[..., None]).permute(0, 1, 3, 2, 4).detach()
    xr, yr = x.permute(0, 1, 3, 2)[..., None], y.permute(0, 1, 3, 2)[..., None]                       # [B,F,W,P,1]
    G = Ap.transpose(-1, -2) @ Ap + Aq.transpose(-1, -2) @ Aq
    b = (Ap.transpose(-1, -2) @ xr + Aq.transpose(-1, -2) @ yr)[..., 0]                                # [B,F,W,J]
    n = live.to(torch.float64).sum(dim=2)
    D = torch.diagonal(G, dim1=-2, dim2=-1)
    pos = (D > 0).all(dim=-1) & (2 * n >= J)
    isd = torch.where(pos[..., None], D.clamp(min=1e-300).rsqrt(), torch.ones_like(D))
    eye = torch.eye(J, dtype=torch.float64, device=x.device)
    Gs = torch.where(pos[..., None, None], G * isd[..., :, None] * isd[..., None, :], eye)
    L, info = torch.linalg.cholesky_ex(Gs)
    piv = torch.diagonal(L, dim1=-2, dim2=-1) ** 2
    valid = pos & (info == 0) & (piv > ZFIT_PIVOT_FLOOR).all(dim=-1)                                   # (NaN > floor is false)
    L = torch.where(valid[..., None, None], L, eye)
    a = torch.cholesky_solve((b * isd)[..., None], L)[..., 0] * isd
    a = torch.where(valid[..., None], a, torch.zeros_like(a))
    qsum = (x * x + y * y).sum(dim=2) - (b * a).sum(dim=-1)
    return n, a, torch.where(valid, qsum, torch.zeros_like(qsum)), valid


def zernike_fit(x, y, ray_ok, px, py, max_order=4, scale=None, fused=None):
    """Zernike coefficients of the wavefront, and its RMS error, from the transverse ray errors of a traced fan.

    The transverse ray error is the gradient of the wavefront over the pupil, so the coefficients follow from a linear
    least-squares fit of the spot (x, y) against the gradients of the Zernike polynomials at each ray's pupil coordinates --
    the modal reconstruction of a Shack-Hartmann sensor.  It needs no optical path length: its inputs are x, y, ray_ok, which
    every trace gives at full accuracy, in either precision.

    x, y, ray_ok: [B, F, P, W] as RayTracer.trace_rays returns them; px, py: the rays' pupil coordinates relative to the pupil
    radius (RayTracer.pupil_coordinates), broadcastable -- [1, 1, P, 1] for one shared pupil, which is not copied.  The
    caller's coordinates define the unit disc.  N = max_order in {2, 3, 4, 5, 6}, J = (N+1)(N+2)/2 - 1 = 5, 9, 14, 20, 27; Z_j,
    j = 2 .. J+1, are the Noll-indexed polynomials of zernike_basis(N), orthonormal over the unit disc, p along x, q along y.
    A ROW is one (lens, field, wavelength).  A ray is live iff ray_ok != 0; a dead ray adds exactly 0 to every sum and receives
    exactly 0 gradient, whatever x, y, px, py hold at it (NaN, +-inf, 1e30).  Per row, over the live rays, minimise over a
        sum_i (x_i - sum_j a_j dZ_j/dp(p_i, q_i))^2 + (y_i - sum_j a_j dZ_j/dq(p_i, q_i))^2:
    the tilt terms have constant gradients, so they absorb the centroid and no separate centring is needed.  The normal
    equations are G a = b with G_jk = sum_i grad Z_j . grad Z_k and b_j = sum_i (x_i dZ_j/dp + y_i dZ_j/dq).  Outputs:
        coeffs    = scale a, [B, F, W, J]; `scale` broadcastable to [B, F, W], default 1; for an object at infinity
                    epd / (2 efl) / lambda gives waves (x, y and lambda in the same unit).  Applied in torch, differentiable.
        rms       = sqrt(sum_{j >= 4} coeffs_j^2): tilt removed;   rms_focus = sqrt(sum_{j >= 5} coeffs_j^2): and defocus
        residual  = sqrt(max(sum (x^2 + y^2) - b . a, 0) / n): the transverse RMS the polynomial does not explain
        n         the live-ray count;   valid   the flag below.
    The root of a value <= 0 is 0 with zero gradient.
    VALIDITY.  With D = diag(G) and G^ = D^-1/2 G D^-1/2, a row is valid iff 2 n >= J (fewer equations than
    unknowns leave G singular in exact arithmetic; rounding must not decide that), every D_jj > 0 and every pivot of the
    Cholesky factorisation of G^ (natural order, no pivoting; the pivot is the value whose root is the factor's diagonal)
    exceeds ZFIT_PIVOT_FLOOR = 2^-30.  That leaves float64 23 bits in the coefficients, the precision of the inputs; a full
    disc's smallest pivot is ~1/130 at order 6.  An invalid row (one ray, fewer than J / 2 rays, a meridional-only fan)
    returns 0 everywhere with zero gradients and valid = False.
    SIGN.  W = +scale a agrees with the oracle's optical path length (held by a test).  The relation between slope and
    wavefront is first order in the pupil's aberration: off axis the coefficients differ from a fit of the optical path
    difference by a few per cent (README).  Gradients flow to x, y and scale; px, py and ray_ok get none.

    Returns ZernikeFit(n, valid, coeffs, rms, rms_focus, residual) in the dtype of x (valid bool).  `fused`: False -- this
    definition in float64 torch ops on any device and dtype (it holds the rays x J design matrix); True -- the HIP kernels
    (ops.ZernikeFitFunction: float32 x, y on one AMD GPU, anything else raises), which form G and b from K = 3 N^2 + 2
    monomial sums per row; None -- the kernels where they apply.  Either way every product and sum is in float64."""
    ops.zfit_sizes(max_order)
    tensors = (x, y, ray_ok, px, py) + ((scale,) if torch.is_tensor(scale) else ())
    use = _uses_kernels(fused, tensors, 2, "Zernike-fit", "zernike_fit", "rays")
    x, y, ray_ok, px, py = _rays_4d("zernike_fit", x, y, ray_ok, px, py)
    if use:
        M, a, q, valid = ops.ZernikeFitFunction.apply(x, y, ray_ok, px, py, max_order)
        n, valid = M[..., 0], valid != 0
    else:
        n, a, q, valid = _zernike_fit_torch(x, y, ray_ok, px, py, max_order)
    if scale is None:
        coeffs = a
    elif torch.is_tensor(scale):
        coeffs = a * scale.to(torch.float64)[..., None]
    else:
        coeffs = a * float(scale)
    sq = coeffs * coeffs
    out = ZernikeFit(n=n.detach(), valid=valid, coeffs=coeffs, rms=_root_of_variance(sq[..., 2:].sum(dim=-1)),
                     rms_focus=_root_of_variance(sq[..., 3:].sum(dim=-1)), residual=_root_of_variance(q / n.detach().clamp(min=1.0)))
    return ZernikeFit(*(t if t.dtype == torch.bool else t.to(x.dtype) for t in out))


# ---------------------------------------------------------------------------- geometric MTF: Fourier sums over the spot
class GeometricMTF(NamedTuple):
    """What geometric_mtf returns."""
    n: torch.Tensor                 # weighted live rays, [B, F, W] less the pooled dimension
    mtf: torch.Tensor               # modulus of the geometric OTF, [..., D, K]: directions x frequencies
    centre: torch.Tensor            # the origin every row's phase was measured from, [B, F, W, 2]


def _mtf_vectors(frequencies, directions):
    """(nu_x, nu_y, D, K): the D K frequency vectors as Python floats, direction-major, formed on the host in float64."""
    freqs = tuple(float(f) for f in frequencies)
    if not freqs or not all(0.0 <= f < float("inf") for f in freqs):
        raise ValueError("frequencies must hold at least one finite float >= 0 (cycles per unit of x)")
    directions = tuple(directions)
    if not directions:
        raise ValueError("directions must hold at least one of 'tangential', 'sagittal' or an angle in degrees")
    nu_x, nu_y = [], []
    for d in directions:
        if isinstance(d, str):
            if d not in ("tangential", "sagittal"):
                raise ValueError(f"direction must be 'tangential', 'sagittal' or an angle in degrees from +x, got {d!r}")
            cs = (0.0, 1.0) if d == "tangential" else (1.0, 0.0)
        elif isinstance(d, (int, float)) and not isinstance(d, bool) and math.isfinite(d):
            cs = (math.cos(math.radians(float(d))), math.sin(math.radians(float(d))))
        else:
            raise ValueError(f"direction must be 'tangential', 'sagittal' or a finite angle in degrees from +x, got {d!r}")
        nu_x += [f * cs[0] for f in freqs]
        nu_y += [f * cs[1] for f in freqs]
    return tuple(nu_x), tuple(nu_y), len(directions), len(freqs)


def _spot_sums(x, y, ray_ok, use):
    """S [B, F, W, 3] = (n, sum x, sum y) over the live rays, float64, detached: tl_enclosed_centroid, or the same in torch."""
    with torch.no_grad():
        if use:
            return ops.EnclosedEnergyFunction.apply(x, y, ray_ok, "row", (), (), "circle")[0]
        live = ray_ok != 0
        x64, y64 = (torch.where(live, t.to(torch.float64), t.new_zeros((), dtype=torch.float64)) for t in (x, y))
        return torch.stack([live.to(torch.float64).sum(dim=2), x64.sum(dim=2), y64.sum(dim=2)], dim=-1)


def _otf_sums_torch(x, y, ray_ok, origin, nu_x, nu_y):
    """The definition of otf_sums in torch ops, in float64, on any device.  It holds the ray x J tensors the kernels never form."""
    live = ray_ok != 0
    zero = x.new_zeros((), dtype=torch.float64)
    # a dead ray is the ray at 0 that is not counted: nothing of what it holds reaches a sum or a gradient
    x, y = torch.where(live, x.to(torch.float64), zero), torch.where(live, y.to(torch.float64), zero)
    o = origin.detach()
    dx, dy = x - o[:, :, None, :, 0], y - o[:, :, None, :, 1]
    nx, ny = const_tensor(nu_x, torch.float64, x.device), const_tensor(nu_y, torch.float64, x.device)   # cached: no upload per call
    u = nx * dx[..., None] + ny * dy[..., None]             # cycles, [B, F, P, W, J]
    r = u - torch.round(u)                                  # (round: to nearest even, rint's; its derivative is 0)
    cos, sin = _sincos_turns(r)                             # (two rays half a period apart cancel exactly)
    keep = live[..., None]
    return torch.stack([torch.where(keep, cos, zero).sum(dim=2), torch.where(keep, sin, zero).sum(dim=2)], dim=-1)


def otf_sums(x, y, ray_ok, origin, nu_x, nu_y, fused=None):
    """The Fourier sums [B, F, W, J, 2] (float64) of a traced fan: per row (lens, field, wavelength) and frequency vector j

        sums[row, j] = (C_j, S_j) = sum over the live rays of (cos, sin)(2 pi (nu_xj (x - o_x) + nu_yj (y - o_y))),

    so that OTF_j = (C_j - i S_j) / n.  The low-level form of geometric_mtf, which states the definition; differentiable in x, y.
    `origin`: broadcastable to [B, F, W, 2], a constant (no gradient); nu_x, nu_y: J Python floats each, cycles per unit of x,
    finite, of any sign.  `fused` as for geometric_mtf; more than ops.MTF_MAX_J vectors go in several launches."""
    nu_x, nu_y = tuple(float(v) for v in nu_x), tuple(float(v) for v in nu_y)
    if not nu_x or len(nu_x) != len(nu_y) or not all(math.isfinite(v) for v in nu_x + nu_y):
        raise ValueError("nu_x and nu_y must hold the same number (at least one) of finite floats")
    use = _uses_kernels(fused, (x, y, ray_ok, origin), 2, "MTF", "otf_sums")
    x, y, ray_ok = _rays_4d("otf_sums", x, y, ray_ok)
    B, F, _, W = x.shape
    origin = origin.detach().to(torch.float64).expand(B, F, W, 2)
    if not use:
        return _otf_sums_torch(x, y, ray_ok, origin, nu_x, nu_y)
    parts = [ops.MTFSumsFunction.apply(x, y, ray_ok, origin, nu_x[j:j + ops.MTF_MAX_J], nu_y[j:j + ops.MTF_MAX_J])
             for j in range(0, len(nu_x), ops.MTF_MAX_J)]
    return parts[0] if len(parts) == 1 else torch.cat(parts, dim=3)


def geometric_mtf(x, y, ray_ok, frequencies, directions=("tangential", "sagittal"), common=("wavelength",), centre="field",
                  weights=None, fused=None):
    """The geometric MTF of a traced fan at given spatial frequencies: the modulus of the characteristic function of the spot.

    It is a sum over the traced rays, not the transform of a histogram: exact for those rays at any frequency, with no bin width
    in the result, and smooth in the ray coordinates, so it needs no softening to be differentiable.

    RAYS.  x, y, ray_ok: [B, F, P, W] as RayTracer.trace_rays returns them, broadcastable.  A ROW is one (lens, field,
    wavelength); a ray is LIVE iff ray_ok != 0.  A dead ray adds exactly 0 to every sum and receives exactly 0 gradient, whatever
    its coordinates hold (NaN, +-inf, 1e30): it is excluded by a select, not by a product with 0.  Live rays must be finite.
    FREQUENCY VECTORS.  `frequencies`: K Python floats >= 0 in cycles per length unit of x (cycles / mm here); 0, repeats and
    any order are allowed.  `directions`: D entries, each "tangential" -- modulation along +y, the meridian the tracer puts its
    fields on, nu = (0, nu); "sagittal" -- nu = (nu, 0); or a float, degrees from +x, nu = (nu cos, nu sin), formed on the host in
    float64.  The J = D K vectors (nu_x, nu_y)_j are host doubles.
    DEFINITION.  With the row's origin o (float64, a constant), per row over the live rays, every operation in float64 from the
    inputs and nothing contracted:
        dx = x - o_x,   dy = y - o_y,   u = nu_x dx + nu_y dy  (two products, one sum: cycles),   r = u - rint(u)  (exact)
        C_j = sum cos(2 pi r),   S_j = sum sin(2 pi r)         (the kernels: sincospi(2 r); pi never multiplies into the phase)
        OTF_j = (C_j - i S_j) / n,   MTF_j = sqrt(C_j^2 + S_j^2) / n.
    nu = 0 gives the term (1, 0) exactly: C = n, S = 0 and MTF = 1 with no rounding at all.  |OTF| does not depend on o, only
    the phase does: o carries no gradient because that gradient vanishes identically, and exists for conditioning only -- at an
    image height of 9 mm and 75 cycles / mm the raw phase is ~700 cycles, and float32 anywhere in u leaves nothing of it.
    POOLING.  `common` is a subset of ("wavelength",): C, S and n are added over the wavelengths, each times a weight a_w >= 0
    (`weights`: W Python floats, not all 0; default all 1), before the modulus and the division -- the polychromatic MTF, in which
    lateral colour counts as blur.  It is an OTF only when the pooled rows share one origin, so with pooling the origin must not
    depend on the wavelength.  "field" in `common` raises: rows at different image points have no common OTF.  Without pooling
    the weights multiply each row's own C, S and n (a row of weight 0 is an empty one).  A set with sum a_w n_w = 0 gives MTF 0
    with zero gradient; a modulus of exactly 0 gives zero gradient, by definition.
    ORIGIN.  `centre`: "field" (default) -- the centroid of the field's live rays of all wavelengths; "row" -- the row's own
    (only with common=()); or a tensor broadcastable to [B, F, W, 2] (with pooling: from [B, F, 1, 2]).  A named centre is
    formed from S = (n, sum x, sum y), ROUNDED TO FLOAT32 and widened again, and detached: dx, dy are then exact differences in
    float64, and the origin does not depend on the last bits of a summation order.  An empty row gets origin 0.
    GRADIENTS, with phi = 2 pi r:  dC_j / dx_i = -2 pi nu_xj sin phi_ij,  dS_j / dx_i = 2 pi nu_xj cos phi_ij;  for seeds gC, gS
    gx_i = 2 pi sum_j nu_xj q_ij,  gy_i = 2 pi sum_j nu_yj q_ij,  q_ij = gS_j cos phi_ij - gC_j sin phi_ij (the kernels: the sums
    over j in float64, rounded once to float32 at the store).

    Returns GeometricMTF(n, mtf, centre): mtf [B, F, W, D, K], or [B, F, D, K] when pooled, in the dtype of x; n the (pooled)
    weighted live count, detached; centre the origin used, [B, F, W, 2].  `fused`: False -- the definition in float64 torch ops
    on any device (it holds the ray x J tensors several times over); True -- the HIP kernels (ops.MTFSumsFunction: float32 x, y
    on one AMD GPU, anything else raises; at most ops.MTF_MAX_J vectors per launch, longer lists go in several launches that each
    read the rays again); None -- the kernels where they apply.  The finish (weights, pooling, modulus, division, the zero
    rules) is plain float64 torch on tiny tensors either way.  No host synchronisation.  Designers multiply the curve by
    diffraction_limit_mtf; this function does not."""
    pooled = _mtf_pooled(common, centre)
    nu_x, nu_y, D, K = _mtf_vectors(frequencies, directions)
    tensors = (x, y, ray_ok) + (() if isinstance(centre, str) else (centre,))
    use = _uses_kernels(fused, tensors, 2, "MTF", "geometric_mtf")
    x, y, ray_ok = _rays_4d("geometric_mtf", x, y, ray_ok)
    a = _mtf_weights(weights, x.shape[3])
    S = _spot_sums(x, y, ray_ok, use)
    origin = _mtf_origin(S, centre, pooled)
    sums = otf_sums(x, y, ray_ok, origin, nu_x, nu_y, fused=use)
    n, mtf = _mtf_finish(sums, S[..., 0], a, pooled)
    return GeometricMTF(n.detach().to(x.dtype), mtf.reshape(*mtf.shape[:-1], D, K).to(x.dtype), origin.to(x.dtype))


def _mtf_pooled(common, centre):
    """Whether the rows are pooled over the wavelengths; what geometric_mtf refuses of `common` and a named `centre` raises."""
    common = tuple(common)
    if "field" in common:
        raise ValueError("common must not hold 'field': rows at different image points have no common OTF")
    if any(c != "wavelength" for c in common):
        raise ValueError("common must be a subset of ('wavelength',)")
    pooled = bool(common)
    if isinstance(centre, str):
        if centre not in ("row", "field"):
            raise ValueError("centre must be 'row', 'field' or a tensor broadcastable to [B, F, W, 2]")
        if centre == "row" and pooled:
            raise ValueError("centre='row' gives every wavelength its own origin: pooled rows need one (centre='field' or a tensor)")
    return pooled


def _mtf_weights(weights, W):
    a = (1.0,) * W if weights is None else tuple(float(v) for v in weights)
    if len(a) != W or not all(0.0 <= v < float("inf") for v in a) or not any(v > 0.0 for v in a):
        raise ValueError(f"weights must be {W} finite floats >= 0 (one per wavelength), not all 0")
    return a


def _mtf_origin(S, centre, pooled):
    """The origin [B, F, W, 2] (float64, detached) of S [B, F, W, 3] = (n, sum x, sum y): a named centre rounded to float32 and
    widened again, or the given tensor."""
    B, F, W = S.shape[:3]
    if isinstance(centre, str):
        return _enclosed_centre(S, centre).to(torch.float32).to(torch.float64)
    shape = (1,) * (4 - centre.dim()) + tuple(centre.shape)
    if centre.dim() > 4 or (pooled and shape[2] != 1):
        raise ValueError("with pooling the centre must not depend on the wavelength: broadcastable from [B, F, 1, 2]")
    return centre.detach().to(torch.float64).expand(B, F, W, 2)


def _mtf_finish(sums, n, a, pooled):
    """(n, mtf) of sums [B, F, W, .., 2] and the live counts n [B, F, W]: the weights a (W floats), pooling over the wavelengths,
    modulus, division and the zero rules, in float64; n and mtf lose the wavelength dimension when pooled."""
    a = const_tensor(a, torch.float64, sums.device)
    sums, n = sums * a.reshape(-1, *(1,) * (sums.dim() - 3)), n * a
    if pooled:
        sums, n = sums.sum(dim=2), n.sum(dim=2)
    m2 = sums[..., 0] * sums[..., 0] + sums[..., 1] * sums[..., 1]
    some, lit = m2 > 0, (n > 0).reshape(*n.shape, *(1,) * (m2.dim() - n.dim()))
    n1 = n.reshape(lit.shape)
    modulus = torch.where(some, torch.sqrt(torch.where(some, m2, torch.ones_like(m2))), torch.zeros_like(m2))
    return n, torch.where(lit, modulus / torch.where(lit, n1, torch.ones_like(m2)), torch.zeros_like(m2))


# ---------------------------------------------------------------------------- through-focus MTF: one rotor per ray and frequency
class ThroughFocusMTF(NamedTuple):
    """What through_focus_mtf returns."""
    n: torch.Tensor                 # weighted live rays, [B, F, W] less the pooled dimension
    mtf: torch.Tensor               # modulus of the geometric OTF, [..., Z, D, K]: planes x directions x frequencies
    shifts: torch.Tensor            # the Z plane positions along +z (float64)
    centre: torch.Tensor            # the origin every row's phase was measured from, [B, F, W, 2]


def _planes(planes):
    """(first, step, Z) of `planes` as two Python floats and an int."""
    try:
        first, step, count = planes
        first, step = float(first), float(step)
    except (TypeError, ValueError):
        raise ValueError("planes must be (first, step, count): two finite floats and an int >= 1") from None
    if not (math.isfinite(first) and math.isfinite(step)) or isinstance(count, bool) or not isinstance(count, int) or count < 1:
        raise ValueError("planes must be (first, step, count): two finite floats and an int >= 1")
    if count > 1 and step == 0.0:
        raise ValueError("planes: a step of 0 puts every plane at one shift; two or more planes need a step other than 0")
    return first, step, count


def _plane_chunks(first, step, Z):
    """[(first of the chunk, planes in it)]: the planes in chunks of ops.TFMTF_MAX_Z, chunk q starting at first + (16 q) step
    formed on the host in float64, where the recurrence restarts."""
    return [(first + z0 * step, min(ops.TFMTF_MAX_Z, Z - z0)) for z0 in range(0, Z, ops.TFMTF_MAX_Z)]


def plane_shifts(planes):
    """The positions of the planes (first, step, count) as the through-focus MTF takes them: Python floats, plane 16 q + r at
    (first + (16 q) step) + r step, every operation in float64."""
    first, step, Z = _planes(planes)
    return tuple(f0 + r * step for f0, n in _plane_chunks(first, step, Z) for r in range(n))


def _sincos_turns(r):
    """(cos, sin)(2 pi r) for |r| <= 1 / 2 as the device library's sincospi(2 r) forms them: quarter turns taken off exactly, pi
    multiplies only into |t| <= 1 / 8, so that r = 0, 1 / 4, 1 / 2 give (1, 0), (0, 1), (-1, 0) without a rounding."""
    k = torch.round(4.0 * r)
    phi = (2.0 * math.pi) * (r - 0.25 * k)
    c0, s0, k = torch.cos(phi), torch.sin(phi), torch.remainder(k, 4.0)
    cos = torch.where(k == 0, c0, torch.where(k == 1, -s0, torch.where(k == 2, -c0, s0)))
    sin = torch.where(k == 0, s0, torch.where(k == 1, c0, torch.where(k == 2, -s0, -c0)))
    return cos, sin


def _tfmtf_sums_torch(x, y, cx, cy, ray_ok, origin, nu_x, nu_y, first, step, Z):
    """The definition of otf_sums_through_focus for one chunk of planes in torch ops, in float64, on any device, the recurrence
    included.  It holds the ray x J tensors the kernels never form."""
    x, y, cx, cy = (t.to(torch.float64) for t in (x, y, cx, cy))
    live = (ray_ok != 0) & (1 - cx * cx - cy * cy > 0)                # (NaN > 0 is false)
    zero = x.new_zeros(())
    # a dead ray is the ray at 0 along the axis that is not counted: nothing of what it holds reaches a sum or a gradient
    x, y, cx, cy = (torch.where(live, t, zero) for t in (x, y, cx, cy))
    cz = torch.sqrt(1 - cx * cx - cy * cy)
    u, v = cx / cz, cy / cz
    o = origin.detach()
    dx, dy = x - o[:, :, None, :, 0], y - o[:, :, None, :, 1]
    nx, ny = const_tensor(nu_x, torch.float64, x.device), const_tensor(nu_y, torch.float64, x.device)
    a = nx * dx[..., None] + ny * dy[..., None]             # cycles, [B, F, P, W, J]
    b = nx * u[..., None] + ny * v[..., None]               # cycles per unit of shift
    p0 = a + first * b
    c, s = _sincos_turns(p0 - torch.round(p0))              # (round: to nearest even, rint's; its derivative is 0)
    q = (step if Z > 1 else 0.0) * b
    cr, sr = _sincos_turns(q - torch.round(q))
    keep = live[..., None]
    out = []
    for z in range(Z):
        out.append(torch.stack([torch.where(keep, c, zero).sum(dim=2), torch.where(keep, s, zero).sum(dim=2)], dim=-1))
        if z + 1 < Z:
            c, s = c * cr - s * sr, s * cr + c * sr
    return torch.stack(out, dim=-2)                         # [B, F, W, J, Z, 2]


def otf_sums_through_focus(x, y, cx, cy, ray_ok, origin, nu_x, nu_y, planes, fused=None):
    """The Fourier sums [B, F, W, J, Z, 2] (float64) of a traced fan at Z equally spaced focal planes; the low-level form of
    through_focus_mtf, which states the definition.  sums[row, j, z] = (C_jz, S_jz) over the live rays, OTF_jz = (C - i S) / n.
    Differentiable in x, y, cx, cy.  `origin`, nu_x, nu_y as for otf_sums; planes = (first, step, count).  `fused` as for
    through_focus_mtf.  More than ops.TFMTF_MAX_J vectors or ops.TFMTF_MAX_Z planes go in several calls: vectors in 16s, planes in
    16s with chunk q starting at first + (16 q) step, formed on the host in float64, where the recurrence restarts -- that is
    part of the definition (either path), so a plane's bits do not depend on how many planes follow it."""
    nu_x, nu_y = tuple(float(v) for v in nu_x), tuple(float(v) for v in nu_y)
    if not nu_x or len(nu_x) != len(nu_y) or not all(math.isfinite(v) for v in nu_x + nu_y):
        raise ValueError("nu_x and nu_y must hold the same number (at least one) of finite floats")
    first, step, Z = _planes(planes)
    use = _uses_kernels(fused, (x, y, cx, cy, ray_ok, origin), 4, "through-focus MTF", "otf_sums_through_focus")
    x, y, cx, cy, ray_ok = _rays_4d("otf_sums_through_focus", x, y, cx, cy, ray_ok)
    B, F, _, W = x.shape
    origin = origin.detach().to(torch.float64).expand(B, F, W, 2)
    mj = ops.TFMTF_MAX_J
    cols = []
    for f0, nz in _plane_chunks(first, step, Z):
        if use:
            parts = [ops.TFMTFSumsFunction.apply(x, y, cx, cy, ray_ok, origin, nu_x[j:j + mj], nu_y[j:j + mj], f0, step, nz)
                     for j in range(0, len(nu_x), mj)]
        else:
            parts = [_tfmtf_sums_torch(x, y, cx, cy, ray_ok, origin, nu_x[j:j + mj], nu_y[j:j + mj], f0, step, nz)
                     for j in range(0, len(nu_x), mj)]
        cols.append(parts[0] if len(parts) == 1 else torch.cat(parts, dim=3))
    return cols[0] if len(cols) == 1 else torch.cat(cols, dim=4)


def through_focus_mtf(x, y, cx, cy, ray_ok, frequencies, planes, directions=("tangential", "sagittal"), common=("wavelength",),
                      centre="field", weights=None, fused=None):
    """The geometric MTF of a traced fan against focus shift: geometric_mtf at Z equally spaced focal planes, from one pass over
    the rays as they stand.

    Behind the last surface a ray is a straight line: at an image plane shifted by d along +z (the sign of through_focus) it lands
    at (x + d u, y + d v), u = cx / cz, v = cy / cz, so its phase there is a + d b with a = nu . (r - o) and b = nu . (u, v), and
    over equally spaced planes exp(2 pi i (a + d_z b)) is a geometric sequence.

    RAYS.  x, y, cx, cy, ray_ok: [B, F, P, W] as RayTracer.trace_rays returns them, broadcastable.  A ray is LIVE iff ray_ok != 0
    and s = 1 - cx^2 - cy^2 > 0 (through_focus's rule, in float64).  A dead ray is excluded by a select: it adds +0.0 to every sum
    and receives exactly 0 gradient whatever it holds.
    PLANES.  planes = (first, step, count): plane z lies at first + z step; at most ops.TFMTF_MAX_Z = 16 planes share one
    recurrence, chunk q of a longer list starts at first + (16 q) step (formed on the host in float64) and restarts it.
    FREQUENCY VECTORS, POOLING, WEIGHTS, ORIGIN: geometric_mtf's, word for word; a named centre and n come from the first three
    of focus_moments' moments (n, sum x, sum y), so the live rule is the one above.
    DEFINITION.  Per row over the live rays, every operation in float64 from the inputs and nothing contracted, d0 the chunk's
    first shift and dd the step:
        cz = sqrt(s),  u = cx / cz,  v = cy / cz,  dx = x - o_x,  dy = y - o_y
        a  = nu_x dx + nu_y dy  (cycles),   b = nu_x u + nu_y v  (cycles per unit of shift)
        p0 = a + d0 b,  r0 = p0 - rint(p0),  (c_0, s_0) = sincospi(2 r0)          plane 0 of the chunk
        q  = dd b,      rq = q - rint(q),    (cr, sr)   = sincospi(2 rq)          the rotor
        (c_z, s_z) = (c_{z-1} cr - s_{z-1} sr,  s_{z-1} cr + c_{z-1} sr),  z = 1 .. 15
        C_jz = sum c_z,  S_jz = sum s_z;   OTF = (C - i S) / n,  MTF = sqrt(C^2 + S^2) / n.
    nu = 0 gives a = b = 0 and the term (1, 0) at every plane exactly: MTF = 1 with no rounding.  Two sincospi per ray and
    frequency vector instead of one per plane, and no shifted coordinate is ever rounded to float32.
    GRADIENTS.  For seeds (gC, gS)_jz, Q_jz = gS c_z - gC s_z:  gx = 2 pi sum_j nu_xj sum_z Q_jz,  gu = 2 pi sum_j nu_xj sum_z
    d_z Q_jz, gy and gv with nu_y; the slopes pass to the cosines by du/dcx = (1 - cy^2) / cz^3, du/dcy = dv/dcx = cx cy / cz^3,
    dv/dcy = (1 - cx^2) / cz^3.  No gradient to the origin (the modulus does not depend on it), the frequencies, shifts or weights.

    Returns ThroughFocusMTF(n, mtf, shifts, centre): mtf [B, F, W, Z, D, K], or [B, F, Z, D, K] when pooled, in the dtype of x;
    shifts the Z plane positions (float64, on the rays' device; plane_shifts gives them on the host); n and centre as
    geometric_mtf's.  `fused`: False -- the definition above, recurrence included, in float64 torch ops on any device; True --
    the HIP kernels (ops.TFMTFSumsFunction: float32 x, y, cx, cy on one AMD GPU, anything else raises); None -- the kernels
    where they apply.  The finish is geometric_mtf's.  No host synchronisation.  mtf_best_focus reads the MTF-best focus off it."""
    pooled = _mtf_pooled(common, centre)
    nu_x, nu_y, D, K = _mtf_vectors(frequencies, directions)
    first, step, Z = _planes(planes)
    tensors = (x, y, cx, cy, ray_ok) + (() if isinstance(centre, str) else (centre,))
    use = _uses_kernels(fused, tensors, 4, "through-focus MTF", "through_focus_mtf")
    x, y, cx, cy, ray_ok = _rays_4d("through_focus_mtf", x, y, cx, cy, ray_ok)
    a = _mtf_weights(weights, x.shape[3])
    if use:                                                 # what is expanded or strided differently is copied here, once: both nodes
        (x, y, cx, cy), ray_ok, _, _ = ops._row_rays({"x": x, "y": y, "cx": cx, "cy": cy}, ray_ok, "through-focus MTF")     # then read in place
    with torch.no_grad():
        S = focus_moments(x, y, cx, cy, ray_ok, fused=use)[..., :3]
    origin = _mtf_origin(S, centre, pooled)
    sums = otf_sums_through_focus(x, y, cx, cy, ray_ok, origin, nu_x, nu_y, (first, step, Z), fused=use)
    n, mtf = _mtf_finish(sums, S[..., 0], a, pooled)        # mtf [.., J, Z]
    mtf = mtf.reshape(*mtf.shape[:-2], D, K, Z).movedim(-1, -3)
    shifts = const_tensor(plane_shifts((first, step, Z)), torch.float64, x.device)
    return ThroughFocusMTF(n.detach().to(x.dtype), mtf.to(x.dtype), shifts, origin.to(x.dtype))


def mtf_best_focus(mtf, shifts):
    """The MTF-best focus of a through-focus curve: for mtf [..., Z, D, K] (through_focus_mtf's) and the Z plane positions
    `shifts`, per (..., D, K) the plane of the largest MTF, refined by the parabola through that sample and its two neighbours.

    Returns (shift, mtf_peak, interior), each [..., D, K]: the vertex of the parabola and its value there; `interior` (bool) is
    False where the maximum sits on the first or the last plane (or Z < 3) -- there `shift` is that plane and `mtf_peak` its
    sample.  Of equal maxima the first counts.  The shifts must be distinct (through_focus_mtf's are: it refuses a step of 0).
    Differentiable in mtf, with the arg-max detached.  Plain torch on the tiny result."""
    if mtf.dim() < 3 or shifts.dim() != 1 or mtf.shape[-3] != shifts.shape[0]:
        raise ValueError(f"mtf must be [..., Z, D, K] and shifts [Z], got {tuple(mtf.shape)} and {tuple(shifts.shape)}")
    Z = shifts.shape[0]
    m = mtf.to(torch.float64)
    d = shifts.to(device=m.device, dtype=torch.float64)
    top = m.detach().argmax(dim=-3, keepdim=True)           # the first of equal maxima
    interior = (top > 0) & (top < Z - 1)
    mid = top.clamp(1, Z - 2) if Z >= 3 else top
    at = lambda i: (m.gather(-3, i).squeeze(-3), d[i.squeeze(-3)])          # noqa: E731
    y1, x1 = at(torch.where(interior, mid, top))
    if Z < 3:
        return x1.to(mtf.dtype), y1.to(mtf.dtype), interior.squeeze(-3)
    (y0, x0), (y2, x2) = at(mid - 1), at(mid + 1)
    ym, xm = m.gather(-3, mid).squeeze(-3), d[mid.squeeze(-3)]
    # Newton's form through (x0, y0), (xm, ym), (x2, y2): y = y0 + d01 (x - x0) + a2 (x - x0) (x - xm)
    d01, d12 = (ym - y0) / (xm - x0), (y2 - ym) / (x2 - xm)
    a2 = (d12 - d01) / (x2 - x0)
    # (the first of the largest samples has a smaller one before it and none larger after it: a2 < 0 wherever it is interior)
    inside = interior.squeeze(-3)
    a2 = torch.where(inside, a2, -torch.ones_like(a2))
    xv = 0.5 * (x0 + xm) - d01 / (2.0 * a2)
    yv = y0 + d01 * (xv - x0) + a2 * (xv - x0) * (xv - xm)
    return torch.where(inside, xv, x1).to(mtf.dtype), torch.where(inside, yv, y1).to(mtf.dtype), inside


def diffraction_limit_mtf(frequencies, wavelength, f_number):
    """The MTF of an aberration-free circular pupil, 2 / pi (acos s - s sqrt(1 - s^2)) with s = nu lambda N, 0 from the cutoff
    1 / (lambda N) on.  frequencies: floats or a tensor, cycles per length unit; wavelength in that unit; returns a float64
    tensor of the frequencies' shape.  Plain torch."""
    nu = torch.as_tensor(frequencies, dtype=torch.float64)
    s = (nu.abs() * wavelength * f_number).clamp(max=1.0)
    return (2.0 / math.pi) * (torch.acos(s) - s * torch.sqrt(1.0 - s * s))
