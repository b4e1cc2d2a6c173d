"""
Rendering an image through the lens.  First, the spatially varying overlap-add convolution of an image with a grid of PSFs (the
reference's `svola_convolution`, image_ops.py:6-98, which cannot run as written: `fft` is undefined, `F.pad(mode='symmetric')`
and `torch.nn.functional.resize_with_crop_or_pad` do not exist in torch, and it transforms over (C, H) instead of (H, W)).

The definition implemented here is the evident intent of that text; see `svola_convolution`.  Behind it: the PSF grid over the
image, the bicubic warp for distortion and relative illumination, and the metrics the reference's renderer reports on the
result, `ssim` and `psnr`.
"""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from . import ops
from .lens_modeling import const_tensor


def _axis(n, g, o, window_type, name):
    p = n // g + 2 * o
    full = n + 2 * o
    lo = np.round(np.linspace(0, 1, g) * (full - p)).astype(int)
    hi = lo + p
    x = np.linspace(0, 1, p + 2)[1:-1]
    if window_type == "boxcar":
        win = np.ones_like(x)
    elif window_type == "hann":
        win = np.sin(np.pi * x) ** 2
    else:
        raise ValueError(f"window_type must be 'boxcar' or 'hann', got {window_type!r}")
    tab = np.zeros((g, full), dtype=np.float64)
    for i in range(g):
        tab[i, lo[i]:hi[i]] = win
    total = tab.sum(axis=0)
    uncovered = np.nonzero(total[o:o + n] <= 0)[0]
    if uncovered.size:
        raise ValueError(f"svola_convolution: {name} {int(uncovered[0])} of the image lies in no patch "
                         f"({n} {name}s, grid {g}, overlap {o}: patches of {p} at {lo.tolist()}); the reference divides by zero there")
    tab = np.divide(tab, total, out=np.zeros_like(tab), where=total > 0)
    return lo, hi, win, tab


@functools.lru_cache(maxsize=64)
def svola_geometry(H, W, gh, gw, oh, ow, window_type="boxcar"):
    """The patch layout of svola_convolution, shared by the torch path, the kernels and the tests (memoised).

    r0, r1 [gh] / c0, c1 [gw]: patch n = i gw + j owns rows [r0[i], r1[i]) and columns [c0[j], c1[j]) of the frame of
    Ih = H + 2 oh rows and Iw = W + 2 ow columns; win_r [ph], win_c [pw]: the window along each axis; tab_r [gh, Ih],
    tab_c [gw, Iw] (float64): the window of patch row i at frame row r, 0 outside, divided by the sum over the patches of
    that axis -- the window is separable, so the normalised weight of patch n at (r, q) is tab_r[i, r] tab_c[j, q].
    Raises ValueError when a row or column of the central H x W lies in no patch."""
    r0, r1, win_r, tab_r = _axis(H, gh, oh, window_type, "row")
    c0, c1, win_c, tab_c = _axis(W, gw, ow, window_type, "column")
    bounds = tuple((C.c_int32 * len(a))(*a.tolist()) for a in (r0, r1, c0, c1))         # host ints of the C ABI
    return SimpleNamespace(H=H, W=W, gh=gh, gw=gw, oh=oh, ow=ow, ph=H // gh + 2 * oh, pw=W // gw + 2 * ow, r0=r0, r1=r1, c0=c0,
                           c1=c1, win_r=win_r, win_c=win_c, tab_r=tab_r, tab_c=tab_c, bounds=bounds, device_tables={})


def _symmetric_index(n, pad, device):
    """Indices of numpy's mode='symmetric' extension by `pad` on each side (pad <= n): -1-i -> i, n+i -> n-1-i."""
    i = torch.arange(-pad, n + pad, device=device)
    return torch.where(i < 0, -1 - i, torch.where(i >= n, 2 * n - 1 - i, i))


def _svola_torch(image, psfs, geo):
    """The definition in plain torch ops (any device, any float dtype): per-patch haloed views of the padded image, one
    grouped conv2d with the flipped kernels, a weighted accumulate into the frame, a crop."""
    B, H, W, Cc = image.shape
    N, kh, kw = psfs.shape[1:4]
    a, b = kh // 2, kw // 2
    oh, ow, ph, pw = geo.oh, geo.ow, geo.ph, geo.pw
    img = image.permute(0, 3, 1, 2)                                                      # [B, C, H, W]
    P = img[:, :, _symmetric_index(H, oh + a, image.device)][:, :, :, _symmetric_index(W, ow + b, image.device)]
    slabs = [P[:, :, geo.r0[n // geo.gw]:geo.r1[n // geo.gw] + 2 * a, geo.c0[n % geo.gw]:geo.c1[n % geo.gw] + 2 * b]
             for n in range(N)]
    x = torch.stack(slabs, dim=0).reshape(1, N * B * Cc, ph + 2 * a, pw + 2 * b)
    k = psfs.expand(B, N, kh, kw, Cc).permute(1, 0, 4, 2, 3).flip(-1, -2).reshape(N * B * Cc, 1, kh, kw)
    y = F.conv2d(x, k, groups=N * B * Cc).reshape(N, B, Cc, ph, pw)
    key = ("torch", image.device, image.dtype)
    if key not in geo.device_tables:                       # uploaded once per device and dtype (a captured step uploads nothing)
        geo.device_tables[key] = (torch.from_numpy(geo.tab_r).to(device=image.device, dtype=image.dtype),
                                  torch.from_numpy(geo.tab_c).to(device=image.device, dtype=image.dtype))
    tab_r, tab_c = geo.device_tables[key]
    frame = torch.zeros((B, Cc, H + 2 * oh, W + 2 * ow), dtype=y.dtype, device=image.device)
    for n in range(N):
        i, j = divmod(n, geo.gw)
        r0, r1, c0, c1 = geo.r0[i], geo.r1[i], geo.c0[j], geo.c1[j]
        frame[:, :, r0:r1, c0:c1] += y[n] * (tab_r[i, r0:r1, None] * tab_c[j, None, c0:c1])
    return frame[:, :, oh:oh + H, ow:ow + W].permute(0, 2, 3, 1)


def svola_convolution(image, overlap_size, psfs, psfs_grid_shape, window_type="boxcar", fused=None):
    """Spatially varying overlap-add convolution: the image is cut into a gh x gw grid of overlapping patches, each patch is
    convolved with the PSF of its field position, and the patches are blended back with window weights.

    image [B, H, W, C]; psfs [B, N, kh, kw, C] or [1, N, ...] (shared by the batch), N = gh gw row-major over the grid, kh and
    kw odd; overlap_size an int or (oh, ow); window_type 'boxcar' or 'hann'.  Returns [B, H, W, C].

    With a = kh//2, b = kw//2, Ih = H + 2 oh, Iw = W + 2 ow:
      * P is the image extended by oh + a rows and ow + b columns on each side by SYMMETRIC reflection, edge pixel included
        (-1-i -> i, H+i -> H-1-i: numpy's mode='symmetric', not torch's 'reflect'); oh + a <= H and ow + b <= W (ValueError).
      * ph = H//gh + 2 oh, r0 = np.round(np.linspace(0, 1, gh) * (Ih - ph)).astype(int), r1 = r0 + ph, columns likewise;
        patch n = i gw + j owns rows [r0_i, r1_i) and columns [c0_j, c1_j) of the Ih x Iw frame (the image plus the overlap
        margin, without the kernel halo).
      * win_r = f(np.linspace(0, 1, ph + 2)[1:-1]), f = 1 (boxcar) or sin^2(pi x) (hann); w_n(r, q) = win_r[r - r0] win_c[q - c0]
        inside the patch, 0 outside, normalised by the sum over the patches.  A pixel of the image that no patch covers
        (H = 23, gh = 2, oh = 0) raises ValueError and names the axis.
      * out[b,y,x,c] = sum_n w_n(r,q) sum_{i,j} psfs[b,n,i,j,c] P[b, r + 2a - i, q + 2b - j, c],  (r, q) = (y + oh, x + ow).
        The frame pixel (r, q) sits at P[r + a, q + b]: a true, centred convolution -- a point of light becomes the PSF, not
        its mirror image.

    Deviations from the letter of image_ops.py:6-98: (1) the transform axes are (H, W), not (C, H); (2) the result is centred
    (the reference's roll by -(pad+1) followed by a central crop lands one pixel off); (3) the `torch.abs` of the inverse FFT
    is dropped (the identity for non-negative images and PSFs); (4) the uncovered-pixel case is refused instead of returning
    NaN.

    `fused=False`: the definition in plain torch ops (a direct grouped conv2d, not an FFT) -- any device, any float dtype,
    autograd does the rest.  `fused=True`: the HIP kernels of csrc/tl_svola.hip (ops.SvolaFunction): float32 tensors on one
    GPU, kh, kw <= 31, gh, gw <= 128; no patch tensor is built, and the gradients to psfs (and to the image, when it needs
    one) are kernels too; anything else raises (there is no CPU fallback).  `fused=None` (default): the kernels when they
    apply, torch otherwise."""
    if image.dim() != 4 or psfs.dim() != 5:
        raise ValueError("svola_convolution: image must be [B, H, W, C] and psfs [B or 1, N, kh, kw, C]")
    B, H, W, Cc = image.shape
    gh, gw = (int(v) for v in psfs_grid_shape)
    oh, ow = (int(overlap_size),) * 2 if isinstance(overlap_size, int) else (int(v) for v in overlap_size)
    Bp, N, kh, kw, Cp = psfs.shape
    if gh < 1 or gw < 1 or N != gh * gw:
        raise ValueError(f"svola_convolution: psfs holds {N} kernels, the grid {gh} x {gw} needs {gh * gw}")
    if Bp not in (1, B) or Cp != Cc:
        raise ValueError(f"svola_convolution: psfs {tuple(psfs.shape)} does not fit the image {tuple(image.shape)}")
    if kh % 2 == 0 or kw % 2 == 0:
        raise ValueError(f"svola_convolution: kh and kw must be odd, got {kh} x {kw}")
    if oh < 0 or ow < 0 or oh + kh // 2 > H or ow + kw // 2 > W:
        raise ValueError(f"svola_convolution: overlap + kernel half-width ({oh} + {kh // 2}, {ow} + {kw // 2}) must not exceed "
                         f"the image ({H}, {W})")
    geo = svola_geometry(H, W, gh, gw, oh, ow, window_type)
    applies = (image.is_cuda and psfs.device == image.device and image.dtype == torch.float32 and psfs.dtype == torch.float32
               and max(kh, kw) <= ops.SVOLA_MAX_TAPS and max(gh, gw) <= ops.SVOLA_MAX_GRID)
    if fused is None:
        fused = applies              # the kernels are ~10 x the torch path on the recorded workload (profiles/svola_timing.txt)
    if not fused:
        return _svola_torch(image, psfs, geo)
    if max(kh, kw) > ops.SVOLA_MAX_TAPS or max(gh, gw) > ops.SVOLA_MAX_GRID:
        raise ValueError(f"svola_convolution(fused=True) takes PSFs of at most {ops.SVOLA_MAX_TAPS} x {ops.SVOLA_MAX_TAPS} taps on "
                         f"grids of at most {ops.SVOLA_MAX_GRID} x {ops.SVOLA_MAX_GRID}; got {kh} x {kw} on {gh} x {gw}")
    if not applies:
        raise RuntimeError(f"svola_convolution(fused=True): image is {image.dtype} on {image.device}, psfs {psfs.dtype} on "
                           f"{psfs.device}; the fused convolution runs only as HIP kernels on float32 tensors on one AMD GPU "
                           "(there is no CPU fallback): use fused=False")
    return ops.SvolaFunction.apply(image, psfs, geo)


def psf_grid_from_fields(kernels, grid_shape, index_map=None):
    """Arrange compute_psf's kernels [n_fields, C, kh, kw] as the psfs [1, N, kh, kw, C] of svola_convolution.

    Without `index_map` the fields are the grid in row-major order (n_fields = gh gw; a column of fields is a gh x 1 grid) and
    the result is a permuted VIEW of `kernels`: the fused kernels read it through its strides, nothing is copied.  With
    `index_map` ([gh, gw] integers: the field of every grid cell, e.g. by image height) the kernels are gathered, which
    copies N small kernels unless the map is the identity.  A map given as host values (nested lists, a numpy array, a CPU
    tensor) is checked on the host and its device copy is cached: pass it so inside a captured step.  A map that is a device
    tensor is checked on the device, which synchronises."""
    gh, gw = (int(v) for v in grid_shape)
    if kernels.dim() != 4:
        raise ValueError("psf_grid_from_fields: kernels must be [n_fields, C, kh, kw]")
    if index_map is not None and not (torch.is_tensor(index_map) and index_map.device.type != "cpu"):
        host = (index_map.numpy() if torch.is_tensor(index_map) else np.asarray(index_map)).reshape(-1)
        if host.size != gh * gw:
            raise ValueError(f"psf_grid_from_fields: index_map must hold {gh} x {gw} entries")
        host = host.astype(np.int64)
        if int(host.min()) < 0 or int(host.max()) >= kernels.shape[0]:
            raise ValueError("psf_grid_from_fields: index_map names a field that does not exist")
        if not (host.size == kernels.shape[0] and np.array_equal(host, np.arange(host.size))):
            kernels = kernels.index_select(0, const_tensor(host.tolist(), torch.long, kernels.device))
    elif index_map is not None:
        idx = index_map.to(torch.long).reshape(-1)
        if idx.numel() != gh * gw:
            raise ValueError(f"psf_grid_from_fields: index_map must hold {gh} x {gw} entries")
        if int(idx.min()) < 0 or int(idx.max()) >= kernels.shape[0]:
            raise ValueError("psf_grid_from_fields: index_map names a field that does not exist")
        if not (idx.numel() == kernels.shape[0] and bool((idx == torch.arange(idx.numel(), device=idx.device)).all())):
            kernels = kernels.index_select(0, idx.to(kernels.device))
    elif kernels.shape[0] != gh * gw:
        raise ValueError(f"psf_grid_from_fields: {kernels.shape[0]} fields do not fill a {gh} x {gw} grid (give an index_map)")
    return kernels.permute(0, 2, 3, 1).unsqueeze(0)


@functools.lru_cache(maxsize=64)
def _psf_grid_cells(H, W, gh, gw, oh, ow, fields, aspect, blend):
    geo = svola_geometry(H, W, gh, gw, oh, ow)
    f = np.asarray(fields, dtype=np.float64)
    # the middle pixel of a patch, (lo + hi - 1) / 2 in the frame, less the overlap margin; then _pixel_axes' normalisation,
    # written (2 p - (n - 1)) / (n - 1) so that mirrored patches get exactly opposite coordinates
    norm = lambda lo, hi, o, n: ((lo + hi - 1.0) - 2.0 * o - (n - 1)) / (n - 1) if n > 1 else np.zeros(len(lo))  # noqa: E731
    yn, xn = norm(geo.r0, geo.r1, oh, H), norm(geo.c0, geo.c1, ow, W)
    a = float(W) / float(H) if aspect is None else float(aspect)
    X, Y = np.broadcast_to(xn[None, :] * a, (gh, gw)).reshape(-1), np.broadcast_to(yn[:, None], (gh, gw)).reshape(-1)
    rad = np.hypot(X, Y)
    h = rad / np.sqrt(a * a + 1.0)
    centre = rad == 0
    safe = np.where(centre, 1.0, rad)
    s_cell, c_cell = np.where(centre, 0.0, X / safe), np.where(centre, 1.0, Y / safe)
    src, cell, beta = [], [], []
    for n in range(gh * gw):
        if blend == "nearest":
            terms = [(int(np.argmin(np.abs(f - h[n]))), 1.0)]
        elif h[n] <= f[0]:
            terms = [(0, 1.0)]
        elif h[n] >= f[-1]:
            terms = [(len(f) - 1, 1.0)]
        else:
            k = int(np.searchsorted(f, h[n], side="right")) - 1
            t = (h[n] - f[k]) / (f[k + 1] - f[k])
            terms = [(k, 1.0 - t), (k + 1, t)]
        for k, b in terms:
            if b != 0.0:
                src.append(k)
                cell.append(n)
                beta.append(b)
    cell = np.asarray(cell, dtype=np.int64)
    grid = ops.psf_rot_grid(np.asarray(src, dtype=np.int64), c_cell[cell], s_cell[cell], len(f))
    return SimpleNamespace(gh=gh, gw=gw, N=gh * gw, n_fields=len(f), X=X, Y=Y, h=h, s_cell=s_cell, c_cell=c_cell, grid=grid,
                           src=grid.src, c=grid.c, s=grid.s, field_start=grid.field_start, field_grids=grid.field_grids,
                           cell=cell, beta=np.asarray(beta, dtype=np.float64), batched={1: grid}, blend_tables={})


def psf_grid_cells(image_size, grid_shape, overlap_size, fields, aspect=None, blend="linear"):
    """Where the PSFs of a gh x gw svola grid come from, for a rotationally symmetric lens traced along the +y meridian: pure
    host geometry (numpy, no GPU), memoised.

    image_size (H, W), grid_shape (gh, gw) and overlap_size (int or (oh, ow)) are svola_convolution's; `fields` [K] are the
    relative image heights of the traced fields (ascending, >= 0; 0 is allowed), in units of the half-diagonal as in
    radial_map; `aspect` is width / height (default W / H).

    Cell n = i gw + j sits at the middle of its patch [r0, r1) x [c0, c1) of svola_geometry less the overlap margin, in the
    normalised pixel coordinates of the warp (columns are x, rows are y, both growing with the index, -1 .. +1 over the
    image): (X, Y) = (x aspect, y) and h = |(X, Y)| / sqrt(aspect^2 + 1), 1 at the corner.  Its rotation is
    (s, c) = (X, Y) / |(X, Y)|, (0, 1) at the exact centre: a spot traced at (xi, eta) about its centre lands at
    x' = c xi + s eta (columns), y' = -s xi + c eta (rows), so the trace's +y meridian points along the cell's radius.
    Every cell is up to two terms (field, beta): with blend="linear" the two traced fields that bracket h with linear weights
    in h (one term of beta = 1 at or beyond the first and the last field, and terms of beta = 0 are dropped); with
    blend="nearest" the nearest field alone.

    Returns a namespace: the flat term list `src`, `c`, `s` [T] (int32 / float32, as the kernels take them), `cell` [T] (the
    cell of every term, ascending) and `beta` [T] (float64; sums to 1 per cell), the CSR inverse of src `field_start` [K+1] and
    `field_grids` [T], and per cell X, Y, h, s_cell, c_cell [N] (float64); `grid` is the ops.psf_rot_grid of the term list."""
    H, W = (int(v) for v in image_size)
    gh, gw = (int(v) for v in grid_shape)
    oh, ow = (int(overlap_size),) * 2 if isinstance(overlap_size, int) else (int(v) for v in overlap_size)
    f = tuple(float(v) for v in np.asarray(fields, dtype=np.float64).reshape(-1))
    if len(f) < 1 or f[0] < 0 or any(b <= a for a, b in zip(f, f[1:])):
        raise ValueError("psf_grid_cells: fields must be ascending and >= 0")
    if blend not in ("linear", "nearest"):
        raise ValueError(f"psf_grid_cells: blend must be 'linear' or 'nearest', got {blend!r}")
    if gh < 1 or gw < 1:
        raise ValueError(f"psf_grid_cells: grid_shape must be (gh, gw) >= 1, got {tuple(grid_shape)}")
    return _psf_grid_cells(H, W, gh, gw, oh, ow, f, None if aspect is None else float(aspect), blend)


def _batched_grid(cells, B):
    """The term list of `cells` repeated for B lenses: grid b T + t reads fan b K + src[t]."""
    if B not in cells.batched:
        g, K = cells.grid, cells.n_fields
        src = (np.arange(B)[:, None] * K + g.src[None, :].astype(np.int64)).reshape(-1)
        cells.batched[B] = ops.psf_rot_grid(src, np.tile(g.c, B), np.tile(g.s, B), B * K)
    return cells.batched[B]


PSF_GRID_FUSED_BY_DEFAULT = True          # profiles/psf_grid_timing.txt


def psf_grid_from_trace(x, y, ray_ok, cells, n_bins, increment, y_target=None, fused=None):
    """The PSFs of a whole svola grid from one traced column of fields of a rotationally symmetric lens: psfs
    [B, N, ny, nx, W], ready for svola_convolution.

    x, y [B, F, P, W]: the tracer's outputs for F fields along the +y meridian (metrics.psf_from_trace takes the same);
    ray_ok the same shape or None (every ray counts); cells: psf_grid_cells(...) for F fields; n_bins = (nx, ny);
    `increment`: the pixel pitch of the sensor, required (a grid sized from the data makes no sense across cells);
    y_target [B F] or None: the centre of every field's spot, by default its ok-weighted mean y as in psf_from_trace.

    The kernel of one term (field k, rotation (c, s)) is the soft histogram of compute_psf on the FULL nx x ny grid (pixel
    centres increment (j + 1/2 - nx/2), nothing mirrored) of the field's rays turned about (0, y_target[k]):
        xi = x, eta = y - y_target[k];   x' = c xi + s eta,  y' = -s xi + c eta      (c, s: the float32 values of `cells`)
    normalised to unit sum per channel; the PSF of a cell is sum beta kernel over its terms -- normalised first, blended
    after, so that a vignetted field does not count for less.  Exact for a rotationally symmetric lens: nothing is resampled.

    `fused=False`: the definition in plain torch ops (rotate per term, the two Gaussian operands, a matmul) -- any device, any
    float dtype, and 8 (nx + ny) bytes per ray and TERM of operands.  `fused=True`: the HIP kernels of csrc/tl_psf.hip
    (ops.PsfRotAccumulateFunction): float32 on the GPU, at most 32 bins per axis; the rotation and the field lookup happen in
    the kernels' loads and nothing per ray and term is stored; anything else raises.  `fused=None` (default): the kernels when
    they apply (they are faster on the recorded workload, profiles/psf_grid_timing.txt), torch otherwise.
    Gradients flow to x and y, and to y_target when it is derived from them (or given as a tensor that requires one); the
    pitch and ray_ok carry none."""
    if x.dim() != 4 or y.shape != x.shape:
        raise ValueError(f"psf_grid_from_trace: x and y must both be [B, F, P, W], got {tuple(x.shape)} and {tuple(y.shape)}")
    B, F_, P, W = x.shape
    if F_ != cells.n_fields:
        raise ValueError(f"psf_grid_from_trace: x holds {F_} fields, the cells were laid out for {cells.n_fields}")
    nx, ny = (int(v) for v in n_bins)
    if nx < 1 or ny < 1:
        raise ValueError(f"psf_grid_from_trace: n_bins must be (nx, ny) >= 1, got {tuple(n_bins)}")
    inc = float(increment)
    applies = (x.is_cuda and y.device == x.device and x.dtype == torch.float32 and y.dtype == torch.float32
               and max(nx, ny) <= ops.PSF_MAX_BINS)
    if fused is None:
        fused = applies and PSF_GRID_FUSED_BY_DEFAULT
    if fused:
        if max(nx, ny) > ops.PSF_MAX_BINS:
            raise ValueError(f"psf_grid_from_trace(fused=True) takes at most {ops.PSF_MAX_BINS} bins per axis, got {tuple(n_bins)}")
        if not applies:
            raise RuntimeError(f"psf_grid_from_trace(fused=True): x is {x.dtype} on {x.device}; the fused PSF runs only as a HIP "
                               "kernel on float32 tensors on an AMD GPU (there is no CPU fallback): use fused=False")
    K = B * F_
    xs, ys = x.permute(0, 1, 3, 2).reshape(K, W, P), y.permute(0, 1, 3, 2).reshape(K, W, P)
    ok = None if ray_ok is None else ray_ok.permute(0, 1, 3, 2).reshape(K, W, P)
    if y_target is None:
        if ok is None:
            y_target = ys.reshape(K, -1).mean(dim=1)
        else:
            wf = ok.to(y.dtype)
            y_target = (ys * wf).reshape(K, -1).sum(dim=1) / wf.reshape(K, -1).sum(dim=1).clamp_min(1)
    else:
        y_target = torch.as_tensor(y_target, dtype=y.dtype, device=y.device).reshape(K)
    grid = _batched_grid(cells, B)
    if fused:
        hist = ops.PsfRotAccumulateFunction.apply(xs, ys, ok, grid, inc, inc, y_target, nx, ny, 0.5 - nx / 2, 0.5 - ny / 2)
    else:
        tkey = ("torch", x.device, x.dtype)
        if tkey not in grid.device_tables:                  # uploaded once per device and dtype, like the kernels' tables
            grid.device_tables[tkey] = (torch.from_numpy(grid.src.astype(np.int64)).to(x.device),
                                        torch.from_numpy(grid.c).to(device=x.device, dtype=x.dtype)[:, None, None],
                                        torch.from_numpy(grid.s).to(device=x.device, dtype=x.dtype)[:, None, None])
        src, c, s = grid.device_tables[tkey]
        xi, eta = xs[src], (ys - y_target[:, None, None])[src]                              # [G, W, P]
        xr, yr = c * xi + s * eta, c * eta - s * xi
        rng = lambda n: (torch.arange(n, dtype=x.dtype, device=x.device) + (0.5 - n / 2)) * inc       # noqa: E731
        g_x = torch.exp(-((xr[:, :, None, :] - rng(nx)[:, None]) / (inc / 2)) ** 2 / 2)      # [G, W, nx, P]
        g_y = torch.exp(-((yr[:, :, None, :] - rng(ny)[:, None]) / (inc / 2)) ** 2 / 2)      # [G, W, ny, P]
        if ok is not None:
            g_y = g_y * ok[src][:, :, None, :].to(x.dtype)
        hist = torch.matmul(g_y, g_x.transpose(-1, -2))                                      # [G, W, ny, nx]
    kern = hist / hist.sum(dim=(-1, -2), keepdim=True)
    key = (x.device, B, kern.dtype)
    if key not in cells.blend_tables:                       # uploaded once per device, batch and dtype (a captured step uploads nothing)
        cells.blend_tables[key] = (
            torch.from_numpy((np.arange(B)[:, None] * cells.N + cells.cell[None, :]).reshape(-1)).to(x.device),
            torch.from_numpy(np.tile(cells.beta, B)).to(device=x.device, dtype=kern.dtype))
    cell, beta = cells.blend_tables[key]
    assert kern.shape[0] == cell.numel()
    psfs = torch.zeros((B * cells.N, W, ny, nx), dtype=kern.dtype, device=x.device).index_add(
        0, cell, kern * beta[:, None, None, None])
    return psfs.reshape(B, cells.N, W, ny, nx).permute(0, 1, 3, 4, 2)


WARP_ALPHA = -0.75        # the cubic convolution parameter of the reference's matrix (image_ops.py:150-153)
WARP_IMAGE_GRAD_MAX_PIXELS = 1 << 26      # Ho Wo of the fixed-point image gradient (tl_warp_bwd_image)


def _warp_axis(x, n):
    """One axis of warp_bicubic in plain torch ops: the four clipped tap indices and the four weights, in the arithmetic of
    the kernel (csrc/tl_warp.hip: axis_taps).  The clamp is written with comparisons, so that x = +-1 exactly passes the
    gradient and a NaN coordinate stays NaN (torch.clamp's backward would hand a NaN coordinate a zero gradient)."""
    one = torch.ones((), dtype=x.dtype, device=x.device)
    xc = torch.where(x < -1, -one, torch.where(x > 1, one, x))
    u = (xc + 1) / 2 * (n - 1)
    fl = torch.floor(u.detach())
    t = u - fl
    j0 = torch.nan_to_num(fl, nan=0.0).to(torch.long)
    idx = [(j0 + k).clamp(0, n - 1) for k in (-1, 0, 1, 2)]
    a, tt = WARP_ALPHA, t * t
    w = [((a * t - 2 * a) * t + a) * t, ((a + 2) * t - (a + 3)) * tt + 1, ((-(a + 2) * t + (2 * a + 3)) * t - a) * t,
         (a - a * t) * tt]
    return idx, w


def _warp_torch(image, x, y, gain):
    """The definition in plain torch ops (any device, any float dtype): 16 gathers and the weight algebra around them."""
    B, H, W, _ = image.shape
    cols, wx = _warp_axis(x, W)
    rows, wy = _warp_axis(y, H)
    b = torch.arange(B, device=image.device)[:, None, None]
    out = None
    for i in range(4):
        row = None
        for j in range(4):
            term = wx[j][..., None] * image[b, rows[i], cols[j]]
            row = term if row is None else row + term
        out = wy[i][..., None] * row if out is None else out + wy[i][..., None] * row
    return out if gain is None else out * gain


def warp_bicubic(image, x, y, gain=None, fused=None, image_grad="torch"):
    """Bicubic resampling of an image at per-pixel source coordinates, times an optional gain: the distortion warp and the
    relative illumination of a rendered image (the reference's `interpolate_bicubic`, image_ops.py:109-198, which cannot run
    as written: it calls `.float()` on Python ints, sizes its output by the input's pixel count, and its `base.repeat` only
    lines up when input and output sizes agree).

    image [B, H, W, C]; x, y [B or 1, Ho, Wo] (the same shape): normalised source coordinates, -1 at the centre of the first
    column (row) and +1 at the centre of the last; gain [B or 1, Ho, Wo, C or 1] or None.  Returns [B, Ho, Wo, C].

    Per output pixel: xc = clamp(x, -1, 1), u = (xc + 1) / 2 (W - 1), j0 = floor(u), t = u - j0; the taps are the columns
    j0 - 1, j0, j0 + 1, j0 + 2, each clipped into [0, W - 1] (replicate padding); rows likewise from y and H.  The weights are
    the reference's matrix with a = -0.75, in order of the tap's offset:
        w(-1) = a (t^3 - 2 t^2 + t)            w(0) = (a + 2) t^3 - (a + 3) t^2 + 1
        w(1)  = -(a + 2) t^3 + (2a + 3) t^2 - a t      w(2) = a (t^2 - t^3)
    and out[b,yo,xo,c] = gain sum_i sum_j wy_i wx_j image[b, row_i, col_j, c].  The weights sum to 1 (constants are
    reproduced); lines are not (only a = -0.5 does that): on the ramp image[.., q, ..] = q the interior result is
    j0 + t^3 - 1.5 t^2 + 1.5 t.

    Gradients: d/dx is the derivative weights times (W - 1)/2 where -1 <= x <= 1 (x = +-1 exactly included) and zero outside;
    the interpolant is C1 across integer u, replicate edges included, and at an integer u the cell with t = 0 is used; d/dy
    likewise; d/dgain; d/dimage.  Whatever is shared (x, y or gain by the batch, gain by the channels) receives the sum over
    what shares it.  A NaN coordinate gives NaN in that output pixel and in that pixel's gradients.

    Deviations from the letter of image_ops.py:109-198: (1) the output size comes from the coordinates' shape, not from an
    `out_size` argument; (2) the coordinates are per-pixel arrays, optionally per lens, not one x and one y vector; (3) the
    integer sizes are ints; (4) the dead `out_size` and `base` bookkeeping is dropped.  PARITY UNPINNED: the text cannot run.

    `fused=False`: the definition in plain torch ops -- any device, any float dtype, autograd does the rest.  `fused=True`:
    the HIP kernels of csrc/tl_warp.hip (ops.WarpFunction): float32 tensors on one GPU, one launch forward and one backward
    for the gradients to x, y and gain; anything else raises (there is no CPU fallback).  `fused=None` (default): the kernels
    when they apply, torch otherwise.

    The gradient to the image is a scatter, and `image_grad` says who computes it when `image.requires_grad`:
    `"torch"` (default): not the kernels -- `fused=True` raises and says so, `fused=None` takes the torch path.
    `"fused"`: tl_warp_bwd_image -- `fused=True` no longer raises for it and `fused=None` takes the kernels whenever they
    apply.  Its contract: with a = g_out gain (the fp32 product), m the largest finite |a| of the call, 2^(E-1) <= m < 2^E and
    Hb = ceil(log2(16 Ho Wo)), every contribution wy_i wx_j a (an fp32 product) is rounded to a multiple of the quantum
    Q = 2^(E + Hb - 62) and added as a 64-bit integer; the result is fp32(sum Q), rounded once.  Integer sums do not depend on
    the order, so the result has the same bits in every run, for any order or grouping of the output pixels and under any
    launch plan, and scaling g_out by a power of two scales it exactly.  At most 16 Ho Wo <= 2^Hb contributions of magnitude
    <= 2^(62 - Hb) quanta reach one element, so the sum cannot overflow; this needs Ho Wo <= 2^26 (then Q <= 2^(E-32)), and
    a larger output raises a RuntimeError with `fused=True` and takes the torch path with `fused=None`.  The error is
    ABSOLUTE on the scale of the largest seed -- Q/2 per contribution, at least 2^-32 of m -- and not relative per pixel: where
    seeds of very different magnitude meet in one call, the small ones are resolved to 2^-32 of the largest.  A source pixel
    that no tap reaches gets exactly +0.0.  A non-finite a, or a NaN coordinate, is left out of m and of the sums and turns the
    elements under its 16 clipped taps into NaN; every other element keeps the bits of the clean run.
    Any other value of `image_grad` is a ValueError."""
    if image.dim() != 4:
        raise ValueError(f"warp_bicubic: image must be [B, H, W, C], got {tuple(image.shape)}")
    B, H, W, Cc = image.shape
    if x.dim() != 3 or y.shape != x.shape or x.shape[0] not in (1, B):
        raise ValueError(f"warp_bicubic: x and y must both be [B or 1, Ho, Wo] with B = {B}, got {tuple(x.shape)} and {tuple(y.shape)}")
    Ho, Wo = x.shape[1:]
    if min(B, H, W, Cc, Ho, Wo) < 1:
        raise ValueError(f"warp_bicubic: every size must be at least 1, got image {tuple(image.shape)} and x {tuple(x.shape)}")
    if gain is not None and (gain.dim() != 4 or gain.shape[0] not in (1, B) or tuple(gain.shape[1:3]) != (Ho, Wo)
                             or gain.shape[3] not in (1, Cc)):
        raise ValueError(f"warp_bicubic: gain must be [B or 1, {Ho}, {Wo}, C or 1] with B = {B}, C = {Cc}, got {tuple(gain.shape)}")
    if image_grad not in ("torch", "fused"):
        raise ValueError(f"warp_bicubic: image_grad must be 'torch' or 'fused', got {image_grad!r}")
    tensors = [t for t in (image, x, y, gain) if t is not None]
    applies = image.is_cuda and all(t.device == image.device and t.dtype == torch.float32 for t in tensors)
    needs_image_grad = image.requires_grad and torch.is_grad_enabled()
    too_large = needs_image_grad and image_grad == "fused" and Ho * Wo > WARP_IMAGE_GRAD_MAX_PIXELS
    if fused is None:
        # the kernels beat the torch path on the recorded workloads (profiles/warp_timing.txt, warp_image_grad_timing.txt)
        fused = applies and not too_large and (not needs_image_grad or image_grad == "fused")
    if not fused:
        return _warp_torch(image, x, y, gain)
    if needs_image_grad and image_grad != "fused":
        raise RuntimeError("warp_bicubic(fused=True): the image requires a gradient, and the image gradient is a scatter that is "
                           "deliberately not a kernel (it would need atomics, the first result here that is not bit-reproducible, "
                           "or a sort pass): use fused=False or fused=None, or detach the image")
    if too_large:
        raise RuntimeError(f"warp_bicubic(fused=True, image_grad='fused'): the output has {Ho} x {Wo} pixels, and the fixed-point "
                           "image gradient takes at most 2^26 (the headroom of its 64-bit sums): use fused=False")
    if not applies:
        what = ", ".join(f"{n} {t.dtype} on {t.device}" for n, t in zip(("image", "x", "y", "gain"), (image, x, y, gain)) if t is not None)
        raise RuntimeError(f"warp_bicubic(fused=True): {what}; the fused warp runs only as HIP kernels on float32 tensors on "
                           "one AMD GPU (there is no CPU fallback): use fused=False")
    return ops.WarpFunction.apply(image, x, y, gain, image_grad == "fused")


def _pixel_axes(out_size, aspect, dtype, device):
    """Normalised pixel-centre coordinates xn [Wo], yn [Ho] (-1 .. +1, 0 for a single pixel) and the relative image height
    h [Ho, Wo]: the distance from the image centre in units of the half-diagonal.  aspect = width / height (default Wo / Ho)."""
    Ho, Wo = (int(v) for v in out_size)
    if Ho < 1 or Wo < 1:
        raise ValueError(f"out_size must be (Ho, Wo) >= 1, got {tuple(out_size)}")
    lin = lambda n: torch.linspace(-1, 1, n, dtype=dtype, device=device) if n > 1 else torch.zeros(1, dtype=dtype, device=device)  # noqa: E731
    xn, yn = lin(Wo), lin(Ho)
    a = float(Wo) / float(Ho) if aspect is None else float(aspect)
    h = torch.sqrt((xn[None, :] * a) ** 2 + yn[:, None] ** 2) / (a * a + 1) ** 0.5
    return xn, yn, h


_NUMPY_FLOAT = {torch.float16: np.float16, torch.float32: np.float32, torch.float64: np.float64}


def radial_map(values, fields, out_size, v0=0.0, aspect=None):
    """A radial profile painted over the image: values [L, K] or [L, K, C], sampled at the relative fields `fields` [K]
    (ascending, > 0), become [L, Ho, Wo, C or 1] by piecewise-linear interpolation in h, the pixel's distance from the image
    centre in units of the half-diagonal (the corner pixels are at h = 1).  There is a node (0, v0) at the centre -- v0 = 0
    for distortion, 1 for relative illumination -- and the profile is held constant beyond the last field.  `aspect` is the
    image's width / height (default Wo / Ho: square pixels).  Plain torch ops, differentiable in `values`.

    `fields` given as host values (a tuple or list of numbers, a numpy array, a CPU tensor) are checked on the host and their
    device copy is cached: nothing is uploaded and nothing is read back per call, so a captured step passes host values.
    `fields` given as a tensor on another device than the CPU are checked there, which synchronises."""
    if values.dim() not in (2, 3):
        raise ValueError(f"radial_map: values must be [L, K] or [L, K, C], got {tuple(values.shape)}")
    on_device = torch.is_tensor(fields) and fields.device.type != "cpu"
    if on_device:
        f = fields.to(dtype=values.dtype, device=values.device).reshape(-1)
        K = f.numel()
    else:
        # rounded to the dtype of `values` first, as the device copy is: the check sees the numbers the interpolation uses
        host = np.asarray(fields.detach().numpy() if torch.is_tensor(fields) else fields, dtype=np.float64).reshape(-1)
        host = host.astype(_NUMPY_FLOAT.get(values.dtype, np.float64)).astype(np.float64)
        K = host.size
    if values.shape[1] != K or K < 1:
        raise ValueError(f"radial_map: values {tuple(values.shape)} hold {values.shape[1]} samples per lens, fields {K}")
    if on_device:
        ascending = bool((f > 0).all()) and bool((f[1:] > f[:-1]).all())
    else:
        ascending = bool((host > 0).all()) and bool((host[1:] > host[:-1]).all())
    if not ascending:
        raise ValueError("radial_map: fields must be ascending and > 0")
    if not on_device:
        f = const_tensor(host.tolist(), values.dtype, values.device)
    v = values if values.dim() == 3 else values[..., None]                               # [L, K, C or 1]
    _, _, h = _pixel_axes(out_size, aspect, values.dtype, values.device)
    nodes_h = torch.cat((f.new_zeros(1), f))                                             # [K + 1]
    nodes_v = torch.cat((torch.full_like(v[:, :1], float(v0)), v), dim=1)                # [L, K + 1, C or 1]
    seg = (torch.searchsorted(nodes_h, h.contiguous(), right=True) - 1).clamp(0, K - 1)  # [Ho, Wo]
    frac = ((h - nodes_h[seg]) / (nodes_h[seg + 1] - nodes_h[seg])).clamp(max=1.0)[None, :, :, None]
    lo, hi = nodes_v[:, seg], nodes_v[:, seg + 1]                                        # [L, Ho, Wo, C or 1]
    return lo + frac * (hi - lo)


def distortion_grid(d, fields, out_size, aspect=None):
    """The source coordinates that warp an ideal image into the distorted one the sensor sees: d [L, K] is the relative
    distortion (metrics.compute_distortion) at the relative fields `fields` [K] (ascending, > 0).  Returns x, y [L, Ho, Wo],

        (x, y) = (x_out, y_out) / (1 + D(h_out)),

    D the radial profile of d (radial_map with 0 at the centre), (x_out, y_out) the normalised pixel centres and h_out their
    relative image height.  This is the first-order inverse of "ideal height -> real height = ideal (1 + D(ideal))": the sensor
    pixel at the real position samples the scene at the ideal one.  The exact inverse would evaluate D at the ideal height,
    not at the real one; the difference is O(D D').  Plain torch ops, differentiable in d."""
    if d.dim() != 2:
        raise ValueError(f"distortion_grid: d must be [L, K], got {tuple(d.shape)}")
    D = radial_map(d, fields, out_size, 0.0, aspect)[..., 0]
    xn, yn, _ = _pixel_axes(out_size, aspect, d.dtype, d.device)
    return xn[None, None, :] / (1 + D), yn[None, :, None] / (1 + D)


def ssim_window(filter_size, filter_sigma, dtype=torch.float64):
    """The 1-D Gaussian window of ssim: w[i] ~ exp(-(i - (K - 1)/2)^2 / (2 sigma^2)), normalised to sum 1 in float64 and rounded
    once to `dtype` (a CPU tensor of K weights).  The 2-D window is its outer product with itself."""
    K = int(filter_size)
    i = np.arange(K, dtype=np.float64) - (K - 1) / 2.0
    w = np.exp(-(i * i) / (2.0 * float(filter_sigma) ** 2))
    return torch.from_numpy(w / w.sum()).to(dtype)


@functools.lru_cache(maxsize=64)
def _ssim_window_on(filter_size, filter_sigma, dtype, device):
    """ssim_window on `device`, uploaded once per (window, dtype, device): a captured step uploads nothing."""
    return ssim_window(filter_size, filter_sigma, dtype).to(device)


def _ssim_blur(Cc, filter_size, filter_sigma, dtype, device):
    """t [B, C, H, W] -> its VALID convolution with the 2-D window, as two 1-D grouped conv2d calls."""
    w = _ssim_window_on(int(filter_size), float(filter_sigma), dtype, torch.device(device))
    w_row = w.reshape(1, 1, 1, -1).expand(Cc, 1, 1, -1)
    w_col = w.reshape(1, 1, -1, 1).expand(Cc, 1, -1, 1)
    return lambda t: F.conv2d(F.conv2d(t, w_row, groups=Cc), w_col, groups=Cc)


def _ssim_moments(x, y, blur):
    """(x0, y0, m_a, m_b, va, vb, cab) of one level x, y [B, C, H, W]: the window means m of the centred images, the
    variances and the covariance.

    The moments are taken about each image's own mean x0, y0 per lens and channel (a constant to autograd), which the caller
    adds back to the window means: variances and covariance are shift invariant, and without the shift w*a^2 - mu_a^2
    subtracts two numbers of size mu^2 to get one of size C2 -- on two nearly equal flat images that costs even float64 four
    digits of the gradient."""
    x0, y0 = x.detach().mean(dim=(2, 3), keepdim=True), y.detach().mean(dim=(2, 3), keepdim=True)
    x, y = x - x0, y - y0
    m_a, m_b = blur(x), blur(y)
    va, vb, cab = blur(x * x) - m_a * m_a, blur(y * y) - m_b * m_b, blur(x * y) - m_a * m_b
    return x0, y0, m_a, m_b, va, vb, cab


def _ssim_torch(a, b, max_value, filter_size, filter_sigma, k1, k2):
    """The definition of ssim in plain torch ops (any device, any float dtype; autograd does the rest).  Returns
    (ssim [B], S [B, Hm, Wm, C])."""
    blur = _ssim_blur(a.shape[3], filter_size, filter_sigma, a.dtype, a.device)
    x0, y0, m_a, m_b, va, vb, cab = _ssim_moments(a.permute(0, 3, 1, 2), b.permute(0, 3, 1, 2), blur)
    mu_a, mu_b = m_a + x0, m_b + y0
    c1, c2 = (k1 * max_value) ** 2, (k2 * max_value) ** 2
    S = ((2 * mu_a * mu_b + c1) * (2 * cab + c2)) / ((mu_a * mu_a + mu_b * mu_b + c1) * (va + vb + c2))
    return S.mean(dim=(1, 2, 3)), S.permute(0, 2, 3, 1)


def _ssim_arguments(fn, a, b, filter_size, first=None, too_large=None):
    """The argument checks that ssim and ms_ssim (`fn` in the messages) share.  Returns (K, why_not): why_not names why the
    kernels do not apply, or is None.  first: the message of a fault of the caller's own that is reported before the sizes
    (ms_ssim's levels).  too_large(H, W, C): a further size that the kernels do not take; with one, the message names C."""
    if a.dim() != 4 or b.dim() != 4:
        raise ValueError(f"{fn}: a and b must be [B, H, W, C], got {tuple(a.shape)} and {tuple(b.shape)}")
    if a.shape != b.shape:
        raise ValueError(f"{fn}: a and b must have one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
    if first is not None:
        raise ValueError(first)
    K = int(filter_size)
    B, H, W, Cc = a.shape
    if K < 1 or min(B, Cc) < 1:
        raise ValueError(f"{fn}: filter_size and every size must be at least 1, got filter_size {K} and {tuple(a.shape)}")
    why_not = None
    if a.dtype != torch.float32 or b.dtype != torch.float32:
        why_not = f"dtype: a is {a.dtype}, b is {b.dtype}; the kernels are float32"
    elif not a.is_cuda or b.device != a.device:
        why_not = f"device: a is on {a.device}, b on {b.device}; the kernels run on one AMD GPU (there is no CPU fallback)"
    elif K % 2 == 0 or K < 3 or K > ops.SSIM_MAX_TAPS:
        why_not = f"K: filter_size must be odd, 3 <= filter_size <= {ops.SSIM_MAX_TAPS}, got {K}"
    elif max(H, W) > 1 << 20 or ((H + 15) // 16) * ((W + 31) // 32) > 1 << 22 or (too_large is not None and too_large(H, W, Cc)):
        size = f"{H} x {W} pixels" if too_large is None else f"{H} x {W} x {Cc}"
        why_not = f"size: {size} are more than the kernels tile"
    return K, why_not


def ssim(a, b, max_value=1.0, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03, fused=None, return_map=False):
    """The mean structural similarity of two images per lens (the reference scores its rendered image with `tf.image.ssim`,
    optics_simulator_lite.py's commented-out apply_optics_model; the defaults are tf.image.ssim's).

    a, b [B, H, W, C] of one shape.  Returns ssim [B]; with `return_map=True`, (ssim, S [B, Hm, Wm, C]).

    The 1-D window is w[i] ~ exp(-(i - (K - 1)/2)^2 / (2 sigma^2)), K = filter_size, normalised to sum 1 in float64 and rounded
    once to the working precision; the 2-D window is its outer product and the convolution is VALID, so the map has
    Hm = H - K + 1 rows and Wm = W - K + 1 columns.  With L = max_value, C1 = (k1 L)^2, C2 = (k2 L)^2:
        mu_a = w*a,  mu_b = w*b,  va = w*a^2 - mu_a^2,  vb = w*b^2 - mu_b^2,  cab = w*ab - mu_a mu_b
        S = (2 mu_a mu_b + C1)(2 cab + C2) / ((mu_a^2 + mu_b^2 + C1)(va + vb + C2)),   ssim[b] = mean of S over Hm x Wm x C.

    `fused=False`: the definition in plain torch ops -- any device, any float dtype, autograd does the rest.  `fused=True`: the
    HIP kernels of csrc/tl_ssim.hip (ops.SsimFunction): float32 tensors on one GPU, filter_size odd in 3..11, no map; one launch
    (plus a tiny reduction) forward and one launch backward per image that needs a gradient, no atomics, the same bits on every
    run; it keeps 4 bytes per map element per stored partial map (three maps for one gradient, five for both).  Anything else
    raises a ValueError that names the reason (there is no CPU fallback).  `fused=None` (default): the kernels when they
    apply, torch otherwise.  Both paths take the second moments about a constant (the torch path about each image's mean, the
    kernels about each tile's first pixel) and add it back to the means: the fp32 variances then lose digits with the local
    contrast, not with the brightness."""
    K, why_not = _ssim_arguments("ssim", a, b, filter_size)
    H, W = a.shape[1:3]
    if H < K or W < K:
        raise ValueError(f"ssim: H and W must be at least filter_size = {K} (the window is valid only), got {H} x {W}")
    if fused is None:
        fused = why_not is None and not return_map
    if not fused:
        value, S = _ssim_torch(a, b, float(max_value), K, float(filter_sigma), float(k1), float(k2))
        return (value, S) if return_map else value
    if return_map:
        raise ValueError("ssim(fused=True, return_map=True): the kernels do not keep the map S; use fused=False")
    if why_not is not None:
        raise ValueError(f"ssim(fused=True) does not apply -- {why_not}: use fused=False")
    window = tuple(float(v) for v in ssim_window(K, filter_sigma, torch.float32))
    c1, c2 = (float(k1) * float(max_value)) ** 2, (float(k2) * float(max_value)) ** 2
    return ops.SsimFunction.apply(a, b, window, c1, c2)


MS_SSIM_POWER_FACTORS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)        # tf.image.ssim_multiscale's defaults


def _ms_ssim_torch(a, b, max_value, power_factors, filter_size, filter_sigma, k1, k2):
    """The definition of ms_ssim in plain torch ops (any device, any float dtype; autograd does the rest).  Returns
    (ms_ssim [B], terms [B, C, M]).  Per level the moments are taken as in _ssim_torch, about each image's detached mean."""
    M = len(power_factors)
    blur = _ssim_blur(a.shape[3], filter_size, filter_sigma, a.dtype, a.device)
    c1, c2 = (k1 * max_value) ** 2, (k2 * max_value) ** 2
    x, y = a.permute(0, 3, 1, 2), b.permute(0, 3, 1, 2)
    terms = []
    for k in range(M):
        if k:          # the 2 x 2 mean with stride 2; the last row / column of an odd side is counted twice
            pad = (0, x.shape[3] % 2, 0, x.shape[2] % 2)
            x, y = F.avg_pool2d(F.pad(x, pad, mode="replicate"), 2), F.avg_pool2d(F.pad(y, pad, mode="replicate"), 2)
        x0, y0, m_a, m_b, va, vb, cab = _ssim_moments(x, y, blur)
        q = (2 * cab + c2) / (va + vb + c2)
        if k == M - 1:
            mu_a, mu_b = m_a + x0, m_b + y0
            q = q * (2 * mu_a * mu_b + c1) / (mu_a * mu_a + mu_b * mu_b + c1)
        terms.append(q.mean(dim=(2, 3)))
    v = torch.stack(terms, dim=2)                                                      # [B, C, M]
    p = const_tensor(list(power_factors), a.dtype, a.device)
    # where any term of a (lens, channel) is <= 0 the product is 0 and so are all its gradients: the power is taken of 1
    # there (a finite derivative, which the `where` then multiplies by 0), never of 0
    positive = (v > 0).all(dim=2, keepdim=True)
    ms = torch.where(positive[..., 0], (torch.where(positive, v, torch.ones_like(v)) ** p).prod(dim=2),
                     (v.detach().clamp(min=0) ** p).prod(dim=2))
    return ms.mean(dim=1), v.detach()


def ms_ssim_level_sizes(H, W, levels):
    """[(H_k, W_k)] of the pyramid: each level halves the one below, rounding up."""
    out = []
    for _ in range(levels):
        out.append((H, W))
        H, W = (H + 1) // 2, (W + 1) // 2
    return out


def ms_ssim(a, b, max_value=1.0, power_factors=MS_SSIM_POWER_FACTORS, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03,
            fused=None, return_terms=False):
    """The multi-scale structural similarity of two images per lens, as `tf.image.ssim_multiscale` computes it (the defaults
    are its defaults).  a, b [B, H, W, C] of one shape; M = len(power_factors), 1 <= M <= 8.  Returns ms_ssim [B]; with
    `return_terms=True`, (ms_ssim, v [B, C, M]) with v detached (a diagnostic: which level is off).

    Level 0 is the images; level k + 1 is the 2 x 2 mean of level k with stride 2, ceil(H_k / 2) x ceil(W_k / 2), the last row or
    column of an odd side counted twice.  Every level must have both sides >= filter_size (ValueError otherwise).  Per level,
    lens and channel, with window, VALID convolution, C1 and C2 as in `ssim`:
        cs_k = mean over the level's map of (2 cab + C2) / (va + vb + C2),   ssim_k = mean over the map of S
        v_k = cs_k for k < M - 1,  v_{M-1} = ssim_{M-1},   ms[b,c] = prod_k max(v_k, 0)^p_k,   ms_ssim[b] = mean_c ms[b,c].
    d ms / d v_k = p_k ms / v_k where every term of that (b, c) is > 0; if any term is <= 0, ms is 0 and all its gradients are
    exactly 0 (finite: never the NaN / inf of relu().pow() at 0).  Both paths implement this rule.

    `fused=False`: plain torch ops, any device and float dtype.  `fused=True`: the HIP kernels (ops.MsSsimFunction): float32
    tensors on one GPU, filter_size odd in 3..11; ONE C-ABI call forward for the whole pyramid and one backward per image that
    needs a gradient, no atomics, the same bits on every run.  Anything else raises a ValueError that names the reason (there
    is no CPU fallback).  `fused=None` (default): the kernels when they apply, torch otherwise."""
    power = tuple(float(p) for p in power_factors)
    M = len(power)
    levels_fault = None
    if not 1 <= M <= ops.MS_SSIM_MAX_LEVELS:
        levels_fault = f"ms_ssim: levels: power_factors must hold 1 .. {ops.MS_SSIM_MAX_LEVELS} weights, got {M}"
    K, why_not = _ssim_arguments("ms_ssim", a, b, filter_size, first=levels_fault,
                                 too_large=lambda H, W, Cc: H * W * Cc >= 1 << 31)
    H, W = a.shape[1:3]
    for k, (h, w) in enumerate(ms_ssim_level_sizes(H, W, M)):
        if h < K or w < K:
            raise ValueError(f"ms_ssim: level {k} is {h} x {w}: every level must be at least filter_size = {K} on both sides "
                             f"(the window is valid only); {H} x {W} carries fewer than {M} levels")
    if fused is None:
        fused = why_not is None
    if not fused:
        value, v = _ms_ssim_torch(a, b, float(max_value), power, K, float(filter_sigma), float(k1), float(k2))
    else:
        if why_not is not None:
            raise ValueError(f"ms_ssim(fused=True) does not apply -- {why_not}: use fused=False")
        window = tuple(float(t) for t in ssim_window(K, filter_sigma, torch.float32))
        c1, c2 = (float(k1) * float(max_value)) ** 2, (float(k2) * float(max_value)) ** 2
        value, v = ops.MsSsimFunction.apply(a, b, window, c1, c2, power)
    return (value, v) if return_terms else value


def psnr(a, b, max_value=1.0):
    """The peak signal-to-noise ratio per image, 10 log10(L^2 / mse) with mse the mean of (a - b)^2 over everything but the
    first axis and L = max_value (the other half of the reference's pair, `tf.image.psnr`).  a, b [B, ...] of one shape;
    returns [B].  Plain torch ops."""
    if a.shape != b.shape or a.dim() < 2:
        raise ValueError(f"psnr: a and b must have one shape [B, ...], got {tuple(a.shape)} and {tuple(b.shape)}")
    mse = ((a - b) ** 2).reshape(a.shape[0], -1).mean(dim=1)
    return 10.0 * torch.log10(float(max_value) ** 2 / mse)
