"""
Rendering an image through the lens: the spatially varying overlap-add convolution of an image with a grid of PSFs (the
reference's `svola_convolution`, image_ops.py:6-98, which cannot run as written: `fft` is undefined, `F.pad(mode='symmetric')`
and `torch.nn.functional.resize_with_crop_or_pad` do not exist in torch, and it transforms over (C, H) instead of (H, W)).

The definition implemented here is the evident intent of that text; see `svola_convolution`.
"""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from . import ops


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
    tab_r = torch.from_numpy(geo.tab_r).to(device=image.device, dtype=image.dtype)
    tab_c = torch.from_numpy(geo.tab_c).to(device=image.device, dtype=image.dtype)
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
    copies N small kernels unless the map is the identity."""
    gh, gw = (int(v) for v in grid_shape)
    if kernels.dim() != 4:
        raise ValueError("psf_grid_from_fields: kernels must be [n_fields, C, kh, kw]")
    if index_map is not None:
        idx = torch.as_tensor(index_map, dtype=torch.long).reshape(-1)
        if idx.numel() != gh * gw:
            raise ValueError(f"psf_grid_from_fields: index_map must hold {gh} x {gw} entries")
        if int(idx.min()) < 0 or int(idx.max()) >= kernels.shape[0]:
            raise ValueError("psf_grid_from_fields: index_map names a field that does not exist")
        if not (idx.numel() == kernels.shape[0] and bool((idx == torch.arange(idx.numel())).all())):
            kernels = kernels.index_select(0, idx.to(kernels.device))
    elif kernels.shape[0] != gh * gw:
        raise ValueError(f"psf_grid_from_fields: {kernels.shape[0]} fields do not fill a {gh} x {gw} grid (give an index_map)")
    return kernels.permute(0, 2, 3, 1).unsqueeze(0)
