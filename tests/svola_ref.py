"""The independent reference of svola_convolution: a float64 restatement of the definition, slow and obviously right.

    out[b,y,x,c] = sum_n  W_n[y + oh, x + ow] / sum_m W_m[y + oh, x + ow]  *  (patch n of the padded image convolved with psf n)

np.pad(mode='symmetric'), an explicit loop over the patches, F.conv2d of each haloed slice with the flipped kernel, weights
built as full [N, Ih, Iw] maps and normalised by their sum, accumulation, crop.  Gradients come from autograd in float64.
Nothing here is shared with torchoptics_amd.imaging."""
import numpy as np
import torch
import torch.nn.functional as F


def patch_starts(size, grid, overlap):
    patch = size // grid + 2 * overlap
    start = np.round(np.linspace(0, 1, grid) * (size + 2 * overlap - patch)).astype(int)
    return start, start + patch, patch


def window_1d(patch, window_type):
    x = np.linspace(0, 1, patch + 2)[1:-1]
    return np.ones(patch) if window_type == "boxcar" else np.sin(np.pi * x) ** 2


def weight_maps(H, W, grid, overlap, window_type):
    """W_n as [N, Ih, Iw] float64 (unnormalised), and the patch corners."""
    (gh, gw), (oh, ow) = grid, overlap
    r0, r1, ph = patch_starts(H, gh, oh)
    c0, c1, pw = patch_starts(W, gw, ow)
    wr, wc = window_1d(ph, window_type), window_1d(pw, window_type)
    maps = np.zeros((gh * gw, H + 2 * oh, W + 2 * ow))
    for i in range(gh):
        for j in range(gw):
            maps[i * gw + j, r0[i]:r1[i], c0[j]:c1[j]] = np.outer(wr, wc)
    return maps, (r0, r1, c0, c1)


def n_cover(H, W, grid, overlap):
    """[H, W] ints: how many patches cover each pixel of the image."""
    maps, _ = weight_maps(H, W, grid, overlap, "boxcar")
    oh, ow = overlap
    return (maps > 0).sum(axis=0)[oh:oh + H, ow:ow + W]


def symmetric_pad(image, pr, pc):
    """[B,H,W,C] torch float64 -> padded by (pr, pc) on each side like np.pad(mode='symmetric'), differentiable: the index
    map is np.pad's own, applied to the row and column numbers."""
    H, W = image.shape[1:3]
    rows = np.pad(np.arange(H), pr, mode="symmetric")
    cols = np.pad(np.arange(W), pc, mode="symmetric")
    return image[:, torch.from_numpy(rows)][:, :, torch.from_numpy(cols)]


def svola_ref(image, overlap, psfs, grid, window_type="boxcar"):
    """image [B,H,W,C], psfs [B or 1,N,kh,kw,C] (torch; computed in float64 on the CPU) -> [B,H,W,C] float64."""
    image, psfs = image.to("cpu", torch.float64), psfs.to("cpu", torch.float64)
    B, H, W, C = image.shape
    overlap = (overlap, overlap) if isinstance(overlap, int) else tuple(overlap)
    (oh, ow), (gh, gw) = overlap, grid
    kh, kw = psfs.shape[2:4]
    a, b = kh // 2, kw // 2
    maps, (r0, r1, c0, c1) = weight_maps(H, W, grid, overlap, window_type)
    total = maps.sum(axis=0)
    assert (total[oh:oh + H, ow:ow + W] > 0).all(), "a pixel of the image lies in no patch"
    norm = torch.from_numpy(maps / np.where(total > 0, total, 1.0))
    P = symmetric_pad(image, oh + a, ow + b)
    frames = [torch.zeros((H + 2 * oh, W + 2 * ow, C), dtype=torch.float64) for _ in range(B)]
    for n in range(gh * gw):
        i, j = divmod(n, gw)
        for bi in range(B):
            k = psfs[bi if psfs.shape[0] > 1 else 0, n]                                   # [kh, kw, C]
            sl = P[bi, r0[i]:r1[i] + 2 * a, c0[j]:c1[j] + 2 * b]                          # haloed patch [ph+2a, pw+2b, C]
            res = F.conv2d(sl.permute(2, 0, 1)[None], torch.flip(k, (0, 1)).permute(2, 0, 1)[:, None], groups=C)[0]
            piece = res.permute(1, 2, 0) * norm[n, r0[i]:r1[i], c0[j]:c1[j], None]
            frames[bi] = frames[bi] + F.pad(piece, (0, 0, c0[j], W + 2 * ow - c1[j], r0[i], H + 2 * oh - r1[i]))
    return torch.stack(frames)[:, oh:oh + H, ow:ow + W]


def make_case(B, H, W, C, grid, k, seed, psf_batch=None):
    """Seeded non-negative inputs: uniform(0, 1) image and g_out, PSFs normalised to unit sum per channel (float64, CPU)."""
    g = torch.Generator().manual_seed(seed)
    image = torch.rand((B, H, W, C), generator=g, dtype=torch.float64)
    psfs = torch.rand((B if psf_batch is None else psf_batch, grid[0] * grid[1], k[0], k[1], C), generator=g, dtype=torch.float64)
    psfs = psfs / psfs.sum(dim=(2, 3), keepdim=True)
    g_out = torch.rand((B, H, W, C), generator=g, dtype=torch.float64)
    return image, psfs, g_out


def ref_with_grads(image, overlap, psfs, grid, window_type, g_out):
    """(out, g_image, g_psfs) of sum(out * g_out), all float64."""
    im = image.detach().to("cpu", torch.float64).requires_grad_(True)
    ps = psfs.detach().to("cpu", torch.float64).requires_grad_(True)
    out = svola_ref(im, overlap, ps, grid, window_type)
    (out * g_out.to("cpu", torch.float64)).sum().backward()
    return out.detach(), im.grad, ps.grad
