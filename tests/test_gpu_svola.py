"""The fused spatially varying PSF convolution (tl_svola_fwd / tl_svola_bwd_psf / tl_svola_bwd_image behind
imaging.svola_convolution(fused=True)) on the GPU against tests/svola_ref.py in float64.

Tolerances are derived, not tuned.  Inputs are non-negative (uniform(0, 1), PSFs of unit sum per channel), so every sum here is
over non-negative terms and any fp32 evaluation order of m terms is within (m + 8) 2^-24 of the exact sum, relative to the sum:
    forward   per pixel   (kh kw + n_cover + 8) 2^-24 ref
    g_psfs    per tap     (ph pw + 8) 2^-24 ref          (the fp64 reduction of the partials makes the real error far smaller)
    g_image   per pixel   (4 kh kw n_cover + 8) 2^-24 ref   (4: the mirror images folded in)
Every element is checked; the largest observed ratio to the bound is printed per case (lines "SVOLA-ACC ...", kept in
profiles/svola_accuracy.txt)."""
import numpy as np
import pytest
import torch

from conftest import rel_l2
import svola_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24

# B, H, W, C, grid, PSF, overlap, window, psf_batch
CASES = {
    "1-odd-boxcar": (2, 23, 29, 2, (2, 3), (5, 3), (2, 3), "boxcar", None),
    "1-odd-hann": (2, 23, 29, 2, (2, 3), (5, 3), (2, 3), "hann", None),
    "2-taps31": (1, 40, 40, 1, (1, 2), (31, 31), (0, 4), "boxcar", None),
    "3-tiles-hann": (1, 70, 131, 3, (3, 4), (7, 7), (5, 5), "hann", None),
    "4-cover3": (1, 24, 24, 1, (4, 4), (3, 3), (5, 5), "boxcar", None),
    "5-shared-psfs": (3, 23, 29, 2, (2, 3), (5, 3), (2, 3), "hann", 1),
    "6-degenerate": (1, 8, 8, 1, (1, 1), (1, 1), (0, 0), "boxcar", None),
}
_REF = {}


@pytest.fixture(scope="module")
def im():
    from torchoptics_amd import _lib, imaging
    _lib.lib()
    return imaging


def _case(name):
    """Inputs (float32 values as float64 CPU tensors) and the float64 reference of one case: computed once, never changed."""
    if name not in _REF:
        B, H, W, Cc, grid, k, ov, win, pb = CASES[name]
        image, psfs, g_out = (t.float().double() for t in ref.make_case(B, H, W, Cc, grid, k, seed=len(name), psf_batch=pb))
        _REF[name] = (image, psfs, g_out) + ref.ref_with_grads(image, ov, psfs, grid, win, g_out)
    return _REF[name]


def _fused(im, image, psfs, g_out, ov, grid, win, image_grad=True):
    a = image.float().to(DEV).requires_grad_(image_grad)
    p = psfs.float().to(DEV).requires_grad_(True)
    out = im.svola_convolution(a, ov, p, grid, win, fused=True)
    (out * g_out.float().to(DEV)).sum().backward()
    return out.detach(), a.grad, p.grad


def _ratio(got, want, bound):
    """max over ALL elements of |got - want| / (bound * want)."""
    got, want = got.double().cpu(), want.double()
    assert got.shape == want.shape and torch.isfinite(got).all() and (want > 0).all()
    return float(((got - want).abs() / (torch.as_tensor(bound, dtype=torch.float64) * U * want)).max())


@pytest.mark.parametrize("name", list(CASES))
def test_values_and_both_gradients_against_the_reference_and_twice_the_same_bits(im, name):
    B, H, W, Cc, grid, (kh, kw), ov, win, pb = CASES[name]
    image, psfs, g_out, out64, gi64, gp64 = _case(name)
    out, g_image, g_psfs = _fused(im, image, psfs, g_out, ov, grid, win)
    again = _fused(im, image, psfs, g_out, ov, grid, win)
    for a, b in zip((out, g_image, g_psfs), again):
        assert torch.equal(a, b), "two runs must give the same bits"
    cover = torch.from_numpy(ref.n_cover(H, W, grid, ov)).double()[None, :, :, None]
    ph, pw = H // grid[0] + 2 * ov[0], W // grid[1] + 2 * ov[1]
    r_out = _ratio(out, out64, kh * kw + cover + 8)
    r_psf = _ratio(g_psfs, gp64, ph * pw + 8)
    r_img = _ratio(g_image, gi64, 4 * kh * kw * cover + 8)
    print(f"SVOLA-ACC {name:15s} B={B} {H}x{W}x{Cc} grid {grid[0]}x{grid[1]} psf {kh}x{kw} overlap {ov} {win:6s}: largest "
          f"error / bound  out {r_out:.3f}  g_psfs {r_psf:.4f}  g_image {r_img:.4f}   (max cover {int(cover.max())})")
    assert r_out <= 1 and r_psf <= 1 and r_img <= 1, (name, r_out, r_psf, r_img)


def test_channel_major_psfs_reach_the_kernel_without_a_copy(im):
    """Case 7: shape 1 with psfs given as the permuted view of a channel-major [N, C, kh, kw] tensor (compute_psf's layout)."""
    from torchoptics_amd import ops
    B, H, W, Cc, grid, (kh, kw), ov, win, _ = CASES["1-odd-hann"]
    image, _, g_out = _case("1-odd-hann")[:3]
    psfs = ref.make_case(1, H, W, Cc, grid, (kh, kw), seed=7, psf_batch=1)[1].float().double()          # [1, N, kh, kw, C]
    out64, gi64, gp64 = ref.ref_with_grads(image, ov, psfs, grid, win, g_out)
    base = psfs[0].permute(0, 3, 1, 2).contiguous().float().to(DEV).requires_grad_(True)               # [N, C, kh, kw]
    view = im.psf_grid_from_fields(base, grid)
    assert view.data_ptr() == base.data_ptr() and not view.is_contiguous()
    a = image.float().to(DEV).requires_grad_(True)
    out = im.svola_convolution(a, ov, view, grid, win, fused=True)
    assert ops.svola_counts()["psfs_ptr"] == base.data_ptr(), "the strided view must reach the kernel as it is"
    (out * g_out.float().to(DEV)).sum().backward()
    cover = torch.from_numpy(ref.n_cover(H, W, grid, ov)).double()[None, :, :, None]
    ph, pw = H // grid[0] + 2 * ov[0], W // grid[1] + 2 * ov[1]
    r_out = _ratio(out.detach(), out64, kh * kw + cover + 8)
    r_psf = _ratio(base.grad.permute(0, 2, 3, 1)[None], gp64, ph * pw + 8)
    r_img = _ratio(a.grad, gi64, 4 * kh * kw * cover + 8)
    print(f"SVOLA-ACC 7-channel-major  B={B} {H}x{W}x{Cc} shared psfs as a [N,C,kh,kw] view: largest error / bound  out {r_out:.3f}  "
          f"g_psfs {r_psf:.4f}  g_image {r_img:.4f}")
    assert r_out <= 1 and r_psf <= 1 and r_img <= 1


def _delta(N, kh, kw, Cc, i, j):
    psfs = torch.zeros((1, N, kh, kw, Cc), dtype=torch.float32, device=DEV)
    psfs[:, :, i, j, :] = 1.0
    return psfs


@pytest.mark.parametrize("win", ["boxcar", "hann"])
def test_analytic_pins_through_the_kernels(im, win):
    B, H, W, Cc, grid, (kh, kw), ov = 2, 23, 29, 2, (2, 3), (5, 3), (2, 3)
    a, b = kh // 2, kw // 2
    image = ref.make_case(B, H, W, Cc, grid, (kh, kw), seed=5)[0].float().to(DEV)
    cover = torch.from_numpy(ref.n_cover(H, W, grid, ov)).to(DEV)[None, :, :, None]
    single = (cover == 1).expand_as(image)
    shifted = torch.cat((image[:, :1], image[:, :-1]), dim=1)
    for tap, want in (((a, b), image), ((a + 1, b), shifted)):        # the image; the image one row down (symmetric top edge)
        out = im.svola_convolution(image, ov, _delta(6, kh, kw, Cc, *tap), grid, win, fused=True)
        if win == "boxcar":
            assert torch.equal(out[single], want[single]), "one covering patch, boxcar: bit for bit"
        assert ((out - want).abs() <= (cover + 2) * U * want).all()
    psfs = ref.make_case(1, H, W, Cc, grid, (kh, kw), seed=6, psf_batch=1)[1].float().to(DEV)
    psfs = psfs / psfs.sum(dim=(2, 3), keepdim=True)
    out = im.svola_convolution(torch.full_like(image, 0.75), ov, psfs, grid, win, fused=True)
    assert ((out - 0.75).abs() <= (kh * kw + cover + 8 + kh * kw) * U * 0.75).all()     # (+ kh kw: the fp32 PSF's own unit sum)
    geo = im.svola_geometry(H, W, *grid, *ov, win)
    y, x = int(geo.r0[1]) - ov[0] + geo.ph // 2 + 2, int(geo.c0[1]) - ov[1] + geo.pw // 2
    assert bool((cover[0, y - a:y + a + 1, x - b:x + b + 1, 0] == 1).all())
    point = torch.zeros_like(image)
    point[:, y, x, :] = 1.0
    out = im.svola_convolution(point, ov, psfs, grid, win, fused=True)
    spot = out[:, y - a:y + a + 1, x - b:x + b + 1, :]
    assert ((spot - psfs[:, 4]).abs() <= 3 * U * psfs[:, 4]).all(), "a point of light becomes the PSF of its patch"
    assert not torch.allclose(spot, psfs[:, 4].flip(1, 2), atol=1e-3), "... not its mirror image"


def test_the_image_backward_is_launched_only_when_the_image_needs_a_gradient(im):
    from torchoptics_amd import ops
    B, H, W, Cc, grid, k, ov, win, _ = CASES["1-odd-hann"]
    image, psfs, g_out = _case("1-odd-hann")[:3]
    before = ops.svola_counts()
    out, g_image, g_psfs = _fused(im, image, psfs, g_out, ov, grid, win, image_grad=False)
    mid = ops.svola_counts()
    assert g_image is None and g_psfs is not None
    assert (mid["fwd"], mid["bwd_psf"], mid["bwd_image"]) == (before["fwd"] + 1, before["bwd_psf"] + 1, before["bwd_image"])
    _fused(im, image, psfs, g_out, ov, grid, win, image_grad=True)
    after = ops.svola_counts()
    assert (after["bwd_psf"], after["bwd_image"]) == (mid["bwd_psf"] + 1, mid["bwd_image"] + 1)
    a = image.float().to(DEV).requires_grad_(True)                       # psfs without a gradient: only the image backward
    im.svola_convolution(a, ov, psfs.float().to(DEV), grid, win, fused=True).sum().backward()
    last = ops.svola_counts()
    assert (last["bwd_psf"], last["bwd_image"]) == (after["bwd_psf"], after["bwd_image"] + 1) and a.grad is not None
    dflt = im.svola_convolution(a.detach(), ov, psfs.float().to(DEV), grid, win)         # fused=None on the GPU
    assert torch.equal(dflt, im.svola_convolution(a.detach(), ov, psfs.float().to(DEV), grid, win, fused=True))


def test_leaf_gradients_through_trace_psf_and_convolution():
    """Cooke triplet, 16 x 16 circular pupil, 3 fields, 3 wavelengths -> psf_from_trace(fused=True) -> a 3 x 1 grid ->
    svola_convolution of a 30 x 20 x 3 chart -> sum of squares; fused against fused=False in the svola step only."""
    import torchoptics_amd as ta
    import yaml_free_lenses as L
    chart = torch.rand((1, 30, 20, 3), generator=torch.Generator().manual_seed(3)).to(DEV)
    got = {}
    for fused in (False, True):
        lens, specs, leaves = L.build("cooke", DEV, epd=8.578)
        tr = ta.RayTracer(mode="circular", n_rays=(16, 16), rel_fields=(0., 0.7, 1.0), wavelengths=("C", "d", "F"),
                          default_device=DEV)
        x, y, cx, cy, ok, back = tr.trace_rays(specs, lens)
        kernels = ta.metrics.psf_from_trace(x, y, ok, n_bins=(9, 9), increment=0.004, fused=True)[3]
        psfs = ta.imaging.psf_grid_from_fields(kernels, (3, 1))
        out = ta.imaging.svola_convolution(chart, 4, psfs, (3, 1), "hann", fused=fused)
        (out ** 2).sum().backward()
        got[fused] = {n: leaves[n].grad.cpu().numpy() for n in ("c", "t")}
    for n in ("c", "t"):
        e = rel_l2(got[True][n], got[False][n])
        print(f"SVOLA-ACC leaf gradient {n} through trace -> PSF -> convolution: fused vs torch rel-L2 {e:.3e}")
        assert np.isfinite(got[True][n]).all() and np.linalg.norm(got[False][n]) > 0
        assert e <= 1e-5, (n, e)
