"""The fused spatially varying PSF convolution (tl_svola_fwd / tl_svola_bwd_psf / tl_svola_bwd_image behind
imaging.svola_convolution(fused=True)) on the GPU against tests/svola_ref.py in float64.

Tolerances are derived, not tuned.  Inputs are non-negative (uniform(0, 1), PSFs of unit sum per channel), so every sum here is
over non-negative terms and any fp32 evaluation order of m terms is within (m + 8) 2^-24 of the exact sum, relative to the sum:
    forward   per pixel   (kh kw + n_cover + 8) 2^-24 ref
    g_psfs    per tap     (ph pw + 8) 2^-24 ref          (the fp64 reduction of the partials makes the real error far smaller)
    g_image   per pixel   (4 kh kw n_cover + 8) 2^-24 ref   (4: the mirror images folded in)
With signed data the same argument bounds the error by (m + 8) 2^-24 times the sum of the terms' absolute values, which is the
reference evaluated on the absolute values of the inputs.
Every element is checked; the largest observed ratio to the bound is printed per case (lines "SVOLA-ACC ...", kept in
profiles/svola_accuracy.txt).

The shapes live in tests/svola_cases.py, whose docstring says which branch of the host code each one from 8 on exists for:
more than 96 tile rows or columns (8-12: several launches per kernel, row_base / col_base non-zero in the slot index of the
PSF backward), more than 65535 / C lenses (13-15: b0 non-zero, the reduce in several launches on an offset workspace), the
reflection at kh/2 == H (16, 17) and grids with hundreds of patches over one tile (18, 19).  Beyond the table:
    strides       cases 1-odd-hann and 3-tiles-hann with the same values arriving as permuted [B,C,H,W] tensors, as interior
                  slices of larger tensors and with the psfs of one lens expanded over the batch: the same bits, and no copy
    signs         cases 1-odd-boxcar, 4-cover3, 16 and 19 with seeded signs on image, psfs and g_out (the `w != 0` shortcut of
                  the image backward, the += of the per-patch accumulators and the fold see negative values)
    fuzz          64 seeded small geometries, of which 48 are valid, both windows alternating
    refusal       C = 65536 is refused by the C ABI before anything is launched"""
import numpy as np
import pytest
import torch

from conftest import rel_l2
import svola_cases as sc
import svola_ref as ref
from svola_cases import CASES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24

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
    print(f"SVOLA-ACC {name:21s} B={B} {H}x{W}x{Cc} grid {grid[0]}x{grid[1]} psf {kh}x{kw} overlap {ov} {win:6s}: largest "
          f"error / bound  out {r_out:.3f}  g_psfs {r_psf:.4f}  g_image {r_img:.4f}   (max cover {int(cover.max())})")
    if name == "12-both-chunked":
        _REF.pop(name)                        # the largest reference by far, and no other test uses it
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


def _bounds(H, W, grid, k, ov):
    """The three m of the module docstring in the order of _fused's results: forward [1,H,W,1], g_image [1,H,W,1], g_psfs (a
    number); and the largest cover."""
    cover = torch.from_numpy(ref.n_cover(H, W, grid, ov)).double()[None, :, :, None]
    ph, pw = H // grid[0] + 2 * ov[0], W // grid[1] + 2 * ov[1]
    return k[0] * k[1] + cover + 8, 4 * k[0] * k[1] * cover + 8, ph * pw + 8, int(cover.max())


def _views(kind, image, psfs):
    """The values of image and psfs as float32 leaves on the GPU that are not what the kernels index, and the views of them
    that are: (image leaf, image view, psfs leaf, psfs view, leaf gradient -> the view's layout for the image, for the psfs)."""
    a, p = image.float().to(DEV), psfs.float().to(DEV)
    if kind == "permuted":                       # [B,C,H,W] and [B,N,C,kh,kw] in memory
        la, lp = a.permute(0, 3, 1, 2).contiguous().requires_grad_(True), p.permute(0, 1, 4, 2, 3).contiguous().requires_grad_(True)
        return (la, la.permute(0, 2, 3, 1), lp, lp.permute(0, 1, 3, 4, 2), lambda g: g.permute(0, 2, 3, 1),
                lambda g: g.permute(0, 1, 3, 4, 2))
    if kind == "sliced":                         # the interior of larger tensors: a storage offset, rows with gaps between them
        (B, H, W, Cc), (Bp, N, kh, kw, _) = a.shape, p.shape
        cut_a = (slice(None), slice(2, 2 + H), slice(1, 1 + W), slice(1, 1 + Cc))
        cut_p = (slice(None), slice(1, 1 + N), slice(0, kh), slice(2, 2 + kw), slice(0, Cc))
        la = torch.full((B, H + 3, W + 2, Cc + 2), 7.0, device=DEV)
        lp = torch.full((Bp, N + 1, kh + 1, kw + 3, Cc + 1), 7.0, device=DEV)
        la[cut_a], lp[cut_p] = a, p
        la.requires_grad_(True), lp.requires_grad_(True)
        return la, la[cut_a], lp, lp[cut_p], lambda g: g[cut_a], lambda g: g[cut_p]
    assert kind == "expanded"                    # one lens's psfs for the whole batch: batch stride 0, psf_batch == B
    la, lp = a.requires_grad_(True), p[:1].clone().requires_grad_(True)
    return la, la, lp, lp.expand(a.shape[0], -1, -1, -1, -1), lambda g: g, lambda g: g


@pytest.mark.parametrize("kind", ["permuted", "sliced", "expanded"])
@pytest.mark.parametrize("name", ["1-odd-hann", "3-tiles-hann"])
def test_strided_views_reach_the_kernels_without_a_copy_and_give_the_contiguous_bits(im, name, kind):
    """A kernel's order of arithmetic does not depend on the strides, so output and gradients are compared bit for bit with the
    run on contiguous tensors of the same values.  With expanded psfs autograd sums the per-lens PSF gradients in fp32: that
    sum is held to the reference with shared psfs, B more roundings allowed."""
    from torchoptics_amd import ops
    B, H, W, Cc, grid, k, ov, win, _ = CASES[name]
    image, psfs, g_out = _case(name)[:3]
    if kind == "expanded":
        psfs = psfs[:1].expand(B, -1, -1, -1, -1)
    want = _fused(im, image, psfs.contiguous(), g_out, ov, grid, win)
    la, va, lp, vp, pick_a, pick_p = _views(kind, image, psfs)
    assert not vp.is_contiguous() or B == 1, "the case must hand over psfs that are not contiguous"
    if kind == "expanded":
        assert vp.shape[0] == B and (vp.stride(0) == 0 or B == 1) and vp.data_ptr() == lp.data_ptr()
    else:
        assert not va.is_contiguous()
    if kind == "sliced":
        assert va.storage_offset() > 0 and vp.storage_offset() > 0 and va.stride(1) > W * va.stride(2)
    out = im.svola_convolution(va, ov, vp, grid, win, fused=True)
    assert ops.svola_counts()["psfs_ptr"] == vp.data_ptr(), "the psfs view must reach the kernel as it is"
    for saved, view in zip(out.grad_fn.saved_tensors, (va, vp)):          # what the backward kernels will index
        assert saved.data_ptr() == view.data_ptr() and saved.stride() == view.stride(), "the view must reach the kernel as it is"
    (out * g_out.float().to(DEV)).sum().backward()
    assert torch.equal(out.detach(), want[0]), "output"
    assert torch.equal(pick_a(la.grad), want[1]), "image gradient"
    if kind != "expanded":
        assert torch.equal(pick_p(lp.grad), want[2]), "PSF gradient"
        return
    gp64 = ref.ref_with_grads(image, ov, psfs[:1], grid, win, g_out)[2]
    ph, pw = H // grid[0] + 2 * ov[0], W // grid[1] + 2 * ov[1]
    r_psf = _ratio(lp.grad, gp64, ph * pw + B + 8)
    print(f"SVOLA-ACC {name + '/expanded':21s} B={B} psfs [1,N,...] expanded over the batch, g_psfs summed by autograd: largest "
          f"error / bound  g_psfs {r_psf:.4f}")
    assert r_psf <= 1, (name, r_psf)


@pytest.mark.parametrize("name", ["1-odd-boxcar", "4-cover3", "16-halo-is-image", "19-crowded"])
def test_signed_data_within_the_bound_on_the_absolute_values(im, name):
    """Image, psfs (not renormalised) and g_out with seeded signs: |got - ref(signed)| <= m 2^-24 ref(|inputs|) at every element,
    m as for the unsigned case, whose reference is ref(|inputs|)."""
    B, H, W, Cc, grid, k, ov, win, pb = CASES[name]
    image, psfs, g_out, *ref_abs = _case(name)
    g = torch.Generator().manual_seed(1000 + len(name))
    image, psfs, g_out = (t * (2.0 * torch.randint(0, 2, t.shape, generator=g) - 1.0) for t in (image, psfs, g_out))
    ref_signed = ref.ref_with_grads(image, ov, psfs, grid, win, g_out)
    got = _fused(im, image, psfs, g_out, ov, grid, win)
    *bounds, cover = _bounds(H, W, grid, k, ov)
    ratios = []
    for have, want, scale, bound in zip(got, ref_signed, ref_abs, bounds):
        have = have.double().cpu()
        assert have.shape == want.shape and torch.isfinite(have).all() and (scale > 0).all() and (want < 0).any()
        ratios.append(float(((have - want).abs() / (torch.as_tensor(bound, dtype=torch.float64) * U * scale)).max()))
    print(f"SVOLA-ACC {name + '/signed':21s} B={B} {H}x{W}x{Cc} grid {grid[0]}x{grid[1]} psf {k[0]}x{k[1]} overlap {ov} {win:6s}: largest "
          f"error / bound on |inputs|  out {ratios[0]:.3f}  g_psfs {ratios[2]:.4f}  g_image {ratios[1]:.4f}   (max cover {cover})")
    assert max(ratios) <= 1, (name, ratios)


def test_seeded_fuzz_over_small_geometries(im):
    """64 seeded draws of (H, W, grid, PSF, overlap, B, C), the windows alternating; the valid ones against the reference with
    the bounds of the parametrised test.  The cap on the skipped draws keeps the test from passing on nothing."""
    kept, skipped = sc.fuzz_survivors(im.svola_geometry)
    assert skipped <= sc.FUZZ_MAX_SKIPPED, f"{skipped} of {sc.FUZZ_DRAWS} draws skipped"
    worst, failed, covers = (0.0, None, ""), [], []
    for t, (B, H, W, Cc, grid, k, ov, win) in kept:
        image, psfs, g_out = (x.float().double() for x in ref.make_case(B, H, W, Cc, grid, k, seed=t))
        want = ref.ref_with_grads(image, ov, psfs, grid, win, g_out)
        got = _fused(im, image, psfs, g_out, ov, grid, win)
        *bounds, cover = _bounds(H, W, grid, k, ov)
        ratios = [_ratio(a, b, m) for a, b, m in zip(got, want, bounds)]
        covers.append(cover)
        for what, r in zip(("out", "g_image", "g_psfs"), ratios):
            if r > worst[0]:
                worst = (r, (t, B, H, W, Cc, grid, k, ov, win), what)
        if max(ratios) > 1:
            failed.append(((t, B, H, W, Cc, grid, k, ov, win), ratios))
    print(f"SVOLA-ACC {'fuzz':21s} {len(kept)} of {sc.FUZZ_DRAWS} draws (seed {sc.FUZZ_SEED}), max cover {max(covers)}, "
          f"{sum(c > 4 for c in covers)} with cover > 4: largest error / bound {worst[0]:.3f} ({worst[2]}) at draw, B, H, W, C, grid, "
          f"psf, overlap, window = {worst[1]}")
    assert not failed, failed


def test_more_channels_than_one_launch_takes_are_refused_before_any_launch(im):
    """C = 65536 cannot be a launch's grid z even for one lens: the C ABI says so and nothing runs."""
    from torchoptics_amd import ops
    image = torch.ones((1, 1, 1, 65536), dtype=torch.float32, device=DEV)
    psfs = torch.ones((1, 1, 1, 1, 65536), dtype=torch.float32, device=DEV)
    before = ops.svola_counts()
    with pytest.raises(RuntimeError, match=r"tl_svola_fwd failed \(code -1\): tl_svola_fwd: B, H, W, C must be >= 1, C <= 65535"):
        im.svola_convolution(image, 0, psfs, (1, 1), fused=True)
    assert ops.svola_counts() == before
    out = im.svola_convolution(image[..., :65535], 0, psfs[..., :65535], (1, 1), fused=True)       # one channel fewer runs
    assert torch.equal(out, image[..., :65535])


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
