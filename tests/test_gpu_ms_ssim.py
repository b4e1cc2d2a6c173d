"""The fused MS-SSIM (tl_ms_ssim_fwd / tl_ms_ssim_bwd behind imaging.ms_ssim(fused=True)) on the GPU against tests/ms_ssim_ref.py
in float64.

The cases, the error measures and the bounds live in tests/ms_ssim_cases.py; tests/test_ms_ssim_cpu.py holds the bounds to be
sufficient and sharp.  Per case the fused and the torch float32 errors are printed next to the bound (lines "MSSSIM-ACC ...",
kept in profiles/ms_ssim_accuracy.txt).  Beyond the table:
    needs        only a, only b and both requiring a gradient: the same bits for everything they share, one backward call per
                 image that needs a gradient (ops.ms_ssim_counts()), and ops.ssim_counts() does not move
    twice        every case is run twice for the same bits
    negative     b = L - a: value exactly 0, both gradients exactly 0 and finite
    strided      a channel slice and a transposed view reach the kernel uncopied and give the bits of the dense run
    many lenses  B = 65 537, one more launch than grid y holds: the bits of the same lenses in two smaller batches
    refusals     fused=True with float64 images or a window of 13 taps; nine levels
    chain        svola_convolution -> warp_bicubic -> 1 - ms_ssim: the gradient on the PSFs against the float64 torch chain"""
import numpy as np
import pytest
import torch

import ms_ssim_cases as mc
from ms_ssim_ref import ms_ssim_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("value", "terms", "g_a", "g_b")


@pytest.fixture(scope="module")
def im():
    from torchoptics_amd import _lib, imaging
    _lib.lib()
    return imaging


def _line(name, tag, err, bnd):
    cells = "  ".join(f"{k} {e:.2e} / {b:.2e}" for k, e, b in zip(KEYS, err, bnd))
    return f"MSSSIM-ACC {name:16s} {tag:6s} error / bound  {cells}"


@pytest.mark.parametrize("name", mc.BOUNDED)
def test_value_terms_and_gradients_within_the_bound_for_every_needs_setting_and_twice_the_same_bits(im, name):
    from torchoptics_amd import ops
    single = ops.ssim_counts()
    before = ops.ms_ssim_counts()
    both, again = mc.run(im, name, DEV, torch.float32, True), mc.run(im, name, DEV, torch.float32, True)
    middle = ops.ms_ssim_counts()
    only_a = mc.run(im, name, DEV, torch.float32, True, needs=("a",))
    only_b = mc.run(im, name, DEV, torch.float32, True, needs=("b",))
    after = ops.ms_ssim_counts()
    assert (middle["fwd"] - before["fwd"], middle["bwd"] - before["bwd"]) == (2, 4), "one forward; one backward call per image"
    assert (after["fwd"] - middle["fwd"], after["bwd"] - middle["bwd"]) == (2, 2)
    assert ops.ssim_counts() == single, "ms_ssim does not go through SsimFunction"
    for key in KEYS:
        assert np.array_equal(both[key], again[key]), f"{key}: two runs must give the same bits"
    assert only_a["g_b"] is None and only_b["g_a"] is None
    for key in ("value", "terms"):
        assert np.array_equal(only_a[key], both[key]) and np.array_equal(only_b[key], both[key]), key
    assert np.array_equal(only_a["g_a"], both["g_a"]) and np.array_equal(only_b["g_b"], both["g_b"])
    err, bnd = mc.errors(name, *(both[k] for k in KEYS)), mc.bounds(name)
    print(_line(name, "fused", err, bnd))
    assert all(np.isfinite(e) and e <= b for e, b in zip(err, bnd)), (name, err, bnd)


@pytest.mark.parametrize("name", mc.BOUNDED)
def test_the_torch_float32_path_on_the_gpu_stays_within_the_same_bounds(im, name):
    got = mc.run(im, name, DEV, torch.float32, False)
    err, bnd = mc.errors(name, *(got[k] for k in KEYS)), mc.bounds(name)
    print(_line(name, "torch", err, bnd))
    assert all(e <= b for e, b in zip(err, bnd)), (name, err, bnd)


def test_the_default_takes_the_kernels_and_no_gradient_needs_no_backward(im):
    from torchoptics_amd import ops
    name = "map_16x32"
    before = ops.ms_ssim_counts()
    got = mc.run(im, name, DEV, torch.float32, None)
    after = ops.ms_ssim_counts()
    assert (after["fwd"], after["bwd"]) == (before["fwd"] + 1, before["bwd"] + 2), "fused=None on float32 GPU tensors is the kernels"
    a, b, _, par = mc.case_inputs(name)
    ta, tb = mc.as_tensor(a, "dense", torch.float32, DEV), mc.as_tensor(b, "dense", torch.float32, DEV)
    value = im.ms_ssim(ta, tb, **par)
    assert not value.requires_grad
    assert (ops.ms_ssim_counts()["fwd"], ops.ms_ssim_counts()["bwd"]) == (after["fwd"] + 1, after["bwd"])
    assert np.array_equal(value.cpu().numpy(), got["value"]), "keeping the maps does not change the value"


def test_a_negative_term_gives_exact_zeros(im):
    ref = mc.reference("negative")
    assert ref["terms"].min() < 0
    for fused in (True, False):
        got = mc.run(im, "negative", DEV, torch.float32, fused)
        assert np.abs(got["terms"] - ref["terms"]).max() <= 1e-5, fused
        for key in ("value", "g_a", "g_b"):
            assert np.all(np.isfinite(got[key])) and np.all(got[key] == 0), (fused, key)


@pytest.mark.parametrize("name", ["channel_slice", "transposed"])
def test_strided_views_reach_the_kernel_uncopied_and_give_the_bits_of_the_dense_run(im, name):
    from torchoptics_amd import ops
    a, b, seed, par = mc.case_inputs(name)
    layout = mc.CASES[name][9]
    ta, tb = mc.as_tensor(a, layout, torch.float32, DEV), mc.as_tensor(b, layout, torch.float32, DEV)
    assert not ta.is_contiguous() and not tb.is_contiguous()
    ta.requires_grad_(True)
    tb.requires_grad_(True)
    value = im.ms_ssim(ta, tb, fused=True, **par)
    seen = ops.ms_ssim_counts()
    assert (seen["a_ptr"], seen["b_ptr"]) == (ta.data_ptr(), tb.data_ptr())
    value.backward(torch.from_numpy(seed).to(dtype=torch.float32, device=DEV))
    da, db = mc.as_tensor(a, "dense", torch.float32, DEV).requires_grad_(True), mc.as_tensor(b, "dense", torch.float32, DEV).requires_grad_(True)
    dense = im.ms_ssim(da, db, fused=True, **par)
    dense.backward(torch.from_numpy(seed).to(dtype=torch.float32, device=DEV))
    assert torch.equal(value, dense) and torch.equal(ta.grad, da.grad) and torch.equal(tb.grad, db.grad)


def test_more_lenses_than_one_launch_takes_give_the_bits_of_two_smaller_batches(im):
    """B = 65 537 > 65 535 (grid y): every launch of the pyramid is cut in two.  Lenses are independent, so the result must
    have the bits of the same lenses run as two batches that fit one launch each."""
    B, cut = 65537, 40000
    g = torch.Generator(device=DEV).manual_seed(11)
    a = torch.rand((B, 6, 7, 1), generator=g, device=DEV)
    b = (a + 0.1 * torch.rand((B, 6, 7, 1), generator=g, device=DEV)).clamp(0, 1)
    seed = torch.rand(B, generator=g, device=DEV) - 0.5

    def run(lo, hi):
        ta, tb = a[lo:hi].clone().requires_grad_(True), b[lo:hi].clone().requires_grad_(True)
        value, v = im.ms_ssim(ta, tb, filter_size=3, power_factors=(0.4, 0.6), fused=True, return_terms=True)
        value.backward(seed[lo:hi])
        return value.detach(), v, ta.grad, tb.grad

    whole, parts = run(0, B), [run(0, cut), run(cut, B)]
    for k in range(4):
        assert torch.equal(whole[k], torch.cat([p[k] for p in parts])), k
    assert bool(torch.isfinite(whole[0]).all()) and float(whole[2][-1].abs().max()) > 0


def test_fused_refuses_float64_a_window_of_13_taps_and_nine_levels(im):
    a = torch.rand(1, 40, 40, 3, device=DEV)
    two = dict(power_factors=(0.5, 0.5))
    with pytest.raises(ValueError, match="dtype"):
        im.ms_ssim(a.double(), a.double(), fused=True, **two)
    with pytest.raises(ValueError, match="K"):
        im.ms_ssim(a, a, filter_size=13, fused=True, **two)
    with pytest.raises(ValueError, match="levels"):
        im.ms_ssim(a, a, filter_size=3, power_factors=(0.1,) * 9, fused=True)
    assert im.ms_ssim(a.double(), a.double(), **two).dtype == torch.float64, "fused=None falls to the torch path for float64"


def test_one_step_through_blur_and_warp_into_one_minus_ms_ssim_gives_the_torch_paths_gradients_on_the_psfs(im):
    """svola_convolution -> warp_bicubic(image_grad='fused') -> 1 - ms_ssim (K = 5, M = 3), gradient to the PSFs.  Reference:
    the same chain in torch ops in float64.  Bound, as for the ssim chain: 4 x the float32 torch chain's error on the same GPU,
    with the floor 16 eps32 x (the size of the terms that cancel in d ms_ssim / d rendered) / (its largest element), from
    ms_ssim_ref on the float64 rendering: the two linear adjoints behind it add many such elements with weights below 1."""
    H, W, Cc, gh, gw, k = 48, 64, 3, 2, 2, 5
    par = dict(filter_size=5, power_factors=mc.power(3))
    rng = np.random.RandomState(7)
    y, x = np.mgrid[0:H, 0:W]
    chart = (0.5 + 0.4 * np.sign(np.sin(0.5 * x) * np.sin(0.4 * y)))[None, :, :, None] * np.array([1.0, 0.9, 0.8]) + 0.02 * rng.rand(1, H, W, Cc)
    psf = rng.rand(1, gh * gw, k, k, Cc) + 0.2
    psf /= psf.sum(axis=(2, 3), keepdims=True)
    gx, gy = np.meshgrid(np.linspace(-1, 1, W), np.linspace(-1, 1, H))
    r2 = gx * gx + gy * gy
    xs, ys = (gx * (1 - 0.03 * r2))[None], (gy * (1 - 0.03 * r2))[None]

    def chain(dtype, fused):
        t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dtype=dtype, device=DEV)        # noqa: E731
        psfs = t(psf).requires_grad_(True)
        blurred = im.svola_convolution(t(chart), 4, psfs, (gh, gw), "hann", fused=fused)
        rendered = im.warp_bicubic(blurred, t(xs), t(ys), None, fused=fused, image_grad="fused" if fused else "torch")
        loss = 1 - im.ms_ssim(rendered, t(chart), fused=fused, **par).mean()
        loss.backward()
        return loss.detach().cpu().numpy(), psfs.grad.cpu().numpy(), rendered.detach().cpu().numpy()

    _, g64, rendered64 = chain(torch.float64, False)
    _, g32, _ = chain(torch.float32, False)
    _, gk, _ = chain(torch.float32, True)
    assert np.isfinite(gk).all() and np.abs(gk).max() > 0
    r = ms_ssim_ref(rendered64, chart, seed=-np.ones(1), **par)
    assert r["terms"].min() >= mc.MIN_TERM
    floor = 16 * mc.EPS32 * float(np.max(r["cond_a"])) / float(np.max(np.abs(r["g_a"])))
    top = np.abs(g64).max()
    e32, ek = np.abs(g32 - g64).max() / top, np.abs(gk - g64).max() / top
    bound = max(mc.MARGIN * e32, floor)
    print(f"MSSSIM-ACC chain            d loss / d psfs: fused {ek:.2e}, torch float32 {e32:.2e}, bound {bound:.2e}")
    assert ek <= bound, (ek, e32, bound)
