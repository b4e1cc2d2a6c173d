"""The fused SSIM (tl_ssim_fwd / tl_ssim_bwd behind imaging.ssim(fused=True)) on the GPU against tests/ssim_ref.py in float64.

The cases, the error measures and the bounds live in tests/ssim_cases.py, whose docstring says what each shape exists for and
where the bounds come from; tests/test_ssim_cpu.py holds the bounds to be sufficient and sharp.  Per case the fused and the
torch float32 errors are printed next to the bound (lines "SSIM-ACC ...", kept in profiles/ssim_accuracy.txt).  Beyond the table:
    needs        only a, only b and both requiring a gradient: the same bits for everything they share
    twice        every case is run twice for the same bits
    bookkeeping  fused=None takes the kernels; the backward is launched once per image that needs a gradient and not at all
                 with neither (ops.ssim_counts()); strided views reach the kernel uncopied (the same data pointers)
    many lenses  B = 65 537, one more launch than grid y holds: the bits of the same lenses in two smaller batches
    refusals     fused=True with float64 images or a window of 13 taps
    chain        svola_convolution -> warp_bicubic -> 1 - ssim: finite gradients on the PSFs, equal to the torch path's"""
import numpy as np
import pytest
import torch

import ssim_cases as sc
from ssim_ref import ssim_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def im():
    from torchoptics_amd import _lib, imaging
    _lib.lib()
    return imaging


def _line(name, tag, err, bnd):
    cells = "  ".join(f"{k} {e:.2e} / {b:.2e}" for k, e, b in zip(("value", "g_a", "g_b"), err, bnd))
    return f"SSIM-ACC {name:14s} {tag:6s} error / bound  {cells}"


@pytest.mark.parametrize("name", list(sc.CASES))
def test_value_and_gradients_within_the_bound_for_every_needs_setting_and_twice_the_same_bits(im, name):
    both, again = sc.run(im, name, DEV, torch.float32, True), sc.run(im, name, DEV, torch.float32, True)
    only_a = sc.run(im, name, DEV, torch.float32, True, needs=("a",))
    only_b = sc.run(im, name, DEV, torch.float32, True, needs=("b",))
    for key in ("value", "g_a", "g_b"):
        assert np.array_equal(both[key], again[key]), f"{key}: two runs must give the same bits"
    assert only_a["g_b"] is None and only_b["g_a"] is None
    assert np.array_equal(only_a["value"], both["value"]) and np.array_equal(only_b["value"], both["value"])
    assert np.array_equal(only_a["g_a"], both["g_a"]) and np.array_equal(only_b["g_b"], both["g_b"])
    err, bnd = sc.errors(name, both["value"], both["g_a"], both["g_b"]), sc.bounds(name)
    print(_line(name, "fused", err, bnd))
    assert all(np.isfinite(e) and e <= b for e, b in zip(err, bnd)), (name, err, bnd)


@pytest.mark.parametrize("name", list(sc.CASES))
def test_the_torch_float32_path_on_the_gpu_stays_within_the_same_bounds(im, name):
    got = sc.run(im, name, DEV, torch.float32, False)
    err, bnd = sc.errors(name, got["value"], got["g_a"], got["g_b"]), sc.bounds(name)
    print(_line(name, "torch", err, bnd))
    assert all(e <= b for e, b in zip(err, bnd)), (name, err, bnd)


def test_the_default_takes_the_kernels_and_the_backward_runs_once_per_image_that_needs_a_gradient(im):
    from torchoptics_amd import ops
    name = "map_16x32"
    for needs, launches in ((("a", "b"), 2), (("a",), 1), (("b",), 1)):
        before = ops.ssim_counts()
        got = sc.run(im, name, DEV, torch.float32, None, needs=needs)
        after = ops.ssim_counts()
        assert after["fwd"] == before["fwd"] + 1, "fused=None on float32 GPU tensors is the kernels"
        assert after["bwd"] == before["bwd"] + launches, needs
        assert np.array_equal(got["value"], sc.run(im, name, DEV, torch.float32, True, needs=needs)["value"])
    before = ops.ssim_counts()
    a, b, _, par = sc.case_inputs(name)
    ta, tb = sc.as_tensor(a, "dense", torch.float32, DEV), sc.as_tensor(b, "dense", torch.float32, DEV)
    value = im.ssim(ta, tb, **par)
    assert not value.requires_grad
    after = ops.ssim_counts()
    assert (after["fwd"], after["bwd"]) == (before["fwd"] + 1, before["bwd"]), "no gradient needed: no backward, no maps"
    assert np.array_equal(value.cpu().numpy(), sc.run(im, name, DEV, torch.float32, True)["value"]), "the maps do not change the value"


@pytest.mark.parametrize("name", ["channel_slice", "transposed"])
def test_strided_views_reach_the_kernel_uncopied_and_give_the_bits_of_the_dense_run(im, name):
    from torchoptics_amd import ops
    a, b, seed, par = sc.case_inputs(name)
    layout = sc.CASES[name][8]
    ta, tb = sc.as_tensor(a, layout, torch.float32, DEV), sc.as_tensor(b, layout, torch.float32, DEV)
    assert not ta.is_contiguous() and not tb.is_contiguous()
    ta.requires_grad_(True)
    tb.requires_grad_(True)
    value = im.ssim(ta, tb, fused=True, **par)
    seen = ops.ssim_counts()
    assert (seen["a_ptr"], seen["b_ptr"]) == (ta.data_ptr(), tb.data_ptr())
    value.backward(torch.from_numpy(seed).to(dtype=torch.float32, device=DEV))
    da, db = sc.as_tensor(a, "dense", torch.float32, DEV).requires_grad_(True), sc.as_tensor(b, "dense", torch.float32, DEV).requires_grad_(True)
    dense = im.ssim(da, db, fused=True, **par)
    dense.backward(torch.from_numpy(seed).to(dtype=torch.float32, device=DEV))
    assert torch.equal(value, dense) and torch.equal(ta.grad, da.grad) and torch.equal(tb.grad, db.grad)


def test_more_lenses_than_one_launch_takes_give_the_bits_of_two_smaller_batches(im):
    """B = 65 537 > 65 535 (grid y): the calls are cut into two launches.  Lenses are independent, so the result must have
    the bits of the same lenses run as two batches that fit one launch each."""
    B, cut = 65537, 40000
    g = torch.Generator(device=DEV).manual_seed(11)
    a, b = torch.rand((B, 11, 12, 1), generator=g, device=DEV), torch.rand((B, 11, 12, 1), generator=g, device=DEV)
    seed = torch.rand(B, generator=g, device=DEV) - 0.5

    def run(lo, hi):
        ta, tb = a[lo:hi].clone().requires_grad_(True), b[lo:hi].clone().requires_grad_(True)
        value = im.ssim(ta, tb, fused=True)
        value.backward(seed[lo:hi])
        return value.detach(), ta.grad, tb.grad

    whole, parts = run(0, B), [run(0, cut), run(cut, B)]
    for k in range(3):
        assert torch.equal(whole[k], torch.cat([p[k] for p in parts])), k
    assert bool(torch.isfinite(whole[0]).all()) and float(whole[1][-1].abs().max()) > 0


def test_fused_refuses_float64_and_a_window_of_13_taps(im):
    a = torch.rand(1, 20, 20, 3, device=DEV)
    with pytest.raises(ValueError, match="dtype"):
        im.ssim(a.double(), a.double(), fused=True)
    with pytest.raises(ValueError, match="K"):
        im.ssim(a, a, filter_size=13, fused=True)
    with pytest.raises(ValueError, match="return_map"):
        im.ssim(a, a, fused=True, return_map=True)
    assert im.ssim(a.double(), a.double()).dtype == torch.float64, "fused=None falls to the torch path for float64"


def test_one_step_through_blur_and_warp_into_one_minus_ssim_gives_the_torch_paths_gradients_on_the_psfs(im):
    """svola_convolution -> warp_bicubic(image_grad='fused') -> 1 - ssim, gradient to the PSFs.  Reference: the same chain in
    torch ops in float64.  Bound: as in ssim_cases -- 4 x the float32 torch chain's error on the same GPU, with the floor
    16 eps32 x (the size of the terms that cancel in d ssim / d rendered) / (its largest element), from ssim_ref on the float64
    rendering: the two linear adjoints behind it add many such elements with weights below 1."""
    H, W, Cc, gh, gw, k = 48, 64, 3, 2, 2, 5
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
        loss = 1 - im.ssim(rendered, t(chart), fused=fused).mean()
        loss.backward()
        return loss.detach().cpu().numpy(), psfs.grad.cpu().numpy(), rendered.detach().cpu().numpy()

    _, g64, rendered64 = chain(torch.float64, False)
    _, g32, _ = chain(torch.float32, False)
    _, gk, _ = chain(torch.float32, True)
    assert np.isfinite(gk).all() and np.abs(gk).max() > 0
    r = ssim_ref(rendered64, chart, seed=-np.ones(1))
    floor = 16 * sc.EPS32 * float(np.max(r["cond_a"])) / float(np.max(np.abs(r["g_a"])))
    top = np.abs(g64).max()
    e32, ek = np.abs(g32 - g64).max() / top, np.abs(gk - g64).max() / top
    bound = max(sc.MARGIN * e32, floor)
    print(f"SSIM-ACC chain          d loss / d psfs: fused {ek:.2e}, torch float32 {e32:.2e}, bound {bound:.2e}")
    assert ek <= bound, (ek, e32, bound)
