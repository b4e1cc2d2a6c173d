"""The fused bicubic warp (tl_warp_fwd / tl_warp_bwd behind imaging.warp_bicubic(fused=True)) on the GPU against
tests/warp_ref.py in float64.

The bounds are derived, not tuned: tests/warp_cases.py states them (rounding of the weights against the sums of their absolute
monomials, of the 16-term sum and the products against the sum of absolute terms, and of u and v themselves through the
derivative weights) and tests/test_warp_cpu.py holds them to be sharp (five wrong float64 evaluations exceed them) and
sufficient (the float32 torch path stays within them).  Every element is checked; the largest observed error / bound is
printed per case (lines "WARP-ACC ...", kept in profiles/warp_accuracy.txt).

The shapes live in tests/warp_cases.py, whose docstring says what each one exists for.  Beyond the table:
    twice        every case is run twice for the same bits
    signs        three cases with seeded signs on image, gain and g_out, held to the bound on the absolute values
    strides      a permuted [B,C,H,W] image, an interior slice, x and y as the two halves of a stacked [..,2] grid: the bits of
                 the contiguous run, and the same data_ptr reaching the kernel
    fuzz         48 seeded small geometries with the sharing flags drawn too, all valid by construction
    NaN          one NaN coordinate: that pixel's output and gradients are NaN, every other element keeps its bits
    bookkeeping  the backward is launched once, and only when a coordinate or the gain needs a gradient (ops.warp_counts())
    chain        Cooke triplet -> compute_distortion -> distortion_grid -> warp_bicubic -> sum of squares: leaf gradients"""
import numpy as np
import pytest
import torch

from conftest import rel_l2
import warp_cases as wc
import warp_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GPU_NAMES = ("out", "g_x", "g_y", "g_gain")          # the image gradient is not a kernel


@pytest.fixture(scope="module")
def im():
    from torchoptics_amd import _lib, imaging
    _lib.lib()
    return imaging


def _fused(im, args, needs=("x", "y", "gain")):
    return wc.run(im, args, DEV, torch.float32, fused=True, needs=needs)


def _ratios(got, r):
    return {what: wc.ratio(got[what], getattr(r, what), wc.bound(r, what)) for what in GPU_NAMES if getattr(r, what) is not None}


def _line(tag, ratios):
    return f"WARP-ACC {tag}: largest error / bound  " + "  ".join(f"{k} {v:.3f}" for k, v in ratios.items())


@pytest.mark.parametrize("name", list(wc.CASES))
def test_values_and_gradients_against_the_reference_and_twice_the_same_bits(im, name):
    B, (H, W, Cc), (Ho, Wo), *_ = wc.CASES[name]
    args, r = wc.inputs(name), wc.reference(name)
    got, again = _fused(im, args), _fused(im, args)
    for what in got:
        assert np.array_equal(got[what], again[what]), f"{what}: two runs must give the same bits"
    ratios = _ratios(got, r)
    print(_line(f"{name:12s} B={B} {H}x{W}x{Cc} -> {Ho}x{Wo}", ratios))
    assert set(ratios) == set(got) and max(ratios.values()) <= 1, (name, ratios)
    if name == "identity":
        assert np.array_equal(got["out"], args[0]), "t = 0 everywhere: the output is the image bit for bit"
    if name == "thin-row":
        assert not got["g_y"].any(), "H - 1 = 0: no gradient to y"
    if name == "thin-col":
        assert not got["g_x"].any(), "W - 1 = 0: no gradient to x"


@pytest.mark.parametrize("name", wc.SIGNED)
def test_signed_data_within_the_bound_on_the_absolute_values(im, name):
    args, r = wc.inputs(name, signed=True), wc.reference(name, signed=True)
    assert (args[0] < 0).any() and (args[3] < 0).any() and (args[4] < 0).any()
    ratios = _ratios(_fused(im, args), r)
    print(_line(f"{name + '/signed':12s}", ratios))
    assert max(ratios.values()) <= 1, (name, ratios)


def test_seeded_fuzz_over_small_geometries(im):
    worst, failed = (0.0, None, ""), []
    draws = wc.fuzz_draws()
    for t, (B, H, W, Cc, Ho, Wo, cb, gshape) in draws:
        args = ref.make_inputs(B, H, W, Cc, Ho, Wo, cb, gshape, seed=t, signed=bool(t % 2))
        ratios = _ratios(_fused(im, args), ref.evaluate(*args))
        for what, v in ratios.items():
            if v > worst[0]:
                worst = (v, (t, B, H, W, Cc, Ho, Wo, cb, gshape), what)
        if max(ratios.values()) > 1:
            failed.append(((t, B, H, W, Cc, Ho, Wo, cb, gshape), ratios))
    shared = sum(cb == 1 and B > 1 for _, (B, *_, cb, _) in draws)
    print(f"WARP-ACC fuzz         {len(draws)} draws (seed {wc.FUZZ_SEED}), {shared} with coordinates shared by B > 1, "
          f"{sum(g is not None for *_, (*_, g) in draws)} with gain: largest error / bound {worst[0]:.3f} ({worst[2]}) at draw, B, H, W, C, "
          f"Ho, Wo, coordinate batch, gain = {worst[1]}")
    assert len(draws) == 48 and not failed, failed


def _views(kind, image, x, y):
    """float32 GPU leaves that are not what the kernels index, and the views of them that are."""
    a, xs, ys = (torch.as_tensor(v).float().to(DEV) for v in (image, x, y))
    if kind == "permuted":                        # [B,C,H,W] in memory
        la = a.permute(0, 3, 1, 2).contiguous()
        return la.permute(0, 2, 3, 1), xs, ys, None
    if kind == "sliced":                          # the interior of larger tensors: a storage offset, rows with gaps
        B, H, W, Cc = a.shape
        la = torch.full((B, H + 3, W + 2, Cc + 2), 7.0, device=DEV)
        cut = (slice(None), slice(2, 2 + H), slice(1, 1 + W), slice(1, 1 + Cc))
        la[cut] = a
        lx = torch.full((xs.shape[0], xs.shape[1] + 2, xs.shape[2] + 3), 7.0, device=DEV)
        ly = lx.clone()
        lx[:, 1:-1, 2:-1], ly[:, 1:-1, 2:-1] = xs, ys
        return la[cut], lx[:, 1:-1, 2:-1], ly[:, 1:-1, 2:-1], None
    assert kind == "stacked"                      # x = grid[..., 0], y = grid[..., 1]
    grid = torch.stack((xs, ys), dim=-1).requires_grad_(True)
    return a, grid[..., 0], grid[..., 1], grid


@pytest.mark.parametrize("kind", ["permuted", "sliced", "stacked"])
@pytest.mark.parametrize("name", ["general", "shared"])
def test_strided_views_reach_the_kernels_without_a_copy_and_give_the_contiguous_bits(im, name, kind):
    from torchoptics_amd import ops
    image, x, y, gain, g_out = wc.inputs(name)
    want = _fused(im, (image, x, y, gain, g_out))
    va, vx, vy, grid = _views(kind, image, x, y)
    assert not (va.is_contiguous() and vx.is_contiguous() and vy.is_contiguous())
    if grid is None:
        vx, vy = vx.detach().requires_grad_(True), vy.detach().requires_grad_(True)     # leaves that keep their strides
        assert (kind == "permuted") or not vx.is_contiguous()
    gn = torch.as_tensor(gain).float().to(DEV).requires_grad_(True)
    out = im.warp_bicubic(va, vx, vy, gn, fused=True)
    seen = ops.warp_counts()
    assert (seen["image_ptr"], seen["x_ptr"], seen["y_ptr"]) == (va.data_ptr(), vx.data_ptr(), vy.data_ptr()), "no copy"
    for saved, view in zip(out.grad_fn.saved_tensors, (va, vx, vy)):
        assert saved.data_ptr() == view.data_ptr() and saved.stride() == view.stride(), "the view must reach the kernel as it is"
    (out * torch.as_tensor(g_out).float().to(DEV)).sum().backward()
    g_x, g_y = (grid.grad[..., 0], grid.grad[..., 1]) if grid is not None else (vx.grad, vy.grad)
    for what, have in (("out", out.detach()), ("g_x", g_x), ("g_y", g_y), ("g_gain", gn.grad)):
        assert np.array_equal(have.double().cpu().numpy(), want[what]), what


def test_one_nan_coordinate_poisons_its_pixel_and_nothing_else(im):
    image, x, y, gain, g_out = wc.inputs("general")
    clean = _fused(im, (image, x, y, gain, g_out))
    b, yo, xo = 1, 7, 11
    bad = x.copy()
    bad[b, yo, xo] = np.nan
    got = _fused(im, (image, bad, y, gain, g_out))
    hit = {"out": (b, yo, xo, slice(None)), "g_x": (b, yo, xo), "g_y": (b, yo, xo), "g_gain": (b, yo, xo, slice(None))}
    for what in GPU_NAMES:
        assert np.isnan(got[what][hit[what]]).all(), what
        mask = np.ones(got[what].shape, dtype=bool)
        mask[hit[what]] = False
        assert np.array_equal(got[what][mask], clean[what][mask]), f"{what}: every other element keeps its bits"
    torch_path = wc.run(im, (image, bad, y, gain, g_out), DEV, torch.float32, fused=False, needs=("x", "y", "gain"))
    for what in GPU_NAMES:
        assert np.isnan(torch_path[what][hit[what]]).all(), f"the torch path does the same: {what}"
        assert np.isnan(torch_path[what]).sum() == np.isnan(got[what]).sum(), what


def test_the_backward_is_launched_once_and_only_when_something_needs_it(im):
    from torchoptics_amd import ops
    args = wc.inputs("general")
    count = lambda: tuple(ops.warp_counts()[k] for k in ("fwd", "bwd"))                 # noqa: E731
    c0 = count()
    got = _fused(im, args, needs=("gain",))                                                # only the gain
    assert set(got) == {"out", "g_gain"} and count() == (c0[0] + 1, c0[1] + 1)
    r = wc.reference("general")
    assert wc.ratio(got["g_gain"], r.g_gain, wc.bound(r, "g_gain")) <= 1
    got = _fused(im, wc.inputs("no-gain"), needs=("x",))                                   # no gain at all, only x
    assert set(got) == {"out", "g_x"} and count() == (c0[0] + 2, c0[1] + 2)
    r = wc.reference("no-gain")
    assert wc.ratio(got["g_x"], r.g_x, wc.bound(r, "g_x")) <= 1
    image, x, y, gain, _ = (None if v is None else torch.as_tensor(v).float().to(DEV) for v in args)
    out = im.warp_bicubic(image, x, y, gain, fused=True)                                  # nothing needs a gradient
    assert not out.requires_grad and count() == (c0[0] + 3, c0[1] + 2)
    assert torch.equal(im.warp_bicubic(image, x, y, gain), out), "fused=None on the GPU takes the kernels"
    assert count() == (c0[0] + 4, c0[1] + 2)
    image.requires_grad_(True)
    with pytest.raises(RuntimeError, match="image requires a gradient"):
        im.warp_bicubic(image, x, y, gain, fused=True)
    dflt = im.warp_bicubic(image, x, y, gain)                                             # fused=None: the torch path
    assert count() == (c0[0] + 4, c0[1] + 2)
    dflt.sum().backward()
    assert image.grad is not None and torch.isfinite(image.grad).all()


def test_leaf_gradients_through_distortion_grid_and_warp():
    """Cooke triplet -> compute_distortion at four fields -> distortion_grid -> warp_bicubic of a 30 x 20 x 3 chart -> sum of
    squares.  d/d(distortion values): the fused run and the float32 torch run against the float64 torch path from
    d.detach().double() onward; the fused error must be no larger than twice the torch float32 error.  Leaf gradients on c
    and t: finite, non-zero, fused against fused=False within rel-L2 1e-5 (as tests/test_gpu_svola.py has it)."""
    import torchoptics_amd as ta
    import yaml_free_lenses as L
    chart = torch.rand((1, 30, 20, 3), generator=torch.Generator().manual_seed(3)).to(DEV)
    got, g_d = {}, {}
    for fused in (False, True):
        lens, specs, leaves = L.build("cooke", DEV, epd=8.578)
        d = ta.metrics.compute_distortion(specs, lens, wc.FIELDS, default_device=DEV)
        d.retain_grad()
        x, y = ta.imaging.distortion_grid(d, wc.FIELDS, (30, 20))
        out = ta.imaging.warp_bicubic(chart, x, y, fused=fused)
        (out ** 2).sum().backward()
        got[fused] = {n: leaves[n].grad.cpu().numpy() for n in ("c", "t")}
        g_d[fused] = d.grad.double().cpu().numpy()
    d64 = d.detach().double().requires_grad_(True)
    x, y = ta.imaging.distortion_grid(d64, wc.FIELDS, (30, 20))
    (ta.imaging.warp_bicubic(chart.double(), x, y, fused=False) ** 2).sum().backward()
    want = d64.grad.cpu().numpy()
    e_fused, e_torch = rel_l2(g_d[True], want), rel_l2(g_d[False], want)
    print(f"WARP-ACC chain        d(sum out^2)/d(distortion values) against float64: fused rel-L2 {e_fused:.3e}, torch float32 {e_torch:.3e}")
    assert np.linalg.norm(want) > 0 and e_fused <= 2 * e_torch, (e_fused, e_torch)
    for n in ("c", "t"):
        e = rel_l2(got[True][n], got[False][n])
        print(f"WARP-ACC chain        leaf gradient {n} through trace -> distortion -> grid -> warp: fused vs torch rel-L2 {e:.3e}")
        assert np.isfinite(got[True][n]).all() and np.linalg.norm(got[True][n]) > 0 and np.linalg.norm(got[False][n]) > 0
        assert e <= 1e-5, (n, e)
