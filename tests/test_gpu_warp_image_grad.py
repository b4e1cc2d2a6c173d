"""The fixed-point image gradient of the fused bicubic warp (tl_warp_bwd_image behind imaging.warp_bicubic(image_grad="fused"))
on the GPU against tests/warp_ref.py in float64.

The bound is derived, not tuned: tests/warp_image_cases.py states it (the float bound of tests/warp_cases.py plus half a quantum
per contribution, the quantum derived from the inputs as the contract states it) and tests/test_warp_image_grad_cpu.py holds
it to be sharp and sufficient.  Every element is checked; the largest error / bound is printed per case (lines
"WARP-IMG-ACC ...", kept in profiles/warp_image_grad_accuracy.txt).  The shapes live in tests/warp_image_cases.py.  Beyond
accuracy:
    reproducible  two runs, "direct" and "auto", the transposed output, expanded coordinates, strided views: the same bits
    scale         g_out times 2^40 and 2^-40 scale the result exactly; an all-zero g_out gives zeros
    poison        a NaN coordinate, an infinite g_out: NaN under that pixel's 16 clipped taps, the clean bits elsewhere, the
                  same set of non-finite elements as the torch path
    bookkeeping   tl_warp_bwd_image runs once and only when the image needs a gradient, tl_warp_bwd as before
    chain         Cooke triplet -> PSFs -> svola_convolution -> warp (the reference's order) -> sum of squares: leaf gradients"""
import numpy as np
import pytest
import torch

from conftest import rel_l2
import warp_cases as wc
import warp_image_cases as wic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def im():
    from torchoptics_amd import _lib, imaging
    _lib.lib()
    return imaging


@pytest.fixture()
def path():
    from torchoptics_amd import ops
    yield ops.set_warp_image_grad_path
    ops.set_warp_image_grad_path("auto")


def _g(im, args, **kw):
    return wic.run(im, args, DEV, **kw)["g_image"]


@pytest.mark.parametrize("name,signed", [(n, False) for n in wic.ALL] + [(n, True) for n in wc.SIGNED])
def test_within_the_bound_twice_the_same_bits_and_direct_equals_auto(im, path, name, signed):
    B, (H, W, Cc), (Ho, Wo), *_ = wic.shape_of(name)
    args, r = wic.inputs(name, signed), wic.reference(name, signed)
    got, again = _g(im, args), _g(im, args)
    path("direct")
    direct = _g(im, args)
    q = wc.ratio(got, r.g_image, wic.bound(r, args[3], args[4]))
    print(f"WARP-IMG-ACC {name + ('/signed' if signed else ''):16s} B={B} {H}x{W}x{Cc} <- {Ho}x{Wo}: largest error / bound {q:.3f}")
    assert wic.same_bits(got, again), "two runs must give the same bits"
    assert wic.same_bits(got, direct), "the LDS box and the direct atomics must give the same bits"
    assert q <= 1, (name, q)
    untouched = r.g_image_terms == 0
    assert (got[untouched] == 0).all() and not np.signbit(got[untouched]).any(), "no tap: exactly +0.0"


@pytest.mark.parametrize("name", ["general", "shared", "barrel", "outliers", "pile-up"])
def test_the_transposed_output_gives_the_same_bits(im, name):
    """The same output pixels in another order and another grouping into tiles: x, y, gain and g_out transposed."""
    image, x, y, gain, g_out = wic.inputs(name)
    want = _g(im, (image, x, y, gain, g_out))
    tr = lambda v: None if v is None else np.ascontiguousarray(np.swapaxes(v, 1, 2))      # noqa: E731
    assert wic.same_bits(_g(im, (image, tr(x), tr(y), tr(gain), tr(g_out))), want)


def test_shared_coordinates_and_their_expansion_give_the_same_bits(im):
    image, x, y, gain, g_out = wic.inputs("shared")
    B = image.shape[0]
    assert x.shape[0] == 1 and B > 1
    want = _g(im, (image, x, y, gain, g_out))
    wide = lambda v: np.ascontiguousarray(np.broadcast_to(v, (B,) + v.shape[1:]))          # noqa: E731
    assert wic.same_bits(_g(im, (image, wide(x), wide(y), wide(gain), g_out)), want)


@pytest.mark.parametrize("name", ["general", "shared"])
def test_strided_coordinates_and_gain_give_the_contiguous_bits(im, name):
    from torchoptics_amd import ops
    image, x, y, gain, g_out = wic.inputs(name)
    want = _g(im, (image, x, y, gain, g_out))
    t = lambda v: torch.as_tensor(v).float().to(DEV)                                        # noqa: E731
    grid = torch.stack((t(x), t(y)), dim=-1)                                               # x and y: the halves of one grid
    big = torch.full((gain.shape[0], gain.shape[1] + 2, gain.shape[2] + 3, gain.shape[3] + 1), 7.0, device=DEV)
    big[:, 1:-1, 2:-1, 1:] = t(gain)
    vx, vy, vg = grid[..., 0], grid[..., 1], big[:, 1:-1, 2:-1, 1:]
    assert not (vx.is_contiguous() or vy.is_contiguous() or vg.is_contiguous())
    got = _g(im, (image, vx, vy, vg, g_out))
    seen = ops.warp_counts()
    assert (seen["x_ptr"], seen["y_ptr"], seen["gain_ptr"]) == (vx.data_ptr(), vy.data_ptr(), vg.data_ptr()), "no copy"
    assert wic.same_bits(got, want)


@pytest.mark.parametrize("name", ["general", "range", "barrel"])
def test_a_power_of_two_in_g_out_scales_the_result_exactly(im, name):
    image, x, y, gain, g_out = wic.inputs(name)
    want = _g(im, (image, x, y, gain, g_out)).astype(np.float64)
    assert np.abs(want).max() < 2.0 ** 80 and np.abs(want[want != 0]).min() > 2.0 ** -80       # no fp32 under- or overflow below
    for k in (40, -40):
        got = _g(im, (image, x, y, gain, g_out * 2.0 ** k))
        assert wic.same_bits(got, (want * 2.0 ** k).astype(np.float32)), k


def test_an_all_zero_g_out_gives_zeros(im):
    image, x, y, gain, g_out = wic.inputs("general")
    got = _g(im, (image, x, y, gain, np.zeros_like(g_out)))
    assert (got == 0).all() and not np.signbit(got).any()


def _poison_case(which):
    """(args of the clean run, args of the poisoned run, the elements under the poisoned pixel's 16 clipped taps).  The clean
    run is the one without the poisoned contributions: their seeds are zero there (none of them is m, so the scale stays)."""
    image, x, y, gain, g_out = wic.inputs("general")
    B, H, W, Cc = image.shape
    b, yo, xo, c = 1, 7, 11, 2
    taps = lambda v, n: np.clip(int(np.floor(np.float32((np.clip(v, -1, 1) + 1) / 2 * (n - 1)))) + np.arange(-1, 3), 0, n - 1)   # noqa: E731
    rows = taps(y[b, yo, xo], H)
    hit = np.zeros(image.shape, dtype=bool)
    clean_g, bad_x, bad_g = g_out.copy(), x, g_out
    if which == "nan-coordinate":                       # the taps of a NaN x: the clipped columns around j0 = 0
        bad_x = x.copy()
        bad_x[b, yo, xo] = np.nan
        clean_g[b, yo, xo, :] = 0
        hit[b, rows[:, None], np.clip(np.arange(-1, 3), 0, W - 1)[None, :], :] = True
    else:
        bad_g = g_out.copy()
        bad_g[b, yo, xo, c] = np.inf
        clean_g[b, yo, xo, c] = 0
        hit[b, rows[:, None], taps(x[b, yo, xo], W)[None, :], c] = True
    assert np.abs(clean_g * gain).max() == np.abs(g_out * gain).max(), "none of the poisoned seeds is m itself"
    return (image, x, y, gain, clean_g), (image, bad_x, y, gain, bad_g), hit


@pytest.mark.parametrize("which", ["nan-coordinate", "inf-in-g_out"])
def test_a_non_finite_contribution_poisons_its_taps_and_nothing_else(im, path, which):
    clean_args, bad_args, hit = _poison_case(which)
    clean = _g(im, clean_args)
    got = _g(im, bad_args)
    assert np.isnan(got[hit]).all(), "the elements under the 16 clipped taps are NaN"
    assert np.isfinite(got[~hit]).all()
    assert wic.same_bits(got[~hit], clean[~hit]), "every other element keeps the clean run's bits"
    path("direct")
    assert wic.same_bits(_g(im, bad_args), got)
    torch_path = wic.run(im, bad_args, DEV, fused=False, image_grad="torch")["g_image"]
    assert np.array_equal(~np.isfinite(torch_path), ~np.isfinite(got)), "the same set of non-finite elements as the torch path"


def test_each_backward_runs_once_and_only_when_it_is_needed(im):
    from torchoptics_amd import ops
    args = wic.inputs("general")
    count = lambda: tuple(ops.warp_counts()[k] for k in ("fwd", "bwd", "bwd_image"))        # noqa: E731
    c0 = count()
    only_image = wic.run(im, args, DEV, needs=("image",))
    assert count() == (c0[0] + 1, c0[1], c0[2] + 1)
    without = wic.run(im, args, DEV, needs=("x", "y", "gain"))
    assert count() == (c0[0] + 2, c0[1] + 1, c0[2] + 1)
    both = wic.run(im, args, DEV, needs=("image", "x", "y", "gain"))
    assert count() == (c0[0] + 3, c0[1] + 2, c0[2] + 2)
    for what in ("g_x", "g_y", "g_gain"):
        assert wic.same_bits(both[what], without[what]), f"{what} keeps its bits next to an image gradient"
    assert wic.same_bits(both["g_image"], only_image["g_image"])
    dflt = wic.run(im, args, DEV, fused=None, needs=("image", "gain"))                       # fused=None takes the kernels
    assert count() == (c0[0] + 4, c0[1] + 3, c0[2] + 3) and wic.same_bits(dflt["g_image"], only_image["g_image"])
    image, x, y, gain, _ = (torch.as_tensor(v).float().to(DEV) for v in args)
    out = im.warp_bicubic(image, x, y, gain, fused=True, image_grad="fused")                # nothing needs a gradient
    assert not out.requires_grad and count() == (c0[0] + 5, c0[1] + 3, c0[2] + 3)
    image.requires_grad_(True)
    with pytest.raises(RuntimeError, match="image requires a gradient"):                    # the default stays as it was
        im.warp_bicubic(image, x, y, gain, fused=True)
    im.warp_bicubic(image, x, y, gain).sum().backward()                                     # fused=None: the torch path
    assert count() == (c0[0] + 5, c0[1] + 3, c0[2] + 3) and image.grad is not None


def test_leaf_gradients_in_the_reference_order():
    """Cooke triplet -> psf_from_trace -> fused svola_convolution of a 30 x 20 x 3 chart -> relative illumination (radial_map)
    and distortion (distortion_grid) -> warp_bicubic -> sum of squares: the whole gradient through the PSFs passes through
    d warp / d image.  image_grad="fused" against the same chain with the warp at fused=False: rel-L2 1e-5 on c and t."""
    import torchoptics_amd as ta
    import yaml_free_lenses as L
    from torchoptics_amd import ops
    chart = torch.rand((1, 30, 20, 3), generator=torch.Generator().manual_seed(3)).to(DEV)
    fields = (0., 0.7, 1.0)
    got = {}
    for fused in (False, True):
        before = ops.warp_counts()["bwd_image"]
        lens, specs, leaves = L.build("cooke", DEV, epd=8.578)
        tr = ta.RayTracer(mode="circular", n_rays=(16, 16), rel_fields=fields, wavelengths=("C", "d", "F"), default_device=DEV)
        xr, yr, cx, cy, ok, back = tr.trace_rays(specs, lens)
        kernels = ta.metrics.psf_from_trace(xr, yr, ok, n_bins=(9, 9), increment=0.004, fused=True)[3]
        psfs = ta.imaging.psf_grid_from_fields(kernels, (3, 1))
        blurred = ta.imaging.svola_convolution(chart, 4, psfs, (3, 1), "hann", fused=True)
        d = ta.metrics.compute_distortion(specs, lens, fields[1:], default_device=DEV)
        ri = ta.metrics.compute_relative_illumination(specs, lens, fields, wavelengths=("C", "d", "F"), default_device=DEV)
        x, y = ta.imaging.distortion_grid(d, fields[1:], (30, 20))
        gain = ta.imaging.radial_map(ri[:, 1:], fields[1:], (30, 20), v0=1.0)
        out = ta.imaging.warp_bicubic(blurred, x, y, gain, fused=fused, image_grad="fused")
        (out ** 2).sum().backward()
        got[fused] = {n: leaves[n].grad.cpu().numpy() for n in ("c", "t")}
        assert ops.warp_counts()["bwd_image"] == before + int(fused)
    for n in ("c", "t"):
        e = rel_l2(got[True][n], got[False][n])
        print(f"WARP-IMG-ACC chain leaf gradient {n} through trace -> PSF -> convolution -> warp: fused vs torch warp rel-L2 {e:.3e}")
        assert np.isfinite(got[True][n]).all() and np.isfinite(got[False][n]).all()
        assert np.linalg.norm(got[True][n]) > 0 and np.linalg.norm(got[False][n]) > 0
        assert e <= 1e-5, (n, e)
