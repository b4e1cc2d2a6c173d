"""imaging.warp_bicubic without a GPU: the torch path in float64 against tests/warp_ref.py on every case of tests/warp_cases.py
and all five results; analytic pins; the bounds of warp_cases held to be SHARP (five deliberately wrong float64 evaluations
exceed them) as well as sufficient (the float32 torch path on the CPU stays within them); radial_map and distortion_grid; the
tl_warp_* entry points (declared, bound, exported, refusing bad arguments before any HIP call); the Python layer's errors."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import warp_cases as wc
import warp_ref as ref
from torchoptics_amd import _lib, imaging

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
ONE = C.c_void_p(8)                  # a pointer that is never dereferenced on the paths tested here


# ------------------------------------------------------------------------------------------------- the torch path, float64

@pytest.mark.parametrize("name", list(wc.CASES))
def test_the_torch_path_in_float64_is_the_reference_on_every_case_and_all_five_results(name):
    args, r = wc.inputs(name), wc.reference(name)
    got = wc.run(imaging, args, "cpu", torch.float64, fused=False)
    dflt = wc.run(imaging, args, "cpu", torch.float64, fused=None)
    for what in wc.NAMES:
        want = getattr(r, what)
        if want is None:
            assert what not in got
            continue
        err = np.abs(got[what] - want).max() / np.abs(want).max() if np.abs(want).max() > 0 else np.abs(got[what]).max()
        assert err <= 1e-12, (name, what, err)
        assert np.array_equal(got[what], dflt[what]), "fused=None on the CPU is the same path"


def test_the_torch_path_is_the_reference_on_the_fuzz_geometries():
    for t, (B, H, W, Cc, Ho, Wo, cb, gshape) in wc.fuzz_draws():
        args = ref.make_inputs(B, H, W, Cc, Ho, Wo, cb, gshape, seed=t, signed=bool(t % 2))
        r = ref.evaluate(*args)
        got = wc.run(imaging, args, "cpu", torch.float64, fused=False)
        for what in wc.NAMES:
            want = getattr(r, what)
            if want is not None:
                scale = max(np.abs(want).max(), 1e-300)
                assert np.abs(got[what] - want).max() / scale <= 1e-12, (t, what)


# ------------------------------------------------------------------------------------------------------------ analytic pins

def _grid(Ho, Wo, dtype=torch.float64):
    y, x = torch.meshgrid(torch.linspace(-1, 1, Ho, dtype=dtype), torch.linspace(-1, 1, Wo, dtype=dtype), indexing="ij")
    return x[None].clone(), y[None].clone()


def test_a_constant_image_gives_the_constant():
    image = torch.full((2, 7, 9, 3), 0.625, dtype=torch.float64)
    g = torch.Generator().manual_seed(1)
    x, y = (torch.rand((2, 11, 13), generator=g, dtype=torch.float64) * 2.4 - 1.2 for _ in range(2))
    out = imaging.warp_bicubic(image, x, y)
    assert out.shape == (2, 11, 13, 3) and (out - 0.625).abs().max() <= 1e-15


def test_the_ramp_gives_the_closed_form_and_its_derivative():
    """image[.., q, ..] = q: the interior result is j0 + t^3 - 1.5 t^2 + 1.5 t (not u: only alpha = -0.5 reproduces lines), and
    g_x is (3 t^2 - 3 t + 1.5) (W - 1)/2."""
    H, W = 5, 12
    image = torch.arange(W, dtype=torch.float64)[None, None, :, None].expand(1, H, W, 1).contiguous()
    u = torch.linspace(1.0, W - 2.0, 37, dtype=torch.float64)[:-1] + 0.013           # interior cells: 1 <= j0 <= W - 3
    x = (2 * u / (W - 1) - 1)[None, None, :].requires_grad_(True)
    y = torch.zeros_like(x)
    out = imaging.warp_bicubic(image, x, y)
    u = (x.detach() + 1) / 2 * (W - 1)
    j0 = torch.floor(u)
    t = u - j0
    assert (out[..., 0] - (j0 + t ** 3 - 1.5 * t ** 2 + 1.5 * t)).abs().max() <= 1e-13
    out.sum().backward()
    assert (x.grad - (3 * t ** 2 - 3 * t + 1.5) * (W - 1) / 2).abs().max() <= 1e-12
    assert (out[..., 0] - u).abs().max() > 1e-2, "the ramp result is not u"


def test_integer_shifts_give_the_shifted_image_with_replicate_edges():
    g = torch.Generator().manual_seed(2)
    image = torch.rand((1, 9, 17, 2), generator=g, dtype=torch.float64)            # W - 1, H - 1 powers of two: u is exact
    x, y = _grid(9, 17)
    for dy, dx in ((0, 0), (0, 3), (-2, 0), (1, -4)):
        out = imaging.warp_bicubic(image, x + 2.0 * dx / 16, y + 2.0 * dy / 8)
        rows = (torch.arange(9) + dy).clamp(0, 8)
        cols = (torch.arange(17) + dx).clamp(0, 16)
        assert torch.equal(out, image[:, rows][:, :, cols]), (dy, dx)


def test_outside_the_image_gives_the_edge_value_and_no_coordinate_gradient_and_exactly_one_passes_it():
    g = torch.Generator().manual_seed(3)
    image = torch.rand((1, 6, 7, 1), generator=g, dtype=torch.float64)
    x = torch.tensor([[[-1.5, -1.0, 1.0, 1.5, float("inf"), 0.3]]], dtype=torch.float64, requires_grad=True)
    y = torch.tensor([[[0.2, 0.2, 0.2, 0.2, 0.2, -7.0]]], dtype=torch.float64, requires_grad=True)
    out = imaging.warp_bicubic(image, x, y)
    edge = imaging.warp_bicubic(image, torch.tensor([[[-1.0, -1.0, 1.0, 1.0, 1.0, 0.3]]], dtype=torch.float64),
                                torch.tensor([[[0.2, 0.2, 0.2, 0.2, 0.2, -1.0]]], dtype=torch.float64))
    assert torch.equal(out, edge)
    out.sum().backward()
    assert x.grad[0, 0, 0] == 0 and x.grad[0, 0, 3] == 0 and x.grad[0, 0, 4] == 0 and y.grad[0, 0, 5] == 0
    # exactly +-1: the gradient is passed; at the replicate edge it is 0.75 (I[1] - I[0]) (W - 1)/2 seen from inside
    r = ref.evaluate(image.numpy(), x.detach().clamp(-9, 9).numpy(), y.detach().numpy(), None, np.ones((1, 1, 6, 1)))
    assert abs(float(x.grad[0, 0, 1]) - r.g_x[0, 0, 1]) <= 1e-13 and abs(float(x.grad[0, 0, 2]) - r.g_x[0, 0, 2]) <= 1e-13
    assert x.grad[0, 0, 1] != 0 and x.grad[0, 0, 2] != 0 and x.grad[0, 0, 5] != 0


def test_the_coordinate_gradient_is_continuous_across_integer_u():
    """C1: g_x at u = j from the cell with t = 0 and from the cell below with t -> 1 agree, replicate edges included."""
    g = torch.Generator().manual_seed(4)
    image = torch.rand((1, 3, 9, 1), generator=g, dtype=torch.float64)             # W - 1 = 8
    for j in range(0, 9):
        grads = []
        for shift in (0.0, -1e-9, 1e-9):
            if (j == 0 and shift < 0) or (j == 8 and shift > 0):
                continue
            x = torch.tensor([[[2 * (j + shift) / 8 - 1]]], dtype=torch.float64, requires_grad=True)
            imaging.warp_bicubic(image, x, torch.zeros_like(x)).sum().backward()
            grads.append(float(x.grad))
        assert max(grads) - min(grads) <= 1e-6 * max(1.0, abs(grads[0])), (j, grads)


# ------------------------------------------------------------------------------------- the yardstick: sharp and sufficient

@pytest.mark.parametrize("name", wc.MAIN)
@pytest.mark.parametrize("variant,what", [("alpha", "out"), ("swap", "out"), ("tap", "out"), ("wrap", "out"), ("factor", "g_x")])
def test_a_wrong_float64_evaluation_exceeds_the_bound(name, variant, what):
    """alpha = -0.5, x and y exchanged, one tap displaced by a pixel, indices wrapped instead of clipped, the (W - 1)/2 factor
    missing from g_x: each in float64, each over the bound of the main cases somewhere."""
    r = wc.reference(name)
    wrong = ref.evaluate(*wc.inputs(name), variant=variant)
    limit = wc.bound(r, what)
    over = np.abs(getattr(wrong, what) - getattr(r, what)) > limit
    assert over.any(), (name, variant)
    if variant in ("alpha", "swap", "factor"):
        assert over.mean() > 0.5, (name, variant, over.mean())


@pytest.mark.parametrize("name,signed", [(n, False) for n in wc.CASES] + [(n, True) for n in wc.SIGNED])
def test_the_float32_torch_path_on_the_cpu_stays_within_the_bound(name, signed):
    """A correct fp32 evaluation passes: the inputs and the bounds are such that the GPU test can be passed."""
    args, r = wc.inputs(name, signed), wc.reference(name, signed)
    got = wc.run(imaging, args, "cpu", torch.float32, fused=False)
    ratios = {what: wc.ratio(got[what], getattr(r, what), wc.bound(r, what)) for what in wc.NAMES if getattr(r, what) is not None}
    print(f"WARP-ACC cpu-fp32 {name}{'/signed' if signed else ''}: largest error / bound  " + "  ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert max(ratios.values()) <= 1, (name, ratios)


# --------------------------------------------------------------------------------------------- radial_map, distortion_grid

def test_radial_map_nodes_centre_hold_and_corner():
    fields = (0.25, 0.5, 1.0)
    values = torch.tensor([[0.1, 0.3, -0.2], [0.0, 1.0, 2.0]], dtype=torch.float64)
    Ho, Wo = 5, 9
    m = imaging.radial_map(values, fields, (Ho, Wo), v0=0.5, aspect=1.0)
    assert m.shape == (2, Ho, Wo, 1)
    assert torch.allclose(m[:, 2, 4, 0], torch.full((2,), 0.5, dtype=torch.float64)), "the centre node"
    assert torch.allclose(m[:, 0, 0, 0], values[:, 2]) and torch.allclose(m[:, 4, 8, 0], values[:, 2]), "the corner is h = 1"
    # along the middle row h = |x| / sqrt(2): x = +-0.5 -> 0.3536, between the nodes 0.25 and 0.5
    h = 0.5 / 2 ** 0.5
    want = values[:, 0] + (h - 0.25) / 0.25 * (values[:, 1] - values[:, 0])
    assert torch.allclose(m[:, 2, 6, 0], want) and torch.allclose(m[:, 2, 2, 0], want)
    short = imaging.radial_map(values[:, :2], fields[:2], (Ho, Wo), v0=0.5, aspect=1.0)
    assert torch.allclose(short[:, 0, 0, 0], values[:, 1]) and torch.allclose(short[:, 0, 8, 0], values[:, 1]), "held beyond the last field"
    at_node = imaging.radial_map(values, (0.25, 0.5, 1.0), (1, 5), v0=0.5, aspect=1e6)      # h = |x|: -1, -0.5, 0, 0.5, 1
    assert torch.allclose(at_node[:, 0, :, 0], torch.stack((values[:, 2], values[:, 1], torch.full((2,), 0.5, dtype=torch.float64),
                                                            values[:, 1], values[:, 2]), dim=1), atol=1e-9)
    rgb = imaging.radial_map(values[:, :, None].expand(2, 3, 3), fields, (Ho, Wo), v0=1.0)
    assert rgb.shape == (2, Ho, Wo, 3)
    with pytest.raises(ValueError, match="ascending"):
        imaging.radial_map(values, (0.5, 0.25, 1.0), (Ho, Wo))
    with pytest.raises(ValueError, match="samples"):
        imaging.radial_map(values, (0.5, 1.0), (Ho, Wo))


def test_distortion_grid_identity_and_pure_magnification():
    Ho, Wo = 6, 11
    xi, yi = _grid(Ho, Wo)
    x, y = imaging.distortion_grid(torch.zeros((2, 3), dtype=torch.float64), (0.3, 0.6, 1.0), (Ho, Wo))
    assert x.shape == (2, Ho, Wo) and torch.equal(x, xi.expand(2, -1, -1)) and torch.equal(y, yi.expand(2, -1, -1))
    d = 0.04
    # a constant d is a constant D only beyond the first field (the centre node is 0): place the first field inside the centre pixel's reach
    x, y = imaging.distortion_grid(torch.full((1, 2), d, dtype=torch.float64), (1e-9, 1.0), (Ho, Wo))
    assert torch.allclose(x, xi / (1 + d)) and torch.allclose(y, yi / (1 + d))


def test_gradients_of_the_helpers_with_respect_to_the_values():
    g = torch.Generator().manual_seed(5)
    fields = (0.2, 0.55, 0.8, 1.0)
    v = (torch.rand((2, 4, 3), generator=g, dtype=torch.float64) * 0.2).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a: imaging.radial_map(a, fields, (5, 7), 1.0), (v,))
    d = (torch.rand((2, 4), generator=g, dtype=torch.float64) * 0.1 - 0.05).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a: torch.stack(imaging.distortion_grid(a, fields, (5, 7))), (d,))


# ------------------------------------------------------------------------------------------------------------------ C ABI

def _geom(B=2, H=5, W=6, Cc=3, Ho=4, Wo=7, cb=2, gb=2, gc=3):
    q = _lib.tl_warp_geom(device=0, B=B, H=H, W=W, C=Cc, Ho=Ho, Wo=Wo, coord_batch=cb, gain_batch=gb, gain_channels=gc)
    q.image_stride[:] = (H * W * Cc, W * Cc, Cc, 1)
    q.x_stride[:] = q.y_stride[:] = q.g_x_stride[:] = q.g_y_stride[:] = (Ho * Wo, Wo, 1)
    q.gain_stride[:] = q.g_gain_stride[:] = (Ho * Wo * gc, Wo * gc, gc, 1)
    return q


def test_entry_points_are_declared_bound_and_exported_and_the_abi_version_stays():
    hdr = open(os.path.join(ROOT, "include", "tl_trace.h")).read()
    declared = set(re.findall(r"\b(tl_[a-z0-9_]+)\s*\(", hdr))
    dll = _lib.lib()
    for name in ("tl_warp_fwd", "tl_warp_bwd"):
        assert name in declared and name in _lib.EXPORTS and hasattr(dll, name), name
        assert _lib._SIGNATURES[name][1][0] is C.POINTER(_lib.tl_warp_geom)
    assert declared == set(_lib.EXPORTS)
    assert dll.tl_version() == _lib.TL_ABI_VERSION == 15
    assert int(re.search(r"#define TL_ABI_VERSION (\d+)", hdr).group(1)) == 15
    body = re.search(r"typedef struct tl_warp_geom \{(.*?)\} tl_warp_geom;", hdr, re.S).group(1)
    members = re.findall(r"\b(\w+)(?:\[\d\])?\s*[;,]", re.sub(r"/\*.*?\*/", "", body))
    assert members == [n for n, _ in _lib.tl_warp_geom._fields_], members


def test_bad_arguments_are_refused_before_any_device_call():
    dll = _lib.lib()
    fwd = lambda q, image=ONE, x=ONE, y=ONE, gain=ONE, out=ONE: dll.tl_warp_fwd(C.byref(q), image, x, y, gain, out, None)  # noqa: E731
    bwd = lambda q, image=ONE, x=ONE, y=ONE, gain=ONE, g_out=ONE, g_x=ONE, g_y=ONE, g_gain=ONE: dll.tl_warp_bwd(       # noqa: E731
        C.byref(q), image, x, y, gain, g_out, g_x, g_y, g_gain, None)

    def refused(rc, *words):
        msg = dll.tl_last_error()
        assert rc == EINVAL and all(w in msg for w in words), (rc, msg, words)

    for fn, name in ((fwd, b"tl_warp_fwd"), (bwd, b"tl_warp_bwd")):
        for size in ("B", "H", "W", "Cc", "Ho", "Wo"):
            refused(fn(_geom(**{size: 0})), name, b">= 1")
        refused(fn(_geom(cb=3)), name, b"coord_batch")
        refused(fn(_geom(cb=1, gb=3)), name, b"gain_batch")
        refused(fn(_geom(gc=2)), name, b"gain_channels")
        refused(fn(_geom(H=(1 << 20) + 1)), name, b"2^20")
        for arg in ("image", "x", "y"):
            refused(fn(_geom(), **{arg: None}), name, arg.encode())
    refused(fwd(_geom(), out=None), b"tl_warp_fwd", b"out")
    refused(bwd(_geom(), g_out=None), b"tl_warp_bwd", b"g_out")
    refused(bwd(_geom(), g_x=None), b"tl_warp_bwd", b"g_x")
    refused(bwd(_geom(), g_y=None), b"tl_warp_bwd", b"g_y")
    refused(bwd(_geom(), g_x=None, g_y=None, g_gain=None), b"tl_warp_bwd", b"nothing")
    refused(bwd(_geom(), gain=None), b"tl_warp_bwd", b"g_gain", b"gain is NULL")
    # without a gain its extents are not read
    q = _geom(gb=7, gc=9)
    refused(fwd(q, gain=None, out=None), b"tl_warp_fwd", b"out")
    rc = dll.tl_warp_fwd(None, ONE, ONE, ONE, ONE, ONE, None)
    refused(rc, b"tl_warp_fwd", b"g is NULL")


# ------------------------------------------------------------------------------------------------------- Python layer

def test_errors_of_the_python_layer():
    image = torch.rand((2, 5, 6, 3))
    x, y = torch.zeros((2, 4, 7)), torch.zeros((2, 4, 7))
    for fused in (None, False, True):
        with pytest.raises(ValueError, match=r"image must be \[B, H, W, C\], got \(5, 6, 3\)"):
            imaging.warp_bicubic(image[0], x, y, fused=fused)
        with pytest.raises(ValueError, match=r"got \(3, 4, 7\)"):
            imaging.warp_bicubic(image, torch.zeros((3, 4, 7)), torch.zeros((3, 4, 7)), fused=fused)
        with pytest.raises(ValueError, match=r"\(2, 4, 7\) and \(2, 4, 8\)"):
            imaging.warp_bicubic(image, x, torch.zeros((2, 4, 8)), fused=fused)
        with pytest.raises(ValueError, match=r"gain must be .* got \(2, 4, 7, 2\)"):
            imaging.warp_bicubic(image, x, y, torch.ones((2, 4, 7, 2)), fused=fused)
        with pytest.raises(ValueError, match=r"gain must be .* got \(2, 7, 4, 3\)"):
            imaging.warp_bicubic(image, x, y, torch.ones((2, 7, 4, 3)), fused=fused)
        with pytest.raises(ValueError, match="at least 1"):
            imaging.warp_bicubic(image, x[:, :0], y[:, :0], fused=fused)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        imaging.warp_bicubic(image, x, y, fused=True)                                   # CPU tensors
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        imaging.warp_bicubic(image.double(), x.double(), y.double(), fused=True)         # float64
    assert imaging.warp_bicubic(image[:1], x[:1], y[:1], torch.ones((1, 4, 7, 1))).shape == (1, 4, 7, 3)
    assert imaging.warp_bicubic(image, x[:1], y[:1]).shape == (2, 4, 7, 3)


def test_fused_with_an_image_gradient_is_refused_and_says_why():
    image = torch.rand((1, 5, 6, 3), requires_grad=True)
    x = torch.zeros((1, 4, 7))
    with pytest.raises(RuntimeError, match="image requires a gradient.*scatter"):
        imaging.warp_bicubic(image, x, x, fused=True)
    with torch.no_grad():                                    # no graph is recorded: the image's flag does not matter
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            imaging.warp_bicubic(image, x, x, fused=True)
    out = imaging.warp_bicubic(image, x, x)                  # fused=None takes the torch path
    out.sum().backward()
    assert image.grad is not None and float(image.grad.sum()) == pytest.approx(4 * 7 * 3)
