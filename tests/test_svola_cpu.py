"""imaging.svola_convolution without a GPU: the torch path (fused=False, float64) against the independent reference
tests/svola_ref.py, the patch geometry against hand-written expectations, analytic pins of the definition, the C ABI of the
tl_svola_* entry points (declared, bound, exported, refusing bad arguments before any HIP call) and the errors of the Python
layer."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import svola_cases as sc
import svola_ref as ref

from torchoptics_amd import _lib, imaging

# The shared table (tests/svola_cases.py); this file has always named the shapes without their number.
SHAPES = {name.split("-", 1)[1]: case for name, case in sc.CASES.items()}


@pytest.mark.parametrize("name", list(SHAPES))
def test_the_torch_path_is_the_reference_in_float64(name):
    B, H, W, Cc, grid, k, ov, win, pb = SHAPES[name]
    image, psfs, g_out = ref.make_case(B, H, W, Cc, grid, k, seed=11, psf_batch=pb)
    want = ref.ref_with_grads(image, ov, psfs, grid, win, g_out)
    im, ps = image.clone().requires_grad_(True), psfs.clone().requires_grad_(True)
    out = imaging.svola_convolution(im, ov, ps, grid, win, fused=False)
    assert out.shape == (B, H, W, Cc) and out.dtype == torch.float64
    (out * g_out).sum().backward()
    for what, got, exp in zip(("out", "g_image", "g_psfs"), (out.detach(), im.grad, ps.grad), want):
        err = ((got - exp).abs().max() / exp.abs().max()).item()
        assert err <= 1e-12, (name, what, err)
    dflt = imaging.svola_convolution(image, ov, psfs, grid, win)            # fused=None on the CPU: the same torch path
    assert torch.equal(dflt, out.detach())


@pytest.mark.parametrize("H,g,o,r0,r1", [(23, 2, 2, [0, 12], [15, 27]), (29, 3, 3, [0, 10, 20], [15, 25, 35]),
                                         (70, 3, 5, [0, 24, 47], [33, 57, 80]),          # 23.5 rounds to even
                                         (131, 4, 5, [0, 33, 66, 99], [42, 75, 108, 141]), (40, 1, 0, [0], [40])])
def test_patch_bounds(H, g, o, r0, r1):
    for win in ("boxcar", "hann"):
        geo = imaging.svola_geometry(H, 40, g, 1, o, 0, win)
        assert geo.r0.tolist() == r0 and geo.r1.tolist() == r1 and geo.ph == H // g + 2 * o
        assert geo.c0.tolist() == [0] and geo.c1.tolist() == [40]
        geo_t = imaging.svola_geometry(40, H, 1, g, 0, o, win)                 # the same along the columns
        assert geo_t.c0.tolist() == r0 and geo_t.c1.tolist() == r1 and geo_t.pw == H // g + 2 * o
        assert np.allclose(geo.tab_r.sum(axis=0)[o:o + H], 1.0, atol=1e-15)
        assert geo.win_r.shape == (geo.ph,) and (geo.win_r > 0).all()
        assert imaging.svola_geometry(H, 40, g, 1, o, 0, win) is geo           # memoised
    x = np.linspace(0, 1, geo.ph + 2)[1:-1]
    assert np.array_equal(geo.win_r, np.sin(np.pi * x) ** 2)


def test_an_uncovered_pixel_is_refused_and_the_axis_named():
    with pytest.raises(ValueError, match="row 11"):
        imaging.svola_geometry(23, 40, 2, 1, 0, 0, "boxcar")
    with pytest.raises(ValueError, match="column 11"):
        imaging.svola_geometry(40, 23, 1, 2, 0, 0, "hann")
    image, psfs, _ = ref.make_case(1, 23, 40, 1, (2, 1), (3, 3), seed=0)
    with pytest.raises(ValueError, match="row 11"):
        imaging.svola_convolution(image, 0, psfs, (2, 1))
    with pytest.raises(ValueError, match="window_type"):
        imaging.svola_geometry(24, 24, 2, 2, 1, 1, "hamming")


def _delta(B, N, kh, kw, Cc, i, j):
    psfs = torch.zeros((B, N, kh, kw, Cc), dtype=torch.float64)
    psfs[:, :, i, j, :] = 1.0
    return psfs


@pytest.mark.parametrize("win", ["boxcar", "hann"])
def test_analytic_pins(win):
    B, H, W, Cc, grid, (kh, kw), ov = 2, 23, 29, 2, (2, 3), (5, 3), (2, 3)
    image = ref.make_case(B, H, W, Cc, grid, (kh, kw), seed=5)[0]
    a, b = kh // 2, kw // 2
    conv = lambda psfs: imaging.svola_convolution(image, ov, psfs, grid, win, fused=False)      # noqa: E731
    # a centred delta everywhere: the image itself
    out = conv(_delta(B, 6, kh, kw, Cc, a, b))
    assert ((out - image).abs() <= 4 * 2.0 ** -53 * image.abs()).all()
    # a delta one tap below the centre: the image one row down, the top row equal to itself by the symmetric edge
    out = conv(_delta(B, 6, kh, kw, Cc, a + 1, b))
    shifted = torch.cat((image[:, :1], image[:, :-1]), dim=1)
    assert ((out - shifted).abs() <= 4 * 2.0 ** -53 * shifted.abs()).all()
    # unit-sum PSFs on a constant image: that constant
    psfs = ref.make_case(B, H, W, Cc, grid, (kh, kw), seed=6)[1]
    out = imaging.svola_convolution(torch.full_like(image, 0.75), ov, psfs, grid, win, fused=False)
    assert (out - 0.75).abs().max() <= (kh * kw + 8) * 2.0 ** -53
    # a single bright pixel in the interior of one patch: that patch's PSF around it, not flipped
    geo = imaging.svola_geometry(H, W, *grid, *ov, win)
    cover = ref.n_cover(H, W, grid, ov)
    n = 4                                                  # patch (1, 1)
    y = int(geo.r0[1]) - ov[0] + geo.ph // 2 + 2
    x = int(geo.c0[1]) - ov[1] + geo.pw // 2
    assert (cover[y - a:y + a + 1, x - b:x + b + 1] == 1).all(), "the test's pixel must sit where only one patch covers"
    point = torch.zeros_like(image)
    point[:, y, x, :] = 1.0
    out = imaging.svola_convolution(point, ov, psfs, grid, win, fused=False)
    assert torch.allclose(out[:, y - a:y + a + 1, x - b:x + b + 1, :], psfs[:, n], rtol=0, atol=1e-15)
    assert not torch.allclose(out[:, y - a:y + a + 1, x - b:x + b + 1, :], psfs[:, n].flip(1, 2), atol=1e-3)
    assert out.sum().item() == pytest.approx(B * Cc, abs=1e-12)


# ---------------------------------------------------------------------------------------------------------------- C ABI

NAMES = ("tl_svola_workspace_bytes", "tl_svola_fwd", "tl_svola_bwd_psf", "tl_svola_bwd_image")
EINVAL, EWORKSPACE = -1, -3                 # TL_EINVAL, TL_EWORKSPACE (include/tl_trace.h)
ONE = C.c_void_p(8)                         # any non-NULL pointer: never dereferenced on the paths taken here


def test_entry_points_are_declared_bound_and_exported_and_the_abi_version_stays():
    hdr = open(os.path.join(ROOT, "include", "tl_trace.h")).read()
    declared = set(re.findall(r"\b(tl_[a-z0-9_]+)\s*\(", hdr))
    dll = _lib.lib()
    for name in NAMES:
        assert name in declared and name in _lib.EXPORTS and hasattr(dll, name), name
    assert dll.tl_version() == 15 == _lib.TL_ABI_VERSION
    assert int(re.search(r"#define TL_ABI_VERSION (\d+)", hdr).group(1)) == 15
    assert C.sizeof(_lib.tl_problem) == dll.tl_problem_size() == 248
    assert C.sizeof(_lib.tl_svola_geom) == 12 * 4 + 14 * 8


def _geom(B=2, H=23, W=29, Cc=2, pb=2, gh=2, gw=3, kh=5, kw=3, oh=2, ow=3):
    q = _lib.tl_svola_geom(device=0, B=B, H=H, W=W, C=Cc, psf_batch=pb, gh=gh, gw=gw, kh=kh, kw=kw, oh=oh, ow=ow)
    q.image_stride[:] = (H * W * Cc, W * Cc, Cc, 1)
    q.psfs_stride[:] = (gh * gw * kh * kw * Cc, kh * kw * Cc, kw * Cc, Cc, 1)
    q.g_psfs_stride[:] = q.psfs_stride[:]
    return q


def _bounds(H=23, W=29, gh=2, gw=3, oh=2, ow=3):
    r0, r1, _ = ref.patch_starts(H, gh, oh)
    c0, c1, _ = ref.patch_starts(W, gw, ow)
    return [(C.c_int32 * len(v))(*v.tolist()) for v in (r0, r1, c0, c1)]


def _calls(dll, q, bounds, ptrs=None, ws=ONE, ws_bytes=1 << 30):
    """The three launching entry points with pointers that are never dereferenced: [(name, return code, message)]."""
    p = dict(wr=ONE, wc=ONE, image=ONE, psfs=ONE, out=ONE, g_out=ONE, g_psfs=ONE, g_image=ONE)
    p.update(ptrs or {})
    g = C.byref(q) if q is not None else None
    dll.tl_unsup_loss(0, 0, 3, 100.0, ONE, None, 7.0, 0.2, ONE, ONE, ONE, ONE, None)       # another call's message first
    done = []
    for name, call in (
            (b"tl_svola_fwd", lambda: dll.tl_svola_fwd(g, *bounds, p["wr"], p["wc"], p["image"], p["psfs"], p["out"], None)),
            (b"tl_svola_bwd_psf", lambda: dll.tl_svola_bwd_psf(g, *bounds, p["wr"], p["wc"], p["image"], p["g_out"], p["g_psfs"],
                                                               ws, ws_bytes, None)),
            (b"tl_svola_bwd_image", lambda: dll.tl_svola_bwd_image(g, *bounds, p["wr"], p["wc"], p["psfs"], p["g_out"],
                                                                   p["g_image"], ws, ws_bytes, None))):
        rc = call()
        done.append((name, rc, dll.tl_last_error() if rc else b""))
    return done


BAD_GEOM = [(dict(kh=4), b"kh"), (dict(kw=2), b"kw"), (dict(kh=33), b"kh"), (dict(kw=33), b"kw"),      # even or > 31
            (dict(oh=22), b"oh"), (dict(ow=29), b"ow"),                                                 # the padding rule
            (dict(gh=0), b"gh"), (dict(gw=129), b"gw"), (dict(pb=3), b"psf_batch"), (dict(B=0), b"B"), (dict(Cc=0), b"C"),
            (dict(Cc=65536), b"C <= 65535")]                                   # one more than a launch's grid z


@pytest.mark.parametrize("bad,word", BAD_GEOM, ids=lambda v: ",".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else "")
def test_bad_geometry_is_refused_before_any_hip_call(bad, word):
    dll = _lib.lib()
    q = _geom(**bad)
    assert dll.tl_svola_workspace_bytes(C.byref(q), *_bounds()) == 0
    for name, rc, msg in _calls(dll, q, _bounds()):
        assert rc == EINVAL, (name, bad)
        assert name + b":" in msg and word in msg, msg


def test_null_pointers_bad_bounds_and_a_small_workspace_are_refused():
    dll = _lib.lib()
    q, bounds = _geom(), _bounds()
    assert [rc for _, rc, _ in _calls(dll, None, bounds)] == [EINVAL] * 3
    for k in range(4):
        holed = list(bounds)
        holed[k] = None
        assert [rc for _, rc, _ in _calls(dll, q, holed)] == [EINVAL] * 3
        assert dll.tl_svola_workspace_bytes(C.byref(q), *holed) == 0
    used = {b"tl_svola_fwd": ("wr", "wc", "image", "psfs", "out"), b"tl_svola_bwd_psf": ("wr", "wc", "image", "g_out", "g_psfs"),
            b"tl_svola_bwd_image": ("wr", "wc", "psfs", "g_out", "g_image")}
    for key in ("wr", "wc", "image", "psfs", "out", "g_out", "g_psfs", "g_image"):
        for name, rc, _ in _calls(dll, q, bounds, {key: None}):
            if key in used[name]:
                assert rc == EINVAL, (name, key)
    assert dll.tl_svola_bwd_image(C.byref(q), *bounds, ONE, ONE, ONE, ONE, None, ONE, 1 << 30, None) == EINVAL
    assert b"tl_svola_bwd_image" in dll.tl_last_error() and b"g_image" in dll.tl_last_error()
    # patch bounds: another patch length, decreasing, outside the frame, a hole in the coverage
    shifted = _bounds()
    shifted[1][0] += 1
    assert [rc for _, rc, _ in _calls(dll, q, shifted)] == [EINVAL] * 3 and b"r0/r1" in dll.tl_last_error()
    swapped = _bounds()
    for arr in swapped[2:]:
        arr[0], arr[1] = arr[1], arr[0]
    assert [rc for _, rc, _ in _calls(dll, q, swapped)] == [EINVAL] * 3 and b"c0/c1" in dll.tl_last_error()
    outside = _bounds()
    outside[0][1] += 5
    outside[1][1] += 5
    assert [rc for _, rc, _ in _calls(dll, q, outside)] == [EINVAL] * 3 and b"r0/r1" in dll.tl_last_error()
    hole = [(C.c_int32 * 2)(0, 12), (C.c_int32 * 2)(11, 23), (C.c_int32 * 1)(0), (C.c_int32 * 1)(40)]
    qh = _geom(B=1, H=23, W=40, Cc=1, pb=1, gh=2, gw=1, kh=3, kw=3, oh=0, ow=0)
    assert [rc for _, rc, _ in _calls(dll, qh, hole)] == [EINVAL] * 3
    assert b"r0/r1" in dll.tl_last_error() and b"no patch" in dll.tl_last_error()
    # the workspace
    need = dll.tl_svola_workspace_bytes(C.byref(q), *bounds)
    assert need >= 2 * 2 * (23 + 4) * (29 + 2) * 4
    fwd, bwd_psf, bwd_image = _calls(dll, q, bounds, ws=None)
    assert bwd_psf[1] == EWORKSPACE and bwd_image[1] == EWORKSPACE
    fwd, bwd_psf, bwd_image = _calls(dll, q, bounds, ws_bytes=16)
    assert bwd_psf[1] == EWORKSPACE and bwd_image[1] == EWORKSPACE and b"tl_svola_bwd_image" in dll.tl_last_error()


def test_workspace_grows_with_the_batch_and_every_test_shape_plans():
    dll = _lib.lib()
    for name, (B, H, W, Cc, grid, k, ov, win, pb) in SHAPES.items():
        q = _geom(B, H, W, Cc, pb or B, grid[0], grid[1], k[0], k[1], ov[0], ov[1])
        b = _bounds(H, W, grid[0], grid[1], ov[0], ov[1])
        one = dll.tl_svola_workspace_bytes(C.byref(q), *b)
        assert one >= B * Cc * (H + k[0] - 1) * (W + k[1] - 1) * 4, name
        assert one == sc.workspace_bytes(B, H, W, Cc, grid, k, ov), name        # the planner's tiles under every patch
        q8 = _geom(8 * B, H, W, Cc, 8 * B if pb is None else 1, grid[0], grid[1], k[0], k[1], ov[0], ov[1])
        assert dll.tl_svola_workspace_bytes(C.byref(q8), *b) > one, name
        assert dll.tl_svola_workspace_bytes(C.byref(q8), *b) == sc.workspace_bytes(8 * B, H, W, Cc, grid, k, ov), name


def test_the_chunked_shapes_have_more_tiles_than_one_launch_takes():
    """The tile counts that make shapes 8 to 12 run more than one chunk on the GPU, from the Python statement of the tile
    cutting that test_workspace_... holds the planner to; and that statement on an axis small enough to do by hand."""
    # 70 rows, 3 patches of 33 at 0, 24, 47 of an 80-row frame, centre [5, 75): cells [5,24) [24,33) [33,47) [47,57) [57,75)
    assert sc.cut_tiles(70, 3, 5) == (5, [2, 3, 2])
    # 100 rows, one patch: four tiles of 25
    assert sc.cut_tiles(100, 1, 0) == (4, [4])
    for name, (rows, cols) in sc.TILE_COUNTS.items():
        B, H, W, Cc, grid, k, ov, win, pb = sc.CASES[name]
        assert (sc.cut_tiles(H, grid[0], ov[0])[0], sc.cut_tiles(W, grid[1], ov[1])[0]) == (rows, cols), name
        assert max(rows, cols) > sc.MAX_SEG, name
    rows, cols = sc.TILE_COUNTS["12-both-chunked"]
    assert rows > sc.MAX_SEG and cols > sc.MAX_SEG
    tiles, under = sc.cut_tiles(384, 128, 1)
    assert tiles - under[-1] > 2 * sc.MAX_SEG                 # the last patch starts in the third chunk (first_c > 192)


def test_the_torch_path_is_the_reference_on_the_fuzz_geometries():
    """The seeded draws of the GPU fuzz test through fused=False in float64: uneven geometries, both windows."""
    kept, skipped = sc.fuzz_survivors(imaging.svola_geometry)
    assert skipped <= sc.FUZZ_MAX_SKIPPED and len(kept) + skipped == sc.FUZZ_DRAWS, skipped
    for t, (B, H, W, Cc, grid, k, ov, win) in kept:
        image, psfs, g_out = ref.make_case(B, H, W, Cc, grid, k, seed=t)
        want = ref.ref_with_grads(image, ov, psfs, grid, win, g_out)
        im, ps = image.clone().requires_grad_(True), psfs.clone().requires_grad_(True)
        out = imaging.svola_convolution(im, ov, ps, grid, win, fused=False)
        (out * g_out).sum().backward()
        for what, got, exp in zip(("out", "g_image", "g_psfs"), (out.detach(), im.grad, ps.grad), want):
            err = ((got - exp).abs().max() / exp.abs().max()).item()
            assert err <= 1e-12, (t, (B, H, W, Cc, grid, k, ov, win), what, err)


# ------------------------------------------------------------------------------------------------------- Python layer

def test_errors_of_the_python_layer():
    image, psfs, _ = ref.make_case(2, 23, 29, 2, (2, 3), (5, 3), seed=1)
    f32 = lambda t: t.float()                                                               # noqa: E731
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        imaging.svola_convolution(f32(image), (2, 3), f32(psfs), (2, 3), fused=True)       # CPU tensors
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        imaging.svola_convolution(image, (2, 3), psfs, (2, 3), fused=True)                 # float64
    for fused in (None, False, True):
        with pytest.raises(ValueError, match="odd"):
            imaging.svola_convolution(image, (2, 3), psfs[:, :, :4], (2, 3), fused=fused)
        with pytest.raises(ValueError, match="needs 4"):
            imaging.svola_convolution(image, (2, 3), psfs, (2, 2), fused=fused)            # N != gh gw
        with pytest.raises(ValueError, match="must not exceed"):
            imaging.svola_convolution(image, (22, 3), psfs, (2, 3), fused=fused)           # 22 + 2 > 23
        with pytest.raises(ValueError, match="must not exceed"):
            imaging.svola_convolution(image, (2, 29), psfs, (2, 3), fused=fused)
    big = torch.rand((1, 1, 33, 3, 1), dtype=torch.float64)
    img = torch.rand((1, 40, 40, 1), dtype=torch.float64)
    with pytest.raises(ValueError, match="at most 31"):
        imaging.svola_convolution(img, 0, big, (1, 1), fused=True)                          # kh = 33
    assert imaging.svola_convolution(img, 0, big, (1, 1)).shape == (1, 40, 40, 1)           # the torch path has no such limit
    with pytest.raises(ValueError, match="does not fit"):
        imaging.svola_convolution(image, (2, 3), psfs[..., :1], (2, 3))


def test_psf_grid_from_fields_is_a_view():
    kernels = torch.rand((3, 2, 9, 7), dtype=torch.float64)
    psfs = imaging.psf_grid_from_fields(kernels, (3, 1))
    assert psfs.shape == (1, 3, 9, 7, 2) and psfs.data_ptr() == kernels.data_ptr()
    assert torch.equal(psfs[0, 2, :, :, 1], kernels[2, 1])
    same = imaging.psf_grid_from_fields(kernels, (3, 1), index_map=[[0], [1], [2]])
    assert same.data_ptr() == kernels.data_ptr()
    grid = imaging.psf_grid_from_fields(kernels, (2, 2), index_map=[[2, 1], [1, 0]])
    assert grid.shape == (1, 4, 9, 7, 2) and torch.equal(grid[0, 0, :, :, 0], kernels[2, 0]) and torch.equal(grid[0, 3], psfs[0, 0])
    with pytest.raises(ValueError):
        imaging.psf_grid_from_fields(kernels, (2, 2))
    with pytest.raises(ValueError):
        imaging.psf_grid_from_fields(kernels, (2, 2), index_map=[[0, 1], [2, 3]])
