"""The rotated PSF grid kernels (tl_psf_rot_accumulate / _bwd behind ops.PsfRotAccumulateFunction) on the GPU: every element
of hist, gx and gy of every case of tests/psf_rot_ref.py against its float64 reference within the derived bounds; g_y_centre
against the float64 sum of the kernel's own gy; exact pins against the plain kernels at the four right angles; every backward
instantiation; weight kinds, hostile dead rays, strides, partial gradients; then imaging.psf_grid_from_trace(fused=True)
against fused=False with the yardstick of tests/test_gpu_psf_fused.py, and a traced Cooke triplet rendered through a 3 x 3 grid.
The lines "PSF-ROT-BND ..." and "PSF-ROT-ACC ..." are kept in profiles/psf_rot_accuracy.txt."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import psf_cases as pc
import psf_rot_ref as rr
from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 4.0                                # tests/test_gpu_psf_fused.py: a fused error is at most 4 x the unfused fp32 error
GATE = 1e-5                                 # and its gate on leaf gradients, fused against unfused
ALL = rr.RESULTS + ("g_y_centre",)
_RUNS = {}


@pytest.fixture(scope="module")
def ops():
    from torchoptics_amd import _lib, ops
    _lib.lib()
    return ops


def _clean(ops, name):
    """The op on a case as it stands in the table: run once, shared, never changed."""
    if name not in _RUNS:
        a = rr.inputs(name)
        _RUNS[name] = rr.run(ops, rr.tensors(a, DEV), a)
    return _RUNS[name]


def _assert_same_bits(got, want, names=ALL, what=""):
    for k in names:
        assert pc.same_bits(got[k], want[k]), f"{what}: {k} differs"


def _held(label, got, r, a):
    """Print the line of a run and hold every result to its bound."""
    q = rr.ratios(got, r)
    q["g_y_centre"] = rr.centre_ratio(got["g_y_centre"], got["gy"])
    K, W, R = a.shape
    rel = float(np.max(np.abs(got["g_y_centre"].astype(np.float64) - r.g_y_centre) / np.maximum(np.abs(r.g_y_centre), 1e-300)))
    print(f"PSF-ROT-BND {label} {K}x{W}x{R} G={a.G} {a.ny}x{a.nx}: largest error / bound hist {q['hist']:.3f} gx {q['gx']:.3f} "
          f"gy {q['gy']:.3f}; g_y_centre / sum tolerance {q['g_y_centre']:.3f} (relative to the float64 reference {rel:.2e})")
    for k in ALL:
        assert got[k].dtype == np.float32 and np.isfinite(got[k]).all(), k
    assert max(q.values()) <= 1.0, (label, q)


# --------------------------------------------------------------------------------------------------------- 1. every case
@pytest.mark.parametrize("name", list(rr.CASES))
def test_every_case_within_its_bounds_and_the_same_bits_twice(ops, name):
    a, r = rr.inputs(name), rr.reference(name)
    got = _clean(ops, name)
    again = rr.run(ops, rr.tensors(a, DEV), a)
    _assert_same_bits(again, got, what=name)
    K, W, R = a.shape
    assert got["hist"].shape == (a.G, W, a.ny, a.nx) and got["gx"].shape == got["gy"].shape == a.shape
    assert got["g_y_centre"].shape == (K,)
    _held(name, got, r, a)
    if name == "shared":                                    # fan 2 is read by no grid: exactly +0.0
        assert 2 not in a.src
        for k in ("gx", "gy"):
            assert not got[k][2].view(np.uint32).any(), k
        assert got["g_y_centre"][2] == 0 and got["gx"][1].any()
    if name == "dead-channel":
        k, w = rr.DEAD_CHANNEL
        assert not got["gx"][k, w].any() and not got["gy"][k, w].any()
        for g in np.nonzero(a.src == k)[0]:
            assert not got["hist"][g, w].any()
        assert got["hist"][0, 0].all() and got["gx"][0, 0].any()
    if name == "many-rows":
        assert a.G * W == 65792 > 65535


# -------------------------------------------------------------------------------------- 2. the right angles, bit for bit
PIN = (3, 2, 257, 32, 25)                                   # K = G, W, R, ny, nx: two blocks each way


def _pin_inputs():
    """The rays stay on the tile and 1.5 pixels around it: no live ray's gradient underflows to an exact zero, whose sign the
    turn back (x + 0 y) would not keep."""
    K, W, R, ny, nx = PIN
    return rr.make_inputs(K, W, R, np.arange(K), ny, nx, "float", seed=77, angles=np.zeros(K), tile=True)


def _plain(ops, a, x, y, yc):
    """The plain kernels (ops.PsfAccumulateFunction) on the full grid: nxh = nx, x_first = 0.5 - nx/2."""
    b = SimpleNamespace(x=x, y=y, weight=a.weight, x_pitch=a.x_pitch, y_pitch=a.y_pitch, y_centre=yc, T=a.T, nxh=a.nx, ny=a.ny,
                        x_first=a.x_first, y_first=a.y_first, shape=a.shape)
    return pc.run(ops, pc.tensors(b, DEV), b)


def test_the_identity_has_the_bits_of_the_plain_kernels(ops):
    a = _pin_inputs()
    assert (a.c == 1).all() and (a.s == 0).all()
    got = rr.run(ops, rr.tensors(a, DEV), a)
    want = _plain(ops, a, a.x, a.y, a.y_centre)
    _assert_same_bits(got, want, what="identity")
    assert got["hist"].any() and got["gx"].any()


@pytest.mark.parametrize("c,s", [(0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)])
def test_a_right_angle_has_the_bits_of_the_plain_kernels_on_turned_coordinates(ops, c, s):
    """x' = c xi + s eta, y' = -s xi + c eta: the plain call is fed (x', y') about a centre of 0, and its gradients are turned
    back by hand (gx = c gx' - s gy', gy = s gx' + c gy').  No tolerance: this pins the sign convention.  The sign of an exact
    zero aside (a dead ray's -0.0 after a negation), hence == and not a comparison of bits for the gradients."""
    a = _pin_inputs()
    a.c[:], a.s[:] = c, s
    xi, eta = a.x, a.y - a.y_centre[:, None, None]           # the float32 difference the kernel forms
    assert eta.dtype == np.float32
    xr, yr = {(0.0, 1.0): (eta, -xi), (-1.0, 0.0): (-xi, -eta), (0.0, -1.0): (-eta, xi)}[(c, s)]
    got = rr.run(ops, rr.tensors(a, DEV), a)
    want = _plain(ops, a, xr, yr, np.zeros_like(a.y_centre))
    assert pc.same_bits(got["hist"], want["hist"])
    gx = np.float32(c) * want["gx"] - np.float32(s) * want["gy"]
    gy = np.float32(s) * want["gx"] + np.float32(c) * want["gy"]
    assert np.array_equal(got["gx"], gx) and np.array_equal(got["gy"], gy) and got["gx"].any()
    _held(f"right angle c={c:+.0f} s={s:+.0f}", got, rr.evaluate(a), a)


# ---------------------------------------------------------------------------------------------- 3. all eight instantiations
@pytest.mark.parametrize("nx", rr.SWEEP_NX)
def test_every_instantiation_of_the_backward(ops, nx):
    a, r = rr.inputs(("sweep", nx)), rr.reference(("sweep", nx))
    assert a.shape == (2, 3, 321) and a.ny == 3 and a.G == 4
    _held(f"nx={nx}", rr.run(ops, rr.tensors(a, DEV), a), r, a)


# ----------------------------------------------------------------------------------------------------- 4. the same bits
def test_bytes_bools_and_floats_of_0_and_1_give_the_same_bits(ops):
    a = rr.inputs("block-edge")
    live = a.weight != 0
    runs = []
    for w in (live.astype(np.float32), live, live.astype(np.uint8)):
        t = rr.tensors(a, DEV)
        t["weight"] = torch.from_numpy(w).to(DEV)
        runs.append(rr.run(ops, t, a))
    _assert_same_bits(runs[1], runs[0], what="bool")
    _assert_same_bits(runs[2], runs[0], what="uint8")
    _held("block-edge 0/1 weights", runs[0], rr.evaluate(a, weight=live.astype(np.float64)), a)


def test_a_ray_of_weight_0_changes_no_bit_whatever_its_coordinates(ops):
    a = rr.inputs("block-edge")
    clean = _clean(ops, "block-edge")
    dead = torch.from_numpy(a.weight == 0).to(DEV)
    assert dead.any()
    for bad in (float("nan"), float("inf"), 1e30):
        t = rr.tensors(a, DEV)
        t["x"][dead] = bad
        t["y"][dead] = bad
        got = rr.run(ops, t, a)
        _assert_same_bits(got, clean, what=f"{bad}")
        assert not got["gx"][a.weight == 0].any() and not got["gy"][a.weight == 0].any()


def test_a_strided_x_is_read_in_place_and_gives_the_bits_of_the_contiguous_run(ops):
    a = rr.inputs("block-edge")
    K, W, R = a.shape
    clean = _clean(ops, "block-edge")
    t = rr.tensors(a, DEV)
    big = torch.zeros((K + 1, W + 2, R + 5), device=DEV).requires_grad_(True)
    with torch.no_grad():
        big[1:, 1:W + 1, 3:3 + R] = t["x"]
    xv = big[1:, 1:W + 1, 3:3 + R]
    assert xv.stride() == ((W + 2) * (R + 5), R + 5, 1) and xv.stride(0) != W * xv.stride(1) and not xv.is_contiguous()
    t["x"] = xv
    got = rr.run(ops, t, a)
    assert got["saved_x_ptr"] == xv.data_ptr(), "a strided x with contiguous rays must reach the kernel without a copy"
    _assert_same_bits(got, clean, what="strided")
    g = big.grad.cpu().numpy()
    assert np.array_equal(g[1:, 1:W + 1, 3:3 + R], clean["gx"])
    g[1:, 1:W + 1, 3:3 + R] = 0
    assert not g.any()


@pytest.mark.parametrize("needs", [("y_centre",), ("x",), ("y", "y_centre")], ids=lambda n: "+".join(n))
def test_a_gradient_that_is_asked_for_alone_has_the_bits_of_the_full_run(ops, needs):
    a = rr.inputs("block-edge")
    full = _clean(ops, "block-edge")
    got = rr.run(ops, rr.tensors(a, DEV), a, needs=needs)
    assert pc.same_bits(got["hist"], full["hist"])
    for n, k in zip(rr.LEAVES, ("gx", "gy", "g_y_centre")):
        if n in needs:
            assert pc.same_bits(got[k], full[k]), k
        else:
            assert got[k] is None, k


# ------------------------------------------------------------------------------------------- 5. through the Python layer
F, W = 3, 3


def _fan(R, seed):
    """Three fields at y = 0 .. 3 mm, three channels, comatic towards +y; every 7th ray failed.  fp32 CPU tensors in the
    tracer's [1, F, P, W] (memory [1, F, W, P])."""
    rng = np.random.default_rng(seed)
    hf = np.linspace(0, 1, F)[None, :, None, None]
    rho, th = np.sqrt(rng.uniform(0, 1, (1, F, W, R))), rng.uniform(0, 2 * np.pi, (1, F, W, R))
    x = 0.01 * rho * np.cos(th) + 0.01 * hf * rho ** 2 * np.sin(2 * th)
    y = 3.0 * hf + 0.01 * rho * np.sin(th) + 0.01 * hf * rho ** 2 * (2 + np.cos(2 * th))
    ok = np.broadcast_to(np.arange(R) % 7 != 0, x.shape).copy()
    return tuple(torch.from_numpy(v).permute(0, 1, 3, 2) for v in (x.astype(np.float32), y.astype(np.float32), ok))


def _eval(imaging, x, y, ok, yt, cells, T, n_bins, inc, fused):
    x, y, yt = (v.clone().requires_grad_(True) for v in (x, y, yt))
    p = imaging.psf_grid_from_trace(x, y, ok, cells, n_bins, inc, y_target=yt, fused=fused)
    (p * T).sum().backward()
    return p.detach(), x.grad, y.grad, yt.grad


@pytest.mark.parametrize("shape,size", [((3, 3), (48, 48)), ((2, 5), (40, 60))])
def test_psf_grid_from_trace_fused_against_the_float64_definition(ops, shape, size):
    from torchoptics_amd import imaging
    x, y, ok = _fan(4099, seed=shape[1])
    cells = imaging.psf_grid_cells(size, shape, 4, (0.0, 0.6, 1.0))
    n_bins, inc = (21, 19), float(np.float32(0.004))
    yt = (torch.linspace(0, 3, F) + 0.02 * torch.linspace(0, 1, F) + torch.tensor([1e-3, -2e-3, 5e-4])).float()
    T = torch.randn((1, cells.N, n_bins[1], n_bins[0], W), generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    ora = _eval(imaging, x.double(), y.double(), ok, yt.double(), cells, T, n_bins, inc, False)
    dev = [v.to(DEV) for v in (x, y, ok, yt)]
    unf = _eval(imaging, *dev, cells, T.float().to(DEV), n_bins, inc, False)
    fus = _eval(imaging, *dev, cells, T.float().to(DEV), n_bins, inc, True)
    assert fus[0].shape == (1, cells.N, n_bins[1], n_bins[0], W) and fus[0].dtype == torch.float32
    assert torch.allclose(fus[0].sum(dim=(2, 3)), torch.ones(1, cells.N, W, device=DEV), atol=1e-5)
    rows = []
    for i, name in enumerate(("values", "grad x", "grad y", "grad y_target")):
        if i == 0:
            peak = ora[0].amax(dim=(2, 3), keepdim=True)
            eu = float(((unf[0].double().cpu() - ora[0]).abs() / peak).max())
            ef = float(((fus[0].double().cpu() - ora[0]).abs() / peak).max())
        else:
            eu, ef = rel_l2(unf[i].cpu().numpy(), ora[i].numpy()), rel_l2(fus[i].cpu().numpy(), ora[i].numpy())
        print(f"PSF-ROT-ACC grid {shape[0]}x{shape[1]} {name}: fused {ef:.3e} unfused {eu:.3e} ratio {ef / max(eu, 1e-300):.2f}")
        rows.append((name, ef, eu))
    for name, ef, eu in rows:
        assert np.isfinite(ef) and ef <= MARGIN * eu, f"{shape} {name}: fused {ef:.3e} > {MARGIN} x unfused {eu:.3e}"
    dead = ~ok.to(DEV)
    assert (fus[1][dead] == 0).all() and (fus[2][dead] == 0).all() and (fus[1][~dead] != 0).any()


def test_the_default_takes_the_kernels_when_they_apply_and_two_lenses_are_two_grids(ops):
    from torchoptics_amd import imaging
    x, y, ok = (v.to(DEV) for v in _fan(515, seed=3))
    cells = imaging.psf_grid_cells((48, 48), (3, 3), 4, (0.0, 0.6, 1.0))
    one = imaging.psf_grid_from_trace(x, y, ok, cells, (9, 9), 0.006, fused=True)
    auto = imaging.psf_grid_from_trace(x, y, ok, cells, (9, 9), 0.006)
    plain = imaging.psf_grid_from_trace(x, y, ok, cells, (9, 9), 0.006, fused=False)
    assert torch.equal(auto, one if imaging.PSF_GRID_FUSED_BY_DEFAULT else plain)
    x2, y2, ok2 = torch.cat((x, 1.1 * x)), torch.cat((y, y)), torch.cat((ok, ok))
    two = imaging.psf_grid_from_trace(x2, y2, ok2, cells, (9, 9), 0.006, fused=True)
    assert two.shape == (2, 9, 9, 9, 3) and not torch.equal(two[1], one[0])
    want = imaging.psf_grid_from_trace(x2, y2, ok2, cells, (9, 9), 0.006, fused=False)
    # 68 roundings of hist, as many of its sum, the fp32 torch path's own: 1e-5 of the peak is two hundred U
    # (the first lens need not have the BITS of the one-lens call: torch's normalising sum is free to take a tensor of
    # another shape in another order)
    assert float((two - want).abs().max()) <= 1e-5 * float(want.max())
    assert float((two[0] - one[0]).abs().max()) <= 1e-5 * float(one.max())


# ------------------------------------------------------------------------------------------------------- 6. end to end
def test_leaf_gradients_of_a_rendered_image_through_the_trace(ops):
    import yaml_free_lenses as L
    import torchoptics_amd as ta
    from torchoptics_amd import imaging
    fields = (0.0, 0.6, 1.0)
    cells = imaging.psf_grid_cells((48, 48), (3, 3), 4, fields)
    yy, xx = torch.meshgrid(torch.arange(48, device=DEV), torch.arange(48, device=DEV), indexing="ij")
    img = (((xx // 6 + yy // 6) % 2).float()[None, :, :, None] * torch.tensor([1.0, 0.8, 0.6], device=DEV)).contiguous()
    target = torch.roll(img, 1, dims=2)
    got = {}
    for fused in (False, True):
        lens, specs, leaves = L.build("cooke", DEV)
        tr = ta.RayTracer(mode="circular", n_rays=(16, 16), rel_fields=fields, wavelengths=("C", "d", "F"), default_device=DEV)
        x, y, cx, cy, ok, back = tr.trace_rays(specs, lens)
        psfs = imaging.psf_grid_from_trace(x, y, ok, cells, (9, 9), 0.004, fused=fused)
        out = imaging.svola_convolution(img, 4, psfs, (3, 3), "hann", fused=True)
        ((out - target) ** 2).mean().backward()
        got[fused] = {n: leaves[n].grad.cpu().numpy() for n in ("c", "t")}
    for n in ("c", "t"):
        e = rel_l2(got[True][n], got[False][n])
        print(f"PSF-ROT-ACC rendered 3x3 leaf gradient {n}: fused vs unfused rel-L2 {e:.3e}")
        assert np.isfinite(got[True][n]).all() and np.linalg.norm(got[False][n]) > 0
        assert e <= GATE, (n, e)
