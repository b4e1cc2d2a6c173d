"""imaging.ssim and imaging.psnr without a GPU: the torch path in float64 against tests/ssim_ref.py on every case of
tests/ssim_cases.py (value, map and both gradients); analytic pins; the bounds of ssim_cases held to be SUFFICIENT (the float32
torch path on the CPU stays within them) and SHARP (six deliberately wrong float64 evaluations exceed them on the noise and
chart cases); the tl_ssim_* entry points (declared, bound, exported, refusing bad arguments before any HIP call, the planner's
numbers); the Python layer's errors; psnr against its closed form."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import ssim_cases as sc
from ssim_ref import WRONG, ssim_ref
from torchoptics_amd import _lib, imaging

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
ONE = C.c_void_p(8)                  # a pointer that is never dereferenced on the paths tested here
ENTRIES = ("tl_ssim_work_bytes", "tl_ssim_maps_elems", "tl_ssim_fwd", "tl_ssim_bwd")


# ------------------------------------------------------------------------------------------------- the torch path, float64

@pytest.mark.parametrize("name", list(sc.CASES))
def test_the_torch_path_in_float64_is_the_reference_on_every_case(name):
    got = sc.run(imaging, name, "cpu", torch.float64, False)
    dflt = sc.run(imaging, name, "cpu", torch.float64, None)
    err = sc.errors(name, got["value"], got["g_a"], got["g_b"])
    assert max(err) <= 1e-12, (name, err)
    for key in ("value", "g_a", "g_b"):
        assert np.array_equal(got[key], dflt[key]), "fused=None on the CPU is the same path, bit for bit"
    a, b, _, par = sc.case_inputs(name)
    layout = sc.CASES[name][8]
    value, S = imaging.ssim(sc.as_tensor(a, layout, torch.float64), sc.as_tensor(b, layout, torch.float64), return_map=True, **par)
    assert np.array_equal(value.numpy(), got["value"])
    assert np.abs(S.numpy() - sc.reference(name)["S"]).max() <= 1e-12, name


# ------------------------------------------------------------------------------------------------------------ analytic pins

def test_two_constant_images_give_the_closed_form():
    al, be = sc.CONSTANTS
    got = sc.run(imaging, "constant", "cpu", torch.float64, False)
    al, be = float(np.float32(al)), float(np.float32(be))
    c1 = 0.01 ** 2
    want = (2 * al * be + c1) / (al * al + be * be + c1)
    assert np.abs(got["value"] - want).max() <= 4 * np.finfo(np.float64).eps


def test_equal_images_give_one_and_no_gradient():
    got = sc.run(imaging, "equal", "cpu", torch.float64, False)
    assert np.abs(got["value"] - 1).max() <= 1e-12
    assert np.abs(got["g_a"]).max() <= 1e-12 and np.abs(got["g_b"]).max() <= 1e-12


def test_ssim_is_symmetric_in_its_arguments():
    a, b, seed, par = sc.case_inputs("map_17x33")
    g = torch.from_numpy(seed)
    ta, tb = torch.from_numpy(a).requires_grad_(True), torch.from_numpy(b).requires_grad_(True)
    v1 = imaging.ssim(ta, tb, **par)
    v1.backward(g)
    ua, ub = torch.from_numpy(a).requires_grad_(True), torch.from_numpy(b).requires_grad_(True)
    v2 = imaging.ssim(ub, ua, **par)
    v2.backward(g)
    top = ta.grad.abs().max()
    assert (v1 - v2).abs().max() <= 1e-14
    assert (ta.grad - ua.grad).abs().max() <= 1e-12 * top and (tb.grad - ub.grad).abs().max() <= 1e-12 * top


def test_scaling_images_and_range_by_255_leaves_the_value():
    a, b, _, par = sc.case_inputs("map_32x31")
    v1 = imaging.ssim(torch.from_numpy(a), torch.from_numpy(b), **par)
    v2 = imaging.ssim(torch.from_numpy(a * 255), torch.from_numpy(b * 255), **{**par, "max_value": 255.0})
    assert (v1 - v2).abs().max() <= 1e-12


# ---------------------------------------------------------------------------------------------------------------- the bounds

@pytest.mark.parametrize("name", list(sc.CASES))
def test_the_float32_torch_path_on_the_cpu_stays_within_the_bounds(name):
    got = sc.run(imaging, name, "cpu", torch.float32, False)
    err, bnd = sc.errors(name, got["value"], got["g_a"], got["g_b"]), sc.bounds(name)
    assert all(e <= b for e, b in zip(err, bnd)), (name, err, bnd)


VARIANTS = [("sigma_1.6", dict(filter_sigma=1.6)), ("k2_0.02", dict(k2=0.02))] + [(w, dict(wrong=w)) for w in WRONG]


@pytest.mark.parametrize("name", sc.SHARP)
def test_a_wrong_float64_evaluation_exceeds_the_bounds(name):
    a, b, seed, par = sc.case_inputs(name)
    bnd = sc.bounds(name)
    for tag, kw in VARIANTS:
        r = ssim_ref(a, b, seed, **par, **kw)
        err = sc.errors(name, r["value"], r["g_a"], r["g_b"])
        assert all(e > bd for e, bd in zip(err, bnd)), (name, tag, err, bnd)


# -------------------------------------------------------------------------------------------------------------- the C ABI

def test_entry_points_are_declared_bound_and_exported_and_the_abi_version_stays():
    hdr = open(os.path.join(ROOT, "include", "tl_trace.h")).read()
    dll = _lib.lib()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTS and hasattr(dll, name), name
    assert dll.tl_version() == _lib.TL_ABI_VERSION == 15
    body = re.search(r"typedef struct tl_ssim_geom \{(.*?)\} tl_ssim_geom;", hdr, re.S).group(1)
    members = re.findall(r"(\w+)(?:\[\d+\])?\s*[;,]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert members == [n for n, _ in _lib.tl_ssim_geom._fields_], members


def _geom(**over):
    par = dict(device=0, B=2, H=43, W=41, C=3, K=11, C1=1e-4, C2=9e-4, flags=3)
    par.update(over)
    g = _lib.tl_ssim_geom(**par)
    g.window[:11] = [1.0 / 11] * 11
    for s in (g.a_stride, g.b_stride, g.g_stride):
        s[:] = (par["H"] * par["W"] * par["C"], par["W"] * par["C"], par["C"], 1)
    return g


def test_bad_arguments_are_refused_before_any_device_call():
    dll = _lib.lib()
    big = 1 << 20

    def fwd(g, a=ONE, b=ONE, value=ONE, maps=(ONE,) * 5, work=ONE, nbytes=big):
        return dll.tl_ssim_fwd(C.byref(g) if g is not None else None, a, b, value, *maps, work, nbytes, None)

    def bwd(g, p=ONE, q=ONE, dm=ONE, ds=ONE, dc=ONE, gv=ONE, gp=ONE):
        return dll.tl_ssim_bwd(C.byref(g) if g is not None else None, p, q, dm, ds, dc, gv, gp, None)

    def refused(rc, *words):
        msg = dll.tl_last_error().decode()
        assert rc == EINVAL and all(w in msg for w in words), (rc, msg, words)

    ok = _geom()
    for call, fn in ((fwd, "tl_ssim_fwd"), (bwd, "tl_ssim_bwd")):
        refused(call(None), fn, "g is NULL")
        for size in ("B", "H", "W", "C"):
            refused(call(_geom(**{size: 0})), fn, "B, H, W, C")
        for K in (2, 1, 4, 10, 13):
            refused(call(_geom(K=K)), fn, "K must be odd")
        refused(call(_geom(H=10)), fn, "H and W must be >= K")
        refused(call(_geom(W=10)), fn, "H and W must be >= K")
        refused(call(_geom(H=(1 << 20) + 1)), fn, "2^20")
        refused(call(_geom(W=(1 << 20) + 1)), fn, "2^20")
        refused(call(_geom(H=1 << 20, W=1 << 20)), fn, "tiles")
        refused(call(_geom(flags=4)), fn, "flags")
    for k, arg in enumerate(("a", "b", "value")):
        refused(fwd(ok, **{arg: None}), "tl_ssim_fwd", f"{arg} is NULL")
    for k, arg in enumerate(("dm_a", "ds_a", "dm_b", "ds_b", "dc")):
        refused(fwd(ok, maps=tuple(None if j == k else ONE for j in range(5))), "tl_ssim_fwd", f"{arg} is NULL")
    refused(fwd(_geom(flags=1), maps=(ONE, ONE, None, None, None)), "tl_ssim_fwd", "dc is NULL")
    refused(fwd(ok, work=None), "tl_ssim_fwd", "work is NULL")
    refused(fwd(ok, work=C.c_void_p(12)), "tl_ssim_fwd", "aligned to 8")
    refused(fwd(ok, nbytes=dll.tl_ssim_work_bytes(C.byref(ok)) - 1), "tl_ssim_fwd", "work_bytes")
    for arg in ("p", "q", "dm", "ds", "dc"):
        refused(bwd(ok, **{arg: None}), "tl_ssim_bwd", f"{arg} is NULL")
    refused(bwd(ok, gv=None), "tl_ssim_bwd", "g_value is NULL")
    refused(bwd(ok, gp=None), "tl_ssim_bwd", "g_p is NULL")
    for bad in (_geom(K=13), _geom(H=5), _geom(B=0), _geom(flags=8)):
        assert dll.tl_ssim_work_bytes(C.byref(bad)) == 0 and dll.tl_ssim_maps_elems(C.byref(bad)) == 0
    assert dll.tl_ssim_work_bytes(None) == 0 and dll.tl_ssim_maps_elems(None) == 0


@pytest.mark.parametrize("name", list(sc.CASES))
def test_the_planner_gives_the_restated_numbers(name):
    B, H, W, Cc, K = sc.CASES[name][:5]
    g = _geom(B=B, H=H, W=W, C=Cc, K=K)
    dll = _lib.lib()
    assert (dll.tl_ssim_work_bytes(C.byref(g)), dll.tl_ssim_maps_elems(C.byref(g))) == sc.planner(name)


# ------------------------------------------------------------------------------------------------------- the Python layer

def test_errors_of_the_python_layer():
    a = torch.rand(1, 20, 20, 3, dtype=torch.float64)
    with pytest.raises(ValueError, match="one shape"):
        imaging.ssim(a, a[:, :19])
    with pytest.raises(ValueError, match=r"\[B, H, W, C\]"):
        imaging.ssim(a[0], a[0])
    for fused in (None, False, True):
        with pytest.raises(ValueError, match="at least filter_size"):
            imaging.ssim(a[:, :10], a[:, :10], fused=fused)
        with pytest.raises(ValueError, match="at least filter_size"):
            imaging.ssim(a[:, :, :10], a[:, :, :10], fused=fused)
    with pytest.raises(ValueError, match="dtype"):
        imaging.ssim(a, a, fused=True)
    with pytest.raises(ValueError, match="device"):
        imaging.ssim(a.float(), a.float(), fused=True)
    with pytest.raises(ValueError, match="return_map"):
        imaging.ssim(a.float(), a.float(), fused=True, return_map=True)
    value, S = imaging.ssim(a, a, filter_size=5, return_map=True)
    assert value.shape == (1,) and S.shape == (1, 16, 16, 3)


def test_the_window_is_normalised_in_float64_and_rounded_once():
    w64 = imaging.ssim_window(11, 1.5)
    i = np.arange(11) - 5.0
    want = np.exp(-i * i / 4.5)
    want /= want.sum()
    assert np.array_equal(w64.numpy(), want)
    assert np.array_equal(imaging.ssim_window(11, 1.5, torch.float32).numpy(), want.astype(np.float32))


def test_psnr_against_its_closed_form():
    rng = np.random.RandomState(3)
    a, b = rng.rand(2, 9, 7, 3), rng.rand(2, 9, 7, 3)
    for L in (1.0, 255.0):
        want = 10 * np.log10(L * L / ((a - b) ** 2 * L * L).reshape(2, -1).mean(axis=1))
        got = imaging.psnr(torch.from_numpy(a * L), torch.from_numpy(b * L), max_value=L)
        assert got.shape == (2,) and np.abs(got.numpy() - want).max() <= 1e-12
    a8 = torch.full((1, 4, 4, 1), 0.5, dtype=torch.float64)
    assert abs(float(imaging.psnr(a8, a8 + 0.1)) - 20.0) <= 1e-12
    with pytest.raises(ValueError):
        imaging.psnr(a8, a8[:, :3])
