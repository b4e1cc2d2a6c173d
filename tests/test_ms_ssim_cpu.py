"""imaging.ms_ssim without a GPU: the torch path in float64 against tests/ms_ssim_ref.py on every case of tests/ms_ssim_cases.py
(value, terms and both gradients); the cases' conditions (every term >= 0.2); the `negative` case's exact zeros; the bounds of
ms_ssim_cases held to be SUFFICIENT (the float32 torch path on the CPU stays within them) and SHARP (each deliberately wrong
float64 evaluation exceeds them on the quantity it affects); the tl_ms_ssim_* entry points (declared, bound, exported, refusing
bad arguments before any HIP call, the planners' numbers); the Python layer's errors."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import ms_ssim_cases as mc
from ms_ssim_ref import WRONG, ms_ssim_ref
from torchoptics_amd import _lib, imaging

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
ONE = C.c_void_p(8)                  # a pointer that is never dereferenced on the paths tested here
ENTRIES = ("tl_ms_ssim_work_bytes", "tl_ms_ssim_keep_elems", "tl_ms_ssim_fwd", "tl_ms_ssim_bwd")


# ------------------------------------------------------------------------------------------------- the torch path, float64

@pytest.mark.parametrize("name", mc.BOUNDED)
def test_the_torch_path_in_float64_is_the_reference_on_every_case(name):
    got = mc.run(imaging, name, "cpu", torch.float64, False)
    dflt = mc.run(imaging, name, "cpu", torch.float64, None)
    err = mc.errors(name, got["value"], got["terms"], got["g_a"], got["g_b"])
    assert max(err) <= 1e-12, (name, err)
    for key in ("value", "terms", "g_a", "g_b"):
        assert np.array_equal(got[key], dflt[key]), "fused=None on the CPU is the same path, bit for bit"
    a, b, _, par = mc.case_inputs(name)
    layout = mc.CASES[name][9]
    plain = imaging.ms_ssim(mc.as_tensor(a, layout, torch.float64), mc.as_tensor(b, layout, torch.float64), **par)
    assert isinstance(plain, torch.Tensor) and np.array_equal(plain.numpy(), got["value"])


@pytest.mark.parametrize("name", mc.BOUNDED)
def test_every_term_of_the_reference_is_at_least_a_fifth(name):
    assert mc.reference(name)["terms"].min() >= mc.MIN_TERM, name


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_a_negative_term_gives_zero_and_exactly_zero_finite_gradients(dtype):
    ref = mc.reference("negative")
    assert ref["terms"].min() < 0, "b = L - a: the contrast-structure factor is negative"
    assert np.all(ref["value"] == 0) and np.all(ref["g_a"] == 0) and np.all(ref["g_b"] == 0)
    got = mc.run(imaging, "negative", "cpu", dtype, False)
    assert np.abs(got["terms"] - ref["terms"]).max() <= (1e-12 if dtype == torch.float64 else 1e-5)
    for key in ("value", "g_a", "g_b"):
        assert np.all(np.isfinite(got[key])) and np.all(got[key] == 0), key


def test_one_negative_channel_leaves_the_gradients_of_the_others():
    a, b, seed, par = mc.case_inputs("odd_every_level")
    b = b.copy()
    b[0, :, :, 1] = 1.0 - a[0, :, :, 1]
    ta, tb = torch.from_numpy(a).requires_grad_(True), torch.from_numpy(b).requires_grad_(True)
    value, v = imaging.ms_ssim(ta, tb, return_terms=True, **par)
    value.backward(torch.from_numpy(seed))
    r = ms_ssim_ref(a, b, seed, **par)
    assert float(v[0, 1].min()) < 0 and torch.isfinite(ta.grad).all()
    assert bool((ta.grad[0, :, :, 1] == 0).all()) and bool((tb.grad[0, :, :, 1] == 0).all())
    assert np.abs(ta.grad.numpy() - r["g_a"]).max() <= 1e-12 * np.abs(r["g_a"]).max()
    assert np.abs(value.detach().numpy() - r["value"]).max() <= 1e-12


def test_one_level_with_weight_one_is_ssim_per_channel():
    a, b, _, par = mc.case_inputs("one_level")
    par = dict(par, power_factors=(1.0,))
    ms = imaging.ms_ssim(torch.from_numpy(a), torch.from_numpy(b), **par)
    ss = imaging.ssim(torch.from_numpy(a), torch.from_numpy(b), max_value=par["max_value"], filter_size=par["filter_size"])
    assert (ms - ss).abs().max() <= 1e-14


# ---------------------------------------------------------------------------------------------------------------- the bounds

@pytest.mark.parametrize("name", mc.BOUNDED)
def test_the_float32_torch_path_on_the_cpu_stays_within_the_bounds(name):
    got = mc.run(imaging, name, "cpu", torch.float32, False)
    err, bnd = mc.errors(name, got["value"], got["terms"], got["g_a"], got["g_b"]), mc.bounds(name)
    assert all(e <= b for e, b in zip(err, bnd)), (name, err, bnd)


# what each mistake moves: the value (and with it everything) or only the gradients
AFFECTS = {"floor_halving": (0, 1, 2, 3), "zero_padding": (0, 1, 2, 3), "ssim_at_every_level": (0, 1, 2, 3),
           "weights_reversed": (0, 2, 3), "product_of_channel_means": (0, 2, 3), "unpool_without_edge_doubling": (2, 3)}


@pytest.mark.parametrize("wrong", WRONG)
def test_a_wrong_float64_evaluation_exceeds_the_bounds_on_a_sharp_case(wrong):
    caught = []
    for name in mc.SHARP:
        a, b, seed, par = mc.case_inputs(name)
        r = ms_ssim_ref(a, b, seed, **par, wrong=wrong)
        err, bnd = mc.errors(name, r["value"], r["terms"], r["g_a"], r["g_b"]), mc.bounds(name)
        caught.append(all(err[k] > bnd[k] for k in AFFECTS[wrong]))
    assert any(caught), (wrong, caught)


def test_the_value_floor_is_the_stated_formula():
    name = "odd_every_level"
    ref, p = mc.reference(name), np.asarray(mc.power(3))
    floor = (4 * np.max(np.sum(p / ref["terms"], axis=2)) + 6) * mc.EPS32
    assert mc.bounds(name)[0] == max(4 * mc.MEASURED[name][0], floor)


# -------------------------------------------------------------------------------------------------------------- the C ABI

def test_entry_points_are_declared_bound_and_exported_and_the_abi_version_stays():
    hdr = open(os.path.join(ROOT, "include", "tl_trace.h")).read()
    dll = _lib.lib()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTS and hasattr(dll, name), name
    assert dll.tl_version() == _lib.TL_ABI_VERSION == 15
    body = re.search(r"typedef struct tl_ms_ssim_geom \{(.*?)\} tl_ms_ssim_geom;", hdr, re.S).group(1)
    members = re.findall(r"(\w+)(?:\[\d+\])?\s*[;,]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert members == [n for n, _ in _lib.tl_ms_ssim_geom._fields_], members


def _geom(**over):
    par = dict(device=0, B=2, H=43, W=41, C=3, K=5, C1=1e-4, C2=9e-4, levels=3, flags=3)
    par.update(over)
    g = _lib.tl_ms_ssim_geom(**par)
    g.window[:11] = [1.0 / 11] * 11
    g.power[:8] = [0.125] * 8
    for s in (g.a_stride, g.b_stride, g.g_stride):
        s[:] = (par["H"] * par["W"] * par["C"], par["W"] * par["C"], par["C"], 1)
    return g


def test_bad_arguments_are_refused_before_any_device_call():
    dll = _lib.lib()
    big = 1 << 30

    def fwd(g, a=ONE, b=ONE, value=ONE, terms=ONE, keep=ONE, n_keep=big, work=ONE, nbytes=big):
        return dll.tl_ms_ssim_fwd(C.byref(g) if g is not None else None, a, b, value, terms, keep, n_keep, work, nbytes, None)

    def bwd(g, p=ONE, q=ONE, keep=ONE, n_keep=big, gv=ONE, gp=ONE, which=0, work=ONE, nbytes=big):
        return dll.tl_ms_ssim_bwd(C.byref(g) if g is not None else None, p, q, keep, n_keep, gv, gp, which, work, nbytes, None)

    def refused(rc, *words):
        msg = dll.tl_last_error().decode()
        assert rc == EINVAL and all(w in msg for w in words), (rc, msg, words)

    ok = _geom()
    for call, fn in ((fwd, "tl_ms_ssim_fwd"), (bwd, "tl_ms_ssim_bwd")):
        refused(call(None), fn, "g is NULL")
        for size in ("B", "H", "W", "C"):
            refused(call(_geom(**{size: 0})), fn, "B, H, W, C")
        for K in (2, 1, 4, 10, 13):
            refused(call(_geom(K=K)), fn, "K must be odd")
        for levels in (0, -1, 9):
            refused(call(_geom(levels=levels)), fn, "levels must be 1 .. 8")
        refused(call(_geom(H=4)), fn, "level 0 is 4 x 41")
        refused(call(_geom(levels=5)), fn, "level 4 is 3 x 3", "K = 5")          # 43 x 41 -> 22 x 21 -> 11 x 11 -> 6 x 6 -> 3 x 3
        refused(call(_geom(W=16)), fn, "level 2 is 11 x 4")                      # 43 x 16 -> 22 x 8 -> 11 x 4
        refused(call(_geom(H=(1 << 20) + 1)), fn, "2^20")
        refused(call(_geom(H=1 << 15, W=1 << 15)), fn, "2^31")                   # 2^21 tiles, 3 x 2^30 elements
        refused(call(_geom(flags=4)), fn, "flags")
        for arg in ("keep", "work"):
            refused(call(ok, **{arg: None}), fn, f"{arg} is NULL")
            refused(call(ok, **{arg: C.c_void_p(12)}), fn, f"{arg} must be aligned to 8")
        refused(call(ok, n_keep=dll.tl_ms_ssim_keep_elems(C.byref(ok)) - 1), fn, "keep_elems")
        refused(call(ok, nbytes=dll.tl_ms_ssim_work_bytes(C.byref(ok)) - 1), fn, "work_bytes")
    for arg in ("a", "b", "value", "terms"):
        refused(fwd(ok, **{arg: None}), "tl_ms_ssim_fwd", f"{arg} is NULL")
    for arg in ("p", "q"):
        refused(bwd(ok, **{arg: None}), "tl_ms_ssim_bwd", f"{arg} is NULL")
    refused(bwd(ok, gv=None), "tl_ms_ssim_bwd", "g_value is NULL")
    refused(bwd(ok, gp=None), "tl_ms_ssim_bwd", "g_p is NULL")
    refused(bwd(ok, which=2), "tl_ms_ssim_bwd", "which")
    refused(bwd(_geom(flags=1), which=1), "tl_ms_ssim_bwd", "which")
    for bad in (_geom(K=13), _geom(H=4), _geom(B=0), _geom(flags=8), _geom(levels=9), _geom(levels=5)):
        assert dll.tl_ms_ssim_work_bytes(C.byref(bad)) == 0 and dll.tl_ms_ssim_keep_elems(C.byref(bad)) == 0
    assert dll.tl_ms_ssim_work_bytes(None) == 0 and dll.tl_ms_ssim_keep_elems(None) == 0


@pytest.mark.parametrize("name", list(mc.CASES))
def test_the_planners_give_the_restated_numbers(name):
    B, H, W, Cc, K, M = mc.CASES[name][:6]
    dll = _lib.lib()
    for flags, n_maps in ((0, 0), (1, 3), (2, 3), (3, 4)):
        g = _geom(B=B, H=H, W=W, C=Cc, K=K, levels=M, flags=flags)
        assert (dll.tl_ms_ssim_work_bytes(C.byref(g)), dll.tl_ms_ssim_keep_elems(C.byref(g))) == mc.planner(name, n_maps)


# ------------------------------------------------------------------------------------------------------- the Python layer

def test_errors_of_the_python_layer():
    a = torch.rand(1, 40, 40, 3, dtype=torch.float64)
    with pytest.raises(ValueError, match="one shape"):
        imaging.ms_ssim(a, a[:, :39])
    with pytest.raises(ValueError, match=r"\[B, H, W, C\]"):
        imaging.ms_ssim(a[0], a[0])
    for fused in (None, False, True):
        with pytest.raises(ValueError, match="level 2 is 10 x 10"):                     # 40 -> 20 -> 10 < 11
            imaging.ms_ssim(a, a, fused=fused)
        with pytest.raises(ValueError, match="level 0 is 40 x 4"):
            imaging.ms_ssim(a[:, :, :4], a[:, :, :4], filter_size=5, power_factors=(1.0,), fused=fused)
        with pytest.raises(ValueError, match="levels"):
            imaging.ms_ssim(a, a, filter_size=3, power_factors=(0.1,) * 9, fused=fused)
        with pytest.raises(ValueError, match="levels"):
            imaging.ms_ssim(a, a, filter_size=3, power_factors=(), fused=fused)
    with pytest.raises(ValueError, match="dtype"):
        imaging.ms_ssim(a, a, filter_size=5, power_factors=(0.5, 0.5), fused=True)
    with pytest.raises(ValueError, match="device"):
        imaging.ms_ssim(a.float(), a.float(), filter_size=5, power_factors=(0.5, 0.5), fused=True)
    value, v = imaging.ms_ssim(a, a, filter_size=5, power_factors=(0.5, 0.5), return_terms=True)
    assert value.shape == (1,) and v.shape == (1, 3, 2) and not v.requires_grad
    assert imaging.ms_ssim(a, a, filter_size=4, power_factors=(0.5, 0.5)).shape == (1,), "an even window is the torch path's"


def test_the_defaults_are_tf_image_ssim_multiscales():
    assert imaging.MS_SSIM_POWER_FACTORS == (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
    a, b, _, par = mc.case_inputs("tf_minimum")
    got = imaging.ms_ssim(torch.from_numpy(a), torch.from_numpy(b))
    assert np.abs(got.numpy() - mc.reference("tf_minimum")["value"]).max() <= 1e-12
