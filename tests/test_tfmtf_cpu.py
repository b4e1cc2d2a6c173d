"""The through-focus MTF (metrics.through_focus_mtf / otf_sums_through_focus / mtf_best_focus; tl_tfmtf_sums / tl_tfmtf_seed), what
can be checked without a GPU: the float64 torch path (recurrence included) against the long-double definition of
tests/tfmtf_ref.py, which evaluates every plane directly, on the cases of tests/tfmtf_cases.py; that the bounds the GPU tests use
tell float64 from float32; the finish; gradients; the chunking rule; mtf_best_focus; the refusals of the Python functions and of
the C ABI with its workspace plan; analytic pins."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

import tfmtf_cases as TC
import tfmtf_ref as R
from conftest import ROOT

from torchoptics_amd import _lib, metrics, ops
from torchoptics_amd.metrics import mtf_best_focus, otf_sums_through_focus, through_focus_mtf      # noqa: F401 (the feature: every
from torchoptics_amd.ops import TFMTFSumsFunction                                                 # noqa: F401  test here needs it)

EINVAL, EWORKSPACE = -1, -3                 # TL_EINVAL, TL_EWORKSPACE (include/tl_trace.h)
ONE = C.c_void_p(8)                         # any non-NULL pointer: never dereferenced on the paths taken here
SMALL = tuple(n for n in TC.CASES if not n.startswith("many-rows"))


@functools.lru_cache(maxsize=None)
def _ref(name):
    """The case's rays and the long-double sums about given_centre, computed once and left unchanged."""
    r = TC.rays(name)
    nu = R.vectors(TC.frequencies_of(name), TC.DIRECTIONS)
    return r, nu, R.sums(*(r[k] for k in TC.KEYS), r["ok"], TC.given_centre(name), *nu, TC.planes_of(name))


def _torch(r, dtype=torch.float64, grad=False):
    with np.errstate(invalid="ignore", over="ignore"):
        return [torch.from_numpy(r[k].astype(np.float64)).to(dtype).requires_grad_(grad) for k in TC.KEYS] + [torch.from_numpy(r["ok"])]


def _tf(r, *args, **kw):
    return metrics.through_focus_mtf(*_torch(r), *args, fused=False, **kw)


@pytest.mark.parametrize("name", TC.CASES)
def test_torch_path_against_the_long_double_definition(name):
    r, nu, ref = _ref(name)
    planes = TC.planes_of(name)
    sums = metrics.otf_sums_through_focus(*_torch(r), torch.from_numpy(TC.given_centre(name)), tuple(nu[0]), tuple(nu[1]), planes, fused=False)
    assert sums.dtype == torch.float64 and tuple(sums.shape) == ref["sums"].shape
    worst = float((np.abs(sums.numpy() - ref["sums"]) / ref["bound"].clip(1e-300)).max())
    print(f"TFMTF-ACC cpu torch path   case {name:14s} sums err/bound {worst:.3f}")
    assert np.isfinite(sums.numpy()).all() and worst <= 1
    zero = [j for j in range(len(nu[0])) if nu[0][j] == 0 and nu[1][j] == 0]
    still = sums.numpy()[:, :, :, zero]                                                            # nu = 0: C = n, S = 0 at every plane
    assert np.all(still[..., 0] == ref["n"][..., None, None]) and np.all(still[..., 1] == 0)
    assert np.all(sums.numpy()[ref["n"] == 0] == 0)
    # pooling, weights, centre variants and the zero rules against the reference finish
    K, Z, W = len(TC.frequencies_of(name)), planes[2], r["x"].shape[3]
    weights = tuple(0.5 + 0.25 * w for w in range(W))
    given = TC.given_centre(name)[:, :, :1]
    for common, centre in (((), "row"), ((), "field"), ((), "given"), (("wavelength",), "field"), (("wavelength",), "given")):
        for a in (None, weights):
            c = torch.from_numpy(given) if centre == "given" else centre
            out = _tf(r, TC.frequencies_of(name), planes, common=common, centre=c, weights=a)
            o = np.broadcast_to(given, given.shape[:2] + (W, 2)) if centre == "given" else R.centre_of(*(r[k] for k in TC.KEYS), r["ok"], centre)
            want = R.sums(*(r[k] for k in TC.KEYS), r["ok"], o, *nu, planes)
            n, mtf = R.finish(want["sums_ld"], want["n"], a, bool(common))
            assert out.mtf.dtype == out.n.dtype == out.centre.dtype == out.shifts.dtype == torch.float64
            assert tuple(out.mtf.shape) == mtf.shape[:-2] + (Z, 2, K) and np.array_equal(out.centre.numpy(), o)
            assert np.array_equal(out.shifts.numpy(), R.shifts(planes))
            assert np.array_equal(out.n.numpy(), n) or np.allclose(out.n.numpy(), n, rtol=1e-15, atol=0)
            # a modulus of sums inside their bounds, over n: the bound of C and S together, and three roundings of a value <= 1
            slack = (want["bound"] * (1.0 if a is None else max(a))).sum(axis=-1)
            slack = (slack.sum(axis=2) if common else slack) / np.maximum(n, 1e-300)[..., None, None] + 8 * R.U
            got = np.moveaxis(out.mtf.numpy(), -3, -1).reshape(mtf.shape)                     # [.., Z, D, K] -> [.., J, Z]
            assert np.all(np.abs(got - mtf) <= slack), (name, common, centre, a)
            assert np.all(out.mtf.numpy()[n == 0] == 0)                                        # an empty set: exactly 0
            if TC.frequencies_of(name)[0] == 0:
                assert np.all(out.mtf.numpy()[..., 0][n > 0] == 1)                             # nu = 0: exactly 1 at every plane


def test_the_cases_reach_what_they_claim():
    """The planes bracket the foci: per row and direction the curve at 25 cycles / mm peaks inside the range, well above its ends."""
    for name in ("block-edge", "multi-partial", "lens-batch", "layout-tracer"):
        r, nu, ref = _ref(name)
        n, mtf = R.finish(ref["sums_ld"], ref["n"], None, False)
        mtf = mtf.reshape(mtf.shape[:-2] + (2, 4, 16))[n > 1][:, :, 2]                          # [rows, D, Z] at 25 cycles / mm
        top = mtf.argmax(axis=-1)
        assert np.all((top > 0) & (top < 15)) and np.all(mtf.max(axis=-1) > 0.7), (name, top)
        assert np.all(mtf.max(axis=-1) > mtf[..., 0] + 0.2) and np.all(mtf.max(axis=-1) > mtf[..., -1] + 0.1), name
    assert len(TC.CASES) == 14 and R.SEED_C == 36 and R.MAX_J == ops.TFMTF_MAX_J == 16 and R.MAX_Z == ops.TFMTF_MAX_Z == 16
    assert all(float(v).hex() == float(w).hex() for v, w in zip(R.shifts(TC.PLANES), -0.125 + np.arange(16) / 32))


def test_the_bound_tells_fp64_from_fp32():
    """Two float64 summation orders of the float64 recurrence stay inside the bound on every case and plane, z = 15 included; a
    slope formed in fp32, a phase formed in fp32 and the recurrence run in fp32 do not."""
    worst, least = 0.0, {}
    for name in SMALL:
        r, nu, ref = _ref(name)
        args = (*(r[k] for k in TC.KEYS), r["ok"], TC.given_centre(name), *nu, TC.PLANES)
        hot = [j for j in range(len(nu[0])) if nu[0][j] != 0 or nu[1][j] != 0]
        for order in ("reverse", "blocks"):
            ratio = np.abs(R.recurrence(*args, order) - ref["sums"]) / ref["bound"].clip(1e-300)
            worst = max(worst, float(ratio.max()))
            assert ratio.max() <= 1 and ratio[..., 15, :].max() <= 1, (name, order)
        for what in ("slope", "phase", "rot"):
            s32 = R.recurrence(*args, "forward", **{what: np.float32})
            ratio = (np.abs(s32 - ref["sums"]) / ref["bound"].clip(1e-300))[..., hot, :, :].max()
            assert ratio > 1, (name, what, ratio)
            least[what] = min(least.get(what, np.inf), float(ratio))
            assert np.allclose(s32, ref["sums"], atol=2e-3 * r["x"].shape[2])                      # (the same quantity, only coarser)
    print(f"TFMTF-ACC cpu float64 recurrence, two orders: err/bound <= {worst:.3f}; fp32 slope >= {least['slope']:.3g} bounds, "
          f"fp32 phase >= {least['phase']:.3g}, fp32 recurrence >= {least['rot']:.3g}")


# ---------------------------------------------------------------------------------------------------------------- gradients
def _small_fan():
    r = {k: a[:, :2, :7, :2].copy() for k, a in TC.rays("sub-wave").items()}
    r = {k: np.concatenate([a, a[:, ::-1]], axis=0) for k, a in r.items()}                     # [2, 2, 7, 2]
    r["x"][1] += np.float32(0.01)
    r["ok"][0, 0, 3, 0] = False
    return r


def test_gradcheck_of_the_float64_path():
    r = _small_fan()
    ok = torch.from_numpy(r["ok"])
    leaves = tuple(torch.from_numpy(r[k].astype(np.float64)).requires_grad_(True) for k in TC.KEYS)
    nu, dirs, weights, planes = (4.0, 11.0), ("tangential", "sagittal", 30.0), (0.7, 1.3), (-0.05, 0.04, 3)
    nx, ny = R.vectors(nu, dirs)
    origin = torch.from_numpy(R.centre_of(*(r[k] for k in TC.KEYS), r["ok"], "field"))
    assert torch.autograd.gradcheck(lambda *q: metrics.otf_sums_through_focus(*q, ok, origin, tuple(nx), tuple(ny), planes, fused=False), leaves)
    for common, centre, a in (((), "row", None), (("wavelength",), "field", weights)):
        fn = lambda *q: metrics.through_focus_mtf(*q, ok, nu, planes, dirs, common=common, centre=centre, weights=a, fused=False).mtf    # noqa: E731
        assert torch.autograd.gradcheck(fn, leaves), (common, centre, a)


def test_the_seed_reference_is_the_gradient_of_the_sums():
    for name in ("sub-wave", "dead-row", "poisoned", "lens-batch"):
        r, nu, ref = _ref(name)
        g = TC.seeds(name, len(nu[0]), TC.PLANES[2])
        want = R.seeds(ref, g)
        *leaves, ok = _torch(r, grad=True)
        sums = metrics.otf_sums_through_focus(*leaves, ok, torch.from_numpy(TC.given_centre(name)), tuple(nu[0]), tuple(nu[1]), TC.PLANES, fused=False)
        (sums * torch.from_numpy(g)).sum().backward()
        live = ref["terms"].live
        for t, k in zip(leaves, ("gx", "gy", "gcx", "gcy")):
            assert np.allclose(t.grad.numpy(), want[k], rtol=1e-10, atol=1e-10 * np.abs(want[k]).max()), (name, k)
            assert np.all(t.grad.numpy()[~live] == 0) and np.isfinite(t.grad.numpy()).all()
            assert np.all(want[k + "_bound"][live] < 1e-6 * np.abs(want[k]).max() + 2.0 ** -23 * np.abs(want[k][live]))


# ----------------------------------------------------------------------------------------------------------------- chunking
def test_planes_go_in_sixteens_and_vectors_in_sixteens():
    """Chunk q of the planes starts at first + (16 q) step, formed on the host, and restarts the recurrence: 17 and 33 planes equal
    the concatenation of their chunks' own calls, and 17 vectors that of 16 and 1."""
    r = TC.rays("sub-wave")
    args = _torch(r)
    o = torch.from_numpy(TC.given_centre("sub-wave"))
    nu = R.vectors(tuple(3.0 * k for k in range(17)), (20.0,))
    first, step = -0.11, 0.013
    for Z in (17, 33):
        whole = metrics.otf_sums_through_focus(*args, o, tuple(nu[0][:3]), tuple(nu[1][:3]), (first, step, Z), fused=False)
        parts = [metrics.otf_sums_through_focus(*args, o, tuple(nu[0][:3]), tuple(nu[1][:3]), (first + z0 * step, step, min(16, Z - z0)), fused=False)
                 for z0 in range(0, Z, 16)]
        assert tuple(whole.shape) == (1, 2, 3, 3, Z, 2) and torch.equal(whole, torch.cat(parts, dim=4))
        assert metrics.plane_shifts((first, step, Z)) == tuple(R.shifts((first, step, Z)))
        assert metrics.plane_shifts((first, step, Z))[16] == first + 16 * step
    whole = metrics.otf_sums_through_focus(*args, o, tuple(nu[0]), tuple(nu[1]), (first, step, 3), fused=False)
    parts = [metrics.otf_sums_through_focus(*args, o, tuple(nu[0][j]), tuple(nu[1][j]), (first, step, 3), fused=False) for j in (slice(0, 16), slice(16, 17))]
    assert tuple(whole.shape) == (1, 2, 3, 17, 3, 2) and torch.equal(whole, torch.cat(parts, dim=3))
    ref = R.sums(*(r[k] for k in TC.KEYS), r["ok"], TC.given_centre("sub-wave"), nu[0][:3], nu[1][:3], (first, step, 33))
    whole = metrics.otf_sums_through_focus(*args, o, tuple(nu[0][:3]), tuple(nu[1][:3]), (first, step, 33), fused=False)
    assert np.all(np.abs(whole.numpy() - ref["sums"]) <= ref["bound"])


# ----------------------------------------------------------------------------------------------------------- mtf_best_focus
def test_mtf_best_focus_on_a_sampled_parabola_and_on_edge_maxima():
    d = torch.tensor(R.shifts((-0.125, 2.0 ** -5, 9)))
    peak = torch.tensor([[0.03, -0.07], [0.0, 0.101]], dtype=torch.float64)                       # [D, K], all inside the range
    top = torch.tensor([[0.9, 0.5], [0.75, 0.6]], dtype=torch.float64)
    curve = (top - 40.0 * (d[:, None, None] - peak) ** 2).requires_grad_(True)                    # [Z, D, K]
    shift, value, interior = metrics.mtf_best_focus(curve[None, None], d)
    assert tuple(shift.shape) == (1, 1, 2, 2) and interior.dtype == torch.bool and interior.all()
    assert torch.allclose(shift[0, 0], peak, rtol=0, atol=1e-13) and torch.allclose(value[0, 0], top, rtol=0, atol=1e-13)
    value.sum().backward()                                                                         # the arg-max is detached
    assert torch.isfinite(curve.grad).all() and (curve.grad != 0).any(dim=0).all() and ((curve.grad != 0).sum(dim=0) <= 3).all()
    rising, falling = d[:, None, None].expand(9, 1, 1).clone(), -d[:, None, None].expand(9, 1, 1).clone()
    for c, at in ((rising, 8), (falling, 0)):
        shift, value, interior = metrics.mtf_best_focus(c, d)
        assert not interior.any() and shift.item() == d[at].item() and value.item() == c[at].item()
    flat = torch.ones(9, 1, 1, dtype=torch.float64)
    shift, value, interior = metrics.mtf_best_focus(flat, d)
    assert shift.item() == d[0].item() and value.item() == 1 and not interior.any()
    step = torch.tensor([0.1, 0.5, 0.5, 0.1], dtype=torch.float64).reshape(4, 1, 1)                # two equal maxima: the first one counts,
    shift, value, interior = metrics.mtf_best_focus(step, d[:4])                                   # and the vertex lies midway
    assert interior.all() and abs(shift.item() - 0.5 * (d[1] + d[2]).item()) <= 1e-15 and abs(value.item() - 0.55) <= 1e-15
    f32 = metrics.mtf_best_focus(curve.detach().float(), d)
    assert f32[0].dtype == f32[1].dtype == torch.float32
    one = metrics.mtf_best_focus(curve.detach()[:1], d[:1])
    assert not one[2].any() and torch.equal(one[1], curve.detach()[0])
    with pytest.raises(ValueError):
        metrics.mtf_best_focus(curve, d[:4])


# ------------------------------------------------------------------------------------------------------------ analytic pins
def _pin_tol(r, out, frequencies, planes, directions=TC.DIRECTIONS):
    """The bound of the modulus of pooled sums inside their bounds over n, [.., Z, D, K] like out.mtf, for fp64 outputs."""
    ref = R.sums(*(r[k] for k in TC.KEYS), r["ok"], out.centre.double().cpu().numpy(), *R.vectors(frequencies, directions), planes)
    n = np.maximum(ref["n"].sum(axis=2), 1)[..., None, None]
    tol = ref["bound"].sum(axis=(2, -1)) / n + 8 * R.U                                            # [B,F,J,Z]
    D, K = len(directions), len(frequencies)
    return np.moveaxis(tol.reshape(tol.shape[:2] + (D, K, planes[2])), -1, -3)


def check_pins(mtf_of, tol_of):
    """The analytic pins for either path: mtf_of(rays, frequencies, planes, directions) -> (mtf [.., Z, D, K] float64 numpy, out)."""
    nu = (0.0, 10.0, 25.0, 50.0)
    r, a, zeta = TC.two_rays()
    got, out = mtf_of(r, nu, TC.PLANES, TC.DIRECTIONS)
    d = R.shifts(TC.PLANES)
    want = np.abs(np.cos(2 * np.pi * np.asarray(nu)[None, :] * a * (d[:, None] - zeta)))           # [Z, K]
    tol = tol_of(r, out, nu, TC.PLANES)
    assert abs(zeta - 0.0625) < 1e-6 and abs(a - 0.05) < 1e-6
    # (1e-13: the float64 rounding of the closed form itself, a phase of a few radians)
    assert np.all(np.abs(got[0, 0, :, 0] - want) <= tol[0, 0, :, 0] + 1e-13), np.abs(got[0, 0, :, 0] - want).max()
    assert np.all(got[0, 0, :, 1] == 1)                             # sagittal: cx = 0 and x IS the origin, a = b = 0: exactly 1
    one = {k: v[:, :, :1] for k, v in r.items()}
    dirs = ("tangential", "sagittal", 30.0)
    got, out = mtf_of(one, nu, TC.PLANES, dirs)                     # a single ray: 1 everywhere, to the rounding of c^2 + s^2
    assert np.all(np.abs(got - 1) <= tol_of(one, out, nu, TC.PLANES, dirs)) and np.all(got[..., 0] == 1)
    fan = TC.point_fan()
    got, out = mtf_of(fan, nu, TC.PLANES, TC.DIRECTIONS)
    z = int(np.flatnonzero(d == 0.09375)[0])
    # every ray passes the point within the float32 rounding of x, y (2^-24 of 0.5 and 4): a phase of <= 2 pi 50 2^-22 at most
    assert np.all(1 - got[0, 0, z] <= 0.5 * (2 * np.pi * 50 * 2.0 ** -22) ** 2 + tol_of(fan, out, nu, TC.PLANES)[0, 0, z])
    assert np.all(got[0, 0, z] >= got[0, 0].max(axis=0) - 1e-6) and got[0, 0, 0, 0, 3] < 0.5


def test_two_rays_one_ray_and_a_fan_through_one_point():
    def mtf_of(r, frequencies, planes, directions):
        out = _tf(r, frequencies, planes, directions)
        return out.mtf.numpy(), out
    check_pins(mtf_of, _pin_tol)


def test_dead_rows_and_dead_rays_get_exact_zeros():
    rays = TC.rays("dead-row")
    *leaves, ok = _torch(rays, grad=True)
    out = metrics.through_focus_mtf(*leaves, ok, TC.FREQUENCIES, TC.PLANES, common=(), fused=False)
    assert out.n[0, 0, 0] == 0 and (out.mtf[0, 0, 0] == 0).all() and (out.mtf[..., 0][out.n > 0] == 1).all()
    out.mtf[0, 0, 0].sum().backward()
    assert all((t.grad == 0).all() for t in leaves)
    rays = TC.rays("poisoned")
    *leaves, ok = _torch(rays, grad=True)
    metrics.through_focus_mtf(*leaves, ok, TC.FREQUENCIES, TC.PLANES, common=(), fused=False).mtf.sum().backward()
    live = _ref("poisoned")[2]["terms"].live
    assert all(torch.isfinite(t.grad).all() and (t.grad.numpy()[~live] == 0).all() and (t.grad.numpy()[live] != 0).any() for t in leaves)


# ----------------------------------------------------------------------------------------------------------------- refusals
def test_python_refusals_and_the_dispatch():
    r = TC.rays("sub-wave")
    f32, f64 = _torch(r, torch.float32), _torch(r)
    per_w = torch.zeros(1, 2, 3, 2, dtype=torch.float64)
    ok_planes = (-0.1, 0.05, 4)
    for bad in (dict(common=("field",)), dict(common=("pupil",)), dict(centre="row"), dict(centre=per_w), dict(centre="lens"),
                dict(frequencies=(-1.0,)), dict(frequencies=(float("nan"),)), dict(frequencies=()), dict(directions=("radial",)),
                dict(directions=()), dict(weights=(1.0, 1.0)), dict(weights=(0.0, 0.0, 0.0)), dict(planes=(0.0, 0.1, 0)),
                dict(planes=(0.0, 0.1, 2.0)), dict(planes=(float("nan"), 0.1, 2)), dict(planes=(0.0, float("inf"), 2)),
                dict(planes=(0.0, 0.1)), dict(planes=(0.0, 0.1, True)), dict(planes=None), dict(planes=(0.1, 0.0, 2))):
        kw = dict(dict(frequencies=(10.0, 20.0), planes=ok_planes), **bad)
        with pytest.raises(ValueError):
            metrics.through_focus_mtf(*f64, fused=False, **kw)
    with pytest.raises(ValueError):
        metrics.through_focus_mtf(*(t[0] for t in f64), (10.0,), ok_planes, fused=False)           # not [B, F, P, W]
    with pytest.raises(ValueError):
        metrics.otf_sums_through_focus(*f64, per_w, (1.0, 2.0), (1.0,), ok_planes, fused=False)
    with pytest.raises(ValueError):
        metrics.otf_sums_through_focus(*f64, per_w, (1.0,), (1.0,), (0.0, 0.1, 0), fused=False)
    metrics.through_focus_mtf(*f64, (10.0,), ok_planes, common=(), centre=per_w, fused=False)     # (without pooling it may)
    for args in (f32, f64):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            metrics.through_focus_mtf(*args, TC.FREQUENCIES, ok_planes, fused=True)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            metrics.otf_sums_through_focus(*args, per_w, (1.0,), (0.0,), ok_planes, fused=True)
    a, b = metrics.through_focus_mtf(*f32, TC.FREQUENCIES, ok_planes), metrics.through_focus_mtf(*f32, TC.FREQUENCIES, ok_planes, fused=False)
    assert all(torch.equal(p, q) for p, q in zip(a, b)) and a.mtf.dtype == a.n.dtype == a.centre.dtype == torch.float32
    assert a.shifts.dtype == torch.float64 and tuple(a.shifts.shape) == (4,)
    assert tuple(a.mtf.shape) == (1, 2, 4, 2, 4) and tuple(a.n.shape) == (1, 2) and tuple(a.centre.shape) == (1, 2, 3, 2)
    assert tuple(metrics.through_focus_mtf(*f32, (1.0, 1.0, 0.0), (0.0, 0.0, 1), (45.0,), common=()).mtf.shape) == (1, 2, 3, 1, 1, 3)
    assert isinstance(a, metrics.ThroughFocusMTF) and a._fields == ("n", "mtf", "shifts", "centre")


# ------------------------------------------------------------------------------------------------------------------- C ABI
NAMES = ("tl_tfmtf_workspace_bytes", "tl_tfmtf_sums", "tl_tfmtf_seed")


def test_entry_points_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "tl_trace.h")).read()
    declared = set(re.findall(r"\b(tl_[a-z0-9_]+)\s*\(", hdr))
    dll = _lib.lib()
    for name in NAMES:
        assert name in declared and name in _lib.EXPORTS and hasattr(dll, name), name


def _dbl(v):
    return None if v is None else (C.c_double * len(v))(*v)


def _args(F=3, P=1000, W=3, x=ONE, y=ONE, cx=ONE, cy=ONE, ok=ONE, origin=ONE, nu_x=(0.0, 10.0), nu_y=(10.0, 0.0), J=None, first=-0.1,
          step=0.05, Z=4, **_):
    return (0, F, P, W, x, y, cx, cy, ok, W * P, 1, P, origin, _dbl(nu_x), _dbl(nu_y), (len(nu_x) if nu_x is not None else 2) if J is None else J,
            first, step, Z)


def _sums(dll, sums=ONE, ws=ONE, ws_bytes=1 << 30, **kw):
    return dll.tl_tfmtf_sums(*_args(**kw), sums, ws, ws_bytes, None)


def _seed(dll, g_sums=ONE, out=(ONE, ONE, ONE, ONE), ws=ONE, ws_bytes=1 << 30, **kw):
    return dll.tl_tfmtf_seed(*_args(**kw), g_sums, *out, ws, ws_bytes, None)


CALLS = ((_sums, b"tl_tfmtf_sums"), (_seed, b"tl_tfmtf_seed"))
NAN, INF = float("nan"), float("inf")
BAD = [dict(x=None), dict(y=None), dict(cx=None), dict(cy=None), dict(ok=None), dict(origin=None), dict(F=0), dict(P=0), dict(W=0),
       dict(F=-1), dict(P=-7), dict(F=1 << 16, W=1 << 15), dict(P=1 << 31), dict(nu_x=None), dict(nu_y=None), dict(J=0), dict(J=-1),
       dict(J=17), dict(Z=0), dict(Z=-1), dict(Z=17), dict(nu_x=(0.0, NAN)), dict(nu_y=(INF, 0.0)), dict(first=NAN), dict(first=-INF),
       dict(step=NAN), dict(step=INF)]
_ids = lambda d: ",".join(f"{k}={'NULL' if v is None else v}" for k, v in d.items())           # noqa: E731


def _refused(dll, call, name, **bad):
    dll.tl_unsup_loss(0, 0, 3, 100.0, ONE, None, 7.0, 0.2, ONE, ONE, ONE, ONE, None)               # another call's message first
    assert call(dll, **bad) == EINVAL, (name, bad)
    assert name + b":" in dll.tl_last_error(), dll.tl_last_error()


@pytest.mark.parametrize("bad", BAD, ids=_ids)
def test_bad_arguments_are_refused_before_any_hip_call(bad):
    for call, name in CALLS:
        _refused(_lib.lib(), call, name, **bad)


def test_missing_outputs_are_refused_and_one_plane_ignores_the_step():
    dll = _lib.lib()
    _refused(dll, _sums, b"tl_tfmtf_sums", sums=None)
    _refused(dll, _seed, b"tl_tfmtf_seed", g_sums=None)
    _refused(dll, _seed, b"tl_tfmtf_seed", out=(None, None, None, None))
    for call, name in CALLS:                                # Z = 1 with a step that is not finite: past the checks, to the workspace
        assert call(dll, Z=1, step=NAN, ws=None) == EWORKSPACE and name in dll.tl_last_error()


def test_workspace_plan_and_a_short_workspace():
    dll = _lib.lib()
    assert [R.bucket(16, Z) for Z in (1, 2, 3, 4, 5, 8, 9, 16)] == [(16, 1), (16, 2), (8, 4), (8, 4), (4, 8), (4, 8), (2, 16), (2, 16)]
    assert [R.bucket(J, 4) for J in (1, 2, 3, 4, 5, 8, 9)] == [(1, 4), (2, 4), (4, 4), (4, 4), (8, 4), (8, 4), (8, 4)] and R.bucket(1, 1) == (1, 1)
    for F, P, W in ((1, 1, 1), (2, 63, 3), (1, 4161, 2), (3, 1 << 20, 3), (65537, 2, 1), (21845, 3, 3), (7, 1 << 24, 1),
                    (1, (1 << 31) - 1, 1), (0, 5, 5), (5, 0, 5), (5, 5, 0), (1 << 16, 5, 1 << 15), (1, 1 << 31, 1)):
        for J in (0, 1, 2, 4, 5, 8, 16, 17):
            for Z in (0, 1, 2, 3, 4, 5, 8, 9, 16, 17):
                assert dll.tl_tfmtf_workspace_bytes(F, P, W, J, Z) == R.workspace_bytes(F, P, W, J, Z), (F, P, W, J, Z)
    need = dll.tl_tfmtf_workspace_bytes(3, 1 << 20, 3, 4, 16)
    assert 0 < need < (1 << 21), "the partials stay far below a byte per ray"
    for call, name in CALLS:
        assert call(dll, P=1 << 20, ws=None) == EWORKSPACE and name in dll.tl_last_error()
        short = dll.tl_tfmtf_workspace_bytes(3, 1 << 20, 3, 2, 4) - 1
        assert call(dll, P=1 << 20, ws_bytes=short) == EWORKSPACE and name in dll.tl_last_error()
