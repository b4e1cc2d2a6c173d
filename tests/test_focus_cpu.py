"""Through-focus spot moments (metrics.focus_moments / through_focus; tl_focus_moments / tl_focus_seed), what can be checked
without a GPU: the float64 torch path against the numpy definition of tests/focus_ref.py on the reference's fixture rays, against
brute force and analytic pins, its degenerate rows, pooling and gradients; the kernels' arithmetic emulated on the cases of
tests/focus_cases.py against the bounds the GPU tests use, with six wrong evaluations that must exceed them; the C ABI.

HOW "1e-12 RELATIVE" IS READ on the fixture rays.  The moments M agree with the reference to 1e-12 of the sum of their terms'
magnitudes (measured: 7e-15), and the finish, given the SAME M, agrees to 1e-12 of every output (measured: 2e-16).  End to end
the centred sums n a, n b, n c agree to 1e-12 of the RAW sums they are differences of.  They cannot agree to 1e-12 of
themselves: M is float64 by definition, the raw second moment of y is ~4e5 times the variance on these fixtures, so two correct
float64 evaluations of M that differ in the last bit already differ by 1e-16 x 4e5 in a (measured: 4e-10 of a on G2, both sides
being float64 evaluations of the definition)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import focus_cases as FC
import focus_ref as R
from conftest import ROOT, load_golden

from torchoptics_amd import _lib, metrics

FIXTURES = ("G2_cooke_16x16", "G4_tessar_32x32", "G5_cooke_failures")
COMMONS = (("wavelength",), (), ("field",), ("field", "wavelength"))
KEYS = ("n", "rms", "best_focus", "rms_best", "focus_t", "focus_s", "a", "b", "c")
EINVAL, EWORKSPACE = -1, -3                 # TL_EINVAL, TL_EWORKSPACE (include/tl_trace.h)
ONE = C.c_void_p(8)                         # any non-NULL pointer: never dereferenced on the paths taken here
_cache = {}


def fixture_rays(name):
    if name not in _cache:
        g = load_golden(name)
        _cache[name] = tuple(g[k] for k in ("x", "y", "cx", "cy", "ok"))
    return _cache[name]


def as_torch(arrays, dtype=torch.float64, grad=False):
    out = [torch.from_numpy(np.ascontiguousarray(a)) for a in arrays]
    return [t.to(dtype).requires_grad_(grad) if t.is_floating_point() else t for t in out]


def pooled(a, common):
    axes = tuple(d for d, name in ((1, "field"), (2, "wavelength")) if name in common)
    return a.sum(axis=axes) if axes else a


@pytest.mark.parametrize("name", FIXTURES)
def test_definition_on_fixture_rays(name):
    rays = fixture_rays(name)
    Mr, T = R.moments(*rays)
    if name == "G5_cooke_failures":
        assert Mr[..., 0].min() >= 636 and Mr[..., 0].max() <= 896 and Mr[..., 0].max() < rays[0].shape[2]
    M = metrics.focus_moments(*as_torch(rays), fused=False)
    assert M.dtype == torch.float64 and tuple(M.shape) == Mr.shape
    err = np.abs(M.numpy() - Mr) / np.maximum(T, 1e-300)
    print(name, "moments: largest error / sum|terms| =", err.max())
    assert err.max() <= 1e-12
    for common in COMMONS:
        ref = R.finish(Mr, common)
        same_m = metrics.through_focus_from_moments(torch.from_numpy(Mr), common)
        out = metrics.through_focus(*as_torch(rays), common=common, fused=False)
        n = ref["n"]
        raw = dict(a=pooled(T[..., 5] + T[..., 6] + (Mr[..., 1] ** 2 + Mr[..., 2] ** 2) / Mr[..., 0], common),
                   b=pooled(T[..., 9] + T[..., 10] + (np.abs(Mr[..., 1] * Mr[..., 3]) + np.abs(Mr[..., 2] * Mr[..., 4])) / Mr[..., 0], common),
                   c=pooled(T[..., 7] + T[..., 8] + (Mr[..., 3] ** 2 + Mr[..., 4] ** 2) / Mr[..., 0], common))
        for k in KEYS:
            got = getattr(same_m, k).numpy()
            assert got.shape == ref[k].shape and np.all(np.abs(got - ref[k]) <= 1e-12 * np.abs(ref[k])), (common, k)
            assert getattr(out, k).dtype == torch.float64 and tuple(getattr(out, k).shape) == ref[k].shape
        for k in "abc":
            e = np.abs(getattr(out, k).numpy() - ref[k]) * n / raw[k]
            print(name, common, k, "end to end: largest error / raw sum =", e.max(),
                  " / own value =", (np.abs(getattr(out, k).numpy() - ref[k]) / np.abs(ref[k])).max())
            assert e.max() <= 1e-12, (common, k)


def test_the_issues_numbers_on_the_cooke_fixture():
    out = R.through_focus(*fixture_rays("G2_cooke_16x16"), common=())
    assert np.allclose(out["best_focus"][0, 0], (0.283, 0.229, 0.105), atol=5e-4)           # axial colour, on axis, C d F
    assert abs(out["focus_t"][0, 2, 1] - 0.090) < 5e-4 and abs(out["focus_s"][0, 2, 1] + 0.063) < 5e-4
    assert abs(out["rms"][0, 0, 0] - 0.044) < 5e-4 and abs(out["rms_best"][0, 0, 0] - 0.018) < 5e-4


@pytest.mark.parametrize("common,centroid", [(c, "row") for c in COMMONS] + [(("wavelength",), "field"), (("field", "wavelength"), "field")])
def test_parabola_against_brute_force(common, centroid):
    """R(d) = sqrt(a + 2 b d + c d^2) against the RMS of the shifted live rays at five d.  Tolerance: the brute force centres
    before it squares, so its error is a few U; the parabola's coefficients carry U times raw / centred <= 4e5 (G2) .. 1e6, so
    64 U 1e6 = 7e-9 of R^2, half of it of R: 1e-8."""
    for name in ("G2_cooke_16x16", "G5_cooke_failures"):
        rays = fixture_rays(name)
        out = metrics.through_focus(*as_torch(rays), common=common, centroid=centroid, fused=False)
        a, b, c, bf = (getattr(out, k).numpy() for k in ("a", "b", "c", "best_focus"))
        for d in (-0.3, -0.05, 0.0, 0.1, 0.4):
            brute = R.rms_shifted(*rays, d, common, centroid)
            assert np.allclose(np.sqrt(a + 2 * b * d + c * d * d), brute, rtol=1e-8, atol=0), (name, d)
        at_best = R.rms_shifted(*rays, bf, common, centroid)
        assert np.allclose(out.rms_best.numpy(), at_best, rtol=1e-8, atol=0)
        for step in (-0.01, 0.01):
            assert np.all(R.rms_shifted(*rays, bf + step, common, centroid) > at_best)


def _cone(zs, zt, x0=0.3, y0=2.0, n=200, seed=0):
    rng = np.random.default_rng(seed)
    u, v = 0.2 * rng.uniform(-1, 1, (1, 1, n, 1)), 0.1 + 0.2 * rng.uniform(-1, 1, (1, 1, n, 1))
    cz = 1 / np.sqrt(1 + u * u + v * v)
    return x0 - zs * u, y0 - zt * v, u * cz, v * cz, np.ones(u.shape, bool)


def test_analytic_pins():
    """A stigmatic cone focuses at z0 with no spot left; an astigmatic bundle gives its two foci back and the slope-variance
    weighted mean of them.  Tolerances: u = cx / cz is recovered to a few U, the sums cancel to U raw / centred (<= 1e3 here):
    1e-11 of a focus; rms_best^2 is what is left of A after a cancellation to 1e-13 of it: rms_best <= 1e-6 rms."""
    rays = _cone(0.7, 0.7)
    out = metrics.through_focus(*as_torch(rays), common=(), fused=False)
    for k in ("best_focus", "focus_t", "focus_s"):
        assert abs(getattr(out, k).item() - 0.7) <= 1e-11, k
    assert out.rms.item() > 0.05 and out.rms_best.item() <= 1e-6 * out.rms.item()
    rays = _cone(-0.4, 0.9, seed=1)
    out = metrics.through_focus(*as_torch(rays), common=(), fused=False)
    _, (_, _, Cx), (_, _, Cy) = R.centred(R.moments(*rays)[0])
    assert abs(out.focus_s.item() + 0.4) <= 1e-11 and abs(out.focus_t.item() - 0.9) <= 1e-11
    assert abs(out.best_focus.item() - ((-0.4 * Cx + 0.9 * Cy) / (Cx + Cy)).item()) <= 1e-11
    assert out.rms_best.item() > 1e-3


def test_on_axis_rows_have_one_focus():
    """The fixtures' pupil grid maps onto itself under x <-> y, and so does an axial bundle: focus_t = focus_s up to the fp32
    rounding of the rays (2^-24 of coordinates and slopes, against centred sums of their own size: 1e-6 of a focus of ~0.1-1)."""
    for name in FIXTURES[:2]:
        tf = metrics.through_focus(*as_torch(fixture_rays(name)), common=(), fused=False)
        out = {k: getattr(tf, k).numpy() for k in KEYS}
        d = np.abs(out["focus_t"][0, 0] - out["focus_s"][0, 0])
        print(name, "on axis |focus_t - focus_s| =", d)
        assert np.all(d <= 1e-6 * np.maximum(1.0, np.abs(out["focus_t"][0, 0])))
        assert np.all(np.abs(out["focus_t"][0, 2] - out["focus_s"][0, 2]) > 0.05)


def test_degenerate_rows_are_finite_with_zero_gradients():
    x, y, cx, cy, ok = (a.copy() for a in fixture_rays("G2_cooke_16x16"))
    ok[0, 0, :, 0] = False                                   # n = 0
    ok[0, 0, :, 1] = False
    ok[0, 0, 11, 1] = True                                   # n = 1
    cx[0, 1, :, 0], cy[0, 1, :, 0] = cx[0, 1, 0, 0], cy[0, 1, 0, 0]          # a collimated bundle
    x[0, 1, :, 1], cx[0, 1, :, 1] = 0.0, 0.0                 # a meridional fan
    x[0, 0, :5, 0], cy[0, 0, :5, 0] = np.nan, np.inf         # what dead rays may hold
    t = as_torch((x, y, cx, cy, ok), grad=True)
    out = metrics.through_focus(*t, common=(), fused=False)
    for k in KEYS:
        assert torch.isfinite(getattr(out, k)).all(), k
    for f, w in ((0, 0), (0, 1)):
        assert out.n[0, f, w] == (0, 1)[w]
        for k in KEYS[1:]:
            assert getattr(out, k)[0, f, w] == 0, (f, w, k)
    assert out.best_focus[0, 1, 0] == 0 and out.focus_t[0, 1, 0] == 0 and out.focus_s[0, 1, 0] == 0
    assert out.rms_best[0, 1, 0] == out.rms[0, 1, 0] > 0
    assert out.focus_s[0, 1, 1] == 0 and out.focus_t[0, 1, 1] != 0 and out.best_focus[0, 1, 1] == out.focus_t[0, 1, 1]
    sum(getattr(out, k).sum() for k in KEYS[1:]).backward()
    for g in (q.grad for q in t[:4]):
        assert torch.isfinite(g).all()
        assert (g[0, 0, :, :2] == 0).all()                   # n = 0 and n = 1: nothing depends on the rays
    # the quotients that the rule zeroes carry no gradient: only rms = rms_best reaches the collimated row's slopes -- not at all
    t = as_torch((x, y, cx, cy, ok), grad=True)
    out = metrics.through_focus(*t, common=(), fused=False)
    (out.best_focus[0, 1, 0] + out.focus_t[0, 1, 0] + out.focus_s[0, 1, 0] + out.focus_s[0, 1, 1]).backward()
    assert all((q.grad == 0).all() for q in t[:4])


def test_pooling_and_the_field_centroid():
    rays = fixture_rays("G5_cooke_failures")
    Mr, T = R.moments(*rays)
    for common in COMMONS:
        out = metrics.through_focus(*as_torch(rays), common=common, fused=False)
        n, (Ax, Bx, Cx), (Ay, By, Cy) = R.centred(Mr)
        A, B, Cc = pooled(Ax + Ay, common), pooled(Bx + By, common), pooled(Cx + Cy, common)
        assert np.allclose(out.best_focus.numpy(), -B / Cc, rtol=1e-9) and np.array_equal(out.n.numpy(), pooled(n, common))
        assert np.allclose(out.rms_best.numpy() ** 2, (A - B * B / Cc) / pooled(n, common), rtol=1e-9)
    with pytest.raises(ValueError):
        metrics.through_focus(*as_torch(rays), common=(), centroid="field", fused=False)
    with pytest.raises(ValueError):
        metrics.through_focus(*as_torch(rays), common=("pupil",), fused=False)
    # centroid="field" differs from "row" by the lateral-colour term: sum_w n_w |c_w - c|^2, and likewise in b and c
    for common in (("wavelength",), ("field", "wavelength")):
        row = metrics.through_focus(*as_torch(rays), common=common, fused=False)
        fld = metrics.through_focus(*as_torch(rays), common=common, centroid="field", fused=False)
        n = Mr[..., 0]
        cen = Mr[..., 1:5] / n[..., None]                                           # x, y, u, v centroids per row
        mean = Mr[..., 1:5].sum(axis=2, keepdims=True) / n.sum(axis=2, keepdims=True)[..., None]
        d = cen - mean
        extra = dict(a=n * (d[..., 0] ** 2 + d[..., 1] ** 2), b=n * (d[..., 0] * d[..., 2] + d[..., 1] * d[..., 3]),
                     c=n * (d[..., 2] ** 2 + d[..., 3] ** 2))
        raw = dict(a=T[..., 5] + T[..., 6], b=T[..., 9] + T[..., 10], c=T[..., 7] + T[..., 8])
        for k in "abc":
            diff = (getattr(fld, k) - getattr(row, k)).numpy() * row.n.numpy()
            assert np.all(np.abs(diff - pooled(extra[k], common)) <= 1e-12 * pooled(raw[k], common)), k
        assert (fld.a > row.a).all() and torch.equal(fld.n, row.n)


def test_gradcheck_of_the_float64_path():
    B, F, W, P = FC.SHAPES["sub-wave"]
    rays = {k: a[:, :2, :7, :2] for k, a in FC.rays("sub-wave").items()}
    rays["ok"] = rays["ok"].copy()
    rays["ok"][0, 0, 3, 0] = False
    ok = torch.from_numpy(rays["ok"])
    t = [torch.from_numpy(rays[k].astype(np.float64)).requires_grad_(True) for k in ("x", "y", "cx", "cy")]
    for common, centroid in ((("wavelength",), "row"), ((), "row"), (("field", "wavelength"), "field")):
        fn = lambda x, y, cx, cy: torch.cat([q.reshape(-1) for q in                                     # noqa: E731
                                             metrics.through_focus(x, y, cx, cy, ok, common, centroid, fused=False)[1:]])
        assert torch.autograd.gradcheck(fn, t)
    assert torch.autograd.gradcheck(lambda *a: metrics.focus_moments(*a, ok, fused=False), t)


# ------------------------------------------------------------------------------------------- the kernels' arithmetic, emulated
@pytest.mark.parametrize("name", FC.CASES)
def test_emulated_kernel_arithmetic_stays_inside_the_bounds(name):
    rays = FC.rays(name)
    a = tuple(rays[k] for k in ("x", "y", "cx", "cy", "ok"))
    P = a[0].shape[2]
    Mr, T = R.moments(*a)
    with np.errstate(invalid="ignore", over="ignore"):
        M = R.emulate_moments(*a, FC.aligned_rows(name))
    bound = R.moment_bound(T, P)
    assert np.all(np.abs(M - Mr) <= bound), (np.abs(M - Mr) / np.maximum(bound, 1e-300)).max()
    if "clean" in rays:
        Mc = R.emulate_moments(*(rays["clean"][k] for k in ("x", "y", "cx", "cy", "ok")), FC.aligned_rows(name))
        assert np.array_equal(M, Mc) and np.array_equal(Mr, R.moments(*(rays["clean"][k] for k in ("x", "y", "cx", "cy", "ok")))[0])
    # the seeds of a dead ray are exact zeros, of a live one finite
    g, mag = R.seeds(*a, FC.g_moments(name))
    live = R.live_rays(a[2], a[3], a[4])
    assert all(np.isfinite(q).all() and np.all(q[~live] == 0) for q in g)


@pytest.mark.parametrize("wrong", ("drop", "twice", "dead", "cx_for_u", "swap9", "transpose"))
def test_wrong_evaluations_exceed_the_bounds(wrong):
    for name in ("sub-wave", "block-edge"):
        rays = FC.rays(name)
        a = tuple(rays[k] for k in ("x", "y", "cx", "cy", "ok"))
        Mr, T = R.moments(*a)
        M = R.emulate_moments(*a, FC.aligned_rows(name), wrong=wrong)
        assert np.any(np.abs(M - Mr) > R.moment_bound(T, a[0].shape[2])), (name, wrong)


def test_the_cases_reach_what_they_claim():
    al = {n: FC.aligned_rows(n) for n in FC.CASES}
    assert al["sub-wave"].any() and not al["sub-wave"].all()                   # both load paths in one case
    assert al["layout-tracer"].all() and not al["layout-slice"].any() and al["lens-batch"].all()
    assert R.plan(2, 4161) == (5, 1) and R.plan(6, 257) == (1, 1)
    assert len(R.launches(65535)) == 1 and R.launches(65537) == [(0, 65535), (65535, 2)]
    assert R.plan(9, 1 << 20)[0] * 9 <= 2048 + 9 and R.plan(9, 1 << 20)[1] > 1


# ------------------------------------------------------------------------------------------------------------------- C ABI
NAMES = ("tl_focus_workspace_bytes", "tl_focus_moments", "tl_focus_seed")


def test_entry_points_are_declared_bound_and_exported_and_the_abi_version_stays():
    hdr = open(os.path.join(ROOT, "include", "tl_trace.h")).read()
    declared = set(re.findall(r"\b(tl_[a-z0-9_]+)\s*\(", hdr))
    dll = _lib.lib()
    for name in NAMES:
        assert name in declared and name in _lib.EXPORTS and hasattr(dll, name), name
    assert dll.tl_version() == 15 == _lib.TL_ABI_VERSION
    assert int(re.search(r"#define TL_ABI_VERSION (\d+)", hdr).group(1)) == 15


def _fwd(dll, F=3, P=1000, W=3, x=ONE, y=ONE, cx=ONE, cy=ONE, ok=ONE, mom=ONE, ws=ONE, ws_bytes=1 << 30):
    return dll.tl_focus_moments(0, F, P, W, x, y, cx, cy, ok, W * P, 1, P, mom, ws, ws_bytes, None)


def _seed(dll, F=3, P=1000, W=3, x=ONE, y=ONE, cx=ONE, cy=ONE, ok=ONE, mom=ONE, out=(ONE, ONE, ONE, ONE), **_):
    return dll.tl_focus_seed(0, F, P, W, x, y, cx, cy, ok, W * P, 1, P, mom, *out, None)


BAD = [dict(x=None), dict(y=None), dict(cx=None), dict(cy=None), dict(ok=None), dict(mom=None),
       dict(F=0), dict(P=0), dict(W=0), dict(F=-1), dict(P=-7), dict(F=1 << 16, W=1 << 15), dict(P=1 << 31)]


@pytest.mark.parametrize("bad", BAD, ids=lambda d: ",".join(f"{k}={'NULL' if v is None else v}" for k, v in d.items()))
def test_bad_arguments_are_refused_before_any_hip_call(bad):
    dll = _lib.lib()
    for call, name in ((_fwd, b"tl_focus_moments"), (_seed, b"tl_focus_seed")):
        dll.tl_unsup_loss(0, 0, 3, 100.0, ONE, None, 7.0, 0.2, ONE, ONE, ONE, ONE, None)       # another call's message first
        assert call(dll, **bad) == EINVAL, (name, bad)
        assert name + b":" in dll.tl_last_error()
    assert _seed(dll, out=(None,) * 4) == EINVAL and b"tl_focus_seed" in dll.tl_last_error()


def test_workspace_plan_and_a_short_workspace():
    dll = _lib.lib()
    for F, P, W in ((1, 1, 1), (2, 63, 3), (1, 4161, 2), (3, 1 << 20, 3), (65537, 2, 1), (21845, 3, 3), (7, 1 << 24, 1),
                    (256, 4096, 3), (1, (1 << 31) - 1, 1), (0, 5, 5), (5, 0, 5), (5, 5, 0), (1 << 16, 5, 1 << 15), (1, 1 << 31, 1)):
        assert dll.tl_focus_workspace_bytes(F, P, W) == R.workspace_bytes(F, P, W), (F, P, W)
    need = dll.tl_focus_workspace_bytes(3, 1 << 20, 3)
    assert 0 < need < (1 << 20), "the partials stay far below a byte per ray"
    assert _fwd(dll, P=1 << 20, ws=None) == EWORKSPACE
    assert _fwd(dll, P=1 << 20, ws_bytes=need - 1) == EWORKSPACE and b"tl_focus_moments" in dll.tl_last_error()


def test_fused_has_no_cpu_fallback_and_none_takes_the_torch_path():
    rays = fixture_rays("G2_cooke_16x16")
    f32 = as_torch(rays, torch.float32)
    for fn in (metrics.focus_moments, metrics.through_focus):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(*f32, fused=True)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(*as_torch(rays), fused=True)
    a, b = metrics.through_focus(*f32), metrics.through_focus(*f32, fused=False)
    assert all(torch.equal(p, q) and p.dtype == torch.float32 for p, q in zip(a, b))
    assert tuple(a.rms.shape) == (1, 3) and tuple(metrics.through_focus(*f32, common=()).rms.shape) == (1, 3, 3)
    assert metrics.focus_moments(*f32).dtype == torch.float64
