"""Encircled / ensquared energy (metrics.enclosed_energy / enclosed_radius / spot_centroid; tl_enclosed_centroid / tl_enclosed_sums /
tl_enclosed_seed), what can be checked without a GPU: the float64 torch path against the numpy definition of tests/enclosed_ref.py
on the cases of tests/enclosed_cases.py, its gradients, the inverse, the bounds the GPU tests use (two float64 summation orders stay
inside them, an fp32 inner loop does not), what the cases claim, and the C ABI's refusals and workspace plan."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

import enclosed_cases as EC
import enclosed_ref as R
from conftest import ROOT

from torchoptics_amd import _lib, metrics

EINVAL, EWORKSPACE = -1, -3                 # TL_EINVAL, TL_EWORKSPACE (include/tl_trace.h)
ONE = C.c_void_p(8)                         # any non-NULL pointer: never dereferenced on the paths taken here
SMALL = tuple(n for n in EC.CASES if not n.startswith("many-rows"))


@functools.lru_cache(maxsize=None)
def _ref(name, shape, centre="row", soft=EC.SOFT):
    r = EC.rays(name)
    c = EC.given_centre(name) if centre == "given" else centre
    with np.errstate(invalid="ignore", over="ignore"):
        return r, R.enclosed_sums(r["x"], r["y"], r["ok"], EC.radii_of(name), soft, shape, c)


def _torch(r, dtype=torch.float64, grad=False):
    return [torch.from_numpy(r[k].astype(np.float64)).to(dtype).requires_grad_(grad) for k in ("x", "y")] + [torch.from_numpy(r["ok"])]


@pytest.mark.parametrize("shape", EC.SHAPE_NAMES)
@pytest.mark.parametrize("name", EC.CASES)
def test_torch_path_against_the_numpy_definition(name, shape):
    """Both are float64 evaluations of the definition (the torch path multiplies by 1 / tau, numpy divides): inside the bound."""
    for centre in ("row", "field", "given"):
        r, ref = _ref(name, shape, centre)
        c = torch.from_numpy(EC.given_centre(name)) if centre == "given" else centre
        S, sums, cen = metrics._enclosed_torch(*_torch(r), EC.radii_of(name), tuple(1 / EC.SOFT for _ in EC.radii_of(name)), shape, c)
        assert np.all(np.abs(S.numpy() - ref["S"]) <= ref["S_bound"]) and np.array_equal(S.numpy()[..., 0], ref["S"][..., 0])
        assert np.all(np.abs(sums.numpy() - ref["sums"]) <= ref["sums_bound"]), (name, shape, centre)
        assert np.isfinite(sums.numpy()).all()
        for common in (("wavelength",), (), ("field", "wavelength")):
            out = metrics.enclosed_energy(*_torch(r), EC.radii_of(name), EC.SOFT, shape=shape, common=common, centre=c, fused=False)
            n, E = R.energy(ref["S"], ref["sums"], common)
            assert np.array_equal(out.n.numpy(), n) and np.allclose(out.energy.numpy(), E, rtol=1e-9, atol=1e-12)
            assert out.energy.dtype == torch.float64 and tuple(out.centre.shape) == ref["centre"].shape
            assert np.all(out.energy.numpy()[n == 0] == 0)


def test_the_cases_reach_what_they_claim():
    """The curve runs from a fraction at R_4 to exactly 1 at R_16 on every regular case, so the 0.8 crossing lies inside the
    range; nearly every live ray lies in some band; with softness 1e-12 no ray lies in a band and every sum is an integer."""
    for name in SMALL:
        for shape in EC.SHAPE_NAMES:
            r, ref = _ref(name, shape)
            n, E = R.energy(ref["S"], ref["sums"], ())
            rows = n > 1
            assert np.all(E[n > 0][:, -1] == 1.0), name
            if rows.any() and name != "one-ray":
                assert 0.1 <= E[rows][:, 3].min() and E[rows][:, 3].max() <= 0.85, (name, shape, E[rows][:, 3])
            rad, reached = R.enclosed_radius(E[n > 0], EC.RADII, 0.8)
            assert reached.all() and np.all((rad > 0) & (rad < EC.RADII[-1]))
            t = ref["terms"]
            in_band = ((t.e > 0) & (t.e < 1)).any(axis=-1)
            assert in_band[t.live].mean() >= (0.9 if name != "one-ray" else 0.0), (name, in_band[t.live].mean())
            _, hard = _ref(name, shape, soft=1e-12)
            assert np.all((hard["terms"].e == 0) | (hard["terms"].e == 1)) and np.all(hard["sums"] == np.round(hard["sums"]))
    r = EC.rays("poisoned")
    assert not np.isfinite(r["x"][~r["ok"]]).all() and np.isfinite(r["x"][r["ok"]]).all() and np.abs(r["x"][r["ok"]]).max() < 100
    assert np.array_equal(r["clean"]["x"][r["ok"]], r["x"][r["ok"]]) and np.all(r["clean"]["x"][~r["ok"]] == 0)
    assert R.plan(2, 4161) == (5, 1) and R.launches(65537) == [(0, 65535), (65535, 2)]


@pytest.mark.parametrize("shape", EC.SHAPE_NAMES)
def test_the_bound_tells_fp64_from_fp32(shape):
    """Two float64 evaluations in other summation orders stay inside the bound on every case; with the inner loop in float32 at
    least one case breaks it (in fact every one with more than a ray: fp32 leaves ~2^-24 (R + rho) / tau ~ 1e-6 per term)."""
    broken = []
    for name in SMALL:
        for centre in ("row", "given"):
            r, ref = _ref(name, shape, centre)
            args = (r["x"], r["y"], r["ok"], EC.RADII, EC.SOFT, shape, ref["centre"])
            with np.errstate(invalid="ignore", over="ignore"):
                for order in ("forward", "reverse", "blocks"):
                    s = R.sums_in_order(*args, order)
                    assert np.all(np.abs(s - ref["sums"]) <= ref["sums_bound"]), (name, centre, order)
                s32 = R.sums_in_order(*args, "forward", inner=np.float32)
            broken.append(bool(np.any(np.abs(s32 - ref["sums"]) > ref["sums_bound"])))
            assert np.allclose(s32, ref["sums"], atol=1e-2 * r["x"].shape[2])       # (the same quantity, only coarser)
    assert any(broken)
    print("fp32 inner loop breaks the bound on", sum(broken), "of", len(broken), "evaluations")


def test_the_seed_reference_is_the_gradient_of_the_sums():
    """The analytic seeds of enclosed_ref against autograd through the float64 torch definition (another derivation of them)."""
    for name, shape, centre in (("sub-wave", "circle", "row"), ("sub-wave", "square", "field"), ("dead-row", "circle", "given"),
                                ("poisoned", "square", "row"), ("lens-batch", "circle", "field"), ("block-edge", "square", "given")):
        r, ref = _ref(name, shape, centre)
        K = len(EC.RADII)
        g_sums, g_S = EC.seeds(name, K)
        want = R.seeds(ref, g_sums, g_S, EC.given_centre(name) if centre == "given" else centre)
        x, y, ok = _torch(r, grad=True)
        c = torch.from_numpy(EC.given_centre(name)).requires_grad_(True) if centre == "given" else centre
        S, sums, _ = metrics._enclosed_torch(x, y, ok, EC.RADII, tuple(1 / EC.SOFT for _ in EC.RADII), shape, c)
        ((sums * torch.from_numpy(g_sums)).sum() + (S * torch.from_numpy(g_S)).sum()).backward()
        for got, k in ((x.grad, "gx"), (y.grad, "gy")):
            scale = np.abs(want[k]).max()
            assert np.allclose(got.numpy(), want[k], rtol=1e-9, atol=1e-9 * scale), (name, shape, centre, k)
            assert np.all(got.numpy()[~r["ok"]] == 0) and np.isfinite(got.numpy()).all()
        if centre == "given":
            assert np.allclose(c.grad.numpy(), want["gc"], rtol=1e-9, atol=1e-9 * np.abs(want["gc"]).max())


@pytest.mark.parametrize("shape", EC.SHAPE_NAMES)
def test_gradcheck_of_the_float64_path(shape):
    r = {k: a[:, :2, :7, :2].copy() for k, a in EC.rays("sub-wave").items()}
    r["ok"][0, 0, 3, 0] = False
    ok = torch.from_numpy(r["ok"])
    x, y = (torch.from_numpy(r[k].astype(np.float64)).requires_grad_(True) for k in ("x", "y"))
    radii, soft = EC.RADII[1::3], 0.006
    inv = tuple(1 / soft for _ in radii)
    given = torch.from_numpy(EC.given_centre("sub-wave")[:, :2, :2]).requires_grad_(True)
    for centre in ("row", "field"):
        assert torch.autograd.gradcheck(lambda a, b: metrics._enclosed_torch(a, b, ok, radii, inv, shape, centre)[:2], (x, y))
        fn = lambda a, b: metrics.enclosed_energy(a, b, ok, radii, soft, shape=shape, centre=centre, fused=False).energy     # noqa: E731
        assert torch.autograd.gradcheck(fn, (x, y))
    assert torch.autograd.gradcheck(lambda a, b, c: metrics._enclosed_torch(a, b, ok, radii, inv, shape, c)[:2], (x, y, given))
    fn = lambda a, b: metrics.enclosed_radius(metrics.enclosed_energy(a, b, ok, radii, soft, shape=shape, fused=False).energy,   # noqa: E731
                                              radii, 0.6)[0]
    assert torch.autograd.gradcheck(fn, (x, y))
    assert torch.autograd.gradcheck(lambda a, b: metrics.spot_centroid(a, b, ok, fused=False)[1], (x, y))


def test_enclosed_radius():
    radii = (1.0, 2.0, 3.0, 5.0)
    E = torch.tensor([[0.2, 0.4, 0.6, 1.0],                 # a linear curve: E = R / 5
                      [0.1, 0.2, 0.3, 0.4],                 # never reaches 0.5
                      [0.0, 0.9, 0.3, 0.95],                # the FIRST crossing is taken, not the last
                      [0.7, 0.8, 0.9, 1.0]], dtype=torch.float64, requires_grad=True)   # in the first interval, from (0, 0)
    for frac in (0.1, 0.3, 0.5, 0.77, 1.0):
        rad, reached = metrics.enclosed_radius(E[:1], radii, frac)
        assert reached.all() and abs(rad.item() - 5 * frac) <= 1e-15 * 5
    rad, reached = metrics.enclosed_radius(E, radii, 0.5)
    assert reached.tolist() == [True, False, True, True] and rad.dtype == torch.float64
    assert rad[1].item() == 5.0 and abs(rad[2].item() - (1 + 0.5 / 0.9)) < 1e-15 and abs(rad[3].item() - 0.5 / 0.7) < 1e-15
    rad.sum().backward()
    assert (E.grad[1] == 0).all() and E.grad[2, 2] == 0 and E.grad[2, 3] == 0 and E.grad[2, 1] != 0 and E.grad[3, 0] != 0
    ref, ref_reached = R.enclosed_radius(E.detach().numpy(), radii, 0.5)
    assert np.allclose(rad.detach().numpy(), ref, rtol=1e-15) and np.array_equal(reached.numpy(), ref_reached)
    f32 = metrics.enclosed_radius(E.detach().float()[None], radii, 0.5)[0]
    assert f32.dtype == torch.float64 and tuple(f32.shape) == (1, 4)
    with pytest.raises(ValueError):
        metrics.enclosed_radius(E, radii[:3], 0.5)


def test_python_refusals_and_the_dispatch():
    r = EC.rays("sub-wave")
    f32, f64 = _torch(r, torch.float32), _torch(r)
    for bad in (dict(radii=()), dict(radii=(0.01, 0.01)), dict(radii=(0.02, 0.01)), dict(radii=(-1.0, 1.0)), dict(softness=0.0),
                dict(softness=(0.1, 0.2, 0.3)), dict(softness=float("inf")), dict(radii=(float("nan"),)), dict(shape="disc"),
                dict(common=("pupil",)), dict(centre="lens")):
        kw = dict(dict(radii=(0.01, 0.02), softness=0.004), **bad)
        with pytest.raises(ValueError):
            metrics.enclosed_energy(*f64, fused=False, **kw)
    for args in (f32, f64):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            metrics.enclosed_energy(*args, EC.RADII, EC.SOFT, fused=True)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            metrics.spot_centroid(*args, fused=True)
    a, b = metrics.enclosed_energy(*f32, EC.RADII, EC.SOFT), metrics.enclosed_energy(*f32, EC.RADII, EC.SOFT, fused=False)
    assert all(torch.equal(p, q) and p.dtype == torch.float32 for p, q in zip(a, b))
    assert tuple(a.energy.shape) == (1, 2, 16) and tuple(a.n.shape) == (1, 2) and tuple(a.centre.shape) == (1, 2, 3, 2)
    n, c = metrics.spot_centroid(*f32)
    S, _ = R.spot_sums(r["x"], r["y"], r["ok"])
    assert np.array_equal(n.numpy(), S[..., 0]) and np.allclose(c.numpy(), S[..., 1:3] / S[..., :1], rtol=1e-6)
    soft = tuple(0.002 + 0.0005 * k for k in range(16))                         # one softness per radius
    per = metrics.enclosed_energy(*f64, EC.RADII, soft, common=(), fused=False)
    ref = R.enclosed_sums(r["x"], r["y"], r["ok"], EC.RADII, soft, "circle", "row")
    assert np.allclose(per.energy.numpy(), R.energy(ref["S"], ref["sums"], ())[1], rtol=1e-12, atol=1e-14)


# ------------------------------------------------------------------------------------------------------------------- C ABI
NAMES = ("tl_enclosed_workspace_bytes", "tl_enclosed_centroid", "tl_enclosed_sums", "tl_enclosed_seed")


def test_entry_points_are_declared_bound_and_exported_and_the_abi_version_stays():
    hdr = open(os.path.join(ROOT, "include", "tl_trace.h")).read()
    declared = set(re.findall(r"\b(tl_[a-z0-9_]+)\s*\(", hdr))
    dll = _lib.lib()
    for name in NAMES:
        assert name in declared and name in _lib.EXPORTS and hasattr(dll, name), name
    assert dll.tl_version() == 15 == _lib.TL_ABI_VERSION
    assert int(re.search(r"#define TL_ABI_VERSION (\d+)", hdr).group(1)) == 15


def _dbl(v):
    return None if v is None else (C.c_double * len(v))(*v)


def _args(F=3, P=1000, W=3, x=ONE, y=ONE, ok=ONE, **_):
    return (0, F, P, W, x, y, ok, W * P, 1, P)


def _edge(radii=(0.01, 0.02), inv=(250.0, 250.0), K=None, shape=0, **_):
    return (_dbl(radii), _dbl(inv), len(radii) if K is None else K, shape)


def _centroid(dll, S=ONE, ws=ONE, ws_bytes=1 << 30, **kw):
    return dll.tl_enclosed_centroid(*_args(**kw), S, ws, ws_bytes, None)


def _sums(dll, centre=ONE, sums=ONE, ws=ONE, ws_bytes=1 << 30, **kw):
    return dll.tl_enclosed_sums(*_args(**kw), centre, *_edge(**kw), sums, ws, ws_bytes, None)


def _seed(dll, centre=ONE, g_sums=ONE, g_lin=None, out=(ONE, ONE, ONE), ws=ONE, ws_bytes=1 << 30, **kw):
    return dll.tl_enclosed_seed(*_args(**kw), centre, *_edge(**kw), g_sums, g_lin, *out, ws, ws_bytes, None)


CALLS = ((_centroid, b"tl_enclosed_centroid"), (_sums, b"tl_enclosed_sums"), (_seed, b"tl_enclosed_seed"))
BAD_RAYS = [dict(x=None), dict(y=None), dict(ok=None), dict(F=0), dict(P=0), dict(W=0), dict(F=-1), dict(P=-7),
            dict(F=1 << 16, W=1 << 15), dict(P=1 << 31)]
NAN, INF = float("nan"), float("inf")
BAD_EDGE = [dict(centre=None), dict(radii=None, K=2), dict(inv=None), dict(K=0), dict(K=-1), dict(K=33), dict(shape=2), dict(shape=-1),
            dict(radii=(0.0, 0.02)), dict(radii=(-0.01, 0.02)), dict(radii=(0.01, NAN)), dict(radii=(0.01, INF)),
            dict(inv=(250.0, 0.0)), dict(inv=(-1.0, 250.0)), dict(inv=(NAN, 250.0)), dict(inv=(250.0, INF)),
            dict(radii=(0.02, 0.02)), dict(radii=(0.02, 0.01))]
_ids = lambda d: ",".join(f"{k}={'NULL' if v is None else v}" for k, v in d.items())           # noqa: E731


def _refused(dll, call, name, **bad):
    dll.tl_unsup_loss(0, 0, 3, 100.0, ONE, None, 7.0, 0.2, ONE, ONE, ONE, ONE, None)               # another call's message first
    assert call(dll, **bad) == EINVAL, (name, bad)
    assert name + b":" in dll.tl_last_error(), dll.tl_last_error()


@pytest.mark.parametrize("bad", BAD_RAYS, ids=_ids)
def test_bad_rays_are_refused_before_any_hip_call(bad):
    for call, name in CALLS:
        _refused(_lib.lib(), call, name, **bad)


@pytest.mark.parametrize("bad", BAD_EDGE, ids=_ids)
def test_a_bad_edge_is_refused_before_any_hip_call(bad):
    for call, name in CALLS[1:]:
        _refused(_lib.lib(), call, name, **bad)


def test_missing_outputs_are_refused():
    dll = _lib.lib()
    _refused(dll, _centroid, b"tl_enclosed_centroid", S=None)
    _refused(dll, _sums, b"tl_enclosed_sums", sums=None)
    _refused(dll, _seed, b"tl_enclosed_seed", g_sums=None)
    _refused(dll, _seed, b"tl_enclosed_seed", out=(None, None, None))


def test_workspace_plan_and_a_short_workspace():
    dll = _lib.lib()
    for F, P, W in ((1, 1, 1), (2, 63, 3), (1, 4161, 2), (3, 1 << 20, 3), (65537, 2, 1), (21845, 3, 3), (7, 1 << 24, 1),
                    (256, 4096, 3), (1, (1 << 31) - 1, 1), (0, 5, 5), (5, 0, 5), (5, 5, 0), (1 << 16, 5, 1 << 15), (1, 1 << 31, 1)):
        for K in (0, 1, 2, 3, 4, 16, 32, 33):
            assert dll.tl_enclosed_workspace_bytes(F, P, W, K) == R.workspace_bytes(F, P, W, K), (F, P, W, K)
        # the plan is the focus kernels', restated in tl_enclosed.hip: one partial per block of the same grid
        assert dll.tl_enclosed_workspace_bytes(F, P, W, 11) == dll.tl_focus_workspace_bytes(F, P, W), (F, P, W)
    need = dll.tl_enclosed_workspace_bytes(3, 1 << 20, 3, 2)
    assert 0 < need < (1 << 20), "the partials stay far below a byte per ray"
    for call, name in CALLS:
        assert call(dll, P=1 << 20, ws=None) == EWORKSPACE and name in dll.tl_last_error()
        short = dll.tl_enclosed_workspace_bytes(3, 1 << 20, 3, 1 if call is _centroid else 2) - 1
        assert call(dll, P=1 << 20, ws_bytes=short) == EWORKSPACE and name in dll.tl_last_error()
