"""The Zernike wavefront fit from ray errors (metrics.zernike_fit / zernike_moments / zernike_basis; tl_zfit_moments / tl_zfit_solve /
tl_zfit_seed), what can be checked without a GPU: the float64 torch path against the numpy definition of tests/zfit_ref.py
(lstsq on the design matrix) on the cases of tests/zfit_cases.py, exact recovery of known coefficients, the basis by quadrature,
the validity rule, the kernels' summation emulated against the bounds the GPU tests use -- with an fp32 inner loop and wrong
evaluations that must exceed them --, the C ABI's refusals, and the pin against the oracle's optical path length.

THE ORACLE PIN.  11-row double Gauss in float64, d line, a 24 x 48 polar fan, no ray aiming, traced by
oracle.trace_skew_general with n_index.  The slope fit with scale = epd / (2 efl) / lambda is compared with a direct Zernike fit
of W = OPD - ((x - Qx) cx + (y - Qy) cy) over the same pupil coordinates, Q the slope fit's tilt point.  Measured (waves,
slope fit / OPD fit): on axis rms 0.0445 / 0.0448 (0.5 %), Z4 0.00600 / 0.00591 (1.6 %), Z11 -0.04389 / -0.04413 (0.6 %); field
0.707 rms 0.0693 / 0.0683 (1.4 %); full field rms 0.1193 / 0.1135 (5.1 %), Z4 4.4 %.  The asserted limits are three times the
measured on-axis and full-field differences: 5 % and 15 %.  A wrong Noll norm or a factor 2 in the slope relation is off by 40 %
and more."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

import zfit_cases as ZC
import zfit_ref as R
from conftest import ROOT

from torchoptics_amd import _lib, metrics

EINVAL, EWORKSPACE = -1, -3                 # TL_EINVAL, TL_EWORKSPACE (include/tl_trace.h)
ONE = C.c_void_p(8)                         # any non-NULL pointer: never dereferenced on the paths taken here
BAND = (2.0 ** -34, 2.0 ** -26)             # reference pivots in here are too close to the floor to compare flags
COMBOS = [(name, pupil, order) for name in ZC.CASES for pupil in ZC.PUPILS for order in ZC.orders_of(name)]


@functools.lru_cache(maxsize=None)
def reference(name, pupil, order):
    """The case's arrays, seeds and float64 reference, computed once and left unchanged."""
    rays = ZC.rays(name, pupil)
    g_a, g_q = ZC.seeds(name, order)
    with np.errstate(invalid="ignore", over="ignore"):
        ref = R.fit(rays["x"], rays["y"], rays["ok"], rays["px"], rays["py"], order, g_a, g_q)
    return rays, g_a, g_q, ref


def as_torch(rays, dtype=torch.float64, grad=False):
    out = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in rays.items() if k != "clean"}
    return {k: (t.to(dtype).requires_grad_(grad and k in "xy") if t.is_floating_point() else t) for k, t in out.items()}


def worst(got, ref, bound):
    return float((np.abs(np.asarray(got, np.float64) - ref) / np.maximum(bound, 1e-300)).max())


@pytest.mark.parametrize("name,pupil,order", COMBOS, ids=lambda v: str(v))
def test_float64_path_against_the_numpy_definition(name, pupil, order):
    """fused=False (normal equations, torch.linalg) against lstsq on the design matrix, inside the bounds the kernels get."""
    rays, g_a, g_q, ref = reference(name, pupil, order)
    t = as_torch(rays, grad=True)
    M = metrics.zernike_moments(t["x"], t["y"], t["ok"], t["px"], t["py"], order, fused=False)
    n, a, q, valid = metrics._zernike_fit_torch(t["x"], t["y"], t["ok"], t["px"], t["py"], order)
    ((a * torch.from_numpy(g_a)).sum() + (q * torch.from_numpy(g_q)).sum()).backward()
    assert M.dtype == a.dtype == q.dtype == torch.float64 and not M.requires_grad
    compare = (ref["pivot"] < BAND[0]) | (ref["pivot"] > BAND[1])
    assert np.array_equal(valid.numpy()[compare], ref["valid"][compare]) and np.array_equal(n.numpy(), ref["n"])
    same = valid.numpy() == ref["valid"]
    got = dict(M=M.numpy(), a=a.detach().numpy(), q=q.detach().numpy(), gx=t["x"].grad.numpy(), gy=t["y"].grad.numpy())
    for k, v in got.items():
        mask = same if k in ("q",) else same[..., None] if k in ("a", "M") else np.broadcast_to(same[:, :, None, :], v.shape)
        assert np.isfinite(v).all() and np.all((np.abs(v - ref[k]) <= ref[k + "_bound"]) | ~mask), (k, worst(v, ref[k], ref[k + "_bound"]))
    dead = ~np.broadcast_to(rays["ok"], got["gx"].shape)
    assert np.all(got["gx"][dead] == 0) and np.all(got["gy"][dead] == 0)
    off = ~valid.numpy()
    assert np.all(got["a"][off] == 0) and np.all(got["q"][off] == 0)
    assert np.all(got["gx"][np.broadcast_to(off[:, :, None, :], got["gx"].shape)] == 0)
    # the public function: the finish of the definition, in the dtype of x
    out = metrics.zernike_fit(*(as_torch(rays)[k] for k in ZC.KEYS), max_order=order, scale=2.5, fused=False)
    want = R.finish(ref["a"], ref["q"], ref["n"], ref["valid"], 2.5)
    assert out.coeffs.dtype == torch.float64 and out.valid.dtype == torch.bool and tuple(out.coeffs.shape) == ref["a"].shape
    ok = same & ref["valid"]
    assert np.allclose(out.coeffs.numpy()[ok], want["coeffs"][ok], rtol=0, atol=2.5 * ref["a_bound"][ok].max() if ok.any() else 0)
    for k in ("rms", "rms_focus"):
        tol = 2.5 * np.sqrt((ref["a_bound"] ** 2).sum(-1))
        assert np.all(np.abs(getattr(out, k).numpy() - want[k])[ok] <= tol[ok] + 1e-15 * want[k][ok]), k
    assert np.all(out.rms.numpy()[off] == 0) and np.all(out.residual.numpy()[off] == 0) and np.all(out.coeffs.numpy()[off] == 0)


def test_the_validity_rule_on_the_cases():
    """Rows with 2 n < J are invalid, every row of P >= 63 rays is valid (but the empty and one-ray rows of "dead-row"), and no
    reference pivot lies in the band where flags are not compared."""
    seen = 0
    for name, pupil, order in COMBOS:
        _, _, _, ref = reference(name, pupil, order)
        J = ZC.sizes(order)[0]
        few = 2 * ref["n"] < J
        assert not ref["valid"][few].any()
        piv = ref["pivot"][~few]
        assert not ((piv >= BAND[0]) & (piv <= BAND[1])).any(), (name, pupil, order, piv.min())
        if ZC.SHAPES[name][3] >= 63:
            assert np.array_equal(ref["valid"], ~few) and ref["valid"].any(), (name, pupil, order)
            assert piv.min() > 0.05, (name, pupil, order, piv.min())
            seen += 1
        else:
            assert not ref["valid"].any(), name
    assert seen and reference("one-ray", "shared", 4)[3]["n"].item() == 1
    assert reference("dead-row", "shared", 4)[3]["n"][0, 0].tolist() == [0, 1]
    assert not reference("many-rows-b", "per-row", 2)[3]["valid"].any()


def test_a_meridional_fan_is_invalid_with_zero_gradients():
    P = 80
    py = torch.linspace(-1, 1, P, dtype=torch.float64).reshape(1, 1, P, 1)
    px = torch.zeros_like(py)
    x = torch.zeros(1, 1, P, 1, dtype=torch.float64, requires_grad=True)
    y = (0.01 * py ** 3).detach().requires_grad_(True)
    out = metrics.zernike_fit(x, y, torch.ones_like(py, dtype=torch.bool), px, py, max_order=4, fused=False)
    assert not out.valid.any() and out.n.item() == P
    assert all((getattr(out, k) == 0).all() for k in ("coeffs", "rms", "rms_focus", "residual"))
    (out.rms.sum() + out.residual.sum() + out.coeffs.sum()).backward()
    assert (x.grad == 0).all() and (y.grad == 0).all()


@pytest.mark.parametrize("order", ZC.ORDERS)
def test_known_coefficients_are_recovered_exactly(order):
    """Spots that ARE a Zernike gradient field, in float64: the coefficients come back to 1e-10 relative, the residual is
    rounding noise, and px, py, ray_ok get no gradient."""
    J = ZC.sizes(order)[0]
    rng = np.random.default_rng(order)
    P = 300
    rho, th = np.sqrt(rng.random((1, 1, P, 1))), 2 * np.pi * rng.random((1, 1, P, 1))
    p, q = rho * np.cos(th), rho * np.sin(th)
    a = rng.standard_normal((2, 3, 2, J))
    Zp, Zq, _, _ = R.gradients(p[0, 0, :, 0], q[0, 0, :, 0], order, R.basis(order))
    x = np.einsum("pj,bfwj->bfpw", Zp, a)
    y = np.einsum("pj,bfwj->bfpw", Zq, a)
    ok = rng.random(x.shape) > 0.15
    px, py = torch.from_numpy(p).requires_grad_(True), torch.from_numpy(q).requires_grad_(True)
    xt, yt = torch.from_numpy(x).requires_grad_(True), torch.from_numpy(y).requires_grad_(True)
    scale = torch.tensor([1.5, 0.5], dtype=torch.float64, requires_grad=True)              # one per wavelength
    out = metrics.zernike_fit(xt, yt, torch.from_numpy(ok), px, py, max_order=order, scale=scale, fused=False)
    want = a * np.array([1.5, 0.5])[:, None]
    assert out.valid.all() and np.array_equal(out.n.numpy(), ok.sum(axis=2))
    assert np.all(np.abs(out.coeffs.detach().numpy() - want) <= 1e-10 * np.abs(want).max())
    assert np.allclose(out.rms.detach().numpy(), np.sqrt((want[..., 2:] ** 2).sum(-1)), rtol=1e-10)
    assert np.allclose(out.rms_focus.detach().numpy(), np.sqrt((want[..., 3:] ** 2).sum(-1)), rtol=1e-10)
    assert out.residual.max().item() <= 1e-6 * np.abs(x).max()
    (out.rms.sum() + out.rms_focus.sum()).backward()
    assert px.grad is None and py.grad is None and torch.isfinite(xt.grad).all() and (xt.grad[torch.from_numpy(~ok)] == 0).all()
    assert scale.grad is not None and (scale.grad != 0).all()


def test_gradcheck_of_the_float64_path():
    rays = ZC.rays("sub-wave", "per-row")
    t = as_torch({k: v[:, :1, :40, :2] for k, v in rays.items()})
    t["ok"][0, 0, 3, 0] = False
    x, y = t["x"].requires_grad_(True), t["y"].requires_grad_(True)
    scale = torch.tensor(3.0, dtype=torch.float64, requires_grad=True)
    fn = lambda x, y, s: torch.cat([q.reshape(-1) for q in                                         # noqa: E731
                                    metrics.zernike_fit(x, y, t["ok"], t["px"], t["py"], 3, s, fused=False)[2:]])
    assert torch.autograd.gradcheck(fn, (x, y, scale))


@pytest.mark.parametrize("order", ZC.ORDERS)
def test_the_basis_is_orthonormal_by_quadrature(order):
    """Gauss-Legendre in rho (exact for the degrees here), equal weights in theta: <Z_j Z_k> = delta_jk over the unit disc, with
    the constant terms put back (zernike_basis leaves them out: they have no gradient); and the named polynomials."""
    b = metrics.zernike_basis(order)
    J = ZC.sizes(order)[0]
    assert tuple(b.T.shape) == (J, J) and len(b.exponents) == len(b.noll) == J and b.noll[0] == (2, 1, 1) and b.noll[1] == (3, 1, -1)
    assert b.noll[2] == (4, 2, 0) and [j for j, _, _ in b.noll] == list(range(2, J + 2))
    assert np.allclose(b.T.numpy(), R.basis(order), rtol=0, atol=1e-12)
    r, wr = np.polynomial.legendre.leggauss(16)
    r, wr = (r + 1) / 2, wr / 2
    th = 2 * np.pi * (np.arange(32) + 0.5) / 32
    rr, tt = np.meshgrid(r, th, indexing="ij")
    w = (2 * wr[:, None] * rr / 32).ravel()                                    # the mean over the disc
    p, q = (rr * np.cos(tt)).ravel(), (rr * np.sin(tt)).ravel()
    Z = np.stack([p ** a * q ** c for a, c in b.exponents], axis=-1) @ b.T.numpy()
    Z = Z - w @ Z                                                              # every Z_j, j >= 2, has mean 0
    assert np.allclose(Z.T @ (w[:, None] * Z), np.eye(J), rtol=0, atol=1e-12)
    rho2 = p * p + q * q
    assert np.allclose(Z[:, 0], 2 * p) and np.allclose(Z[:, 1], 2 * q) and np.allclose(Z[:, 2], np.sqrt(3) * (2 * rho2 - 1))
    if order >= 4:
        assert np.allclose(Z[:, 9], np.sqrt(5) * (6 * rho2 ** 2 - 6 * rho2 + 1))
    with pytest.raises(ValueError):
        metrics.zernike_basis(7)
    with pytest.raises(ValueError):
        metrics.zernike_fit(*(torch.zeros(1, 1, 4, 1),) * 2, torch.ones(1, 1, 4, 1), *(torch.zeros(1, 1, 4, 1),) * 2, max_order=1)


# ------------------------------------------------------------------------------------------- the kernels' arithmetic, emulated
EMULATED = [c for c in COMBOS if c[0] != "many-rows-b"]


@pytest.mark.parametrize("name,pupil,order", EMULATED, ids=lambda v: str(v))
def test_emulated_kernel_sums_stay_inside_the_bounds_and_an_fp32_inner_loop_does_not(name, pupil, order):
    rays, _, _, ref = reference(name, pupil, order)
    a = tuple(rays[k] for k in ZC.KEYS)
    al = ZC.aligned_rows(name, pupil)
    with np.errstate(invalid="ignore", over="ignore"):
        M = R.emulate_moments(*a, order, al)
        M32 = R.emulate_moments(*a, order, al, dtype=np.float32)
    assert np.all(np.abs(M - ref["M"]) <= ref["M_bound"]), worst(M, ref["M"], ref["M_bound"])
    assert np.array_equal(M[..., 0], ref["n"])
    if ref["n"].max() > 1:
        assert np.any(np.abs(M32 - ref["M"]) > ref["M_bound"])
        assert worst(M32, ref["M"], ref["M_bound"]) > 1e3                      # (not by a hair: by the ratio of the two precisions)
    if "clean" in rays:
        Mc = R.emulate_moments(*(rays["clean"][k] for k in ZC.KEYS), order, al)
        assert np.array_equal(M, Mc) and np.isfinite(M).all()


@pytest.mark.parametrize("wrong", ("drop", "twice", "swap_pq"))
def test_wrong_evaluations_exceed_the_bounds(wrong):
    for name in ZC.ALL_ORDER_CASES:
        rays, _, _, ref = reference(name, "per-row", 4)
        M = R.emulate_moments(*(rays[k] for k in ZC.KEYS), 4, ZC.aligned_rows(name, "per-row"), wrong=wrong)
        assert np.any(np.abs(M - ref["M"]) > ref["M_bound"]), (name, wrong)


# ------------------------------------------------------------------------------------------------------------------- C ABI
NAMES = ("tl_zfit_workspace_bytes", "tl_zfit_moments", "tl_zfit_solve", "tl_zfit_seed")


def test_entry_points_are_declared_bound_and_exported_and_the_abi_version_stays():
    hdr = open(os.path.join(ROOT, "include", "tl_trace.h")).read()
    declared = set(re.findall(r"\b(tl_[a-z0-9_]+)\s*\(", hdr))
    dll = _lib.lib()
    for name in NAMES:
        assert name in declared and name in _lib.EXPORTS and hasattr(dll, name), name
    assert dll.tl_version() == 15 == _lib.TL_ABI_VERSION
    assert int(re.search(r"#define TL_ABI_VERSION (\d+)", hdr).group(1)) == 15


def _fwd(dll, F=3, P=1000, W=3, order=4, x=ONE, y=ONE, ok=ONE, px=ONE, py=ONE, out=ONE, ws=ONE, ws_bytes=1 << 30):
    return dll.tl_zfit_moments(0, F, P, W, order, x, y, ok, W * P, 1, P, px, py, 0, 1, 0, out, ws, ws_bytes, None)


def _seed(dll, F=3, P=1000, W=3, order=4, x=ONE, y=ONE, ok=ONE, px=ONE, py=ONE, out=ONE, g=(ONE, ONE), **_):
    return dll.tl_zfit_seed(0, F, P, W, order, x, y, ok, W * P, 1, P, px, py, 0, 1, 0, out, *g, None)


BAD = [dict(x=None), dict(y=None), dict(ok=None), dict(px=None), dict(py=None), dict(out=None), dict(F=0), dict(P=0), dict(W=0),
       dict(F=-1), dict(P=-7), dict(F=1 << 16, W=1 << 15), dict(P=1 << 31), dict(order=1), dict(order=7)]


@pytest.mark.parametrize("bad", BAD, ids=lambda d: ",".join(f"{k}={'NULL' if v is None else v}" for k, v in d.items()))
def test_bad_arguments_are_refused_before_any_hip_call(bad):
    dll = _lib.lib()
    for call, name in ((_fwd, b"tl_zfit_moments"), (_seed, b"tl_zfit_seed")):
        dll.tl_unsup_loss(0, 0, 3, 100.0, ONE, None, 7.0, 0.2, ONE, ONE, ONE, ONE, None)       # another call's message first
        assert call(dll, **bad) == EINVAL, (name, bad)
        assert name + b":" in dll.tl_last_error()
    assert _seed(dll, g=(None, None)) == EINVAL and b"tl_zfit_seed" in dll.tl_last_error()


def test_the_solve_refuses_bad_arguments():
    dll = _lib.lib()
    fit = dict(rows=9, order=4, moments=ONE, g_a=None, g_q=None, a=ONE, q=ONE, valid=ONE, factor=ONE, coef=None)
    adj = dict(fit, moments=None, g_a=ONE, g_q=ONE, q=None, coef=ONE)
    call = lambda d: dll.tl_zfit_solve(0, d["rows"], d["order"], d["moments"], d["g_a"], d["g_q"], d["a"], d["q"], d["valid"],   # noqa: E731
                                       d["factor"], d["coef"], None)
    for base, keys in ((fit, ("a", "q", "valid", "factor")), (adj, ("a", "valid", "factor", "g_a", "g_q", "coef"))):
        for bad in [{k: None} for k in keys] + [dict(rows=0), dict(rows=1 << 31), dict(order=1), dict(order=7)]:
            dll.tl_unsup_loss(0, 0, 3, 100.0, ONE, None, 7.0, 0.2, ONE, ONE, ONE, ONE, None)
            assert call(dict(base, **bad)) == EINVAL, bad
            assert b"tl_zfit_solve:" in dll.tl_last_error()


def test_workspace_plan_and_a_short_workspace():
    dll = _lib.lib()
    for order in (2, 4, 6, 1, 7):
        for F, P, W in ((1, 1, 1), (2, 63, 3), (1, 4161, 2), (3, 1 << 20, 3), (65537, 2, 1), (7, 1 << 24, 1), (1, (1 << 31) - 1, 1),
                        (0, 5, 5), (5, 0, 5), (5, 5, 0), (1 << 16, 5, 1 << 15), (1, 1 << 31, 1)):
            assert dll.tl_zfit_workspace_bytes(F, P, W, order) == R.workspace_bytes(F, P, W, order), (F, P, W, order)
    need = dll.tl_zfit_workspace_bytes(3, 1 << 20, 3, 6)
    assert 0 < need < (3 * 3 << 20), "the partials stay below a byte per ray"
    assert _fwd(dll, P=1 << 20, ws=None) == EWORKSPACE
    need = dll.tl_zfit_workspace_bytes(3, 1 << 20, 3, 4)
    assert _fwd(dll, P=1 << 20, ws_bytes=need - 1) == EWORKSPACE and b"tl_zfit_moments" in dll.tl_last_error()


def test_fused_has_no_cpu_fallback_and_none_takes_the_torch_path():
    rays = ZC.rays("sub-wave", "shared")
    f32, f64 = as_torch(rays, torch.float32), as_torch(rays)
    for fn in (metrics.zernike_moments, metrics.zernike_fit):
        for t in (f32, f64):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                fn(*(t[k] for k in ZC.KEYS), fused=True)
    a, b = metrics.zernike_fit(*(f32[k] for k in ZC.KEYS)), metrics.zernike_fit(*(f32[k] for k in ZC.KEYS), fused=False)
    assert all(torch.equal(p, q) for p, q in zip(a, b)) and a.rms.dtype == torch.float32 and tuple(a.coeffs.shape) == (1, 2, 3, 14)
    assert metrics.zernike_moments(*(f32[k] for k in ZC.KEYS)).dtype == torch.float64


# -------------------------------------------------------------------------------------------------------- the oracle pin
def test_sign_and_size_agree_with_a_fit_of_the_oracles_optical_path_length():
    import torchoptics_amd as ta
    from oracle import trace_oracle as orc
    from torchoptics_amd import paraxial, prescriptions
    order, lam = 6, 587.6e-6
    lens, specs, _ = prescriptions.double_gauss(device="cpu", requires_grad=False, dtype=torch.float64)
    tr = ta.RayTracer(mode="circular", n_rays=(24, 48), rel_fields=(0., 0.707, 1.), wavelengths=("d",), double_precision=True,
                      default_device="cpu")
    a = tr.assemble(specs, lens)
    n = lens.get_refractive_indices(tr.wavelengths)
    n = torch.cat((torch.ones_like(n[:, :1, :]), n), dim=1).transpose(1, 2)
    n = n.reshape(n.shape[0], 1, 1, n.shape[1], -1)
    x, y, cx, cy, ok, _, opd = orc.trace_skew_general(a["x"], a["y"], a["z"], a["cx"], a["cy"], a["c"], a["t"], a["mu"], a["mask"],
                                                      n_index=n)
    assert ok.all() and tuple(x.shape) == (1, 3, 24 * 48, 1)
    px, py = tr.pupil_coordinates(specs, lens)
    assert tuple(px.shape) == (1, 1, 24 * 48, 1) and torch.equal(a["x"], px * specs.epd.reshape(-1, 1, 1, 1) / 2)
    scale = (specs.epd / (2 * paraxial.get_first_order(lens)[0]) / lam).reshape(-1, 1, 1)
    fit = metrics.zernike_fit(x, y, ok, px, py, max_order=order, scale=scale, fused=False)
    assert fit.valid.all()
    J = ZC.sizes(order)[0]
    p, q = px.numpy().ravel(), py.numpy().ravel()
    pp, qq = R.powers(p, order), R.powers(q, order)
    polys = [R.zernike_polynomial(j, order + 1) for j in range(1, J + 2)]                      # Z_1 (piston) .. Z_{J+1}, with constants
    Z = np.stack([sum(c[i, k] * pp[i] * qq[k] for i in range(order + 1) for k in range(order + 1 - i)) for c in polys], axis=-1)
    rows = []
    for f in range(3):
        c = fit.coeffs[0, f, 0].numpy()
        Q = 2 * c[:2] / scale.item()                                                           # the tilt terms' constant gradients
        xf, yf, cxf, cyf, w = (t[0, f, :, 0].numpy() for t in (x, y, cx, cy, opd))
        z = np.linalg.lstsq(Z, (w - ((xf - Q[0]) * cxf + (yf - Q[1]) * cyf)) / lam, rcond=None)[0][1:]      # less the piston
        rows.append((fit.rms[0, f, 0].item(), np.sqrt((z[2:] ** 2).sum()), c[2], z[2], c[9], z[9]))
        print(f"ZFIT-ACC oracle pin field {(0., 0.707, 1.)[f]:5.3f}  rms {rows[-1][0]:.4f} / {rows[-1][1]:.4f}  Z4 {c[2]:+.5f} / {z[2]:+.5f}"
              f"  Z11 {c[9]:+.5f} / {z[9]:+.5f}   (slope fit / OPD fit, waves at the d line)")
    for rms_s, rms_o, z4_s, z4_o, z11_s, z11_o in rows:
        assert z4_s * z4_o > 0 and z11_s * z11_o > 0
    rms_s, rms_o, z4_s, z4_o, z11_s, z11_o = rows[0]
    assert abs(rms_s / rms_o - 1) <= 0.05 and abs(z4_s / z4_o - 1) <= 0.05 and abs(z11_s / z11_o - 1) <= 0.05
    assert abs(rows[2][0] / rows[2][1] - 1) <= 0.15
