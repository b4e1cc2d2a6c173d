"""The Zernike-fit kernels (zfit_moments_kernel, zfit_reduce_kernel, zfit_factor_kernel, zfit_adjoint_kernel, zfit_seed_kernel of
csrc/tl_zfit.hip behind ops.ZernikeFitFunction, metrics.zernike_fit and metrics.zernike_moments) against the float64 numpy
definition of tests/zfit_ref.py (lstsq on the design matrix) on the same fp32 inputs, element by element, on the cases of
tests/zfit_cases.py; bit checks that need no reference; then through the tracer, without a host synchronisation, from a HIP
graph and under the fresh-memory harness.

Bounds (derived in zfit_ref.py, U = 2^-53): moments (P + 8) U sum|terms|; coefficients and q from the moment bounds through the
normal equations and the scaled system's condition number; seeds 2^-24 |ref| + the coefficients' share + 64 U sum|monomial terms|
+ 2^-149.  The lines "ZFIT-ACC ..." (largest error / bound per case, the tracer test's figures) are kept in
profiles/zfit_accuracy.txt."""
import numpy as np
import pytest
import torch

import zfit_cases as ZC
from test_gpu_enclosed import _cooke, _same, _worst
from test_zfit_cpu import BAND, COMBOS, reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ta():
    import torchoptics_amd
    from torchoptics_amd import _lib
    _lib.lib()
    return torchoptics_amd


def _run(rays, name, order, g_a, g_q, need=(True, True), ok_dtype=torch.bool):
    """dict M, a, q (float64), valid (uint8), gx, gy (float32 or None) of the node on the case placed in its layout."""
    from torchoptics_amd import ops
    t = ZC.place(rays, name, DEV)
    x, y = (t[k].detach().requires_grad_(n) for k, n in zip("xy", need))
    px, py = (t[k].expand_as(x) for k in ("px", "py"))
    M, a, q, valid = ops.ZernikeFitFunction.apply(x, y, t["ok"].to(ok_dtype), px, py, order)
    J, K = ZC.sizes(order)
    assert M.dtype == a.dtype == q.dtype == torch.float64 and valid.dtype == torch.uint8 and a.is_cuda
    assert tuple(M.shape) == tuple(q.shape) + (K,) and tuple(a.shape) == tuple(q.shape) + (J,) and not M.requires_grad
    if any(need):
        ((a * torch.from_numpy(g_a).to(DEV)).sum() + (q * torch.from_numpy(g_q).to(DEV)).sum()).backward()
    grad = lambda v: None if v.grad is None else v.grad.cpu().numpy()                              # noqa: E731
    return dict(M=M.cpu().numpy(), a=a.detach().cpu().numpy(), q=q.detach().cpu().numpy(), valid=valid.cpu().numpy(), gx=grad(x),
                gy=grad(y))


@pytest.mark.parametrize("name,pupil,order", COMBOS, ids=lambda v: str(v))
def test_moments_fit_and_seeds_against_the_definition(ta, name, pupil, order):
    rays, g_a, g_q, ref = reference(name, pupil, order)
    got = _run(rays, name, order, g_a, g_q)
    valid = got["valid"] != 0
    compare = (ref["pivot"] < BAND[0]) | (ref["pivot"] > BAND[1])
    assert compare.all() and np.array_equal(valid, ref["valid"])
    assert np.array_equal(got["M"][..., 0], ref["n"])                                              # the count is exact
    worst = {k: _worst(got[k], ref[k], ref[k + "_bound"]) for k in ("M", "a", "q", "gx", "gy")}
    print(f"ZFIT-ACC case {name:14s} pupil {pupil:7s} order {order} rows x rays {ref['n'].size:6d} x {ref['P']:5d} valid {int(valid.sum()):6d}"
          "  err/bound  " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    for k in ("M", "a", "q"):
        assert np.all(np.abs(got[k] - ref[k]) <= ref[k + "_bound"]), (k, worst[k])
    for k in ("gx", "gy"):
        assert got[k].dtype == np.float32 and np.all(np.abs(got[k].astype(np.float64) - ref[k]) <= ref[k + "_bound"]), (k, worst[k])
        assert np.all(got[k][~np.broadcast_to(rays["ok"], got[k].shape)] == 0)                     # a dead ray gets exact zeros
        assert np.all(got[k][np.broadcast_to(~valid[:, :, None, :], got[k].shape)] == 0)           # and so does an invalid row
    assert np.all(got["a"][~valid] == 0) and np.all(got["q"][~valid] == 0)
    if name == "dead-row":
        assert ref["n"][0, 0].tolist() == [0, 1] and not valid[0, 0].any() and valid[0, 1].all()
    if name in ("one-ray", "many-rows-b"):
        assert not valid.any()
    if name == "poisoned":
        twin = _run(rays["clean"], name, order, g_a, g_q)                                          # the dead rays zeroed: no bit changes
        assert _same(got, twin) and all(np.isfinite(v).all() for v in got.values())


@pytest.mark.parametrize("pupil", ZC.PUPILS)
@pytest.mark.parametrize("name", ("block-edge", "multi-partial", "layout-slice"))
def test_same_bits_twice_for_either_ok_dtype_and_for_a_gradient_asked_alone(ta, name, pupil):
    for order in (4, 6):
        rays = ZC.rays(name, pupil)
        g_a, g_q = ZC.seeds(name, order)
        first = _run(rays, name, order, g_a, g_q)
        assert _same(first, _run(rays, name, order, g_a, g_q)) and _same(first, _run(rays, name, order, g_a, g_q, ok_dtype=torch.uint8))
        for i, k in enumerate(("gx", "gy")):
            alone = _run(rays, name, order, g_a, g_q, need=tuple(j == i for j in range(2)))
            assert alone["a"].tobytes() == first["a"].tobytes() and alone[k].tobytes() == first[k].tobytes()
            assert alone["gy" if k == "gx" else "gx"] is None


def test_layouts_are_read_in_place_and_a_shared_pupil_is_not_copied(ta):
    from torchoptics_amd import ops
    for name, pupil in (("block-edge", "shared"), ("layout-slice", "per-row"), ("layout-dense", "per-row"), ("lens-batch", "shared")):
        t = ZC.place(ZC.rays(name, pupil), name, DEV)
        x = t["x"].detach().requires_grad_(True)
        _, a, _, _ = ops.ZernikeFitFunction.apply(x, t["y"], t["ok"], t["px"].expand_as(x), t["py"].expand_as(x), 4)
        saved = a.grad_fn.saved_tensors
        assert [s.data_ptr() == t[k].data_ptr() for s, k in zip(saved, ZC.KEYS)] == [True] * 5, (name, pupil)
        if pupil == "shared":
            assert saved[3].untyped_storage().nbytes() == 4 * x.shape[2]                          # P floats: expanded, not copied
            assert all(st == (d == 2) for d, (st, n) in enumerate(zip(saved[3].stride(), x.shape)) if n > 1)


def test_through_the_tracer(ta):
    """Fused against fused=False on the Cooke triplet, values and leaf gradients (the float64 twin is the yardstick)."""
    from conftest import rel_l2
    from torchoptics_amd import metrics
    import yaml_free_lenses as L

    def tracer(double):
        return ta.RayTracer(mode="circular", n_rays=(32, 32), rel_fields=(0., 0.707, 1.), wavelengths=("C", "d", "F"),
                            double_precision=double, default_device=DEV)
    (x, y, ok), _ = _cooke(ta)
    lens, specs, _ = L.build("cooke", DEV)
    px, py = tracer(False).pupil_coordinates(specs, lens)
    assert tuple(px.shape) == (1, 1, 1024, 1) and px.dtype == torch.float32 and px.abs().max() < 1
    scale = 1.0 / 587.6e-6
    for order in (4, 6):
        fu = metrics.zernike_fit(x, y, ok, px, py, order, scale, fused=True)
        un = metrics.zernike_fit(x, y, ok, px, py, order, scale, fused=False)
        de = metrics.zernike_fit(x, y, ok, px, py, order, scale)
        assert fu.valid.all() and torch.equal(fu.valid, un.valid)
        for k, a, b, c in zip(fu._fields, fu, un, de):
            assert torch.equal(a, c) and (a.dtype == torch.float32 or k == "valid")
            if k in ("n", "valid"):
                assert torch.equal(a, b)
                continue
            # both are float64 evaluations on the same inputs rounded to fp32 at the end: 4 ulp of fp32, the coefficients in
            # units of the row's largest one (a small coefficient carries the absolute error of the solve, not its own ulp).
            # The residual is the root of q = S - b . a, S = sum (x^2 + y^2): each evaluation of q is within (P + 8 + 4 J) U S
            # of the exact one (the sums' bound and the J products), and d residual = d q / (2 n residual)
            top = b.double().abs().amax(dim=-1, keepdim=True) if k == "coeffs" else b.double().abs()
            tol = 4 * 2.0 ** -23 * top
            if k == "residual":
                M = metrics.zernike_moments(x, y, ok, px, py, order, fused=True)
                S, J = M[..., -2] + M[..., -1], ZC.sizes(order)[0]
                tol = tol + 2 * (x.shape[2] + 8 + 4 * J) * 2.0 ** -53 * S / (2 * M[..., 0] * b.double())
            err = ((a.double() - b.double()).abs() / tol.clamp(min=1e-300)).max().item()
            print(f"ZFIT-ACC tracer order {order} {k:9s} fused vs unfused: {err:.3f} of the tolerance")
            assert err <= 1.0, (order, k)
    grads = {}
    for tag, double, fused in (("fused", False, True), ("unfused", False, False), ("twin", True, False)):
        (xx, yy, kk), lv = _cooke(ta, double=double)
        metrics.zernike_fit(xx, yy, kk, px, py, 4, scale, fused=fused).rms_focus.mean().backward()
        grads[tag] = {k: lv[k].grad.double().cpu().numpy() for k in ("c", "t")}
    for k in ("c", "t"):
        e_f, e_u = rel_l2(grads["fused"][k], grads["twin"][k]), rel_l2(grads["unfused"][k], grads["twin"][k])
        print(f"ZFIT-ACC tracer d rms_focus.mean() / d{k}: fused {e_f:.3e}  unfused {e_u:.3e}  ratio {e_f / max(e_u, 1e-300):.3f}")
        assert e_f <= 2 * e_u + 1e-6, (k, e_f, e_u)


# ------------------------------------------------------------------------------------- no synchronisation, graph, fresh memory
def _step_case(order, pupil):
    """A step in the sense of tests/step_cases.py: the mean rms_focus and residual of "block-edge" and their gradients."""
    import step_cases
    from torchoptics_amd import metrics
    rays = ZC.rays("block-edge", pupil)                          # F = 3, W = 2, P = 257
    rng = np.random.default_rng(707)
    A = {k: step_cases._tracer_layout(rays[k].transpose(0, 1, 3, 2)) for k in "xy"}
    B = {k: step_cases._tracer_layout((rays[k] + 1e-3 * rng.standard_normal(rays[k].shape)).transpose(0, 1, 3, 2)) for k in "xy"}
    ok = step_cases._tracer_layout(rays["ok"].transpose(0, 1, 3, 2)).to(torch.bool).to(DEV)
    px, py = (torch.from_numpy(rays[k]).to(DEV) for k in ("px", "py"))

    def body(L):
        fit = metrics.zernike_fit(L["x"], L["y"], ok, px, py, order, 1700.0, fused=True)
        (fit.rms_focus.mean() + fit.residual.mean()).backward()
        return fit.coeffs, fit.rms_focus, fit.residual
    return step_cases.Case(DEV, {"A": A, "B": B}, body, ("coeffs", "rms_focus", "residual"), ("x", "y"))


@pytest.mark.parametrize("order,pupil", ((4, "shared"), (6, "per-row")))
def test_a_warm_step_is_sync_free_and_replays_its_eager_bits_from_a_graph(ta, order, pupil):
    """One stream, no parallel branches.  The sync check comes first: a step that synchronises is never captured."""
    from torchoptics_amd import graphs
    eager = {}
    for which in "AB":
        case = _step_case(order, pupil)
        case.load(which)
        eager[which] = [t.clone() for t in case.step()]
    torch.cuda.synchronize()
    assert not any(torch.equal(a, b) for a, b in zip(eager["A"], eager["B"]))
    case = _step_case(order, pupil)
    case.step()
    case.step()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = [t.clone() for t in case.step()]
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(got, eager["A"]))
    case = _step_case(order, pupil)                              # fresh leaves: no AccumulateGrad node of another stream
    graph, out = graphs.capture_step(case.step, DEV, warmup=3)

    def replayed():
        graph.replay()
        torch.cuda.synchronize()
        return [t.clone() for t in out]
    for t in out:
        t.zero_()
    for which in ("A", "B", "A"):
        case.load(which)
        got = replayed()
        for what, a, b in zip(case.names, got, eager[which]):
            assert torch.equal(a, b), f"{what} replayed on input set {which} does not have the eager bits"


@pytest.mark.parametrize("name,pupil,order", (("block-edge", "shared", 4), ("dead-row", "per-row", 4), ("layout-slice", "per-row", 6)))
def test_the_same_bytes_whatever_the_buffers_held(ta, name, pupil, order):
    from test_gpu_fresh_memory import hold
    rays = ZC.rays(name, pupil)
    g_a, g_q = ZC.seeds(name, order)
    hold("zfit", f"{name}-{pupil}-{order}", lambda: _run(rays, name, order, g_a, g_q))
