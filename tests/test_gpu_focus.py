"""The focus kernels (focus_moments_kernel / focus_reduce_kernel, focus_seed_kernel of csrc/tl_focus.hip behind
ops.FocusMomentsFunction, metrics.focus_moments and metrics.through_focus) against the float64 numpy definition of
tests/focus_ref.py on the same fp32 inputs, element by element, on the cases of tests/focus_cases.py; then through the tracer.

Bounds (derived in focus_ref.py, U = 2^-53): moments |M_k - ref| <= (P + 8) U sum|terms|; seeds |g - ref| <= 2^-24 |ref| +
16 U sum|its terms| + 2^-149.  The lines "FOCUS-ACC ..." (largest error / bound per case, the tracer test's errors and ratios)
are kept in profiles/focus_accuracy.txt."""
import functools

import numpy as np
import pytest
import torch

import focus_cases as FC
import focus_ref as R
from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("x", "y", "cx", "cy")


@pytest.fixture(scope="module")
def ta():
    import torchoptics_amd
    from torchoptics_amd import _lib
    _lib.lib()
    return torchoptics_amd


@functools.lru_cache(maxsize=None)
def _reference(name):
    """The case's arrays, seeds and float64 references, computed once and left unchanged."""
    rays = FC.rays(name)
    a = tuple(rays[k] for k in KEYS + ("ok",))
    g = FC.g_moments(name)
    with np.errstate(invalid="ignore", over="ignore"):
        M, T = R.moments(*a)
        seeds, mags = R.seeds(*a, g)
    return rays, g, M, T, seeds, mags


def _run(rays, name, g, need=(True,) * 4, ok_dtype=torch.bool):
    """(M, grads) of the kernels on the case placed in its layout: M [B,F,W,11] and the four per-ray gradients (or None) as
    float64 / float32 numpy."""
    from torchoptics_amd import metrics
    t = FC.place({k: rays[k] for k in KEYS + ("ok",)}, name, DEV)
    leaves = [t[k].detach().requires_grad_(n) for k, n in zip(KEYS, need)]
    M = metrics.focus_moments(*leaves, t["ok"].to(ok_dtype), fused=True)
    assert M.dtype == torch.float64 and M.is_cuda
    (M * torch.from_numpy(g).to(DEV)).sum().backward()
    return M.detach().cpu().numpy(), [None if q.grad is None else q.grad.cpu().numpy() for q in leaves]


@pytest.mark.parametrize("name", FC.CASES)
def test_moments_and_seeds_against_the_definition(ta, name):
    rays, g, Mr, T, seeds, mags = _reference(name)
    P = rays["x"].shape[2]
    M, grads = _run(rays, name, g)
    bound = R.moment_bound(T, P)
    worst = float((np.abs(M - Mr) / np.maximum(bound, 1e-300)).max())
    worst_g = max(float((np.abs(q.astype(np.float64) - s) / R.seed_bound(s, m)).max()) for q, s, m in zip(grads, seeds, mags))
    print(f"FOCUS-ACC case {name:14s} rows x rays {Mr.size // 11:6d} x {P:5d}  moments err/bound {worst:.3f}  seeds err/bound {worst_g:.3f}")
    assert np.all(np.abs(M - Mr) <= bound), worst
    for q, s, m, k in zip(grads, seeds, mags, KEYS):
        assert q.dtype == np.float32 and np.all(np.abs(q.astype(np.float64) - s) <= R.seed_bound(s, m)), (k, worst_g)
    live = R.live_rays(rays["cx"], rays["cy"], rays["ok"])
    assert all(np.all(q[~live] == 0) for q in grads)                        # a dead ray gets exact zeros
    dead_rows = Mr[..., 0] == 0
    assert np.all(M[dead_rows] == 0) and np.array_equal(M[..., 0], Mr[..., 0])
    if name == "dead-row":
        assert dead_rows[0, 0, 0] and Mr[0, 0, 1, 0] == 1
    if name == "poisoned":
        Mc, gc = _run(rays["clean"], name, g)                               # the dead rays zeroed: no bit changes
        assert M.tobytes() == Mc.tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(grads, gc))
        assert np.isfinite(M).all() and all(np.isfinite(q).all() for q in grads)


@pytest.mark.parametrize("name", ("block-edge", "multi-partial", "layout-slice"))
def test_same_bits_twice_for_either_ok_dtype_and_for_a_gradient_asked_alone(ta, name):
    rays, g, *_ = _reference(name)
    M, grads = _run(rays, name, g)
    M2, grads2 = _run(rays, name, g)
    M8, grads8 = _run(rays, name, g, ok_dtype=torch.uint8)
    for Mo, go in ((M2, grads2), (M8, grads8)):
        assert M.tobytes() == Mo.tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(grads, go))
    for i in range(4):
        need = tuple(j == i for j in range(4))
        Mi, gi = _run(rays, name, g, need=need)
        assert Mi.tobytes() == M.tobytes() and gi[i].tobytes() == grads[i].tobytes()
        assert all(gi[j] is None for j in range(4) if j != i)


def test_layouts_are_read_in_place_or_copied(ta):
    """The tracer's view and the interior slice reach the kernels as they are (their storage is what the node saves); the
    expanded cx is copied."""
    from torchoptics_amd import ops
    seen = {}
    for name in ("layout-tracer", "layout-slice", "layout-expand", "layout-dense", "lens-batch"):
        t = FC.place({k: v for k, v in FC.rays(name).items() if k != "clean"}, name, DEV)
        x = t["x"].detach().requires_grad_(True)
        M = ops.FocusMomentsFunction.apply(x, t["y"], t["cx"], t["cy"], t["ok"])
        saved = M.grad_fn.saved_tensors
        seen[name] = [s.data_ptr() == t[k].data_ptr() for s, k in zip(saved, KEYS + ("ok",))]
        if name == "layout-slice":
            assert x.data_ptr() % 16 == 4
    assert seen["layout-tracer"] == [True] * 5 and seen["layout-slice"] == [True] * 5 and seen["layout-dense"] == [True] * 5
    assert seen["layout-expand"] == [True, True, False, True, True] and seen["lens-batch"] == [True] * 5


# ------------------------------------------------------------------------------------------------------- through the tracer
def _cooke(ta, double=False, shift=None):
    import yaml_free_lenses as L
    from torchoptics_amd import lens_modeling as lm
    lens, specs, leaves = L.build("cooke", DEV)
    if shift is not None:
        t = leaves["t"].detach().clone()
        t[-1] += shift
        lens = lm.Lens(lens.structure, leaves["c"], t, leaves["nd"], leaves["v"])
    tr = ta.RayTracer(mode="circular", n_rays=(32, 32), rel_fields=(0., 0.707, 1.), wavelengths=("C", "d", "F"),
                      double_precision=double, default_device=DEV)
    return tr.trace_rays(specs, lens)[:5], leaves


def test_through_the_tracer(ta):
    from torchoptics_amd import metrics
    (x, y, cx, cy, ok), leaves = _cooke(ta)
    assert tuple(x.shape) == (1, 3, 1024, 3) and x.dtype == torch.float32
    # (a) fused against unfused: the same float64 finish on moments that agree to ~1e-13: 2 ulp of fp32
    for common in (("wavelength",), (), ("field", "wavelength")):
        fu = metrics.through_focus(x, y, cx, cy, ok, common=common, fused=True)
        un = metrics.through_focus(x, y, cx, cy, ok, common=common, fused=False)
        de = metrics.through_focus(x, y, cx, cy, ok, common=common)
        for k, a, b, c in zip(fu._fields, fu, un, de):
            assert a.dtype == torch.float32 and torch.equal(a, c)
            ulps = ((a.double() - b.double()).abs() / (b.double().abs() * 2.0 ** -23).clamp(min=1e-45)).max().item()
            print(f"FOCUS-ACC tracer (a) common={','.join(common) or '-':17s} {k:10s} fused vs unfused {ulps:.2f} ulp")
            assert ulps <= 2.0, (common, k)
    # (b) the plane moved to the common best focus: the traced spot there is rms_best
    tf = metrics.through_focus(x, y, cx, cy, ok, common=("field", "wavelength"), fused=True)
    bf, rms_best = tf.best_focus.item(), tf.rms_best.item()
    at = {}
    for step in (-0.01, 0.0, 0.01):
        rays, _ = _cooke(ta, shift=bf + step)
        xs, ys, cxs, cys, oks = (q.detach().cpu().numpy() for q in rays)
        at[step] = R.rms_shifted(xs, ys, cxs, cys, oks, 0.0, ("field", "wavelength")).item()
    print(f"FOCUS-ACC tracer (b) best_focus {bf:+.6f} mm  rms_best {rms_best:.6f}  traced there {at[0.0]:.6f}  "
          f"at -0.01 {at[-0.01]:.6f}  at +0.01 {at[0.01]:.6f}  (rms at the nominal plane {tf.rms.item():.6f})")
    assert abs(at[0.0] - rms_best) <= 2e-5 and at[-0.01] > at[0.0] < at[0.01]
    # (c) leaf gradients of rms_best.mean() against the float64 twin
    grads = {}
    for tag, double, fused in (("fused", False, True), ("unfused", False, False), ("twin", True, False)):
        rays, lv = _cooke(ta, double=double)
        metrics.through_focus(*rays, fused=fused).rms_best.mean().backward()
        grads[tag] = {k: lv[k].grad.double().cpu().numpy() for k in ("c", "t")}
    for k in ("c", "t"):
        e_f, e_u = rel_l2(grads["fused"][k], grads["twin"][k]), rel_l2(grads["unfused"][k], grads["twin"][k])
        print(f"FOCUS-ACC tracer (c) d rms_best.mean() / d{k}: fused {e_f:.3e}  unfused {e_u:.3e}  ratio {e_f / max(e_u, 1e-300):.3f}")
        assert e_f <= 2 * e_u + 1e-6, (k, e_f, e_u)
