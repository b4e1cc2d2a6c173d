"""The through-focus MTF kernels (tfmtf_sums_kernel, tfmtf_seed_kernel, tfmtf_reduce_kernel of csrc/tl_tfmtf.hip behind
ops.TFMTFSumsFunction, metrics.otf_sums_through_focus and metrics.through_focus_mtf) against the long-double numpy definition of
tests/tfmtf_ref.py, which evaluates every plane directly, on the same fp32 inputs, element by element, on the cases of
tests/tfmtf_cases.py; the bit contract (columns, plane 0 against tl_mtf_sums, repeatability); layouts; the analytic pins; then
through the tracer, without a host synchronisation, from a HIP graph and under the fresh-memory harness.

Bounds: derived in tfmtf_ref.py.  The lines "TFMTF-ACC ..." (largest error / bound per case, the tracer test's figures) are kept in
profiles/tfmtf_accuracy.txt."""
import functools

import numpy as np
import pytest
import torch

import tfmtf_cases as TC
import tfmtf_ref as R
from conftest import rel_l2
from test_tfmtf_cpu import _pin_tol, check_pins

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRADS = ("gx", "gy", "gcx", "gcy")


@pytest.fixture(scope="module")
def ta():
    import torchoptics_amd
    from torchoptics_amd import _lib
    _lib.lib()
    return torchoptics_amd


@functools.lru_cache(maxsize=None)
def _reference(name):
    """The case's arrays, origin, frequency vectors, planes, seeds and long-double references, computed once and left unchanged."""
    rays = TC.rays(name)
    nu = R.vectors(TC.frequencies_of(name), TC.DIRECTIONS)
    o, planes = TC.given_centre(name), TC.planes_of(name)
    g = TC.seeds(name, len(nu[0]), planes[2])
    ref = R.sums(*(rays[k] for k in TC.KEYS), rays["ok"], o, *nu, planes)
    return rays, nu, o, planes, g, ref, R.seeds(ref, g)


def _node(t, leaves, o, nu, planes, ok_dtype=torch.bool):
    from torchoptics_amd import ops
    return ops.TFMTFSumsFunction.apply(*leaves, t["ok"].to(ok_dtype), o, tuple(nu[0]), tuple(nu[1]), *planes)


def _run(rays, name, o, nu, planes, g, need=(True,) * 4, ok_dtype=torch.bool):
    """dict sums (float64), gx, gy, gcx, gcy (float32 or None) of the node on the case placed in its layout."""
    t = TC.place(rays, name, DEV)
    leaves = [t[k].detach().requires_grad_(n) for k, n in zip(TC.KEYS, need)]
    sums = _node(t, leaves, torch.from_numpy(np.ascontiguousarray(o)).to(DEV), nu, planes, ok_dtype)
    assert sums.dtype == torch.float64 and sums.is_cuda and tuple(sums.shape) == g.shape
    if any(need):
        (sums * torch.from_numpy(g).to(DEV)).sum().backward()
    return dict(sums=sums.detach().cpu().numpy(), **{k: None if q.grad is None else q.grad.cpu().numpy() for k, q in zip(GRADS, leaves)})


def _worst(got, ref, bound):
    return float((np.abs(got.astype(np.float64) - ref) / np.maximum(bound, 1e-300)).max())


def _same(a, b):
    return all((a[k] is None and b[k] is None) or a[k].tobytes() == b[k].tobytes() for k in a)


@pytest.mark.parametrize("name", TC.CASES)
def test_sums_and_seeds_against_the_definition(ta, name):
    rays, nu, o, planes, g, ref, want = _reference(name)
    got = _run(rays, name, o, nu, planes, g)
    worst = dict(sums=_worst(got["sums"], ref["sums"], ref["bound"]), **{k: _worst(got[k], want[k], want[k + "_bound"]) for k in GRADS})
    print(f"TFMTF-ACC case {name:14s} rows x rays {ref['n'].size:6d} x {ref['P']:5d}  J {len(nu[0]):2d} Z {planes[2]:2d}  err/bound  "
          + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert np.all(np.abs(got["sums"] - ref["sums"]) <= ref["bound"]), worst["sums"]
    live = ref["terms"].live
    for k in GRADS:
        assert got[k].dtype == np.float32 and np.all(np.abs(got[k].astype(np.float64) - want[k]) <= want[k + "_bound"]), (k, worst[k])
        assert np.all(got[k][~live] == 0)                                                          # a dead ray gets exact zeros
    empty = ref["n"] == 0
    assert np.all(got["sums"][empty] == 0)                                                         # empty rows: exact zeros
    if name == "dead-row":
        assert empty[0, 0, 0] and ref["n"][0, 0, 1] == 1
    still = got["sums"][:, :, :, [j for j in range(len(nu[0])) if nu[0][j] == 0 and nu[1][j] == 0]]
    assert np.all(still[..., 0] == ref["n"][..., None, None]) and np.all(still[..., 1] == 0)       # nu = 0: C = n, S = 0 at every plane
    if name == "poisoned":
        assert (rays["ok"] & ~live).sum() > 5                                                      # ok-true rays without a direction
        twin = _run(rays["clean"], name, o, nu, planes, g)                                         # the dead rays zeroed: no bit changes
        assert _same(got, twin) and all(np.isfinite(v).all() for v in got.values())


@pytest.mark.parametrize("name", ("block-edge", "multi-partial", "layout-slice"))
def test_same_bits_twice_for_either_ok_dtype_and_for_gradients_asked_alone_or_in_pairs(ta, name):
    rays, nu, o, planes, g, ref, _ = _reference(name)
    args = (rays, name, o, nu, planes, g)
    first = _run(*args)
    assert _same(first, _run(*args)) and _same(first, _run(*args, ok_dtype=torch.uint8))
    for need in ((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (1, 0, 1, 0), (0, 1, 0, 1), (0, 0, 1, 1)):
        some = _run(*args, need=tuple(bool(n) for n in need))
        assert some["sums"].tobytes() == first["sums"].tobytes()
        for k, n in zip(GRADS, need):
            assert (some[k] is None) if not n else some[k].tobytes() == first[k].tobytes(), (need, k)


def test_every_column_has_the_bits_it_has_alone_whatever_the_call_holds(ta):
    """Bit contract (i).  Column (j, z) computed with J = 1, Z = z + 1 has the bits it has in calls of J in {1, 2, 3, 4, 5, 8, 9, 16}
    and Z in {1, 2, 3, 4, 5, 8, 9, 16}: every register bucket JB x ZB (powers of two, JB ZB <= 32) full and one past it, one launch
    and several.  The chunking of metrics.otf_sums_through_focus at 17 and 33 planes and 17 vectors is the concatenation of its
    chunks' own calls."""
    from torchoptics_amd import metrics
    name = "block-edge"
    rays = TC.rays(name)
    t = TC.place(rays, name, DEV)
    leaves = [t[k] for k in TC.KEYS]
    o = torch.from_numpy(TC.given_centre(name)).to(DEV)
    nu = R.vectors(tuple(2.5 * k for k in range(1, 18)), (20.0,))                                  # 17 oblique vectors
    first, step = -0.11, 0.027
    alone = {(j, z): _node(t, leaves, o, (nu[0][j:j + 1], nu[1][j:j + 1]), (first, step, z + 1))[:, :, :, 0, z]
             for j in range(16) for z in range(16)}
    whole = torch.stack([torch.stack([alone[j, z] for z in range(16)], dim=3) for j in range(16)], dim=3)      # [1,3,2,16,16,2]
    for J in (1, 2, 3, 4, 5, 8, 9, 16):
        for Z in (1, 2, 3, 4, 5, 8, 9, 16):
            got = _node(t, leaves, o, (nu[0][:J], nu[1][:J]), (first, step, Z))
            assert tuple(got.shape) == (1, 3, 2, J, Z, 2) and torch.equal(got, whole[:, :, :, :J, :Z]), (J, Z)
    got = _node(t, leaves, o, (nu[0][3:8], nu[1][3:8]), (first, step, 7))                          # other neighbours, the same columns
    assert torch.equal(got, whole[:, :, :, 3:8, :7])
    ref = R.sums(*(rays[k] for k in TC.KEYS), rays["ok"], TC.given_centre(name), nu[0][:16], nu[1][:16], (first, step, 16))
    assert _worst(whole.cpu().numpy(), ref["sums"], ref["bound"]) <= 1
    args = (*leaves, t["ok"], o)
    for Z in (17, 33):
        got = metrics.otf_sums_through_focus(*args, tuple(nu[0][:3]), tuple(nu[1][:3]), (first, step, Z), fused=True)
        parts = [_node(t, leaves, o, (nu[0][:3], nu[1][:3]), (first + z0 * step, step, min(16, Z - z0))) for z0 in range(0, Z, 16)]
        assert tuple(got.shape) == (1, 3, 2, 3, Z, 2) and torch.equal(got, torch.cat(parts, dim=4))
    got = metrics.otf_sums_through_focus(*args, tuple(nu[0]), tuple(nu[1]), (first, step, 3), fused=True)
    parts = [_node(t, leaves, o, (nu[0][s], nu[1][s]), (first, step, 3)) for s in (slice(0, 16), slice(16, 17))]
    assert tuple(got.shape) == (1, 3, 2, 17, 3, 2) and torch.equal(got, torch.cat(parts, dim=3))
    ref = R.sums(*(rays[k] for k in TC.KEYS), rays["ok"], TC.given_centre(name), nu[0][:3], nu[1][:3], (first, step, 33))
    got = metrics.otf_sums_through_focus(*args, tuple(nu[0][:3]), tuple(nu[1][:3]), (first, step, 33), fused=True)
    assert _worst(got.cpu().numpy(), ref["sums"], ref["bound"]) <= 1


@pytest.mark.parametrize("name", ("block-edge", "multi-partial", "layout-slice", "lens-batch"))
def test_plane_0_at_shift_0_has_the_bits_of_tl_mtf_sums(ta, name):
    """Bit contract (ii), where no ok-live ray fails the direction rule: the same x, y, ok and origin."""
    from torchoptics_amd import ops
    rays, nu, o, _, _, ref, _ = _reference(name)
    assert np.array_equal(ref["terms"].live, rays["ok"])
    t = TC.place(rays, name, DEV)
    o = torch.from_numpy(o).to(DEV)
    want = ops.MTFSumsFunction.apply(t["x"], t["y"], t["ok"], o, tuple(nu[0]), tuple(nu[1]))
    for planes in ((0.0, 2.0 ** -5, 16), (0.0, 0.013, 5), (0.0, 1.0, 1)):
        got = _node(t, [t[k] for k in TC.KEYS], o, nu, planes)
        assert torch.equal(got[:, :, :, :, 0], want), planes


def test_layouts_are_read_in_place_or_copied(ta):
    """The tracer's view, the interior slice, the dense tensor and lens-batch reach the kernels as they are (their storage is what
    the node saves); the expanded cx of "layout-expand" is copied.  "layout-slice" (bases 4 bytes off) and "layout-dense" (ray
    stride W) take the one-ray path, another order of the sums than the 16-byte path the same fan takes in the tracer's
    layout: both agree with the definition inside the bounds."""
    from torchoptics_amd import ops
    seen, got = {}, {}
    nu = R.vectors(TC.FREQUENCIES, TC.DIRECTIONS)

    def run(name, layout):
        t = TC.place(TC.rays(name), layout, DEV)
        leaves = [t[k].detach().requires_grad_(True) for k in TC.KEYS]
        o = torch.from_numpy(TC.given_centre(name)).to(DEV)
        out = ops.TFMTFSumsFunction.apply(*leaves, t["ok"], o, tuple(nu[0]), tuple(nu[1]), *TC.PLANES)
        same = [s.data_ptr() == q.data_ptr() for s, q in zip(out.grad_fn.saved_tensors, (*(t[k] for k in TC.KEYS), t["ok"], o))]
        if layout == "layout-slice":
            assert leaves[0].data_ptr() % 16 == 4
        out.sum().backward()
        return same, dict(sums=out.detach().cpu().numpy(), **{k: q.grad.cpu().numpy() for k, q in zip(GRADS, leaves)})
    for name in ("layout-tracer", "layout-slice", "layout-expand", "layout-dense", "lens-batch"):
        seen[name], got[name] = run(name, name)
    for name in ("layout-tracer", "layout-slice", "layout-dense", "lens-batch"):
        assert seen[name] == [True] * 6, name
    assert seen["layout-expand"] == [True, True, False, True, True, True]
    for name in ("layout-slice", "layout-dense"):
        rays = TC.rays(name)
        ref = R.sums(*(rays[k] for k in TC.KEYS), rays["ok"], TC.given_centre(name), *nu, TC.PLANES)
        want = R.seeds(ref, np.ones(ref["sums"].shape))
        for res in (got[name], run(name, "layout-tracer")[1]):
            assert _worst(res["sums"], ref["sums"], ref["bound"]) <= 1, name
            assert all(_worst(res[k], want[k], want[k + "_bound"]) <= 1 for k in GRADS), name


def test_the_analytic_pins_on_the_device(ta):
    from torchoptics_amd import metrics

    def mtf_of(r, frequencies, planes, directions):
        t = {k: torch.from_numpy(v).to(DEV) for k, v in r.items()}
        out = metrics.through_focus_mtf(*(t[k] for k in TC.KEYS), t["ok"], frequencies, planes, directions, fused=True)
        assert out.mtf.dtype == torch.float32
        return out.mtf.double().cpu().numpy(), out
    check_pins(mtf_of, lambda *a: _pin_tol(*a) + 2.0 ** -24)                                     # the float32 rounding of a value <= 1
    rays = TC.rays("dead-row")
    t = TC.place(rays, "dead-row", DEV)
    leaves = [t[k].detach().requires_grad_(True) for k in TC.KEYS]
    out = metrics.through_focus_mtf(*leaves, t["ok"], TC.FREQUENCIES, TC.PLANES, common=(), fused=True)
    assert (out.mtf[..., 0][out.n > 0] == 1).all() and out.n[0, 0, 0] == 0 and (out.mtf[0, 0, 0] == 0).all()
    out.mtf[0, 0, 0].sum().backward()
    assert all((q.grad == 0).all() for q in leaves)


# ------------------------------------------------------------------------------------------------------- through the tracer
T_NU = (0.0, 20.0, 40.0)
T_PLANES = (-0.15, 0.02, 16)


def _cooke(ta, double=False):
    import yaml_free_lenses as L
    lens, specs, leaves = L.build("cooke", DEV)
    tr = ta.RayTracer(mode="circular", n_rays=(32, 32), rel_fields=(0., 0.707, 1.), wavelengths=("C", "d", "F"),
                      double_precision=double, default_device=DEV)
    out = tr.trace_rays(specs, lens)
    return (out[0], out[1], out[2], out[3], out[4]), leaves


def test_through_the_tracer(ta):
    from torchoptics_amd import metrics
    (x, y, cx, cy, ok), _ = _cooke(ta)
    assert tuple(x.shape) == (1, 3, 1024, 3) and x.dtype == cx.dtype == torch.float32
    # (a) fused against unfused: float64 arithmetic on the same inputs, another summation order: 2 ulp of fp32
    for common, centre, weights in ((("wavelength",), "field", None), ((), "row", None), ((), "field", (0.5, 1.0, 0.25)),
                                    (("wavelength",), "field", (0.5, 1.0, 0.25))):
        kw = dict(common=common, centre=centre, weights=weights)
        fu, un, de = (metrics.through_focus_mtf(x, y, cx, cy, ok, T_NU, T_PLANES, fused=f, **kw) for f in (True, False, None))
        for k, a, b, c in zip(fu._fields, fu, un, de):
            assert a.dtype == (torch.float64 if k == "shifts" else torch.float32) and torch.equal(a, c)
            ulps = ((a.double() - b.double()).abs() / (b.double().abs() * 2.0 ** -23).clamp(min=1e-45)).max().item()
            print(f"TFMTF-ACC tracer (a) common={','.join(common) or '-':10s} centre={centre:5s} weights={'given' if weights else 'none':5s} {k:6s} "
                  f"fused vs unfused {ulps:.2f} ulp")
            assert ulps <= 2.0, (common, centre, k)
    # (b) against geometric_mtf(fused=False) on rays shifted in float64, plane by plane, about the same origin: fp32 rounding of the
    # result plus the bounds of the sums
    out = metrics.through_focus_mtf(x, y, cx, cy, ok, T_NU, T_PLANES, fused=True)
    xs, ys, cxs, cys, live = (q.detach().cpu().numpy() for q in (x, y, cx, cy, ok))
    nu = R.vectors(T_NU, TC.DIRECTIONS)
    ref = R.sums(xs, ys, cxs, cys, live, out.centre.double().cpu().numpy(), *nu, T_PLANES)
    n = np.maximum(ref["n"].sum(axis=2), 1)[..., None, None]
    tol = np.moveaxis((2.0 ** -24 + ref["bound"].sum(axis=(2, -1)) / n + 8 * R.U).reshape(1, 3, 2, 3, 16), -1, -3)
    x64, y64, cx64, cy64 = (q.detach().double() for q in (x, y, cx, cy))
    cz = torch.sqrt(1 - cx64 * cx64 - cy64 * cy64)
    worst = 0.0
    for z, d in enumerate(metrics.plane_shifts(T_PLANES)):
        at = metrics.geometric_mtf(x64 + d * cx64 / cz, y64 + d * cy64 / cz, ok, T_NU, centre=out.centre.double()[:, :, :1], fused=False)
        diff = (out.mtf[:, :, z].double() - at.mtf).abs().detach().cpu().numpy()
        # the shifted coordinate rounds once in float64 (2^-53 of millimetres): a phase of 2 pi 40 2^-53 16 per ray, far below tol
        assert np.all(diff <= tol[:, :, z] + 1e-12), (z, float((diff / tol[:, :, z]).max()))
        worst = max(worst, float((diff / tol[:, :, z]).max()))
    print(f"TFMTF-ACC tracer (b) fused vs geometric_mtf(fused=False) on float64-shifted rays, 16 planes: err/tol {worst:.3f}; "
          f"MTF at 40 cycles / mm on axis {out.mtf[0, 0, :, 0, 2].min().item():.3f} .. {out.mtf[0, 0, :, 0, 2].max().item():.3f}")
    # (c) leaf gradients of the mean MTF against the float64 twin
    grads = {}
    for tag, double, fused in (("fused", False, True), ("unfused", False, False), ("twin", True, False)):
        rays, lv = _cooke(ta, double=double)
        metrics.through_focus_mtf(*rays, T_NU, T_PLANES, fused=fused).mtf.mean().backward()
        grads[tag] = {k: lv[k].grad.double().cpu().numpy() for k in ("c", "t")}
    for k in ("c", "t"):
        e_f, e_u = rel_l2(grads["fused"][k], grads["twin"][k]), rel_l2(grads["unfused"][k], grads["twin"][k])
        print(f"TFMTF-ACC tracer (c) d mtf.mean() / d{k}: fused {e_f:.3e}  unfused {e_u:.3e}  ratio {e_f / max(e_u, 1e-300):.3f}")
        assert e_f <= 2 * e_u + 1e-6, (k, e_f, e_u)


# ------------------------------------------------------------------------------------- no synchronisation, graph, fresh memory
def _step_case(common, centre):
    """A step in the sense of tests/step_cases.py: the through-focus MTF of "block-edge" and its gradients, two input sets."""
    import step_cases
    from torchoptics_amd import metrics
    rays = TC.rays("block-edge")                                 # F = 3, W = 2, P = 257
    rng = np.random.default_rng(709)
    A = {k: step_cases._tracer_layout(rays[k].transpose(0, 1, 3, 2)) for k in TC.KEYS}
    B = {k: step_cases._tracer_layout((rays[k] + (1e-3 if k in "xy" else 1e-4) * rng.standard_normal(rays[k].shape)).transpose(0, 1, 3, 2))
         for k in TC.KEYS}
    ok = step_cases._tracer_layout(rays["ok"].transpose(0, 1, 3, 2)).to(torch.bool).to(DEV)
    given = torch.from_numpy(TC.given_centre("block-edge")[:, :, :1]).to(DEV)
    weights = (0.75, 1.25)

    def body(L):
        out = metrics.through_focus_mtf(L["x"], L["y"], L["cx"], L["cy"], ok, TC.FREQUENCIES, TC.PLANES, common=common,
                                        centre=given if centre == "given" else centre, weights=weights, fused=True)
        shift, peak, _ = metrics.mtf_best_focus(out.mtf, out.shifts)
        (out.mtf.mean() + peak.mean()).backward()
        return out.mtf, out.centre, shift
    return step_cases.Case(DEV, {"A": A, "B": B}, body, ("mtf", "centre", "best"), TC.KEYS)


@pytest.mark.parametrize("common,centre", ((("wavelength",), "field"), ((), "row"), (("wavelength",), "given")))
def test_a_warm_step_is_sync_free_and_replays_its_eager_bits_from_a_graph(ta, common, centre):
    """One stream, no parallel branches.  The sync check comes first: a step that synchronises is never captured."""
    from torchoptics_amd import graphs
    eager = {}
    for which in "AB":
        case = _step_case(common, centre)
        case.load(which)
        eager[which] = [t.clone() for t in case.step()]
    torch.cuda.synchronize()
    differ = {what for what, a, b in zip(case.names, eager["A"], eager["B"]) if not torch.equal(a, b)}
    assert differ == set(case.names) - ({"centre"} if centre == "given" else set())        # (a given centre is the same for both)
    case = _step_case(common, centre)
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
    case = _step_case(common, centre)                            # fresh leaves: no AccumulateGrad node of another stream
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


@pytest.mark.parametrize("name", ("block-edge", "dead-row", "layout-slice"))
def test_the_same_bytes_whatever_the_buffers_held(ta, name):
    from test_gpu_fresh_memory import hold
    rays, nu, o, planes, g, _, _ = _reference(name)
    hold("tfmtf", name, lambda: _run(rays, name, o, nu, planes, g))
