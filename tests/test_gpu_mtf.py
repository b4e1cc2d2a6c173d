"""The MTF kernels (mtf_sums_kernel, mtf_seed_kernel, mtf_reduce_kernel of csrc/tl_mtf.hip behind ops.MTFSumsFunction,
metrics.otf_sums and metrics.geometric_mtf) against the long-double numpy definition of tests/mtf_ref.py on the same fp32 inputs,
element by element, on the cases of tests/mtf_cases.py; bit checks that need no reference; the analytic pins; then through the
tracer, without a host synchronisation, from a HIP graph and under the fresh-memory harness.

Bounds (derived in mtf_ref.py, U = 2^-53): per live term b = 2 pi 4 U (|nu_x dx| + |nu_y dy|) + 4 U, a sum sum_live b + (P + 8) U
sum|terms|; seeds 2^-24 |ref| + 25 U sum_j |2 pi nu_j q_j| (1 + 2 pi (|nu_x dx| + |nu_y dy|)) + 2^-149.  The lines "MTF-ACC ..."
(largest error / bound per case, the tracer test's figures) are kept in profiles/mtf_accuracy.txt."""
import functools

import numpy as np
import pytest
import torch

import mtf_cases as MC
import mtf_ref as R
from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ta():
    import torchoptics_amd
    from torchoptics_amd import _lib
    _lib.lib()
    return torchoptics_amd


@functools.lru_cache(maxsize=None)
def _reference(name, frequencies=None, directions=MC.DIRECTIONS):
    """The case's arrays, origin, frequency vectors, seeds and long-double references, computed once and left unchanged."""
    rays = MC.rays(name)
    nu = R.vectors(frequencies or MC.frequencies_of(name), directions)
    o = MC.given_centre(name)
    g = MC.seeds(name, len(nu[0]))
    with np.errstate(invalid="ignore", over="ignore"):
        ref = R.otf_sums(rays["x"], rays["y"], rays["ok"], o, *nu)
        want = R.seeds(ref, g)
    return rays, nu, o, g, ref, want


def _node(t, x, y, o, nu, ok_dtype=torch.bool):
    """sums [B,F,W,J,2] of the node, the frequency vectors in calls of at most MTF_MAX_J as metrics.otf_sums makes them."""
    from torchoptics_amd import ops
    parts = [ops.MTFSumsFunction.apply(x, y, t["ok"].to(ok_dtype), o, tuple(nu[0][j:j + ops.MTF_MAX_J]), tuple(nu[1][j:j + ops.MTF_MAX_J]))
             for j in range(0, len(nu[0]), ops.MTF_MAX_J)]
    return torch.cat(parts, dim=3)


def _run(rays, name, o, nu, g, need=(True, True), ok_dtype=torch.bool):
    """dict sums (float64), gx, gy (float32 or None) of the node on the case placed in its layout."""
    t = MC.place(rays, name, DEV)
    x, y = (t[k].detach().requires_grad_(n) for k, n in zip("xy", need))
    sums = _node(t, x, y, torch.from_numpy(np.ascontiguousarray(o)).to(DEV), nu, ok_dtype)
    assert sums.dtype == torch.float64 and sums.is_cuda and tuple(sums.shape) == g.shape
    if any(need):
        (sums * torch.from_numpy(g).to(DEV)).sum().backward()
    grad = lambda q: None if q.grad is None else q.grad.cpu().numpy()          # noqa: E731
    return dict(sums=sums.detach().cpu().numpy(), gx=grad(x), gy=grad(y))


def _worst(got, ref, bound):
    return float((np.abs(got.astype(np.float64) - ref) / np.maximum(bound, 1e-300)).max())


def _same(a, b):
    return all((a[k] is None and b[k] is None) or a[k].tobytes() == b[k].tobytes() for k in a)


@pytest.mark.parametrize("name", MC.CASES)
def test_sums_and_seeds_against_the_definition(ta, name):
    rays, nu, o, g, ref, want = _reference(name)
    got = _run(rays, name, o, nu, g)
    worst = dict(sums=_worst(got["sums"], ref["sums"], ref["bound"]), **{k: _worst(got[k], want[k], want[k + "_bound"]) for k in ("gx", "gy")})
    print(f"MTF-ACC case {name:14s} rows x rays {ref['n'].size:6d} x {ref['P']:5d}  J {len(nu[0]):2d}  err/bound  "
          + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert np.all(np.abs(got["sums"] - ref["sums"]) <= ref["bound"]), worst["sums"]
    for k in ("gx", "gy"):
        assert got[k].dtype == np.float32 and np.all(np.abs(got[k].astype(np.float64) - want[k]) <= want[k + "_bound"]), (k, worst[k])
        assert np.all(got[k][~rays["ok"]] == 0)                                                    # a dead ray gets exact zeros
    empty = ref["n"] == 0
    assert np.all(got["sums"][empty] == 0)                                                         # empty rows: exact zeros
    if name == "dead-row":
        assert empty[0, 0, 0] and ref["n"][0, 0, 1] == 1
    if nu[0][0] == 0 and nu[1][0] == 0:                                                            # nu = 0: C = n, S = 0, no rounding
        assert np.array_equal(got["sums"][..., 0, 0], ref["n"]) and np.all(got["sums"][..., 0, 1] == 0)
    if name == "poisoned":
        twin = _run(rays["clean"], name, o, nu, g)                                                 # the dead rays zeroed: no bit changes
        assert _same(got, twin) and all(np.isfinite(v).all() for v in got.values())


@pytest.mark.parametrize("name", ("block-edge", "multi-partial", "layout-slice"))
def test_same_bits_twice_for_either_ok_dtype_and_for_a_gradient_asked_alone(ta, name):
    rays, nu, o, g, ref, _ = _reference(name)
    args = (rays, name, o, nu, g)
    first = _run(*args)
    assert _same(first, _run(*args)) and _same(first, _run(*args, ok_dtype=torch.uint8))
    for j in (0, 16):                                                                              # both directions' nu = 0 columns
        assert np.array_equal(first["sums"][..., j, 0], ref["n"]) and np.all(first["sums"][..., j, 1] == 0)
    for i, k in enumerate(("gx", "gy")):
        alone = _run(*args, need=tuple(j == i for j in range(2)))
        assert alone["sums"].tobytes() == first["sums"].tobytes() and alone[k].tobytes() == first[k].tobytes()
        assert alone["gy" if k == "gx" else "gx"] is None


def test_j_buckets_and_chunking_keep_every_column_s_bits(ta):
    """J = 1, 4, 5, 8, 9, 16: each register bucket full and one past it; K D = 17, 33 go through the chunking of
    metrics.otf_sums.  Every column has the bits it has when it is computed alone."""
    from torchoptics_amd import metrics
    name = "block-edge"
    rays = MC.rays(name)
    t = MC.place(rays, name, DEV)
    o = torch.from_numpy(MC.given_centre(name)).to(DEV)
    freqs = tuple(2.5 * k for k in range(17))
    nu = R.vectors(freqs, (20.0, "tangential"))                                                    # 34 vectors, the first 17 oblique
    alone = [_node(t, t["x"], t["y"], o, (nu[0][j:j + 1], nu[1][j:j + 1])) for j in range(34)]
    for J in (1, 4, 5, 8, 9, 16):
        got = _node(t, t["x"], t["y"], o, (nu[0][3:3 + J], nu[1][3:3 + J]))
        assert tuple(got.shape) == (1, 3, 2, J, 2)
        for j in range(J):
            assert torch.equal(got[:, :, :, j], alone[3 + j][:, :, :, 0]), (J, j)
    ref = R.otf_sums(rays["x"], rays["y"], rays["ok"], MC.given_centre(name), *nu)
    assert _worst(torch.cat(alone, dim=3).cpu().numpy(), ref["sums"], ref["bound"]) <= 1
    for D, dirs in ((1, (20.0,)), (2, (20.0, "tangential"))):                                      # K D = 17 and 34 >= 33: 2 and 3 launches
        x, y = (t[k].detach().requires_grad_(True) for k in "xy")
        out = metrics.geometric_mtf(x, y, t["ok"], freqs, dirs, common=(), centre=o, fused=True)
        n, want = R.finish(ref["sums_ld"][..., :17 * D, :], ref["n"], None, False)
        assert tuple(out.mtf.shape) == (1, 3, 2, D, 17) and out.mtf.dtype == torch.float32 and np.array_equal(out.n.cpu().numpy(), n)
        # the float32 rounding of a modulus of sums that are inside their bounds, over n
        tol = 2.0 ** -24 + ref["bound"][..., :17 * D, :].sum(axis=-1) / np.maximum(n, 1)[..., None] + 8 * R.U
        assert np.all(np.abs(out.mtf.detach().cpu().numpy().reshape(want.shape).astype(np.float64) - want) <= tol)
        sums = metrics.otf_sums(x, y, t["ok"], o, tuple(nu[0][:17 * D]), tuple(nu[1][:17 * D]), fused=True)
        assert torch.equal(sums, torch.cat(alone[:17 * D], dim=3))
        out.mtf[..., -1].sum().backward()                                                          # the last chunk reaches the rays
        assert torch.isfinite(x.grad).all() and (y.grad != 0).any() and (x.grad[~t["ok"]] == 0).all()


def test_layouts_are_read_in_place_or_copied(ta):
    """The tracer's view, the interior slice, the dense tensor and a contiguous origin reach the kernels as they are (their
    storage is what the node saves); expanded flags and an origin expanded over the wavelengths are copied (the C ABI takes a
    contiguous [F, W, 2] origin).  Against the same fan in the tracer's contiguous layout (16-byte loads on every row):
    "layout-expand", whose copied flags land in that layout, takes the same load path and has the same bits; "layout-slice" (bases
    4 bytes off) and "layout-dense" (ray stride W) take the one-ray path, another order of the sums, and agree inside the bounds."""
    from torchoptics_amd import ops
    seen, got = {}, {}
    nu = R.vectors(MC.FREQUENCIES[:8], MC.DIRECTIONS)

    def run(name, layout):
        t = MC.place(MC.rays(name), layout, DEV)
        x, y = (t[k].detach().requires_grad_(True) for k in "xy")
        o = torch.from_numpy(MC.given_centre(name)).to(DEV)
        out = ops.MTFSumsFunction.apply(x, y, t["ok"], o, tuple(nu[0]), tuple(nu[1]))
        same = [s.data_ptr() == q.data_ptr() for s, q in zip(out.grad_fn.saved_tensors, (t["x"], t["y"], t["ok"], o))]
        if layout == "layout-slice":
            assert x.data_ptr() % 16 == 4
        out.sum().backward()
        return same, dict(sums=out.detach().cpu().numpy(), gx=x.grad.cpu().numpy(), gy=y.grad.cpu().numpy())
    for name in ("layout-tracer", "layout-slice", "layout-expand", "layout-dense", "lens-batch"):
        seen[name], got[name] = run(name, name)
    assert seen["layout-tracer"] == [True] * 4 and seen["layout-slice"] == [True] * 4 and seen["layout-dense"] == [True] * 4
    assert seen["layout-expand"] == [True, True, False, True] and seen["lens-batch"] == [True] * 4
    assert _same(got["layout-expand"], run("layout-expand", "layout-tracer")[1])                   # the same load path: the same bits
    for name in ("layout-slice", "layout-dense"):                                                  # the other load path: the bounds
        rays = MC.rays(name)
        ref = R.otf_sums(rays["x"], rays["y"], rays["ok"], MC.given_centre(name), *nu)
        want = R.seeds(ref, np.ones(ref["sums"].shape))
        for res in (got[name], run(name, "layout-tracer")[1]):
            assert _worst(res["sums"], ref["sums"], ref["bound"]) <= 1, name
            assert all(_worst(res[k], want[k], want[k + "_bound"]) <= 1 for k in ("gx", "gy")), name
    t = MC.place(MC.rays("layout-tracer"), "layout-tracer", DEV)
    o = torch.from_numpy(MC.given_centre("layout-tracer")[:, :, :1]).to(DEV)
    wide = ops.MTFSumsFunction.apply(t["x"].requires_grad_(True), t["y"], t["ok"], o.expand(1, 3, 3, 2), tuple(nu[0]), tuple(nu[1]))
    assert wide.grad_fn.saved_tensors[3].data_ptr() != o.data_ptr() and wide.grad_fn.saved_tensors[3].is_contiguous()
    assert torch.equal(wide, ops.MTFSumsFunction.apply(t["x"], t["y"], t["ok"], o.expand(1, 3, 3, 2).contiguous(), tuple(nu[0]), tuple(nu[1])))


def test_the_analytic_pins_on_the_device(ta):
    """Two rays, the comb, one ray, nu = 0 and an empty row with fp32 inputs on the kernels: to the bounds."""
    from torchoptics_amd import metrics
    nu = (0.0, 10.0, 33.0, 50.0, 75.0, 125.0)

    def mtf(r, frequencies, directions=MC.DIRECTIONS, **kw):
        t = {k: torch.from_numpy(v).to(DEV) for k, v in r.items()}
        out = metrics.geometric_mtf(t["x"], t["y"], t["ok"], frequencies, directions, fused=True, **kw)
        ref = R.otf_sums(r["x"], r["y"], r["ok"], out.centre.double().cpu().numpy(), *R.vectors(frequencies, directions))
        n = np.maximum(ref["n"].sum(axis=2), 1)[..., None]
        tol = 2.0 ** -24 + ref["bound"].sum(axis=(2, -1)) / n + 8 * R.U                             # pooled sums inside their bounds; fp32
        return out.mtf.double().cpu().numpy(), tol.reshape(out.mtf.shape)
    r, a = MC.two_rays()
    got, tol = mtf(r, nu)
    assert np.all(np.abs(got[0, 0, 0] - np.abs(np.cos(2 * np.pi * np.asarray(nu) * a))) <= tol[0, 0, 0]) and np.all(got[0, 0, 1] == 1)
    got, tol = mtf(MC.comb(), nu + (1024.0, 16.0))
    assert np.all(np.abs(got[0, 0, 0] - MC.dirichlet(nu + (1024.0, 16.0))) <= tol[0, 0, 0]) and np.all(got[0, 0, 1] == 1)
    one = {k: v[:, :, :1] for k, v in MC.comb().items()}
    assert np.all(mtf(one, nu, ("tangential", "sagittal", 30.0))[0] == 1)                          # the origin IS the ray: every phase is 0
    rays = MC.rays("dead-row")
    t = MC.place(rays, "dead-row", DEV)
    x, y = (t[k].detach().requires_grad_(True) for k in "xy")
    out = metrics.geometric_mtf(x, y, t["ok"], nu, common=(), fused=True)
    assert (out.mtf[..., 0][out.n > 0] == 1).all() and out.n[0, 0, 0] == 0 and (out.mtf[0, 0, 0] == 0).all()
    out.mtf[0, 0, 0].sum().backward()
    assert (x.grad == 0).all() and (y.grad == 0).all()
    half = dict(x=np.zeros((1, 1, 2, 1), np.float32), y=np.array([3.0, 3.0 + 2.0 ** -5], np.float32).reshape(1, 1, 2, 1), ok=np.ones((1, 1, 2, 1), bool))
    t = {k: torch.from_numpy(v).to(DEV) for k, v in half.items()}
    x, y = (t[k].requires_grad_(True) for k in "xy")
    out = metrics.geometric_mtf(x, y, t["ok"], (16.0,), ("tangential",), fused=True)               # half a period apart: modulus exactly 0
    assert out.mtf.item() == 0.0
    out.mtf.sum().backward()
    assert (x.grad == 0).all() and (y.grad == 0).all()


# ------------------------------------------------------------------------------------------------------- through the tracer
T_NU = (0.0, 5.0, 10.0, 20.0, 30.0, 40.0, 50.0, 60.0)


def _cooke(ta, double=False):
    import yaml_free_lenses as L
    lens, specs, leaves = L.build("cooke", DEV)
    tr = ta.RayTracer(mode="circular", n_rays=(32, 32), rel_fields=(0., 0.707, 1.), wavelengths=("C", "d", "F"),
                      double_precision=double, default_device=DEV)
    out = tr.trace_rays(specs, lens)
    return (out[0], out[1], out[4]), leaves


def test_through_the_tracer(ta):
    from torchoptics_amd import metrics
    (x, y, ok), _ = _cooke(ta)
    assert tuple(x.shape) == (1, 3, 1024, 3) and x.dtype == torch.float32
    # (a) fused against unfused: float64 arithmetic on the same inputs, another summation order: 2 ulp of fp32
    for common, centre, weights in ((("wavelength",), "field", None), ((), "row", None), ((), "field", (0.5, 1.0, 0.25)),
                                    (("wavelength",), "field", (0.5, 1.0, 0.25))):
        kw = dict(common=common, centre=centre, weights=weights)
        fu, un, de = (metrics.geometric_mtf(x, y, ok, T_NU, fused=f, **kw) for f in (True, False, None))
        for k, a, b, c in zip(fu._fields, fu, un, de):
            assert a.dtype == torch.float32 and torch.equal(a, c)
            ulps = ((a.double() - b.double()).abs() / (b.double().abs() * 2.0 ** -23).clamp(min=1e-45)).max().item()
            print(f"MTF-ACC tracer (a) common={','.join(common) or '-':10s} centre={centre:5s} weights={'given' if weights else 'none':5s} {k:6s} "
                  f"fused vs unfused {ulps:.2f} ulp")
            assert ulps <= 2.0, (common, centre, k)
    # (b) the moment bracket on the traced spots, per row, at the two lowest frequencies above 0
    out = metrics.geometric_mtf(x, y, ok, (1.0, 2.5), common=(), centre="row", fused=True).mtf.detach().double().cpu().numpy()
    xs, ys, live = (q.detach().cpu().numpy() for q in (x, y, ok))
    n = np.maximum(live.sum(axis=2), 1)
    for d, q in ((0, ys), (1, xs)):
        mean = np.where(live, q.astype(np.float64), 0).sum(axis=2) / n
        for k, nu in enumerate((1.0, 2.5)):
            lo, hi = MC.bracket(2 * np.pi * nu * (q - mean[:, :, None]), live)
            print(f"MTF-ACC tracer (b) {'TS'[d]} nu {nu:3.1f}: bracket widths <= {(hi - lo).max():.2e}, MTF {out[..., d, k].min():.4f} .. {out[..., d, k].max():.4f}")
            assert np.all(lo - 2.0 ** -23 <= out[..., d, k]) and np.all(out[..., d, k] <= hi + 2.0 ** -23), (d, nu)
    # (c) leaf gradients of the mean MTF against the float64 twin
    grads = {}
    for tag, double, fused in (("fused", False, True), ("unfused", False, False), ("twin", True, False)):
        (xx, yy, kk), lv = _cooke(ta, double=double)
        metrics.geometric_mtf(xx, yy, kk, T_NU, fused=fused).mtf.mean().backward()
        grads[tag] = {k: lv[k].grad.double().cpu().numpy() for k in ("c", "t")}
    for k in ("c", "t"):
        e_f, e_u = rel_l2(grads["fused"][k], grads["twin"][k]), rel_l2(grads["unfused"][k], grads["twin"][k])
        print(f"MTF-ACC tracer (c) d mtf.mean() / d{k}: fused {e_f:.3e}  unfused {e_u:.3e}  ratio {e_f / max(e_u, 1e-300):.3f}")
        assert e_f <= 2 * e_u + 1e-6, (k, e_f, e_u)


# ------------------------------------------------------------------------------------- no synchronisation, graph, fresh memory
def _step_case(common, centre):
    """A step in the sense of tests/step_cases.py: the MTF of "block-edge" at 32 vectors and its gradients, two input sets."""
    import step_cases
    from torchoptics_amd import metrics
    rays = MC.rays("block-edge")                                 # F = 3, W = 2, P = 257
    rng = np.random.default_rng(707)
    A = {k: step_cases._tracer_layout(rays[k].transpose(0, 1, 3, 2)) for k in "xy"}
    B = {k: step_cases._tracer_layout((rays[k] + 1e-3 * rng.standard_normal(rays[k].shape)).transpose(0, 1, 3, 2)) for k in "xy"}
    ok = step_cases._tracer_layout(rays["ok"].transpose(0, 1, 3, 2)).to(torch.bool).to(DEV)
    given = torch.from_numpy(MC.given_centre("block-edge")[:, :, :1]).to(DEV)
    weights = (0.75, 1.25)

    def body(L):
        out = metrics.geometric_mtf(L["x"], L["y"], ok, MC.FREQUENCIES, common=common, centre=given if centre == "given" else centre,
                                    weights=weights, fused=True)
        out.mtf.mean().backward()
        return out.mtf, out.centre
    return step_cases.Case(DEV, {"A": A, "B": B}, body, ("mtf", "centre"), ("x", "y"))


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
    rays, nu, o, g, _, _ = _reference(name)
    hold("mtf", name, lambda: _run(rays, name, o, nu, g))
