"""The enclosed-energy kernels (enclosed_centroid_kernel, enclosed_sums_kernel, enclosed_seed_kernel, enclosed_reduce_kernel of
csrc/tl_enclosed.hip behind ops.EnclosedEnergyFunction, metrics.enclosed_energy and metrics.spot_centroid) against the float64
numpy definition of tests/enclosed_ref.py on the same fp32 inputs, element by element, on the cases of tests/enclosed_cases.py;
bit checks that need no reference; then through the tracer, without a host synchronisation, from a HIP graph and under the
fresh-memory harness.

Bounds (derived in enclosed_ref.py, U = 2^-53): S and sums (P + 8) U sum|terms| plus, for the sums, the per-term part that
carries the amplification (R_k + rho_i) / tau_k; seeds 2^-24 |ref| + c U sum|its terms| + 2^-149.  The lines "ENCLOSED-ACC ..."
(largest error / bound per case, the tracer test's figures) are kept in profiles/enclosed_accuracy.txt."""
import functools

import numpy as np
import pytest
import torch

import enclosed_cases as EC
import enclosed_ref as R
from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CENTRES = ("row", "field", "given")


@pytest.fixture(scope="module")
def ta():
    import torchoptics_amd
    from torchoptics_amd import _lib
    _lib.lib()
    return torchoptics_amd


def _inv(soft, K):
    return tuple(1.0 / s for s in (soft if isinstance(soft, tuple) else (soft,) * K))


@functools.lru_cache(maxsize=None)
def _reference(name, shape, centre, radii=None, soft=EC.SOFT):
    """The case's arrays, seeds and float64 references, computed once and left unchanged."""
    rays = EC.rays(name)
    radii = radii or EC.radii_of(name)
    c = EC.given_centre(name) if centre == "given" else centre
    g_sums, g_S = EC.seeds(name, len(radii))
    with np.errstate(invalid="ignore", over="ignore"):
        ref = R.enclosed_sums(rays["x"], rays["y"], rays["ok"], radii, soft, shape, c)
        want = R.seeds(ref, g_sums, g_S, c)
    return rays, radii, c, g_sums, g_S, ref, want


def _run(rays, name, shape, centre, radii, soft, g_sums, g_S, need=(True, True), ok_dtype=torch.bool, want_centre=True):
    """dict S, sums (float64), gx, gy (float32 or None), gc (float64 or None) of the node on the case placed in its layout."""
    from torchoptics_amd import ops
    t = EC.place(rays, name, DEV)
    x, y = (t[k].detach().requires_grad_(n) for k, n in zip("xy", need))
    c = centre if isinstance(centre, str) else torch.from_numpy(np.ascontiguousarray(centre)).to(DEV).requires_grad_(want_centre)
    S, sums = ops.EnclosedEnergyFunction.apply(x, y, t["ok"].to(ok_dtype), c, tuple(radii), _inv(soft, len(radii)), shape)
    assert S.dtype == sums.dtype == torch.float64 and sums.is_cuda and tuple(sums.shape) == tuple(S.shape[:3]) + (len(radii),)
    if any(need) or (torch.is_tensor(c) and want_centre):
        ((sums * torch.from_numpy(g_sums).to(DEV)).sum() + (S * torch.from_numpy(g_S).to(DEV)).sum()).backward()
    grad = lambda q: None if not torch.is_tensor(q) or q.grad is None else q.grad.cpu().numpy()          # noqa: E731
    return dict(S=S.detach().cpu().numpy(), sums=sums.detach().cpu().numpy(), gx=grad(x), gy=grad(y), gc=grad(c))


def _worst(got, ref, bound):
    return float((np.abs(got.astype(np.float64) - ref) / np.maximum(bound, 1e-300)).max())


def _same(a, b):
    return all((a[k] is None and b[k] is None) or a[k].tobytes() == b[k].tobytes() for k in a)


@pytest.mark.parametrize("shape", EC.SHAPE_NAMES)
@pytest.mark.parametrize("name", EC.CASES)
def test_sums_and_seeds_against_the_definition(ta, name, shape):
    for centre in CENTRES:
        rays, radii, c, g_sums, g_S, ref, want = _reference(name, shape, centre)
        P = ref["P"]
        got = _run(rays, name, shape, c, radii, EC.SOFT, g_sums, g_S)
        worst = {k: _worst(got[k], ref[k], ref[k + "_bound"]) for k in ("S", "sums")}
        worst.update({k: _worst(got[k], want[k], want[k + "_bound"]) for k in ("gx", "gy") + (("gc",) if centre == "given" else ())})
        print(f"ENCLOSED-ACC case {name:14s} {shape:6s} centre {centre:5s} rows x rays {ref['S'].size // 3:6d} x {P:5d}  err/bound  "
              + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
        assert np.array_equal(got["S"][..., 0], ref["S"][..., 0])                                  # the count is exact
        for k in ("S", "sums"):
            assert np.all(np.abs(got[k] - ref[k]) <= ref[k + "_bound"]), (centre, k, worst[k])
        for k in ("gx", "gy"):
            assert got[k].dtype == np.float32 and np.all(np.abs(got[k].astype(np.float64) - want[k]) <= want[k + "_bound"]), (centre, k, worst[k])
            assert np.all(got[k][~rays["ok"]] == 0)                                                # a dead ray gets exact zeros
        if centre == "given":
            assert got["gc"].dtype == np.float64 and np.all(np.abs(got["gc"] - want["gc"]) <= want["gc_bound"]), worst["gc"]
        else:
            assert got["gc"] is None
        empty = ref["S"][..., 0] == 0
        assert np.all(got["S"][empty] == 0) and np.all(got["sums"][empty] == 0)                    # empty rows: exact zeros
        if centre == "given":
            assert np.all(got["gc"][empty] == 0)
        if name == "dead-row":
            assert empty[0, 0, 0] and ref["S"][0, 0, 1, 0] == 1
        if name == "poisoned":
            twin = _run(rays["clean"], name, shape, c, radii, EC.SOFT, g_sums, g_S)                # the dead rays zeroed: no bit changes
            assert _same(got, twin) and all(np.isfinite(v).all() for v in got.values() if v is not None)


@pytest.mark.parametrize("shape", EC.SHAPE_NAMES)
@pytest.mark.parametrize("name", ("sub-wave", "block-edge", "multi-partial", "dead-row", "lens-batch", "layout-slice"))
def test_bits_that_need_no_reference(ta, name, shape):
    rays, radii, c, g_sums, g_S, ref, _ = _reference(name, shape, "given")
    # (1) softness 1e-12: no ray lies in a band (the reference's terms are all exactly 0 or 1), so every sum is the integer count
    _, _, _, _, _, hard, _ = _reference(name, shape, "given", soft=1e-12)
    assert np.all((hard["terms"].e == 0) | (hard["terms"].e == 1))
    got = _run(rays, name, shape, c, radii, 1e-12, g_sums, g_S, need=(False, False), want_centre=False)
    assert np.array_equal(got["sums"], hard["sums"]) and np.array_equal(got["sums"], np.round(got["sums"]))
    # (2) where R_K exceeds every rho of a row by the softness, the last sum IS n; (3) sums do not decrease with k
    got = _run(rays, name, shape, c, radii, EC.SOFT, g_sums, g_S, need=(False, False), want_centre=False)
    full = np.all((ref["terms"].e[..., -1] == 1) | ~ref["terms"].live, axis=2)
    assert full.any() and np.array_equal(got["sums"][..., -1][full], got["S"][..., 0][full])
    assert np.all(np.diff(got["sums"], axis=-1) >= 0)
    # (4) the fan turned by 90 degrees about the centre, the centre turned along: the circle's sums keep their bits
    if shape == "circle":
        turned = dict(x=-rays["y"], y=rays["x"], ok=rays["ok"])
        rot = _run(turned, name, shape, np.stack([-c[..., 1], c[..., 0]], axis=-1), radii, EC.SOFT, g_sums, g_S, need=(False, False),
                   want_centre=False)
        assert rot["sums"].tobytes() == got["sums"].tobytes() and np.array_equal(rot["S"][..., 0], got["S"][..., 0])


@pytest.mark.parametrize("centre", CENTRES)
@pytest.mark.parametrize("name", ("block-edge", "multi-partial", "layout-slice"))
def test_same_bits_twice_for_either_ok_dtype_and_for_a_gradient_asked_alone(ta, name, centre):
    for shape in EC.SHAPE_NAMES:
        rays, radii, c, g_sums, g_S, _, _ = _reference(name, shape, centre)
        args = (rays, name, shape, c, radii, EC.SOFT, g_sums, g_S)
        first = _run(*args)
        assert _same(first, _run(*args)) and _same(first, _run(*args, ok_dtype=torch.uint8))
        for i, k in enumerate(("gx", "gy")):
            alone = _run(*args, need=tuple(j == i for j in range(2)), want_centre=False)
            assert alone["sums"].tobytes() == first["sums"].tobytes() and alone[k].tobytes() == first[k].tobytes()
            assert alone["gy" if k == "gx" else "gx"] is None and alone["gc"] is None
        if centre == "given":
            alone = _run(*args, need=(False, False))
            assert alone["gc"].tobytes() == first["gc"].tobytes() and alone["gx"] is None and alone["gy"] is None


@pytest.mark.parametrize("shape", EC.SHAPE_NAMES)
def test_k_buckets_chunking_and_a_softness_per_radius(ta, shape):
    """K = 1, 8, 9, 32: one, a full, the next and the largest register bucket; 33 goes through the Python chunking."""
    from torchoptics_amd import metrics
    name = "block-edge"
    for K in (1, 8, 9, 32):
        radii = tuple(0.002 * k for k in range(1, K + 1)) if K > 1 else (0.03,)
        soft = tuple(0.002 + 0.0002 * k for k in range(K)) if K == 9 else EC.SOFT
        for centre in ("row", "given"):
            rays, radii, c, g_sums, g_S, ref, want = _reference(name, shape, centre, radii, soft)
            got = _run(rays, name, shape, c, radii, soft, g_sums, g_S)
            worst = {k: _worst(got[k], r[k], r[k + "_bound"]) for k, r in (("sums", ref), ("gx", want), ("gy", want))}
            print(f"ENCLOSED-ACC K {K:2d} {shape:6s} centre {centre:5s} softness {'per radius' if K == 9 else 'one':10s} err/bound  "
                  + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
            assert all(v <= 1 for v in worst.values()), (K, centre, worst)
    radii = tuple(0.001 * k for k in range(1, 34))                              # the 33rd, 0.033 mm, has rays in its band
    rays, radii, _, _, _, ref, _ = _reference(name, shape, "row", radii)
    t = EC.place(rays, name, DEV)
    x, y = (t[k].detach().requires_grad_(True) for k in "xy")
    out = metrics.enclosed_energy(x, y, t["ok"], radii, EC.SOFT, shape=shape, common=(), fused=True)
    n, E = R.energy(ref["S"], ref["sums"], ())
    assert tuple(out.energy.shape) == E.shape and out.energy.dtype == torch.float32 and np.array_equal(out.n.cpu().numpy(), n)
    # the float32 rounding of a quotient of sums that are inside their bounds: 2^-24 of a value <= 1 and the bound over n
    tol = 2.0 ** -24 + ref["sums_bound"] / np.maximum(n, 1)[..., None]
    assert np.all(np.abs(out.energy.detach().cpu().numpy().astype(np.float64) - E) <= tol)
    whole = metrics.enclosed_energy(x, y, t["ok"], radii[:32], EC.SOFT, shape=shape, common=(), fused=True)
    assert torch.equal(whole.energy, out.energy[..., :32])
    out.energy[..., 32:].sum().backward()                                        # the second chunk reaches the rays
    assert torch.isfinite(x.grad).all() and (x.grad != 0).any() and (x.grad[~t["ok"]] == 0).all()
    assert ((ref["terms"].e[..., 32] > 0) & (ref["terms"].e[..., 32] < 1)).any()               # (rays in the 33rd band exist)


def test_layouts_are_read_in_place_or_copied(ta):
    """The tracer's view and the interior slice reach the kernels as they are (their storage is what the node saves); the
    expanded flags are copied."""
    from torchoptics_amd import ops
    seen = {}
    for name in ("layout-tracer", "layout-slice", "layout-expand", "layout-dense", "lens-batch"):
        t = EC.place(EC.rays(name), name, DEV)
        x = t["x"].detach().requires_grad_(True)
        S, sums = ops.EnclosedEnergyFunction.apply(x, t["y"], t["ok"], "row", EC.RADII, _inv(EC.SOFT, 16), "circle")
        saved = sums.grad_fn.saved_tensors
        seen[name] = [s.data_ptr() == t[k].data_ptr() for s, k in zip(saved, EC.KEYS)]
        if name == "layout-slice":
            assert x.data_ptr() % 16 == 4
    assert seen["layout-tracer"] == [True] * 3 and seen["layout-slice"] == [True] * 3 and seen["layout-dense"] == [True] * 3
    assert seen["layout-expand"] == [True, True, False] and seen["lens-batch"] == [True] * 3


def test_spot_centroid(ta):
    from torchoptics_amd import metrics
    rays = EC.rays("block-edge")
    t = EC.place(rays, "block-edge", DEV)
    x, y = (t[k].detach().requires_grad_(True) for k in "xy")
    n, c = metrics.spot_centroid(x, y, t["ok"], fused=True)
    S, T = R.spot_sums(rays["x"], rays["y"], rays["ok"])
    want = S[..., 1:3] / S[..., :1]
    assert np.array_equal(n.cpu().numpy(), S[..., 0]) and c.dtype == torch.float32
    assert np.all(np.abs(c.detach().cpu().numpy() - want) <= 2.0 ** -24 * np.abs(want) + R.spot_bound(T, 257)[..., 1:3] / S[..., :1])
    (c[..., 0].sum() + 2 * c[..., 1].sum()).backward()
    live = torch.from_numpy(rays["ok"]).to(DEV)
    per_row = (1 / torch.from_numpy(S[..., 0]).to(DEV))[:, :, None, :].expand_as(x).float()
    assert torch.equal(x.grad, torch.where(live, per_row, torch.zeros_like(per_row)))          # 1 / n on live rays, 0 on dead ones
    assert torch.equal(y.grad, torch.where(live, (2 * per_row.double()).float(), torch.zeros_like(per_row)))


# ------------------------------------------------------------------------------------------------------- through the tracer
T_RADII = tuple(0.01 * k for k in range(1, 17))
T_SOFT = 0.001


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
    for shape in EC.SHAPE_NAMES:
        for common, centre in ((("wavelength",), "row"), ((), "row"), (("field", "wavelength"), "field")):
            fu = metrics.enclosed_energy(x, y, ok, T_RADII, T_SOFT, shape=shape, common=common, centre=centre, fused=True)
            un = metrics.enclosed_energy(x, y, ok, T_RADII, T_SOFT, shape=shape, common=common, centre=centre, fused=False)
            de = metrics.enclosed_energy(x, y, ok, T_RADII, T_SOFT, shape=shape, common=common, centre=centre)
            for k, a, b, c in zip(fu._fields, fu, un, de):
                assert a.dtype == torch.float32 and torch.equal(a, c)
                ulps = ((a.double() - b.double()).abs() / (b.double().abs() * 2.0 ** -23).clamp(min=1e-45)).max().item()
                print(f"ENCLOSED-ACC tracer (a) {shape:6s} common={','.join(common) or '-':17s} centre={centre:5s} {k:6s} fused vs unfused {ulps:.2f} ulp")
                assert ulps <= 2.0, (shape, common, k)
    # (b) the 80 % radius lies between the radii that bracket the hard count's 80 %
    e = metrics.enclosed_energy(x, y, ok, T_RADII, T_SOFT, fused=True)
    r80, reached = metrics.enclosed_radius(e.energy, T_RADII, 0.8)
    xs, ys, oks = (q.detach().cpu().numpy() for q in (x, y, ok))
    S, _ = R.spot_sums(xs, ys, oks)
    c = S[..., 1:3] / S[..., :1]
    rho = np.sqrt((xs - c[:, :, None, :, 0]) ** 2 + (ys - c[:, :, None, :, 1]) ** 2)
    hard = np.stack([((rho <= Rk) & (oks != 0)).sum(axis=(2, 3)) for Rk in T_RADII], axis=-1) / S[..., 0].sum(axis=2)[..., None]
    j = (hard >= 0.8).argmax(axis=-1)
    lo, hi = np.asarray((0.0,) + T_RADII)[j], np.asarray(T_RADII)[j]
    r80 = r80.detach().cpu().numpy()
    print(f"ENCLOSED-ACC tracer (b) 80 % radius {r80.ravel()}  hard count reaches 0.8 in ({lo.ravel()}, {hi.ravel()}]")
    assert reached.all() and (hard[..., -1] >= 0.8).all()
    assert np.all((lo <= r80) & (r80 <= hi))
    # (c) leaf gradients of the mean 80 % radius against the float64 twin
    grads = {}
    for tag, double, fused in (("fused", False, True), ("unfused", False, False), ("twin", True, False)):
        (xx, yy, kk), lv = _cooke(ta, double=double)
        en = metrics.enclosed_energy(xx, yy, kk, T_RADII, T_SOFT, fused=fused)
        metrics.enclosed_radius(en.energy, T_RADII, 0.8)[0].mean().backward()
        grads[tag] = {k: lv[k].grad.double().cpu().numpy() for k in ("c", "t")}
    for k in ("c", "t"):
        e_f, e_u = rel_l2(grads["fused"][k], grads["twin"][k]), rel_l2(grads["unfused"][k], grads["twin"][k])
        print(f"ENCLOSED-ACC tracer (c) d r80.mean() / d{k}: fused {e_f:.3e}  unfused {e_u:.3e}  ratio {e_f / max(e_u, 1e-300):.3f}")
        assert e_f <= 2 * e_u + 1e-6, (k, e_f, e_u)


# ------------------------------------------------------------------------------------- no synchronisation, graph, fresh memory
def _step_case(shape, centre):
    """A step in the sense of tests/step_cases.py: the mean 80 % radius of "block-edge" and its gradients, two input sets."""
    import step_cases
    from torchoptics_amd import metrics
    rays = EC.rays("block-edge")                                 # F = 3, W = 2, P = 257
    rng = np.random.default_rng(606)
    A = {k: step_cases._tracer_layout(rays[k].transpose(0, 1, 3, 2)) for k in "xy"}
    B = {k: step_cases._tracer_layout((rays[k] + 1e-3 * rng.standard_normal(rays[k].shape)).transpose(0, 1, 3, 2)) for k in "xy"}
    ok = step_cases._tracer_layout(rays["ok"].transpose(0, 1, 3, 2)).to(torch.bool).to(DEV)
    given = torch.from_numpy(EC.given_centre("block-edge")).to(DEV)
    metrics.enclosed_radius(torch.zeros(1, 1, 16, device=DEV), EC.RADII, 0.8)          # (the radii's constant goes up once, here)

    def body(L):
        e = metrics.enclosed_energy(L["x"], L["y"], ok, EC.RADII, EC.SOFT, shape=shape, centre=given if centre == "given" else centre,
                                    fused=True)
        r80, _ = metrics.enclosed_radius(e.energy, EC.RADII, 0.8)
        (r80.mean() + e.energy.mean()).backward()
        return e.energy, r80
    return step_cases.Case(DEV, {"A": A, "B": B}, body, ("energy", "r80"), ("x", "y"))


@pytest.mark.parametrize("shape,centre", (("circle", "row"), ("square", "field"), ("circle", "given")))
def test_a_warm_step_is_sync_free_and_replays_its_eager_bits_from_a_graph(ta, shape, centre):
    """One stream, no parallel branches.  The sync check comes first: a step that synchronises is never captured."""
    from torchoptics_amd import graphs
    eager = {}
    for which in "AB":
        case = _step_case(shape, centre)
        case.load(which)
        eager[which] = [t.clone() for t in case.step()]
    torch.cuda.synchronize()
    assert not any(torch.equal(a, b) for a, b in zip(eager["A"], eager["B"]))
    case = _step_case(shape, centre)
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
    case = _step_case(shape, centre)                             # fresh leaves: no AccumulateGrad node of another stream
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


@pytest.mark.parametrize("shape", EC.SHAPE_NAMES)
@pytest.mark.parametrize("name", ("block-edge", "dead-row", "layout-slice"))
def test_the_same_bytes_whatever_the_buffers_held(ta, name, shape):
    from test_gpu_fresh_memory import hold
    for centre in CENTRES:
        rays, radii, c, g_sums, g_S, _, _ = _reference(name, shape, centre)
        hold("enclosed", f"{name}-{shape}-{centre}", lambda: _run(rays, name, shape, c, radii, EC.SOFT, g_sums, g_S))
