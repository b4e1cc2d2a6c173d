"""
The fp32 trace kernels on skew fields and under per-ray (dense) seeds, against the oracle's fp64 autograd.

test_gpu_kernel_matrix.py holds every backward instantiation to fp64 on a meridional fan (cx = 0, never a leaf) under the
moment seeds of compute_rms2d and the penalty.  Here the same fan is turned about the axis (seed_cases.turned), cx is a
leaf, and the losses are linear in the per-ray outputs with fixed random weights, so that the kernels receive the gx, gy,
gcx, gcy arrays: all four with and without the moment seed, and the partial sets autograd produces (gx alone, gcx alone,
gy + gcy).  What that reaches and the existing matrix does not:

  d/dcx          the direct sum (acc_cx), its column in reduce_bwd_kernel, cx_stride / cx_stride_b, fold(g_cx, cx) of the
                 host chains, and the fold of the cz0 adjoint (cz0 = sqrt(1 - cx^2 - cy^2)) into g_cx and g_cy, which cx = 0
                 multiplies by zero: `v -= s_cz * cx / cz0` in trace_bwd_kernel, k_cx / k_cy in the walk-back kernels
  the forward    strict mode bit-equal to the IEEE oracle at cx != 0
  dense seeds    the pointer tests of the spherical walk-back, the seed bits of the aspheric one, the moment seed added on
                 top, the rolled kernel, the checkpoint buckets, the device-side fallback; non-zero seeds on dead rays
  x_in, y_in     per-ray input gradients (checkpoint kernel) on skew fans, zero on dead rays

Cases, losses and reference: seed_cases.py, which test_seed_cases_cpu.py checks without a GPU.  Gates: those of
test_gpu_kernel_matrix.py (_gate, _grad_errors), d/dcx under the rule of d/dcy.  Each test prints one SEED-ACC line; the
lines of one run are kept as profiles/seed_accuracy.txt.
"""
import pytest
import torch

import seed_cases as sc
import test_gpu_kernel_matrix as km
from conftest import rel_l2

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_MODES = ("strict", "fast")
_ALGOS = ("inverse", "checkpoint")
_PER_LENS = ("z", "cx", "cy", "c", "t")        # of a lens batch; mu, kappa, poly are shared


@pytest.fixture(scope="module")
def ta():
    import torchoptics_amd
    from torchoptics_amd import _lib
    _lib.lib()
    return torchoptics_amd


def _run_gpu(ta, lenses, variant, loss, mode, algo, wts, lens_w=None, need_xy=False):
    """The kernels on one lens (or a batch, stacked along dim 0) through ta.trace_skew, as km._run_gpu runs them, with cx a
    leaf and the loss `loss` of seed_cases (dense terms NOT masked: dead rays carry seeds)."""
    from torchoptics_amd import ops, ray_tracing as rt
    a0, B = lenses[0], len(lenses)
    names = sc.names_of(a0)
    lv = {}
    for n in names:
        v = torch.cat([a[n] for a in lenses], 0) if (B > 1 and n in _PER_LENS) else a0[n]
        lv[n] = v.to(DEV).clone().requires_grad_(True)
    x, y = a0["x"].to(DEV).clone().requires_grad_(need_xy), a0["y"].to(DEV).clone().requires_grad_(need_xy)
    kw = {}
    if a0["rows"]:
        kw = dict(kappa=lv["kappa"], poly=lv["poly"], surf_kind=torch.tensor(a0["kind"], dtype=torch.bool, device=DEV))
    ops.set_backward_algorithm(algo)
    ops.set_asph_hit_slots(km.HIT_SLOTS.get(variant, 4))
    try:
        out = ta.trace_skew(x, y, lv["z"], lv["cx"], lv["cy"], lv["c"], lv["t"], lv["mu"], a0["mask"].to(DEV), False, True,
                            mode=mode, **kw)
        inv = ops.used_walk_back(out[0])
        if B > 1:
            assert loss == "rms+all"
            per_lens = rt.compute_rms2d_batch(out[0], out[1], out[4])
            for n, q in zip(sc.OUTS, out[:4]):
                per_lens = per_lens + (q * wts[n].float().to(DEV)).sum(dim=(1, 2, 3))
            total = (per_lens * torch.tensor(lens_w, device=DEV)).sum()
        else:
            total = sc.loss_of(loss, out[:4], wts, lambda: ta.compute_rms2d(out[0], out[1], out[4]))
        total.backward()
    finally:
        ops.set_backward_algorithm("inverse")
        ops.set_asph_hit_slots(4)
    grads = {n: lv[n].grad.detach().cpu().double() for n in names}
    if need_xy:
        grads["x"], grads["y"] = x.grad.detach().cpu().double(), y.grad.detach().cpu().double()
    return dict(fwd=[t.detach().cpu() for t in out[:6]], inv=inv, grads=grads)


def _check_forward(tag, got, r, exact, k):
    """km._check_forward (spherical + strict: bit-equal to the fp32 IEEE oracle in x, y, cx, cy, ok, back), and all four
    outputs of every dead ray parked at zero: the unmasked dense terms rely on it."""
    km._check_forward(tag, got, r["f32"]["fwd"], r["f64"]["fwd"], exact, k)
    dead = ~got[4]
    for n, q in zip(sc.OUTS, got[:4]):
        assert not q[dead].any(), f"{tag}: output {n} of a dead ray is not parked at zero"


def _check_grads(tag, got, r32, r64, k, rows, S, live):
    """Every gradient but d/dcx through km._grad_errors (lens parameters km._gate, z the per-ray-noise rule, cy
    max(3 noise, 3e-5) k + 2 noise); d/dcx under cy's rule against the per-ray reference summed to the kernel's shape.
    Prints the SEED-ACC line, returns {parameter: error / gate}."""
    msg = km._grad_errors(tag, {n: g for n, g in got.items() if n != "cx"}, r32, r64, False, k, rows, S)
    ratio = {}
    for m in msg:
        n, e, noise = m.split()[0], *(float(v) for v in m.split()[1].split("/")[:2])
        ratio[n] = e / km._gate(n, False, noise, k)
    if "cx" in got:
        g = got["cx"]
        assert torch.isfinite(g).all(), f"{tag}: d/dcx not finite"
        w32, w64 = sc.summed("cx", r32["cx"]), sc.summed("cx", r64["cx"])
        e64, noise = rel_l2(g.numpy(), w64.numpy()), rel_l2(w32.numpy(), w64.numpy())
        gate = km._gate("cy", False, noise, k)
        msg.insert(1, f"cx {e64:.1e}/{noise:.1e}")
        ratio["cx"] = e64 / gate
    print(f"SEED-ACC {tag}: live {live} | e64/noise " + ", ".join(msg))
    if "cx" in got:
        assert e64 <= gate, f"{tag} d/dcx: vs fp64 {e64:.2e}, oracle fp32 itself {noise:.2e}, gate {gate:.2e}"
    return ratio


def _live(r):
    ok = r["f32"]["fwd"][4]
    return f"{int(ok.sum())}/{ok.numel()}"


_CASE_IDS = [f"S{s}-{v}-P{p}-{loss}" for (s, v, p), loss in sc.CASES]


@pytest.mark.parametrize("algo", _ALGOS)
@pytest.mark.parametrize("mode", _MODES)
@pytest.mark.parametrize("lens,loss", sc.CASES, ids=_CASE_IDS)
def test_skew_fan_and_dense_seeds_match_fp64_oracle(ta, lens, loss, mode, algo):
    S, variant, P = lens
    r = sc.reference(S, variant, P)
    a, k = r["args"], (10.0 if mode == "fast" else 1.0)
    assert bool((a["cx"] != 0).all())
    got = _run_gpu(ta, [a], variant, loss, mode, algo, r["wts"])
    tag = f"S={S} {variant} P={P} {loss} {mode} {algo}"
    assert got["inv"] is (algo == "inverse"), tag
    _check_forward(tag, got["fwd"], r, exact=(variant == "sph" and mode == "strict"), k=k)
    _check_grads(tag, got["grads"], r["f32"]["grads"][loss], r["f64"]["grads"][loss], k, a["rows"], S, _live(r))


@pytest.mark.parametrize("mode", _MODES)
@pytest.mark.parametrize("variant", ("sph", "asph"))
@pytest.mark.parametrize("S", sc.XY_ROWS)
def test_input_gradients_on_skew_fans(ta, S, variant, mode):
    """x_in, y_in requiring a gradient: ops takes the checkpoint kernel whatever the algorithm asked for.  d/dx_in, d/dy_in
    within 3e-5 k + 2 noise of fp64 (test_gpu_parity.py's gate), and exactly zero on every ray dead in the GPU's own mask
    (the kernel is handed an uninitialised buffer)."""
    r = sc.reference(S, variant, sc.P_MAIN)
    a, k, loss = r["args"], (10.0 if mode == "fast" else 1.0), "rms+all"
    got = _run_gpu(ta, [a], variant, loss, mode, "inverse", r["wts"], need_xy=True)
    tag = f"xy S={S} {variant} P={sc.P_MAIN} {loss} {mode}"
    assert got["inv"] is False, f"{tag}: per-ray input gradients take the checkpoint kernel"
    _check_forward(tag, got["fwd"], r, exact=(variant == "sph" and mode == "strict"), k=k)
    r32, r64 = r["f32"]["grads"][loss], r["f64"]["grads"][loss]
    lens_grads = {n: g for n, g in got["grads"].items() if n not in ("x", "y")}
    ratio = _check_grads(tag, lens_grads, r32, r64, k, a["rows"], S, _live(r))
    dead = ~got["fwd"][4]
    line = []
    for n in ("x", "y"):
        g = got["grads"][n]
        assert torch.isfinite(g).all(), f"{tag}: d/d{n}_in not finite"
        assert g[dead].abs().max().item() == 0.0, f"{tag}: d/d{n}_in of a dead ray is not zero"
        e64, noise = rel_l2(g.numpy(), r64[n].numpy()), rel_l2(r32[n].numpy(), r64[n].numpy())
        line.append(f"{n}_in {e64:.1e}/{noise:.1e}")
        ratio[n + "_in"] = e64 / (3e-5 * k + 2 * noise)
    print(f"SEED-ACC {tag}: live {_live(r)} | e64/noise " + ", ".join(line))
    for n in ("x", "y"):
        assert ratio[n + "_in"] <= 1.0, f"{tag} d/d{n}_in: {ratio[n + '_in']:.2f} x the gate"


@pytest.mark.parametrize("algo", _ALGOS)
@pytest.mark.parametrize("mode", _MODES)
@pytest.mark.parametrize("S,variant,P", sc.BATCH_LENSES, ids=[f"S{s}-{v}" for s, v, _ in sc.BATCH_LENSES])
def test_lens_batch_with_per_lens_directions(ta, S, variant, P, mode, algo):
    """B = 3 perturbed lenses in one launch, cx and cy [B,F,1,1] (lens b looks along 1 + 0.005 b times the directions of lens
    0), weighted per-lens losses rms+all: z, c, t, cx, cy of each lens against its own oracle run, the shared mu, kappa, poly
    against the weighted sum.  cx_stride_b, cy_stride_b and the per-lens branch of fold()."""
    rs = [sc.reference(S, variant, P, b) for b in range(len(km.BATCH_W))]
    k, loss = (10.0 if mode == "fast" else 1.0), "rms+all"
    got = _run_gpu(ta, [r["args"] for r in rs], variant, loss, mode, algo, rs[0]["wts"], lens_w=km.BATCH_W)
    tag = f"batch S={S} {variant} {loss} {mode} {algo}"
    assert got["inv"] is (algo == "inverse"), tag
    assert got["grads"]["cx"].shape == (len(rs),) + tuple(rs[0]["args"]["cx"].shape[1:])
    shared = {}
    for b, (r, w) in enumerate(zip(rs, km.BATCH_W)):
        tb = f"{tag} lens {b}"
        _check_forward(tb, [t[b:b + 1] for t in got["fwd"]], r, exact=(variant == "sph" and mode == "strict"), k=k)
        ref32 = {n: w * g for n, g in r["f32"]["grads"][loss].items()}
        ref64 = {n: w * g for n, g in r["f64"]["grads"][loss].items()}
        _check_grads(tb, {n: got["grads"][n][b:b + 1] for n in _PER_LENS}, ref32, ref64, k, r["args"]["rows"], S, _live(r))
        for n in r["names"]:
            if n not in _PER_LENS:
                acc = shared.setdefault(n, [0.0, 0.0])
                acc[0], acc[1] = acc[0] + ref32[n], acc[1] + ref64[n]
    _check_grads(tag + " shared", {n: got["grads"][n] for n in shared}, {n: v[0] for n, v in shared.items()},
                 {n: v[1] for n, v in shared.items()}, k, rs[0]["args"]["rows"], S, "-")
