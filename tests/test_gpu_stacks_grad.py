"""
Gradients through the per-surface penalty stacks of trace_skew(aggregate=True) (the g_stacks member of the tl_seeds block of
tl_trace_bwd / tl_trace_bwd_from_outputs).

The lists z_RELU, theta_norm, theta_prime_norm are graph tensors, as in the reference: any function of them
back-propagates through the backward kernels with one seed per ray, row and term (kPenRay: trace_bwd_inv_unrolled_stk_kernel
for the rays alive at the image plane, trace_bwd_stk_kernel for the rest and for every lens the walk-back does not take).
References: the oracle's fp64 autograd of the same function of its own stacks, with the gates of test_gpu_kernel_matrix.py
(its fan and helpers are imported, not copied), and the fused seed of rt.unsupervised_loss where the function is the
caller's plain sum.
"""
import numpy as np
import pytest
import torch

import test_gpu_kernel_matrix as km
from conftest import load_golden, rel_l2

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KEYS = ("z_RELU", "theta_norm", "theta_prime_norm")
ROWS = (3, 7, 11, 12, 13, 20, 21, 25)


@pytest.fixture(scope="module")
def ta():
    import torchoptics_amd
    from torchoptics_amd import _lib
    _lib.lib()
    return torchoptics_amd


def _weights(S, shape, seed):
    """Per-element seeds [3, S, *shape]: positive (no cancellation between terms), seeded."""
    g = torch.Generator().manual_seed(seed)
    return 0.5 + torch.rand((3, S) + tuple(shape), generator=g, dtype=torch.float64)


def _stack_loss(stk, w):
    """sum over the three terms and the S rows of w * stacks (lists of S tensors)."""
    tot = 0.0
    for j, key in enumerate(KEYS):
        st = torch.stack(list(stk[key]), 0)
        tot = tot + (w[j].to(st.dtype).to(st.device) * st).sum()
    return tot


_OR = {}
_FAN = {}


def _fan(S, variant, P):
    if (S, variant, P) not in _FAN:
        _FAN[(S, variant, P)] = km._fan(S, variant, P)
    return _FAN[(S, variant, P)]


def _oracle(S, variant, P, w, tag):
    """fp32 (IEEE sqrt) and fp64 oracle gradients of _stack_loss(stacks, w) on the fan of test_gpu_kernel_matrix."""
    from oracle import trace_oracle as orc
    key = (S, variant, P, tag)
    if key in _OR:
        return _OR[key]
    a = _fan(S, variant, P)
    names = km._LEAVES + (("kappa", "poly") if a["rows"] else ())
    res = {"args": a, "names": names}
    for t, dt in (("f32", torch.float32), ("f64", torch.float64)):
        lv = {n: (a[n].to(dt).expand(a["x"].shape) if n in km._PER_RAY else a[n].to(dt)).clone().requires_grad_(True)
              for n in names}
        kw = dict(kappa=lv["kappa"], poly=lv["poly"], kind=a["kind"]) if a["rows"] else {}
        o = orc.trace_skew_general(a["x"].to(dt), a["y"].to(dt), lv["z"], a["cx"].to(dt), lv["cy"], lv["c"], lv["t"],
                                   lv["mu"], a["mask"], ieee_sqrt=(dt == torch.float32), aggregate=True, **kw)
        loss = _stack_loss(o[7], w)
        g = torch.autograd.grad(loss, [lv[n] for n in names], allow_unused=True)
        res[t] = {n: (torch.zeros_like(lv[n]) if gi is None else gi).double() for n, gi in zip(names, g)}
        res[t + "_ok"] = o[4].detach()
    _OR[key] = res
    return res


def _gpu(ta, a, mode, algo, loss_fn, need_xy=False):
    """The kernels on the fan `a`: loss_fn(out, rt) is back-propagated; gradients of the lens / launch leaves."""
    from torchoptics_amd import ops, ray_tracing as rt
    names = km._LEAVES + (("kappa", "poly") if a["rows"] else ())
    lv = {n: a[n].to(DEV).clone().requires_grad_(True) for n in names}
    x, y = a["x"].to(DEV).clone(), a["y"].to(DEV).clone()
    if need_xy:
        x.requires_grad_(True)
        y.requires_grad_(True)
    kw = {}
    if a["rows"]:
        kw = dict(kappa=lv["kappa"], poly=lv["poly"], surf_kind=torch.tensor(a["kind"], dtype=torch.bool, device=DEV))
    ops.set_backward_algorithm(algo)
    try:
        out = ta.trace_skew(x, y, lv["z"], a["cx"].to(DEV), lv["cy"], lv["c"], lv["t"], lv["mu"], a["mask"].to(DEV),
                            True, True, mode=mode, **kw)
        inv = ops.used_walk_back(out[0])
        loss_fn(out, rt).backward()
    finally:
        ops.set_backward_algorithm("inverse")
    g = {n: lv[n].grad.detach().cpu().double() for n in names}
    if need_xy:
        g["x"], g["y"] = x.grad.detach().cpu().double(), y.grad.detach().cpu().double()
    return g, inv


def _check(tag, got, r, mode, S):
    k = 1.0 if mode == "strict" else 10.0
    km._grad_errors(tag, {n: got[n] for n in r["names"]}, r["f32"], r["f64"], True, k, r["args"]["rows"], S)


# ------------------------------------------------------------------ 1. the caller's loss through the stacks
def test_caller_loss_through_the_stacks_matches_fused_seed_and_reference(ta):
    """compute_loss_out's sumQ written on the stack lists (fixture G7, RayTracer.trace_rays): the penalty has a graph,
    and its gradient and that of rms + 0.2 sumQ are the fused seed's (rt.unsupervised_loss) and the reference's."""
    import yaml_free_lenses as L
    from torchoptics_amd import ray_tracing as rt
    g = load_golden("G7_harness_cooke")
    keys = ("c", "t", "nd", "v")
    res = {}
    for how in ("stacks", "fused"):
        lens, specs, leaves = L.build("cooke", DEV, epd=8.578)
        tr = ta.RayTracer(mode="circular", n_rays=(8, 8), rel_fields=list(np.linspace(0, 1, 3)), wavelengths=[459., 520., 640.],
                          n_ray_aiming_iter=1, default_device=DEV)
        out = tr.trace_rays(specs, lens, aggregate=True)
        if how == "stacks":
            penalty = rt.penalty_sum(dict(out[6]), 7)          # a plain dict: summed through the lists
            assert penalty.grad_fn is not None
            rms = ta.compute_rms2d(out[0], out[1], out[4])
        else:
            ld = rt.unsupervised_loss(out, 7, 0.2)
            penalty, rms = ld["penalty"], ld["rms"]
        loss = rms + 0.2 * penalty
        gp = torch.autograd.grad(penalty, [leaves[k] for k in keys], retain_graph=True)
        gl = torch.autograd.grad(loss, [leaves[k] for k in keys])
        res[how] = (penalty.item(), [t.cpu().numpy() for t in gp], [t.cpu().numpy() for t in gl])
    assert abs(res["stacks"][0] - res["fused"][0]) <= 1e-6 * abs(res["fused"][0])
    for i, k in enumerate(keys):
        for j, what in ((1, "penalty"), (2, "loss_unsup")):
            got, fused = res["stacks"][j][i], res["fused"][j][i]
            assert rel_l2(got, fused) <= 1e-6, f"d {what} / d{k} vs fused seed: {rel_l2(got, fused):.2e}"
            ref = g[f"g_{what}_{k}"]
            assert rel_l2(got, ref) <= 3e-4, f"d {what} / d{k} vs reference: {rel_l2(got, ref):.2e}"


# ------------------------------------------------------------------ 2. random per-element seeds vs fp64 autograd
@pytest.mark.parametrize("algo", ("inverse", "checkpoint"))
@pytest.mark.parametrize("mode", ("strict", "fast"))
@pytest.mark.parametrize("variant", ("sph", "asph"))
@pytest.mark.parametrize("S,P", [(S, km.P_MAIN) for S in ROWS] + [(3, km.P_SMALL), (12, km.P_SMALL)])
def test_random_stack_seeds_match_fp64_oracle(ta, S, P, variant, mode, algo):
    a = _fan(S, variant, P)
    w = _weights(S, a["x"].shape, 1000 + S)
    r = _oracle(S, variant, P, w, "rand")
    got, inv = _gpu(ta, r["args"], mode, algo, lambda out, rt: _stack_loss(out[6], w))
    assert inv == (algo == "inverse"), "backward algorithm"
    assert bool((~r["f64_ok"]).any()), "the fan should lose rays on the way"
    _check(f"S={S} {variant} P={P} {mode} {algo}", got, r, mode, S)


# ------------------------------------------------------------------ 3. sparse seeds
def _sparse(S, shape, which, ok64):
    w = torch.zeros((3, S) + tuple(shape), dtype=torch.float64)
    if which == "zrelu_mid":
        w[0, S // 2] = 1.0
    elif which == "thetap_last":
        w[2, S - 1] = 1.0
    else:                                                   # one ray's theta at one row: a ray alive at the image plane
        idx = torch.nonzero(ok64.reshape(shape))[len(torch.nonzero(ok64.reshape(shape))) // 3]
        w[(1, S // 3) + tuple(idx.tolist())] = 1.0
    return w


@pytest.mark.parametrize("algo", ("inverse", "checkpoint"))
@pytest.mark.parametrize("variant", ("sph", "asph"))
@pytest.mark.parametrize("which", ("zrelu_mid", "thetap_last", "one_ray_theta"))
def test_sparse_stack_seeds_match_fp64_oracle(ta, which, variant, algo):
    S, P, mode = 11, km.P_MAIN, "strict"
    a = _fan(S, variant, P)
    ok64 = _oracle(S, variant, P, _weights(S, a["x"].shape, 1000 + S), "rand")["f64_ok"]
    w = _sparse(S, a["x"].shape, which, ok64)
    r = _oracle(S, variant, P, w, which)
    got, _ = _gpu(ta, r["args"], mode, algo, lambda out, rt: _stack_loss(out[6], w))
    _check(f"{which} {variant} {algo}", got, r, mode, S)


# ------------------------------------------------------------------ 4. both seed kinds in one loss
@pytest.mark.parametrize("algo", ("inverse", "checkpoint"))
@pytest.mark.parametrize("variant", ("sph", "asph"))
def test_fused_and_stack_seeds_add(ta, variant, algo):
    S, P, lam = 11, km.P_MAIN, 0.3
    a = _fan(S, variant, P)
    w = _weights(S, a["x"].shape, 7)
    fused = lambda out, rt: ta.compute_rms2d(out[0], out[1], out[4]) + lam * rt.penalty_sum(out[6], S)   # noqa: E731
    stack = lambda out, rt: _stack_loss(out[6], w)                                                       # noqa: E731
    both, _ = _gpu(ta, a, "strict", algo, lambda out, rt: fused(out, rt) + stack(out, rt))
    g1, _ = _gpu(ta, a, "strict", algo, fused)
    g2, _ = _gpu(ta, a, "strict", algo, stack)
    for n in both:
        tol = 1e-3 if n in km._PER_RAY else 1e-5
        want = g1[n] + g2[n]
        if n in km._PER_RAY:
            got_n, want = km._reduce(n, both[n], None), km._reduce(n, want, None)
        else:
            got_n = both[n]
        assert rel_l2(got_n.numpy(), want.numpy()) <= tol, f"d/d{n}: {rel_l2(got_n.numpy(), want.numpy()):.2e}"


# ------------------------------------------------------------------ 5. lens batches
def _batch_run(ta, c, t, x, y, cx, cy, z, mu, mask, w, algo="inverse"):
    from torchoptics_amd import ops
    cl, tl = c.clone().requires_grad_(True), t.clone().requires_grad_(True)
    ops.set_backward_algorithm(algo)
    try:
        out = ta.trace_skew(x, y, z, cx, cy, cl, tl, mu, mask, True, True)
        _stack_loss(out[6], w).backward()
    finally:
        ops.set_backward_algorithm("inverse")
    return cl.grad.detach().cpu(), tl.grad.detach().cpu()


@pytest.mark.parametrize("algo", ("inverse", "checkpoint"))
def test_lens_batch_of_three_per_lens(ta, algo):
    """B = 3 perturbed lenses in one launch: each lens' d/dc, d/dt equal that lens traced alone."""
    S, P = 11, km.P_MAIN
    a = _fan(S, "sph", P)
    lenses = [km._perturbed(a, b) for b in range(3)]
    c = torch.cat([l["c"] for l in lenses], 0).to(DEV)
    t = torch.cat([l["t"] for l in lenses], 0).to(DEV)
    common = [a[k].to(DEV) for k in ("x", "y", "cx", "cy")]
    z, mu, mask = a["z"].to(DEV), a["mu"].to(DEV), a["mask"].to(DEV)
    w = _weights(S, (3,) + tuple(a["x"].shape[1:]), 3)
    gc, gt = _batch_run(ta, c, t, *common, z, mu, mask, w, algo)
    for b in range(3):
        gcb, gtb = _batch_run(ta, c[b:b + 1], t[b:b + 1], *common, z, mu, mask, w[:, :, b:b + 1], algo)
        assert rel_l2(gc[b].numpy(), gcb[0].numpy()) <= 1e-6, b
        assert rel_l2(gt[b].numpy(), gtb[0].numpy()) <= 1e-6, b


def test_lens_batch_past_the_grid_limit_equals_lenses_one_at_a_time(ta):
    """A batch of more than 65 535 grid rows (lens, field, wavelength) takes the lens-chunked path: the stacks stay
    differentiable through its cat / stack, and sampled lenses' gradients equal those lenses traced alone."""
    from torchoptics_amd import ray_tracing as rt
    S, P = 7, 16
    a = _fan(S, "sph", P)
    F, W = a["cy"].shape[1], a["mu"].shape[3]
    B = rt._MAX_GRID_ROWS // (F * W) + 40
    g = torch.Generator().manual_seed(5)
    scale = 1 + 0.01 * torch.randn((B, 1, 1, 1, S), generator=g)
    c = (a["c"] * scale).to(DEV)
    t = (a["t"] * (1 + 0.01 * torch.rand((B, 1, 1, 1, S), generator=g))).to(DEV)
    common = [a[k].to(DEV) for k in ("x", "y", "cx", "cy")]
    z, mu, mask = a["z"].to(DEV), a["mu"].to(DEV), a["mask"].to(DEV)
    w = _weights(S, (B,) + tuple(a["x"].shape[1:]), 11)
    gc, gt = _batch_run(ta, c, t, *common, z, mu, mask, w)
    nb = rt._MAX_GRID_ROWS // (F * W)
    for b in (0, nb - 1, nb, B - 1):
        gcb, gtb = _batch_run(ta, c[b:b + 1], t[b:b + 1], *common, z, mu, mask, w[:, :, b:b + 1])
        assert rel_l2(gc[b].numpy(), gcb[0].numpy()) <= 1e-6, b
        assert rel_l2(gt[b].numpy(), gtb[0].numpy()) <= 1e-6, b


# ------------------------------------------------------------------ 6. the other checkpoint routes
@pytest.mark.parametrize("variant", ("sph", "asph"))
def test_per_ray_input_gradients_with_stack_seeds(ta, variant):
    """x, y requiring grad keep the checkpoint algorithm: the lens gradients and d/dx, d/dy against fp64."""
    from oracle import trace_oracle as orc
    S, P, mode = 11, km.P_MAIN, "strict"
    a = _fan(S, variant, P)
    w = _weights(S, a["x"].shape, 1000 + S)
    r = _oracle(S, variant, P, w, "rand")
    got, inv = _gpu(ta, r["args"], mode, "inverse", lambda out, rt: _stack_loss(out[6], w), need_xy=True)
    assert not inv
    _check(f"xy {variant}", got, r, mode, S)
    xd = a["x"].double().clone().requires_grad_(True)
    yd = a["y"].double().clone().requires_grad_(True)
    kw = dict(kappa=a["kappa"].double(), poly=a["poly"].double(), kind=a["kind"]) if a["rows"] else {}
    o = orc.trace_skew_general(xd, yd, *[a[k].double() for k in ("z", "cx", "cy", "c", "t", "mu")], a["mask"],
                               aggregate=True, **kw)
    gx, gy = torch.autograd.grad(_stack_loss(o[7], w), [xd, yd])
    assert rel_l2(got["x"].numpy(), gx.numpy()) <= 1e-3
    assert rel_l2(got["y"].numpy(), gy.numpy()) <= 1e-3


# ------------------------------------------------------------------ 7. the two host chains
@pytest.mark.parametrize("case", ("inverse", "checkpoint", "asph", "xy", "small_p", "sparse"))
def test_host_chains_agree_bit_for_bit(ta, case):
    from test_gpu_host_chain import _both
    S, variant, P, algo, need_xy = 11, "sph", km.P_MAIN, "inverse", False
    if case == "checkpoint":
        algo = "checkpoint"
    elif case == "asph":
        variant = "asph"
    elif case == "xy":
        need_xy = True
    elif case == "small_p":
        S, P = 12, km.P_SMALL
    a = _fan(S, variant, P)
    w = _weights(S, a["x"].shape, 21)
    if case == "sparse":
        w[:, :S - 1] = 0.0
    res = _both(lambda: _gpu(ta, a, "strict", algo, lambda out, rt: _stack_loss(out[6], w), need_xy=need_xy)[0])
    assert res[0].keys() == res[1].keys()
    for n in res[0]:
        assert torch.equal(res[0][n], res[1][n]), n
