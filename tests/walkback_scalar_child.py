#!/usr/bin/env python3
"""Fans and GPU runs of tests/test_gpu_walkback_scalar.py, and its child process.

    python tests/walkback_scalar_child.py OUT.npz LAM

runs the several-chunks fan (CHUNK_FAN) through the walk-back with the three backward seeds (LOSSES) and writes every
gradient to OUT.npz: the lens / launch gradients of the real caller's path (trace_skew), and the per-ray input gradients
g_x_in, g_y_in of the walk-back kernel through the C entry (run_cabi: the host chains send a backward that needs them to
the checkpoint algorithm).  The launch plan variables (TL_PLAN_FEW ...) are read once per process by the library, so the
test starts this file as a fresh process per plan; nothing here touches the GPU before the library reads them."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

DEV = "cuda:0"
KEYS = ("z_RELU", "theta_norm", "theta_prime_norm")
LEAVES = ("z", "cy", "c", "t", "mu", "kappa", "poly")
LOSSES = ("rms", "sum", "stk")      # moment seeds alone | + the uniform penalty seed (aggregate='sum') | + per-ray stack seeds
REL_FIELDS = {1: (0.707,), 2: (0.5, 1.0), 3: (0.3, 0.65, 1.0)}
WAVELENGTHS = {1: ("d",), 2: ("C", "F"), 3: ("C", "d", "F")}
FILL = 0.95                         # pupil radius / entrance pupil radius: every ray passes (prescriptions._DG_ASPH)
# P = 256 * 37 + 19 points, 2 fields, 1 wavelength, aspheres on rows 1 and 10: with TL_PLAN_FEW=4 the plan is 5 blocks
# per (f, w) with 7 or 8 chunks each and a ragged last chunk (make_plan in csrc/tl_api.hip: 38 chunks * 2 / 4 -> R = 8)
CHUNK_FAN = dict(P=256 * 37 + 19, F=2, W=1, rows=(1, 10))


def fan(P, F, W, rows, seed=0):
    """CPU kernel arguments of the 11-row double Gauss with the rows `rows` aspheric (mild conic + a4, a6 of the size of
    prescriptions._DG_ASPH; rows 1 and 10 keep the prescription's own), a random P-point pupil shared by F fields and
    W wavelengths."""
    import torchoptics_amd as ta
    from torchoptics_amd import prescriptions as PR
    lens, specs, _ = PR.double_gauss("cpu", requires_grad=False, aspheres=True)
    tr = ta.RayTracer(mode="circular", n_rays=(4, 4), rel_fields=REL_FIELDS[F], wavelengths=WAVELENGTHS[W],
                      default_device="cpu")
    with torch.no_grad():
        a = dict(tr.assemble(specs, lens))
    S = a["c"].shape[-1]
    assert S == 11
    kap, pol = np.zeros(S, np.float32), np.zeros((S, 4), np.float32)
    mild = [PR._DG_ASPH[1], PR._DG_ASPH[10]]
    for i, k in enumerate(rows):
        kap[k], pol[k] = PR._DG_ASPH.get(k, mild[i & 1])
    a["kappa"], a["poly"] = torch.from_numpy(kap), torch.from_numpy(pol)
    a["rows"] = list(rows)
    a["kind"] = [1 if k in rows else 0 for k in range(S)]
    rng = np.random.default_rng(4000 + 17 * P + seed)
    r = (np.sqrt(rng.random(P)) * (0.5 * float(specs.epd.item()) * FILL)).astype(np.float32)
    th = (rng.random(P) * 2 * np.pi).astype(np.float32)
    a["x"] = torch.from_numpy(r * np.cos(th)).reshape(1, 1, P, 1).expand(1, F, P, W)
    a["y"] = torch.from_numpy(r * np.sin(th)).reshape(1, 1, P, 1).expand(1, F, P, W)
    for n in ("z", "cx", "cy", "c", "t", "mu"):
        a[n] = a[n].detach().float()
    return a


def stack_weights(S, shape, seed=5):
    """Per-element seeds [3, S, *shape] of the stacks: positive (no cancellation between terms), seeded."""
    g = torch.Generator().manual_seed(seed)
    return 0.5 + torch.rand((3, S) + tuple(shape), generator=g, dtype=torch.float64)


def stack_loss(stk, w):
    """sum over the three terms and the S rows of w * stacks (lists of S tensors)."""
    tot = 0.0
    for j, key in enumerate(KEYS):
        st = torch.stack(list(stk[key]), 0)
        tot = tot + (w[j].to(st.dtype).to(st.device) * st).sum()
    return tot


def run_gpu(a, loss, lam, algo="inverse", mode="strict"):
    """The kernels on the fan `a`: gradients of every leaf (float32 arrays), and whether the host took the walk-back.
    loss: 'rms' | 'sum' = rms + lam penalty_sum (aggregate='sum') | 'stk' = rms + lam stack_loss."""
    import torchoptics_amd as ta
    from torchoptics_amd import ops, ray_tracing as rt
    S = a["c"].shape[-1]
    lv = {n: a[n].to(DEV).clone().requires_grad_(True) for n in LEAVES}
    x, y = a["x"].to(DEV), a["y"].to(DEV)
    aggregate = {"rms": False, "sum": "sum", "stk": True}[loss]
    ops.set_backward_algorithm(algo)
    try:
        out = ta.trace_skew(x, y, lv["z"], a["cx"].to(DEV), lv["cy"], lv["c"], lv["t"], lv["mu"], a["mask"].to(DEV),
                            aggregate, True, mode=mode, kappa=lv["kappa"], poly=lv["poly"],
                            surf_kind=torch.tensor(a["kind"], dtype=torch.bool, device=DEV))
        inv = ops.used_walk_back(out[0])
        total = ta.compute_rms2d(out[0], out[1], out[4])
        if loss == "sum":
            total = total + lam * rt.penalty_sum(out[6], S)
        elif loss == "stk":
            total = total + lam * stack_loss(out[6], stack_weights(S, out[0].shape))
        total.backward()
    finally:
        ops.set_backward_algorithm("inverse")
    g = {n: lv[n].grad.detach().cpu().numpy() for n in LEAVES}
    g["ok"] = out[4].detach().cpu().numpy()
    return g, inv


def run_cabi(a, loss, mode="strict"):
    """tl_trace_fwd + tl_trace_bwd_from_outputs on the fan `a` with g_x_in, g_y_in requested: the walk-back kernel's per-ray
    input gradients [1,F,W,P] and its lens gradients, for seeded random upstream gradients (moments; 'sum': the problem
    carries the penalty term, moment 8 is its uniform seed; 'stk': + per-ray, per-row stack seeds)."""
    import ctypes as C
    from torchoptics_amd import _lib, ops
    lib = _lib.lib()
    dev = torch.device(DEV)
    F, P, W = a["x"].shape[1:]
    S = a["c"].shape[-1]
    d = lambda t: t.to(dev).contiguous()                                             # noqa: E731
    x_e, y_e = a["x"].to(dev), a["y"].to(dev)                                        # [1,F,P,W] expanded views
    z, cxv, cyv = d(a["z"].reshape(1)), d(a["cx"].reshape(1, -1)), d(a["cy"].reshape(1, -1))
    c, t = d(a["c"].reshape(S)), d(a["t"].reshape(S))
    mu = d(a["mu"].reshape(-1, S).expand(W, S))
    mask = d(a["mask"].reshape(-1).to(torch.uint8))
    kap, pol = d(a["kappa"].reshape(S)), d(a["poly"].reshape(S, 4))
    kind = d(torch.tensor(a["kind"], dtype=torch.uint8))
    hits = torch.empty((ops.ASPH_HIT_SLOTS, 2, 1, F, W, P), dtype=torch.float32, device=dev)
    prob = ops._problem(x_e, y_e, z, cxv, cyv, c, t, mu, mask, True, mode, kap, pol, kind, None, loss != "rms", hits)
    outs = [torch.empty((1, F, W, P), dtype=torch.float32, device=dev) for _ in range(4)]
    flags = [torch.empty((1, F, W, P), dtype=torch.uint8, device=dev) for _ in range(2)]
    mom = torch.empty((F, _lib.TL_NMOM), dtype=torch.float64, device=dev)
    gen = torch.Generator().manual_seed(11)
    gmom = d(torch.randn((F, _lib.TL_NMOM), generator=gen, dtype=torch.float64) * 1e-3)
    gstk = d(torch.rand((3, S, 1, F, W, P), generator=gen, dtype=torch.float32) * 1e-3) if loss == "stk" else None
    gpar = torch.zeros(2 * S + W * S + 1 + 2 * F + 5 * S, dtype=torch.float32, device=dev)
    g_c, g_t, g_mu, g_z, g_cx, g_cy, g_kap, g_pol = torch.split(gpar, [S, S, W * S, 1, F, F, S, 4 * S])
    gxin = torch.zeros((1, F, W, P), dtype=torch.float32, device=dev)
    gyin = torch.zeros((1, F, W, P), dtype=torch.float32, device=dev)
    ws = torch.zeros(lib.tl_workspace_bytes(C.byref(prob)), dtype=torch.uint8, device=dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rays = _lib.rays(x=outs[0], y=outs[1], cx=outs[2], cy=outs[3], ok=flags[0], back=flags[1], moments=mom)
    seeds = _lib.seeds(g_moments=gmom, g_stacks=gstk)
    grads = _lib.grads(g_c=g_c, g_t=g_t, g_mu=g_mu, g_z=g_z, g_cx=g_cx, g_cy=g_cy, g_kappa=g_kap, g_poly=g_pol,
                       g_x_in=gxin, g_y_in=gyin)
    _lib.check(lib.tl_trace_fwd(C.byref(prob), rays, _lib.ptr(ws), ws.numel(), st), "tl_trace_fwd")
    _lib.check(lib.tl_trace_bwd_from_outputs(C.byref(prob), seeds, rays, grads, _lib.ptr(ws), ws.numel(), st),
               "tl_trace_bwd_from_outputs")
    torch.cuda.synchronize()
    # (no ill-conditioned live ray, every ray alive: the walk-back kernel did this launch, not its checkpoint fallback)
    assert mom[:, 9].sum().item() == 0 and bool(flags[0].all())
    return dict(x=gxin.cpu().numpy(), y=gyin.cpu().numpy(), par=gpar.cpu().numpy())


def main():
    out_path, lam = sys.argv[1], float(sys.argv[2])
    a = fan(**CHUNK_FAN)
    res = {}
    for loss in LOSSES:
        g, inv = run_gpu(a, loss, lam)
        assert inv, f"{loss}: the host did not take the walk-back"
        for n, v in g.items():
            res[f"{loss}.{n}"] = v
        for n, v in run_cabi(a, loss).items():
            res[f"{loss}.cabi.{n}"] = v
    np.savez(out_path, **res)


if __name__ == "__main__":
    main()
