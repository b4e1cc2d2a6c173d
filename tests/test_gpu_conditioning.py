"""
Ill-conditioned rays (smallest cos^2 of incidence or refraction below 0.01, counted by moment 9) and the backward.

The walk-back kernels reconstruct every ray from the forward's outputs; for a grazing ray that reconstruction amplifies fp32
rounding by ~1/cos^2, so such rays are differentiated by the checkpoint kernel (bit-faithful re-trace).  With the per-ray
flags the forward leaves (tl_problem.cond_flags: 0 dead, 1 live, 2 live and ill-conditioned) the split is PER RAY: the
walk-back takes the rays marked 1, the checkpoint kernel queued behind it exactly those marked 2, the reduction adds the two
partial sums.  Without the flags (a C caller that passes NULL) one such ray still hands the whole launch to the checkpoint
kernel, bit for bit what tl_trace_bwd gives.

Checker: the oracle's autograd (fp32 as the reference runs it, and fp64) on the reference's own failure-heavy fixture (G5: Cooke
triplet, 35 degree field, grazing rays), gate 2e-5 norm-relative plus the oracle's own fp32-vs-fp64 distance as in
test_gpu_parity.py; the checkpoint algorithm of this library as a second, tighter witness (1e-5).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_golden, rel_l2
from test_oracle_asphere import asphere_params

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IN = ("in_x", "in_y", "in_z", "in_cx", "in_cy", "in_c", "in_t", "in_mu")


@pytest.fixture(scope="module")
def ta():
    import torchoptics_amd
    from torchoptics_amd import _lib
    _lib.lib()
    return torchoptics_amd


def _g5(pupil=None):
    """Fixture G5's lens and fields; pupil: None = its own 32 x 32 grid, an int n = an n x n grid over the same square,
    a slice = a subset of its points (small pupils take the rolled walk-back kernel)."""
    g = load_golden("G5_cooke_failures")
    ins = [torch.from_numpy(g[n]) for n in IN]
    if isinstance(pupil, int):
        lin = torch.linspace(-7.75, 7.75, pupil)
        yy, xx = torch.meshgrid(lin, lin, indexing="ij")
        ins[0], ins[1] = xx.reshape(1, 1, -1, 1).contiguous(), yy.reshape(1, 1, -1, 1).contiguous()
    elif pupil is not None:
        ins[0], ins[1] = ins[0][:, :, pupil].contiguous(), ins[1][:, :, pupil].contiguous()
    return ins, torch.from_numpy(g["in_mask"])


def _grads(ta, ins, mask, algo, mode="strict", aggregate=False, asph=False, hook=None):
    from torchoptics_amd import ops, ray_tracing as rt
    S = ins[5].shape[-1]
    ops.set_backward_algorithm(algo)
    try:
        lv = [ins[i].to(DEV).clone().requires_grad_(True) for i in (2, 4, 5, 6, 7)]
        kw = {}
        if asph:
            kap0, pol0, _ = asphere_params(S)
            lv += [(0.2 * kap0).to(DEV).requires_grad_(True), (0.2 * pol0).to(DEV).requires_grad_(True)]
            kw.update(kappa=lv[5], poly=lv[6])
        x_in, y_in = ins[0].to(DEV), ins[1].to(DEV)
        if aggregate:                       # (the reference's aggregate branch wants the fan broadcast up front)
            F, P, W = ins[4].shape[1], ins[0].shape[2], ins[7].shape[3]
            x_in, y_in = x_in.expand(1, F, P, W), y_in.expand(1, F, P, W)
        out = ta.trace_skew(x_in, y_in, lv[0], ins[3].to(DEV), lv[1], lv[2], lv[3], lv[4], mask.to(DEV),
                            "sum" if aggregate else False, True, mode=mode, **kw)
        n_ill = out[1]._tl_spot[0][:, 9].sum().item()
        loss = ta.compute_rms2d(out[0], out[1], out[4])
        if aggregate:
            loss = loss + 0.2 * rt.penalty_sum(out[6], S)
        if hook:
            hook(out)
        loss.backward()
        return [q.grad.clone() for q in lv], n_ill, ops.used_walk_back(out[0]), int(out[4].sum().item())
    finally:
        ops.set_backward_algorithm("inverse")


@pytest.mark.parametrize("mode", ["strict", "fast"])
@pytest.mark.parametrize("pupil", ["fixture", "small", "dense"])
def test_split_backward_matches_checkpoint_and_oracle_on_the_failure_heavy_fixture(ta, mode, pupil):
    from oracle import trace_oracle as orc
    ins, mask = _g5({"fixture": None, "small": slice(0, 1024, 5), "dense": 192}[pupil])
    got, n_ill, inv, n_ok = _grads(ta, ins, mask, "inverse", mode)
    ck, n_ill2, inv2, _ = _grads(ta, ins, mask, "checkpoint", mode)
    assert inv is True and inv2 is False
    assert n_ill == n_ill2 and 0 < n_ill < n_ok, (n_ill, n_ok)       # some live rays are ill-conditioned, most are not
    want = {}
    for dt in (torch.float32, torch.float64):           # the reference's own precision, and the exact derivative
        cpu = [a.to(dt) for a in ins]
        clv = [cpu[i].clone().requires_grad_(True) for i in (2, 4, 5, 6, 7)]
        o = orc.trace_skew(cpu[0], cpu[1], clv[0], cpu[3], clv[1], clv[2], clv[3], clv[4], mask, False, True)
        orc.compute_rms2d(o[0], o[1], o[4]).backward()
        want[dt] = [q.grad.numpy() for q in clv]
    tol = 2e-5 if mode == "strict" else 2e-4
    for i, nme in enumerate(("z", "cy", "c", "t", "mu")):
        a = got[i].cpu().numpy()
        e_ck, e32, e64 = rel_l2(a, ck[i].cpu().numpy()), rel_l2(a, want[torch.float32][i]), rel_l2(a, want[torch.float64][i])
        noise = rel_l2(want[torch.float32][i], want[torch.float64][i])
        print(f"G5 {pupil} {mode} d/d{nme}: split vs checkpoint {e_ck:.2e}, vs oracle fp32 {e32:.2e} fp64 {e64:.2e} (oracle fp32 "
              f"itself {noise:.2e}; {n_ill:.0f} of {n_ok} live rays flagged)")
        # (rays just above the threshold amplify the walk-back's rounding ~100-fold: allow 1 % of the reference's own fp32
        #  noise on this fan -- d/dz of the dense grid is only good to 2 % in the reference's fp32 itself)
        assert e_ck <= (1e-5 if mode == "strict" else 1e-4) + 0.01 * noise, nme
        # grazing rays: the reference's own fp32 autograd sits `noise` away from the exact derivative (as in test_gpu_parity)
        # (the dense grid over the whole failure square: d/dz is only determined to a few per cent in fp32 at all -- two fp32
        #  evaluations that differ in operation order, the reference's autograd and either kernel here, sit ~3 noise apart)
        assert e32 <= tol or e64 <= tol + (4 if pupil == "dense" else 2) * noise, nme


@pytest.mark.parametrize("asph", [False, True])
def test_split_backward_with_the_penalty_term_and_aspheric_rows(ta, asph):
    """Three kinds of rays in one launch: alive and well-conditioned (walk-back), alive and ill-conditioned, dead on the way
    (both: checkpoint pass) -- with the penalty term, whose gradient the dead rays keep."""
    ins, mask = _g5(64)
    got, n_ill, inv, n_ok = _grads(ta, ins, mask, "inverse", aggregate=True, asph=asph)
    ck, _, inv2, _ = _grads(ta, ins, mask, "checkpoint", aggregate=True, asph=asph)
    n_rays = ins[4].shape[1] * ins[7].shape[3] * ins[0].shape[2]
    assert inv is True and inv2 is False and 0 < n_ill < n_ok < n_rays
    names = ("z", "cy", "c", "t", "mu") + (("kappa", "poly") if asph else ())
    for nme, a, b in zip(names, got, ck):
        e = rel_l2(a.cpu().numpy(), b.cpu().numpy())
        print(f"G5 penalty asph={asph} d/d{nme}: split vs checkpoint {e:.2e}")
        assert torch.isfinite(a).all() and e <= 2e-5, nme


def test_flag_bytes_and_the_c_abi_with_and_without_them(ta):
    """tl_trace_fwd writes cond_flags = ok + (ill-conditioned ? 1 : 0) per ray; tl_trace_bwd_from_outputs reads them in
    place of fwd->ok (which may then be NULL).  Without them the whole launch goes to the checkpoint kernel: the bits of
    tl_trace_bwd.  With them the result differs in the last bits only."""
    from torchoptics_amd import _lib, ops
    ins, mask = _g5()
    dev = [a.to(DEV) for a in ins]
    F, P, W, S = ins[4].shape[1], ins[0].shape[2], ins[7].shape[3], ins[5].shape[-1]
    x_e, y_e = dev[0].expand(1, F, P, W), dev[1].expand(1, F, P, W)
    cond = torch.full((1, F, W, P), 77, dtype=torch.uint8, device=DEV)

    # (tl_problem holds raw pointers: every tensor behind one must outlive the calls -- the fixture's mu is not contiguous)
    keep = [dev[2].reshape(1), dev[3].reshape(1, -1), dev[4].reshape(1, -1).contiguous(), dev[5].reshape(1, S).contiguous(),
            dev[6].reshape(1, S).contiguous(), dev[7].reshape(1, W, S).contiguous(),
            mask.to(DEV).reshape(1, S).view(torch.uint8).contiguous()]

    def problem(c_):
        return ops._problem(x_e, y_e, *keep, True, "strict", cond=c_)
    lib = _lib.lib()
    prob, prob0 = problem(cond), problem(None)
    ws = torch.zeros(lib.tl_workspace_bytes(C.byref(prob)), dtype=torch.uint8, device=DEV)
    outs = [torch.empty((1, F, W, P), dtype=torch.float32, device=DEV) for _ in range(4)]
    flags = [torch.empty((1, F, W, P), dtype=torch.uint8, device=DEV) for _ in range(2)]
    mom = torch.empty((F, _lib.TL_NMOM), dtype=torch.float64, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P_ = _lib.ptr
    out = _lib.rays(x=outs[0], y=outs[1], cx=outs[2], cy=outs[3], ok=flags[0], back=flags[1], moments=mom)
    rc = lib.tl_trace_fwd(C.byref(prob), out, P_(ws), ws.numel(), st)
    assert rc == 0, lib.tl_last_error()
    n_ill = int(mom[:, 9].sum().item())
    assert n_ill > 0
    assert torch.equal(cond != 0, flags[0] != 0) and int(cond.max().item()) == 2
    assert int((cond == 2).sum().item()) == n_ill
    assert torch.equal(flags[0], (flags[0] != 0).to(torch.uint8))             # the ok output itself stays 0 / 1
    gmom = torch.randn((F, _lib.TL_NMOM), dtype=torch.float64, device=DEV, generator=torch.Generator(DEV).manual_seed(5)) * 1e-3
    res = {}
    for tag, pr, okp in (("flags", prob, None), ("flags_and_ok", prob, flags[0]), ("no_flags", prob0, flags[0]), ("bwd", prob0, None)):
        g = [torch.zeros(n, device=DEV) for n in (S, S, W * S, 1, F, F)]
        seeds = _lib.seeds(g_moments=gmom)
        grads = _lib.grads(g_c=g[0], g_t=g[1], g_mu=g[2], g_z=g[3], g_cx=g[4], g_cy=g[5])
        if tag == "bwd":
            rc = lib.tl_trace_bwd(C.byref(pr), seeds, grads, P_(ws), ws.numel(), st)
        else:
            fwd = _lib.rays(x=outs[0], y=outs[1], cx=outs[2], cy=outs[3], ok=okp, moments=mom)
            rc = lib.tl_trace_bwd_from_outputs(C.byref(pr), seeds, fwd, grads, P_(ws), ws.numel(), st)
        assert rc == 0, (tag, lib.tl_last_error())
        res[tag] = torch.cat([q.reshape(-1) for q in g])
    assert torch.equal(res["no_flags"], res["bwd"])
    assert torch.equal(res["flags"], res["flags_and_ok"])
    assert not torch.equal(res["flags"], res["bwd"])                           # the walk-back really took the other rays
    assert rel_l2(res["flags"].cpu().numpy(), res["bwd"].cpu().numpy()) < 1e-5
    # fwd->ok is only optional when the flags are there
    g = [torch.zeros(n, device=DEV) for n in (S, S, W * S, 1, F, F)]
    fwd = _lib.rays(x=outs[0], y=outs[1], cx=outs[2], cy=outs[3], moments=mom)
    rc = lib.tl_trace_bwd_from_outputs(C.byref(prob0), _lib.seeds(g_moments=gmom), fwd,
                                       _lib.grads(g_c=g[0], g_t=g[1], g_mu=g[2], g_z=g[3], g_cx=g[4], g_cy=g[5]),
                                       P_(ws), ws.numel(), st)
    assert rc != 0


def test_split_backward_under_saved_tensor_hooks_and_both_host_chains(ta):
    """The flag bytes are a saved tensor of the autograd node like the forward's outputs: offloaded and restored by
    save_on_cpu they reach the backward in other storage; both host chains give the same bits."""
    from torchoptics_amd import ops
    ins, mask = _g5()
    base, n_ill, _, _ = _grads(ta, ins, mask, "inverse")
    assert n_ill > 0
    res = {}
    for chain in ("cpp", "python"):
        ops.set_host_chain(chain)
        try:
            with torch.autograd.graph.save_on_cpu():
                res[chain] = _grads(ta, ins, mask, "inverse")[0]
        finally:
            ops.set_host_chain("cpp")
    for a, b, c_ in zip(base, res["cpp"], res["python"]):
        assert torch.equal(a, b) and torch.equal(a, c_)


def test_a_few_grazing_rays_no_longer_cost_the_walk_back(ta):
    """Performance contract of the split: a 3 x 3 x 2^20-ray fan with a few hundred ill-conditioned rays (the outer field
    pushed to 30 degrees: ~0.005 % of the rays graze the last surface) runs its backward in about the time of the same fan
    without them (outer field 26.7 degrees), not in the checkpoint kernel's (~1.8 x).  Timed with the library's own events."""
    from torchoptics_amd import ops
    ins, mask = _g5(1024)
    ins[0], ins[1] = ins[0] * 0.5, ins[1] * 0.5
    times = {}
    for tag, cy_max in (("clean", 0.45), ("few_ill", 0.5)):
        ins[4] = torch.tensor([0.0, 0.3, cy_max]).reshape(1, 3, 1, 1)
        _grads(ta, ins, mask, "inverse")                      # warm-up
        ops.enable_timing(True)
        try:
            for _ in range(5):
                _, n_ill, inv, n_ok = _grads(ta, ins, mask, "inverse")
            times[tag] = (ops.timing_ms()["bwd"], n_ill, n_ok)
        finally:
            ops.enable_timing(False)
    (t0, ill0, _), (t1, ill1, ok1) = times["clean"], times["few_ill"]
    print(f"backward of 3 x 3 x 2^20 rays: no flagged ray {t0:.3f} ms; {ill1:.0f} flagged of {ok1} live {t1:.3f} ms")
    assert ill0 == 0 and 0 < ill1 < 1e-3 * ok1
    assert t1 < 1.4 * t0
