"""The kernels that turn rays into the number Adam minimises -- spot_moments_kernel, reduce_moments_kernel / sum_rows,
spot_seed_kernel, spot_rms_kernel, unsup_loss_kernel, unsup_loss_bwd_kernel, aim_fan_kernel (csrc/tl_api.hip) -- against
plain fp64 references on the CPU, across tensor layouts, launch plans, field and lens counts, degenerate fields and fp64 rays.
The shapes, the exact (dyadic) inputs and the restated launch plan are in tests/spot_cases.py; their premises are checked
without a GPU by tests/test_spot_cases_cpu.py.

Tolerances: the moments and seeds of the dyadic inputs are exact, so those tests ask for equality.  rms and penalty returned in
fp32 are fp64 numbers rounded once: 2^-23 relative (2^-22 where the closed form's cancellation adds to it), the penalty of
dyadic sums bit-equal; loss_unsup is two more fp32 operations on those two, checked exactly; a gradient element in fp32 is an
fp64 number rounded once: rel-L2 2^-23; the fp64 gradient with respect to the moments: rel-L2 1e-12."""
import functools
import itertools
import math

import numpy as np
import pytest
import torch

import spot_cases as sc
from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NMOM = sc.NMOM


@pytest.fixture(scope="module")
def ta():
    import torchoptics_amd
    from torchoptics_amd import _lib, ops
    _lib.lib()
    assert ops.host_chain() == "cpp", "the C++ host extension (_tlx.so) is not built / does not load"
    return torchoptics_amd


def _chains(fn):
    """[fn('cpp'), fn('python')], each under that host chain."""
    from torchoptics_amd import ops
    res = []
    for chain in ("cpp", "python"):
        ops.set_host_chain(chain)
        try:
            assert ops.host_chain() == chain
            res.append(fn(chain))
        finally:
            ops.set_host_chain("cpp")
    return res


# ================================================================================= 3.1 moments and seeds at op level
@functools.lru_cache(maxsize=2)
def _case(shape, expanded=False, dead_at_zero=True):
    """Inputs and references of one shape, computed once for all its layouts."""
    F, W, P = shape
    x, y, ok = sc.rays(F, W, P, expanded, dead_at_zero)
    g = sc.seeds(F)
    gx_ref, gy_ref = sc.reference_seeds(x, y, ok, g)
    return x, y, ok, sc.reference_moments(x, y, ok), sc.reference_moments(None, y, ok), g, gx_ref, gy_ref


def _dense_strides(shape):
    return torch.empty(shape, device="meta").stride()


def _check_op(shape, layout, ok_dtype=torch.bool, ray_dtype=torch.float32, dead_at_zero=True):
    from torchoptics_amd import ops
    F, W, P = shape
    x, y, ok, m_ref, m_ref_nox, g, gx_ref, gy_ref = _case(shape, layout == "y_expanded", dead_at_zero)
    has_x = layout != "x_none"
    yd = sc.lay_out(y.to(DEV, ray_dtype), layout, "y").requires_grad_(True)
    xd = sc.lay_out(x.to(DEV, ray_dtype), layout, "x").requires_grad_(True) if has_x else None
    okd = sc.lay_out(ok.to(DEV), layout, "ok").to(ok_dtype) if ok_dtype != torch.bool else sc.lay_out(ok.to(DEV), layout, "ok")
    mom = ops.SpotMomentsFunction.apply(xd, yd, okd)
    assert mom.shape == (F, NMOM) and mom.dtype == torch.float64
    want = m_ref if has_x else m_ref_nox
    got = mom.detach().cpu()
    assert torch.equal(got[:, :7], want[:, :7]), f"moments differ in columns {sorted(set((got != want).nonzero()[:, 1].tolist()))}"
    assert (got[:, 7:] == 0).all()
    grads = torch.autograd.grad(mom, [yd] + ([xd] if has_x else []), g.to(DEV))
    # the seeds come back laid out like the y the kernel read: y's own strides, or dense where the op had to copy y
    as_is = ray_dtype == torch.float32 and layout != "y_expanded"
    strides = yd.stride() if as_is else _dense_strides(yd.shape)
    for name, got_g, want_g in zip(("gy", "gx"), grads, (gy_ref, gx_ref)):
        assert got_g.shape == yd.shape and got_g.dtype == ray_dtype
        assert got_g.stride() == strides, (name, got_g.stride(), strides)
        assert torch.equal(got_g.cpu(), want_g.to(ray_dtype)), name


@pytest.mark.parametrize("shape,layout", list(itertools.product(sc.SHAPES, sc.LAYOUTS)),
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_moments_and_seeds_equal_the_fp64_reference(ta, shape, layout):
    _check_op(shape, layout)


@pytest.mark.parametrize("ok_dtype", [torch.bool, torch.uint8, torch.float32], ids=str)
@pytest.mark.parametrize("layout", ["contiguous", "fwp", "ok_contiguous"])
def test_ok_as_bool_bytes_or_floats(ta, ok_dtype, layout):
    _check_op((3, 3, 257), layout, ok_dtype=ok_dtype)


@pytest.mark.parametrize("layout", ["contiguous", "fwp", "slice"])
def test_fp64_rays_are_converted_not_reinterpreted(ta, layout):
    """The op itself takes any float type and sums the fp32 values (the dyadic inputs are the same numbers in fp64)."""
    _check_op((3, 3, 257), layout, ray_dtype=torch.float64)


@pytest.mark.parametrize("layout", ["contiguous", "fwp"])
def test_dead_rays_off_the_origin(ta, layout):
    """sum y (all rays) and sum ok y (live rays) differ only when a dead ray is not at the origin."""
    _check_op((3, 3, 257), layout, dead_at_zero=False)


def test_gx_is_absent_when_x_needs_no_gradient(ta, monkeypatch):
    from torchoptics_amd import ops
    x, y, ok, m_ref, _, g, gx_ref, gy_ref = _case((3, 3, 257))
    seen = []
    real = ops._call

    def spy(name, dev, *args, **kw):
        if name == "tl_spot_seed":
            seen.append(args[-2:])                  # (gx, gy)
        return real(name, dev, *args, **kw)
    monkeypatch.setattr(ops, "_call", spy)
    for x_grad in (False, True):
        xd, yd = x.to(DEV).requires_grad_(x_grad), y.to(DEV).requires_grad_(True)
        mom = ops.SpotMomentsFunction.apply(xd, yd, ok.to(DEV))
        assert torch.equal(mom.cpu(), m_ref)
        (mom * g.to(DEV)).sum().backward()
        gx, gy = seen[-1]
        assert (gx is not None) == x_grad and gy is not None
        assert torch.equal(yd.grad.cpu(), gy_ref)
        assert (xd.grad is None) if not x_grad else torch.equal(xd.grad.cpu(), gx_ref)
    assert len(seen) == 2


# ================================================================================= 3.2 public metrics on real-valued rays
def _gauss_spots(B, F, P, W, seed, dead_at_zero):
    """Gaussian spots of 1e-2 mm at field heights 0 ... 3 mm, 10 % of the rays dead: (x, y, ok) [B,F,P,W] on the CPU."""
    gen = torch.Generator().manual_seed(seed)
    h = torch.linspace(0.0, 3.0, F).view(1, F, 1, 1) if F > 1 else torch.full((1, 1, 1, 1), 3.0)
    y = (h + 1e-2 * torch.randn(B, F, P, W, generator=gen)).float()
    x = (0.05 + 0.7e-2 * torch.randn(B, F, P, W, generator=gen)).float()
    ok = torch.rand(B, F, P, W, generator=gen) >= 0.1
    if dead_at_zero:
        y[~ok] = 0
        x[~ok] = 0
    return x, y, ok


def _two_pass(x, y, ok, xy=False):
    """[B] fp64: the definition -- per field the centroid over ALL rays, the squared distances of the live rays to it over
    the count of all rays, the root; the mean over fields."""
    n = y.shape[2] * y.shape[3]
    d2 = (y - y.mean((2, 3), keepdim=True)) ** 2
    if xy:
        d2 = d2 + (x - x.mean((2, 3), keepdim=True)) ** 2
    return torch.sqrt((d2 * ok).sum((2, 3)) / n).mean(1)


def _to_dev(t, permuted):
    t = t.to(DEV)
    return t.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2) if permuted else t.contiguous()


GATE_VALUE, GATE_GRAD = 2.0 ** -22, 2.0 ** -23


@pytest.mark.parametrize("dead_at_zero", [True, False], ids=["dead-at-origin", "dead-in-place"])
@pytest.mark.parametrize("permuted", [False, True], ids=["contiguous", "permuted"])
@pytest.mark.parametrize("metric,B", [("rms2d", 1), ("rms_spot_xy", 1), ("rms2d_batch", 3), ("rms2d_batch", 70)])
def test_public_metrics_against_the_two_pass_definition(ta, metric, B, permuted, dead_at_zero):
    from oracle import trace_oracle as orc
    from torchoptics_amd import ray_tracing as rt
    F, P, W = 4, 300, 3
    x, y, ok = _gauss_spots(B, F, P, W, 100 * B + 7, dead_at_zero)
    x64, y64 = x.double().requires_grad_(True), y.double().requires_grad_(True)
    if metric == "rms2d":
        want = orc.compute_rms2d(x64, y64, ok)
        assert abs(_two_pass(x64, y64, ok)[0].item() - want.item()) <= 1e-13 * want.item()       # the analogue below is the same form
    else:
        want = _two_pass(x64, y64, ok, xy=metric == "rms_spot_xy")
        want = want[0] if metric == "rms_spot_xy" else want
    want.sum().backward()
    xd, yd, okd = _to_dev(x, permuted).requires_grad_(True), _to_dev(y, permuted).requires_grad_(True), _to_dev(ok, permuted)
    fn = {"rms2d": rt.compute_rms2d, "rms_spot_xy": rt.compute_rms_spot_xy, "rms2d_batch": rt.compute_rms2d_batch}[metric]
    got = fn(xd, yd, okd)
    assert got.dtype == torch.float32 and got.shape == want.shape
    got.sum().backward()
    e_val = ((got.detach().cpu().double() - want.detach()).abs() / want.detach()).max().item()
    e_gy = rel_l2(yd.grad.cpu().numpy(), y64.grad.numpy())
    e_gx = rel_l2(xd.grad.cpu().numpy(), x64.grad.numpy()) if metric == "rms_spot_xy" else 0.0
    print(f"SPOT-ACC {metric} B={B} {'permuted' if permuted else 'contiguous'} "
          f"{'dead-at-origin' if dead_at_zero else 'dead-in-place'}: value {e_val:.3e} (gate {GATE_VALUE:.3e}) "
          f"d/dy {e_gy:.3e} d/dx {e_gx:.3e} (gate {GATE_GRAD:.3e})")
    assert e_val <= GATE_VALUE
    assert e_gy <= GATE_GRAD and e_gx <= GATE_GRAD
    assert yd.grad.stride() == yd.stride()
    if metric != "rms_spot_xy":
        assert xd.grad is None or (xd.grad == 0).all()                  # compute_rms2d reads y only


# ================================================================================= 3.3 spot_rms and unsup_loss on synthetic moments
RATE = 0.2
N_RAYS = (16, 2)            # P, W of the synthetic fans: 32 rays per field


@functools.lru_cache(maxsize=None)
def _moments(B, F):
    """[B F, NMOM] fp64 on the CPU: the moments of B F dyadic fans summed on the CPU, a dyadic penalty sum in column 8 (exact
    in any order of summation), and junk in the columns these kernels must not read (7, 9)."""
    P, W = N_RAYS
    x, y, ok = sc.rays(B * F, W, P)
    m = sc.reference_moments(x, y, ok)
    rng = np.random.default_rng(B * 1000 + F)
    m[:, 8] = torch.from_numpy(rng.integers(0, 1 << 16, size=B * F).astype(np.float64) / 1024)
    m[:, 7], m[:, 9] = 5.0, 3.0
    return m


def _n_seq(kind, B):
    if kind == "int":
        return 7
    return torch.tensor([5.0 + (b % 4) for b in range(B)], dtype=torch.float64)


def _reference_loss(m, B, F, n, n_seq):
    """(loss, rms, penalty, rms in fp64) of the op sequence rms_from_moments / rms + rate * (q / n_seq).to(float32) per lens in
    torch fp64 on the CPU, with the op sequence's rounding points: rms and penalty rounded to fp32, the loss formed in fp32.
    (A Python number divides a GPU tensor as a multiplication by its reciprocal -- the kernel's documented rounding point for
    an int n_sequence -- so that is how the reference divides by one.)"""
    mm = m.view(B, F, NMOM)
    mean = mm[..., 0] / n
    var = (mm[..., 2] - 2 * mean * mm[..., 1] + mean * mean * mm[..., 3]) / n
    rms64 = torch.sqrt(var).mean(1)
    q = mm[..., 8].sum(1)
    pen = (q * (1.0 / n_seq) if isinstance(n_seq, int) else q / n_seq).to(torch.float32)
    rms = rms64.to(torch.float32)
    return rms + RATE * pen, rms, pen, rms64


def _weights(B, dev):
    b = torch.arange(B, dtype=torch.float32, device=dev)
    return 1.0 + 0.25 * (b % 5), -0.5 + 0.125 * (b % 7), 0.125 * (1 + b % 3)


def _upstream(kind, loss, rms, pen):
    """The scalar whose gradient with respect to the moments is taken: one upstream gradient, all three with per-lens weights,
    or a plain sum (an expanded, stride-0 gradient)."""
    w1, w2, w3 = _weights(loss.numel(), loss.device)
    w1, w2, w3 = (w.reshape(loss.shape) for w in (w1, w2, w3))
    return {"loss": (loss * w1).sum(), "rms": (rms * w2).sum(), "penalty": (pen * w3).sum(),
            "all": (loss * w1).sum() + (rms * w2).sum() + (pen * w3).sum(), "sum": loss.sum(),
            "sum-all": loss.sum() + rms.sum() + pen.sum()}[kind]


UPSTREAM = ("loss", "rms", "penalty", "all", "sum", "sum-all")


def _gpu_loss(chain, m, n, B, n_seq):
    """(loss, rms, penalty) per lens on the GPU: tl_unsup_loss under the C++ chain, the op sequence around tl_spot_rms that
    unsupervised_loss_batch composes under the Python one."""
    from torchoptics_amd import ops
    ns = n_seq if isinstance(n_seq, int) else n_seq.to(DEV)
    out = ops.unsup_loss(m, n, B, ns, RATE)
    if chain == "cpp":
        assert out is not None
        return out
    assert out is None
    rms = ops.spot_rms(m, n, B)
    rms = rms.reshape(B) if B > 1 else rms
    q = m[:, 8].view(B, -1).sum(dim=1) if B > 1 else m[:, 8].sum()
    pen = (q / ns).to(torch.float32) if not torch.is_tensor(ns) or B > 1 else (q / ns.reshape(())).to(torch.float32)
    return rms + RATE * pen, rms, pen


@pytest.mark.parametrize("B", [1, 2, 3, 300])
@pytest.mark.parametrize("F", [1, 3, 64, 65, 130])
def test_spot_rms_and_unsup_loss_against_the_fp64_op_sequence(ta, F, B):
    from torchoptics_amd import ops
    n = float(N_RAYS[0] * N_RAYS[1])
    m_cpu = _moments(B, F)
    for kind in ("int", "tensor"):
        n_seq = _n_seq(kind, B)
        mr = m_cpu.clone().requires_grad_(True)
        ref = _reference_loss(mr, B, F, n, n_seq)
        ref_grads = {k: torch.autograd.grad(_upstream(k, *ref[:3]), mr, retain_graph=True)[0] for k in UPSTREAM}

        def run(chain):
            m = m_cpu.to(DEV).requires_grad_(True)
            loss, rms, pen = _gpu_loss(chain, m, n, B, n_seq)
            for t in (loss, rms, pen):
                assert t.dtype == torch.float32 and t.shape == (() if B == 1 else (B,))
            grads = {k: torch.autograd.grad(_upstream(k, loss, rms, pen), m, retain_graph=True)[0] for k in UPSTREAM}
            # tl_spot_rms on its own: its value and its derivative
            r2 = ops.spot_rms(m, n, B).reshape(rms.shape)
            (g2,) = torch.autograd.grad((r2 * _weights(B, DEV)[1].reshape(rms.shape)).sum(), m)
            return loss.detach(), rms.detach(), pen.detach(), grads, g2, r2.detach()
        res = _chains(run)
        for chain, (loss, rms, pen, grads, g2, r2) in zip(("cpp", "python"), res):
            what = f"F={F} B={B} n_seq={kind} {chain}"
            rms_c = rms.cpu().double().reshape(B)
            assert ((rms_c - ref[3].detach()).abs() <= 2.0 ** -23 * ref[3].detach()).all(), what
            assert ((r2.cpu().double().reshape(B) - ref[3].detach()).abs() <= 2.0 ** -23 * ref[3].detach()).all(), what
            assert torch.equal(pen.cpu().reshape(B), ref[2].detach()), what
            # the loss is an fp32 product and an fp32 sum of the two fp32 numbers above (three roundings against fp64, not
            # one): held to those two operations exactly, on the values just checked
            assert torch.equal(loss.cpu(), rms.cpu() + RATE * pen.cpu()), what
            for k in UPSTREAM:
                g = grads[k].cpu()
                assert g.dtype == torch.float64 and g.shape == m_cpu.shape
                e = rel_l2(g.numpy(), ref_grads[k].numpy())
                assert e <= 1e-12, f"{what} upstream={k}: {e:.2e}"
                assert (g[:, 7] == 0).all() and (g[:, 9] == 0).all() and (g[:, 4:7] == 0).all()
            assert rel_l2(g2.cpu().numpy(), ref_grads["rms"].numpy()) <= 1e-12, what
        if (F, B) == (3, 3):
            # one launch each way under the C++ chain = the op sequence under the Python chain, bit for bit
            for a, b in zip(res[0][:3], res[1][:3]):
                assert torch.equal(a, b)
            for k in UPSTREAM:
                assert torch.equal(res[0][3][k], res[1][3][k]), k


# ================================================================================= 3.4 degenerate fields
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=str)
def test_one_dead_field_among_live_ones(ta, dtype):
    """Field 2 of 4 all dead: rms = 3/4 of the mean over the live fields, no gradient on the dead field's rays, and the
    gradient of the live fields' rays is what it is when field 2 is alive (a field's term depends on its own rays only)."""
    from oracle import trace_oracle as orc
    from torchoptics_amd import ray_tracing as rt
    x, y, ok = _gauss_spots(1, 4, 300, 3, 31, True)
    live = [0, 1, 3]
    y_dead, ok_dead = y.clone(), ok.clone()
    y_dead[:, 2], ok_dead[:, 2] = 0, False
    y64 = y[:, live].double().requires_grad_(True)
    want = 0.75 * orc.compute_rms2d(None, y64, ok[:, live])
    want.backward()
    res = {}
    for name, yy, oo in (("dead", y_dead, ok_dead), ("alive", y, ok)):
        yd = yy.to(DEV, dtype).requires_grad_(True)
        rms = rt.compute_rms2d(None, yd, oo.to(DEV))
        rms.backward()
        res[name] = (rms.item(), yd.grad.cpu())
    rms, g = res["dead"]
    assert abs(rms - want.item()) <= 2.0 ** -23 * want.item()
    assert torch.isfinite(g).all()
    assert (g[:, 2] == 0).all()
    assert torch.equal(g[:, live], res["alive"][1][:, live])
    assert rel_l2(g[:, live].numpy(), y64.grad.numpy()) <= (2.0 ** -23 if dtype == torch.float32 else 1e-9)


def _check_degenerate(rms, bound, what):
    rms = rms.detach().cpu().double().reshape(-1)
    assert torch.isfinite(rms).all(), f"{what}: {int((~torch.isfinite(rms)).sum())} of {rms.numel()} not finite"
    assert (rms >= 0).all() and (rms <= bound).all(), what


@pytest.mark.parametrize("name", ["n3", "n5", "n7", "n48", "n777", "mixed"])
def test_coincident_rays_give_zero_not_nan(ta, name):
    """2048 lenses of one field whose rays all coincide, in ONE launch: the closed form M2 - 2 m M1 + m^2 M3 cancels to a
    small NEGATIVE number for part of them (tests/test_spot_cases_cpu.py proves that for these very moments), and a root of
    it would make the lens' whole rms NaN.  Every rms must be finite, >= 0 and below the rounding noise sqrt(16 2^-53 M2 / n),
    every derivative finite -- through tl_spot_rms, through tl_unsup_loss and through the torch closed forms on fp64 tensors on
    the GPU and on the CPU."""
    from torchoptics_amd import ops, ray_tracing as rt
    m_np, n = {k: (m, n) for k, m, n in sc.coincident_sets()}[name]
    B = m_np.shape[0]
    m_cpu = torch.from_numpy(m_np)
    bound = torch.sqrt(16 * 2.0 ** -53 * m_cpu[:, 2] / n)

    def kernels(chain):
        m = m_cpu.to(DEV).requires_grad_(True)
        rms = ops.spot_rms(m, float(n), B)
        _check_degenerate(rms, bound, f"{name} spot_rms {chain}")
        (g,) = torch.autograd.grad(rms.sum(), m)
        assert torch.isfinite(g).all(), f"{name} spot_rms {chain}: d_moments"
        if chain == "cpp":
            m8 = m_cpu.clone()
            m8[:, 8] = 1.5
            m8 = m8.to(DEV).requires_grad_(True)
            loss, rms, pen = ops.unsup_loss(m8, float(n), B, 8, RATE)
            _check_degenerate(rms, bound, f"{name} unsup_loss")
            assert torch.equal(loss, rms + RATE * pen) and torch.isfinite(loss).all()
            (g,) = torch.autograd.grad(loss.sum() + rms.sum(), m8)
            assert torch.isfinite(g).all(), f"{name} unsup_loss: d_moments"
    _chains(kernels)
    # the torch closed forms (fp64 callers), fed through the tag that trace_skew leaves on its y: every lens its own rms ...
    for dev in (DEV, "cpu"):
        m = m_cpu.clone().to(dev)
        m[:, 4:7] = m[:, 0:3]                                         # the same spot in x
        m.requires_grad_(True)
        y = torch.zeros(B, 1, 1, 1, dtype=torch.float64, device=dev)
        ok = torch.ones(B, 1, 1, 1, dtype=torch.bool, device=dev)
        y._tl_spot = rt._SpotTag(m, ok, y._version, n, True)
        per_lens = rt.compute_rms2d_batch(None, y, ok)
        _check_degenerate(per_lens, bound, f"{name} compute_rms2d_batch {dev}")
        (g,) = torch.autograd.grad(per_lens.sum(), m)
        assert torch.isfinite(g).all(), f"{name} compute_rms2d_batch {dev}: d_moments"
        # ... and the B moments rows read as the fields of one lens: a mean over fields, NaN if any field is
        yf = torch.zeros(1, B, 1, 1, dtype=torch.float64, device=dev)
        okf = torch.ones(1, B, 1, 1, dtype=torch.bool, device=dev)
        yf._tl_spot = rt._SpotTag(m, okf, yf._version, n, True)
        for fn, scale in ((rt.compute_rms2d, 1.0), (rt.compute_rms_spot_xy, math.sqrt(2.0))):
            r = fn(None, yf, okf)
            assert r.dtype == torch.float64
            _check_degenerate(r, scale * bound.mean(), f"{name} {fn.__name__} {dev}")
            (g,) = torch.autograd.grad(r, m)
            assert torch.isfinite(g).all(), f"{name} {fn.__name__} {dev}: d_moments"
        assert rt.rms_from_moments(m.detach(), n).item() == rt.compute_rms2d(None, yf, okf).item()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=str)
def test_coincident_rays_end_to_end(ta, dtype):
    """The same through the rays: 2048 fields of 777 coincident rays each, untagged, through tl_spot_moments (fp32) or the
    fp64 sums, the three public metrics and their gradients."""
    from torchoptics_amd import ray_tracing as rt
    v = torch.from_numpy(sc.coincident_values()).to(dtype)
    F, P = v.numel(), 777
    y = v.view(1, F, 1, 1).expand(1, F, P, 1).contiguous()
    ok = torch.ones(1, F, P, 1, dtype=torch.bool)
    ok[:, ::3, ::5] = False                          # dead rays at the same point: the centroid stays there
    bound = math.sqrt(16 * 2.0 ** -53 * float((v.double() ** 2).max()))
    for fn in (rt.compute_rms2d, rt.compute_rms_spot_xy, rt.compute_rms2d_batch):
        yd = y.to(DEV).requires_grad_(True)
        xd = (0.5 * y).to(DEV).requires_grad_(True)
        if fn is rt.compute_rms2d_batch:
            r = fn(xd.view(F, 1, P, 1), yd.view(F, 1, P, 1), ok.to(DEV).view(F, 1, P, 1))
        else:
            r = fn(xd, yd, ok.to(DEV))
        assert r.dtype == dtype
        assert torch.isfinite(r).all() and (r >= 0).all() and (r <= 2 * bound).all(), fn.__name__
        r.sum().backward()
        assert torch.isfinite(yd.grad).all(), fn.__name__
        if fn is rt.compute_rms_spot_xy:
            assert torch.isfinite(xd.grad).all()


# ================================================================================= 3.5 fp64 rays without a tag
def test_fp64_rays_that_lost_their_tag_keep_fp64_accuracy(ta):
    """RayTracer(double_precision=True), then any op on y: the spot metrics must still be those of the fp64 rays (the generic
    path used to round x and y to fp32 before summing)."""
    import yaml_free_lenses as L
    from oracle import trace_oracle as orc
    from test_gpu_batch import _batch
    from torchoptics_amd import ray_tracing as rt
    kw = dict(mode="circular", n_rays=(16, 16), rel_fields=(0., 0.707, 1.), wavelengths=("C", "d", "F"),
              double_precision=True, default_device=DEV)
    lens, specs, leaves = L.build("cooke", DEV)
    x, y, cx, cy, ok, back = ta.RayTracer(**kw).trace_rays(specs, lens)
    assert y.dtype == torch.float64 and rt._spot_tag(y, ok) is not None
    xc, yc, okc = x.detach().cpu(), y.detach().cpu(), ok.cpu()
    oracle = {"rms2d": orc.compute_rms2d(xc, yc, okc).item(), "rms_spot_xy": _two_pass(xc, yc, okc, xy=True)[0].item()}
    for metric, fn in (("rms2d", rt.compute_rms2d), ("rms_spot_xy", rt.compute_rms_spot_xy)):
        tagged = fn(x, y, ok)
        y2 = y * 1.0
        assert rt._spot_tag(y2, ok) is None
        untagged = fn(x * 1.0, y2, ok)
        assert untagged.dtype == torch.float64
        e_tag = abs(untagged.item() - tagged.item()) / tagged.item()
        e_orc = abs(untagged.item() - oracle[metric]) / oracle[metric]
        print(f"SPOT-ACC fp64-untagged {metric}: vs tagged {e_tag:.3e} vs oracle {e_orc:.3e} (gate 1e-10)")
        assert e_tag <= 1e-10 and e_orc <= 1e-10, (metric, e_tag, e_orc)
        ga = torch.autograd.grad(tagged, [leaves["c"], leaves["t"]], retain_graph=True)
        gb = torch.autograd.grad(untagged, [leaves["c"], leaves["t"]], retain_graph=True)
        for k, a, b in zip("ct", ga, gb):
            e = rel_l2(b.cpu().numpy(), a.cpu().numpy())
            print(f"SPOT-ACC fp64-untagged {metric} d/d{k}: vs tagged {e:.3e} (gate 1e-9)")
            assert e < 1e-9, (metric, k, e)
    # the padded two-lens batch
    lens, specs, leaves = _batch(DEV)
    x, y, cx, cy, ok, back = ta.RayTracer(**kw).trace_rays(specs, lens)
    tagged = rt.compute_rms2d_batch(x, y, ok)
    untagged = rt.compute_rms2d_batch(x * 1.0, y * 1.0, ok)
    want = _two_pass(x.detach().cpu(), y.detach().cpu(), ok.cpu())
    assert untagged.dtype == torch.float64 and untagged.shape == (2,)
    e_tag = ((untagged - tagged).abs() / tagged).max().item()
    e_orc = ((untagged.detach().cpu() - want).abs() / want).max().item()
    print(f"SPOT-ACC fp64-untagged rms2d_batch: vs tagged {e_tag:.3e} vs two-pass {e_orc:.3e} (gate 1e-10)")
    assert e_tag <= 1e-10 and e_orc <= 1e-10
    w = torch.tensor([1.0, 0.5], dtype=torch.float64, device=DEV)
    ga = torch.autograd.grad((tagged * w).sum(), [leaves["c"], leaves["t"]], retain_graph=True)
    gb = torch.autograd.grad((untagged * w).sum(), [leaves["c"], leaves["t"]])
    for k, a, b in zip("ct", ga, gb):
        e = rel_l2(b.cpu().numpy(), a.cpu().numpy())
        print(f"SPOT-ACC fp64-untagged rms2d_batch d/d{k}: vs tagged {e:.3e} (gate 1e-9)")
        assert e < 1e-9, (k, e)


# ================================================================================= 3.6 tl_aim_fan on ragged fans
FANS = [("meridional", (1,)), ("meridional", (255,)), ("meridional", (257,)), ("meridional", (1000,)),
        ("circular", (1, 1)), ("circular", (15, 17)), ("circular", (257, 1)), ("circular", (25, 40))]


def _check_fan(aim, epd, xp, yp, shape):
    from torchoptics_amd import ray_tracing as rt
    xp, yp = 2.5 * xp, 2.5 * yp                               # beyond the clamp for part of the fan
    fx, fy = aim.fan(xp, yp, epd)
    ox, oy = (rt.scale_to_epd(torch.clamp(v, -2, 2), epd) for v in aim(xp, yp))
    assert fx.shape == ox.shape == shape and fy.shape == shape
    assert fx.stride(2) == 1 and fy.stride(2) == 1            # consecutive pupil points are contiguous
    assert torch.equal(fx, ox) and torch.equal(fy, oy)
    assert torch.isfinite(fx).all() and torch.isfinite(fy).all()


@pytest.mark.parametrize("kind,args", FANS, ids=[k + "-" + "x".join(map(str, a)) for k, a in FANS])
def test_one_launch_fan_on_ragged_fans(ta, kind, args):
    """tl_aim_fan bit for bit against remap, clamp, scale_to_epd for pupil counts that are not one full block: 1, 255, 257 and
    1000 points on a line and on a polar grid."""
    import yaml_free_lenses as L
    from torchoptics_amd import ray_tracing as rt
    lens, specs, _ = L.build("cooke", DEV, grad=False, epd=12.0, hfov_deg=30.0)
    tr = ta.RayTracer(mode="circular", n_rays=(16, 16), rel_fields=(0., 0.5, 0.707, 1.), wavelengths=("C", "d", "F"),
                      n_ray_aiming_iter=1, default_device=DEV)
    aim = tr.ray_aiming(specs, lens.detach(), True)
    assert callable(getattr(aim, "fan", None))
    xp, yp = rt.meridional_uniform(None, *args, DEV) if kind == "meridional" else rt.circle(None, *args, DEV)
    P = int(np.prod(args))
    assert P in (1, 255, 257, 1000) and xp.shape == (1, 1, P, 1)
    _check_fan(aim, specs.epd, xp, yp, (1, 4, P, 3))
    if P > 1:
        assert any((torch.clamp(v, -2, 2) != v).any() for v in aim(2.5 * xp, 2.5 * yp))


@pytest.mark.parametrize("P", [1, 257, 1000])
def test_one_launch_fan_on_a_lens_batch_with_its_own_pupil_diameters(ta, P):
    from test_gpu_batch import _batch
    import yaml_free_lenses as L
    from torchoptics_amd import lens_modeling as lm, ray_tracing as rt
    lens, specs, _ = _batch(DEV)
    specs = lm.Specs(lens.structure, torch.tensor([L.EPD, 1.25 * L.EPD], dtype=torch.float32, device=DEV), specs.hfov.detach())
    tr = ta.RayTracer(mode="circular", n_rays=(16, 16), rel_fields=(0., 0.707, 1.), wavelengths=("C", "d", "F"),
                      n_ray_aiming_iter=1, default_device=DEV)
    aim = tr.ray_aiming(specs, lens.detach(), True)
    assert callable(getattr(aim, "fan", None))
    xp, yp = rt.meridional_uniform(None, P, DEV)
    _check_fan(aim, specs.epd, xp, yp, (2, 3, P, 3))
    fy = aim.fan(xp, yp, specs.epd)[1]
    if P > 1:
        assert not torch.equal(fy[0], fy[1])


# ================================================================================= 3.7 untagged batch and the row limit of one launch
def test_untagged_batch_at_and_above_the_row_limit_of_one_launch(ta):
    """compute_rms2d_batch on rays without a tag reads the fields of all lenses as one list: B F W rows of one launch, whose
    grid takes 65535.  At the limit the values are the per-lens definition; one row above it the call raises and names the limit
    -- it never returns numbers."""
    from torchoptics_amd import ray_tracing as rt
    F, P, W = 1, 4, 3
    for B in (21845, 21846):                                      # B F W = 65535, 65538
        x, y, ok = _gauss_spots(B, F, P, W, 5, True)
        xd, yd, okd = x.to(DEV).clone(), y.to(DEV).clone(), ok.to(DEV).clone()
        if B * F * W <= 65535:
            got = rt.compute_rms2d_batch(xd, yd, okd)
            want = _two_pass(x.double(), y.double(), ok)
            assert got.shape == (B,) and torch.isfinite(got).all()
            assert ((got.cpu().double() - want).abs() <= 2.0 ** -22 * want).all()
        else:
            with pytest.raises(RuntimeError, match="65535"):
                rt.compute_rms2d_batch(xd, yd, okd)
    # B F W = 65536 exactly, as two wavelengths
    x, y, ok = _gauss_spots(16384, 2, 4, 2, 6, True)
    with pytest.raises(RuntimeError, match="65535"):
        rt.compute_rms2d_batch(x.to(DEV).clone(), y.to(DEV).clone(), ok.to(DEV).clone())
