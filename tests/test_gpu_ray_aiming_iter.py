"""tl_ray_aim_iter -- n_ray_aiming_iter Newton steps of ray aiming in one launch -- against tl_ray_aim (N = 1, bit for bit),
the CPU fp64 restatement (aim_iter_ref.py), the public metric, the op-sequence fallback, the oracle's gradients, the fp64
path and a captured HIP graph."""
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIELDS4 = (0., 0.5, 0.707, 1.)
CDF = ("C", "d", "F")


@pytest.fixture(scope="module")
def ta():
    import torchoptics_amd
    from torchoptics_amd import _lib
    _lib.lib()
    return torchoptics_amd


def _mb():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import minibatch_loss as mb
    return mb


def _case(name):
    """(lens, specs) on the GPU, no gradient."""
    import yaml_free_lenses as L
    from torchoptics_amd import lens_modeling as lm, prescriptions as P
    if name.startswith("dg"):
        la, sa, _ = P.double_gauss(DEV, requires_grad=False, aspheres=True)
        ls, ss, _ = P.double_gauss(DEV, requires_grad=False)
        return {"dg_asph": (la, sa), "dg_sph": (ls, ss), "dg_wide": (ls, lm.Specs(ls.structure, ss.epd * 3.2, ss.hfov))}[name]
    if name == "cooke_wide":
        lens, specs, _ = L.build("cooke", DEV, grad=False, epd=12.0, hfov_deg=32.0)
    else:
        lens, specs, _ = L.build(name, DEV, grad=False)
    return lens, specs


def _raw(fn, tr, specs, lens, n_iter=None, tee_ref=None, rs=None):
    """Call tl_ray_aim (n_iter None) or tl_ray_aim_iter on the arguments RayTracer._ray_aiming_kernel builds; [3,B,F,W]."""
    from torchoptics_amd import _lib, ops
    from torchoptics_amd.lens_modeling import const_tensor
    from torchoptics_amd.paraxial import compute_pupil_position
    from torchoptics_amd.ray_tracing import _LINES, _dense
    specs2, front = specs.up_to_stop(), lens.detach().up_to_stop()
    B, K = front.c.shape
    F, W = len(tr.rel_fields), len(tr.wavelengths)
    with torch.no_grad():
        n = _dense(front.get_refractive_indices(tr.wavelengths))
        n_d = _dense(front.get_refractive_indices([_LINES["d"]]))
        z = _dense(compute_pupil_position(lens.detach(), tr.arith, front=front))
    c, t = _dense(front.c), _dense(front.t)
    mask = _dense(front.structure.mask_torch.view(torch.uint8))
    kap = pol = kind = None
    if getattr(front, "kappa", None) is not None:
        kap, pol = _dense(front.kappa.detach().float()), _dense(front.poly.detach().float())
        kind = ((kap != 0) | (pol != 0).any(dim=-1)).to(torch.uint8)
    fields = const_tensor(list(tr.rel_fields), torch.float32, c.device)
    hfov, epd = _dense(specs2.hfov.float()), _dense(specs2.epd.float())
    out = torch.full((3, B, F, W), float("nan"), dtype=torch.float32, device=c.device)
    P = _lib.ptr
    head = (0, B, F, W, K, P(c), P(t), P(n), P(n_d), P(mask), P(kap), P(pol), P(kind), P(z), P(hfov), P(fields), P(epd), 1)
    with ops._on_device(c.device):
        if n_iter is None:
            rc = _lib.lib().tl_ray_aim(*head, P(out[0]), P(out[1]), P(out[2]), ops._stream_ptr(c.device))
        else:
            rc = _lib.lib().tl_ray_aim_iter(*head, n_iter, P(tee_ref), P(rs), P(out[0]), P(out[1]), P(out[2]),
                                            ops._stream_ptr(c.device))
    _lib.check(rc, fn)
    torch.cuda.synchronize()
    return out


def _tracer(ta, fields=FIELDS4, wl=CDF, n_iter=1, **kw):
    return ta.RayTracer(mode="circular", n_rays=(16, 16), rel_fields=fields, wavelengths=wl, n_ray_aiming_iter=n_iter,
                        default_device=DEV, **kw)


# ------------------------------------------------------------------ 1. N = 1 is tl_ray_aim bit for bit
@pytest.mark.parametrize("name", ["cooke", "tessar", "doublet", "cooke_wide", "dg_asph", "dg_sph", "dg_wide"])
def test_one_step_equals_the_one_step_kernel_bit_for_bit(ta, name):
    lens, specs = _case(name)
    tr = _tracer(ta)
    a = _raw("tl_ray_aim", tr, specs, lens)
    b = _raw("tl_ray_aim_iter", tr, specs, lens, n_iter=1)
    assert torch.isfinite(a).all()
    assert torch.equal(a, b)
    assert a.view(torch.int32).eq(b.view(torch.int32)).all()          # signed zeros included


def test_one_step_equals_the_one_step_kernel_on_a_padded_minibatch(ta):
    mb = _mb()
    st, specs, leaves, _ = mb.build_batch(64, DEV)
    lens = ta.Lens(st, leaves["c"], leaves["t"], leaves["nd"], leaves["v"])
    tr = ta.RayTracer(mode="circular", n_rays=(8, 8), rel_fields=mb.FIELDS, wavelengths=mb.WAVELENGTHS, n_ray_aiming_iter=1,
                      default_device=DEV)
    a = _raw("tl_ray_aim", tr, specs, lens)
    b = _raw("tl_ray_aim_iter", tr, specs, lens, n_iter=1)
    assert a.shape == (3, 64, 8, 3) and torch.isfinite(a).all()
    assert a.view(torch.int32).eq(b.view(torch.int32)).all()


# ------------------------------------------------------------------ 2. N >= 2 against the fp64 restatement
def _restated(name, tr, n_iter, **kw):
    import aim_iter_ref as R
    import yaml_free_lenses as L
    from torchoptics_amd import lens_modeling as lm, prescriptions as P
    if name == "dg_wide":
        ls, ss, _ = P.double_gauss("cpu", requires_grad=False)
        lens, specs = ls, lm.Specs(ls.structure, ss.epd * 3.2, ss.hfov)
    elif name == "cooke_wide":
        lens, specs, _ = L.build("cooke", "cpu", grad=False, epd=12.0, hfov_deg=32.0)
    else:
        lens, specs, _ = L.build(name, "cpu", grad=False)
    inp = R.inputs(lens, specs, tr.rel_fields, tr.wavelengths)
    return R.aim(inp, n_iter, return_history=True, **kw)


@pytest.mark.parametrize("n_iter", [2, 3, 5])
@pytest.mark.parametrize("name", ["cooke", "tessar", "doublet"])
def test_iterated_map_matches_the_fp64_restatement(ta, name, n_iter):
    lens, specs = _case(name)
    tr = _tracer(ta)
    got = _raw("tl_ray_aim_iter", tr, specs, lens, n_iter=n_iter).cpu().double()
    want, _, dead = _restated(name, tr, n_iter)
    assert not any(bool(d.any()) for d in dead)
    for g, w in zip(got, want):
        assert (g - w).abs().max().item() <= 1e-6


def _steps_of(m):
    """Accumulated steps (bottom y, top y, sagittal x) [B,F,W,3] of a map with p0 = (-1, 1, 1)."""
    xs, ys, yo = m
    return torch.stack((yo - ys + 1, ys + yo - 1, xs - 1), dim=-1)


@pytest.mark.parametrize("n_iter", [2, 3, 5])
@pytest.mark.parametrize("name", ["cooke_wide", "dg_wide"])
def test_iterated_map_with_dead_tee_rays(ta, name, n_iter):
    """Tee rays that die take no step: the map stays finite and the rays that never moved are the restatement's."""
    lens, specs = _case(name)
    tr = _tracer(ta)
    got = _raw("tl_ray_aim_iter", tr, specs, lens, n_iter=n_iter).cpu().double()
    want, hist, dead = _restated(name, tr, n_iter)
    assert torch.isfinite(got).all()
    assert any(bool(d.any()) for d in dead)                        # the case does have dead tee rays
    s_got = _steps_of(got)
    s_want = hist[-1].permute(0, 1, 3, 2)                          # [B,F,W,3]
    never_ref = torch.stack(dead).all(dim=0).permute(0, 1, 3, 2)   # dead at every step: never moved
    # (steps recovered from the fp32 map: exact zeros come back as |s| < 1e-7)
    assert never_ref.any() and (s_got[never_ref].abs() < 1e-7).all()
    assert ((s_got.abs() >= 1e-7) | never_ref | (s_want.abs() < 1e-6)).all()
    live = ~torch.stack(dead).any(dim=0).any(dim=2)               # (lens, field, wavelength) whose tee rays all lived
    assert live.any()
    for g, w in zip(got, want):
        assert (g - w)[live].abs().max().item() <= 1e-6


# ------------------------------------------------------------------ 3. convergence through the public metric
def test_ray_aiming_error_falls_with_the_iterations(ta):
    import yaml_free_lenses as L
    lens, specs, _ = L.build("cooke", DEV, grad=False)
    err = {n: ta.metrics.compute_ray_aiming_error(specs, lens, (0.5, 0.707, 1.), n_ray_aiming_iter=n, default_device=DEV)
           for n in (1, 2, 3)}
    e = {n: v.abs().max().item() for n, v in err.items()}
    assert e[1] >= 5e-3 and e[3] <= 2e-5 and e[2] < e[1], e


# ------------------------------------------------------------------ 4. kernel against the op-sequence fallback
def _aimed(tr, specs, lens, kernel):
    from torchoptics_amd import ray_tracing as rt
    rt.set_ray_aiming_kernel(kernel)
    try:
        with torch.no_grad():
            a = tr.assemble(specs, lens)
    finally:
        rt.set_ray_aiming_kernel(True)
    return a["x"], a["y"]


def _close(k, r, tol=2e-5):
    (xk, yk), (xr, yr) = k, r
    assert xk.shape == xr.shape and torch.isfinite(xk).all() and torch.isfinite(yk).all()
    assert (xk - xr).abs().max().item() < tol * xr.abs().max().item()
    assert (yk - yr).abs().max().item() < tol * yr.abs().max().item()


@pytest.mark.parametrize("n_iter", [2, 3])
@pytest.mark.parametrize("name", ["cooke", "tessar", "doublet"])
def test_kernel_matches_the_op_sequence_real(ta, name, n_iter):
    lens, specs = _case(name)
    tr = _tracer(ta, n_iter=n_iter)
    _close(_aimed(tr, specs, lens, True), _aimed(tr, specs, lens, False))


def _fan_of_map(tr, specs, m, vig=False):
    """What RayTracer.assemble traces for a given map (remap, clamp, scale_to_epd) on the 16 x 16 circular grid."""
    from torchoptics_amd import ray_tracing as rt
    xp, yp = rt.circle(None, 16, 16, DEV)
    if vig:
        yp, xp = tr._vignette(specs, yp, xp)
    xs, ys, yo = (v[:, :, None, :] for v in m)
    return rt.scale_to_epd(torch.clamp(xp * xs, -2, 2), specs.epd), rt.scale_to_epd(torch.clamp(yp * ys + yo, -2, 2), specs.epd)


@pytest.mark.parametrize("name", ["cooke", "tessar"])
def test_paraxial_mode(ta, name):
    from torchoptics_amd.paraxial import compute_magnification
    lens, specs = _case(name)
    tr = _tracer(ta, n_iter=3, ray_aiming_mode="paraxial")
    _close(_aimed(tr, specs, lens, True), _aimed(tr, specs, lens, False))
    tr1 = _tracer(ta, n_iter=1, ray_aiming_mode="paraxial")
    rs = (compute_magnification(lens.up_to_stop()) * specs.up_to_stop().epd / 2).float().contiguous()
    m = _raw("tl_ray_aim_iter", tr1, specs, lens, n_iter=1, rs=rs)
    _close(_fan_of_map(tr1, specs, m), _aimed(tr1, specs, lens, False))


def _vig_specs(specs):
    return dataclasses.replace(specs, vig_up=torch.tensor([0.3], device=DEV), vig_down=torch.tensor([0.1], device=DEV),
                               vig_x=torch.tensor([0.2], device=DEV))


def _lin(fields, v):
    return fields * v[:, None]


@pytest.mark.parametrize("name", ["cooke", "tessar"])
def test_vignetted_aiming(ta, name):
    lens, specs = _case(name)
    sp = _vig_specs(specs)
    tr = _tracer(ta, n_iter=3, vig_fn=_lin)
    k3, r3 = _aimed(tr, sp, lens, True), _aimed(tr, sp, lens, False)
    _close(k3, r3)
    tr0 = _tracer(ta, n_iter=3)
    assert (k3[1] - _aimed(tr0, specs, lens, True)[1]).abs().max().item() > 1e-3      # the vignetting does act
    tr1 = _tracer(ta, n_iter=1, vig_fn=_lin)
    xt0, yt0 = torch.tensor([0., 0., 1.], device=DEV), torch.tensor([-1., 1., 0.], device=DEV)
    shape = (1, len(FIELDS4), 3, 1)
    yv, xv = tr1._vignette(sp, yt0.reshape(1, 1, 3, 1).expand(shape), xt0.reshape(1, 1, 3, 1).expand(shape))
    tee_ref = torch.stack((yv[:, :, 0, 0], yv[:, :, 1, 0], xv[:, :, 2, 0]), dim=-1).float().contiguous()
    m = _raw("tl_ray_aim_iter", tr1, sp, lens, n_iter=1, tee_ref=tee_ref)
    _close(_fan_of_map(tr1, sp, m, vig=True), _aimed(tr1, sp, lens, False))


def test_minibatch_losses_kernel_vs_op_sequence(ta):
    mb = _mb()
    from torchoptics_amd import ray_tracing as rt
    st, specs, leaves, n_seq = mb.build_batch(64, DEV)
    tr = ta.RayTracer(mode="circular", n_rays=(8, 8), rel_fields=mb.FIELDS, wavelengths=mb.WAVELENGTHS, n_ray_aiming_iter=3,
                      default_device=DEV)
    res = []
    for kernel in (True, False):
        rt.set_ray_aiming_kernel(kernel)
        try:
            with torch.no_grad():
                lens = ta.Lens(st, leaves["c"], leaves["t"], leaves["nd"], leaves["v"])
                ld = rt.unsupervised_loss_batch(tr.trace_rays(specs, lens, aggregate="sum"), n_seq, 0.2)
            res.append(ld["loss_unsup"].clone())
        finally:
            rt.set_ray_aiming_kernel(True)
    assert torch.isfinite(res[0]).all()
    assert ((res[0] - res[1]).abs() / res[1].abs()).max().item() < 2e-5


# ------------------------------------------------------------------ 5. gradients on the aimed fan, fp64
def test_gradients_on_the_aimed_fan_match_the_oracle(ta):
    from oracle import trace_oracle as orc
    import yaml_free_lenses as L
    lens, specs, _ = L.build("cooke", DEV, grad=False)
    tr = _tracer(ta, fields=(0., 0.707, 1.), n_iter=3)
    with torch.no_grad():
        a = tr.assemble(specs, lens)
    names = ("x", "y", "z", "cx", "cy", "c", "t", "mu")
    dev = [a[n].detach().contiguous().requires_grad_(n in ("c", "t", "mu")) for n in names]
    cpu = [d.detach().cpu().requires_grad_(d.requires_grad) for d in dev]
    x, y, cx, cy, ok, back = ta.trace_skew(*dev, a["mask"])
    rms = ta.compute_rms2d(x, y, ok)
    rms.backward()
    xr, yr, _, _, okr, _ = orc.trace_skew(*cpu, a["mask"].cpu(), ieee_sqrt=True)
    rms_ref = orc.compute_rms2d(xr, yr, okr)
    rms_ref.backward()
    assert torch.equal(ok.cpu(), okr)
    assert abs(rms.item() - rms_ref.item()) < 1e-7
    for d, c in zip(dev[5:], cpu[5:]):
        assert rel_l2(d.grad.cpu().numpy(), c.grad.numpy()) < 1e-5


def test_double_precision_at_three_steps(ta):
    import yaml_free_lenses as L
    res = {}
    for dp in (False, True):
        lens, specs, leaves = L.build("cooke", DEV)
        tr = _tracer(ta, fields=(0., 0.707, 1.), n_iter=3, double_precision=dp)
        x, y, cx, cy, ok, back = tr.trace_rays(specs, lens)
        rms = ta.compute_rms2d(x, y, ok)
        rms.backward()
        res[dp] = (rms.item(), leaves["c"].grad.clone())
    assert np.isfinite(res[True][0])
    assert abs(res[True][0] - res[False][0]) < 2e-5 * res[False][0]
    assert rel_l2(res[True][1].cpu().numpy(), res[False][1].cpu().numpy()) < 1e-3


# ------------------------------------------------------------------ 6. a captured step
def test_captured_step_replays_the_eager_loss(ta):
    mb = _mb()
    from torchoptics_amd import graphs, ray_tracing as rt
    st, specs, leaves, n_seq = mb.build_batch(16, DEV)
    tr = ta.RayTracer(mode="circular", n_rays=(8, 8), rel_fields=mb.FIELDS, wavelengths=mb.WAVELENGTHS, n_ray_aiming_iter=3,
                      default_device=DEV)

    def step(lv):
        lv["c"].grad = lv["t"].grad = None
        lens = ta.Lens(st, lv["c"], lv["t"], lv["nd"], lv["v"])
        ld = rt.unsupervised_loss_batch(tr.trace_rays(specs, lens, aggregate="sum"), n_seq, 0.2)
        ld["loss_unsup"].sum().backward()
        return ld["loss_unsup"].detach()

    eager = step(leaves).clone()
    # the captured step works on fresh leaves that only ever see the capture stream (graphs.py)
    gc_, gt_ = graphs.fresh_leaves(leaves["c"], leaves["t"])
    gl = dict(leaves, c=gc_, t=gt_)
    g, out = graphs.capture_step(lambda: step(gl), DEV)
    g.replay()
    torch.cuda.synchronize()
    assert torch.isfinite(eager).all()
    assert torch.equal(out, eager)
