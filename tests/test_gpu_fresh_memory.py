"""Every kernel gives the same bits whatever its buffers held before ("what every entry point may assume about its
buffers").

Each case runs forward and backward on the Python host chain with every uninitialised allocation of the package, and the
shared workspace at every hand-out, holding 0x00, then 0x7F (a huge finite number), then 0xFF (NaN; 255 in a flag byte) --
tests/fresh_memory.py -- and everything it returns must be the same bytes under the three.  Before that, two runs under 0x00
must agree: all of these ops are documented and tested as bit-reproducible, and a difference between fills would mean nothing
otherwise.  The cases and their `run` helpers are the ones of the accuracy tests (the smallest shapes with partial tiles, dead
elements and odd strides: the shapes at which a write is skipped), so nothing here has a reference of its own: the accuracy
tests say the numbers are right, this module says they do not depend on what the memory held.

Per case, so that none passes vacuously: allocations were soiled in the forward, and in the backward where the op has one;
the workspace was handed out (and so refilled) where the op asks for one; and every tensor an autograd node of ops returned
lies inside a soiled allocation, except the entries of EXEMPT, which torch ops produce.

One line per case:  FRESH-MEM <family> <case>  allocations soiled <fwd>/<bwd>  workspace refills <k>  bytes compared <N>
identical under 00/7F/FF  (kept in profiles/fresh_memory.txt).

The C++ host chain (the default) allocates with at::empty inside _tlx.so, which a test cannot intercept, and keeps a cached
workspace of its own that cannot be refilled from Python; it runs the same kernels through the same C ABI.  This module
holds the Python chain only.
"""
import numpy as np
import pytest
import torch

import fresh_memory as fm

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

# Tensors a node of ops returns that lie in no soiled allocation -- each one the result of a torch op, not of a kernel.
EXEMPT = {
    ("SpotRmsFunction", "backward", 0): "dm * g: a torch multiply of the saved derivative (tl_spot_rms wrote dm in the forward)",
    ("TraceFunction", "backward", 3): "fold(): torch.sum of g_cx over the lenses / fields cx is broadcast over",
    ("TraceFunction", "backward", 4): "fold(): torch.sum of g_cy over the lenses / fields cy is broadcast over",
}


@pytest.fixture(scope="module")
def ta():
    import torchoptics_amd
    from torchoptics_amd import _lib
    _lib.lib()
    return torchoptics_amd


def _flat(out, prefix=""):
    """A helper's result (nested dicts / lists of arrays, tensors, None and other things) as {path: array | tensor | None};
    numbers, strings and pointers are left out."""
    flat = {}
    if isinstance(out, dict):
        items = out.items()
    elif isinstance(out, (list, tuple)):
        items = enumerate(out)
    else:
        items = ()
        if out is None or torch.is_tensor(out) or isinstance(out, np.ndarray):
            flat[prefix or "value"] = _host(out)
    for k, v in items:
        if "ptr" in str(k):
            continue
        flat.update(_flat(v, f"{prefix}.{k}" if prefix else str(k)))
    return flat


def _host(t):
    """A tensor on the host with its bits as they are (a bool through its bytes: fresh_memory.logical_bytes)."""
    if not torch.is_tensor(t):
        return t
    t = t.detach()
    return (t.view(torch.uint8) if t.dtype == torch.bool else t).cpu()


def hold(family, case, run, ws=True, bwd=True):
    """`run()` under 0x00 twice, then 0x7F, then 0xFF, on the Python host chain: the conditions of the module docstring, the
    FRESH-MEM line, and the same bytes throughout.  Returns the last run."""
    from torchoptics_amd import ops
    runs, soils = [], []
    for byte in (fm.FILLS[0],) + fm.FILLS:
        with fm.soiled(byte) as soil:
            ops.set_host_chain("python")
            out = _flat(run())
            torch.cuda.synchronize()
        runs.append(out)
        soils.append(soil)
    tag = f"{family} {case}"
    assert any(v is not None for v in runs[0].values()), tag
    for soil in soils:
        n_fwd, n_bwd = soil.counts()
        assert n_fwd > 0, f"{tag}: no allocation was soiled in the forward"
        if bwd:
            assert soil.backward_at is not None and n_bwd > 0, f"{tag}: no allocation was soiled in the backward"
        if ws:
            assert soil.handouts > 0, f"{tag}: the workspace was never handed out"
        assert soil.misplaced(EXEMPT) == [], f"{tag}: returned tensors outside every soiled allocation"
    assert [s.counts() for s in soils[1:]] == [soils[0].counts()] * 3 and len({s.handouts for s in soils}) == 1, tag
    twice = fm.same_bytes(runs[:2])
    assert twice, f"{tag}: two runs under 0x00 differ -- {twice}"
    cmp = fm.same_bytes(runs[1:])
    n_fwd, n_bwd = soils[-1].counts()
    if cmp:
        print(fm.report_line(family, case, n_fwd, n_bwd, soils[-1].handouts, cmp.nbytes))
    assert cmp, f"{tag}: 0x7F is run 1, 0xFF run 2 -- {cmp}"
    return runs[-1]


# ============================================================================================== the harness on the device
def test_the_fills_reach_device_memory_and_a_skipped_element_shows(ta):
    """What tests/test_fresh_memory_cpu.py shows on the host, on the GPU: the allocations and the workspace hold the byte when
    the op gets them (the gaps of a strided layout too), and `hold` reports an op that leaves one element unwritten."""
    from torchoptics_amd import ops
    dev = torch.device(DEV)
    for byte in fm.FILLS:
        with fm.soiled(byte) as soil:
            t = ops.torch.empty_strided((4, 5), (8, 1), dtype=torch.float32, device=dev)
            ws = ops._workspace(4096, dev)
            assert (fm.storage_bytes(t) == byte).all() and fm.storage_bytes(t).numel() == 4 * 29
            assert (ws == byte).all() and ws.numel() >= 1 << 20
            ws.zero_()
            assert (ops._workspace(64, dev) == byte).all() and soil.handouts == 2
    x = torch.linspace(-3, 3, 37, device=dev)

    def leaves_one_out():
        out = ops.torch.empty(37, dtype=torch.float32, device=dev)
        out[:23] = x[:23] * 2
        out[24:] = x[24:] * 2
        return dict(out=out)
    with pytest.raises(AssertionError, match=r"in 1 element\(s\), first \[23\]"):
        hold("harness", "leaves one out", leaves_one_out, ws=False, bwd=False)


# =================================================================================================================== trace
TRACE_LENSES = [(S, v) for S in (3, 13, 21) for v in ("sph", "asph")]
LAM = 0.2


def _some_dead(tag, ok):
    ok = np.asarray(ok)
    assert ok.size and not ok.all() and ok.any(), f"{tag}: the fan must hold live rays and rays that die part-way"


def _run_sum(ta, a, S, mode):
    """km._run_gpu's one-lens penalty loss with aggregate='sum' (the fused sums only, no per-surface stacks)."""
    import test_gpu_kernel_matrix as km
    from torchoptics_amd import ray_tracing as rt
    names = km._LEAVES + (("kappa", "poly") if a["rows"] else ())
    lv = {n: a[n].to(DEV).clone().requires_grad_(True) for n in names}
    kw = {}
    if a["rows"]:
        kw = dict(kappa=lv["kappa"], poly=lv["poly"], surf_kind=torch.tensor(a["kind"], dtype=torch.bool, device=DEV))
    out = ta.trace_skew(a["x"].to(DEV), a["y"].to(DEV), lv["z"], a["cx"].to(DEV), lv["cy"], lv["c"], lv["t"], lv["mu"],
                        a["mask"].to(DEV), "sum", True, mode=mode, **kw)
    rms, q = ta.compute_rms2d(out[0], out[1], out[4]), rt.penalty_sum(out[6], S)
    (rms + LAM * q).backward()
    return dict(fwd=[_host(t) for t in out[:6]], rms=rms.detach().cpu(), q=q.detach().cpu(),
                grads={n: lv[n].grad.detach().cpu() for n in names})


def _run_stacks(ta, a, mode, algo, w):
    """test_gpu_stacks_grad._gpu with its per-element seed on the three stacks; the stacks themselves are kept too (the
    gradient of a weighted sum of them does not depend on what they hold)."""
    import test_gpu_stacks_grad as sg
    stacks = {}

    def loss(out, rt):
        stacks.update({key: _host(torch.stack(list(out[6][key]), 0)) for key in sg.KEYS})
        return sg._stack_loss(out[6], w)
    grads, inv = sg._gpu(ta, a, mode, algo, loss)
    return dict(grads=grads, stacks=stacks)


@pytest.mark.parametrize("S,variant", TRACE_LENSES, ids=[f"S{s}-{v}" for s, v in TRACE_LENSES])
def test_trace_fp32(ta, S, variant):
    """Rows 3 (unrolled walk-back), 13 (past kInvUnrollPairMin) and 21 (rolled), plain and aspheric, at the small pupil: the rms
    loss under both backward algorithms, the penalty through per-element seeds on the three stacks and as the fused sum
    (under the walk-back the checkpoint kernel is queued behind it and the reduction merges two partial layouts), each strict
    and fast; dense seeds x alone and y + cy (three, two null seed pointers)."""
    import seed_cases as sc
    import test_gpu_kernel_matrix as km
    import test_gpu_seed_matrix as sm
    import test_gpu_stacks_grad as sg
    P = km.P_SMALL
    a = sc.fan(S, variant, P)
    w = sg._weights(S, a["x"].shape, 1000 + S)
    for mode in ("strict", "fast"):
        for algo in ("inverse", "checkpoint"):
            got = hold("trace", f"S{S}-{variant} rms {mode} {algo}",
                       lambda: km._run_gpu(ta, [a], S, variant, False, 0.0, mode, algo))
            _some_dead(f"S{S}-{variant}", got["fwd.4"])
        for algo in ("inverse", "checkpoint") if mode == "strict" else ("inverse",):
            got = hold("trace", f"S{S}-{variant} stacks-seed {mode} {algo}", lambda: _run_stacks(ta, a, mode, algo, w))
            assert got["stacks.z_RELU"].shape[0] == S
        hold("trace", f"S{S}-{variant} penalty-sum {mode}", lambda: _run_sum(ta, a, S, mode))
    turned = sc.lens_of(S, variant, P)
    wts = sc.weights(turned["x"].shape, 4000 + 10 * S + len(turned["rows"]))
    for loss in ("x", "y+cy"):
        got = hold("trace", f"S{S}-{variant} dense-seed {loss}",
                   lambda: sm._run_gpu(ta, [turned], variant, loss, "strict", "inverse", wts))
        _some_dead(f"S{S}-{variant} turned", got["fwd.4"])


@pytest.mark.parametrize("variant", ("sph", "asph"))
def test_trace_fp32_input_gradients_and_lens_batch(ta, variant):
    """x_in, y_in requiring a gradient (row 3: g_x_in, g_y_in are uninitialised buffers whose dead rays must come back zero),
    and a batch of three lenses in one launch (row 13)."""
    import seed_cases as sc
    import test_gpu_kernel_matrix as km
    import test_gpu_seed_matrix as sm
    P = km.P_SMALL
    turned = sc.lens_of(3, variant, P)
    wts = sc.weights(turned["x"].shape, 4030 + len(turned["rows"]))
    got = hold("trace", f"S3-{variant} x_in,y_in rms+all",
               lambda: sm._run_gpu(ta, [turned], variant, "rms+all", "strict", "inverse", wts, need_xy=True))
    dead = np.asarray(got["fwd.4"]) == 0
    assert dead.any() and not np.asarray(got["grads.x"])[dead].any() and not np.asarray(got["grads.y"])[dead].any()
    fan3 = sc.fan(13, variant, P, len(km.BATCH_W))
    lenses = [km._perturbed(fan3, b) for b in range(len(km.BATCH_W))]
    for algo in ("inverse", "checkpoint"):
        got = hold("trace", f"S13-{variant} batch-of-3 rms {algo}",
                   lambda: km._run_gpu(ta, lenses, 13, variant, False, 0.0, "strict", algo, weights=km.BATCH_W))
        _some_dead(f"S13-{variant} batch", got["fwd.4"])


def test_trace_fp32_more_aspheric_rows_than_hit_slots(ta):
    """asph5: five aspheric rows, four hit slots -- the walk-back hands the lens to the checkpoint kernel on the device."""
    import seed_cases as sc
    import test_gpu_kernel_matrix as km
    a = sc.fan(16, "asph5", km.P_SMALL)
    for algo in ("inverse", "checkpoint"):
        got = hold("trace", f"S16-asph5 rms strict {algo}", lambda: km._run_gpu(ta, [a], 16, "asph5", False, 0.0, "strict", algo))
        _some_dead("S16-asph5", got["fwd.4"])


@pytest.mark.parametrize("S,variant,P", [(5, "sph", 777), (13, "asph", 777)], ids=["S5-sph", "S13-asph"])
def test_trace_fp32_optical_path_length(ta, S, variant, P):
    """OPD with a path-length seed (opd_cases' host-chain cases at rows 5 and 13): g_n_index is one more uninitialised leaf."""
    import opd_cases as oc
    import test_gpu_opd_matrix as om
    a = oc.lens_case(S, variant, P)
    refs = [dict(args=a, names=oc.leaf_names(a))]
    got = hold("trace", f"S{S}-{variant} opd path", lambda: om._run(ta, refs, "path", "strict"))
    _some_dead(f"opd S{S}-{variant}", got["fwd.4"])
    assert got["grads.n_index"] is not None


def _run_f64(ta, a):
    """The fp64 twin (what RayTracer(double_precision=True) selects: float64 arguments to trace_skew) on a fan of
    test_gpu_kernel_matrix, rms loss."""
    names = ("z", "cy", "c", "t", "mu") + (("kappa", "poly") if a["rows"] else ())
    lv = {n: a[n].double().to(DEV).clone().requires_grad_(True) for n in names}
    kw = {}
    if a["rows"]:
        kw = dict(kappa=lv["kappa"], poly=lv["poly"], surf_kind=torch.tensor(a["kind"], dtype=torch.bool, device=DEV))
    out = ta.trace_skew(a["x"].double().to(DEV), a["y"].double().to(DEV), lv["z"], a["cx"].double().to(DEV), lv["cy"], lv["c"],
                        lv["t"], lv["mu"], a["mask"].to(DEV), False, True, **kw)
    assert out[0].dtype == torch.float64
    rms = ta.compute_rms2d(out[0], out[1], out[4])
    rms.backward()
    return dict(fwd=[_host(t) for t in out[:6]], rms=rms.detach().cpu(), grads={n: lv[n].grad.detach().cpu() for n in names})


@pytest.mark.parametrize("S,variant", [(S, v) for S in (3, 13) for v in ("sph", "asph")], ids=lambda v: str(v))
def test_trace_fp64_twin(ta, S, variant):
    import seed_cases as sc
    import test_gpu_kernel_matrix as km
    a = sc.fan(S, variant, km.P_SMALL)
    got = hold("trace-f64", f"S{S}-{variant} rms", lambda: _run_f64(ta, a))
    _some_dead(f"f64 S{S}-{variant}", got["fwd.4"])


# ==================================================================================================================== spot
SPOT = [(shape, layout) for shape in [(3, 3, 1), (3, 3, 63), (3, 3, 257), (3, 3, 1000)] for layout in ("contiguous", "slice")]


def _run_spot(shape, layout):
    """SpotMomentsFunction on the case in its layout (dead rays at the origin), SpotRmsFunction on its moments, and the loss
    composition the Python chain has where the C++ chain calls tl_unsup_loss (ops.unsup_loss returns None here)."""
    import spot_cases as sc
    import test_gpu_spot_kernels as sk
    from torchoptics_amd import ops
    F, W, P = shape
    x, y, ok = sc.rays(F, W, P, False, True)
    yd = sc.lay_out(y.to(DEV), layout, "y").requires_grad_(True)
    xd = sc.lay_out(x.to(DEV), layout, "x").requires_grad_(True)
    okd = sc.lay_out(ok.to(DEV), layout, "ok")
    mom = ops.SpotMomentsFunction.apply(xd, yd, okd)
    rms = ops.SpotRmsFunction.apply(mom, float(P * W))
    loss, rms2, pen = sk._gpu_loss("python", mom, float(P * W), 1, 7)
    gy, gx = torch.autograd.grad((mom * sc.seeds(F).to(DEV)).sum() + rms + loss, [yd, xd])
    return dict(moments=mom, rms=rms, loss=loss, rms2=rms2, pen=pen, gy=gy, gx=gx)


@pytest.mark.parametrize("shape,layout", SPOT, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_spot(ta, shape, layout):
    got = hold("spot", f"{'x'.join(map(str, shape))} {layout}", lambda: _run_spot(shape, layout))
    assert got["moments"].shape == (shape[0], 10) and torch.isfinite(got["gy"]).all()


# =================================================================================================================== focus
FOCUS = ("one-ray", "wave-plus-one", "block-edge", "multi-partial", "dead-row", "lens-batch", "layout-slice", "layout-expand")


@pytest.mark.parametrize("name", FOCUS)
def test_focus(ta, name):
    import focus_cases as FC
    import test_gpu_focus as tf
    rays, g = FC.rays(name), FC.g_moments(name)
    got = hold("focus", name, lambda: tf._run(rays, name, g))
    if name == "dead-row":
        assert not np.asarray(got["0"])[0, 0, 0].any(), "a row of dead rays gives written zeros"


# ===================================================================================================================== psf
PSF = [("one-ray", None), ("sub-wave", None), ("block-edge", None), ("reduce-17", None), ("dead-channel", None),
       ("sweep", 1), ("sweep", 13), ("sweep", 32)]


@pytest.mark.parametrize("name,nxh", PSF, ids=[n if k is None else f"{n}-{k}" for n, k in PSF])
def test_psf(ta, name, nxh):
    import psf_cases as pc
    from torchoptics_amd import ops
    a = pc.sweep_inputs(nxh) if name == "sweep" else pc.inputs(name)
    got = hold("psf", name if nxh is None else f"sweep-nxh{nxh}", lambda: pc.run(ops, pc.tensors(a, DEV), a))
    assert all(got[k] is not None for k in ("hist", "gx", "gy", "g_x_pitch", "g_y_pitch", "g_y_centre"))
    if name == "dead-channel":
        g, w = pc.DEAD_CHANNEL
        assert not got["hist"][g, w].any() and not got["gx"][g, w].any(), "a dead channel gives written zeros"


ROT = [("one-ray", None), ("shared", None), ("wave-plus-one", None), ("block-edge", None), ("reduce", None), ("dead-channel", None),
       ("sweep", 1), ("sweep", 13), ("sweep", 32)]


@pytest.mark.parametrize("name,nx", ROT, ids=[n if k is None else f"{n}-{k}" for n, k in ROT])
def test_psf_rot(ta, name, nx):
    import psf_rot_ref as pr
    from torchoptics_amd import ops
    a = pr.inputs(("sweep", nx) if name == "sweep" else name)
    got = hold("psf-rot", name if nx is None else f"sweep-nx{nx}", lambda: pr.run(ops, pr.tensors(a, DEV), a))
    assert all(got[k] is not None for k in ("hist", "gx", "gy", "g_y_centre"))
    if name == "shared":
        unread = sorted(set(range(a.shape[0])) - set(a.src.tolist()))
        assert unread == [2], "fan 2 is read by no grid"
        for k in ("gx", "gy", "g_y_centre"):
            assert not got[k][2].any(), f"{k} of the fan no grid reads: written zeros"


# =================================================================================================================== svola
SVOLA = ("1-odd-hann", "2-taps31", "3-tiles-hann", "4-cover3", "5-shared-psfs", "6-degenerate", "16-halo-is-image",
         "17-halo-overlap-limit", "19-crowded")


@pytest.mark.parametrize("name", SVOLA)
def test_svola(ta, name):
    import svola_ref as ref
    import test_gpu_svola as ts
    from svola_cases import CASES
    from torchoptics_amd import imaging
    B, H, W, Cc, grid, k, ov, win, pb = CASES[name]
    image, psfs, g_out = (t.float().double() for t in ref.make_case(B, H, W, Cc, grid, k, seed=len(name), psf_batch=pb))
    got = hold("svola", name, lambda: ts._fused(imaging, image, psfs, g_out, ov, grid, win))
    assert got["1"] is not None and got["2"] is not None, "gradients to the image and to the PSFs"


# ==================================================================================================================== warp
WARP = ("general", "no-gain", "shared", "thin-row", "thin-col", "tiny", "one")
WARP_IMAGE = ("sparse", "pile-up", "range", "outliers")


@pytest.mark.parametrize("name", WARP)
def test_warp(ta, name):
    import warp_cases as wc
    from torchoptics_amd import imaging
    args = wc.inputs(name)
    got = hold("warp", name, lambda: wc.run(imaging, args, DEV, torch.float32, True, needs=("x", "y", "gain")), ws=False)
    assert {"out", "g_x", "g_y"} <= set(got) and ("g_gain" in got) == (args[3] is not None)


@pytest.mark.parametrize("name", WARP_IMAGE)
def test_warp_image_gradient(ta, name):
    """image_grad='fused': the clear-then-atomics fixed-point accumulator of tl_warp_bwd_image lives in the workspace."""
    import warp_image_cases as wic
    from torchoptics_amd import imaging
    args = wic.inputs(name)
    got = hold("warp-image", name, lambda: wic.run(imaging, args, DEV, image_grad="fused", needs=("image",)))
    assert got["g_image"] is not None


# ==================================================================================================================== ssim
NEEDS = (("a",), ("b",), ("a", "b"))
SSIM = ("one_pixel", "thin_band", "map_17x33", "map_31x33", "k5_L255", "constant", "channel_slice", "transposed")
MS_SSIM = ("top_1x1", "odd_every_level", "map_17x33", "image_33x65", "one_level", "channel_slice")


@pytest.mark.parametrize("name", SSIM)
def test_ssim(ta, name):
    import ssim_cases as sc
    from torchoptics_amd import imaging
    for needs in NEEDS:
        got = hold("ssim", f"{name} needs {'+'.join(needs)}", lambda: sc.run(imaging, name, DEV, torch.float32, True, needs=needs))
        assert [got["g_a"] is not None, got["g_b"] is not None] == ["a" in needs, "b" in needs]


@pytest.mark.parametrize("name", MS_SSIM)
def test_ms_ssim(ta, name):
    import ms_ssim_cases as mc
    from torchoptics_amd import imaging
    for needs in NEEDS:
        got = hold("ms-ssim", f"{name} needs {'+'.join(needs)}", lambda: mc.run(imaging, name, DEV, torch.float32, True, needs=needs))
        assert [got["g_a"] is not None, got["g_b"] is not None] == ["a" in needs, "b" in needs]


# ================================================================================================ pupil position and aiming
AIM = ("cooke-f3w1", "batch6", "asph", "back-mixed", "k1", "k32")


def _aim_tensors(name):
    import aim_cases as C
    a = C.arrays(name)
    f32 = lambda v: torch.as_tensor(np.ascontiguousarray(v)).to(device=DEV, dtype=torch.float32)       # noqa: E731
    return a, {k: f32(a[k]) for k in ("c", "t", "n", "n_d", "z", "hfov", "epd")}


@pytest.mark.parametrize("name", AIM)
def test_pupil_position(ta, name):
    """PupilPositionFunction on the rows in front of the stop of the aiming cases (d line), both arithmetic modes."""
    from torchoptics_amd import ops
    a, t = _aim_tensors(name)
    B = t["c"].shape[0]
    n = torch.cat((torch.ones(B, 1, device=DEV), t["n_d"]), dim=1)
    g_z = 0.5 + 0.25 * torch.arange(B, dtype=torch.float32, device=DEV)

    def run(mode):
        leaves = [v.clone().requires_grad_(True) for v in (t["c"], t["t"], n)]
        z = ops.PupilPositionFunction.apply(*leaves, mode)
        z.backward(g_z)
        return dict(z=z, g=[v.grad for v in leaves])
    for mode in ("strict", "fast"):
        hold("pupil", f"{name} {mode}", lambda: run(mode), ws=False)


class _Front:
    """The rows in front of the stop of an aiming case, as much of a Lens as RayTracer._ray_aiming_kernel reads: c, t, the mask,
    kappa and poly where the case has aspheric rows, and the indices at the tracer's wavelengths (asked for with the tracer's
    own list) or at the d line."""

    def __init__(self, a, t, wavelengths):
        from types import SimpleNamespace
        self.c, self.t, self._n, self._n_d, self._wl = t["c"], t["t"], t["n"], t["n_d"], wavelengths
        self.structure = SimpleNamespace(mask_torch=torch.as_tensor(np.ascontiguousarray(a["mask"]).astype(bool)).to(DEV))
        if a["kind"] is not None:
            self.kappa = torch.as_tensor(a["kappa"]).to(DEV)
            self.poly = torch.as_tensor(a["poly"]).to(DEV)

    def get_refractive_indices(self, wavelengths):
        return self._n if wavelengths is self._wl else self._n_d[..., None]


@pytest.mark.parametrize("n_iter", (1, 2))
@pytest.mark.parametrize("name", AIM)
def test_ray_aiming_and_its_fan(ta, name, n_iter):
    """RayTracer.ray_aiming in its kernel form (tl_ray_aim_iter: the map; its `fan`, tl_aim_fan: the aimed pupil of every lens,
    field and wavelength) on the arrays of the aiming cases; back-mixed holds tee rays that take no step.  x_scale is also
    the one tests/test_gpu_aim_matrix.py reads through the C ABI, bit for bit."""
    import aim_cases as C
    import test_gpu_aim_matrix as am
    from types import SimpleNamespace
    from torchoptics_amd import ray_tracing as rt
    a, t = _aim_tensors(name)
    B, F, W = t["c"].shape[0], len(a["fields"]), a["n"].shape[2]
    tr = ta.RayTracer(mode="circular", n_rays=(4, 4), rel_fields=[float(f) for f in a["fields"]], wavelengths=list(C.CDF[:W]),
                      n_ray_aiming_iter=n_iter, allow_backward_rays=bool(a["allow_backward"]), default_device=DEV)
    front, specs = _Front(a, t, tr.wavelengths), SimpleNamespace(hfov=t["hfov"], epd=t["epd"])
    xp, yp = (2.5 * v for v in rt.circle(None, 15, 17, DEV))          # beyond the fan's clamp for part of the pupil
    one, zero = torch.ones(1, 1, 1, 1, device=DEV), torch.zeros(1, 1, 1, 1, device=DEV)

    def run():
        aim = tr._ray_aiming_kernel(specs, front, z=t["z"])
        fx, fy = aim.fan(xp, yp, t["epd"])
        ax, ay = aim(xp, yp)
        return dict(fan_x=fx, fan_y=fy, x=ax, y=ay, x_scale=aim(one, zero)[0])
    got = hold("aim", f"{name} N={n_iter}", run, ws=False, bwd=False)
    assert got["fan_x"].shape == (B, F, 255, W) and got["x_scale"].shape == (B, F, 1, W)
    want = am._run(name, n_iter)                                   # [3,B,F,W]: x_scale, y_scale, y_offset
    assert np.array_equal(am._bits(got["x_scale"].numpy()[:, :, 0, :]), am._bits(want[0])), "the map of the C-ABI test"


# ===================================================================================================== the pipeline, one stream
def _run_pipeline(ta):
    """The chain of test_gpu_psf_rot.test_leaf_gradients_of_a_rendered_image_through_the_trace at its sizes -- trace, rotated
    PSF grid, svola -- then the bicubic warp with its fused image gradient and 1 - ms_ssim (two levels, 5 taps): six op
    families write over the one workspace between the trace's forward and its backward."""
    import ms_ssim_cases as mc
    import warp_cases as wc
    import yaml_free_lenses as L
    from torchoptics_amd import imaging
    fields = (0.0, 0.6, 1.0)
    cells = imaging.psf_grid_cells((48, 48), (3, 3), 4, fields)
    yy, xx = torch.meshgrid(torch.arange(48, device=DEV), torch.arange(48, device=DEV), indexing="ij")
    img = (((xx // 6 + yy // 6) % 2).float()[None, :, :, None] * torch.tensor([1.0, 0.8, 0.6], device=DEV)).contiguous()
    target = torch.roll(img, 1, dims=2)
    lens, specs, leaves = L.build("cooke", DEV)
    tr = ta.RayTracer(mode="circular", n_rays=(16, 16), rel_fields=fields, wavelengths=("C", "d", "F"), default_device=DEV)
    x, y, cx, cy, ok, back = tr.trace_rays(specs, lens)
    psfs = imaging.psf_grid_from_trace(x, y, ok, cells, (9, 9), 0.004, fused=True)
    out = imaging.svola_convolution(img, 4, psfs, (3, 3), "hann", fused=True)
    d = torch.tensor([wc.BARREL_D], dtype=torch.float32, device=DEV)
    wx, wy = imaging.distortion_grid(d, wc.FIELDS, (48, 48))
    warped = imaging.warp_bicubic(out, wx, wy, None, fused=True, image_grad="fused")
    loss = 1 - imaging.ms_ssim(warped, target, power_factors=mc.power(2), filter_size=5, fused=True)
    loss.sum().backward()
    return dict(loss=loss, c=leaves["c"].grad, t=leaves["t"].grad)


def test_pipeline_on_one_stream(ta):
    got = hold("pipeline", "trace > psf-rot > svola > warp > ms-ssim", lambda: _run_pipeline(ta))
    assert torch.isfinite(got["loss"]).all() and got["c"].abs().sum() > 0 and got["t"].abs().sum() > 0
