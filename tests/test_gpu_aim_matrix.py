"""tl_ray_aim and tl_ray_aim_iter (ray_aim_kernel, ray_aim_iter_kernel and the fp64 trace aim_trace they share) at the C ABI
against the fp64 restatement, element by element, on the cases and with the bound of tests/aim_cases.py: aspheric rows,
allow_backward = 0, padded and mixed batches, K = 1 and 32, W = 1, N = 1, 2 and 16, tee_ref and rs, partly filled waves and
a second block.  Run with -s for the AIM-ACC lines (profiles/aim_accuracy.txt)."""
import numpy as np
import pytest
import torch

import aim_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a, dtype):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype).contiguous()


def _run(name, n_iter):
    """tl_ray_aim (n_iter None) or tl_ray_aim_iter on the arrays of a case: [3,B,F,W] fp32 on the host.  The outputs are
    NaN beforehand, so an element that is not written fails every comparison."""
    from torchoptics_amd import _lib, ops
    a = C.arrays(name)
    B, K, W = a["n"].shape
    F = len(a["fields"])
    f32, u8 = torch.float32, torch.uint8
    c, t, n, n_d, z, hfov, fields, epd = (_dev(a[k], f32) for k in ("c", "t", "n", "n_d", "z", "hfov", "fields", "epd"))
    mask, kind = _dev(a["mask"].astype(np.uint8), u8), _dev(a["kind"], u8)
    kap, pol = _dev(a["kappa"], f32), _dev(a["poly"], f32)
    tee_ref, rs = _dev(a["tee_ref"], f32), _dev(a["rs"], f32)
    assert c.shape == (B, K) and n.shape == (B, K, W) and n_d.shape == (B, K) and mask.shape == (B, K) and z.shape == (B,)
    assert kind is None or (kind.shape == (B, K) and kap.shape == (B, K) and pol.shape == (B, K, 4))
    assert tee_ref is None or (tee_ref.shape == (B, F, 3) and rs.shape == (B,))
    out = torch.full((3, B, F, W), float("nan"), dtype=f32, device=DEV)
    P = _lib.ptr
    dev = torch.device(DEV)
    head = (0, B, F, W, K, P(c), P(t), P(n), P(n_d), P(mask), P(kap), P(pol), P(kind), P(z), P(hfov), P(fields), P(epd),
            int(a["allow_backward"]))
    with ops._on_device(dev):
        if n_iter is None:
            assert tee_ref is None and rs is None
            rc = _lib.lib().tl_ray_aim(*head, P(out[0]), P(out[1]), P(out[2]), ops._stream_ptr(dev))
        else:
            rc = _lib.lib().tl_ray_aim_iter(*head, n_iter, P(tee_ref), P(rs), P(out[0]), P(out[1]), P(out[2]), ops._stream_ptr(dev))
    _lib.check(rc, "tl_ray_aim" if n_iter is None else "tl_ray_aim_iter")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def test_the_cases_use_the_library_limits():
    from torchoptics_amd import _lib
    assert C.MAX_ITER == _lib.TL_MAX_AIM_ITER and C.arrays("k32")["c"].shape[1] == _lib.TL_MAX_SURFACES


@pytest.mark.parametrize("n_iter", C.N_ITERS)
@pytest.mark.parametrize("name", C.CASES)
def test_iterated_aiming_is_within_its_bound(name, n_iter):
    """Every element of the three maps within 2^-24 |want| + A of the central-difference restatement; two runs, same bits."""
    got = _run(name, n_iter)
    q = C.ratio(got, C.want(name, n_iter), C.bound(name, n_iter))
    print(f"AIM-ACC {name} N={n_iter}: largest error / bound  x_scale {q[0]:.3f} y_scale {q[1]:.3f} y_offset {q[2]:.3f}")
    assert (q <= 1).all(), (name, n_iter, q)
    assert np.array_equal(_bits(got), _bits(_run(name, n_iter)))


@pytest.mark.parametrize("name", C.PLAIN)
def test_one_step_kernel_is_within_its_bound_and_is_the_iterated_one_bit_for_bit(name):
    """tl_ray_aim against the same restatement at N = 1, and tl_ray_aim_iter(N = 1) equal to it bit for bit (signed zeros
    too) on every case that needs neither tee_ref nor rs."""
    one, it = _run(name, None), _run(name, 1)
    q = C.ratio(one, C.want(name, 1), C.bound(name, 1))
    print(f"AIM-ACC {name} tl_ray_aim: largest error / bound  x_scale {q[0]:.3f} y_scale {q[1]:.3f} y_offset {q[2]:.3f}")
    assert (q <= 1).all(), (name, q)
    assert np.array_equal(_bits(one), _bits(it))
    assert np.array_equal(_bits(one), _bits(_run(name, None)))


@pytest.mark.parametrize("n_iter", (None,) + C.N_ITERS)
def test_dead_marginal_ray_gives_the_identity_map_exactly(n_iter):
    """back-marginal: nothing steps, and the outputs are the bits of (1.0f, 1.0f, 0.0f).  y_offset is +0.0f, not -0.0f:
    both kernels evaluate (-1 * 0 - 1 * 0) / (-1 - 1) = (-0.0) / (-2.0) = +0.0."""
    got = _run("back-marginal", n_iter)
    want = np.stack([np.ones(got.shape[1:], np.float32), np.ones(got.shape[1:], np.float32), np.zeros(got.shape[1:], np.float32)])
    assert np.array_equal(_bits(got), _bits(want))


# ------------------------------------------------------------------ allow_backward_rays = False through the public API
def _back_lens(t2):
    """The back-mixed (t2 = 1) or back-marginal (t2 = 0.95) front of aim_cases as a Lens: rows G A in front of a stop,
    dispersion-free glass (v = 0), a weak doublet behind the stop so that the lens is a whole one."""
    from torchoptics_amd import lens_modeling as lm
    st = lm.Structure(stop_idx=np.array([2]), sequence=np.array(["GAAGA"]), default_device=DEV)
    f = lambda v: torch.tensor(v, dtype=torch.float32, device=DEV)
    lens = lm.Lens(st, f([0.03, 0.12, 0.0, 0.02, -0.02]), f([1.0, t2, 1.0, 1.0, 10.0]), f([1.6, 1.5]), f([0.0, 0.0]))
    return lens, lm.Specs(st, f([8.0]), f([0.3]))


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
    """test_gpu_ray_aiming_iter's yardstick of the kernel against the op sequence."""
    (xk, yk), (xr, yr) = k, r
    assert xk.shape == xr.shape and torch.isfinite(xk).all() and torch.isfinite(yk).all()
    assert (xk - xr).abs().max().item() < tol * xr.abs().max().item()
    assert (yk - yr).abs().max().item() < tol * yr.abs().max().item()


@pytest.mark.parametrize("n_iter", (1, 3))
@pytest.mark.parametrize("name", ("back-mixed", "back-marginal"))
def test_backward_rays_not_allowed_through_the_public_api(name, n_iter):
    """RayTracer(allow_backward_rays=False) on the two hand-made fronts: the kernel and the sequence of tensor ops aim
    the same fan -- a tee ray (back-mixed) or the marginal ray (back-marginal) that reaches the stop plane from behind is
    flagged, keeps its coordinates, and takes no step in either --, and the fan differs from the one with backward rays
    allowed."""
    import torchoptics_amd as ta
    a = C.arrays(name)
    lens, specs = _back_lens(float(a["t"][0, 1]))
    front = lens.up_to_stop()
    assert torch.equal(front.c.cpu(), torch.tensor(a["c"])) and torch.equal(front.t.cpu(), torch.tensor(a["t"]))
    fans = {}
    for allow in (False, True):
        tr = ta.RayTracer(mode="circular", n_rays=(16, 16), rel_fields=tuple(float(f) for f in a["fields"]), wavelengths=("d",),
                          n_ray_aiming_iter=n_iter, allow_backward_rays=allow, default_device=DEV)
        fans[allow] = _aimed(tr, specs, lens, True)
        _close(fans[allow], _aimed(tr, specs, lens, False))
    assert (fans[False][1] - fans[True][1]).abs().max().item() > 1e-3 * fans[True][1].abs().max().item()
    from torchoptics_amd.paraxial import compute_pupil_position
    assert abs(compute_pupil_position(lens).item() - float(a["z"][0])) < 1e-6          # the case's own pupil position
