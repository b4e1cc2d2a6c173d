"""The fused PSF kernels (tl_psf_accumulate / tl_psf_accumulate_bwd behind metrics.compute_psf(fused=True)) on the GPU.

Oracle: the existing compute_psf in fp64 on CPU copies of the same fp32 inputs (tests/test_psf_cpu.py pins it to the reference
text).  Yardstick of every tolerance: the UNFUSED fp32 path on the same device and inputs against that oracle -- a fused error
may be at most MARGIN = 4 x the unfused error measured in the same test (the ray sum is re-ordered into per-block chains, the
hardware exponential is 1 ulp against the library's).  No fixed number is asserted for an error; both errors are printed
(lines "PSF-ACC ...", kept in profiles/psf_fused_accuracy.txt).  The op-level tests pass y_target and increment explicitly:
the same fp32 values go to both fp32 paths and their fp64 casts to the oracle (fp32 arithmetic on the default y_target is
error of the shared torch code, ~1e-5, and would drown what is compared)."""
import numpy as np
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 4.0
PITCH = {(21, 21): 0.004, (8, 10): 0.012, (32, 32): 0.003, (15, 15): 0.006}
RAGGED = 8191 + 64 * 5 + 3
F, W = 3, 3


@pytest.fixture(scope="module")
def ta():
    import torchoptics_amd as ta
    from torchoptics_amd import _lib
    _lib.lib()
    return ta


def _fan(R, seed=0):
    """test_psf_cpu._fan with F = 3 fields at y = 0 .. 3 mm, W = 3: x mirrored, y repeated (10 nm apart, so that the extreme
    ray of a field is one ray on every device), cut to R rays; every 7th ray has weight 0.  fp32 CPU tensors [1,F,W,R]."""
    rng = np.random.default_rng(seed)
    h = (R + 1) // 2
    x = rng.normal(0, 0.01, (1, F, W, h))
    x = np.concatenate((x, -x), axis=-1)[..., :R]
    y = rng.normal(0, 0.02, (1, F, W, h)) + np.linspace(0, 3, F)[None, :, None, None]
    y = np.concatenate((y, y + 1e-5), axis=-1)[..., :R]
    w = np.broadcast_to((np.arange(R) % 7 != 0), x.shape)
    return torch.from_numpy(x).float(), torch.from_numpy(y).float(), torch.from_numpy(w.copy())


def _eval(metrics, x, y, w, T, yt=None, **kw):
    """kernels and the gradients of sum(kernels * T) in x, y (and y_target when given), on the tensors' device and dtype."""
    x, y = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    yt = None if yt is None else yt.clone().requires_grad_(True)
    k = metrics.compute_psf(x, y, weights=w, y_target=yt, **kw)[3]
    (k * T).sum().backward()
    return k.detach(), x.grad, y.grad, (None if yt is None else yt.grad)


def _value_err(k, k64):
    k, k64 = k.double().cpu(), k64.double().cpu()
    return float(((k - k64).abs().amax(dim=(-1, -2)) / k64.amax(dim=(-1, -2))).max())


def _three_ways(metrics, x, y, w, n_bins, seed, yt=None, increment=None, **kw):
    """(oracle, unfused, fused) results of _eval: fp64 on the CPU, fp32 on the GPU twice."""
    g = torch.Generator().manual_seed(seed)
    T = torch.randn((F, W, n_bins[1], n_bins[0]), generator=g, dtype=torch.float64)
    inc32 = None if increment is None else float(np.float32(increment))          # the value fp32 rounds the pitch to
    ora = _eval(metrics, x.double(), y.double(), w.double(), T, None if yt is None else yt.double(), n_bins=n_bins,
                increment=inc32, **kw)
    xd, yd, Td = x.to(DEV), y.to(DEV), T.float().to(DEV)
    ytd = None if yt is None else yt.to(DEV)
    unf = _eval(metrics, xd, yd, w.float().to(DEV), Td, ytd, n_bins=n_bins, increment=inc32, fused=False, **kw)
    fus = _eval(metrics, xd, yd, w.float().to(DEV), Td, ytd, n_bins=n_bins, increment=inc32, fused=True, **kw)
    return ora, unf, fus


def _check(label, ora, unf, fus):
    names = ("values", "grad x", "grad y", "grad y_target")
    rows = []
    for i, name in enumerate(names):
        if ora[i] is None:
            continue
        if i == 0:
            eu, ef = _value_err(unf[0], ora[0]), _value_err(fus[0], ora[0])
        else:
            eu = rel_l2(unf[i].cpu().numpy(), ora[i].numpy())
            ef = rel_l2(fus[i].cpu().numpy(), ora[i].numpy())
        print(f"PSF-ACC {label} {name}: fused {ef:.3e} unfused {eu:.3e} ratio {ef / max(eu, 1e-300):.2f}")
        rows.append((name, ef, eu))
    for name, ef, eu in rows:
        assert np.isfinite(ef) and ef <= MARGIN * eu, f"{label} {name}: fused {ef:.3e} > {MARGIN} x unfused {eu:.3e}"


# ------------------------------------------------------------------ 1. values and gradients at op level
@pytest.mark.parametrize("R", [8192, RAGGED])
@pytest.mark.parametrize("n_bins", list(PITCH))
def test_values_and_ray_gradients_against_the_fp64_oracle(ta, n_bins, R):
    x, y, w = _fan(R, seed=R % 11)
    yt = (torch.linspace(0, 3, F) + torch.tensor([1e-3, -2e-3, 5e-4])).float()
    ora, unf, fus = _three_ways(ta.metrics, x, y, w, n_bins, seed=1, yt=yt, increment=PITCH[n_bins])
    assert fus[0].shape == (F, W, n_bins[1], n_bins[0]) and fus[0].dtype == torch.float32
    _check(f"explicit grid {n_bins} R={R}", ora, unf, fus)
    dead = ~w.to(DEV)
    assert (fus[1][dead] == 0).all() and (fus[2][dead] == 0).all(), "a ray of weight 0 must get exactly no gradient"
    assert (fus[1][~dead] != 0).any()


@pytest.mark.parametrize("R", [8192, RAGGED])
@pytest.mark.parametrize("n_bins", list(PITCH))
def test_gradients_through_a_grid_sized_from_the_data(ta, n_bins, R):
    """increment=None, y_target=None: the pitch comes from the fan's extent and the centre from its mean, so the gradients in
    x and y hold the three per-grid gradients of the kernel (g_x_pitch, g_y_pitch, g_y_centre)."""
    x, y, w = _fan(R, seed=3 + R % 11)
    ora, unf, fus = _three_ways(ta.metrics, x, y, w, n_bins, seed=2, y_extent="centred")
    _check(f"data-sized grid {n_bins} R={R}", ora, unf, fus)


def _hist_torch(x, y, w, px, py, yc, nxh, ny, x_first, y_first):
    """The kernel's definition in plain torch ops (any dtype / device): [G,W,ny,nxh]."""
    u, v = x / px[:, None, None], (y - yc[:, None, None]) / py[:, None, None]
    j = torch.arange(nxh, dtype=x.dtype, device=x.device) + x_first
    i = torch.arange(ny, dtype=x.dtype, device=x.device) + y_first
    g_x = torch.exp(-2 * (u[:, :, None, :] - j[:, None]) ** 2)
    g_y = torch.exp(-2 * (v[:, :, None, :] - i[:, None]) ** 2) * w[:, :, None, :]
    return torch.matmul(g_y, g_x.transpose(-1, -2))


@pytest.mark.parametrize("n_bins", [(21, 21), (8, 10)])
def test_per_grid_gradients_of_the_op(ta, n_bins):
    """g_x_pitch, g_y_pitch, g_y_centre of ops.PsfAccumulateFunction one by one (compute_psf has no pitch leaf): oracle =
    the kernel's definition in torch fp64 on the CPU, yardstick = the same ops in fp32 on the GPU."""
    from torchoptics_amd import ops
    x, y, w = _fan(RAGGED, seed=5)
    x, y, w = x[0], y[0], w[0]
    nxh, x_first = (n_bins[0] // 2 + 1, 0.0) if n_bins[0] % 2 else (n_bins[0] // 2, 0.5)
    ny, y_first = n_bins[1], 0.5 - n_bins[1] / 2
    p = PITCH[n_bins]
    px, py = torch.tensor([p, 1.1 * p, 0.9 * p]), torch.tensor([1.2 * p, p, 0.8 * p])
    yc = torch.linspace(0, 3, F) + 1e-3
    T = torch.randn((F, W, ny, nxh), generator=torch.Generator().manual_seed(4), dtype=torch.float64)

    def grads(fn, dt, dev, wt):
        leaves = [a.to(dt).to(dev).requires_grad_(True) for a in (px, py, yc)]
        h = fn(x.to(dt).to(dev), y.to(dt).to(dev), wt, *leaves, nxh, ny, x_first, y_first)
        (h * T.to(dt).to(dev)).sum().backward()
        return [a.grad for a in leaves]
    ora = grads(_hist_torch, torch.float64, "cpu", w.double())
    unf = grads(_hist_torch, torch.float32, DEV, w.float().to(DEV))
    fus = grads(ops.PsfAccumulateFunction.apply, torch.float32, DEV, w.to(DEV))
    for name, o, u, f in zip(("g_x_pitch", "g_y_pitch", "g_y_centre"), ora, unf, fus):
        eu, ef = rel_l2(u.cpu().numpy(), o.numpy()), rel_l2(f.cpu().numpy(), o.numpy())
        print(f"PSF-ACC op {n_bins} {name}: fused {ef:.3e} unfused {eu:.3e} ratio {ef / max(eu, 1e-300):.2f}")
        assert f.shape == o.shape and ef <= MARGIN * eu, (name, ef, eu)


def test_ok_bytes_and_float_weights_give_the_same_bits(ta):
    x, y, w = _fan(RAGGED, seed=7)
    yt = torch.linspace(0, 3, F).float().to(DEV)
    T = torch.randn((F, W, 21, 21), generator=torch.Generator().manual_seed(5)).to(DEV)
    kw = dict(yt=yt, n_bins=(21, 21), increment=0.004, fused=True)
    a = _eval(ta.metrics, x.to(DEV), y.to(DEV), w.float().to(DEV), T, **kw)
    b = _eval(ta.metrics, x.to(DEV), y.to(DEV), w.to(DEV), T, **kw)                          # bool: passed as bytes
    c = _eval(ta.metrics, x.to(DEV), y.to(DEV), w.to(torch.uint8).to(DEV), T, **kw)
    for p, q, r in zip(a, b, c):
        assert torch.equal(p, q) and torch.equal(p, r)
    n = _eval(ta.metrics, x.to(DEV), y.to(DEV), None, T, **kw)                               # and the weights matter
    assert not torch.equal(n[0], a[0])


# ------------------------------------------------------------------ 2. end to end through the trace
def _traced(ta, requires_grad):
    from torchoptics_amd import prescriptions as P
    lens, specs, leaves = P.double_gauss(DEV, requires_grad=requires_grad)
    tr = ta.RayTracer(mode="circular", n_rays=(32, 64), rel_fields=(0., 0.7, 1.0), wavelengths=("C", "d", "F"),
                      default_device=DEV)
    x, y, cx, cy, ok, back = tr.trace_rays(specs, lens)
    return x, y, ok, leaves


@pytest.mark.parametrize("increment", [None, 0.002])
def test_psf_from_trace_fused_against_unfused(ta, increment):
    x, y, ok, _ = _traced(ta, False)
    unf = ta.metrics.psf_from_trace(x, y, ok, n_bins=(21, 21), increment=increment)
    fus = ta.metrics.psf_from_trace(x, y, ok, n_bins=(21, 21), increment=increment, fused=True)
    ora = ta.metrics.psf_from_trace(x.cpu().double(), y.cpu().double(), ok.cpu(), n_bins=(21, 21),
                                    increment=None if increment is None else float(np.float32(increment)))
    k_u, k_f, k_o = unf[3], fus[3], ora[3]
    assert k_f.shape == (3, 3, 21, 21) and torch.isfinite(k_f).all()
    e_u, e_fu = _value_err(k_u, k_o), _value_err(k_f, k_u)
    print(f"PSF-ACC traced fan increment={increment}: fused-vs-unfused {e_fu:.3e} unfused-vs-oracle {e_u:.3e}")
    assert e_fu <= (MARGIN + 1) * e_u                       # |f - u| <= |f - o| + |u - o| <= (4 + 1) |u - o|
    assert torch.allclose(k_f.sum(dim=(-1, -2)), torch.ones(3, 3, device=DEV), atol=1e-5)       # unit sum per channel
    assert torch.equal(k_f, torch.flip(k_f, dims=(-1,)))                                          # mirrored in x
    for a, b in zip(unf[:3] + unf[4:], fus[:3] + fus[4:]):                                        # the shared torch code
        assert torch.equal(torch.as_tensor(a), torch.as_tensor(b))


def test_leaf_gradients_of_a_psf_loss_through_the_trace(ta):
    T = torch.randn((3, 3, 21, 21), generator=torch.Generator().manual_seed(6)).to(DEV)
    got = {}
    for fused in (False, True):
        x, y, ok, leaves = _traced(ta, True)
        k = ta.metrics.psf_from_trace(x, y, ok, n_bins=(21, 21), fused=fused)[3]
        (k * T).sum().backward()
        got[fused] = {n: leaves[n].grad.cpu().numpy() for n in ("c", "t")}
    for n in ("c", "t"):
        e = rel_l2(got[True][n], got[False][n])
        print(f"PSF-ACC leaf gradient {n}: fused vs unfused rel-L2 {e:.3e}")
        assert np.isfinite(got[True][n]).all() and np.linalg.norm(got[False][n]) > 0
        assert e <= 1e-5, (n, e)                            # the project's gradient gate


# ------------------------------------------------------------------ 3. reproducibility
def test_two_calls_give_the_same_bits(ta):
    from torchoptics_amd import ops
    x, y, w = _fan(1 << 16, seed=9)
    x, y, w = x[0].to(DEV), y[0].to(DEV), w[0].to(DEV)
    T = torch.randn((F, W, 21, 11), generator=torch.Generator().manual_seed(7)).to(DEV)

    def once():
        lv = [a.clone().requires_grad_(True) for a in (x, y)]
        lv += [torch.full((F,), 0.004, device=DEV).requires_grad_(True) for _ in range(2)]
        lv.append(torch.linspace(0, 3, F).to(DEV).requires_grad_(True))
        h = ops.PsfAccumulateFunction.apply(lv[0], lv[1], w, lv[2], lv[3], lv[4], 11, 21, 0.0, -10.0)
        (h * T).sum().backward()
        return [h.detach()] + [a.grad for a in lv]
    a, b = once(), once()
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    assert all(torch.isfinite(p).all() and (p != 0).any() for p in a)


# ------------------------------------------------------------------ 4. / 5. memory and speed at 9.4 M rays
P_BIG = 1 << 20


def _big():
    g = torch.Generator(device=DEV).manual_seed(11)
    x = torch.randn((1, F, W, P_BIG), generator=g, device=DEV) * 0.01
    y = torch.randn((1, F, W, P_BIG), generator=g, device=DEV) * 0.02 + torch.linspace(0, 3, F, device=DEV)[None, :, None, None]
    ok = (torch.arange(P_BIG, device=DEV) % 7 != 0).expand(1, F, W, P_BIG).contiguous()
    yt = torch.linspace(0, 3, F, device=DEV)
    T = torch.randn((F, W, 21, 21), generator=g, device=DEV)
    return x.requires_grad_(True), y.requires_grad_(True), ok, yt, T


def _step(metrics, x, y, ok, yt, T, fused):
    x.grad = y.grad = None
    k = metrics.compute_psf(x, y, n_bins=(21, 21), increment=0.004, y_target=yt, weights=ok, fused=fused)[3]
    (k * T).sum().backward()
    return k.detach()


def _peak_growth(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def test_memory_per_ray_of_forward_and_backward(ta):
    """Derived from the shapes, not measured: the fused step holds the two ray gradients (8 B per ray), the workspace
    (<< 1 B) and the O(1) passes of the shared torch code (the centred y, accounted_ray_proportion); the bound is 64 B per
    ray, half of what the two operands of the unfused forward alone take (128 B)."""
    x, y, ok, yt, T = _big()
    n_rays = F * W * P_BIG
    fused = _peak_growth(lambda: _step(ta.metrics, x, y, ok, yt, T, True))
    x.grad = y.grad = None
    unfused = _peak_growth(lambda: _step(ta.metrics, x, y, ok, yt, T, False))
    print(f"PSF-MEM {n_rays} rays 21x21: peak growth fused {fused / n_rays:.1f} B/ray, unfused {unfused / n_rays:.1f} B/ray")
    assert fused <= 64 * n_rays, fused / n_rays
    assert x.grad is not None and torch.isfinite(x.grad).all()


def test_fused_step_is_faster_than_the_unfused_one(ta):
    x, y, ok, yt, T = _big()
    times = {True: [], False: []}
    for rep in range(2 + 5):                                # two warm-up rounds, five timed; the two paths alternate
        for fused in (True, False):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            _step(ta.metrics, x, y, ok, yt, T, fused)
            b.record()
            torch.cuda.synchronize()
            if rep >= 2:
                times[fused].append(a.elapsed_time(b))
    tf, tu = float(np.median(times[True])), float(np.median(times[False]))
    print(f"PSF-TIME {F * W * P_BIG} rays 21x21 forward+backward: fused {tf:.3f} ms, unfused {tu:.3f} ms, ratio {tu / tf:.2f}")
    assert tf < tu


# ------------------------------------------------------------------ 6. graph capture
def test_a_captured_step_replays_the_eager_bits(ta):
    from torchoptics_amd import graphs
    x0, y0, w = _fan(1 << 14, seed=13)
    yt = torch.linspace(0, 3, F).to(DEV)
    T = torch.randn((F, W, 21, 21), generator=torch.Generator().manual_seed(8)).to(DEV)
    ok = w.to(DEV)

    def step(x, y):
        x.grad = y.grad = None
        k = ta.metrics.compute_psf(x, y, n_bins=(21, 21), increment=0.004, y_target=yt, weights=ok, fused=True)[3]
        (k * T).sum().backward()
        return k.detach(), x.grad, y.grad

    ex, ey = graphs.fresh_leaves(x0.to(DEV), y0.to(DEV))
    eager = [t.clone() for t in step(ex, ey)]
    gx, gy = graphs.fresh_leaves(x0.to(DEV), y0.to(DEV))
    g, out = graphs.capture_step(lambda: step(gx, gy), DEV)
    for t in out:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(out, eager):
        assert torch.equal(a, b)
    assert (eager[1] != 0).any()
