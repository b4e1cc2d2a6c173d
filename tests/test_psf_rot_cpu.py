"""The rotated PSF grid without a GPU: the bounds of tests/psf_rot_ref.py held to be sufficient (a float32 emulation of the
kernels' arithmetic stays inside them on every case of the table) and sharp (every wrong evaluation named in the issue leaves
them); the host geometry of imaging.psf_grid_cells; imaging.psf_grid_from_trace(fused=False) in float64 on a synthetic comatic
fan; and what the C ABI and the Python layer refuse before any HIP call."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import psf_rot_ref as rr
from conftest import ROOT

from torchoptics_amd import _lib, imaging, ops

EINVAL, EWORKSPACE = -1, -3                 # TL_EINVAL, TL_EWORKSPACE (include/tl_trace.h)
ONE = C.c_void_p(8)                         # any non-NULL pointer: never dereferenced on the paths taken here


# ------------------------------------------------------------------------------------------- 1. the bounds are sufficient
@pytest.mark.parametrize("name", list(rr.CASES))
def test_the_float32_emulation_stays_within_the_bounds(name):
    a, r = rr.inputs(name), rr.reference(name)
    q = rr.ratios(rr.emulate(a), r)
    print(f"PSF-ROT-EMU {name}: largest error / bound " + " ".join(f"{k} {v:.3f}" for k, v in q.items()))
    assert max(q.values()) <= 1.0, q
    assert np.isfinite(r.hist_bound).all() and (r.hist_bound > 0).all()
    K = a.shape[0]
    unread = [k for k in range(K) if k not in set(a.src.tolist())]
    for k in unread:                                         # a fan that no grid reads: no gradient, and a bound of nothing
        assert not r.gx[k].any() and not r.gx_bound[k].any()
    if name == "shared":
        assert unread == [2]


def test_the_emulation_with_other_exp2_roundings_stays_within_the_bounds():
    a, r = rr.inputs("shared"), rr.reference("shared")
    for seed in (1, 2, 3):
        assert max(rr.ratios(rr.emulate(a, seed=seed), r).values()) <= 1.0


# ------------------------------------------------------------------------------------------------ 2. the bounds are sharp
@pytest.mark.parametrize("variant,results", [("sign-s", ("hist", "gx", "gy")), ("bwd-transposed", ("gx", "gy")),
                                             ("src-ignored", ("hist", "gx", "gy")), ("centre-per-grid", ("hist", "gx", "gy")),
                                             ("last-grid-only", ("gx", "gy"))])
def test_a_wrong_evaluation_exceeds_the_bounds(variant, results):
    for name in ("shared", "dead-channel"):
        a, r = rr.inputs(name), rr.reference(name)
        wrong = rr.evaluate(a, variant=variant)
        q = rr.ratios({k: getattr(wrong, k) for k in rr.RESULTS}, r)
        print(f"PSF-ROT-SHARP {name} {variant}: " + " ".join(f"{k} {v:.3g}" for k, v in q.items()))
        for k in results:
            assert q[k] > 100.0, (name, variant, k, q[k])


def test_a_dead_ray_turned_before_it_is_dropped_shows_and_one_dropped_first_does_not():
    a, r = rr.inputs("shared"), rr.reference("shared")
    dead = a.weight == 0
    assert dead.any()
    b = rr.SimpleNamespace(**vars(a))
    b.x, b.y = np.where(dead, np.float32(np.nan), a.x), np.where(dead, np.float32(np.nan), a.y)
    clean, hostile = rr.emulate(a), rr.emulate(b)
    for k in rr.RESULTS:
        assert np.array_equal(clean[k].view(np.uint32), hostile[k].view(np.uint32)), k
    q = rr.ratios(rr.emulate(b, rotate_dead=True), r)
    assert q["hist"] == float("inf"), q


def test_beta_applied_before_the_normalisation_exceeds_the_bound():
    a, r = rr.inputs("shared"), rr.reference("shared")
    cell, beta = np.array([0, 0, 1, 2, 2]), np.array([0.25, 0.75, 1.0, 0.6, 0.4])
    assert a.weight.dtype == np.uint8                       # weights of 0 and 1: a PSF
    want, bound = rr.blend(r.hist, cell, beta, 3, r.hist_bound)
    assert np.allclose(want.sum((-1, -2)), 1.0, atol=1e-12)
    got = rr.blend(rr.emulate(a)["hist"], cell, beta, 3)
    assert rr.ratio(got, want, bound) <= 1.0
    wrong = rr.blend(r.hist, cell, beta, 3, beta_first=True)
    assert rr.ratio(wrong[1], want[1], bound[1]) == 0.0     # a cell of one term cannot tell
    assert rr.ratio(wrong[0], want[0], bound[0]) > 100.0 and rr.ratio(wrong[2], want[2], bound[2]) > 100.0


# ------------------------------------------------------------------------------------------------------ 3. psf_grid_cells
def test_cells_of_a_3x3_grid_on_a_square_image():
    cl = imaging.psf_grid_cells((48, 48), (3, 3), 4, (0.3, 0.7, 1.0))
    assert cl.N == 9 and cl.X.shape == (9,)
    assert (cl.s_cell[4], cl.c_cell[4]) == (0.0, 1.0) and cl.h[4] == 0.0           # the centre cell is the identity
    t4 = np.nonzero(cl.cell == 4)[0]
    assert t4.size == 1 and cl.src[t4[0]] == 0 and cl.beta[t4[0]] == 1.0 and (cl.c[t4[0]], cl.s[t4[0]]) == (1.0, 0.0)
    q = 1 / np.sqrt(2)
    for n, (sx, sy) in {0: (-1, -1), 2: (1, -1), 6: (-1, 1), 8: (1, 1)}.items():   # rows are y: cell 0 is at (-x, -y)
        assert abs(cl.s_cell[n] - sx * q) < 1e-15 and abs(cl.c_cell[n] - sy * q) < 1e-15
    for n, sc in {1: (0.0, -1.0), 7: (0.0, 1.0), 3: (-1.0, 0.0), 5: (1.0, 0.0)}.items():
        assert (cl.s_cell[n], cl.c_cell[n]) == sc, n                                # exact 0 and +-1
    assert np.allclose(cl.h[[0, 2, 6, 8]], 32 / 47) and np.allclose(cl.h[[1, 3, 5, 7]], 32 / 47 / np.sqrt(2))
    assert np.array_equal(cl.c, cl.c_cell[cl.cell].astype(np.float32)) and cl.c.dtype == cl.s.dtype == np.float32
    assert cl.src.dtype == cl.field_start.dtype == cl.field_grids.dtype == np.int32
    assert imaging.psf_grid_cells((48, 48), (3, 3), (4, 4), [0.3, 0.7, 1.0]) is cl                  # memoised


@pytest.mark.parametrize("blend", ["linear", "nearest"])
@pytest.mark.parametrize("fields", [(0.3, 0.7, 1.0), (0.0, 0.5, 1.0), (0.1, 0.4), (0.9,)])
def test_terms_per_cell_beta_and_the_csr_lists(fields, blend):
    cl = imaging.psf_grid_cells((42, 60), (3, 5), (3, 2), fields, blend=blend)
    f, K = np.asarray(fields), len(fields)
    assert np.all(np.diff(cl.cell) >= 0)
    sums = np.bincount(cl.cell, weights=cl.beta, minlength=cl.N)
    assert np.allclose(sums, 1.0, atol=1e-15) and (cl.beta > 0).all()
    for n in range(cl.N):
        t = np.nonzero(cl.cell == n)[0]
        if blend == "nearest" or cl.h[n] <= f[0] or cl.h[n] >= f[-1]:
            assert t.size == 1 and cl.beta[t[0]] == 1.0
            want = np.argmin(np.abs(f - cl.h[n])) if blend == "nearest" else (0 if cl.h[n] <= f[0] else K - 1)
            assert cl.src[t[0]] == want
        else:
            assert 1 <= t.size <= 2
            assert abs((cl.beta[t] * f[cl.src[t]]).sum() - cl.h[n]) < 1e-15                       # linear in h
            assert t.size == 1 or cl.src[t[1]] == cl.src[t[0]] + 1
    assert cl.field_start[0] == 0 and cl.field_start[-1] == cl.src.size and cl.field_start.size == K + 1
    for k in range(K):                                                                             # the CSR lists invert src
        g = cl.field_grids[cl.field_start[k]:cl.field_start[k + 1]]
        assert (cl.src[g] == k).all() and np.all(np.diff(g) > 0)
    assert sorted(cl.field_grids.tolist()) == list(range(cl.src.size))
    if fields == (0.1, 0.4):
        assert (np.bincount(cl.cell)[[0, 4, 10, 14]] == 1).all() and cl.h[0] > 0.4              # corners beyond the last field


def test_mirrored_cells_have_mirrored_rotations_and_aspect_counts():
    cl = imaging.psf_grid_cells((42, 60), (3, 5), (3, 2), (0.5, 1.0))
    s, c, h = (v.reshape(3, 5) for v in (cl.s_cell, cl.c_cell, cl.h))
    assert np.array_equal(s, -s[:, ::-1]) and np.array_equal(c, c[:, ::-1]) and np.array_equal(h, h[:, ::-1])
    assert np.array_equal(c[0], -c[2]) and np.array_equal(s[0], s[2]) and np.array_equal(h[0], h[2])
    assert (s[:, 3:] > 0).all() and (c[2] > 0).all() and (c[1, [0, 1, 3, 4]] == 0).all() and s[1, 2] == 0 and c[1, 2] == 1
    assert np.allclose(s * s + c * c, 1.0)
    sq = imaging.psf_grid_cells((42, 60), (3, 5), (3, 2), (0.5, 1.0), aspect=1.0)
    assert abs(sq.s_cell[14]) < abs(cl.s_cell[14])          # the wider the image, the flatter the corner's direction
    with pytest.raises(ValueError, match="ascending"):
        imaging.psf_grid_cells((42, 60), (3, 5), 3, (0.5, 0.5))
    with pytest.raises(ValueError, match="ascending"):
        imaging.psf_grid_cells((42, 60), (3, 5), 3, (-0.1, 0.5))
    with pytest.raises(ValueError, match="blend"):
        imaging.psf_grid_cells((42, 60), (3, 5), 3, (0.5,), blend="cubic")


# ------------------------------------------------------------------------------ 4. psf_grid_from_trace(fused=False), float64
def _comatic_fan(P=400, W=2, seed=0):
    """[1, F=3, P, W] float64: fields at y = 0, 1.5, 3 mm (h = 0, 0.5, 1), a random (not symmetric) pupil sample, coma that
    grows with the field and flares towards +y: dy = A h rho^2 (2 + cos 2t), dx = A h rho^2 sin 2t."""
    rng = np.random.default_rng(seed)
    rho, t = np.sqrt(rng.uniform(0, 1, (P, W))), rng.uniform(0, 2 * np.pi, (P, W))
    hf = np.array([0.0, 0.5, 1.0])[:, None, None]
    amp = 0.012 * (1 + 0.1 * np.arange(W))
    x = (0.004 * rho * np.cos(t) + amp * hf * rho ** 2 * np.sin(2 * t))[None]
    y = (3.0 * hf + 0.004 * rho * np.sin(t) + amp * hf * rho ** 2 * (2 + np.cos(2 * t)))[None]
    return torch.from_numpy(x), torch.from_numpy(y), torch.tensor([0.0, 1.5, 3.0], dtype=torch.float64)


def test_the_flare_of_every_cell_points_along_its_own_radius():
    x, y, chief = _comatic_fan()
    cl = imaging.psf_grid_cells((48, 48), (3, 3), 4, (0.0, 0.5, 1.0))
    psfs = imaging.psf_grid_from_trace(x, y, None, cl, (21, 21), 0.004, y_target=chief, fused=False)
    assert psfs.shape == (1, 9, 21, 21, 2) and psfs.dtype == torch.float64
    p = psfs[0].numpy()
    assert np.allclose(p.sum((1, 2)), 1.0, atol=1e-12) and (p >= 0).all()
    ax = np.arange(21) - 10.0
    cx, cy = (p * ax[None, None, :, None]).sum((1, 2)), (p * ax[None, :, None, None]).sum((1, 2))      # [N, W]: columns, rows
    for n in range(9):
        r = np.hypot(cx[n], cy[n])
        if n == 4:
            assert (r < 0.05).all()                         # on axis: no flare
            continue
        along = cx[n] * cl.s_cell[n] + cy[n] * cl.c_cell[n]
        across = cx[n] * cl.c_cell[n] - cy[n] * cl.s_cell[n]
        assert (along > 0.5).all(), (n, along)              # outwards (the sign), by more than half a pixel
        assert (np.abs(across) < 0.1 * along).all(), (n, across, along)        # and along the radius (the angle)
    # corners see more coma than edges: h = 0.68 against 0.48
    assert (np.hypot(cx[8], cy[8]) > np.hypot(cx[7], cy[7])).all()
    # the +x cell (5) is the +y cell (7) transposed, with the flip of x' = eta, y' = -xi:  psf_x[i, j] = psf_y[j, n-1-i]
    assert np.allclose(p[5], np.flip(np.swapaxes(p[7], 0, 1), axis=0), rtol=0, atol=1e-14)
    assert not np.allclose(p[5], np.swapaxes(p[7], 0, 1), rtol=0, atol=1e-6)
    # the -y cell (1) is the +y one turned by 180 degrees
    assert np.allclose(p[1], np.flip(p[7], axis=(0, 1)), rtol=0, atol=1e-14)


def test_psf_grid_from_trace_against_the_reference_definition_and_its_gradients():
    x, y, chief = _comatic_fan(P=150, seed=1)
    ok = torch.from_numpy(np.arange(150 * 2).reshape(150, 2) % 5 != 0).expand(1, 3, 150, 2)
    cl = imaging.psf_grid_cells((40, 60), (2, 5), 2, (0.0, 0.5, 1.0))
    xg, yg = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    psfs = imaging.psf_grid_from_trace(xg, yg, ok, cl, (9, 7), 0.006, fused=False)                 # default y_target
    assert psfs.shape == (1, 10, 7, 9, 2)
    w = ok[0].permute(0, 2, 1).numpy().astype(np.float64)
    xs, ys = x[0].permute(0, 2, 1).numpy(), y[0].permute(0, 2, 1).numpy()
    yt = (ys * w).sum((1, 2)) / w.sum((1, 2))
    a = rr.SimpleNamespace(x=xs, y=ys, weight=w, src=cl.src, c=cl.c, s=cl.s, x_pitch=np.full(cl.src.size, 0.006),
                           y_pitch=np.full(cl.src.size, 0.006), y_centre=yt, T=np.zeros((cl.src.size, 2, 7, 9)), nx=9, ny=7,
                           x_first=-4.0, y_first=-3.0, shape=xs.shape, G=cl.src.size)
    want = rr.blend(rr.evaluate(a, bounds=False).hist, cl.cell, cl.beta, cl.N)
    assert np.allclose(psfs[0].permute(0, 3, 1, 2).detach().numpy(), want, rtol=0, atol=1e-13)
    T = torch.randn(psfs.shape, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    (psfs * T).sum().backward()
    dead = ~ok
    assert (xg.grad[dead] == 0).all() and (xg.grad[~dead] != 0).any() and torch.isfinite(yg.grad).all()
    eps = 1e-7                                              # a finite difference on one live ray: the gradient is the definition's
    idx = (0, 2, 8, 1)
    assert ok[idx]
    for leaf, grad in ((x, xg.grad), (y, yg.grad)):
        vals = []
        for sgn in (1, -1):
            v = leaf.clone()
            v[idx] += sgn * eps
            args = (v, y) if leaf is x else (x, v)
            vals.append(float((imaging.psf_grid_from_trace(*args, ok, cl, (9, 7), 0.006, fused=False) * T).sum()))
        fd = (vals[0] - vals[1]) / (2 * eps)
        assert abs(fd - float(grad[idx])) <= 1e-5 * max(abs(fd), 1e-3), (fd, float(grad[idx]))


# --------------------------------------------------------------------------------- 5. what is refused before any HIP call
NAMES = ("tl_psf_rot_workspace_bytes", "tl_psf_rot_accumulate", "tl_psf_rot_accumulate_bwd")


def test_entry_points_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "tl_trace.h")).read()
    declared = set(re.findall(r"\b(tl_[a-z0-9_]+)\s*\(", hdr))
    dll = _lib.lib()
    for name in NAMES:
        assert name in declared and name in _lib.EXPORTS and hasattr(dll, name), name
    assert dll.tl_version() == _lib.TL_ABI_VERSION
    assert "1048576" in hdr                                 # the row limit is stated


def _fwd(dll, G=5, K=3, W=3, R=1000, x=ONE, y=ONE, weight=None, ok=None, src=ONE, c=ONE, s=ONE, xp=ONE, yp=ONE, yc=ONE, nx=21,
         ny=21, hist=ONE, ws=ONE, ws_bytes=1 << 40):
    return dll.tl_psf_rot_accumulate(0, G, K, W, R, x, y, weight, ok, W * R, R, src, c, s, xp, yp, yc, nx, ny, -10.0, -10.0, hist,
                                     ws, ws_bytes, None)


def _bwd(dll, G=5, K=3, W=3, R=1000, x=ONE, y=ONE, weight=None, ok=None, src=ONE, c=ONE, s=ONE, xp=ONE, yp=ONE, yc=ONE, nx=21,
         ny=21, fstart=ONE, fgrids=ONE, g_hist=ONE, gx=ONE, gy=ONE, ws=ONE, ws_bytes=1 << 40):
    return dll.tl_psf_rot_accumulate_bwd(0, G, K, W, R, x, y, weight, ok, W * R, R, src, c, s, xp, yp, yc, nx, ny, -10.0, -10.0,
                                         fstart, fgrids, g_hist, gx, gy, None, ws, ws_bytes, None)


BAD = [dict(x=None), dict(y=None), dict(src=None), dict(c=None), dict(s=None), dict(xp=None), dict(yp=None), dict(yc=None),
       dict(nx=0), dict(nx=33), dict(ny=0), dict(ny=33),
       dict(G=0), dict(K=0), dict(W=0), dict(G=1 << 19, W=3), dict(K=1 << 19, W=3), dict(G=(1 << 20) + 1, W=1),
       dict(R=0), dict(R=-5), dict(G=1 << 10, W=1 << 10, R=(1 << 16) + 1),
       dict(weight=ONE, ok=ONE)]


@pytest.mark.parametrize("bad", BAD, ids=lambda d: ",".join(f"{k}={'NULL' if v is None else getattr(v, 'value', v)}" for k, v in d.items()))
def test_bad_arguments_are_refused_before_any_hip_call(bad):
    dll = _lib.lib()
    for call, name in ((_fwd, b"tl_psf_rot_accumulate"), (_bwd, b"tl_psf_rot_accumulate_bwd")):
        dll.tl_unsup_loss(0, 0, 3, 100.0, ONE, None, 7.0, 0.2, ONE, ONE, ONE, ONE, None)       # another call's message first
        assert call(dll, **bad) == EINVAL, (name, bad)
        assert name + b":" in dll.tl_last_error()
    assert _fwd(dll, hist=None) == EINVAL and b"tl_psf_rot_accumulate" in dll.tl_last_error()
    for k in ("fstart", "fgrids", "g_hist", "gx", "gy"):
        assert _bwd(dll, **{k: None}) == EINVAL and b"tl_psf_rot_accumulate_bwd" in dll.tl_last_error()


def test_the_row_limit_of_the_plain_call_does_not_bind_and_the_workspace_is_checked():
    dll = _lib.lib()
    # 65 792 and 2^20 rows pass the argument check (the refusal is the missing workspace); the plain call refuses both
    for G, W in ((256, 257), (1 << 10, 1 << 10), (64 * 64 * 2, 3), (1 << 20, 1)):
        assert _fwd(dll, G=G, K=2, W=W, R=3, ws=None) == EWORKSPACE, (G, W)
        assert _bwd(dll, G=G, K=2, W=W, R=3, ws=None) == EWORKSPACE, (G, W)
        assert dll.tl_psf_rot_workspace_bytes(G, 2, W, 3, 2, 2) > 0
        plain = dll.tl_psf_accumulate(0, G, W, 3, ONE, ONE, None, None, 3 * W, 3, ONE, ONE, ONE, 2, 2, 0.0, 0.0, ONE, None, 0, None)
        assert plain == (EINVAL if G * W > 65535 else EWORKSPACE), (G, W)
    sizes = [dll.tl_psf_rot_workspace_bytes(25, 3, 3, R, 21, 21) for R in (1 << 8, 1 << 12, 1 << 16, 1 << 18)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0
    assert sizes[-1] < 25 * 3 * (1 << 18) // 2, "the workspace must stay far below one byte per ray and grid"
    for bad in ((0, 3, 3, 100, 21, 21), (5, 0, 3, 100, 21, 21), (5, 3, 3, 0, 21, 21), (5, 3, 3, 100, 33, 21), (5, 3, 3, 100, 21, 0),
                ((1 << 20) + 1, 3, 1, 100, 21, 21)):
        assert dll.tl_psf_rot_workspace_bytes(*bad) == 0
    assert _fwd(dll, ws_bytes=16) == EWORKSPACE and b"tl_psf_rot_accumulate" in dll.tl_last_error()
    assert _bwd(dll, ws_bytes=16) == EWORKSPACE and b"tl_psf_rot_accumulate_bwd" in dll.tl_last_error()


def test_the_python_layer_checks_src_and_has_no_cpu_fallback():
    for src in ([0, 3], [-1, 0], [0.5, 1.0]):
        with pytest.raises(ValueError, match="src"):
            ops.psf_rot_grid(np.asarray(src), [1, 1], [0, 0], 3)
    with pytest.raises(ValueError, match="one per grid"):
        ops.psf_rot_grid(np.array([0, 1]), [1.0], [0.0, 0.0], 2)
    g = ops.psf_rot_grid(np.array([1, 1, 0, 1, 1]), np.ones(5), np.zeros(5), 3)
    assert g.field_start.tolist() == [0, 1, 5, 5] and g.field_grids.tolist() == [2, 0, 1, 3, 4]
    assert np.array_equal(g.field_start, rr.csr([1, 1, 0, 1, 1], 3)[0])
    x, y, _ = _comatic_fan(P=50)
    cl = imaging.psf_grid_cells((48, 48), (3, 3), 4, (0.0, 0.5, 1.0))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        imaging.psf_grid_from_trace(x.float(), y.float(), None, cl, (21, 21), 0.004, fused=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        imaging.psf_grid_from_trace(x, y, None, cl, (21, 21), 0.004, fused=True)
    with pytest.raises(ValueError, match="at most 32 bins"):
        imaging.psf_grid_from_trace(x.float(), y.float(), None, cl, (33, 21), 0.004, fused=True)
    assert imaging.psf_grid_from_trace(x.float(), y.float(), None, cl, (33, 35), 0.004).shape == (1, 9, 35, 33, 1 + 1)
    with pytest.raises(ValueError, match="fields"):
        imaging.psf_grid_from_trace(x[:, :2], y[:, :2], None, cl, (21, 21), 0.004)
