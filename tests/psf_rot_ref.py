"""The rotated PSF grid (tl_psf_rot_accumulate / _bwd of include/tl_trace.h behind ops.PsfRotAccumulateFunction and
imaging.psf_grid_from_trace) without the package: a float64 numpy evaluation of the definition, element-wise error bounds in
the style of psf_ref.evaluate / psf_cases.bound, the case table shared by tests/test_psf_rot_cpu.py and
tests/test_gpu_psf_rot.py, a float32 emulation of the kernels' arithmetic, and the helper that runs the op on a case.

THE DEFINITION.  K fans [K,W,R], G grids; grid g reads fan k = src[g] turned by (c[g], s[g]) about (0, y_centre[k]):
    xi = x[k,w,r],  eta = y[k,w,r] - y_centre[k];     x' = c xi + s eta,   y' = -s xi + c eta
    hist[g,w,i,j] = sum_r wt_r Gy_i Gx_j,   Gx_j = exp(-2 (x'/x_pitch[g] - (x_first + j))^2),  Gy_i likewise from y', y_pitch[g]
    gx'_r, gy'_r = the per-ray gradients of sum(T[g] hist[g]) in x', y' (psf_ref's gx, gy of grid g)
    gx[k] = sum_{g: src[g] = k} c gx' - s gy',   gy[k] = sum_{g: src[g] = k} s gx' + c gy',   g_y_centre[k] = -sum_{w,r} gy[k]
The PSF of a cell (`blend`): sum_t beta_t hist[t] / sum_ij hist[t] over the terms t of the cell -- normalised, then blended.

THE BOUNDS.  Everything psf_cases.py counts for one grid stands (the quotient-and-remainder distance, the Gaussian, the 68
roundings of hist, the nx + ny + 4 of a per-ray gradient); what the rotation adds, with U = 2^-24:
  * eta~ = fl(y - y_centre) = eta (1 + d1).  x' is computed as fl(c xi + fl(s eta~)) = (c xi + s eta (1 + d1)(1 + d2))(1 + d3):
        |x'~ - x'| <= U |x'| + 2 U |s eta| + O(U^2) <= U (|c xi| + 3 |s eta|)
    and y'~ = fl(c eta~ - fl(s xi)) = (c eta (1 + d1) - s xi (1 + d2))(1 + d3):
        |y'~ - y'| <= U |y'| + U |c eta| + U |s xi| <= 2 U (|c eta| + |s xi|).
    These are the two products and the fma per coordinate (<= 2 U (|c xi| + |s eta|)) and the rounding of eta, which
    psf_cases charges along y as U |v| and which here reaches both coordinates.  Divided by the pitch (and times 1 + 2^-20 for
    the second order) they are added to the error dd of every distance along that axis, and go from there into the Gaussian's
    relative error 4 |d| dd and the 4 G dd of its derivative exactly as psf_cases' own dd does.
  * The backward turns each grid's (gx', gy'), known to b' = psf_cases' bound, back:  t_xi = fl(c gx' - fl(s gy')),
    t_eta = fl(c gy' + fl(s gx')): a product and an fma,
        |t_xi~ - t_xi| <= |c| bx' + |s| by' + U (|c| mx + 2 |s| my),   mx = |gx'| + bx', my = |gy'| + by'   (and eta likewise),
    and adds the n terms of the fan's grids in list order: at most one rounding per grid of a partial sum no larger than the
    sum of the absolute terms:  + n U sum_g (|c| mx + |s| my).
  * g_y_centre is held as psf_cases holds it: to the exact float64 sum of the kernel's own float32 gy within
    U |S| + n 2^-53 sum |terms|.
  * A cell's PSF from hist known to b (`blend`): with S = sum_ij hist, bS = sum_ij b,
        |psf~ - psf| <= sum_t beta_t (b / S + hist bS / S^2) (1 + 2 bS / S)       (first order, doubled second order).

`variant` evaluates a deliberately WRONG definition (tests hold the bounds to be sharp):
    'sign-s'          s has the other sign                     'bwd-transposed'  the backward turns by the forward's matrix
    'src-ignored'     grid g reads fan g mod K                 'centre-per-grid' y_centre[g mod K] in place of y_centre[src[g]]
    'last-grid-only'  a shared fan's gradient comes from its last grid alone
and `emulate(..., rotate_dead=True)` turns a ray of weight 0 before dropping it; `blend(..., beta_first=True)` applies beta
before the normalisation."""
import math
from types import SimpleNamespace

import numpy as np
import torch

import psf_cases as pc
import psf_ref as ref

U, TINY = ref.U, ref.TINY
SECOND = 1.0 + 2.0 ** -20
VARIANTS = ("sign-s", "bwd-transposed", "src-ignored", "centre-per-grid", "last-grid-only")
RESULTS = ("hist", "gx", "gy")

# K, W, R, src, ny, nx, weight kind                      (G = len(src); the angles are 37 + 61 g degrees)
CASES = {
    "one-ray": (1, 1, 1, (0,), 32, 32, "float"),
    "shared": (3, 3, 63, (1, 1, 0, 1, 1), 5, 17, "ok"),
    "wave-plus-one": (2, 2, 65, (0, 1, 1), 1, 21, None),
    "block-edge": (2, 2, 257, (1, 0, 0, 1), 32, 25, "float"),
    "reduce": (1, 2, 4161, (0, 0), 7, 3, "ok"),
    "many-rows": (2, 257, 3, tuple(g % 2 for g in range(256)), 2, 2, "float"),
    "dead-channel": (2, 3, 300, (0, 1, 1, 0), 10, 4, "float"),
}
DEAD_CHANNEL = (1, 1)                                    # (source fan, channel) of 'dead-channel'
SWEEP_NX = (1, 4, 5, 8, 12, 13, 16, 17, 20, 24, 25, 28, 29, 32)       # the eight instantiations, each at both ends
SWEEP_SHAPE = (2, 3, 321, (0, 1, 1, 0), 3)               # K, W, R, src, ny

_INPUTS, _REF = {}, {}


def _f32(v):
    return np.asarray(v, dtype=np.float64).astype(np.float32)


def make_inputs(K, W, R, src, ny, nx, kind, seed, dead_channel=None, angles=None, tile=False):
    """Seeded float32 inputs: x, y [K,W,R], weight (float32, uint8 or None), src [G], c, s, x_pitch, y_pitch [G], y_centre
    [K], T [G,W,ny,nx].  The rays fill a disc that reaches 1.5 pixels past the far corner of the tile, so every grid sees
    its tile covered at whatever angle (`tile`: the unrotated tile instead)."""
    rng = np.random.default_rng(seed)
    src = np.asarray(src, dtype=np.int32)
    G = src.size
    g = np.arange(G)
    px = _f32(0.004 * (1 + 0.13 * (g % 5) + 0.0007 * (g % 11)))
    py = _f32(0.0031 * (1 + 0.17 * ((g + 2) % 5) + 0.0009 * (g % 7)))
    yc = _f32(np.linspace(1e-4, 3.0, K) if K > 1 else [3.001])
    phi = np.deg2rad(37.0 + 61.0 * g) if angles is None else np.asarray(angles, dtype=np.float64)
    c, s = _f32(np.cos(phi)), _f32(np.sin(phi))
    if tile:                                             # the tile and 1.5 pixels around it, as psf_cases spreads its rays
        x = _f32(rng.uniform(-nx / 2 - 1.5, nx / 2 + 1.5, (K, W, R)) * 0.004)
        y = _f32(yc.astype(np.float64)[:, None, None] + rng.uniform(-ny / 2 - 1.5, ny / 2 + 1.5, (K, W, R)) * 0.0031)
    else:
        rad = (0.5 * math.hypot(nx, ny) + 1.5) * np.sqrt(rng.uniform(0, 1, (K, W, R)))
        th = rng.uniform(0, 2 * np.pi, (K, W, R))
        x = _f32(rad * np.cos(th) * 0.004)
        y = _f32(yc.astype(np.float64)[:, None, None] + rad * np.sin(th) * 0.0031)
    dead = np.arange(K * W * R).reshape(K, W, R) % 7 == 3
    if dead_channel is not None:
        dead[dead_channel] = True
    mag = rng.uniform(0.1, 1.5, (K, W, R)) * (2.0 * rng.integers(0, 2, (K, W, R)) - 1.0)
    weight = {"float": _f32(np.where(dead, 0.0, mag)), "ok": (~dead).astype(np.uint8), None: None}[kind]
    T = _f32(rng.normal(0, 1, (G, W, ny, nx)))
    return SimpleNamespace(x=x, y=y, weight=weight, src=src, c=c, s=s, x_pitch=px, y_pitch=py, y_centre=yc, T=T, nx=nx, ny=ny,
                           x_first=0.5 - nx / 2, y_first=0.5 - ny / 2, shape=(K, W, R), G=G)


def inputs(name):
    """The inputs of a case of the table (or of ('sweep', nx)), made once."""
    if name not in _INPUTS:
        if isinstance(name, tuple):
            K, W, R, src, ny = SWEEP_SHAPE
            _INPUTS[name] = make_inputs(K, W, R, src, ny, name[1], "float", seed=5000 + name[1])
        else:
            K, W, R, src, ny, nx, kind = CASES[name]
            _INPUTS[name] = make_inputs(K, W, R, src, ny, nx, kind, seed=4000 + 13 * len(name) + R,
                                        dead_channel=DEAD_CHANNEL if name == "dead-channel" else None,
                                        angles=[np.deg2rad(37.0)] if name == "one-ray" else None)
    return _INPUTS[name]


def csr(src, K):
    """field_start [K+1], field_grids [G]: the grids of fan k are field_grids[field_start[k]:field_start[k+1]], ascending."""
    src = np.asarray(src)
    return (np.concatenate(([0], np.cumsum(np.bincount(src, minlength=K)))).astype(np.int32),
            np.argsort(src, kind="stable").astype(np.int32))


def _weights(a, weight="own"):
    w = a.weight if isinstance(weight, str) else weight
    return np.ones(a.shape) if w is None else (np.asarray(w) != 0).astype(np.float64) if np.asarray(w).dtype in (np.uint8, np.bool_) \
        else np.asarray(w, dtype=np.float64)


def _axis(cu, first, n, extra):
    """psf_ref._axis with the rotation's error of the coordinate (`extra`, pitch units) in place of its `along_y` term."""
    d = cu[..., None] - (first + np.arange(n, dtype=np.float64))
    G = np.exp(-2.0 * d * d)
    dd = 2 * U * np.abs(d) + 3 * U * U * np.abs(cu)[..., None] + extra[..., None]
    rel = U * (2 + 6 * d * d) + 4 * np.abs(d) * dd
    return d, G, dd, rel


def evaluate(a, variant=None, weight="own", bounds=True):
    """The definition on an input namespace in float64: hist [G,W,ny,nx], gx, gy [K,W,R], g_y_centre [K] and (when `bounds`)
    hist_bound, gx_bound, gy_bound of the module docstring, per element."""
    assert variant is None or variant in VARIANTS, variant
    bounds = bounds and variant is None
    K, W, R = a.shape
    G, nx, ny = a.G, a.nx, a.ny
    x, y, T = (np.asarray(v, dtype=np.float64) for v in (a.x, a.y, a.T))
    px, py, yc, c, s = (np.asarray(v, dtype=np.float64) for v in (a.x_pitch, a.y_pitch, a.y_centre, a.c, a.s))
    wt = _weights(a, weight)
    if variant == "sign-s":
        s = -s
    tr = lambda m: m.transpose(0, 2, 1)                                              # noqa: E731
    r = SimpleNamespace(hist=np.zeros((G, W, ny, nx)), gx=np.zeros(a.shape), gy=np.zeros(a.shape))
    if bounds:
        r.hist_bound, r.gx_bound, r.gy_bound = np.zeros(r.hist.shape), np.zeros(a.shape), np.zeros(a.shape)
        mag = np.zeros((2,) + a.shape)                   # sum over the fan's grids of |c| mx + |s| my and of |c| my + |s| mx
    fstart, fgrids = csr(a.src, K)
    nxp = (nx + 3) & ~3
    for g in range(G):
        k = g % K if variant == "src-ignored" else int(a.src[g])
        ykc = yc[g % K] if variant == "centre-per-grid" else yc[k]
        xi, eta, w = x[k], y[k] - ykc, wt[k]
        xr, yr = c[g] * xi + s[g] * eta, -s[g] * xi + c[g] * eta
        ex = SECOND * U * (np.abs(c[g] * xi) + 3 * np.abs(s[g] * eta)) / px[g]
        ey = SECOND * 2 * U * (np.abs(c[g] * eta) + np.abs(s[g] * xi)) / py[g]
        dx, Gx, ddx, relx = _axis(xr / px[g], a.x_first, nx, ex)
        dy, Gy, ddy, rely = _axis(yr / py[g], a.y_first, ny, ey)
        Gxd, Gyd = -4 * dx * Gx, -4 * dy * Gy
        r.hist[g] = np.matmul(tr(w[..., None] * Gy), Gx)
        gxp = w / px[g] * (np.matmul(Gy, T[g]) * Gxd).sum(-1)
        gyp = w / py[g] * (np.matmul(Gyd, T[g]) * Gx).sum(-1)
        cb, sb = (c[g], -s[g]) if variant == "bwd-transposed" else (c[g], s[g])
        last = variant == "last-grid-only"
        if last and g != fgrids[fstart[k + 1] - 1]:
            continue
        r.gx[k] += cb * gxp - sb * gyp
        r.gy[k] += sb * gxp + cb * gyp
        if not bounds:
            continue
        aw = np.abs(w)
        A = aw[..., None] * Gy
        h_mag = np.matmul(tr(A), Gx)
        h_fac = np.matmul(tr(A * rely), Gx) + np.matmul(tr(A), Gx * relx)
        h_floor = TINY * (3 * aw.sum(-1) + 2 * (w != 0).sum(-1) + 2)[:, None, None]
        r.hist_bound[g] = 68 * U * h_mag + h_fac + h_floor
        M = np.abs(T[g])
        Pm, Pr = np.matmul(Gy, M), np.matmul(Gy * rely, M)
        aGxd, aGyd = np.abs(Gxd), np.abs(Gyd)
        gx_mag = aw / px[g] * (Pm * aGxd).sum(-1)
        gx_fac = aw / px[g] * (Pr * aGxd + Pm * (aGxd * relx + 4 * Gx * ddx)).sum(-1)
        Pdm, Pdr = np.matmul(aGyd, M), np.matmul(aGyd * rely + 4 * Gy * ddy, M)
        gy_mag = aw / py[g] * (Pdm * Gx).sum(-1)
        gy_fac = aw / py[g] * (Pdr * Gx + Pdm * Gx * relx).sum(-1)
        col, row = M.sum(1)[:, None, :], M.sum(2)[:, None, :]
        gx_floor = TINY * (1 + aw / px[g] * (ny * nxp + ny + 2 * (col * (2 + 4 * np.abs(dx))).sum(-1)))
        gy_floor = TINY * (1 + aw / py[g] * (ny * nxp + ny + 2 * (row * (2 + 4 * np.abs(dy))).sum(-1)))
        bx = (nx + ny + 4) * U * gx_mag + gx_fac + gx_floor
        by = (nx + ny + 4) * U * gy_mag + gy_fac + gy_floor
        mx, my = np.abs(gxp) + bx, np.abs(gyp) + by
        ac, as_ = abs(c[g]), abs(s[g])
        r.gx_bound[k] += ac * bx + as_ * by + U * (ac * mx + 2 * as_ * my) + 2 * TINY
        r.gy_bound[k] += ac * by + as_ * bx + U * (ac * my + 2 * as_ * mx) + 2 * TINY
        mag[0, k] += ac * mx + as_ * my
        mag[1, k] += ac * my + as_ * mx
    if bounds:
        n = np.diff(fstart).astype(np.float64)[:, None, None]
        r.gx_bound += n * U * mag[0]
        r.gy_bound += n * U * mag[1]
    r.g_y_centre = -r.gy.reshape(K, -1).sum(1)
    return r


def reference(name):
    """evaluate() of a case (or of ('sweep', nx)): computed once, never changed."""
    if name not in _REF:
        _REF[name] = evaluate(inputs(name))
    return _REF[name]


def ratio(got, want, limit):
    """The largest |got - want| / limit over ALL elements; 0 / 0 counts as 0, a non-finite `got` as inf."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape == np.shape(limit), (got.shape, want.shape, np.shape(limit))
    assert np.isfinite(want).all() and np.isfinite(limit).all()
    if not np.isfinite(got).all():
        return float("inf")
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / limit)
    return float(q.max()) if q.size else 0.0


def ratios(got, r):
    """{'hist': .., 'gx': .., 'gy': ..}: the largest error / bound of each result in `got` against the reference r."""
    return {k: ratio(got[k], getattr(r, k), getattr(r, k + "_bound")) for k in RESULTS if got.get(k) is not None}


def centre_ratio(g_y_centre, gy32):
    """g_y_centre [K] against the exact float64 sum of the float32 gy [K,W,R] it was reduced from: error / tolerance, the
    tolerance U |S| + n 2^-53 sum |terms| of one float32 rounding of a float64 sum of n terms taken in any order."""
    gy = np.asarray(gy32, dtype=np.float64)
    K, n = gy.shape[0], gy.shape[1] * gy.shape[2]
    S = np.array([-math.fsum(gy[k].ravel()) for k in range(K)])
    tol = U * np.abs(S) + n * 2.0 ** -53 * np.abs(gy).reshape(K, -1).sum(1)
    return ratio(g_y_centre, S, np.where(tol == 0, TINY, tol))


def blend(hist, cell, beta, n_cells, hist_bound=None, beta_first=False):
    """psf [N,W,ny,nx] = sum over the terms t of cell n of beta_t hist[t] / sum_ij hist[t], and its bound when hist's is given.
    `beta_first` (WRONG): the terms are blended first and the blend is normalised."""
    hist = np.asarray(hist, dtype=np.float64)
    S = hist.sum((-1, -2), keepdims=True)
    out = np.zeros((n_cells,) + hist.shape[1:])
    if beta_first:
        np.add.at(out, cell, beta[:, None, None, None] * hist)
        return out / out.sum((-1, -2), keepdims=True)
    np.add.at(out, cell, beta[:, None, None, None] * hist / S)
    if hist_bound is None:
        return out
    bS = hist_bound.sum((-1, -2), keepdims=True)
    b = np.zeros_like(out)
    np.add.at(b, cell, beta[:, None, None, None] * (hist_bound / np.abs(S) + np.abs(hist) * bS / S ** 2) * (1 + 2 * bS / np.abs(S)))
    return out, b + 4 * U * np.abs(out)


# ------------------------------------------------------------------------------------------ the kernels' arithmetic in float32

def emulate(a, rotate_dead=False, seed=0):
    """hist, gx, gy as the kernels compute them, in float32 numpy: the rotation (a product and an fma per coordinate, dead rays
    dropped first) in front of psf_cases.emulate grid by grid, then the turn back and the sum in list order.
    `rotate_dead` (WRONG): a ray of weight 0 keeps its coordinates through the rotation and its weight 0 after it."""
    K, W, R = a.shape
    G = a.G
    wt = np.ones(a.shape, np.float32) if a.weight is None else (a.weight != 0).astype(np.float32) if a.weight.dtype == np.uint8 \
        else a.weight
    live = wt != 0
    keep = np.ones_like(live) if rotate_dead else live
    with np.errstate(invalid="ignore"):
        xi = np.where(keep, a.x, np.float32(0))
        eta = np.where(keep, a.y - a.y_centre[:, None, None], np.float32(0))
    hist = np.zeros((G, W, a.ny, a.nx), np.float32)
    gx, gy = np.zeros(a.shape, np.float32), np.zeros(a.shape, np.float32)
    fstart, _ = csr(a.src, K)
    first = np.ones(K, bool)
    for g in range(G):
        k = int(a.src[g])
        c, s = a.c[g], a.s[g]
        with np.errstate(invalid="ignore"):
            xr = pc._fma(c, xi[k], s * eta[k])
            yr = pc._fma(c, eta[k], -(s * xi[k]))
        b = SimpleNamespace(x=xr[None], y=yr[None], weight=wt[k][None], x_pitch=a.x_pitch[g:g + 1], y_pitch=a.y_pitch[g:g + 1],
                            y_centre=np.zeros(1, np.float32), T=a.T[g][None], nxh=a.nx, ny=a.ny, x_first=a.x_first,
                            y_first=a.y_first, shape=(1, W, R))
        with np.errstate(invalid="ignore", over="ignore"):
            e = pc.emulate(b, seed=seed + g)             # (drops the dead rays itself, as load_ray does)
        if rotate_dead:
            # what such a kernel would do with the dead ray it kept: A = fl(0 * Gy(NaN)) = NaN, and the NaN reaches the tile
            nan_hit = (~live[k] & ~(np.isfinite(xr) & np.isfinite(yr))).any(-1)
            e["hist"] = np.where(nan_hit[:, None, None], np.float32(np.nan), e["hist"])
        hist[g] = e["hist"]
        tx = pc._fma(c, e["gx"], -(s * e["gy"]))
        ty = pc._fma(c, e["gy"], s * e["gx"])
        gx[k] = tx if first[k] else gx[k] + tx
        gy[k] = ty if first[k] else gy[k] + ty
        first[k] = False
    gx, gy = np.where(live, gx, np.float32(0)), np.where(live, gy, np.float32(0))
    assert hist.dtype == gx.dtype == gy.dtype == np.float32
    return {"hist": hist, "gx": gx, "gy": gy}


# --------------------------------------------------------------------------------------------------------------- the op

LEAVES = ("x", "y", "y_centre")


def tensors(a, device):
    """The arrays of an input namespace as fresh torch tensors on `device` (weight None stays None)."""
    names = LEAVES + ("weight", "T", "x_pitch", "y_pitch")
    return {n: None if getattr(a, n) is None else torch.from_numpy(getattr(a, n).copy()).to(device) for n in names}


def run(ops, t, a, needs=LEAVES):
    """ops.PsfRotAccumulateFunction on the tensors t and the backward of sum(hist * T): float32 numpy arrays 'hist', then
    'gx', 'gy', 'g_y_centre' for the leaves in `needs` (None for the others), and 'saved_x_ptr'."""
    for n in LEAVES:
        if n in needs:
            t[n].requires_grad_(True) if t[n].is_leaf else t[n].retain_grad()
        else:
            assert not t[n].requires_grad
    grid = ops.psf_rot_grid(a.src, a.c, a.s, a.shape[0])
    hist = ops.PsfRotAccumulateFunction.apply(t["x"], t["y"], t["weight"], grid, t["x_pitch"], t["y_pitch"], t["y_centre"],
                                              a.nx, a.ny, a.x_first, a.y_first)
    out = {"saved_x_ptr": hist.grad_fn.saved_tensors[0].data_ptr()}
    (hist * t["T"]).sum().backward()
    out["hist"] = hist.detach()
    for n, key in zip(LEAVES, ("gx", "gy", "g_y_centre")):
        out[key] = t[n].grad
    return {k: v.cpu().numpy() if torch.is_tensor(v) else v for k, v in out.items()}
