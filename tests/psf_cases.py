"""The shapes of the fused-PSF kernel tests (csrc/tl_psf.hip behind ops.PsfAccumulateFunction), shared by
tests/test_gpu_psf_matrix.py (the kernels) and tests/test_psf_cases_cpu.py (the plan mirror, and the bounds held to be
sufficient and sharp without a GPU): the case table, a Python mirror of the launch plan, seeded inputs, the error bounds, a
float32 emulation of the kernels' arithmetic, and the helper that runs the op on a case.

Each case is the smallest shape that reaches its branch; G != W wherever both exceed 1 (G x W x R rays, ny x nxh bins):
    one-ray        1 x 1 x 1,      32 x 29  one live lane in the launch; all 32 rows and 29 columns of the MFMA tile; <32>
    sub-wave       2 x 3 x 63,      5 x 17  the only batch of the only wave is partial; <20>; `ok` bytes
    wave-plus-one  3 x 2 x 65,      1 x 21  the second wave holds one ray; ny = 1; <24>; no weights
    block-edge     3 x 2 x 257,    32 x 25  two blocks each way, the second holds one ray; <28>
    reduce-17      1 x 2 x 4161,    7 x 1   17 forward partials: the 16-stride loop of psf_reduce_kernel, then its tail; nxh = 1,
                                            so three of the four columns the backward reads are padding; `ok` bytes
    plan-3         10 x 13 x 4133, 21 x 11  nb = 3 batches per wave (6 blocks, the last ragged), rpl = 2 rays per lane (9 blocks)
    many-grids     255 x 257 x 3,   2 x 2   G W = 65535, the largest grid-y; nb = 16 with one batch to take
    dead-channel   2 x 3 x 300,    10 x 4   every weight of channel (1, 1) is 0: its tile and its gradients are exactly 0
The pitches and centres differ from grid to grid and y_pitch != x_pitch; y_centre runs from 1e-4 to 3 mm; y_first = 1/2 - ny/2
is an integer for odd ny and a half-integer for even ny, x_first is 0 (odd nx) or 1/2 (even nx) case by case; the rays are spread
over the tile and 1.5 pixels beyond.  Float weights are +-[0.1, 1.5]; the seventh of every seven rays (counted over the whole
[G, W, R] block, so short fans have some too) has weight 0.  EXPECT states the plan every case must land on, (nb, nbx_fwd, rpl,
nbx_bwd, NXP); `plan` mirrors psf_plan of tl_psf.hip and the CPU test holds it to tl_psf_workspace_bytes.

THE BOUNDS.  U = 2^-24 (half an ulp, relative), TINY = 2^-126; every bound is per element, from sums that psf_ref.py returns
next to each result.  Counted from tl_psf.hip:

  * A distance d to a pixel centre.  u = fl(x / p) and the remainder x - u p is a float32 number, so the fma is exact and
    u + ul = x / p up to the rounding of ul, U |ul| <= U^2 |u|.  The centre a = first + k is exact.  fl(u - a) is NOT always
    exact (u = 3.7, a = 20 loses bits of u), but it is one rounding of a number of size |d| + |ul|, and the add of ul is another:
    |dd| <= 2 U |d| + 3 U^2 |u|.  Along y the difference y - y_centre is rounded before the divide: + U |v|.
  * A Gaussian exp2(fl(fl(kC d) d)): the constant and two products are 3 U relative in the argument, which is 2 d^2 ln-units:
    6 U d^2; the hardware exp2 is taken at 1 ulp = 2 U; the error of d adds |G'| dd / G = 4 |d| dd:
        rel = U (2 + 6 d^2) + 4 |d| dd,
    and absolutely at least TINY: results below the smallest normal may be flushed, where float64 keeps 1e-40.
  * hist.  fl(wt Gy) is 1 rounding; v_mfma_f32_32x32x2_f32 adds the 64 rays of a batch in one chain of fused multiply-adds, 64
    roundings of partial sums no larger than the sum of the absolute terms; the batch totals are added in float64; the block's
    partial tile and the result are one float32 rounding each: 1 + 64 + 2 = 67, and 68 leaves one for the second order.
        |hist - ref| <= 68 U sum_r |wt| Gy Gx + sum_r |wt| Gy Gx (rel_y + rel_x) + TINY (3 sum |wt| + 2 n_live + 2)
    (a flushed factor costs |wt| TINY, a flushed product or batch TINY).
  * gx, gy per ray.  G' = fl(fl(-4 d) G): the product with -4 is exact, so G' carries rel + U and the error of its own d,
    4 G dd.  The chain over the columns is nxh roundings (the padded columns add fma(0, G, s) = s exactly, so it is nxh and not
    NXP), the chain over the rows ny, the weight and the divide one each: with one for the second order
        |gx - ref| <= (nxh + ny + 4) U M + |wt| / x_pitch sum_ij |T_ij| Gy_i (|Gx'_j| (rel_y_i + rel_x_j) + 4 Gx_j dd_j) + floor,
        M = |wt| / x_pitch sum_ij |T_ij| Gy_i |Gx'_j|,  and likewise for gy.
    (Where this count differs from a looser one -- two roundings for G', NXP for the chain -- it is by the two remarks above.)
  * g_x_pitch, g_y_pitch, g_y_centre are sums over W R rays that cancel, so a worst-case bound from the absolute terms says
    nothing.  They are held in two steps: gx, gy to the reference as above, and each per-grid gradient to the float64 sum of
    the kernel's OWN float32 gx, gy (psf_ref.grid_sums) within U |S| + n 2^-53 sum |terms|: float64 products of two float32
    numbers are exact, so this is one float32 rounding of a float64 sum of n terms in any order.  Their relative error
    against the float64 reference is printed, not asserted.

`emulate` follows the kernels in float32 numpy (remainder, k-ordered chains of 64, float64 totals, one float32 partial per block
of the mirrored plan, the two backward chains) with an exp2 that returns either float32 neighbour of the true value on a
seeded coin: within 1 ulp, as the hardware's is taken to be."""
from types import SimpleNamespace

import numpy as np
import torch

import psf_ref as ref

U, TINY = ref.U, ref.TINY
KC = np.float32(-2.885390081777927)
BLOCK, WAVES = 256, 4

# G, W, R, ny, nxh, x_first, weight kind
CASES = {
    "one-ray": (1, 1, 1, 32, 29, 0.0, "float"),
    "sub-wave": (2, 3, 63, 5, 17, 0.5, "ok"),
    "wave-plus-one": (3, 2, 65, 1, 21, 0.0, None),
    "block-edge": (3, 2, 257, 32, 25, 0.5, "float"),
    "reduce-17": (1, 2, 4161, 7, 1, 0.0, "ok"),
    "plan-3": (10, 13, 4133, 21, 11, 0.0, "float"),
    "many-grids": (255, 257, 3, 2, 2, 0.5, "float"),
    "dead-channel": (2, 3, 300, 10, 4, 0.5, "float"),
}
# nb, nbx_fwd, rpl, nbx_bwd, NXP
EXPECT = {
    "one-ray": (1, 1, 1, 1, 32),
    "sub-wave": (1, 1, 1, 1, 20),
    "wave-plus-one": (1, 1, 1, 1, 24),
    "block-edge": (1, 2, 1, 2, 28),
    "reduce-17": (1, 17, 1, 17, 4),
    "plan-3": (3, 6, 2, 9, 12),
    "many-grids": (16, 1, 1, 1, 4),
    "dead-channel": (1, 2, 1, 2, 4),
}
DEAD_CHANNEL = (1, 1)
SWEEP_NXH = (1, 4, 5, 8, 12, 13, 16, 17, 20, 24, 25, 28, 29, 32)       # all eight instantiations, each at both ends
SWEEP_SHAPE = (2, 3, 321, 3)                                           # G, W, R, ny
RESULTS = ("hist", "gx", "gy")
GRID = ("g_x_pitch", "g_y_pitch", "g_y_centre")
LEAVES = ("x", "y", "x_pitch", "y_pitch", "y_centre")

_INPUTS, _REF = {}, {}


def _cdiv(a, b):
    return -(-a // b)


def plan(G, W, R, nxh, ny):
    """psf_plan of csrc/tl_psf.hip: nb, nbx_fwd, rpl, nbx_bwd, nxp and the bytes tl_psf_workspace_bytes returns."""
    GW, batches = G * W, _cdiv(R, 64)
    nb = min(max(_cdiv(batches * GW, WAVES * 1024), 1), 256)
    nbx_fwd = _cdiv(batches, WAVES * nb)
    rpl = min(max(_cdiv(R * GW, BLOCK * 2048), 1), 64)
    nbx_bwd = _cdiv(R, BLOCK * rpl)
    nxp = (nxh + 3) & ~3
    fwd = GW * nbx_fwd * ny * nxh * 4
    gpad = (GW * ny * nxp * 4 + 255) & ~255
    bwd = gpad + GW * nbx_bwd * 3 * 8
    return SimpleNamespace(nb=nb, nbx_fwd=nbx_fwd, rpl=rpl, nbx_bwd=nbx_bwd, nxp=nxp, workspace=max(fwd, bwd) + 256)


def _f32(v):
    return np.asarray(v, dtype=np.float64).astype(np.float32)


def make_inputs(G, W, R, ny, nxh, x_first, kind, seed, yc_range=(1e-4, 3.0), dead_channel=None):
    """Seeded float32 inputs of one shape: a namespace of x, y [G,W,R], weight (float32, uint8 or None), x_pitch, y_pitch,
    y_centre [G], T [G,W,ny,nxh], and the scalars."""
    rng = np.random.default_rng(seed)
    k = np.arange(G)
    px = _f32(0.004 * (1 + 0.13 * (k % 5) + 0.0007 * k))
    py = _f32(0.0031 * (1 + 0.17 * ((k + 2) % 5) + 0.0009 * k))
    yc = _f32(np.linspace(yc_range[0], yc_range[1], G) if G > 1 else [yc_range[0]])
    y_first = 0.5 - ny / 2
    u = rng.uniform(x_first - 1.5, x_first + nxh + 0.5, (G, W, R))
    v = rng.uniform(y_first - 1.5, y_first + ny + 0.5, (G, W, R))
    x = _f32(u * px.astype(np.float64)[:, None, None])
    y = _f32(yc.astype(np.float64)[:, None, None] + v * py.astype(np.float64)[:, None, None])
    dead = np.arange(G * W * R).reshape(G, W, R) % 7 == 3
    if dead_channel is not None:
        dead[dead_channel] = True
    mag = rng.uniform(0.1, 1.5, (G, W, R)) * (2.0 * rng.integers(0, 2, (G, W, R)) - 1.0)
    weight = {"float": _f32(np.where(dead, 0.0, mag)), "ok": (~dead).astype(np.uint8), None: None}[kind]
    T = _f32(rng.normal(0, 1, (G, W, ny, nxh)))
    return SimpleNamespace(x=x, y=y, weight=weight, x_pitch=px, y_pitch=py, y_centre=yc, T=T, nxh=nxh, ny=ny,
                           x_first=float(x_first), y_first=float(y_first), shape=(G, W, R))


def inputs(name):
    """The inputs of a case of the table, made once."""
    if name not in _INPUTS:
        G, W, R, ny, nxh, x_first, kind = CASES[name]
        _INPUTS[name] = make_inputs(G, W, R, ny, nxh, x_first, kind, seed=2000 + 13 * len(name) + R,
                                    yc_range=(3.001, 3.001) if name == "one-ray" else (1e-4, 3.0),
                                    dead_channel=DEAD_CHANNEL if name == "dead-channel" else None)
    return _INPUTS[name]


def sweep_inputs(nxh):
    key = ("sweep", nxh)
    if key not in _INPUTS:
        G, W, R, ny = SWEEP_SHAPE
        _INPUTS[key] = make_inputs(G, W, R, ny, nxh, 0.5 * (nxh % 2), "float", seed=3000 + nxh)
    return _INPUTS[key]


def evaluate(a, weight="own", **kw):
    """psf_ref.evaluate on an input namespace (weight: another weight array in place of the namespace's)."""
    w = a.weight if isinstance(weight, str) else weight
    return ref.evaluate(a.x, a.y, w, a.x_pitch, a.y_pitch, a.y_centre, a.nxh, a.ny, a.x_first, a.y_first, a.T, **kw)


def reference(name):
    """psf_ref.evaluate of a case (or of ('sweep', nxh)): computed once, never changed."""
    if name not in _REF:
        _REF[name] = evaluate(sweep_inputs(name[1]) if isinstance(name, tuple) else inputs(name))
    return _REF[name]


def bound(r, what, a):
    """The bound of the module docstring for result `what` ('hist', 'gx', 'gy') of the reference namespace r, per element."""
    count = 68 if what == "hist" else a.nxh + a.ny + 4
    return count * U * getattr(r, what + "_mag") + getattr(r, what + "_fac") + getattr(r, what + "_floor")


def ratio(got, want, limit):
    """The largest |got - want| / limit over ALL elements (0 / 0 counts as 0, anything else over 0 as inf)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape == np.shape(limit), (got.shape, want.shape, np.shape(limit))
    assert np.isfinite(got).all() and np.isfinite(want).all() and np.isfinite(limit).all()
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / limit)
    return float(q.max()) if q.size else 0.0


def ratios(got, r, a):
    """{'hist': .., 'gx': .., 'gy': ..}: the largest error / bound of each result in `got` against the reference r."""
    return {k: ratio(got[k], getattr(r, k), bound(r, k, a)) for k in RESULTS if got.get(k) is not None}


def grid_ratios(got, a):
    """The three per-grid gradients of `got` against the float64 sums of its own gx, gy: the largest error / tolerance each."""
    S, tol = ref.grid_sums(got["gx"], got["gy"], a.x, a.y, a.x_pitch, a.y_pitch, a.y_centre)
    return {k: ratio(got[k], S[k], tol[k]) for k in GRID}


def grid_rel(got, r):
    """For the record: the largest relative error of each per-grid gradient against the float64 reference."""
    return {k: float((np.abs(got[k].astype(np.float64) - getattr(r, k)) / np.abs(getattr(r, k))).max()) for k in GRID}


# ------------------------------------------------------------------------------------------ the kernels' arithmetic in float32

def _fma(a, b, c):
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + c).astype(np.float32)


def _exp2(arg, rng):
    """exp2 within 1 ulp: one of the two float32 neighbours of the true value, by a seeded coin."""
    true = np.exp2(arg.astype(np.float64))
    with np.errstate(under="ignore"):
        near = true.astype(np.float32)
    lo = np.where(near.astype(np.float64) > true, np.nextafter(near, np.float32(-np.inf)), near)
    hi = np.where(lo.astype(np.float64) < true, np.nextafter(lo, np.float32(np.inf)), lo)
    return np.where(rng.integers(0, 2, arg.shape) == 1, hi, lo).astype(np.float32)


def _gauss(d, rng):
    return _exp2((KC * d) * d, rng)


def emulate(a, channels=None, seed=0):
    """hist, gx, gy of the channels [(g, w), ...] (all by default) as the kernels compute them, in float32 numpy under the
    mirrored plan: {'hist': [C,ny,nxh], 'gx': [C,R], 'gy': [C,R]}."""
    rng = np.random.default_rng(seed)
    G, W, R = a.shape
    if channels is None:
        channels = [(g, w) for g in range(G) for w in range(W)]
    gi, wi = (np.array(v) for v in zip(*channels))
    C, nxh, ny = len(channels), a.nxh, a.ny
    pl = plan(G, W, R, nxh, ny)
    x, y = a.x[gi, wi], a.y[gi, wi]
    wt = np.ones((C, R), np.float32) if a.weight is None else (a.weight[gi, wi] != 0).astype(np.float32) \
        if a.weight.dtype == np.uint8 else a.weight[gi, wi]
    px, py, yc = (v[gi][:, None] for v in (a.x_pitch, a.y_pitch, a.y_centre))
    live = wt != 0
    x0, yc0 = np.where(live, x, np.float32(0)), np.where(live, y - yc, np.float32(0))
    u, v = x0 / px, yc0 / py
    ul, vl = _fma(-u, px, x0) / px, _fma(-v, py, yc0) / py
    assert all(t.dtype == np.float32 for t in (u, v, ul, vl, wt))
    ax = (np.float32(a.x_first) + np.arange(nxh, dtype=np.float32))
    ay = (np.float32(a.y_first) + np.arange(ny, dtype=np.float32))
    T = a.T[gi, wi]

    # forward: chains of 64 rays in the order of the MFMA steps (ray s, then ray s + 32), float64 totals, one float32 partial
    # per block of 4 nb batches, the partials added in float64 and rounded once
    nbat = _cdiv(R, 64)
    pad = lambda t: np.concatenate((t, np.zeros((C, nbat * 64 - R), np.float32)), axis=1).reshape(C, nbat, 64)   # noqa: E731
    up, vp, ulp, vlp, wp = (pad(t) for t in (u, v, ul, vl, wt))
    acc = np.zeros((C, nbat, ny, nxh), np.float32)
    for s in range(32):
        for k in (s, s + 32):
            A = wp[..., k, None] * _gauss((vp[..., k, None] - ay) + vlp[..., k, None], rng)
            B = _gauss((up[..., k, None] - ax) + ulp[..., k, None], rng)
            acc = _fma(A[..., :, None], B[..., None, :], acc)
    tot = acc.astype(np.float64)
    per_block = WAVES * pl.nb
    part = np.stack([tot[:, b * per_block:(b + 1) * per_block].sum(1).astype(np.float32) for b in range(pl.nbx_fwd)])
    assert pl.nbx_fwd * per_block >= nbat
    hist = part.astype(np.float64).sum(0).astype(np.float32)

    # backward: one ray per lane, the chain over the columns inside the chain over the rows
    dx = (u[..., None] - ax) + ul[..., None]
    Gx = _gauss(dx, rng)
    Gd = (np.float32(-4) * dx) * Gx
    Aq, Bq = np.zeros((C, R), np.float32), np.zeros((C, R), np.float32)
    for i in range(ny):
        dy = (v - ay[i]) + vl
        Gy = _gauss(dy, rng)
        Gyd = (np.float32(-4) * dy) * Gy
        s1, s2 = np.zeros((C, R), np.float32), np.zeros((C, R), np.float32)
        for j in range(nxh):
            gij = T[:, i, j, None]
            s1, s2 = _fma(gij, Gd[..., j], s1), _fma(gij, Gx[..., j], s2)
        Aq, Bq = _fma(Gy, s1, Aq), _fma(Gyd, s2, Bq)
    gx = np.where(live, wt * Aq / px, np.float32(0))
    gy = np.where(live, wt * Bq / py, np.float32(0))
    assert hist.dtype == gx.dtype == gy.dtype == np.float32
    return {"hist": hist, "gx": gx, "gy": gy}


# --------------------------------------------------------------------------------------------------------------- the op

def tensors(a, device):
    """The arrays of an input namespace as fresh torch tensors on `device` (weight None stays None)."""
    names = LEAVES + ("weight", "T")
    return {n: None if getattr(a, n) is None else torch.from_numpy(getattr(a, n).copy()).to(device) for n in names}


def run(ops, t, a, needs=LEAVES):
    """ops.PsfAccumulateFunction on the tensors t (of `tensors`, or replaced by views and other dtypes) and the backward of
    sum(hist * T).  Returns float32 numpy arrays: 'hist', then 'gx', 'gy', 'g_x_pitch', 'g_y_pitch', 'g_y_centre' for the leaves
    in `needs` and None for the others, 'g_hist' (what the backward was handed) and 'saved_x_ptr' (the data pointer of the x
    the kernels read)."""
    for n in LEAVES:
        if n in needs:
            t[n].requires_grad_(True) if t[n].is_leaf else t[n].retain_grad()
        else:
            assert not t[n].requires_grad
    hist = ops.PsfAccumulateFunction.apply(t["x"], t["y"], t["weight"], t["x_pitch"], t["y_pitch"], t["y_centre"], a.nxh, a.ny,
                                           a.x_first, a.y_first)
    seen = []
    hist.register_hook(lambda g: seen.append(g.detach().clone()))
    out = {"saved_x_ptr": hist.grad_fn.saved_tensors[0].data_ptr()}
    (hist * t["T"]).sum().backward()
    out["hist"], out["g_hist"] = hist.detach(), seen[0]
    for n, key in zip(LEAVES, ("gx", "gy") + GRID):
        out[key] = t[n].grad
    return {k: v.cpu().numpy() if torch.is_tensor(v) else v for k, v in out.items()}


def same_bits(p, q):
    """Two float32 arrays hold the same bits (NaNs and the sign of zero included)."""
    p, q = np.ascontiguousarray(p), np.ascontiguousarray(q)
    return p.dtype == q.dtype == np.float32 and p.shape == q.shape and np.array_equal(p.view(np.uint32), q.view(np.uint32))
