"""An independent float64 evaluation of imaging.warp_bicubic in numpy, written from the definition with explicit index arrays
(it shares no code with torchoptics_amd/imaging.py), with all five gradients of sum(g_out * out) and, next to each result, the
magnitudes that the error bounds of tests/warp_cases.py need.

    xc = clamp(x, -1, 1), u = (xc + 1) / 2 (W - 1), j0 = floor(u), t = u - j0, columns clip(j0 - 1 .. j0 + 2, 0, W - 1), rows
    likewise;  out = gain sum_i sum_j wy_i wx_j image[b, row_i, col_j, c]  with the cubic convolution weights of alpha.

Magnitudes.  For every weight family f (the weights w, their derivatives dw and second derivatives ddw) there is the family of
the sums of the absolute values of its monomials, A(t) = sum_k |coef_k| t^k >= |f(t)|, which is what the rounding error of a
Horner evaluation is proportional to.  `T(fy, fx)` below is sum_i sum_j fy_i fx_j |image| at the 16 taps.

An fp32 evaluation rounds u, and when u lies within its rounding error of an integer it may work in the neighbouring cell: the
same point of the same C1 interpolant, but other taps and weights near (0, 1, 0, 0) seen from the other side, with other
monomial sums.  So every magnitude is the LARGEST over the cells an fp32 evaluation may use: the cell of floor(u), and, when t
is within 4 x 2^-24 (n - 1) of 0 or 1, the neighbouring cell with t + 1 or t - 1.  (For the scattered image gradient the
magnitudes of those cells are added instead, which is larger still.)

`variant` evaluates a deliberately WRONG definition, for the tests that hold the bounds to be sharp:
    'alpha' alpha = -0.5 | 'swap' x and y exchanged | 'tap' one column tap displaced by a pixel | 'wrap' indices wrapped
    instead of clipped | 'factor' the (W - 1)/2 missing from g_x"""
from types import SimpleNamespace

import numpy as np

ALPHA = -0.75
U = 2.0 ** -24
K2, K3 = 4.5, 7.5          # the largest |second| and |third| derivative of a product of two weights on [0, 1]


def _families(t, a):
    """w, dw, ddw [4, ...] at t, and the monomial-magnitude families A (of w), dA (of dw) at |t|."""
    w = np.stack([a * (t ** 3 - 2 * t ** 2 + t), (a + 2) * t ** 3 - (a + 3) * t ** 2 + 1,
                  -(a + 2) * t ** 3 + (2 * a + 3) * t ** 2 - a * t, a * (t ** 2 - t ** 3)])
    dw = np.stack([a * (3 * t ** 2 - 4 * t + 1), 3 * (a + 2) * t ** 2 - 2 * (a + 3) * t,
                   -3 * (a + 2) * t ** 2 + 2 * (2 * a + 3) * t - a, a * (2 * t - 3 * t ** 2)])
    ddw = np.stack([a * (6 * t - 4), 6 * (a + 2) * t - 2 * (a + 3), -6 * (a + 2) * t + 2 * (2 * a + 3), a * (2 - 6 * t)])
    s, b = np.abs(t), abs(a)
    A = np.stack([b * (s ** 3 + 2 * s ** 2 + s), abs(a + 2) * s ** 3 + abs(a + 3) * s ** 2 + 1,
                  abs(a + 2) * s ** 3 + abs(2 * a + 3) * s ** 2 + b * s, b * (s ** 2 + s ** 3)])
    dA = np.stack([b * (3 * s ** 2 + 4 * s + 1), 3 * abs(a + 2) * s ** 2 + 2 * abs(a + 3) * s,
                   3 * abs(a + 2) * s ** 2 + 2 * abs(2 * a + 3) * s + b, b * (2 * s + 3 * s ** 2)])
    return dict(w=w, dw=dw, ddw=ddw, A=A, dA=dA, aw=np.abs(w), adw=np.abs(dw), addw=np.abs(ddw), one=np.ones_like(w))


def _index(j0, n, wrap):
    taps = np.stack([j0 - 1, j0, j0 + 1, j0 + 2])
    return np.mod(taps, n) if wrap else np.clip(taps, 0, n - 1)


def axis(x, n, alpha=ALPHA, wrap=False):
    """One axis: x [...] float64 -> the cells an evaluation may use, [(idx [4, ...] int, families, valid [...] bool)]; the first
    is the cell of floor(u) and is valid everywhere; `passes` [...]: -1 <= x <= 1; `du`: the bound on the fp32 rounding of u."""
    xc = np.where(x < -1, -1.0, np.where(x > 1, 1.0, x))
    u = (xc + 1) / 2 * (n - 1)
    nan = np.isnan(u)
    fl = np.floor(np.where(nan, 0.0, u))
    j0 = fl.astype(np.int64)
    t = u - fl                                                  # NaN where u is NaN
    cells = [(_index(j0, n, wrap), _families(t, alpha), np.ones(x.shape, dtype=bool))]
    eps = 4 * U * max(n - 1, 1)
    with np.errstate(invalid="ignore"):
        low, high = t < eps, t > 1 - eps
    cells.append((_index(j0 - 1, n, wrap), _families(np.where(low, t + 1, 1.0), alpha), low))
    cells.append((_index(j0 + 1, n, wrap), _families(np.where(high, t - 1, 0.0), alpha), high))
    return SimpleNamespace(cells=cells, passes=(x >= -1) & (x <= 1) | np.isnan(x), du=2 * U * (n - 1))


def _taps(img, rows, cols, fy, fx):
    """sum_i sum_j fy_i fx_j img[b, rows_i, cols_j, :]  ->  [B, Ho, Wo, C]"""
    b = np.arange(img.shape[0])[:, None, None]
    out = 0.0
    for i in range(4):
        row = 0.0
        for j in range(4):
            row = row + fx[j][..., None] * img[b, rows[i], cols[j]]
        out = out + fy[i][..., None] * row
    return out


def evaluate(image, x, y, gain, g_out, variant=None):
    """image [B,H,W,C], x, y [B or 1,Ho,Wo], gain [B or 1,Ho,Wo,C or 1] or None, g_out [B,Ho,Wo,C]: float64 arrays.  Returns a
    namespace of out, g_x, g_y, g_gain (None without gain), g_image, and for each of them NAME_round (the sum of absolute
    terms that the rounding of the weights, the sums and the products is relative to), NAME_coord (the first- and second-order
    effect of the fp32 rounding of u and v) and NAME_terms (how many terms the longest in-lane sum adds up)."""
    image, x, y, g_out = (np.asarray(v, dtype=np.float64) for v in (image, x, y, g_out))
    B, H, W, C = image.shape
    alpha = -0.5 if variant == "alpha" else ALPHA
    if variant == "swap":
        x, y = y, x
    shape = (B,) + x.shape[1:]
    ax = axis(np.broadcast_to(x, shape), W, alpha, wrap=variant == "wrap")
    ay = axis(np.broadcast_to(y, shape), H, alpha, wrap=variant == "wrap")
    (cols, fx, _), (rows, fy, _) = ax.cells[0], ay.cells[0]
    if variant == "tap":
        cols = cols.copy()
        cols[2] = np.clip(cols[2] + 1, 0, W - 1)
    G = np.ones((1, 1, 1, 1)) if gain is None else np.asarray(gain, dtype=np.float64)
    Gb = np.broadcast_to(G, (B,) + shape[1:] + (C,))
    S = _taps(image, rows, cols, fy["w"], fx["w"])
    Sx = _taps(image, rows, cols, fy["w"], fx["dw"])
    Sy = _taps(image, rows, cols, fy["dw"], fx["w"])
    kx, ky = (W - 1) / 2, (H - 1) / 2
    a = g_out * Gb
    r = SimpleNamespace(out=Gb * S)
    share_c = lambda v, like: v.sum(axis=0, keepdims=True) if like.shape[0] == 1 and B > 1 else v      # noqa: E731
    r.g_x = share_c(np.where(ax.passes, (1.0 if variant == "factor" else kx) * (a * Sx).sum(-1), 0.0), x)
    r.g_y = share_c(np.where(ay.passes, ky * (a * Sy).sum(-1), 0.0), y)

    def share_g(v):
        if gain is None:
            return None
        v = v.sum(axis=0, keepdims=True) if G.shape[0] == 1 and B > 1 else v
        return v.sum(axis=3, keepdims=True) if G.shape[3] == 1 and C > 1 else v
    r.g_gain = share_g(g_out * S)
    b = np.arange(B)[:, None, None]
    r.g_image = np.zeros_like(image)
    for i in range(4):
        for j in range(4):
            np.add.at(r.g_image, (b, rows[i], cols[j]), (fy["w"][i] * fx["w"][j])[..., None] * a)

    # ------------------------------------------------------------------------------------------------------ magnitudes
    absI, absA, absG = np.abs(image), np.abs(a), np.abs(g_out)
    du, dv = ax.du, ay.du

    def T(ny, nx):
        """The largest of sum_ij fy_i fx_j |image| over the cells an fp32 evaluation may use."""
        best = None
        for ry, famy, oky in ay.cells:
            for cx, famx, okx in ax.cells:
                ok = (oky & okx)[..., None]
                if not ok.any():
                    continue
                with np.errstate(invalid="ignore"):
                    v = np.where(ok, _taps(absI, ry, cx, famy[ny], famx[nx]), 0.0)
                best = v if best is None else np.fmax(best, v)
        return best

    second = 0.5 * (du + dv) ** 2 * T("one", "one")
    val_round, val_coord = T("A", "A"), du * T("aw", "adw") + dv * T("adw", "aw") + K2 * second
    r.out_round, r.out_coord, r.out_terms = np.abs(Gb) * val_round, np.abs(Gb) * val_coord, 1
    n_xy = C * (B if x.shape[0] == 1 else 1)
    r.g_x_round = share_c(kx * (absA * T("A", "dA")).sum(-1), x)
    r.g_x_coord = share_c(kx * (absA * (du * T("aw", "addw") + dv * T("adw", "adw") + K3 * second)).sum(-1), x)
    r.g_y_round = share_c(ky * (absA * T("dA", "A")).sum(-1), y)
    r.g_y_coord = share_c(ky * (absA * (du * T("adw", "adw") + dv * T("addw", "aw") + K3 * second)).sum(-1), y)
    r.g_x_terms = r.g_y_terms = n_xy
    r.g_gain_round, r.g_gain_coord = share_g(absG * val_round), share_g(absG * val_coord)
    r.g_gain_terms = 1 if gain is None else (B if G.shape[0] == 1 else 1) * (C if G.shape[3] == 1 else 1)
    r.g_image_round, r.g_image_coord, count = np.zeros_like(image), np.zeros_like(image), np.zeros_like(image)
    for ry, famy, oky in ay.cells:
        for cx, famx, okx in ax.cells:
            ok = oky & okx
            if not ok.any():
                continue
            for i in range(4):
                for j in range(4):
                    with np.errstate(invalid="ignore"):
                        m = np.where(ok, famy["A"][i] * famx["A"][j], 0.0)[..., None] * absA
                        s = np.where(ok, du * famy["aw"][i] * famx["adw"][j] + dv * famy["adw"][i] * famx["aw"][j]
                                     + K2 * 0.5 * (du + dv) ** 2, 0.0)[..., None] * absA
                    np.add.at(r.g_image_round, (b, ry[i], cx[j]), m)
                    np.add.at(r.g_image_coord, (b, ry[i], cx[j]), s)
                    np.add.at(count, (b, ry[i], cx[j]), np.broadcast_to(ok[..., None], a.shape).astype(np.float64))
    r.g_image_terms = count
    return r


def make_inputs(B, H, W, C, Ho, Wo, coord_batch, gain_shape, seed, span=1.1, signed=False):
    """Seeded inputs as float64 arrays of float32 values: image, gain and g_out uniform in (0, 1) (with seeded signs when
    `signed`), coordinates uniform in (-span, span) with none within 1e-3 of +-1 (the coordinate gradient jumps there)."""
    rng = np.random.default_rng(seed)
    f32 = lambda v: v.astype(np.float32).astype(np.float64)                        # noqa: E731
    sign = lambda shape: (2.0 * rng.integers(0, 2, shape) - 1.0) if signed else 1.0  # noqa: E731
    image = f32(rng.uniform(0.05, 1, (B, H, W, C)) * sign((B, H, W, C)))
    xy = rng.uniform(-span, span, (2, coord_batch, Ho, Wo))
    edge = np.abs(np.abs(xy) - 1) < 1e-3
    xy = f32(np.where(edge, xy * 0.99, xy))
    assert not (np.abs(np.abs(xy) - 1) < 1e-3).any()
    gain = None if gain_shape is None else f32(rng.uniform(0.05, 1, gain_shape) * sign(gain_shape))
    g_out = f32(rng.uniform(0.05, 1, (B, Ho, Wo, C)) * sign((B, Ho, Wo, C)))
    return image, xy[0], xy[1], gain, g_out
