"""An independent float64 evaluation of the fused PSF soft histogram and its adjoint in numpy, written from the definition at the
top of csrc/tl_psf.hip (it imports nothing from torchoptics_amd), with all five gradients of sum(T * hist) and, next to each
result, the sums that the error bounds of tests/psf_cases.py need.

    hist[g,w,i,j] = sum_r wt_r Gy_i(r) Gx_j(r),   Gx_j = exp(-2 dx_j^2),  dx_j = x / x_pitch[g] - (x_first + j)
                                                  Gy_i = exp(-2 dy_i^2),  dy_i = (y - y_centre[g]) / y_pitch[g] - (y_first + i)
    gx_r = wt_r / x_pitch[g] sum_ij T_ij Gy_i Gx'_j,   gy_r = wt_r / y_pitch[g] sum_ij T_ij Gy'_i Gx_j,   G' = -4 d G
    g_x_pitch[g] = -sum_wr gx_r x_r / x_pitch[g],  g_y_pitch[g] = -sum_wr gy_r (y_r - y_centre[g]) / y_pitch[g],
    g_y_centre[g] = -sum_wr gy_r

The inputs are float64 arrays that hold float32 values; x_first + j and y_first + i must be exact in float32 (multiples of 1/2).

Error terms (U = 2^-24, TINY = 2^-126; psf_cases.py derives them).  A float32 evaluation knows a distance d to a pixel centre to
    dd = 2 U |d| + 3 U^2 |c|  (+ U |c| along y),          c = the coordinate in pitch units,
and a Gaussian to the relative error  rel = U (2 + 6 d^2) + 4 |d| dd.  Returned next to each result:
    hist_mag  = sum_r |wt| Gy Gx                       what the roundings of the products and sums are relative to
    hist_fac  = sum_r |wt| Gy Gx (rel_y + rel_x)       the error of the two factors
    hist_floor, gx_floor, gy_floor                     what flushing below the smallest normal can cost
    gx_mag    = |wt| / x_pitch sum_ij |T_ij| Gy_i |Gx'_j|,   gx_fac = the same with (rel_y_i + rel_x_j) and 4 Gx_j dd_j for |Gx'_j|
    gy_mag, gy_fac likewise.

`variant` evaluates a deliberately WRONG definition, for the tests that hold the bounds to be sharp:
    'drop-last'    the last ray of every channel is left out          'tail-twice'  ray `arg` is counted twice
    'pitch-w'      x_pitch[w mod G] in place of x_pitch[g]            'rows+4'      rows i and i + 4 of the tile are exchanged
    'block-missing' the rays [arg[0], arg[1]) are missing from hist   'pad-col'     the backward sees a column nxh that holds
    'y-first-sign' y_first has the other sign                                       the values of column nxh - 1
    'wt-squared'   the weight is applied squared"""
import math
from types import SimpleNamespace

import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126
VARIANTS = ("drop-last", "tail-twice", "pitch-w", "rows+4", "block-missing", "pad-col", "y-first-sign", "wt-squared")


def _axis(c, first, n, along_y):
    """c [W,R]: a coordinate in pitch units -> d, G, dd, rel [W,R,n] of the n pixel centres first + k."""
    d = c[..., None] - (first + np.arange(n, dtype=np.float64))
    G = np.exp(-2.0 * d * d)
    a = np.abs(c)[..., None]
    dd = 2 * U * np.abs(d) + 3 * U * U * a + (U * a if along_y else 0.0)
    rel = U * (2 + 6 * d * d) + 4 * np.abs(d) * dd
    return d, G, dd, rel


def row_swap(ny):
    """The permutation that exchanges rows i and i + 4 (i with bit 2 clear, where i + 4 exists)."""
    p = np.arange(ny)
    for i in range(ny):
        if not (i & 4) and i + 4 < ny:
            p[i], p[i + 4] = i + 4, i
    return p


def evaluate(x, y, wt, x_pitch, y_pitch, y_centre, nxh, ny, x_first, y_first, T, variant=None, arg=None, magnitudes=True):
    """x, y [G,W,R], wt [G,W,R] or None, x_pitch, y_pitch, y_centre [G], T [G,W,ny,nxh]: float64 arrays of float32 values.
    Returns a namespace of hist, gx, gy, g_x_pitch, g_y_pitch, g_y_centre and (when `magnitudes`) the sums of the module
    docstring."""
    assert variant is None or variant in VARIANTS, variant
    magnitudes = magnitudes and variant is None
    x, y, T = (np.asarray(v, dtype=np.float64) for v in (x, y, T))
    px, py, yc = (np.asarray(v, dtype=np.float64) for v in (x_pitch, y_pitch, y_centre))
    G, W, R = x.shape
    wt = np.ones(x.shape) if wt is None else np.array(wt, dtype=np.float64)
    assert T.shape == (G, W, ny, nxh) and wt.shape == x.shape and px.shape == py.shape == yc.shape == (G,)
    if variant == "drop-last":
        wt[..., R - 1] = 0.0
    elif variant == "tail-twice":
        wt[..., arg] *= 2.0
    elif variant == "wt-squared":
        wt = wt * wt
    elif variant == "y-first-sign":
        y_first = -y_first
    wt_hist = wt
    if variant == "block-missing":
        wt_hist = wt.copy()
        wt_hist[..., arg[0]:arg[1]] = 0.0
    nxb = nxh
    if variant == "pad-col":
        T, nxb = np.concatenate((T, T[..., -1:]), axis=-1), nxh + 1
    perm = row_swap(ny) if variant == "rows+4" else np.arange(ny)
    T = T[:, :, perm, :]

    r = SimpleNamespace(hist=np.zeros((G, W, ny, nxh)), gx=np.zeros(x.shape), gy=np.zeros(x.shape), g_x_pitch=np.zeros(G),
                        g_y_pitch=np.zeros(G), g_y_centre=np.zeros(G))
    names = ("hist_mag", "hist_fac", "hist_floor", "gx_mag", "gx_fac", "gx_floor", "gy_mag", "gy_fac", "gy_floor")
    if magnitudes:
        for n in names:
            setattr(r, n, np.zeros(r.hist.shape if n.startswith("hist") else x.shape))
    tr = lambda a: a.transpose(0, 2, 1)                                              # noqa: E731
    for g in range(G):
        pxw = px[np.arange(W) % G][:, None] if variant == "pitch-w" else np.full((W, 1), px[g])
        u, v = x[g] / pxw, (y[g] - yc[g]) / py[g]
        dx, Gx, ddx, relx = _axis(u, x_first, nxb, False)
        dy, Gy, ddy, rely = _axis(v, y_first, ny, True)
        Gxd, Gyd = -4 * dx * Gx, -4 * dy * Gy
        w, wh = wt[g], wt_hist[g]
        r.hist[g] = np.matmul(tr(wh[..., None] * Gy), Gx[..., :nxh])[:, perm, :]
        Tg = T[g]
        r.gx[g] = w / pxw * (np.matmul(Gy, Tg) * Gxd).sum(-1)
        r.gy[g] = w / py[g] * (np.matmul(Gyd, Tg) * Gx).sum(-1)
        r.g_x_pitch[g] = -(r.gx[g] * x[g] / pxw).sum()
        r.g_y_pitch[g] = -(r.gy[g] * (y[g] - yc[g])).sum() / py[g]
        r.g_y_centre[g] = -r.gy[g].sum()
        if not magnitudes:
            continue
        aw = np.abs(w)
        A = aw[..., None] * Gy
        r.hist_mag[g] = np.matmul(tr(A), Gx)
        r.hist_fac[g] = np.matmul(tr(A * rely), Gx) + np.matmul(tr(A), Gx * relx)
        r.hist_floor[g] = TINY * (3 * aw.sum(-1) + 2 * (w != 0).sum(-1) + 2)[:, None, None]
        M = np.abs(Tg)
        Pm, Pr = np.matmul(Gy, M), np.matmul(Gy * rely, M)
        aGxd, aGyd = np.abs(Gxd), np.abs(Gyd)
        r.gx_mag[g] = aw / pxw * (Pm * aGxd).sum(-1)
        r.gx_fac[g] = aw / pxw * (Pr * aGxd + Pm * (aGxd * relx + 4 * Gx * ddx)).sum(-1)
        Pdm, Pdr = np.matmul(aGyd, M), np.matmul(aGyd * rely + 4 * Gy * ddy, M)
        r.gy_mag[g] = aw / py[g] * (Pdm * Gx).sum(-1)
        r.gy_fac[g] = aw / py[g] * (Pdr * Gx + Pdm * Gx * relx).sum(-1)
        nxp = (nxh + 3) & ~3
        col, row = M.sum(1)[:, None, :], M.sum(2)[:, None, :]                        # [W,1,nxh], [W,1,ny]
        r.gx_floor[g] = TINY * (1 + aw / pxw * (ny * nxp + ny + 2 * (col * (2 + 4 * np.abs(dx))).sum(-1)))
        r.gy_floor[g] = TINY * (1 + aw / py[g] * (ny * nxp + ny + 2 * (row * (2 + 4 * np.abs(dy))).sum(-1)))
    return r


def grid_sums(gx32, gy32, x, y, x_pitch, y_pitch, y_centre):
    """The three per-grid gradients as float64 sums of float32 per-ray gradients (gx32, gy32 [G,W,R], any float dtype holding
    float32 values), and the tolerance of one float32 rounding of a float64 sum of n terms taken in any order:
    ({name: S [G]}, {name: U |S| + n 2^-53 sum |terms|}).  (y - y_centre) is the float32 difference the kernel forms; a product
    of two float32 numbers is exact in float64 and math.fsum adds exactly, so S itself carries the one rounding of its divide
    (the kernel's order of adding costs at most (n - 1) 2^-53 sum |terms|, its divide the rest)."""
    gx, gy, x = (np.asarray(v, dtype=np.float64) for v in (gx32, gy32, x))
    px, py = (np.asarray(v, dtype=np.float64) for v in (x_pitch, y_pitch))
    yc32 = (np.asarray(y, dtype=np.float32) - np.asarray(y_centre, dtype=np.float32)[:, None, None]).astype(np.float64)
    G, n = gx.shape[0], gx.shape[1] * gx.shape[2]
    terms = {"g_x_pitch": (gx * x, px), "g_y_pitch": (gy * yc32, py), "g_y_centre": (gy, np.ones(G))}
    S = {k: np.array([-math.fsum(t[g].ravel()) / div[g] for g in range(G)]) for k, (t, div) in terms.items()}
    tol = {k: U * np.abs(S[k]) + n * 2.0 ** -53 * np.abs(t).sum(axis=(1, 2)) / div for k, (t, div) in terms.items()}
    return S, tol
