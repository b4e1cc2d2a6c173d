"""Encircled / ensquared energy (metrics.enclosed_energy / spot_centroid; tl_enclosed_centroid / tl_enclosed_sums /
tl_enclosed_seed of include/tl_trace.h) restated in float64 numpy from the definition, with the bounds the kernels are held to.
It shares no code with the package.

DEFINITION.  A row is one (lens, field, wavelength); a ray is live iff ok != 0.  S = (n, sum x, sum y) over the live rays.  The
centre c of a row is S[1:3] / n ("row"; 0 for n = 0), the same from S summed over the wavelengths ("field"), or given.  With
dx = x - c_x, dy = y - c_y, sigma(u) = t^2 (3 - 2 t), t = clip((u + 1) / 2, 0, 1), sigma'(u) = 3 t (1 - t):
  circle  e_ik = sigma((R_k - rho_i) / tau_k), rho = sqrt(dx^2 + dy^2)       square  e_ik = sigma((R_k - |dx|) / tau_k) sigma((R_k - |dy|) / tau_k)
  sums[row, k] = sum over live rays of e_ik.

BOUNDS (U = 2^-53; derived here, never fitted to a kernel's output).  The inputs are fp32, exact in fp64.
  S        |S_j - ref| <= (P + 8) U sum|terms|: both sides add the same P exact terms in different orders; any order of n
           additions is within (n - 1) U sum|term| of the exact sum to first order.  n itself is an integer below 2^53: exact.
  centre   an internal centroid is a quotient of such sums: |dc| <= (N + 8) U sum|x| / n + U |c|, N = P ("row") or P W
           ("field": W rows of P terms and W - 1 more additions).  A given centre is exact: dc = 0.
  u        dx carries one rounding (U |dx|) and dc; rho = sqrt(dx^2 + dy^2) five more roundings of which the root halves
           three: |d rho| <= 3 U rho + dc_x + dc_y.  R - rho rounds once, the product with 1 / tau once, 1 / tau itself once, and
           the definition's quotient once: 4 U |u|, |u| <= (R + rho) / tau.  So
               |du| <= A := 7 U (R_k + rho_i) / tau_k + (dc_x + dc_y) / tau_k                 (the amplification (R + rho) / tau)
           and for the square the same with |dx| (or |dy|) for rho and dc_x (dc_y) alone.
  e        t = (u + 1) / 2: |dt| <= A / 2 + U.  |d sigma / dt| = 6 t (1 - t) <= 3 / 2, and the four roundings of t t (3 - 2 t)
           are 4 U of a value <= 1:  |de| <= 3/4 A + 6 U  -- for a ray IN THE BAND, |u| <= 1 + 2 A.  Outside it both sides clamp
           t to exactly 0 or 1 and the term is exactly 0 or 1: de = 0.  Square: e = s_x s_y with both <= 1, so
           |de| <= ds_x + ds_y + U.
  sums     |sums_k - ref| <= (P + 8) U sum_i |e_ik| + sum_i de_ik.
  seeds    per ray, d_i = sum_k g_k d e_ik / dx_i.  |d sigma' / du| = 3/2 |1 - 2 t| <= 3/2, so in the band
           |d sigma'| <= 3/2 A + 4 U sigma'.  Circle: d_i = -s dx / rho with s = sum_k g_k sigma'_k / tau_k:
               |ds| <= sum_k |g_k| / tau_k (3/2 A_k [band]) + (K + 8) U sum_k |g_k| sigma'_k / tau_k,
           and the direction dx / rho moves by at most min(1, 2 (dc_x + dc_y) / rho) + 6 U (all of it, 1, at rho = 0 when the
           centre is not exact).  Square: d_i = -sgn(dx) sum_k g_k sigma'(u_x) sigma(u_y) / tau_k, each factor bounded as above;
           where |dx| <= dc_x the sign itself is open: 2 |d_i| more.  The ray's gradient is d_i + l, l the seed of sum x (plus,
           through an internal centroid, the centre's gradient over n), rounded once to fp32:
               |g - ref| <= 2^-24 |ref| + 16 U (|d_i| + |l|) + dd_i + dl + 2^-149.
  centre   g_c = -sum over live rays of d_i: |g_c - ref| <= (P + 8) U sum |d_i| + sum dd_i; pooled over a field's rows for
           centre = "field" (N = P W), divided by n and added to the seed of sum x: dl = dg_c / n + 4 U (|g_S| + |g_c| / n).
"""
import numpy as np

import rows_ref
from rows_ref import BLOCK, CHUNK, MAX_Y, TARGET_BLOCKS, VEC, launches, plan        # noqa: F401 (the tests read them from here)

U = 2.0 ** -53
MAX_K = 32


def sigma(u):
    t = np.clip(0.5 * (u + 1.0), 0.0, 1.0)
    return t * t * (3.0 - 2.0 * t)


def dsigma(u):
    t = np.clip(0.5 * (u + 1.0), 0.0, 1.0)
    return 3.0 * t * (1.0 - t)


def _live_xy(x, y, ok):
    x, y, ok = np.broadcast_arrays(x, y, ok)
    live = ok != 0
    return np.where(live, np.asarray(x, np.float64), 0.0), np.where(live, np.asarray(y, np.float64), 0.0), live


def spot_sums(x, y, ok):
    """(S, T): S [B,F,W,3] = (n, sum x, sum y) over the live rays of [B,F,P,W] arrays, T the sums of the terms' magnitudes."""
    x, y, live = _live_xy(x, y, ok)
    n = live.sum(axis=2).astype(np.float64)
    return np.stack([n, x.sum(axis=2), y.sum(axis=2)], axis=-1), np.stack([n, np.abs(x).sum(axis=2), np.abs(y).sum(axis=2)], axis=-1)


def spot_bound(T, P):
    return (P + 8) * U * T


def centre_of(S, T, centre, P):
    """(c, dc), both [B,F,W,2]: the centre of every row and the bound of its error.  centre: "row", "field" or an array."""
    if not isinstance(centre, str):
        c = np.broadcast_to(np.asarray(centre, np.float64), S.shape[:3] + (2,))
        return c, np.zeros_like(c)
    terms = P
    if centre == "field":
        terms = P * S.shape[2]
        S, T = (np.broadcast_to(a.sum(axis=2, keepdims=True), a.shape) for a in (S, T))
    n1 = np.maximum(S[..., :1], 1.0)
    c = S[..., 1:3] / n1
    return c, (terms + 8) * U * T[..., 1:3] / n1 + U * np.abs(c)


class Terms:
    """Everything per ray and radius, [B,F,P,W,K]: e and its bound de, the gradients' factors and their bounds."""

    def __init__(self, x, y, ok, c, dc, radii, soft, shape):
        x, y, live = _live_xy(x, y, ok)
        self.live = live
        K = len(radii)
        R = np.asarray(radii, np.float64).reshape(1, 1, 1, 1, K)
        tau = np.broadcast_to(np.asarray(soft, np.float64), (K,)).reshape(1, 1, 1, 1, K)
        dx, dy = x - c[:, :, None, :, 0], y - c[:, :, None, :, 1]
        dcx, dcy = dc[:, :, None, :, 0, None], dc[:, :, None, :, 1, None]
        lv = live[..., None]
        self.dx, self.dy, self.dc, self.tau, self.K = dx, dy, (dcx, dcy), tau, K
        if shape == "circle":
            rho = np.sqrt(dx * dx + dy * dy)
            u = (R - rho[..., None]) / tau
            A = 7 * U * (R + rho[..., None]) / tau + (dcx + dcy) / tau
            band = np.abs(u) <= 1 + 2 * A
            self.rho = rho
            self.e = np.where(lv, sigma(u), 0.0)
            self.de = np.where(lv & band, 0.75 * A + 6 * U, 0.0)
            self.w = np.where(lv, dsigma(u) / tau, 0.0)                                   # sigma' / tau
            self.dw = np.where(lv & band, 1.5 * A / tau, 0.0) + 4 * U * self.w
        elif shape == "square":
            ax, ay = np.abs(dx)[..., None], np.abs(dy)[..., None]
            ux, uy = (R - ax) / tau, (R - ay) / tau
            Ax, Ay = 7 * U * (R + ax) / tau + dcx / tau, 7 * U * (R + ay) / tau + dcy / tau
            bx, by = np.abs(ux) <= 1 + 2 * Ax, np.abs(uy) <= 1 + 2 * Ay
            sx, sy, px, py = sigma(ux), sigma(uy), dsigma(ux), dsigma(uy)
            dsx, dsy = np.where(bx, 0.75 * Ax + 6 * U, 0.0), np.where(by, 0.75 * Ay + 6 * U, 0.0)
            dpx, dpy = np.where(bx, 1.5 * Ax, 0.0) + 4 * U * px, np.where(by, 1.5 * Ay, 0.0) + 4 * U * py
            self.e = np.where(lv, sx * sy, 0.0)
            self.de = np.where(lv, dsx + dsy + U, 0.0)
            self.wx, self.wy = np.where(lv, px * sy / tau, 0.0), np.where(lv, sx * py / tau, 0.0)
            self.dwx = np.where(lv, (dpx * sy + px * dsy) / tau, 0.0) + 4 * U * self.wx
            self.dwy = np.where(lv, (dsx * py + sx * dpy) / tau, 0.0) + 4 * U * self.wy
        else:
            raise ValueError(shape)
        self.shape = shape

    def ray_gradients(self, g_sums):
        """The edge part d = sum_k g_k d e_k / d(x, y) of every ray's gradient: ((d_x, d_y), (dd_x, dd_y)), each [B,F,P,W]."""
        g = np.asarray(g_sums, np.float64)[:, :, None, :, :]
        dcx, dcy = (a[..., 0] for a in self.dc)
        out, err = [], []
        if self.shape == "circle":
            s, mag = (g * self.w).sum(axis=-1), (np.abs(g) * self.w).sum(axis=-1)
            ds = (np.abs(g) * (self.dw - 4 * U * self.w)).sum(axis=-1) + (self.K + 8) * U * mag
            some = self.rho > 0
            rho1 = np.where(some, self.rho, 1.0)
            turn = np.where(some, np.minimum(1.0, 2 * (dcx + dcy) / rho1), np.where(dcx + dcy > 0, 1.0, 0.0)) + 6 * U
            for d in (self.dx, self.dy):
                direction = np.where(some, d / rho1, 0.0)
                out.append(-s * direction)
                err.append(ds * np.abs(direction) + np.abs(s) * turn)
        else:
            for d, w, dw, dcq in ((self.dx, self.wx, self.dwx, dcx), (self.dy, self.wy, self.dwy, dcy)):
                s = (g * w).sum(axis=-1)
                ds = (np.abs(g) * dw).sum(axis=-1) + (self.K + 8) * U * (np.abs(g) * w).sum(axis=-1)
                out.append(-s * np.sign(d))
                err.append(ds + np.where(np.abs(d) <= dcq, 2 * np.abs(s) + ds, 0.0))
        return tuple(np.where(self.live, a, 0.0) for a in out), tuple(np.where(self.live, a, 0.0) for a in err)


def enclosed_sums(x, y, ok, radii, soft, shape, centre):
    """dict: S, sums [B,F,W,K], centre, n and the bounds S_bound, sums_bound, of arrays [B,F,P,W]."""
    P = np.broadcast_arrays(x, y, ok)[0].shape[2]
    S, T = spot_sums(x, y, ok)
    c, dc = centre_of(S, T, centre, P)
    t = Terms(x, y, ok, c, dc, radii, soft, shape)
    return dict(S=S, S_bound=spot_bound(T, P), centre=c, sums=t.e.sum(axis=2),
                sums_bound=(P + 8) * U * np.abs(t.e).sum(axis=2) + t.de.sum(axis=2), terms=t, P=P)


def energy(S, sums, common=("wavelength",)):
    """(n, energy [..., K]): sums and n pooled over the dimensions in `common`, then divided."""
    n = S[..., 0]
    axes = tuple(d for d, name in ((1, "field"), (2, "wavelength")) if name in common)
    if axes:
        n, sums = n.sum(axis=axes), sums.sum(axis=axes)
    return n, sums / np.maximum(n, 1.0)[..., None]


def enclosed_radius(E, radii, fraction):
    """(radius, reached) on the piecewise-linear curve through (0, 0), (R_k, E_k): plain loops."""
    E = np.asarray(E, np.float64)
    flat = E.reshape(-1, E.shape[-1])
    out, reached = np.full(len(flat), float(radii[-1])), np.zeros(len(flat), bool)
    for i, row in enumerate(flat):
        lo_r, lo_e = 0.0, 0.0
        for r, e in zip(radii, row):
            if e >= fraction:
                out[i], reached[i] = (lo_r + (fraction - lo_e) / (e - lo_e) * (r - lo_r) if e > lo_e else lo_r), True
                break
            lo_r, lo_e = r, e
    return out.reshape(E.shape[:-1]), reached.reshape(E.shape[:-1])


def seeds(ref, g_sums, g_S, centre):
    """d(sum g_sums . sums + sum g_S . S) / d(x, y, centre) of the evaluation `ref` (enclosed_sums'): dict gx, gy [B,F,P,W] and
    gc [B,F,W,2] (the centre's gradient: what a GIVEN centre receives) with their bounds gx_bound, gy_bound, gc_bound."""
    t, S, P = ref["terms"], ref["S"], ref["P"]
    g_S = np.asarray(g_S, np.float64)
    (d_x, d_y), (dd_x, dd_y) = t.ray_gradients(g_sums)
    gc = -np.stack([d_x.sum(axis=2), d_y.sum(axis=2)], axis=-1)
    mag = np.stack([np.abs(d_x).sum(axis=2), np.abs(d_y).sum(axis=2)], axis=-1)
    dgc = (P + 8) * U * mag + np.stack([dd_x.sum(axis=2), dd_y.sum(axis=2)], axis=-1)
    lin, dlin = g_S[..., 1:3], 0.0
    if isinstance(centre, str):
        n, pooled, dpooled, pmag = S[..., :1], gc, dgc, mag
        if centre == "field":
            W = S.shape[2]
            n, pooled, dpooled, pmag = (np.broadcast_to(a.sum(axis=2, keepdims=True), a.shape) for a in (n, gc, dgc, mag))
            dpooled = dpooled + (W + 8) * U * pmag
        n1 = np.maximum(n, 1.0)
        lin = g_S[..., 1:3] + pooled / n1
        dlin = dpooled / n1 + 4 * U * (np.abs(g_S[..., 1:3]) + np.abs(pooled) / n1)
    out = dict(gc=gc, gc_bound=dgc)
    for k, j, d, dd in (("gx", 0, d_x, dd_x), ("gy", 1, d_y, dd_y)):
        l = np.broadcast_to((lin[..., j])[:, :, None, :], d.shape)
        dl = np.broadcast_to((dlin[..., j])[:, :, None, :], d.shape) if isinstance(centre, str) else 0.0
        g = np.where(t.live, d + l, 0.0)
        out[k] = g
        out[k + "_bound"] = np.where(t.live, 2.0 ** -24 * np.abs(g) + 16 * U * (np.abs(d) + np.abs(l)) + dd + dl, 0.0) + 2.0 ** -149
    return out


# --------------------------------------------------------------------------------- other evaluations of the same definition
def sums_in_order(x, y, ok, radii, soft, shape, c, order, inner=np.float64):
    """sums [B,F,W,K] about the centre c [B,F,W,2] with the rays of a row added one by one in float64 in the given order
    ("forward", "reverse", or "blocks": rays j, j + 256, ... of every j in turn), every term evaluated in the arithmetic
    `inner` (np.float32: what an fp32 inner loop would give -- centre, differences, root, edge in fp32)."""
    x, y, ok = np.broadcast_arrays(x, y, ok)
    live = ok != 0
    f = inner
    R, tau = np.asarray(radii, f), np.broadcast_to(np.asarray(soft, f), (len(radii),)).astype(f)
    xs, ys = np.where(live, x, 0).astype(f), np.where(live, y, 0).astype(f)
    dx, dy = xs - c[:, :, None, :, 0].astype(f), ys - c[:, :, None, :, 1].astype(f)
    one, half, two, three = f(1), f(0.5), f(2), f(3)

    def sig(a):
        t = np.clip(half * ((R - a[..., None]) * (one / tau) + one), f(0), one)
        return t * t * (three - two * t)
    e = sig(np.sqrt(dx * dx + dy * dy)) if shape == "circle" else sig(np.abs(dx)) * sig(np.abs(dy))
    assert e.dtype == f
    e = np.where(live[..., None], e, 0).astype(np.float64)
    P = e.shape[2]
    idx = {"forward": np.arange(P), "reverse": np.arange(P)[::-1],
           "blocks": np.concatenate([np.arange(P)[j::BLOCK] for j in range(BLOCK)])}[order]
    acc = np.zeros(e.shape[:2] + e.shape[3:])
    for i in idx:
        acc = acc + e[:, :, i]
    return acc


# ---------------------------------------------------------------------------------------------------------------- the plan
def workspace_bytes(F, P, W, K):
    return rows_ref.workspace_bytes(F, P, W, max(K, 3)) if 1 <= K <= MAX_K else 0
