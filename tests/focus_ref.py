"""The through-focus spot moments (metrics.focus_moments / through_focus; tl_focus_moments / tl_focus_seed of
include/tl_trace.h) restated in float64 numpy from the definition, with the bounds the kernels are held to and a CPU
emulation of the kernels' summation order.  It shares no code with the package.

DEFINITION.  A row is one (lens, field, wavelength).  A ray is live iff ok != 0 and s = 1 - cx^2 - cy^2 > 0; then cz = sqrt(s),
u = cx / cz, v = cy / cz, and M[row, 0..10] = sum over live rays of (1, x, y, u, v, x^2, y^2, u^2, v^2, x u, y v).

BOUNDS (U = 2^-53, derived, not measured).
  moments   |M_k - ref| <= (n_terms + 8) U sum_r |term_r|.   Both sides add the same fp64 terms (the kernels contract nothing,
            so a term has the same bits in any IEEE arithmetic, to the one or two roundings of sqrt and the quotient that a
            library may place differently: the 8), in different orders; any order of n additions is within (n - 1) U sum|term|
            of the exact sum to first order, and two orders differ by at most twice that less what they share.  n_terms = P.
  seeds     |g - ref| <= 2^-24 |ref| + 16 U sum|its terms| + 2^-149: one rounding to fp32 (or to its smallest subnormal) of
            an fp64 value made of at most five terms, each from at most six fp64 operations.
"""
import numpy as np

import rows_ref
from rows_ref import BLOCK, CHUNK, MAX_Y, TARGET_BLOCKS, VEC, launches, plan        # noqa: F401 (the tests read them from here)

U = 2.0 ** -53
NMOM = 11


def live_rays(cx, cy, ok):
    with np.errstate(invalid="ignore", over="ignore"):
        s = 1.0 - np.asarray(cx, np.float64) ** 2 - np.asarray(cy, np.float64) ** 2
        return (np.asarray(ok) != 0) & (s > 0)


def ray_terms(x, y, cx, cy, ok, wrong=None):
    """[..., 11] float64: the eleven terms of every ray (zeros for a dead one)."""
    x, y, cx, cy = (np.asarray(a, np.float64) for a in np.broadcast_arrays(x, y, cx, cy))
    live = np.broadcast_to(live_rays(cx, cy, ok), x.shape)
    if wrong == "dead":                                       # a dead ray counted (the first dead ray with finite coordinates)
        with np.errstate(invalid="ignore", over="ignore"):
            cand = np.flatnonzero(~live.ravel() & np.isfinite(x + y).ravel() & ((1 - cx * cx - cy * cy) > 0).ravel())
        live = live.copy()
        live.ravel()[cand[0]] = True
    x, y, cx, cy = (np.where(live, a, 0.0) for a in (x, y, cx, cy))
    cz = np.sqrt(1.0 - cx * cx - cy * cy)
    u, v = (cx, cy) if wrong == "cx_for_u" else (cx / cz, cy / cz)
    t = np.stack([live.astype(np.float64), x, y, u, v, x * x, y * y, u * u, v * v, (y if wrong == "swap9" else x) * u, y * v], axis=-1)
    if wrong in ("drop", "twice"):
        first = np.flatnonzero(live.ravel())[live.sum() // 2]
        t.reshape(-1, NMOM)[first] *= 0.0 if wrong == "drop" else 2.0
    return t


def moments(x, y, cx, cy, ok):
    """(M, T): M [B,F,W,11] the moments of rays [B,F,P,W], T the sums of the terms' magnitudes (what the bound scales with)."""
    t = ray_terms(x, y, cx, cy, ok)
    return t.sum(axis=2), np.abs(t).sum(axis=2)


def moment_bound(T, n_terms):
    return (n_terms + 8) * U * T


def seeds(x, y, cx, cy, ok, g):
    """d(sum g . M) / d(x, y, cx, cy) per ray in float64 and the magnitude sums of their terms: two tuples of four [B,F,P,W]
    arrays.  g: [B,F,W,11]."""
    x, y, cx, cy = (np.asarray(a, np.float64) for a in np.broadcast_arrays(x, y, cx, cy))
    live = np.broadcast_to(live_rays(cx, cy, ok), x.shape)
    x, y, cx, cy = (np.where(live, a, 0.0) for a in (x, y, cx, cy))
    g = [np.asarray(g, np.float64)[:, :, None, :, k] for k in range(NMOM)]
    cz = np.sqrt(1.0 - cx * cx - cy * cy)
    u, v = cx / cz, cy / cz
    gx, mx = g[1] + 2 * x * g[5] + u * g[9], abs(g[1]) + abs(2 * x * g[5]) + abs(u * g[9])
    gy, my = g[2] + 2 * y * g[6] + v * g[10], abs(g[2]) + abs(2 * y * g[6]) + abs(v * g[10])
    gu, mu = g[3] + 2 * u * g[7] + x * g[9], abs(g[3]) + abs(2 * u * g[7]) + abs(x * g[9])
    gv, mv = g[4] + 2 * v * g[8] + y * g[10], abs(g[4]) + abs(2 * v * g[8]) + abs(y * g[10])
    cz3 = cz ** 3
    gcx, mcx = (gu * (1 - cy * cy) + gv * cx * cy) / cz3, (mu * (1 - cy * cy) + mv * abs(cx * cy)) / cz3
    gcy, mcy = (gu * cx * cy + gv * (1 - cx * cx)) / cz3, (mu * abs(cx * cy) + mv * (1 - cx * cx)) / cz3
    zero = lambda a: np.where(live, a, 0.0)                                       # noqa: E731
    return tuple(map(zero, (gx, gy, gcx, gcy))), tuple(map(zero, (mx, my, mcx, mcy)))


def seed_bound(ref, mag):
    return 2.0 ** -24 * np.abs(ref) + 16 * U * mag + 2.0 ** -149


# ---------------------------------------------------------------------------------------------------------------- the finish
def _root(v):
    return np.sqrt(np.where(v > 0, v, 0.0))


def _quotient(num, den, raw):
    good = den > 2.0 ** -40 * raw
    return np.where(good, num / np.where(good, den, 1.0), 0.0)


def centred(M):
    """n, (Ax, Bx, Cx), (Ay, By, Cy) of every row of M [..., 11]."""
    n = M[..., 0]
    n1 = np.maximum(n, 1.0)
    one = lambda q, s, qq, ss, qs: (M[..., qq] - M[..., q] ** 2 / n1, M[..., qs] - M[..., q] * M[..., s] / n1,   # noqa: E731
                                    M[..., ss] - M[..., s] ** 2 / n1)
    return n, one(1, 3, 5, 7, 9), one(2, 4, 6, 8, 10)


def finish(M, common=("wavelength",), centroid="row"):
    """dict of n, rms, best_focus, rms_best, focus_t, focus_s, a, b, c from M [B,F,W,11]."""
    M = np.asarray(M, np.float64)
    if centroid == "field":
        M = M.sum(axis=2, keepdims=True)
    n, (Ax, Bx, Cx), (Ay, By, Cy) = centred(M)
    q = [n, Ax, Ay, Bx, By, Cx, Cy, M[..., 7], M[..., 8]]
    axes = tuple(d for d, name in ((1, "field"), (2, "wavelength")) if name in common)
    if axes:
        q = [a.sum(axis=axes) for a in q]
    n, Ax, Ay, Bx, By, Cx, Cy, rx, ry = q
    A, B, C, n1 = Ax + Ay, Bx + By, Cx + Cy, np.maximum(n, 1.0)
    r = _quotient(B, C, rx + ry)
    return dict(n=n, rms=_root(A / n1), best_focus=-r, rms_best=_root((A - B * r) / n1), focus_t=-_quotient(By, Cy, ry),
                focus_s=-_quotient(Bx, Cx, rx), a=A / n1, b=B / n1, c=C / n1)


def through_focus(x, y, cx, cy, ok, common=("wavelength",), centroid="row"):
    return finish(moments(x, y, cx, cy, ok)[0], common, centroid)


def rms_shifted(x, y, cx, cy, ok, delta, common=("wavelength",), centroid="row"):
    """Brute force: the live-ray RMS radius of the rays moved to the plane at `delta` ([B,F,W] less the pooled dimensions,
    broadcastable against them kept as size 1), every row about its own centroid (or its field's), pooled over `common`."""
    x, y, cx, cy = (np.asarray(a, np.float64) for a in np.broadcast_arrays(x, y, cx, cy))
    live = np.broadcast_to(live_rays(cx, cy, ok), x.shape)
    cxl, cyl = np.where(live, cx, 0.0), np.where(live, cy, 0.0)
    cz = np.sqrt(1 - cxl ** 2 - cyl ** 2)
    d = np.asarray(delta, np.float64)
    if d.ndim == 0:
        d = d.reshape(1, 1, 1)
    else:                                                               # bring delta to [B, F|1, 1, W|1]
        for ax in (1, 2):
            if ((ax == 1 and "field" in common) or (ax == 2 and "wavelength" in common)):
                d = np.expand_dims(d, ax)
    d = d[:, :, None, :]
    xs, ys = np.where(live, x + d * cxl / cz, 0.0), np.where(live, y + d * cyl / cz, 0.0)
    cen = (2, 3) if centroid == "field" else (2,)
    cnt = np.maximum(live.sum(axis=cen, keepdims=True), 1)
    r2 = np.where(live, (xs - xs.sum(axis=cen, keepdims=True) / cnt) ** 2 + (ys - ys.sum(axis=cen, keepdims=True) / cnt) ** 2, 0.0)
    pool = (2,) + tuple(a for a, name in ((1, "field"), (3, "wavelength")) if name in common)
    return np.sqrt(r2.sum(axis=pool) / np.maximum(live.sum(axis=pool), 1))


# ---------------------------------------------------------------------------------------------------- the kernels, emulated
def workspace_bytes(F, P, W):
    return rows_ref.workspace_bytes(F, P, W, NMOM)


def emulate_moments(x, y, cx, cy, ok, aligned, wrong=None, batch=2048):
    """M [B,F,W,11] with the kernels' arithmetic: fp64 terms, per lane in the order of its loop (four consecutive rays per step
    of 1024 where aligned[row], else one per step of 256), the butterfly over the 64 lanes of a wave, the four waves in order,
    the row's partials in order.  x .. ok: [B,F,P,W]; aligned: [B*F*W] bool."""
    t = ray_terms(x, y, cx, cy, ok, wrong=None if wrong == "transpose" else wrong)
    B, F, P, W, _ = t.shape
    t = np.ascontiguousarray(t.transpose(0, 1, 3, 2, 4)).reshape(B * F * W, P, NMOM)
    rows = B * F * W
    out = rows_ref.emulate_sums(t, aligned, batch)
    if wrong == "transpose":                                  # the row of (f, w) taken as (w, f)
        out = out.reshape(B, W, F, NMOM).transpose(0, 2, 1, 3).reshape(rows, NMOM)
    return out.reshape(B, F, W, NMOM)
