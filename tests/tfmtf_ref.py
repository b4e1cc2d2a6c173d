"""The through-focus MTF (metrics.through_focus_mtf / otf_sums_through_focus; tl_tfmtf_sums / tl_tfmtf_seed of
include/tl_trace.h) restated in numpy long double, with the bounds the kernels are held to.  It shares no code with the package.

DEFINITION.  A ray is live iff ok != 0 and s = 1 - cx^2 - cy^2 > 0.  With cz = sqrt(s), u = cx / cz, v = cy / cz, the row's origin
o and the frequency vectors (nu_x, nu_y)_j:  a = nu_x (x - o_x) + nu_y (y - o_y),  b = nu_x u + nu_y v,  and at the plane shifted
by d_z = first + z step the phase is a + d_z b cycles:  C_jz = sum cos 2 pi (a + d_z b),  S_jz = sum sin 2 pi (a + d_z b).  HERE
EVERY PLANE IS EVALUATED DIRECTLY, with no recurrence, every step in np.longdouble (eps 1.08e-19; z step and first + z step are
exact in it for z < 2^11).  The code under test runs the recurrence (c_z, s_z) = (c_{z-1}, s_{z-1}) rotated by (cr, sr) from
plane 0 of each chunk of 16 planes; that it arrives where the direct evaluation does is what the bounds hold it to.

BOUNDS (U = 2^-53; derived here, never fitted to a kernel's output).  Inputs fp32, origin, frequencies and shifts fp64.
  u, v     s = 1 - cx^2 - cy^2 takes four roundings of values <= 1: |ds| <= 4 U, relative 4 U / s; the square root halves it and
           rounds, the quotient rounds:  |du| <= (2 / s + 2) U |u|, v likewise.
  a        as in mtf_ref: with A := |nu_x dx| + |nu_y dy|,  |da| <= 3 U A.
  b        with Bm := |nu_x u| + |nu_y v|: the slopes' errors, two products, one sum:  |db| <= (2 / s + 4) U Bm.
  p0       = a + d0 b: the product rounds (U |d0| Bm), the sum rounds (U (A + |d0| Bm)):
           |dp0| <= 4 U A + (2 / s + 6) U |d0| Bm.   r0 = p0 - rint(p0) and 2 r0 are exact.
  q        = dd b rounds once more:  |dq| <= (2 / s + 5) U |dd| Bm;  rq exact.
  sincospi OpenCL states 4 ulp for sinpi / cospi of values <= 1: 4 U each for (c_0, s_0) and for the rotor; the torch path
           multiplies pi into |t| <= 1 / 8 and calls cos / sin: inside the same 4 U.
  rotation (c cr - s sr, s cr + c sr): two products and a sum of values <= 1 per component, <= 3 U; the rotor's own error turns
           every later plane by 2 pi |dq| + 4 U.  After z rotations, to first order:
               b_z = 2 pi |dp0| + 4 U + z (2 pi |dq| + 4 U + 3 U).
  sums     |C_jz - ref| <= sum_live b_z + (P + 8) U sum_i |term|: any order of P additions (mtf_ref).  S likewise.
  nu = 0   a = b = 0, every term (1, 0), the rotor (1, 0): C = n and S = 0 at every plane, no rounding.
  seeds    Q_jz = gS c_z - gC s_z;  gx = 2 pi sum_j nu_xj sum_z Q_jz,  gu = 2 pi sum_j nu_xj sum_z d_z Q_jz.  With G_jz := |gC_jz| +
           |gS_jz| >= |Q_jz| and >= |dQ / dphase|: the term's error is G (b_z + 3 U) (two products, a difference), then nu_j times
           it (1), the Z - 1 <= 15 and J - 1 <= 15 additions, 2 pi and the product with it (2): SEED_C = 3 + 1 + 15 + 15 + 2 = 36;
           d_z = d0 + z dd and the product with it add 3:
               |gx - ref| <= 2^-24 |ref| + sum_jz |2 pi nu_xj| G_jz (b_jz + 36 U) + 2^-149          (one rounding to fp32)
               |gu - ref| <=               sum_jz |2 pi nu_xj d_z| G_jz (b_jz + 39 U) =: e_u          (gu stays in fp64)
           gcx = (gu (1 - cy^2) + gv cx cy) / cz^3:  the seeds' errors pass through, and the finish rounds: 1 - cy^2 twice, cx cy
           once, two products, a sum, cz three times (2 / s + 1) U and two products, the quotient: <= (12 + 6 / s) U of
           M := ((|gu| + e_u) (1 - cy^2) + (|gv| + e_v) |cx cy|) / cz^3:
               |gcx - ref| <= 2^-24 |ref| + (e_u (1 - cy^2) + e_v |cx cy|) / cz^3 + (12 + 6 / s) U M + 2^-149,   gcy likewise.
"""
import numpy as np

import rows_ref
from mtf_ref import vectors             # noqa: F401 (the frequency vectors are geometric_mtf's; the tests read them from here)
from rows_ref import BLOCK, plan        # noqa: F401

LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, "the reference needs an 80-bit long double"
TWO_PI = 8 * np.arctan(LD(1))
U = 2.0 ** -53
MAX_J = MAX_Z = 16
COLS = 32                               # (vector, plane) columns a launch holds in registers at the most
SEED_C = 3 + 1 + (MAX_Z - 1) + (MAX_J - 1) + 2


def shifts(planes):
    """The Z plane positions (float64): plane 16 q + r at (first + (16 q) step) + r step, every operation in float64."""
    first, step, Z = planes
    return np.array([(first + (z - z % MAX_Z) * step) + (z % MAX_Z) * step for z in range(Z)], np.float64)


def chunk_of(planes):
    """(d0, dd, z within the chunk) per plane: what the recurrence of the code under test starts from."""
    first, step, Z = planes
    z = np.arange(Z)
    return np.array([first + (k - k % MAX_Z) * step for k in z], np.float64), (step if Z > 1 else 0.0), z % MAX_Z


class Terms:
    """Everything per ray, frequency vector and plane, [B,F,P,W,J,Z]: cos and sin of the phase (long double, 0 on dead rays), the
    bound b_z of one term, and per ray [B,F,P,W] the live mask, s, u, v and the cosines (long double, 0 / 1 on dead rays)."""

    def __init__(self, x, y, cx, cy, ok, origin, nu_x, nu_y, planes):
        x, y, cx, cy, ok = np.broadcast_arrays(x, y, cx, cy, ok)
        with np.errstate(invalid="ignore", over="ignore"):
            s = 1 - np.asarray(cx, LD) ** 2 - np.asarray(cy, LD) ** 2
            self.live = live = (ok != 0) & (s > 0)
        x, y, cx, cy = (np.where(live, np.asarray(a, LD), LD(0)) for a in (x, y, cx, cy))
        self.s = s = np.where(live, s, LD(1))
        self.cx, self.cy, self.cz = cx, cy, np.sqrt(s)
        self.u, self.v = cx / self.cz, cy / self.cz
        o = np.broadcast_to(np.asarray(origin, np.float64), (x.shape[0], x.shape[1], x.shape[3], 2)).astype(LD)
        dx, dy = (x - o[:, :, None, :, 0])[..., None], (y - o[:, :, None, :, 1])[..., None]
        self.nx, self.ny = np.asarray(nu_x, LD), np.asarray(nu_y, LD)
        a = self.nx * dx + self.ny * dy                                         # [B,F,P,W,J]
        b = self.nx * self.u[..., None] + self.ny * self.v[..., None]
        self.d = shifts(planes).astype(LD)                                      # [Z]
        u = a[..., None] + self.d * b[..., None]                                # [B,F,P,W,J,Z]
        phi = TWO_PI * (u - np.rint(u))
        lv = live[..., None, None]
        self.cos, self.sin = np.where(lv, np.cos(phi), LD(0)), np.where(lv, np.sin(phi), LD(0))
        A = (np.abs(self.nx * dx) + np.abs(self.ny * dy)).astype(np.float64)
        Bm = (np.abs(self.nx * self.u[..., None]) + np.abs(self.ny * self.v[..., None])).astype(np.float64)
        inv_s = (1 / s).astype(np.float64)[..., None]
        d0, dd, zc = chunk_of(planes)
        dp0 = 4 * U * A[..., None] + ((2 * inv_s + 6) * U * Bm)[..., None] * np.abs(d0)
        dq = (2 * inv_s + 5) * U * abs(dd) * Bm
        self.b = np.where(lv, 2 * np.pi * dp0 + 4 * U + zc * (2 * np.pi * dq[..., None] + 7 * U), 0.0)
        self.P = x.shape[2]


def sums(x, y, cx, cy, ok, origin, nu_x, nu_y, planes):
    """dict: sums [B,F,W,J,Z,2] (float64, rounded from the long-double sums), sums_ld, bound (the same shape), n [B,F,W], terms."""
    t = Terms(x, y, cx, cy, ok, origin, nu_x, nu_y, planes)
    out = np.stack([t.cos.sum(axis=2), t.sin.sum(axis=2)], axis=-1)
    mag = np.stack([np.abs(t.cos).sum(axis=2), np.abs(t.sin).sum(axis=2)], axis=-1).astype(np.float64)
    return dict(sums=out.astype(np.float64), sums_ld=out, bound=t.b.sum(axis=2)[..., None] + (t.P + 8) * U * mag,
                n=t.live.sum(axis=2).astype(np.float64), terms=t, P=t.P)


def seeds(ref, g_sums):
    """d(sum g_sums . sums) / d(x, y, cx, cy) of the evaluation `ref` (sums'): dict gx, gy, gcx, gcy [B,F,P,W] (float64) and their
    bounds gx_bound, .."""
    t = ref["terms"]
    g = np.asarray(g_sums, np.float64).astype(LD)[:, :, None]                   # [B,F,1,W,J,Z,2]
    Q = g[..., 1] * t.cos - g[..., 0] * t.sin                                   # [B,F,P,W,J,Z]
    G = (np.abs(g[..., 0]) + np.abs(g[..., 1])).astype(np.float64)
    out, lin = {}, {}
    for k, nu in (("x", t.nx), ("y", t.ny)):
        w = (TWO_PI * nu)[:, None]                                              # [J,1]
        wa = np.abs(w).astype(np.float64)
        gp = (w * Q).sum(axis=(-2, -1))
        gs = (w * t.d * Q).sum(axis=(-2, -1))
        ep = (wa * G * (t.b + SEED_C * U)).sum(axis=(-2, -1))
        es = (wa * np.abs(t.d).astype(np.float64) * G * (t.b + (SEED_C + 3) * U)).sum(axis=(-2, -1))
        ref_g = np.where(t.live, gp, LD(0)).astype(np.float64)
        out["g" + k] = ref_g
        out["g" + k + "_bound"] = np.where(t.live, 2.0 ** -24 * np.abs(ref_g) + ep, 0.0) + 2.0 ** -149
        lin[k] = (gs, es)
    (gu, eu), (gv, ev) = lin["x"], lin["y"]
    cz3, cxy = t.cz ** 3, t.cx * t.cy
    fin = ((12 + 6 / t.s) * U).astype(np.float64)
    for k, (p, q) in (("cx", (1 - t.cy ** 2, cxy)), ("cy", (cxy, 1 - t.cx ** 2))):
        ref_g = np.where(t.live, (gu * p + gv * q) / cz3, LD(0)).astype(np.float64)
        pa, qa = (np.abs(a / cz3).astype(np.float64) for a in (p, q))
        thru = eu * pa + ev * qa
        M = (np.abs(gu).astype(np.float64) + eu) * pa + (np.abs(gv).astype(np.float64) + ev) * qa
        out["g" + k] = ref_g
        out["g" + k + "_bound"] = np.where(t.live, 2.0 ** -24 * np.abs(ref_g) + thru + fin * M, 0.0) + 2.0 ** -149
    return out


def finish(sums_, n, weights=None, pooled=True):
    """(n, mtf [.., J, Z]) of sums [B,F,W,J,Z,2] and n [B,F,W]: weights, pooling over the wavelengths, modulus, division, zero
    rules."""
    s, n = np.asarray(sums_, LD), np.asarray(n, LD)
    a = np.ones(n.shape[2], LD) if weights is None else np.asarray(weights, np.float64).astype(LD)
    s, n = s * a[:, None, None, None], n * a
    if pooled:
        s, n = s.sum(axis=2), n.sum(axis=2)
    mod = np.sqrt(s[..., 0] ** 2 + s[..., 1] ** 2)
    lit = (n > 0)[..., None, None]
    return n.astype(np.float64), np.where(lit, mod / np.where(lit, n[..., None, None], LD(1)), LD(0)).astype(np.float64)


def centre_of(x, y, cx, cy, ok, centre):
    """The named origin [B,F,W,2] (float64): the live rays' centroid of every row ("row") or of every field's rows together
    ("field"), rounded to float32 and widened; 0 for an empty set."""
    x, y, cx, cy, ok = np.broadcast_arrays(x, y, cx, cy, ok)
    with np.errstate(invalid="ignore", over="ignore"):
        live = (ok != 0) & (1 - np.asarray(cx, LD) ** 2 - np.asarray(cy, LD) ** 2 > 0)
    S = np.stack([live.sum(axis=2).astype(LD)] + [np.where(live, np.asarray(a, LD), LD(0)).sum(axis=2) for a in (x, y)], axis=-1)
    if centre == "field":
        S = np.broadcast_to(S.sum(axis=2, keepdims=True), S.shape)
    return (S[..., 1:3] / np.maximum(S[..., :1], 1)).astype(np.float32).astype(np.float64)


# --------------------------------------------------------------------------------- other evaluations of the same definition
def recurrence(x, y, cx, cy, ok, origin, nu_x, nu_y, planes, order="forward", slope=np.float64, phase=np.float64, rot=np.float64):
    """sums [B,F,W,J,Z,2] by the recurrence of the definition on ONE chunk of planes (Z <= 16), the rays of a row added one by one
    in float64 in the given order ("forward", "reverse", or "blocks": rays j, j + 256, .. of every j in turn).  `slope`: the
    arithmetic u = cx / cz, v = cy / cz are formed in (np.float32: what fp32 slopes would give); `phase`: that of a, b, p0 and q;
    `rot`: that of the rotations.  Everything else is float64."""
    first, step, Z = planes
    assert Z <= MAX_Z
    x, y, cx, cy, ok = np.broadcast_arrays(x, y, cx, cy, ok)
    cx, cy = cx.astype(np.float64), cy.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = 1 - cx * cx - cy * cy
        live = (ok != 0) & (s > 0)
    x, y, cx, cy = (np.where(live, a, 0).astype(np.float64) for a in (x, y, cx, cy))
    cz = np.sqrt(np.where(live, s, 1.0))
    u, v = ((c.astype(slope) / cz.astype(slope)).astype(np.float64) for c in (cx, cy))
    o = np.broadcast_to(np.asarray(origin, np.float64), (x.shape[0], x.shape[1], x.shape[3], 2))
    dx, dy = (x - o[:, :, None, :, 0])[..., None].astype(phase), (y - o[:, :, None, :, 1])[..., None].astype(phase)
    nx, ny = np.asarray(nu_x, phase), np.asarray(nu_y, phase)
    a = nx * dx + ny * dy
    b = nx * u[..., None].astype(phase) + ny * v[..., None].astype(phase)
    p0, q = a + phase(first) * b, phase(step if Z > 1 else 0.0) * b
    assert p0.dtype == phase and q.dtype == phase
    p0, q = p0.astype(np.float64), q.astype(np.float64)
    turn = lambda r: (np.cos((2 * np.pi) * r).astype(rot), np.sin((2 * np.pi) * r).astype(rot))       # noqa: E731
    (c, s_), (cr, sr) = turn(p0 - np.rint(p0)), turn(q - np.rint(q))
    cols = []
    for z in range(Z):
        cols.append(np.stack([c, s_], axis=-1).astype(np.float64))
        c, s_ = c * cr - s_ * sr, s_ * cr + c * sr
        assert c.dtype == rot
    e = np.where(live[..., None, None, None], np.stack(cols, axis=-2), 0.0)      # [B,F,P,W,J,Z,2]
    P = e.shape[2]
    idx = {"forward": np.arange(P), "reverse": np.arange(P)[::-1],
           "blocks": np.concatenate([np.arange(P)[j::BLOCK] for j in range(BLOCK)])}[order]
    acc = np.zeros(e.shape[:2] + e.shape[3:])
    for i in idx:
        acc = acc + e[:, :, i]
    return acc


# ---------------------------------------------------------------------------------------------------------------- the plan
def bucket(J, Z):
    """(JB, ZB): the vectors x planes a launch holds for a call of J vectors and Z planes: the powers of two that hold them, JB
    at most what fits beside ZB planes in COLS columns."""
    ZB = next(b for b in (1, 2, 4, 8, 16) if b >= Z)
    return min(next(b for b in (1, 2, 4, 8, 16) if b >= J), MAX_J, COLS // ZB), ZB


def workspace_bytes(F, P, W, J, Z):
    if not (1 <= J <= MAX_J and 1 <= Z <= MAX_Z):
        return 0
    JB, ZB = bucket(J, Z)
    return rows_ref.workspace_bytes(F, P, W, -(-J // JB) * 2 * JB * ZB)
