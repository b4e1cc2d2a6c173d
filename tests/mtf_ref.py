"""The geometric MTF (metrics.geometric_mtf / otf_sums; tl_mtf_sums / tl_mtf_seed of include/tl_trace.h) restated in numpy
long double from the definition, with the bounds the kernels are held to.  It shares no code with the package.

DEFINITION.  A row is one (lens, field, wavelength); a ray is live iff ok != 0.  With the row's origin o and the frequency
vectors (nu_x, nu_y)_j, over the live rays:  dx = x - o_x, dy = y - o_y, u = nu_x dx + nu_y dy (cycles), r = u - rint(u),
C_j = sum cos(2 pi r), S_j = sum sin(2 pi r);  OTF_j = (C_j - i S_j) / n, MTF_j = sqrt(C_j^2 + S_j^2) / n.  Pooled over the
wavelengths C, S and n are added, each times a weight a_w, before the modulus and the division; a set with sum a n = 0, and a
modulus of 0, give 0.  Here every step is in np.longdouble (eps 1.08e-19 on x86-64: 2^11 times finer than the arithmetic under
test), with 2 pi = 8 arctan(1) in that format.

BOUNDS (U = 2^-53; derived here, never fitted to a kernel's output).  The inputs are fp32 and the origin fp64, exact in fp64.
  u        with A := |nu_x dx| + |nu_y dy| >= |u|: dx and dy round once (U A together; nothing for an fp32 origin, the
           differences are then exact), the products once (U A together), the sum once (U |u| <= U A):  |du| <= 3 U A.
  r        u - rint(u) is exact (Sterbenz for |u| >= 1/2, and rint(u) = 0 below), 2 r is exact.  An evaluation that multiplies
           pi in (the torch path: 2 pi (u - rint u)) rounds twice more, 2 U |phi| <= 2 pi U A.  Four roundings of size U A cover
           the kernels with one to spare and the torch path:  |d phi| <= 2 pi 4 U A.
  term     |d cos|, |d sin| <= |d phi|, plus the evaluation: OpenCL states 4 ulp for sinpi / cospi (the device library's
           sincospi), of values <= 1: 4 U.  So per live term  b_ij = 2 pi 4 U A_ij + 4 U.
  sums     |C_j - ref| <= sum_live b_ij + (P + 8) U sum_i |term_ij|: both sides add the same P terms in different orders, any
           order of n additions is within (n - 1) U sum|term| of the exact sum to first order.  S likewise.
  nu = 0   u = 0, r = 0, the term is (1, 0) exactly: C = n and S = 0, no rounding.
  seeds    per ray  g = 2 pi sum_j nu_j q_j,  q_j = gS_j cos phi_j - gC_j sin phi_j.  Counting the roundings of one term in units
           of U |2 pi nu_j q_j|, to first order in q's own magnitude: cos and sin 4 U for their evaluation and 2 pi 4 U A for
           their phase, together 4 (1 + 2 pi A); the two products and the difference of q 3, nu_j q_j 1, the J - 1 <= 15
           additions of the sum over j 15, the constant 2 pi and the product with it 2:  c = 4 + 3 + 1 + 15 + 2 = SEED_C = 25,
           all of it under the factor (1 + 2 pi A_ij) >= 1 that only the first 4 need.  Then one rounding to fp32:
               |g - ref| <= 2^-24 |ref| + SEED_C U sum_j |2 pi nu_j q_ij| (1 + 2 pi A_ij) + 2^-149.
"""
import math

import numpy as np

import rows_ref
from rows_ref import BLOCK, CHUNK, MAX_Y, TARGET_BLOCKS, VEC, plan        # noqa: F401 (the tests read them from here)

LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, "the reference needs an 80-bit long double"
TWO_PI = 8 * np.arctan(LD(1))
U = 2.0 ** -53
MAX_J = 16
SEED_C = 4 + 3 + 1 + (MAX_J - 1) + 2


def vectors(frequencies, directions):
    """(nu_x, nu_y) float64 [D K], direction-major: "tangential" (0, nu), "sagittal" (nu, 0), a float: degrees from +x."""
    nu_x, nu_y = [], []
    for d in directions:
        c, s = (0.0, 1.0) if d == "tangential" else (1.0, 0.0) if d == "sagittal" else (math.cos(math.radians(d)), math.sin(math.radians(d)))
        nu_x += [f * c for f in frequencies]
        nu_y += [f * s for f in frequencies]
    return np.asarray(nu_x, np.float64), np.asarray(nu_y, np.float64)


class Terms:
    """Everything per ray and frequency vector, [B,F,P,W,J]: cos and sin of the phase (long double, 0 on dead rays), the
    amplification A and the live mask [B,F,P,W]."""

    def __init__(self, x, y, ok, origin, nu_x, nu_y):
        x, y, ok = np.broadcast_arrays(x, y, ok)
        self.live = live = ok != 0
        x, y = np.where(live, np.asarray(x, LD), LD(0)), np.where(live, np.asarray(y, LD), LD(0))
        o = np.broadcast_to(np.asarray(origin, np.float64), (x.shape[0], x.shape[1], x.shape[3], 2)).astype(LD)
        dx, dy = (x - o[:, :, None, :, 0])[..., None], (y - o[:, :, None, :, 1])[..., None]
        self.nx, self.ny = np.asarray(nu_x, LD), np.asarray(nu_y, LD)
        u = self.nx * dx + self.ny * dy
        phi = TWO_PI * (u - np.rint(u))
        lv = live[..., None]
        self.cos, self.sin = np.where(lv, np.cos(phi), LD(0)), np.where(lv, np.sin(phi), LD(0))
        self.A = np.where(lv, np.abs(self.nx * dx) + np.abs(self.ny * dy), LD(0)).astype(np.float64)
        self.P = x.shape[2]


def otf_sums(x, y, ok, origin, nu_x, nu_y):
    """dict: sums [B,F,W,J,2] (float64, rounded from the long-double sums), bound (the same shape), n [B,F,W], terms, P."""
    t = Terms(x, y, ok, origin, nu_x, nu_y)
    b = np.where(t.live[..., None], 2 * np.pi * 4 * U * t.A + 4 * U, 0.0).sum(axis=2)
    sums = np.stack([t.cos.sum(axis=2), t.sin.sum(axis=2)], axis=-1)
    mag = np.stack([np.abs(t.cos).sum(axis=2), np.abs(t.sin).sum(axis=2)], axis=-1).astype(np.float64)
    return dict(sums=sums.astype(np.float64), sums_ld=sums, bound=b[..., None] + (t.P + 8) * U * mag,
                n=t.live.sum(axis=2).astype(np.float64), terms=t, P=t.P)


def seeds(ref, g_sums):
    """d(sum g_sums . sums) / d(x, y) of the evaluation `ref` (otf_sums'): dict gx, gy [B,F,P,W] (float64) and gx_bound, gy_bound."""
    t = ref["terms"]
    g = np.asarray(g_sums, np.float64).astype(LD)[:, :, None]                   # [B,F,1,W,J,2]
    q = g[..., 1] * t.cos - g[..., 0] * t.sin
    turn = 1 + 2 * np.pi * t.A
    out = {}
    for k, nu in (("gx", t.nx), ("gy", t.ny)):
        ref_g = np.where(t.live, (TWO_PI * (nu * q).sum(axis=-1)), LD(0)).astype(np.float64)
        mag = (np.abs(TWO_PI * nu * q).astype(np.float64) * turn).sum(axis=-1)
        out[k] = ref_g
        out[k + "_bound"] = np.where(t.live, 2.0 ** -24 * np.abs(ref_g) + SEED_C * U * mag, 0.0) + 2.0 ** -149
    return out


def finish(sums, n, weights=None, pooled=True):
    """(n, mtf [..., J]) of sums [B,F,W,J,2] and n [B,F,W]: weights, pooling over the wavelengths, modulus, division, zero rules."""
    sums, n = np.asarray(sums, LD), np.asarray(n, LD)
    a = np.ones(n.shape[2], LD) if weights is None else np.asarray(weights, np.float64).astype(LD)
    sums, n = sums * a[:, None, None], n * a
    if pooled:
        sums, n = sums.sum(axis=2), n.sum(axis=2)
    mod = np.sqrt(sums[..., 0] ** 2 + sums[..., 1] ** 2)
    lit = (n > 0)[..., None]
    return n.astype(np.float64), np.where(lit, mod / np.where(lit, n[..., None], LD(1)), LD(0)).astype(np.float64)


def centre_of(x, y, ok, centre):
    """The named origin [B,F,W,2] (float64): the live rays' centroid of every row ("row") or of every field's rows together
    ("field"), rounded to float32 and widened; 0 for an empty set."""
    x, y, ok = np.broadcast_arrays(x, y, ok)
    live = ok != 0
    S = np.stack([live.sum(axis=2).astype(LD)] + [np.where(live, np.asarray(a, LD), LD(0)).sum(axis=2) for a in (x, y)], axis=-1)
    if centre == "field":
        S = np.broadcast_to(S.sum(axis=2, keepdims=True), S.shape)
    return (S[..., 1:3] / np.maximum(S[..., :1], 1)).astype(np.float32).astype(np.float64)


# --------------------------------------------------------------------------------- other evaluations of the same definition
def sums_in_order(x, y, ok, origin, nu_x, nu_y, order, phase=np.float64, trig=np.float64):
    """sums [B,F,W,J,2] with the rays of a row added one by one in float64 in the given order ("forward", "reverse", or
    "blocks": rays j, j + 256, ... of every j in turn).  `phase`: the arithmetic of u = nu_x dx + nu_y dy (np.float32: what an
    fp32 phase would give, from the float64 differences); `trig`: that of the sine and cosine of the float64 phase 2 pi r."""
    x, y, ok = np.broadcast_arrays(x, y, ok)
    live = ok != 0
    o = np.broadcast_to(np.asarray(origin, np.float64), (x.shape[0], x.shape[1], x.shape[3], 2))
    dx = (np.where(live, x, 0).astype(np.float64) - o[:, :, None, :, 0])[..., None].astype(phase)
    dy = (np.where(live, y, 0).astype(np.float64) - o[:, :, None, :, 1])[..., None].astype(phase)
    u = np.asarray(nu_x, phase) * dx + np.asarray(nu_y, phase) * dy
    assert u.dtype == phase
    u = u.astype(np.float64)
    phi = ((2 * np.pi) * (u - np.rint(u))).astype(trig)
    e = np.stack([np.cos(phi), np.sin(phi)], axis=-1)
    assert e.dtype == trig
    e = np.where(live[..., None, None], e, 0).astype(np.float64)
    P = e.shape[2]
    idx = {"forward": np.arange(P), "reverse": np.arange(P)[::-1],
           "blocks": np.concatenate([np.arange(P)[j::BLOCK] for j in range(BLOCK)])}[order]
    acc = np.zeros(e.shape[:2] + e.shape[3:])
    for i in idx:
        acc = acc + e[:, :, i]
    return acc


# ---------------------------------------------------------------------------------------------------------------- the plan
def workspace_bytes(F, P, W, J):
    return rows_ref.workspace_bytes(F, P, W, 2 * J) if 1 <= J <= MAX_J else 0
