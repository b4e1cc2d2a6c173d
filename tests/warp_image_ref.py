"""An independent numpy emulation of the fixed-point image gradient of imaging.warp_bicubic (tl_warp_bwd_image's contract in
include/tl_trace.h), written from the contract: fp32 weights and products, int64 sums, one rounding at the end.  It shares no
code with the kernels or with torchoptics_amd/imaging.py.

    a = fp32(g_out gain);  m = the largest finite |a|;  2^(E-1) <= m < 2^E;  Hb = ceil(log2(16 Ho Wo));  Q = 2^(E + Hb - 62)
    every contribution fp32(fp32(wy_i wx_j) a) / Q is rounded to the nearest int64 and added; the result is fp32(sum Q)
    a non-finite a or a NaN coordinate marks the elements under its 16 clipped taps (NaN) and is left out of m and the sums

It is a model of the arithmetic, not of its bits: the kernels may contract the Horner forms of the weights into FMAs, numpy
rounds every operation.  Both are within the bound of tests/warp_image_cases.py."""
import math

import numpy as np

ALPHA = np.float32(-0.75)
F = np.float32


def seeds(gain, g_out):
    """a = fp32(g_out gain) [B,Ho,Wo,C] as float32 (gain None: g_out itself)."""
    g_out = np.asarray(g_out, dtype=np.float32)
    if gain is None:
        return g_out
    with np.errstate(over="ignore", invalid="ignore"):
        return (g_out * np.broadcast_to(np.asarray(gain, dtype=np.float32), g_out.shape)).astype(np.float32)


def quantum_exponent(a, Ho, Wo):
    """k with Q = 2^k for the seeds a, or None when m = 0 or no seed is finite."""
    mag = np.abs(a[np.isfinite(a)]).astype(np.float64)
    m = float(mag.max()) if mag.size else 0.0
    if m == 0.0:
        return None
    E = math.frexp(m)[1]                                  # m = f 2^E with 0.5 <= f < 1
    assert 2.0 ** (E - 1) <= m < 2.0 ** E
    Hb = (16 * Ho * Wo - 1).bit_length()                  # ceil(log2(n)) for n >= 1
    assert Ho * Wo <= 1 << 26 and Hb <= 30
    return E + Hb - 62


def quantum(gain, g_out):
    """Q of a call (0.0 when every finite contribution is zero)."""
    g_out = np.asarray(g_out)
    k = quantum_exponent(seeds(gain, g_out), g_out.shape[1], g_out.shape[2])
    return 0.0 if k is None else 2.0 ** k


def _axis(x, n):
    """fp32: the four clipped indices [4, ...] and the four weights [4, ...] of one axis (a NaN coordinate: NaN weights and
    the taps around j0 = 0)."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        xc = np.where(x < -1, F(-1), np.where(x > 1, F(1), x)).astype(np.float32)
        u = ((xc + F(1)) * (F(0.5) * F(n - 1))).astype(np.float32)
        fl = np.floor(u)
        t = (u - fl).astype(np.float32)
        j0 = np.where(np.isnan(u), 0, np.nan_to_num(fl, nan=0.0)).astype(np.int64)
        idx = np.stack([np.clip(j0 + k, 0, n - 1) for k in (-1, 0, 1, 2)])
        a, tt = ALPHA, (t * t).astype(np.float32)
        w = np.stack([((a * t - F(2) * a) * t + a) * t, ((a + F(2)) * t - (a + F(3))) * tt + F(1),
                      ((-(a + F(2)) * t + (F(2) * a + F(3))) * t - a) * t, (a - a * t) * tt]).astype(np.float32)
    return idx, w


def emulate(image_shape, x, y, gain, g_out, k=None):
    """The contract on (x, y, gain, g_out) for an image of `image_shape`: (g_image float32 [B,H,W,C], the int64 accumulators).
    `k` overrides the exponent of the quantum (a deliberately wrong fixed scale, for the sharpness test)."""
    B, H, W, C = image_shape
    a = seeds(gain, g_out)
    Ho, Wo = a.shape[1:3]
    if k is None:
        k = quantum_exponent(a, Ho, Wo)
    shape = (B, Ho, Wo)
    cols, wx = _axis(np.broadcast_to(np.asarray(x, dtype=np.float32), shape), W)
    rows, wy = _axis(np.broadcast_to(np.asarray(y, dtype=np.float32), shape), H)
    acc = np.zeros((B, H, W, C), dtype=np.int64)
    marked = np.zeros((B, H, W, C), dtype=bool)
    b = np.broadcast_to(np.arange(B)[:, None, None, None], a.shape)
    c = np.broadcast_to(np.arange(C)[None, None, None, :], a.shape)
    a_ok = np.isfinite(a)
    for i in range(4):
        for j in range(4):
            with np.errstate(invalid="ignore", over="ignore"):
                w = (wy[i] * wx[j]).astype(np.float32)[..., None]
                p = (w * a).astype(np.float32)
            ok = a_ok & ~np.isnan(w)
            r = np.broadcast_to(rows[i][..., None], a.shape)
            q = np.broadcast_to(cols[j][..., None], a.shape)
            marked[b[~ok], r[~ok], q[~ok], c[~ok]] = True
            if k is None:
                continue
            v = np.rint(np.where(ok, p, F(0)).astype(np.float64) * 2.0 ** -k)      # a power of two: exact
            assert np.abs(v).max(initial=0.0) <= 2.0 ** 62
            np.add.at(acc, (b, r, q, c), v.astype(np.int64))
    # 53 bits and a sticky bit, so that the conversion through float64 rounds sum Q once
    hi = (acc >> 11) | ((acc & 0x7ff) != 0)
    with np.errstate(over="ignore"):
        out = (hi.astype(np.float64) * (0.0 if k is None else 2.0 ** (k + 11))).astype(np.float32)
    out[acc == 0] = 0.0
    out[marked] = np.nan
    return out, acc
