"""
The definition of imaging.ssim in numpy float64, written from the formulas with explicit window sums (no conv2d, nothing of
torchoptics_amd): the value, the map S, and the gradients to both images for a seed g [B] on ssim [B].

    w[i] ~ exp(-(i - (K - 1)/2)^2 / (2 sigma^2)), normalised to sum 1; the 2-D window is w (x) w; the convolution is VALID
    mu_a = w*a, mu_b = w*b, va = w*a^2 - mu_a^2, vb = w*b^2 - mu_b^2, cab = w*ab - mu_a mu_b, C1 = (k1 L)^2, C2 = (k2 L)^2
    S = (2 mu_a mu_b + C1)(2 cab + C2) / ((mu_a^2 + mu_b^2 + C1)(va + vb + C2)),  ssim[b] = mean of S over Hm x Wm x C
    ds_a = dS/d va, dc = dS/d cab, dm_a = dS/d mu_a - 2 mu_a ds_a - mu_b dc
    g_a[b,p,c] = g[b] / (Hm Wm C) sum_q w(x)w(p - q) (dm_a[q] + 2 a[p] ds_a[q] + b[p] dc[q])

Being the yardstick, it evaluates these where they are well conditioned: the second moments about each image's own mean (they
are shift invariant and the window sums to 1), and the gradient's bracket as
dS/d mu_a[q] + 2 (a[p] - mu_a[q]) ds_a[q] + (b[p] - mu_b[q]) dc[q], pair by pair -- the same numbers, without subtracting
terms a thousand times the result on flat images.

`wrong` names one deliberate mistake (tests/test_ssim_cpu.py shows that the bounds of tests/ssim_cases.py catch each of them).
"""
import numpy as np

WRONG = ("shifted_window", "same_padding", "no_factor_2", "mean_over_image")


def window(K, sigma, centre_offset=0.0):
    i = np.arange(K, dtype=np.float64) - (K - 1) / 2.0 - centre_offset
    w = np.exp(-(i * i) / (2.0 * float(sigma) ** 2))
    return w / w.sum()


def blur(x, w):
    """Valid correlation of x [B,H,W,C] with w (x) w: [B,Hm,Wm,C]."""
    K = len(w)
    Hm, Wm = x.shape[1] - K + 1, x.shape[2] - K + 1
    t = np.zeros((x.shape[0], x.shape[1], Wm, x.shape[3]))
    for j in range(K):
        t += w[j] * x[:, :, j:j + Wm]
    out = np.zeros((x.shape[0], Hm, Wm, x.shape[3]))
    for i in range(K):
        out += w[i] * t[:, i:i + Hm]
    return out


def _spread(w, p, q, mu_p, mu_q, dmu, ds, dc, absolute):
    """out[pixel] = sum over the map pixels m whose window covers it of w(x)w(pixel - m) (dmu[m] + 2 (p[pixel] - mu_p[m]) ds[m]
    + (q[pixel] - mu_q[m]) dc[m]); with `absolute`, of |dm[m]| + 2 |p| |ds[m]| + |q| |dc[m]| with dm = dmu - 2 mu_p ds - mu_q dc:
    the size of the terms as the definition's g_a adds them."""
    K = len(w)
    Hm, Wm = dmu.shape[1], dmu.shape[2]
    out = np.zeros_like(p)
    dm = np.abs(dmu - 2 * mu_p * ds - mu_q * dc)
    for i in range(K):
        for j in range(K):
            at = (slice(None), slice(i, i + Hm), slice(j, j + Wm))
            if absolute:
                out[at] += w[i] * w[j] * (dm + 2 * np.abs(p[at] * ds) + np.abs(q[at] * dc))
            else:
                out[at] += w[i] * w[j] * (dmu + 2 * (p[at] - mu_p) * ds + (q[at] - mu_q) * dc)
    return out


def ssim_ref(a, b, seed=None, max_value=1.0, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03, wrong=None):
    """a, b [B,H,W,C] -> dict(value [B], S [B,Hm,Wm,C], g_a, g_b [B,H,W,C], cond_a, cond_b [B,H,W,C]) in float64.  seed [B]
    (default ones) is the gradient arriving on value.  cond_* is the sum of g_* over the ABSOLUTE values of the terms as the
    definition writes them: the size of what cancels in the gradient, the scale of a first-order rounding model."""
    assert wrong is None or wrong in WRONG, wrong
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    B, H, W, C = a.shape
    K = int(filter_size)
    w = window(K, filter_sigma, 1.0 if wrong == "shifted_window" else 0.0)
    g = np.ones(B) if seed is None else np.asarray(seed, dtype=np.float64).reshape(B)
    Hm, Wm = H - K + 1, W - K + 1
    h = K // 2
    if wrong == "same_padding":          # zero padding to a map of H x W, of which the top-left Hm x Wm is taken
        pad = ((0, 0), (h, h), (h, h), (0, 0))
        ap, bp = np.pad(a, pad), np.pad(b, pad)
        mean = lambda x: blur(x, w)[:, :Hm, :Wm]                                         # noqa: E731
    else:
        ap, bp = a, b
        mean = lambda x: blur(x, w)                                                      # noqa: E731
    ca, cb = a.mean(axis=(1, 2), keepdims=True), b.mean(axis=(1, 2), keepdims=True)
    ma, mb = mean(ap - ca), mean(bp - cb)                                                # centred means
    va, vb, cab = mean((ap - ca) ** 2) - ma ** 2, mean((bp - cb) ** 2) - mb ** 2, mean((ap - ca) * (bp - cb)) - ma * mb
    mu_a, mu_b = ma + ca, mb + cb
    C1, C2 = (k1 * max_value) ** 2, (k2 * max_value) ** 2
    f = 1.0 if wrong == "no_factor_2" else 2.0
    A1, A2 = 2 * mu_a * mu_b + C1, f * cab + C2
    B1, B2 = mu_a ** 2 + mu_b ** 2 + C1, va + vb + C2
    S = A1 * A2 / (B1 * B2)
    n = float(H * W * C) if wrong == "mean_over_image" else float(Hm * Wm * C)
    value = S.sum(axis=(1, 2, 3)) / n
    ds = -S / B2                                         # dS/d va = dS/d vb
    dc = f * A1 / (B1 * B2)
    dmu_a = 2 * mu_b * A2 / (B1 * B2) - 2 * mu_a * S / B1
    dmu_b = 2 * mu_a * A2 / (B1 * B2) - 2 * mu_b * S / B1
    scale = (g / n)[:, None, None, None]
    crop = (lambda x: x[:, h:h + H, h:h + W]) if wrong == "same_padding" else (lambda x: x)        # noqa: E731
    out = dict(value=value, S=S)
    for key, p, q, mu_p, mu_q, dmu in (("a", ap, bp, mu_a, mu_b, dmu_a), ("b", bp, ap, mu_b, mu_a, dmu_b)):
        out["g_" + key] = scale * crop(_spread(w, p, q, mu_p, mu_q, dmu, ds, dc, False))
        out["cond_" + key] = np.abs(scale) * crop(_spread(w, p, q, mu_p, mu_q, dmu, ds, dc, True))
    return out
