"""
The definition of imaging.ms_ssim in numpy float64, written from the formulas with explicit loops (ssim_ref's window and valid
blur; nothing of torchoptics_amd): the value, the terms and the gradients to both images for a seed g [B] on ms_ssim [B].

    level 0 = the images; level k + 1 = the 2 x 2 mean of level k with stride 2, ceil(H_k / 2) x ceil(W_k / 2):
        pooled[y', x'] = 1/4 sum_{dy,dx in {0,1}} img[min(2y' + dy, H_k - 1), min(2x' + dx, W_k - 1)]
    per level, lens and channel (window, VALID blur, C1, C2 as in ssim_ref):
        cs_k = mean over the map of (2 cab + C2) / (va + vb + C2),   ssim_k = mean over the map of S
    v_k = cs_k for k < M - 1, v_{M-1} = ssim_{M-1};  ms[b,c] = prod_k max(v_k, 0)^p_k;  ms_ssim[b] = mean_c ms[b,c]
    d ms / d v_k = p_k ms / v_k where every term of (b, c) is > 0, else 0 for every k
    the adjoint of the pooling: a level-k pixel receives 1/4 g_{k+1}[y // 2, x // 2], times 2 per axis on which it is the
    doubled last row or column.

As in ssim_ref the moments are taken about each level image's own mean and the gradient's bracket is evaluated pair by pair.
cond_* is the size of the terms that cancel in a gradient: per level ssim_ref's model (the absolute values of the terms as the
definition adds them) times |seed d ms / d v_k|, carried down through the pooling adjoint (its weights are positive) and summed
over the levels.

`wrong` names one deliberate mistake (tests/test_ms_ssim_cpu.py shows that the bounds of tests/ms_ssim_cases.py catch each).
"""
import numpy as np

from ssim_ref import blur, window

WRONG = ("floor_halving", "zero_padding", "ssim_at_every_level", "weights_reversed", "product_of_channel_means",
         "unpool_without_edge_doubling")
TF_POWER = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def _pool_axis(n, mode):
    """[n_out, n] matrix of the mean of pairs along one axis.  'double': the last index of an odd n is taken twice;
    'zero': what lies past the end counts as 0; 'floor': a last odd index is dropped."""
    n_out = n // 2 if mode == "floor" else (n + 1) // 2
    P = np.zeros((n_out, n))
    for o in range(n_out):
        for d in (0, 1):
            i = 2 * o + d
            if i >= n:
                if mode != "double":
                    continue
                i = n - 1
            P[o, i] += 0.5
    return P


def _pool(x, mode):
    Py, Px = _pool_axis(x.shape[1], mode), _pool_axis(x.shape[2], mode)
    return np.einsum("px,boxc->bopc", Px, np.einsum("oy,byxc->boxc", Py, x))


def _unpool(g, H, W, mode):
    """The adjoint of _pool onto a level of H x W."""
    Py, Px = _pool_axis(H, mode), _pool_axis(W, mode)
    return np.einsum("px,bypc->byxc", Px, np.einsum("oy,bopc->bypc", Py, g))


def _spread(w, p, q, mu_p, mu_q, dmu, ds, dc, absolute):
    """out[pixel] = sum over the map pixels m whose window covers it of w(x)w(pixel - m) (dmu[m] + 2 (p[pixel] - mu_p[m]) ds[m]
    + (q[pixel] - mu_q[m]) dc[m]); with `absolute`, of |dm[m]| + 2 |p ds[m]| + |q dc[m]| with dm = dmu - 2 mu_p ds - mu_q dc."""
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


def _level(a, b, w, C1, C2, full):
    """One level: v [B,C] (the mean of S if `full`, of CS otherwise) and grads(seed [B,C]) -> (g_a, g_b, cond_a, cond_b), the
    gradient of sum_{b,c} seed v to the level's images and the size of its terms."""
    ca, cb = a.mean(axis=(1, 2), keepdims=True), b.mean(axis=(1, 2), keepdims=True)
    ma, mb = blur(a - ca, w), blur(b - cb, w)
    va, vb, cab = blur((a - ca) ** 2, w) - ma ** 2, blur((b - cb) ** 2, w) - mb ** 2, blur((a - ca) * (b - cb), w) - ma * mb
    mu_a, mu_b = ma + ca, mb + cb
    A2, B2 = 2 * cab + C2, va + vb + C2
    if full:
        A1, B1 = 2 * mu_a * mu_b + C1, mu_a ** 2 + mu_b ** 2 + C1
        Q = A1 * A2 / (B1 * B2)
        ds, dc = -Q / B2, 2 * A1 / (B1 * B2)
        dmu_a = 2 * mu_b * A2 / (B1 * B2) - 2 * mu_a * Q / B1
        dmu_b = 2 * mu_a * A2 / (B1 * B2) - 2 * mu_b * Q / B1
    else:
        Q = A2 / B2
        ds, dc = -Q / B2, 2 / B2
        dmu_a = dmu_b = np.zeros_like(Q)
    n = float(Q.shape[1] * Q.shape[2])
    v = Q.sum(axis=(1, 2)) / n

    def grads(seed):
        s = (seed / n)[:, None, None, :]
        return (s * _spread(w, a, b, mu_a, mu_b, dmu_a, ds, dc, False), s * _spread(w, b, a, mu_b, mu_a, dmu_b, ds, dc, False),
                np.abs(s) * _spread(w, a, b, mu_a, mu_b, dmu_a, ds, dc, True), np.abs(s) * _spread(w, b, a, mu_b, mu_a, dmu_b, ds, dc, True))
    return v, grads


def ms_ssim_ref(a, b, seed=None, max_value=1.0, power_factors=TF_POWER, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03,
                wrong=None):
    """a, b [B,H,W,C] -> dict(value [B], terms [B,C,M], g_a, g_b, cond_a, cond_b [B,H,W,C]) in float64; seed [B] (default
    ones) is the gradient arriving on value."""
    assert wrong is None or wrong in WRONG, wrong
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    B, H, W, C = a.shape
    p = np.asarray(power_factors, dtype=np.float64)
    if wrong == "weights_reversed":
        p = p[::-1]
    M = len(p)
    w = window(int(filter_size), filter_sigma)
    g = np.ones(B) if seed is None else np.asarray(seed, dtype=np.float64).reshape(B)
    C1, C2 = (k1 * max_value) ** 2, (k2 * max_value) ** 2
    mode = {"floor_halving": "floor", "zero_padding": "zero"}.get(wrong, "double")
    back_mode = "zero" if wrong == "unpool_without_edge_doubling" else mode
    levels = [(a, b)]
    for k in range(1, M):
        levels.append((_pool(levels[-1][0], mode), _pool(levels[-1][1], mode)))
    v = np.zeros((B, C, M))
    grads = []
    for k, (x, y) in enumerate(levels):
        assert min(x.shape[1], x.shape[2]) >= len(w), (k, x.shape)
        v[:, :, k], fn = _level(x, y, w, C1, C2, k == M - 1 or wrong == "ssim_at_every_level")
        grads.append(fn)
    # factor[b,c,k] = d value[b] / d v[b,c,k]
    if wrong == "product_of_channel_means":
        vm = v.mean(axis=1)                                                    # [B,M]
        positive = np.all(vm > 0, axis=1)
        value = np.prod(np.maximum(vm, 0.0) ** p, axis=1)
        factor = np.where(positive[:, None], p * value[:, None] / np.where(positive[:, None], vm, 1.0), 0.0)
        factor = np.repeat(factor[:, None, :], C, axis=1) / C
    else:
        positive = np.all(v > 0, axis=2)                                       # [B,C]
        ms = np.prod(np.maximum(v, 0.0) ** p, axis=2)
        value = ms.mean(axis=1)
        factor = np.where(positive[..., None], p * ms[..., None] / np.where(positive[..., None], v, 1.0), 0.0) / C
    out = dict(value=value, terms=v)
    total = None
    for k in range(M - 1, -1, -1):
        x = levels[k][0]
        parts = grads[k](g[:, None] * factor[:, :, k])
        if total is not None:
            up = [_unpool(t, x.shape[1], x.shape[2], back_mode) for t in total]
            parts = [s + u for s, u in zip(parts, up)]
        total = parts
    out["g_a"], out["g_b"], out["cond_a"], out["cond_b"] = total
    return out
