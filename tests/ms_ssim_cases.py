"""
The cases of the MS-SSIM tests (tests/test_ms_ssim_cpu.py, tests/test_gpu_ms_ssim.py), their inputs, how an error is measured
and the bound it is held to.  tests/ms_ssim_ref.py is the reference.

SHAPES.  The smallest at which the kernels can go wrong.  The term kernels tile each level's map by 32 x 16 (and the level's
image likewise in the backward) and loop the channels in chunks of 4; the pooling halves every side rounding up, doubling the
last row or column of an odd side.  So: a top level whose map is one pixel; sides that are odd at every level (37 x 43 -> 19 x
22 -> 10 x 11), and odd only on a pooled level (38 x 42 -> 19 x 21); level-0 maps of 16 x 32 and 17 x 33 and images of 32 x 64
and 33 x 65 (the tile edges of the forward and the backward); C = 1, 3, 4, 5; B = 1, 2; K = 3, 5, 11; M = 1 .. 5; tf's
defaults at their smallest legal size (176) and on odd sides; L = 255; a == b; a channel slice and a transposed view; and
b = L - a, whose cs is negative.

CONTENT.  `chart` against its box blur, `smooth` +- 1 % noise, and `noisy`: a + 10 % noise, clipped.  Independent noise pairs
are not used: their coarse cs sits near 0 and the gradient p ms / v is unbounded there.  In every case but `negative` every
term of the reference is >= 0.2 (test_ms_ssim_cpu.py asserts it).

ERRORS, as in ssim_cases.  value and terms: max |delta|.  A gradient: max |delta| / max |reference|, with the size of the terms
that cancel (`cond`) as the denominator where the gradient vanishes (a == b).

BOUNDS.  4 x the torch float32 path's error on the CPU against the reference, measured once per case and recorded in MEASURED.
Floors: a term 4 eps32 (ssim_cases' floor of a mean of S); the value (4 sum_k p_k / v_k + 2 M) eps32 -- each term carries
those 4 ulps, ms's relative sensitivity to v_k is p_k / v_k, and the M powers and products add 2 ulps each; a gradient
16 eps32 max cond / denominator.
"""
import numpy as np
import torch

from ms_ssim_ref import TF_POWER, ms_ssim_ref
from ssim_cases import EPS32, MARGIN, as_tensor

#        name               B    H    W  C   K  M      L  content    seed      layout
CASES = {
    "top_1x1":           (1, 12, 12, 1, 3, 3, 1.0, "noisy", "ones", "dense"),
    "odd_every_level":   (2, 37, 43, 3, 5, 3, 1.0, "chart", "signed", "dense"),
    "odd_level1_only":   (1, 38, 42, 3, 5, 3, 1.0, "noisy", "ones", "dense"),
    "map_16x32":         (2, 20, 36, 3, 5, 2, 1.0, "chart", "signed", "dense"),
    "map_17x33":         (1, 21, 37, 4, 5, 2, 1.0, "noisy", "ones", "dense"),
    "image_33x65":       (1, 33, 65, 5, 5, 2, 1.0, "smooth", "ones", "dense"),
    "image_32x64":       (1, 32, 64, 1, 3, 4, 1.0, "chart", "ones", "dense"),
    "tf_minimum":        (1, 176, 176, 1, 11, 5, 1.0, "chart", "ones", "dense"),
    "tf_odd":            (1, 177, 191, 3, 11, 5, 1.0, "noisy", "ones", "dense"),
    "one_level":         (1, 25, 41, 3, 5, 1, 1.0, "chart", "ones", "dense"),
    "L255":              (1, 37, 43, 3, 5, 3, 255.0, "noisy", "ones", "dense"),
    "equal":             (1, 38, 43, 3, 5, 3, 1.0, "equal", "ones", "dense"),
    "channel_slice":     (2, 37, 42, 3, 5, 3, 1.0, "noisy", "signed", "slice"),
    "transposed":        (1, 38, 43, 3, 5, 3, 1.0, "smooth", "ones", "transposed"),
    "negative":          (2, 37, 43, 3, 5, 3, 1.0, "negative", "signed", "dense"),
}
BOUNDED = tuple(n for n in CASES if n != "negative")
SHARP = ("odd_every_level", "odd_level1_only", "L255")          # where a wrong definition must exceed the bounds
MIN_TERM = 0.2

# The torch float32 path's error on the CPU against ms_ssim_ref, per case: (value, terms, g_a, g_b), measured with errors().
MEASURED = {
    "top_1x1": (3.36e-08, 1.28e-07, 1.13e-06, 1.32e-06),
    "odd_every_level": (4.66e-08, 5.24e-08, 8.07e-07, 3.11e-07),
    "odd_level1_only": (8.55e-09, 9.04e-08, 1.37e-06, 1.56e-06),
    "map_16x32": (1.08e-08, 4.97e-08, 5.55e-07, 2.93e-07),
    "map_17x33": (6.10e-08, 5.68e-08, 4.72e-07, 6.37e-07),
    "image_33x65": (2.29e-08, 9.54e-08, 2.46e-06, 2.68e-06),
    "image_32x64": (1.27e-08, 6.27e-08, 2.87e-06, 1.59e-06),
    "tf_minimum": (1.36e-07, 1.20e-07, 2.97e-06, 1.91e-06),
    "tf_odd": (6.25e-08, 1.70e-07, 2.87e-06, 2.48e-06),
    "one_level": (2.00e-08, 5.59e-08, 8.99e-07, 1.32e-06),
    "L255": (5.67e-08, 6.51e-08, 8.64e-07, 9.38e-07),
    "equal": (0.00e+00, 0.00e+00, 6.50e-09, 6.50e-09),
    "channel_slice": (1.71e-08, 1.28e-07, 9.71e-07, 1.07e-06),
    "transposed": (2.38e-08, 1.56e-07, 3.11e-06, 3.13e-06),
}


def power(M):
    """The weights of a case: tf's defaults when M = 5, else their first M normalised to sum 1 and rounded to float32."""
    if M == len(TF_POWER):
        return TF_POWER
    p = np.asarray(TF_POWER[:M])
    return tuple(float(v) for v in (p / p.sum()).astype(np.float32))


def case_inputs(name):
    """(a, b, seed) of a case as float64 arrays whose values are exactly representable in float32, and its parameters
    dict(max_value, filter_size, power_factors)."""
    B, H, W, C, K, M, L, content, seed_kind, _ = CASES[name]
    rng = np.random.RandomState(sum(ord(ch) for ch in name))
    y, x = np.mgrid[0:H, 0:W]
    if content == "chart":            # a checker chart of 6-pixel squares against its 5 x 5 box blur (edges replicated)
        chk = (((y // 6) + (x // 6)) % 2).astype(np.float64)
        a = 0.1 + 0.8 * chk[None, :, :, None] * (1.0 - 0.1 * np.arange(C))[None, None, None, :] * np.ones((B, 1, 1, 1))
        a = a + 0.02 * rng.rand(B, H, W, C)
        p = np.pad(a, ((0, 0), (2, 2), (2, 2), (0, 0)), mode="edge")
        b = sum(p[:, i:i + H, j:j + W] for i in range(5) for j in range(5)) / 25.0
    elif content == "smooth":
        f = 0.5 + 0.3 * np.sin(0.11 * x + 0.3)[None, :, :, None] * np.cos(0.07 * y + 0.02 * x)[None, :, :, None]
        f = f * (1.0 - 0.1 * np.arange(C))[None, None, None, :] * (1.0 - 0.05 * np.arange(B))[:, None, None, None]
        a, b = f + 0.01 * rng.randn(B, H, W, C), f + 0.01 * rng.randn(B, H, W, C)
    elif content in ("noisy", "equal", "negative"):
        a = rng.rand(B, H, W, C)
        b = np.clip(a + 0.1 * rng.randn(B, H, W, C), 0.0, 1.0)
        if content == "equal":
            b = a.copy()
    else:
        raise KeyError(content)
    a, b = (a * L).astype(np.float32).astype(np.float64), (b * L).astype(np.float32).astype(np.float64)
    if content == "negative":
        b = L - a
        b = b.astype(np.float32).astype(np.float64)
    seed = np.ones(B) if seed_kind == "ones" else np.asarray([(-1.0) ** i * (0.5 + i) for i in range(B)])
    return a, b, seed, dict(max_value=L, filter_size=K, power_factors=power(M))


def run(imaging, name, device, dtype, fused, needs=("a", "b"), **other):
    """imaging.ms_ssim on the case in its layout, and the backward with the case's seed for the images named in `needs`:
    dict(value, terms, g_a, g_b (numpy, None when not needed), a_ptr, b_ptr (the data pointers handed in))."""
    a, b, seed, par = case_inputs(name)
    layout = CASES[name][9]
    ta, tb = as_tensor(a, layout, dtype, device), as_tensor(b, layout, dtype, device)
    ta.requires_grad_("a" in needs)
    tb.requires_grad_("b" in needs)
    value, terms = imaging.ms_ssim(ta, tb, fused=fused, return_terms=True, **{**par, **other})
    assert not terms.requires_grad
    if needs:
        value.backward(torch.from_numpy(seed).to(dtype=dtype, device=device))
    grad = lambda t: None if t.grad is None else t.grad.detach().cpu().numpy()            # noqa: E731
    return dict(value=value.detach().cpu().numpy(), terms=terms.cpu().numpy(), g_a=grad(ta), g_b=grad(tb),
                a_ptr=ta.data_ptr(), b_ptr=tb.data_ptr())


_REF = {}


def reference(name):
    """ms_ssim_ref of the case, computed once and shared; do not modify it."""
    if name not in _REF:
        a, b, seed, par = case_inputs(name)
        _REF[name] = ms_ssim_ref(a, b, seed, **par)
    return _REF[name]


def _denominator(g, cond):
    top, scale = float(np.max(np.abs(g))), float(np.max(cond))
    return scale if top < 1e-6 * scale else top


def errors(name, value, terms, g_a, g_b):
    """(value, terms, g_a, g_b) errors of results (array-likes; a gradient may be None -> None) against reference(name)."""
    ref = reference(name)
    out = [float(np.max(np.abs(np.asarray(value, dtype=np.float64) - ref["value"]))),
           float(np.max(np.abs(np.asarray(terms, dtype=np.float64) - ref["terms"])))]
    for got, key, cond in ((g_a, "g_a", "cond_a"), (g_b, "g_b", "cond_b")):
        if got is None:
            out.append(None)
            continue
        out.append(float(np.max(np.abs(np.asarray(got, dtype=np.float64) - ref[key]))) / _denominator(ref[key], ref[cond]))
    return tuple(out)


def bounds(name):
    """(value, terms, g_a, g_b) bounds of a case (not of `negative`, which is held to exact zeros)."""
    ref = reference(name)
    m = MEASURED[name]
    p = np.asarray(case_inputs(name)[3]["power_factors"])
    M = len(p)
    value_floor = (4 * float(np.max(np.sum(p / ref["terms"], axis=2))) + 2 * M) * EPS32
    out = [max(MARGIN * m[0], value_floor), max(MARGIN * m[1], 4 * EPS32)]
    for k, (key, cond) in enumerate((("g_a", "cond_a"), ("g_b", "cond_b")), start=2):
        out.append(max(MARGIN * m[k], 16 * EPS32 * float(np.max(ref[cond])) / _denominator(ref[key], ref[cond])))
    return tuple(out)


def level_sizes(H, W, M):
    out = []
    for _ in range(M):
        out.append((H, W))
        H, W = -(-H // 2), -(-W // 2)
    return out


def planner(name, n_maps):
    """(tl_ms_ssim_work_bytes, tl_ms_ssim_keep_elems) of a case, restated.  work: the larger of one double per (level, lens,
    tile of 16 x 32 map pixels, channel) and one float per element of the pooled levels 1 .. M - 1 of one image, rounded up to
    256 bytes.  keep: B C M doubles (2 floats each), the pooled levels of both images, n_maps maps (3 for one gradient, 4 for
    both, 0 for none) of B Hm Wm C elements per level."""
    B, H, W, C, K, M = CASES[name][:6]
    partials = pooled = maps = 0
    for k, (h, w) in enumerate(level_sizes(H, W, M)):
        hm, wm = h - K + 1, w - K + 1
        partials += B * (-(-hm // 16)) * (-(-wm // 32)) * C
        pooled += B * h * w * C if k else 0
        maps += B * hm * wm * C
    work = -(-max(8 * partials, 4 * pooled) // 256) * 256
    return work, 2 * B * C * M + 2 * pooled + n_maps * maps
