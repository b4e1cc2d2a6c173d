"""
The cases of the SSIM tests (tests/test_ssim_cpu.py, tests/test_gpu_ssim.py), their inputs, how an error is measured and the
bound it is held to.  tests/ssim_ref.py is the reference.

SHAPES.  The kernels tile the map by 32 columns x 16 rows (two rows per lane) and the image likewise in the backward, loop the
channels in chunks of 4 and are instantiated per window size.  So: a 1 x 1 map; a map of one short row band; map widths of 31,
32, 33 (W = 41, 42, 43 at K = 11) and map heights of 15, 16, 17 (H = 25, 26, 27) and of 31, 32, 33 (two tiles, the second one
short, even or odd); one case of three and five tiles per axis; C = 1, 3, 4, 5 (5 is past one chunk); B = 1, 2; K = 11 and 5;
L = 1 and 255; seeds all-one and random-signed; dense images, channel slices of a wider tensor and transposed H/W views.

ERRORS.  value: max |delta|.  A gradient: max |delta| / max |reference|.  Where the gradient vanishes analytically (a == b: the
reference is zero up to its own rounding, max |reference| < 1e-6 of the terms that cancel in it) the denominator is the size
of those terms instead, ssim_ref's `cond`.

BOUNDS.  Taken from the torch float32 formulation's error on the CPU against the float64 reference, measured once on each
case and recorded in MEASURED below, times MARGIN = 4 for a different summation order -- a first-order model of all three
stages (window sums, the subtraction against C2, the quotient) is impractical because the middle one depends on the local
contrast of the data.  Floors, for cases where the torch path happens to be nearly exact: the value 4 ulps of 1 (the result
is at most 1 in magnitude); a gradient 16 eps32 times the size of the terms that cancel in it (max cond / max |reference|):
every stored partial map is rounded to float32 once and the window sum of K^2 of them adds about as much again.
"""
import numpy as np
import torch

from ssim_ref import ssim_ref

EPS32 = float(np.finfo(np.float32).eps)
MARGIN = 4.0
TILE_X, TILE_Y = 32, 16

#        name              B   H   W  C   K     L  content    seed      layout
CASES = {
    "one_pixel":        (1, 11, 11, 1, 11, 1.0, "noise", "ones", "dense"),
    "thin_band":        (2, 12, 51, 3, 11, 1.0, "noise", "signed", "dense"),
    "map_15x31":        (1, 25, 41, 1, 11, 1.0, "smooth", "ones", "dense"),
    "map_16x32":        (2, 26, 42, 3, 11, 1.0, "chart", "signed", "dense"),
    "map_17x33":        (1, 27, 43, 4, 11, 1.0, "noise", "ones", "dense"),
    "map_31x33":        (2, 41, 43, 5, 11, 1.0, "smooth", "signed", "dense"),
    "map_32x31":        (1, 42, 41, 3, 11, 1.0, "noise", "ones", "dense"),
    "map_33x32":        (1, 43, 42, 3, 11, 1.0, "chart", "ones", "dense"),
    "many_tiles":       (2, 75, 80, 3, 11, 1.0, "noise", "signed", "dense"),
    "k5":               (1, 36, 37, 3, 5, 1.0, "chart", "ones", "dense"),
    "k5_L255":          (2, 20, 40, 2, 5, 255.0, "noise", "signed", "dense"),
    "L255":             (1, 43, 42, 3, 11, 255.0, "chart", "ones", "dense"),
    "nearly_equal":     (2, 42, 43, 3, 11, 1.0, "flat", "signed", "dense"),
    "equal":            (1, 41, 42, 3, 11, 1.0, "equal", "ones", "dense"),
    "constant":         (1, 42, 41, 4, 11, 1.0, "constant", "ones", "dense"),
    "channel_slice":    (2, 43, 41, 3, 11, 1.0, "noise", "signed", "slice"),
    "transposed":       (1, 42, 43, 3, 11, 1.0, "smooth", "ones", "transposed"),
}
SHARP = tuple(n for n, c in CASES.items() if c[6] in ("noise", "chart"))       # where a wrong definition must exceed the bounds
CONSTANTS = (0.3, 0.6)                                                        # the two images of the 'constant' case

# The torch float32 path's error on the CPU against ssim_ref, per case: (value, g_a, g_b), measured with errors() below.
MEASURED = {
    "one_pixel": (4.55e-08, 2.44e-07, 1.35e-07),
    "thin_band": (1.35e-08, 2.67e-07, 2.59e-07),
    "map_15x31": (3.84e-08, 5.37e-07, 5.81e-07),
    "map_16x32": (2.18e-08, 4.45e-07, 3.84e-07),
    "map_17x33": (1.25e-09, 2.09e-07, 1.81e-07),
    "map_31x33": (1.38e-08, 2.01e-06, 1.74e-06),
    "map_32x31": (1.39e-09, 2.83e-07, 2.29e-07),
    "map_33x32": (3.60e-08, 5.64e-07, 3.48e-07),
    "many_tiles": (1.16e-09, 2.25e-07, 2.44e-07),
    "k5": (2.15e-08, 1.06e-06, 1.40e-06),
    "k5_L255": (3.53e-09, 2.41e-07, 1.99e-07),
    "L255": (3.59e-09, 5.23e-07, 2.82e-07),
    "nearly_equal": (6.01e-08, 2.08e-07, 3.05e-07),
    "equal": (0.00e+00, 2.41e-08, 2.41e-08),
    "constant": (1.36e-07, 2.67e-07, 2.90e-07),
    "channel_slice": (1.21e-09, 2.07e-07, 2.19e-07),
    "transposed": (8.42e-09, 1.61e-06, 1.91e-06),
}


def case_inputs(name):
    """(a, b, seed) of a case as float64 arrays whose values are exactly representable in float32, and its parameters
    dict(max_value, filter_size)."""
    B, H, W, C, K, L, content, seed_kind, _ = CASES[name]
    rng = np.random.RandomState(sum(ord(ch) for ch in name))
    if content == "noise":
        a, b = rng.rand(B, H, W, C), rng.rand(B, H, W, C)
    elif content == "smooth":
        y, x = np.mgrid[0:H, 0:W]
        f = 0.5 + 0.3 * np.sin(0.11 * x + 0.3)[None, :, :, None] * np.cos(0.07 * y + 0.02 * x)[None, :, :, None]
        f = f * (1.0 - 0.1 * np.arange(C))[None, None, None, :] * (1.0 - 0.05 * np.arange(B))[:, None, None, None]
        a, b = f + 0.01 * rng.randn(B, H, W, C), f + 0.01 * rng.randn(B, H, W, C)
    elif content == "chart":          # a checker chart of 6-pixel squares against its 5 x 5 box blur (edges replicated)
        y, x = np.mgrid[0:H, 0:W]
        chk = (((y // 6) + (x // 6)) % 2).astype(np.float64)
        a = 0.1 + 0.8 * chk[None, :, :, None] * (1.0 - 0.1 * np.arange(C))[None, None, None, :] * np.ones((B, 1, 1, 1))
        a = a + 0.02 * rng.rand(B, H, W, C)
        p = np.pad(a, ((0, 0), (2, 2), (2, 2), (0, 0)), mode="edge")
        b = sum(p[:, i:i + H, j:j + W] for i in range(5) for j in range(5)) / 25.0
    elif content == "flat":
        a, b = np.full((B, H, W, C), 0.9), 0.9 + 1e-3 * rng.rand(B, H, W, C)
    elif content == "equal":
        a = rng.rand(B, H, W, C)
        b = a.copy()
    elif content == "constant":
        a, b = np.full((B, H, W, C), CONSTANTS[0]), np.full((B, H, W, C), CONSTANTS[1])
    else:
        raise KeyError(content)
    a, b = (a * L).astype(np.float32).astype(np.float64), (b * L).astype(np.float32).astype(np.float64)
    seed = np.ones(B) if seed_kind == "ones" else np.asarray([(-1.0) ** i * (0.5 + i) for i in range(B)])
    return a, b, seed, dict(max_value=L, filter_size=K)


def as_tensor(x, layout, dtype, device="cpu"):
    """x [B,H,W,C] (numpy) as a torch tensor of `layout`: 'dense', 'slice' (channels 1 .. C of a tensor of C + 2 channels) or
    'transposed' (a transposed view of a dense [B,W,H,C] tensor)."""
    t = torch.from_numpy(np.ascontiguousarray(x)).to(dtype=dtype, device=device)
    if layout == "slice":
        wide = torch.zeros(t.shape[:3] + (t.shape[3] + 2,), dtype=dtype, device=device)
        wide[..., 1:-1] = t
        t = wide[..., 1:-1]
    elif layout == "transposed":
        t = t.transpose(1, 2).contiguous().transpose(1, 2)
    return t


def run(imaging, name, device, dtype, fused, needs=("a", "b"), **other):
    """imaging.ssim on the case in its layout, and the backward with the case's seed for the images named in `needs`:
    dict(value, g_a, g_b (numpy, None when not needed), a_ptr, b_ptr (the data pointers handed in))."""
    a, b, seed, par = case_inputs(name)
    layout = CASES[name][8]
    ta, tb = as_tensor(a, layout, dtype, device), as_tensor(b, layout, dtype, device)
    ta.requires_grad_("a" in needs)
    tb.requires_grad_("b" in needs)
    value = imaging.ssim(ta, tb, fused=fused, **{**par, **other})
    if needs:
        value.backward(torch.from_numpy(seed).to(dtype=dtype, device=device))
    grad = lambda t: None if t.grad is None else t.grad.detach().cpu().numpy()            # noqa: E731
    return dict(value=value.detach().cpu().numpy(), g_a=grad(ta), g_b=grad(tb), a_ptr=ta.data_ptr(), b_ptr=tb.data_ptr())


_REF = {}


def reference(name):
    """ssim_ref of the case, computed once and shared; do not modify it."""
    if name not in _REF:
        a, b, seed, par = case_inputs(name)
        _REF[name] = ssim_ref(a, b, seed, **par)
    return _REF[name]


def errors(name, value, g_a, g_b):
    """(value error, g_a error, g_b error) of results (array-likes; a gradient may be None -> None) against reference(name),
    measured as the module docstring says."""
    ref = reference(name)
    out = [float(np.max(np.abs(np.asarray(value, dtype=np.float64) - ref["value"])))]
    for got, key, cond in ((g_a, "g_a", "cond_a"), (g_b, "g_b", "cond_b")):
        if got is None:
            out.append(None)
            continue
        out.append(float(np.max(np.abs(np.asarray(got, dtype=np.float64) - ref[key]))) / _denominator(ref[key], ref[cond]))
    return tuple(out)


def _denominator(g, cond):
    top, scale = float(np.max(np.abs(g))), float(np.max(cond))
    return scale if top < 1e-6 * scale else top


def bounds(name):
    """(value bound, g_a bound, g_b bound) of a case."""
    ref = reference(name)
    m = MEASURED[name]
    out = [max(MARGIN * m[0], 4 * EPS32)]
    for k, (key, cond) in enumerate((("g_a", "cond_a"), ("g_b", "cond_b")), start=1):
        out.append(max(MARGIN * m[k], 16 * EPS32 * float(np.max(ref[cond])) / _denominator(ref[key], ref[cond])))
    return tuple(out)


def planner(name):
    """(tl_ssim_work_bytes, tl_ssim_maps_elems) of a case, restated: one double per lens and tile of 16 x 32 map pixels,
    rounded up to 256 bytes; B Hm Wm C map elements."""
    B, H, W, C, K = CASES[name][:5]
    Hm, Wm = H - K + 1, W - K + 1
    tiles = -(-Hm // TILE_Y) * -(-Wm // TILE_X)
    return -(-(B * tiles * 8) // 256) * 256, B * Hm * Wm * C
