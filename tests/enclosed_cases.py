"""The cases the enclosed-energy kernels (tl_enclosed_centroid, tl_enclosed_sums, tl_enclosed_seed) are held on, shared by
tests/test_gpu_enclosed.py and tests/test_enclosed_cpu.py: the seeded fans of tests/focus_cases.py (spots 0.02 - 0.07 mm across at
image heights of millimetres, dead rays among them), their shapes and memory layouts, with radii 0.004 (1 .. 16) mm and softness
0.004 mm: the normalised curve then runs from ~0.15 - 0.3 at R_4 to exactly 1 at R_16, the 0.8 crossing lies inside the range and
the bands overlap, so nearly every live ray gets a gradient.

What differs from the focus cases: a ray is live iff ok != 0 (there is no direction rule), so "poisoned" takes that file's
poisoned coordinates with its clean["ok"] as flags (its ok-true rays at 1e30 are dead here by flag); "layout-expand" expands the
FLAGS over the wavelengths (x and y differ per wavelength); the two many-rows cases run K = 2."""
import numpy as np

import focus_cases as FC

SHAPES = FC.SHAPES
CASES = FC.CASES
SHAPE_NAMES = ("circle", "square")
RADII = tuple(0.004 * k for k in range(1, 17))
SOFT = 0.004
KEYS = ("x", "y", "ok")


def radii_of(name):
    return (0.02, 0.064) if name.startswith("many-rows") else RADII


def rays(name):
    """dict x, y (float32 [B,F,P,W]), ok (bool), and for "poisoned" the same with the dead rays zeroed as `clean`."""
    r = FC.rays(name)
    out = dict(x=r["x"], y=r["y"], ok=r["ok"])
    if name == "poisoned":
        out["ok"] = r["clean"]["ok"]
        out["clean"] = dict(x=r["clean"]["x"], y=r["clean"]["y"], ok=r["clean"]["ok"])
    if name == "layout-expand":
        out["ok"] = np.ascontiguousarray(np.broadcast_to(out["ok"][..., :1], out["ok"].shape))
    return out


def seeds(name, K):
    """Dense seeds of both signs: g_sums [B,F,W,K] and g_S [B,F,W,3] (float64)."""
    B, F, W, _ = SHAPES[name]
    rng = np.random.default_rng(11 + sum(map(ord, name)) + K)
    return rng.standard_normal((B, F, W, K)), rng.standard_normal((B, F, W, 3))


def given_centre(name):
    """A centre [B,F,W,2] (float64) that is not the centroid: the rows' live-ray mean, rounded to fp32, moved by a few microns."""
    r = rays(name).get("clean") or rays(name)
    n = np.maximum(r["ok"].sum(axis=2), 1)
    c = np.stack([np.where(r["ok"], r[k].astype(np.float64), 0.0).sum(axis=2) / n for k in ("x", "y")], axis=-1)
    return c.astype(np.float32).astype(np.float64) + np.array([0.003, -0.002])


def place(arrays, name, device):
    """x, y, ok as torch tensors [B,F,P,W] on `device` in the memory layout the case names (focus_cases.place; the expanded
    array of "layout-expand" is ok)."""
    t = FC.place({k: arrays[k] for k in KEYS}, name, device)
    if name == "layout-expand":
        t["ok"] = t["ok"][..., :1].expand(*t["ok"].shape)
    return t
