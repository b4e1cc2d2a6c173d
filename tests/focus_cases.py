"""The cases the focus kernels (tl_focus_moments, tl_focus_seed) are held on, shared by tests/test_gpu_focus.py (the kernels) and
tests/test_focus_cpu.py (the same arithmetic emulated on the CPU): seeded fans shaped like a lens's -- spots of tens of microns
at image heights of millimetres, so that the raw second moments are ~1e5 times the variances -- with dead rays among them.

Shapes are F x W x P (rows x rays).  Memory is the tracer's unless the case says otherwise: [B,F,W,P] with P contiguous, handed
out as [B,F,P,W]; a row then starts at element (f W + w) P, so with P no multiple of 4 a case has rows on BOTH load paths (16-byte
loads where the row base is aligned, one ray at a time elsewhere)."""
import numpy as np

#        name            B  F      W  P     what it reaches
SHAPES = {
    "one-ray":        (1, 1,     1, 1),       # one live lane
    "sub-wave":       (1, 2,     3, 63),      # a partial wave
    "wave-plus-one":  (1, 3,     2, 65),      # a second wave of one ray
    "block-edge":     (1, 3,     2, 257),     # a second block of one ray (strided path), a tail of one ray (aligned path)
    "multi-partial":  (1, 1,     2, 4161),    # several partials per row, and the reduce loop
    "many-rows-a":    (1, 21845, 3, 3),       # 65535 rows: one launch
    "many-rows-b":    (1, 65537, 1, 2),       # 65537 rows: a second launch of two rows
    "dead-row":       (1, 2,     2, 70),      # a row of all ok = 0 and a row with one live ray
    "poisoned":       (1, 2,     3, 300),     # NaN, +-inf, 1e30 and cx^2 + cy^2 >= 1 on dead rays
    "lens-batch":     (3, 2,     2, 132),     # B folded into F; P a multiple of 4: every row on the aligned path
    "layout-tracer":  (1, 3,     3, 256),     # the tracer's view read in place, all rows aligned
    "layout-slice":   (1, 3,     3, 256),     # an interior slice at a 4-byte offset: the strided path
    "layout-expand":  (1, 3,     3, 256),     # cx expanded over wavelengths (copied)
    "layout-dense":   (1, 2,     3, 100),     # a plain contiguous [B,F,P,W] tensor: ray stride W
}
CASES = tuple(SHAPES)
POISON = (np.nan, np.inf, -np.inf, 1e30, -1e30)


def rays(name):
    """dict x, y, cx, cy (float32 [B,F,P,W]), ok (bool), and for "poisoned" the same with the dead rays zeroed as `clean`."""
    B, F, W, P = SHAPES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    r, th = np.sqrt(rng.random((B, F, P, W))), 2 * np.pi * rng.random((B, F, P, W))
    px, py = r * np.cos(th), r * np.sin(th)
    f = (np.arange(F) % 7).reshape(1, F, 1, 1) / 6.0
    w = np.arange(W).reshape(1, 1, 1, W)
    u = 0.17 * px + 0.004 * px * py
    v = 0.17 * py + 0.35 * f + 0.006 * (px ** 2 + py ** 2) * f
    zs, zt = 0.12 + 0.05 * w - 0.08 * f, 0.12 + 0.05 * w + 0.11 * f          # sagittal / tangential foci per row
    x = -zs * u + 2e-3 * rng.standard_normal(u.shape)
    y = 9.0 * f + 0.003 * w * f - zt * (v - 0.35 * f) + 2e-3 * rng.standard_normal(u.shape)
    cz = 1.0 / np.sqrt(1 + u * u + v * v)
    out = dict(x=x, y=y, cx=u * cz, cy=v * cz)
    if name == "layout-expand":
        out["cx"] = np.broadcast_to(out["cx"][..., :1], out["cx"].shape)
    out = {k: np.ascontiguousarray(a, dtype=np.float32) for k, a in out.items()}
    ok = rng.random((B, F, P, W)) > (0.0 if P < 4 and name != "one-ray" else 0.15)
    if name == "one-ray":
        ok[:] = True
    if name == "dead-row":
        ok[0, 0, :, 0] = False
        ok[0, 0, :, 1] = False
        ok[0, 0, 37, 1] = True
    if name == "many-rows-a":
        ok[0, 5, :, 1] = False
    out["ok"] = ok
    if name == "poisoned":
        keys = ("x", "y", "cx", "cy")
        for j, i in enumerate(np.flatnonzero(~ok.ravel())):
            for k, key in enumerate(keys):
                out[key].ravel()[i] = POISON[(j + k) % len(POISON)]
        no_dir = np.flatnonzero(ok.ravel())[::9]                 # ok = 1 but no real direction: dead by the definition
        for sl, cxv, cyv in ((no_dir[0::3], 0.9, 0.6), (no_dir[1::3], 1.0, 0.0), (no_dir[2::3], 0.1, np.nan)):
            out["cx"].ravel()[sl], out["cy"].ravel()[sl] = cxv, cyv
        out["x"].ravel()[no_dir] = 1e30
        is_dead = ~ok
        is_dead.ravel()[no_dir] = True
        out["clean"] = dict({k: np.where(is_dead, np.float32(0), out[k]) for k in keys}, ok=~is_dead)
    return out


def g_moments(name):
    """Dense seeds [B,F,W,11] (float64) of both signs."""
    B, F, W, _ = SHAPES[name]
    return np.random.default_rng(7 + sum(map(ord, name))).standard_normal((B, F, W, 11))


def aligned_rows(name):
    """[B F W] bool: the rows tl_focus_moments reads with 16-byte loads when the case is placed by place()."""
    B, F, W, P = SHAPES[name]
    rows = np.arange(B * F * W)
    if name in ("layout-slice", "layout-dense"):
        return np.zeros(len(rows), bool)
    return (rows * P) % 4 == 0


def place(arrays, name, device):
    """The case's arrays as torch tensors [B,F,P,W] on `device` in the memory layout the case names."""
    import torch
    out = {}
    for k, a in arrays.items():
        if k == "clean":
            continue
        t = torch.from_numpy(np.ascontiguousarray(a)).to(device)
        if name == "layout-dense":
            out[k] = t
            continue
        B, F, P, W = t.shape
        if name == "layout-slice":                                # rays 1 .. P of rows that hold P + 4: base 4 bytes (1 for ok) off
            buf = torch.zeros((B, F, W, P + 4), dtype=t.dtype, device=device)
            buf[..., 1:P + 1] = t.permute(0, 1, 3, 2)
            out[k] = buf[..., 1:P + 1].permute(0, 1, 3, 2)
            continue
        t = t.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
        if name == "layout-expand" and k == "cx":
            t = t[..., :1].expand(B, F, P, W)
        out[k] = t
    return out
