"""The cases the Zernike-fit kernels (tl_zfit_moments, tl_zfit_solve, tl_zfit_seed) are held on, shared by tests/test_gpu_zfit.py
and tests/test_zfit_cpu.py: the seeded fans of tests/focus_cases.py, their shapes and memory layouts (place() is that file's, by
import), with seeded pupil coordinates added -- a random full unit disc, as ONE pupil [1,1,P,1] shared by every row ("shared")
or one per row [B,F,P,W] ("per-row").  The spots are those fans' x and y; what the polynomial does not explain stays in q.

What differs from the focus cases: a ray is live iff ok != 0 (there is no direction rule), so "poisoned" takes that file's
poisoned x and y with its clean["ok"] as flags, and poisons px, py of the dead rays too (per-row pupil; a shared pupil serves
live rays of other rows and stays clean); "many-rows-b" (65537 rows of 2 rays: a second launch of all three kernels) runs at
order 2, where 2 n = 4 < J = 5 makes every row invalid."""
import numpy as np

import focus_cases as FC

SHAPES = FC.SHAPES
CASES = ("one-ray", "sub-wave", "wave-plus-one", "block-edge", "multi-partial", "dead-row", "poisoned", "lens-batch", "layout-slice",
         "layout-dense", "many-rows-b")
ORDERS = (2, 3, 4, 5, 6)
ALL_ORDER_CASES = ("sub-wave", "block-edge")
PUPILS = ("shared", "per-row")
KEYS = ("x", "y", "ok", "px", "py")
place_rays = FC.place


def orders_of(name):
    return ORDERS if name in ALL_ORDER_CASES else (2,) if name == "many-rows-b" else (4,)


def sizes(order):
    """(J, K): coefficients and monomial sums per row."""
    return (order + 1) * (order + 2) // 2 - 1, 3 * order * order + 2


def rays(name, pupil):
    """dict x, y, px, py (float32; x, y [B,F,P,W], px, py that or [1,1,P,1]), ok (bool), and for "poisoned" the same with the
    dead rays zeroed as `clean`."""
    B, F, W, P = SHAPES[name]
    r = FC.rays(name)
    out = dict(x=r["x"], y=r["y"], ok=r["ok"])
    if name == "poisoned":
        out["ok"] = r["clean"]["ok"]
    rng = np.random.default_rng(31 + sum(map(ord, name)) + PUPILS.index(pupil))
    shape = (1, 1, P, 1) if pupil == "shared" else (B, F, P, W)
    rho, th = np.sqrt(rng.random(shape)), 2 * np.pi * rng.random(shape)
    out["px"], out["py"] = (rho * np.cos(th)).astype(np.float32), (rho * np.sin(th)).astype(np.float32)
    if name == "poisoned":
        if pupil == "per-row":
            for j, i in enumerate(np.flatnonzero(~out["ok"].ravel())):
                out["px"].ravel()[i], out["py"].ravel()[i] = FC.POISON[j % len(FC.POISON)], FC.POISON[(j + 2) % len(FC.POISON)]
        dead = ~out["ok"]
        out["clean"] = dict(x=r["clean"]["x"], y=r["clean"]["y"], ok=out["ok"],
                            px=np.where(dead, np.float32(0), out["px"]) if pupil == "per-row" else out["px"],
                            py=np.where(dead, np.float32(0), out["py"]) if pupil == "per-row" else out["py"])
    return out


def seeds(name, order):
    """Dense seeds of both signs: g_a [B,F,W,J] and g_q [B,F,W] (float64)."""
    B, F, W, _ = SHAPES[name]
    rng = np.random.default_rng(17 + sum(map(ord, name)) + order)
    return rng.standard_normal((B, F, W, sizes(order)[0])), rng.standard_normal((B, F, W))


def aligned_rows(name, pupil):
    """[B F W] bool: the rows the kernels read with 16-byte loads when the case is placed by place(): those of the focus cases
    whose pupil rows are aligned too (a shared pupil always is; a per-row one lies as x does)."""
    return FC.aligned_rows(name)


def place(arrays, name, device):
    """x, y, ok, px, py as torch tensors on `device`: x, y, ok (and a per-row pupil) [B,F,P,W] in the memory layout the case
    names, a shared pupil as a contiguous [1,1,P,1] tensor."""
    import torch
    per_row = arrays["px"].shape == arrays["x"].shape
    t = place_rays({k: arrays[k] for k in (KEYS if per_row else KEYS[:3])}, name, device)
    if not per_row:
        t["px"], t["py"] = (torch.from_numpy(np.ascontiguousarray(arrays[k])).to(device) for k in ("px", "py"))
    return t
