"""The shapes of the warp_bicubic tests, shared by tests/test_gpu_warp.py (the kernels) and tests/test_warp_cpu.py (the torch
path, and the sharpness of the bounds), the seeded fuzz geometries, the error bounds, and the helper that runs
imaging.warp_bicubic on a case.

Each shape is the smallest at which its branch can go wrong (H x W x C is the image, Ho x Wo the output):
    identity     B 1, 9 x 17 x 1 -> 9 x 17, x = 2j/(W-1) - 1: W - 1 and H - 1 are powers of two, so u is exact, t = 0 and the
                 output equals the image bit for bit
    general      B 2, 23 x 29 x 3 -> 19 x 31, per-lens coordinates in [-1.1, 1.1], gain [B,Ho,Wo,C]: clamped and unclamped
                 pixels and every gradient
    no-gain      the general shape without gain
    shared       B 3, 23 x 29 x 3 -> 70 x 67, coordinates [1,..], gain [1,Ho,Wo,1]: the in-lane sums over lenses and channels;
                 Wo is no multiple of 64; more than one wave per row and more than one block
    thin-row     B 2, 1 x 5 x 2 -> 4 x 6, gain [B,Ho,Wo,1]: H - 1 = 0, so v = 0, g_y = 0 and every row tap is the same row
    thin-col     B 2, 5 x 1 x 2 -> 6 x 4, gain [1,Ho,Wo,C]: the same along x; the gain is shared by the batch but not by the
                 channels, so its C running sums live in g_gain itself
    tiny         B 1, 2 x 3 x 1 -> 5 x 5: every neighbourhood is clipped on both sides
    one          B 1, 4 x 4 x 3 -> 1 x 1: a launch of one lane
    barrel       B 1, 48 x 64 x 3 -> 48 x 64, distortion_grid of a +-5 % profile and a radial_map gain: the map the feature
                 exists for
    many-lenses  B 65537, 2 x 2 x 1 -> 1 x 1, per-lens coordinates: the lens dimension in two launches (65535 + 2)

THE BOUNDS.  With U = 2^-24 and for every element,
    |got - ref| <= (M + terms) U ROUND + COORD,
where ROUND, COORD and terms come from tests/warp_ref.py next to each result, and M counts roundings per term:

  * Rounding of the weights.  They have zeros, so there is no relative bound; a Horner form of a cubic is three steps of a
    multiply and an add (6 roundings, 3 with contraction), so |dw_k| <= 6 U A_k(t), A_k = sum |coef| t^k; the derivative
    weights are two steps, 4 U dA_k(t).  t = u - floor(u) is exact.
  * The sums.  A term wy_i wx_j I passes the product with wx (1), three adds of the row (3), the product with wy (1), three adds
    (3) and the gain (1): 9.  With the two weights, out: 6 + 6 + 9 = 21, and M_out = 22 leaves one for the second order.
    A coordinate gradient: 4 + 6 for the weights, 8 for the two dots, 1 for g_out gain, 1 for the product with the dot, 1 for
    the factor (W - 1)/2: 21, plus one add per term of the in-lane sum over channels (and lenses): `terms`.  The gain gradient
    likewise.  The torch formulation gets the same sums by autograd in another order -- the derivative of each Horner form as
    three products, the sum over the channels before the one over the lenses -- with at most 7 more roundings per term and
    no more adds than `terms`: M_grad = 32 holds both.  The image gradient is g_out gain wy wx (3 products, 12 for the
    weights) added up per image pixel: M_image = 16, terms = the number of taps that land on the pixel.
    ROUND is the sum of the absolute terms with A, dA in place of the weights: it bounds the terms themselves too.
  * Rounding of u: xc + 1 and the product with (W - 1)/2 are two roundings, |du| <= 2 U (W - 1).  The output is C1 in u, so
    COORD = |du| sum |wy| |dwx| |I| + |dv| sum |dwy| |wx| |I| + 1/2 (|du| + |dv|)^2 K2 sum |I| with K2 = 4.5 the largest second
    derivative of a product of two weights; the coordinate gradients are Lipschitz in u piecewise with the second-derivative
    weights, and K3 = 7.5 bounds the next order.  Near an integer u an fp32 evaluation may sit in the neighbouring cell:
    ROUND and COORD take the largest over the cells it may use (warp_ref.py)."""
import numpy as np
import torch

import warp_ref as ref

U = ref.U
M = {"out": 22, "g_x": 32, "g_y": 32, "g_gain": 32, "g_image": 16}
NAMES = ("out", "g_x", "g_y", "g_gain", "g_image")

FIELDS = (0.25, 0.5, 0.75, 1.0)
BARREL_D = (0.05, -0.01, -0.03, -0.05)            # relative distortion at FIELDS: within +-5 %, both signs
BARREL_RI = ((0.98, 0.97, 0.99), (0.9, 0.88, 0.92), (0.8, 0.75, 0.82), (0.6, 0.55, 0.65))

# B, (H, W, C), (Ho, Wo), coordinates, coordinate batch, gain shape (with B, Ho, Wo, C as letters) or None
CASES = {
    "identity": (1, (9, 17, 1), (9, 17), "identity", 1, None),
    "general": (2, (23, 29, 3), (19, 31), "random", "B", ("B", "Ho", "Wo", "C")),
    "no-gain": (2, (23, 29, 3), (19, 31), "random", "B", None),
    "shared": (3, (23, 29, 3), (70, 67), "random", 1, (1, "Ho", "Wo", 1)),
    "thin-row": (2, (1, 5, 2), (4, 6), "random", "B", ("B", "Ho", "Wo", 1)),
    "thin-col": (2, (5, 1, 2), (6, 4), "random", "B", (1, "Ho", "Wo", "C")),
    "tiny": (1, (2, 3, 1), (5, 5), "random", 1, (1, "Ho", "Wo", 1)),
    "one": (1, (4, 4, 3), (1, 1), "random", 1, (1, "Ho", "Wo", "C")),
    "barrel": (1, (48, 64, 3), (48, 64), "barrel", 1, "barrel"),
    "many-lenses": (65537, (2, 2, 1), (1, 1), "random", "B", ("B", "Ho", "Wo", 1)),
}
MAIN = ("general", "shared", "barrel")             # the cases whose bounds the sharpness tests use
SIGNED = ("general", "shared", "thin-col")

FUZZ_SEED, FUZZ_DRAWS = 20261019, 48

_INPUTS, _REF = {}, {}


def _f32(v):
    return np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64)


def inputs(name, signed=False):
    """image, x, y, gain, g_out of a case: float64 arrays of float32 values, made once."""
    key = (name, signed)
    if key in _INPUTS:
        return _INPUTS[key]
    B, (H, W, C), (Ho, Wo), coords, cb, gshape = CASES[name]
    sizes = {"B": B, "Ho": Ho, "Wo": Wo, "C": C}
    gs = None if gshape is None or gshape == "barrel" else tuple(sizes.get(v, v) for v in gshape)
    image, x, y, gain, g_out = ref.make_inputs(B, H, W, C, Ho, Wo, sizes.get(cb, cb), gs, seed=1000 + len(name) + 7 * B, signed=signed)
    if coords == "identity":
        x = np.broadcast_to((2.0 * np.arange(W) / (W - 1) - 1)[None, None, :], (1, Ho, Wo)).copy()
        y = np.broadcast_to((2.0 * np.arange(H) / (H - 1) - 1)[None, :, None], (1, Ho, Wo)).copy()
    elif coords == "barrel":
        from torchoptics_amd import imaging
        d = torch.tensor([BARREL_D], dtype=torch.float64)
        x, y = (v.numpy() for v in imaging.distortion_grid(d, FIELDS, (Ho, Wo)))
        # the coordinate gradient jumps at +-1: the few pixels of this regular grid within 1e-3 of it are moved inside
        x, y = (_f32(np.where(np.abs(np.abs(v) - 1) < 1e-3, v * 0.99, v)) for v in (x, y))
        assert (np.abs(x) > 1).any() and not (np.abs(np.abs(np.stack((x, y))) - 1) < 1e-3).any()
        gain = _f32(imaging.radial_map(torch.tensor([BARREL_RI], dtype=torch.float64), FIELDS, (Ho, Wo), 1.0).numpy())
        if signed:
            gain = gain * np.sign(g_out[:1])
    _INPUTS[key] = (image, x, y, gain, g_out)
    return _INPUTS[key]


def reference(name, signed=False):
    """warp_ref.evaluate of a case: computed once, never changed."""
    key = (name, signed)
    if key not in _REF:
        _REF[key] = ref.evaluate(*inputs(name, signed))
    return _REF[key]


def bound(r, name):
    """The bound of the module docstring for result `name` of the reference namespace r, element by element."""
    return (M[name] + getattr(r, name + "_terms")) * U * getattr(r, name + "_round") + getattr(r, name + "_coord")


def ratio(got, want, limit):
    """The largest |got - want| / limit over ALL elements (0 / 0 counts as 0, anything else over 0 as inf)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.isfinite(got).all() and np.isfinite(want).all() and np.isfinite(limit).all()
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / limit)
    return float(q.max())


def run(imaging, args, device, dtype, fused, needs=("x", "y", "gain", "image")):
    """imaging.warp_bicubic on (image, x, y, gain, g_out) and the backward of sum(g_out out): {'out', 'g_x', ...} as float64
    numpy arrays (a gradient that was not asked for, or the gain's without gain, is absent)."""
    image, x, y, gain, g_out = (None if v is None else torch.as_tensor(v).to(device=device, dtype=dtype) for v in args)
    leaves = {"image": image, "x": x, "y": y, "gain": gain}
    for n in needs:
        if leaves[n] is not None:
            leaves[n].requires_grad_(True)
    out = imaging.warp_bicubic(image, x, y, gain, fused=fused)
    (out * g_out).sum().backward()
    res = {"out": out.detach()}
    res.update({"g_" + n: leaves[n].grad for n in needs if leaves[n] is not None})
    return {k: v.double().cpu().numpy() for k, v in res.items()}


def fuzz_draws():
    """The 48 seeded geometries of the fuzz tests, all valid by construction:
    [(index, (B, H, W, C, Ho, Wo, coordinate batch, gain shape or None))]."""
    rng = np.random.default_rng(FUZZ_SEED)
    draws = []
    for t in range(FUZZ_DRAWS):
        B, C = int(rng.integers(1, 4)), int(rng.integers(1, 5))
        H, W = (int(rng.integers(1, 41)) for _ in range(2))
        Ho, Wo = (int(rng.integers(1, 81)) for _ in range(2))
        shared, has_gain, gain_b, gain_c = (bool(rng.integers(0, 2)) for _ in range(4))
        gshape = (1 if gain_b else B, Ho, Wo, 1 if gain_c else C) if has_gain else None
        draws.append((t, (B, H, W, C, Ho, Wo, 1 if shared else B, gshape)))
    return draws
