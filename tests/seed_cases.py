"""
The case table of test_gpu_seed_matrix.py and its reference (CPU only; checked by test_seed_cases_cpu.py).

test_gpu_kernel_matrix.py drives every fp32 backward instantiation with a meridional fan (cx = 0) and the moment seeds of
compute_rms2d and the penalty.  The cases here add the two things it leaves out:

  skew fields   the fan of test_gpu_kernel_matrix._fan turned about the optical axis by AZ (`turned`), cx a leaf.  The lens
                is rotationally symmetric, so every ray is the same ray turned: who dies, and how far everybody stays from
                a normal and from grazing, carries over.  With cx != 0 the fold of the cz0 adjoint into g_cx
                (cz0 = sqrt(1 - cx^2 - cy^2)) is no longer multiplied by zero, and the direct sum no longer cancels.
  dense seeds   losses that are linear in the per-ray outputs with fixed random weights (LOSSES): the backward kernels
                receive gx, gy, gcx, gcy arrays, all four or some (autograd hands over only what a loss produces), with
                and without the moment seed of the rms on top.

The reference is the oracle's autograd in fp64, with an fp32 (IEEE sqrt) twin whose distance from it is the `noise` of every
gate.  z, cx and cy are expanded per ray, as test_gpu_kernel_matrix._oracle does for z and cy.  The fan, its helpers and the
gates are that module's: imported, not copied.
"""
import contextlib
import math

import numpy as np
import torch

import test_gpu_kernel_matrix as km

AZ = math.radians(25.0)
P_MAIN, P_SMALL = km.P_MAIN, km.P_SMALL

# rolled walk-back below (2) and above (21, 32) the unrolled range, the unrolled ends (3, 20), both sides of
# kInvUnrollPairMin (12, 13), three checkpoint buckets; the small pupil (rolled walk-back at an unrolled row count); more
# aspheric rows than hit slots (the device-side fallback)
ROWS = (2, 3, 7, 12, 13, 20, 21, 32)
LENSES = ([(S, v, P_MAIN) for S in ROWS for v in ("sph", "asph")]
          + [(12, v, P_SMALL) for v in ("sph", "asph")]
          + [(16, "asph5", P_MAIN)])
DENSE_LENSES = [(S, v, P_MAIN) for S in (12, 13) for v in ("sph", "asph")]
BATCH_LENSES = [(13, v, P_MAIN) for v in ("sph", "asph")]
BATCH_TILT = 0.005                 # lens b of a batch looks along (1 + BATCH_TILT b) x the directions of lens 0
XY_ROWS = (3, 13, 21)              # x_in, y_in requiring a gradient

OUTS = ("x", "y", "cx", "cy")
# name -> (rms term, the dense terms sum(out * W_out)); the seeds the trace node's backward then receives:
# g_moments from the rms, one per-ray array per dense term, None for the rest (set_materialize_grads(False))
LOSSES = {
    "rms+all": (True, OUTS),          # moment seed and all four arrays together
    "all": (False, OUTS),             # gmom == nullptr with arrays present
    "x": (False, ("x",)),             # gx alone, three null
    "cx": (False, ("cx",)),           # gcx alone: seed bit 4
    "y+cy": (False, ("y", "cy")),     # bits 2 and 8
}
DENSE_LOSSES = ("all", "x", "cx", "y+cy")
CASES = [(lens, "rms+all") for lens in LENSES] + [(lens, loss) for lens in DENSE_LENSES for loss in DENSE_LOSSES]


def seed_bits(loss):
    """The pointer set a loss claims: (moment seed, bit mask of gx 1 | gy 2 | gcx 4 | gcy 8)."""
    rms, terms = LOSSES[loss]
    return rms, sum(1 << OUTS.index(n) for n in terms)


def losses_of(lens):
    return tuple(loss for l, loss in CASES if l == tuple(lens))


def turned(a, az=AZ, dtype=torch.float32):
    """The fan `a` (a test_gpu_kernel_matrix._fan dictionary, cx = 0) turned about the optical axis by `az`:
         x' =  x cos az + y sin az      cx = cy0 sin az
         y' = -x sin az + y cos az      cy = cy0 cos az
    float32 (the cases): cos and sin rounded to float32, the products in float32, so that the kernels, the fp32 oracle and
    the fp64 oracle see the same numbers.  float64: the exact turn of the float32 fan, for the check that the oracle's
    outputs turn with it."""
    assert not a["cx"].any(), "the fan to turn is meridional"
    if dtype == torch.float32:
        co, si = float(np.float32(math.cos(az))), float(np.float32(math.sin(az)))
    else:
        co, si = math.cos(az), math.sin(az)
    x, y, cy0 = a["x"].to(dtype), a["y"].to(dtype), a["cy"].to(dtype)
    out = dict(a)
    out["x"], out["y"] = x * co + y * si, y * co - x * si
    out["cx"], out["cy"] = cy0 * si, cy0 * co
    return out


W_SCALE = 2.0 ** -10


def weights(shape, seed):
    """Wx, Wy, Wcx, Wcy [1,F,P,W]: W_SCALE x seeded randn in float64 rounded to float32 values (a power of two: still exact
    in float32).  Plain randn makes the dense terms' gradient 1e3..1e4 times that of the rms (|g_cy| 5e2..1e3 against
    0.07..0.5): in `rms+all` the moment seed would then sit below every gate, and a kernel that dropped it would pass.  With
    the scale the two parts carry comparable gradient, as lam does for the penalty in test_gpu_kernel_matrix.py."""
    g = torch.Generator().manual_seed(seed)
    return {n: W_SCALE * torch.randn(tuple(shape), generator=g, dtype=torch.float64).float().double() for n in OUTS}


def loss_of(name, outs, wts, rms, ok=None):
    """The loss `name` of the outputs (x, y, cx, cy): [rms()] + the dense terms, on either side.  `rms` is called only by
    the losses that have the term.  `ok`: mask every dense term with it (the reference; the GPU side leaves the terms
    unmasked, so dead rays carry non-zero seeds, which the kernels must ignore)."""
    with_rms, terms = LOSSES[name]
    tot = rms() if with_rms else 0.0
    for n, q in zip(OUTS, outs):
        if n in terms:
            term = q * wts[n].to(q.dtype).to(q.device)
            if ok is not None:
                term = torch.where(ok, term, torch.zeros_like(term))
            tot = tot + term.sum()
    return tot


# Which draw of the weights a lens uses (0 where not listed).  Under mean-free dense weights the cz0 fold is of the order
# cx0^2 of d/dcx, 1e-3..3e-2 from draw to draw, and 100 x the gate is 3e-3: the draw is an input like the lens, and on these
# lenses the first one left some loss below the condition of test_seed_cases_cpu.test_cases_carry_signal (12 draws were
# measured per lens; the ones here clear it by a factor of 1.5 at least in every loss).
WEIGHT_DRAW = {(12, "sph", P_MAIN): 7, (12, "asph", P_MAIN): 4, (20, "sph", P_MAIN): 5, (21, "sph", P_MAIN): 1,
               (32, "sph", P_MAIN): 3}

_FAN = {}


def fan(S, variant, P, n_lens=1):
    """test_gpu_kernel_matrix._fan, once per module run (its own oracle cache is reused where it holds the lens)."""
    key = (S, variant, P, n_lens)
    if key not in _FAN:
        hit = km._ORACLE.get((S, variant, P, None if n_lens == 1 else 0))
        _FAN[key] = hit["args"] if hit is not None else km._fan(S, variant, P, n_lens)
    return _FAN[key]


def lens_of(S, variant, P, b=None):
    """Kernel arguments of a case: the turned fan; lens b of the batch at S when b is not None."""
    if b is None:
        return turned(fan(S, variant, P))
    a = km._perturbed(turned(fan(S, variant, P, len(km.BATCH_W))), b)
    s = float(np.float32(1 + BATCH_TILT * b))
    a["cx"], a["cy"] = a["cx"] * s, a["cy"] * s
    return a


PER_RAY = ("z", "cx", "cy")


def names_of(a):
    return ("z", "cx", "cy", "c", "t", "mu") + (("kappa", "poly") if a["rows"] else ())


def trace(a, dt, lv=None, aggregate=False):
    """The oracle on the arguments `a` in `dt` (fp32: IEEE sqrt), leaves `lv` in place of a's entries."""
    from oracle import trace_oracle as orc
    get = lambda n: lv[n] if lv is not None and n in lv else a[n].to(dt)      # noqa: E731
    kw = dict(kappa=get("kappa"), poly=get("poly"), kind=a["kind"]) if a["rows"] else {}
    return orc.trace_skew_general(*[get(n) for n in ("x", "y", "z", "cx", "cy", "c", "t", "mu")], a["mask"],
                                  ieee_sqrt=(dt == torch.float32), aggregate=aggregate, **kw)


def oracle_grads(a, dt, losses, wts):
    """One oracle run with a retained backward pass per loss: (forward outputs, {loss: {leaf: gradient in fp64}}).
    Leaves: x, y per ray, z, cx, cy expanded per ray, c, t, mu, and kappa, poly where there are aspheric rows."""
    from oracle import trace_oracle as orc
    names = ("x", "y") + names_of(a)
    lv = {n: (a[n].to(dt).expand(a["x"].shape) if n in PER_RAY else a[n].to(dt)).clone().requires_grad_(True) for n in names}
    o = trace(a, dt, lv)
    grads = {}
    for loss in losses:
        val = loss_of(loss, o[:4], wts, lambda: orc.compute_rms2d(o[0], o[1], o[4]), ok=o[4])
        g = torch.autograd.grad(val, [lv[n] for n in names], retain_graph=True, allow_unused=True)
        grads[loss] = {n: (torch.zeros_like(lv[n]) if gi is None else gi).double() for n, gi in zip(names, g)}
    return [t.detach() for t in o[:6]], grads


_REF = {}


def reference(S, variant, P, b=None):
    """fp32 (IEEE sqrt) and fp64 oracle runs of one case lens, with the gradients of its losses (losses_of; a lens of a
    batch: rms+all).  Cached for the module run."""
    key = (S, variant, P, b)
    if key in _REF:
        return _REF[key]
    a = lens_of(S, variant, P, b)
    losses = losses_of((S, variant, P)) if b is None else ("rms+all",)
    wts = weights(a["x"].shape, 4000 + 10 * S + len(a["rows"]) + 1000 * WEIGHT_DRAW.get((S, variant, P), 0))
    res = dict(args=a, names=names_of(a), losses=losses, wts=wts)
    for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
        fwd, grads = oracle_grads(a, dt, losses, wts)
        res[tag] = dict(fwd=fwd, grads=grads)
    _REF[key] = res
    return res


@contextlib.contextmanager
def first_sqrt_detached():
    """The oracle with the first square root of a trace, cz0 = sqrt(1 - cx^2 - cy^2), cut out of the graph: what a backward
    without the fold of the cz0 adjoint into g_cx, g_cy computes."""
    from oracle import trace_oracle as orc
    real, calls = orc._sqrt, [0]

    def cut(v):
        calls[0] += 1
        return real(v).detach() if calls[0] == 1 else real(v)
    orc._sqrt = cut
    try:
        yield
    finally:
        orc._sqrt = real


def summed(n, g):
    """A per-ray launch-condition gradient summed to the kernel's shape (z [1,1,1,1]; cx, cy [1,F,1,1])."""
    return km._reduce("z" if n == "z" else "cy", g, None)


def fold_share(S, variant, P, b=None):
    """{loss: {cx, cy: rel-L2 distance of the gradient without the cz0 fold from the true one}} in fp64."""
    r = reference(S, variant, P, b)
    with first_sqrt_detached():
        _, cut = oracle_grads(r["args"], torch.float64, r["losses"], r["wts"])
    out = {}
    for loss in r["losses"]:
        true = r["f64"]["grads"][loss]
        out[loss] = {n: float((summed(n, cut[loss][n]) - summed(n, true[n])).norm() / summed(n, true[n]).norm())
                     for n in ("cx", "cy")}
    return out
