"""
The case table of test_gpu_fwd_matrix.py and its references (CPU only; checked by test_fwd_cases_cpu.py).

The fp32 forward -- trace_fwd_kernel<PEN, ASPH, OPD> and trace_fwd_plain_kernel<2> in csrc/tl_kernels.inc -- is what every
step runs first.  The other suites hold it bit-equal to the IEEE oracle on all-spherical lenses in strict mode at one chunk
per block, and to a max-norm gate on a fan with the ill-conditioned rays taken out.  The cases here add:

  the fan       nothing filtered: dead, backward, grazing and near-normal rays stay in (`lens`);
  the outputs   rays | opd | pen (stacks) | pensum (stacks pointer NULL), in strict and fast mode: with {sph, asph} every
                forward kernel of the build (KERNELS, held to launch_fwd's `if` chain by the CPU test);
  the plans     one chunk per block, blocks of 1 and 2, and of 2 and 3 chunks in one launch (SHAPES / EXPECT), in a batch of
                four lenses with per-lens c, t and cy;
  the columns   all ten moments against fp64 sums of the fp32 values the kernel wrote (`moments_of`);
  the bytes     cond_flags and asph_hits, which the walk-back reads instead of recomputing.

References per (lens, shape, lens b): one fp32 (IEEE sqrt) and one fp64 run of oracle.trace_skew_general(aggregate=True,
n_index=...).  The per-ray gate is |got - f64| <= C k tol A_i with A_i = 1 / min cos^2 over the ray's live rows (fp64
oracle), k = 10 in fast mode; C is 4 x the fp32 oracle's own worst |o32 - o64| / (tol A_i) over the whole table, measured
on the CPU output by output (`python tests/fwd_cases.py`, C_MEASURED below and profiles/fwd_accuracy.txt).  Two more cosines divide on the
way and enter A_i where they act, each derived at its function: the one to the image plane's normal for x, y and the path
length (image_amplification), and the sine of the angle itself for theta (normal_amplification).  Without them the unfiltered
fan sets C to 4e5 (three rays leaving the last row at right angles to the axis) and the gate holds nothing.
"""
import contextlib
import math

import numpy as np
import torch

import test_gpu_kernel_matrix as km
from opd_cases import mu_of_n, n_of_mu
from spot_cases import make_plan
from zoom20_rows import lens_args

MODES = ("strict", "fast")
OUTPUTS = ("rays", "opd", "pen", "pensum")
VARIANTS = ("sph", "asph")
FILL = 1.2                          # pupil radius / design aperture: radius sqrt(u) 0.6 EPD
FAR_EVERY, FAR_MAX = 16, 5.0        # every 16th point goes 1 .. 5 x further out ...
FAR_FIRST = 8                       # ... from point 8 on: the single point of P = 1 and the last point of every pupil stay in
ILL_COS2 = 0.01                     # kCondThr of tl_kernels.inc: flag 2 and moment 9 count live rays below it
NEAR_THR = 1e-4                     # |min cos^2 - ILL_COS2| below this: left out of the flag comparison
LEFT_OUT_CAP = 2e-5                 # share of a case's rays the reference itself may leave out (ok differs / near threshold)

# name -> (B, F, W, pupil sizes).  EXPECT: (nbx, R, chunks per block) of the forward plan, per (name, P)
SHAPES = {
    "main": (1, 3, 3, (777,)),
    "edge": (1, 2, 3, (1, 63, 64, 65, 255, 256, 257, 511, 513)),
    "r2": (4, 4, 3, (22101,)),
    "r3": (4, 4, 3, (33101,)),
}
EXPECT = {
    ("main", 777): (4, 1, {1}),
    ("edge", 1): (1, 1, {1}), ("edge", 63): (1, 1, {1}), ("edge", 64): (1, 1, {1}), ("edge", 65): (1, 1, {1}),
    ("edge", 255): (1, 1, {1}), ("edge", 256): (1, 1, {1}), ("edge", 257): (2, 1, {1}), ("edge", 511): (2, 1, {1}),
    ("edge", 513): (3, 1, {1}),
    ("r2", 22101): (44, 2, {1, 2}),
    ("r3", 33101): (44, 3, {2, 3}),
}
ALONE = (130, 1, {1})               # one (b, f, w) row of r3 traced alone: B = F = W = 1, P = 33 101
FWD_PLAN = dict(cap=8192, rmax=32, few=2048, rwant=8)          # plan_fwd of csrc/tl_api.hip
FIELDS = {2: (0.3, 1.0), 3: km.REL_FIELDS, 4: (0.3, 0.65, 0.85, 1.0)}
CY_SPREAD = 0.02                    # lens b of a batch looks along (1 -+ 2 %) x the directions of the table

MAIN_ROWS = (1, 2, 5, 7, 12, 20, 31, 32)
BIG_LENSES = ((5, "sph"), (7, "asph"))          # r2, r3
EDGE_ROWS = (7,)
HIT_LENSES = ((7, "asph"), (16, "asph5"))       # 3 and 5 aspheric rows against 4 hit slots
HIT_SLOTS = 4


def lenses_of(name):
    if name == "main":
        # (the 5-row lens is here for its backward rays and as the spherical lens of r2 and r3; with its last row aspheric
        #  the fp32 oracle's Newton loses 1 .. 7 rays that the fp64 one keeps in 30 of 40 draws of the fan: above the cap)
        return tuple((S, v) for S in MAIN_ROWS for v in VARIANTS if (S, v) != (5, "asph"))
    if name == "edge":
        return tuple((S, v) for S in EDGE_ROWS for v in VARIANTS)
    return BIG_LENSES


# (shape, P, S, variant) of every forward case
CASES = [(name, P, S, v) for name, (_, _, _, ps) in SHAPES.items() for P in ps for S, v in lenses_of(name)]

# The kernel a call runs: (variant, output, mode) -> kernel names in launch order (launch_fwd, csrc/tl_kernels.inc)
_K = "trace_fwd_kernel<%s, %s, %s>"
_PLAIN = "trace_fwd_plain_kernel<2>"
KERNELS = {}
for _v, _a in (("sph", "false"), ("asph", "true")):
    for _m in MODES:
        KERNELS[(_v, "pen", _m)] = KERNELS[(_v, "pensum", _m)] = (_K % ("true", _a, "false"),)
        KERNELS[(_v, "rays", _m)] = (_K % ("false", _a, "false"),)
        KERNELS[(_v, "opd", _m)] = (_K % ("false", _a, "true"),)
KERNELS[("sph", "rays", "fast")] = (_PLAIN,)
KERNELS[("sph", "opd", "fast")] = (_PLAIN, _K % ("false", "false", "true"))     # rays and moments, then the OPD alone
ALL_FWD_KERNELS = {_K % (p, a, o) for p, a, o in (("true", "true", "false"), ("true", "false", "false"),
                                                 ("false", "true", "true"), ("false", "true", "false"),
                                                 ("false", "false", "true"), ("false", "false", "false"))} | {_PLAIN}

# Per-ray tolerances of the suite (test_gpu_asphere.py, test_gpu_penalty.py): mm, direction cosines, theta / (pi/2)
TOL = {"x": 2e-5, "y": 2e-5, "cx": 2e-6, "cy": 2e-6, "opd": 2e-5, "hits": 2e-5, "zrelu": 2e-5, "theta": 3e-6, "thetap": 3e-6}
K_FAST = 10.0
# The fp32 IEEE oracle's own worst |o32 - o64| / (tol A_i) over every case, lens and ray of the table, output by output
# (`python tests/fwd_cases.py` prints them with the case that set each), and the gate's constant: 4 x it, not below 1.  The
# margin of 4 is for the kernels' operation order and acosf, which differ from the oracle's.  One constant for all outputs
# would be theta's 6.68 (20 rows, aspheric, 777 points); each output takes its own, none above that: with 6.68 on x and
# y, reading the next wavelength's mu on the colour-corrected 20-row lens would miss the gate by 47 x, not by 100.
C_MEASURED = {"x": 0.2905, "y": 0.2814, "cx": 0.7339, "cy": 0.6275, "opd": 0.4145, "zrelu": 0.0920, "theta": 0.7600,
              "thetap": 1.6696, "hits": 0.2026}
C = {n: max(1.0, 4.0 * v) for n, v in C_MEASURED.items()}


def plan_of(B, F, W, P):
    """(nbx, R, set of chunks per block) of the forward launch: make_plan and TL_BLOCK_CHUNKS."""
    nbx, R = make_plan(P, B * F * W, FWD_PLAN["cap"], FWD_PLAN["rmax"], FWD_PLAN["few"], FWD_PLAN["rwant"])
    chunks = -(-P // 256)
    share = {(bx + 1) * chunks // nbx - bx * chunks // nbx for bx in range(nbx)}
    return nbx, R, share


# ------------------------------------------------------------------------------------------------------------------
# lenses and fans
# ------------------------------------------------------------------------------------------------------------------

# Which draw of the fan a case uses (0 where not listed): seed 1000 S + P + 10^6 draw.  The first draw leaves these cases
# short of a premise of test_fwd_cases_cpu.py -- no ill-conditioned live ray at all (flag 2), or a pupil point that the fp32
# oracle loses at another row than the fp64 one (Newton's convergence test), or one within 1e-4 of the flag's threshold, each
# times three wavelengths and more than the 2e-5 of the rays that a case may leave out.  The draw is an input like the lens.
REDRAW = {("main", 777, 5, "sph"): 1, ("main", 777, 7, "asph"): 1, ("main", 777, 12, "sph"): 1, ("main", 777, 12, "asph"): 1,
          ("edge", 511, 7, "asph"): 1, ("edge", 513, 7, "asph"): 1}

_LENS = {}


def lens(name, P, S, variant):
    """CPU kernel arguments of a case, one dictionary per lens of the launch: x, y [1,1,P,1]; z [1,1,1,1]; cx [1,1,1,1];
    cy [1,F,1,1]; c, t, mask [1,1,1,1,S]; mu [1,1,1,W,S]; n_index [1,1,1,W,S+1]; kappa [S], poly [S,4], kind, rows."""
    key = (name, P, S, variant)
    if key in _LENS:
        return _LENS[key]
    import torchoptics_amd as ta
    from torchoptics_amd import prescriptions as PR
    B, F, W, _ = SHAPES[name]
    a = lens_args(ta, S, n_rays=(4, 4), rel_fields=FIELDS[F])
    assert a["cy"].shape == (1, F, 1, 1) and a["mu"].shape == (1, 1, 1, W, S)
    epd = float(PR.zoom20("cpu", requires_grad=False)[1].epd.item())
    rng = np.random.default_rng(1000 * S + P + 10 ** 6 * REDRAW.get(key, 0))
    r = (np.sqrt(rng.random(P)) * (0.5 * epd * FILL)).astype(np.float32)
    th = (rng.random(P) * 2 * np.pi).astype(np.float32)
    far = np.ones(P, np.float32)
    far[FAR_FIRST::FAR_EVERY] = rng.uniform(1.0, FAR_MAX, len(far[FAR_FIRST::FAR_EVERY])).astype(np.float32)
    r = r * far
    a["x"] = torch.from_numpy(r * np.cos(th)).reshape(1, 1, P, 1)
    a["y"] = torch.from_numpy(r * np.sin(th)).reshape(1, 1, P, 1)
    rows = km._asph_rows(S, variant)
    a["rows"], a["kind"] = rows, None
    if rows:                                    # coefficients drawn as test_gpu_kernel_matrix._fan draws them
        kap, pol = np.zeros(S, np.float32), np.zeros((S, 4), np.float32)
        kap[rows] = rng.uniform(-0.5, 0.3, len(rows))
        pol[rows, 0] = rng.choice([-1.0, 1.0], len(rows)) * rng.uniform(1e-6, 1e-5, len(rows))
        pol[rows, 1] = rng.uniform(-1e-8, 1e-8, len(rows))
        a["kappa"], a["poly"] = torch.from_numpy(kap), torch.from_numpy(pol)
        a["kind"] = [1 if k in rows else 0 for k in range(S)]
    out = []
    for b in range(B):
        ab = dict(km._perturbed(a, b))
        if B > 1:
            ab["cy"] = a["cy"] * float(np.float32(1.0 + CY_SPREAD * (2.0 * b / (B - 1) - 1.0)))
        ab["n_index"] = n_of_mu(ab["mu"].double()).float()
        ab["mu"] = mu_of_n(ab["n_index"].double()).float()
        out.append(ab)
    _LENS[key] = out
    return out


def trace(a, dt, allow_backward_rays=True, aggregate=True, **swap):
    """The oracle on the lens `a` in `dt` (fp32: IEEE sqrt), entries of `swap` in place of a's."""
    from oracle import trace_oracle as orc
    a = dict(a, **swap)
    kw = dict(kappa=a["kappa"].to(dt), poly=a["poly"].to(dt), kind=a["kind"]) if a["rows"] else {}
    return orc.trace_skew_general(*[a[n].to(dt) for n in ("x", "y", "z", "cx", "cy", "c", "t", "mu")], a["mask"],
                                  allow_backward_rays=allow_backward_rays, n_index=a["n_index"].to(dt),
                                  ieee_sqrt=(dt == torch.float32), aggregate=aggregate, **kw)


@contextlib.contextmanager
def recorded_hits():
    """The (X, Y) that oracle.trace_oracle.asphere_hit returns, call by call: entry j is the j-th aspheric row of a trace."""
    from oracle import trace_oracle as orc
    real, rec = orc.asphere_hit, []

    def wrapped(c, kappa, a, r):
        out = real(c, kappa, a, r)
        rec.append((out[2].detach(), out[3].detach()))
        return out
    orc.asphere_hit = wrapped
    try:
        yield rec
    finally:
        orc.asphere_hit = real


def oracle_run(a, dt, allow_backward_rays=True, **swap):
    """One oracle run as a dictionary of [1,F,P,W] tensors: fwd (x, y, cx, cy, ok, back), opd, stk [3,S,1,F,P,W] (z_RELU,
    theta, theta'), hits [rows,2,1,F,P,W] (None without aspheric rows)."""
    with torch.no_grad(), recorded_hits() as rec:
        o = trace(a, dt, allow_backward_rays, **swap)
    shape = o[1].shape
    stk = torch.stack([torch.stack([q.expand(shape) for q in o[7][key]]) for key in ("z_RELU", "theta_norm", "theta_prime_norm")])
    hits = torch.stack([torch.stack([X.expand(shape), Y.expand(shape)]) for X, Y in rec]) if rec else None
    return dict(fwd=[q.expand(shape) for q in o[:6]], opd=o[6].expand(shape), stk=stk, hits=hits)


def died_at(stk):
    """Rows each ray passed alive (S: it reached the image plane), from stacks [3,S,...]: a dead row holds theta = 1 exactly."""
    return (stk[1] != 1.0).sum(dim=0)


def conditioning(stk64):
    """From the fp64 stacks [3,S,1,F,P,W]: (alive, min cos^2 over the live rows of each ray, flags, near the threshold).
    cos^2 = cos^2(theta pi/2); a dead row holds theta = 1 exactly.  Flag 0 dead, 1 live, 2 live with min cos^2 < ILL_COS2."""
    th = stk64[1:3].double()
    live = th != 1.0
    cos2 = torch.where(live, torch.cos(th * (math.pi / 2)).square(), torch.ones_like(th))
    min_cos2 = cos2.amin(dim=(0, 1))
    alive = live[0, -1]                           # behind the last row, before the image plane's backward test
    flags = torch.where(alive, torch.where(min_cos2 < ILL_COS2, 2, 1), 0).to(torch.uint8)
    near = alive & ((min_cos2 - ILL_COS2).abs() < NEAR_THR)
    return alive, min_cos2, flags, near


def image_amplification(fwd64):
    """cz^-3 at the image plane (fp64 oracle; 1 for a dead ray).  The transfer x + (-z / cz) cx divides by the cosine to
    the image plane's normal as a row divides by its own: d x_image = ... + z cx / cz^2 d cz with d cz = -(cx d cx + cy d cy)
    / cz, so a direction error reaches x, y and the last leg of the path length 1 / cz^3 times.  On the 5-row lens at
    22 101 points three live rays leave the last row at cz^2 = 6e-6 (they land 0.5 .. 1.3 m off the axis) and the fp32
    oracle itself is 40 % off there, with every row's cos^2 above 0.004; elsewhere the factor is 1.00 .. 1.1."""
    cz2 = (1.0 - fwd64[2].double().square() - fwd64[3].double().square()).clamp(min=1e-30)
    return torch.where(fwd64[4], cz2.pow(-1.5), torch.ones_like(cz2))


def normal_amplification(theta64):
    """Per row, for theta / (pi/2) alone: max(1, NORMAL_SIN / sin theta).  theta = acos(u) turns an error of u into one
    1 / sin theta times as large, and an fp32 u near 1 carries a few units of 2^-24 whatever computes it: at NORMAL_SIN
    that is the tolerance of theta (4 x 2^-24 / (3e-6 pi/2) = 0.051, 2.9 degrees from the normal); at the oracle's clamp
    u <= 1 - 1e-7, theta = 4.5e-4 rad, it is 113 tolerances, and the fp32 oracle is 64 off there."""
    return (NORMAL_SIN / torch.sin(theta64.double() * (math.pi / 2))).clamp(min=1.0)


NORMAL_SIN = 4 * 2.0 ** -24 / (3e-6 * math.pi / 2)
IMAGE_OUTPUTS = ("x", "y", "opd")   # what the transfer to the image plane writes: A_i carries image_amplification


_REF = {}


def reference(name, P, S, variant, b=0):
    """fp32 (IEEE sqrt) and fp64 oracle runs of lens b of a case, with what the gates need from the fp64 one: alive,
    min_cos2, amp (A_i = 1 / min_cos2; amp_image = A_i cz^-3 for IMAGE_OUTPUTS), flags, near, died_at.  Cached; `free(name)` drops a shape's entries."""
    key = (name, P, S, variant, b)
    if key not in _REF:
        a = lens(name, P, S, variant)[b]
        res = dict(args=a, f32=oracle_run(a, torch.float32), f64=oracle_run(a, torch.float64))
        res["alive"], res["min_cos2"], res["flags"], res["near"] = conditioning(res["f64"]["stk"])
        res["amp"] = 1.0 / res["min_cos2"]
        res["amp_image"] = res["amp"] * image_amplification(res["f64"]["fwd"])
        res["died_at"] = died_at(res["f64"]["stk"])
        _REF[key] = res
    return _REF[key]


def free(name=None):
    for key in [k for k in _REF if name is None or k[0] == name]:
        del _REF[key]


# ------------------------------------------------------------------------------------------------------------------
# gates
# ------------------------------------------------------------------------------------------------------------------

def per_ray_outputs(run):
    """{output name: tensor} of one run (an oracle_run dictionary, or the kernels' outputs in the same form); the stacks
    and hits keep their leading row dimensions, which broadcast against the per-ray amplification."""
    out = dict(zip(("x", "y", "cx", "cy"), run["fwd"][:4]))
    if run.get("opd") is not None:
        out["opd"] = run["opd"]
    if run.get("stk") is not None:
        out["zrelu"], out["theta"], out["thetap"] = run["stk"][0], run["stk"][1], run["stk"][2]
    if run.get("hits") is not None:
        out["hits"] = run["hits"]
    return out


def ratios(run, ref, k=1.0, c=None, keep=None):
    """{output: largest |run - f64| / (c[output] k tol A_i)} (c None: 1) over the rays `keep` (default: alive in `run`
    and in the fp64 oracle).  The stacks are compared on every ray that passed as many rows alive in `run` as in the fp64
    oracle -- a ray that died on the way has live rows -- with A_i over its live rows; the hit points on the rays `keep`
    only (the walk-back reads no others)."""
    f64 = per_ray_outputs(ref["f64"])
    both = (run["fwd"][4] & ref["f64"]["fwd"][4]) if keep is None else keep
    same = (died_at(run["stk"]) == ref["died_at"]) if run.get("stk") is not None else None
    out = {}
    for n, g in per_ray_outputs(run).items():
        if n not in f64:
            continue
        sel = same if n in ("zrelu", "theta", "thetap") else both
        amp = ref["amp_image"] if n in IMAGE_OUTPUTS else ref["amp"]
        if n in ("theta", "thetap"):
            amp = amp * normal_amplification(f64[n])
        e = (g.double() - f64[n]).abs() / ((1.0 if c is None else c[n]) * k * TOL[n] * amp)
        e = torch.where(sel.expand(e.shape), e, torch.zeros_like(e))
        assert not torch.isnan(e).any(), n
        out[n] = float(e.max())
    return out


def rays_differing(run, ref):
    """Rays left out of a value comparison: `ok` differs from the fp64 oracle's, or (with stacks) the ray passed a
    different number of rows alive."""
    d = run["fwd"][4] != ref["f64"]["fwd"][4]
    if run.get("stk") is not None:
        d = d | (died_at(run["stk"]) != ref["died_at"])
    return int(d.sum())


def moments_of(x, y, ok, back, flags=None, stk=None):
    """The ten moment columns [B*F, 10] float64 as fp64 sums over (P, W) of the fp32 values given ([B,F,P,W]; stk
    [3,S,B,F,P,W]):  0 sum y | 1 sum ok y | 2 sum ok y^2 | 3 sum ok | 4..6 the same of x | 7 sum back | 8 sum q, q =
    (sum_k theta + sum_k theta') + sum_k z_RELU rebuilt in fp32 by sequential adds over k, NaN -> 0 (0 without stacks) |
    9 the count of flag 2 (0 without flags).  Also returns the bound n 2^-53 sum |terms| of any summation order."""
    B, F, P, W = y.shape
    okd = ok.double()
    cols, mags = [], []

    def put(v):
        cols.append(v.sum(dim=(2, 3)).reshape(-1))
        mags.append(v.abs().sum(dim=(2, 3)).reshape(-1))
    for q in (y, x):
        qd = q.double()
        put(qd), put(okd * qd), put(okd * qd * qd)
        if q is y:
            put(okd)
    put(back.double())
    if stk is not None:
        s = [torch.zeros_like(stk[0, 0]) for _ in range(3)]
        for k in range(stk.shape[1]):
            for j in range(3):
                s[j] = s[j] + stk[j, k]
        q = (s[1] + s[2]) + s[0]
        assert q.dtype == torch.float32
        put(torch.where(torch.isnan(q), torch.zeros_like(q), q).double())
    else:
        put(torch.zeros_like(okd))
    put((flags == 2).double() if flags is not None else torch.zeros_like(okd))
    m = torch.stack(cols, dim=1)
    bound = torch.stack(mags, dim=1) * (P * W * 2.0 ** -53)
    return m, bound


COUNTS, SUMS = (3, 7, 9), (0, 1, 2, 4, 5, 6, 8)


# ------------------------------------------------------------------------------------------------------------------
# the measurement behind C
# ------------------------------------------------------------------------------------------------------------------

def measure(cases=None, out=print):
    """The fp32 IEEE oracle against the fp64 one over the table: per case and lens the largest |o32 - o64| / (tol A_i) of
    every output, rays alive, backward, flag 2, near the threshold, left out.  Returns {output: largest ratio}."""
    worst, where = {}, {}
    for name, P, S, v in (cases or CASES):
        for b in range(SHAPES[name][0]):
            r = reference(name, P, S, v, b)
            rt = ratios(r["f32"], r)
            ok64 = r["f64"]["fwd"][4]
            for n, val in rt.items():
                if val > worst.get(n, 0.0):
                    worst[n], where[n] = val, (name, P, S, v, b)
            out(f"{name} P={P} S={S} {v} lens {b}: alive {int(ok64.sum())}/{ok64.numel()}, back {int(r['f64']['fwd'][5].sum())}, "
                f"flag2 {int((r['flags'] == 2).sum())}, near {int(r['near'].sum())}, left out {rays_differing(r['f32'], r)}, "
                f"back differs {int((r['f32']['fwd'][5] != r['f64']['fwd'][5]).sum())}, "
                f"image cz^2 < 0.01: {int((r['amp_image'] > 1e3 * r['amp']).sum())} | "
                + ", ".join(f"{k} {val:.3f}" for k, val in rt.items()))
        if name != "main":
            free(name)
    for n in worst:
        out(f"largest ratio of {n}: {worst[n]:.4f} at {where[n]}")
    return worst


if __name__ == "__main__":
    measure()
