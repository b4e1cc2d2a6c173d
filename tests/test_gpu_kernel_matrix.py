"""
Every backward kernel instantiation the build ships against the oracle's fp64 autograd (oracle.trace_skew_general,
aggregate=True).

Which kernel runs depends on the row count S, the pupil size P, aspheric rows, the penalty term, the arithmetic mode and
the backward algorithm (launch_bwd_inv / launch_bwd in csrc/tl_kernels.inc, routing in tl_trace_bwd_from_outputs):

  trace_bwd_inv_unrolled_kernel<NS, ASPH, PEN>   3 <= S <= 20 and P >= 256, one instantiation per row count; from
                                                 kInvUnrollPairMin (13) rows on the lanes of a pair share LDS slots
  trace_bwd_inv_kernel<ASPH> (rolled)            S = 1, 2, 21..32 or P < 256, no penalty term
  trace_bwd_kernel<bucket, ASPH, PEN>            'checkpoint'; the penalty term wherever the unrolled walk-back does
                                                 not run; the rays the walk-back leaves (dead under the penalty, flagged
                                                 grazing rays, more aspheric rows than hit slots)
  reduce_bwd_kernel                              the walk-back's (3S+3 | 8S+3 columns) and the checkpoint kernel's
                                                 (tl_bwd_row(bucket) columns) partials summed

The matrix: S in ROWS (every unrolled NS, both sides of every bucket / unroll / pair boundary, checked against the
sources by test_row_matrix_covers_every_instantiation_and_boundary, which needs no GPU) x {spherical, aspheric} x
{rms, rms + lam * sumQ} x {strict, fast} x {inverse, checkpoint} on a 3 x 3 x 777-ray fan overfilled (some rays die), a 200-point
pupil (P < 256: rolled walk-back, penalty on the checkpoint kernel) at S = 3, 12, 13, 20, two hit-slot edge cases and lens
batches of three.  Lenses: truncations / extensions of zoom20 (zoom20_rows.lens_args).

Each cell also asserts that ops.backward_route names the family listed above for it (_family; tl_bwd_route's own answer is
checked against it without a GPU).  The route is the launch, not every ray's path: test_gpu_backward_route.py found on the
device that trace_bwd_inv_kernel<true> flags a non-finite adjoint on every fan that holds a dead ray -- all of _fan's -- so the
aspheric rms cells of the rolled range here (S = 1, 2, 21..32, and P = 200) are launched on that kernel and differentiated by
the checkpoint kernel behind it.  The rolled aspheric walk-back itself is held to the oracle by that file's cells on the same
fans without their dead rays (ADVICE.md has the finding).

One oracle run per (lens, pupil) in fp32 (IEEE sqrt) and one in fp64, with two retained backward passes (rms, sumQ): the
reference for the penalty loss is g_rms + lam g_Q, lam = |g_rms(c)| / |g_Q(c)| in fp64 so that both terms carry
comparable gradient (sumQ grows with the ray count: ~1.3e3 on these fans against an rms of 1e-3..1).  Gates are against fp64 only;
`noise` is the oracle's own fp32-vs-fp64 distance.
"""
import os
import re

import numpy as np
import pytest
import torch

from conftest import rel_l2
from zoom20_rows import lens_args

DEV = "cuda:0"
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "torchoptics_amd", "csrc")

ROWS = tuple(range(1, 21)) + (21, 24, 25, 28, 32)
SMALL_ROWS = (3, 12, 13, 20)
P_MAIN, P_SMALL = 777, 200
FILL = 1.2                         # pupil radius / design aperture (plus a sprinkling of rays far outside: _fan)
REL_FIELDS = (0.3, 0.65, 1.0)      # 3 .. 10 degrees: off axis, see _fan
BATCH_ROWS = (13, 20)
BATCH_W = (0.5, 1.0, 1.5)          # per-lens loss weights of a lens batch
NEAR_NORMAL_RAD = 3e-3             # rays closer to a surface normal ...
GRAZING_RAD = 1e-2                 # ... or to grazing incidence than this are kept out of the fan (_fan)

# (S, variant, P): variant 'sph' | 'asph' (rows 0, middle, S-1) | 'asph8' (8 aspheric rows, 8 hit slots: the largest LDS
# request of the unrolled walk-back, 20 KB + 16 KB) | 'asph5' (5 aspheric rows, 4 hit slots: the device-side fallback)
LENSES = ([(S, v, P_MAIN) for S in ROWS for v in ("sph", "asph")]
          + [(S, v, P_SMALL) for S in SMALL_ROWS for v in ("sph", "asph")]
          + [(20, "asph8", P_MAIN), (16, "asph5", P_MAIN)])
HIT_SLOTS = {"asph8": 8}           # ops.ASPH_HIT_SLOTS otherwise (4)


def _asph_rows(S, variant):
    if variant == "sph":
        return []
    if variant == "asph8":
        return [0, 3, 6, 9, 12, 14, 17, S - 1]
    if variant == "asph5":
        return [0, 4, 8, 13, S - 1]
    # first, last and a middle row; from 15 rows on the middle one lies in the part of the lens past row 12
    mid = S // 2 if S < 15 else (13 + S - 1) // 2
    return sorted({0, mid, S - 1})


def _fan(S, variant, P, n_lens=1):
    """CPU tensors of one lens: kernel arguments with a random P-point pupil FILL x the entrance pupil, fields 3..10 deg
    (with the penalty term on the axis whole rings of rays sit on the reference's acos clamp at 1 - 1e-7, where two fp32
    evaluations legitimately disagree: test_gpu_fuzz.py), three wavelengths; aspheric coefficients when asked.
    `n_lens`: the fan is shared by that many lenses (_perturbed) of a batch."""
    import torchoptics_amd as ta
    from oracle import trace_oracle as orc
    from torchoptics_amd import prescriptions as PR
    a = lens_args(ta, S, n_rays=(4, 4), rel_fields=REL_FIELDS)
    epd = float(PR.zoom20("cpu", requires_grad=False)[1].epd.item())
    rng = np.random.default_rng(1000 * S + P)
    r = (np.sqrt(rng.random(P)) * (0.5 * epd * FILL)).astype(np.float32)
    th_p = (rng.random(P) * 2 * np.pi).astype(np.float32)
    rows = _asph_rows(S, variant)
    a["rows"] = rows
    if rows:
        kap = np.zeros(S, np.float32)
        pol = np.zeros((S, 4), np.float32)
        kap[rows] = rng.uniform(-0.5, 0.3, len(rows))
        pol[rows, 0] = rng.choice([-1.0, 1.0], len(rows)) * rng.uniform(1e-6, 1e-5, len(rows))
        pol[rows, 1] = rng.uniform(-1e-8, 1e-8, len(rows))
        a["kappa"], a["poly"] = torch.from_numpy(kap), torch.from_numpy(pol)
        a["kind"] = [1 if k in rows else 0 for k in range(S)]
    F, W = a["cy"].shape[1], a["mu"].shape[3]

    def put(rad):
        a["x"] = torch.from_numpy(rad * np.cos(th_p)).reshape(1, 1, P, 1).expand(1, F, P, W)
        a["y"] = torch.from_numpy(rad * np.sin(th_p)).reshape(1, 1, P, 1).expand(1, F, P, W)
    # The 1.2 x fan alone loses no ray on these lenses.  Every 16th point goes 5 x further out, where rays miss a row or
    # fail to refract on the way (2..5 % of the fan from 3 rows on): under the penalty term the checkpoint kernel queued
    # behind the walk-back takes those rays, and the reduction merges the two partial layouts.  An outer ray that gets
    # through does so at grazing angles, where fp32 evaluations of its gradient differ by per cent (it made the
    # oracle's own fp32-vs-fp64 distance 1e-2 on the 20-row lens): those points go back into the fan, as does every outer
    # point that a 0.1 % change of its radius would keep alive somewhere (fp64 oracle, every field, wavelength, lens).
    out = np.zeros(P, bool)
    out[::16] = True
    for scale in (0.999, 1.001, 1.0):
        put(np.where(out, r * np.float32(5.0 * scale), r).astype(np.float32))
        for b in range(n_lens):
            ab = _perturbed(a, b)
            kw = dict(kappa=ab["kappa"].double(), poly=ab["poly"].double(), kind=ab["kind"]) if rows else {}
            o = orc.trace_skew_general(*[ab[k].double() for k in ("x", "y", "z", "cx", "cy", "c", "t", "mu")], ab["mask"], **kw)
            out &= ~o[4].reshape(-1, P, W).any(dim=(0, 2)).numpy()
    rad = np.where(out, r * np.float32(5.0), r).astype(np.float32)
    # The penalty term's d theta / d cos^2 = -1 / (2 cos sin) is unbounded at both ends: within 3 mrad of a surface
    # normal the fp32 cosine near 1 is quantised to 6e-8 (test_gpu_penalty.py), and within 10 mrad of grazing one ray
    # carries a gradient 1 / cos larger than its neighbours'.  Any two fp32 evaluations then differ by per cent on that
    # ray: on the 20-row lens one outer ray at 3.8 mrad from grazing on row 5 (dead at row 9) held 40 % of d sumQ / d mu
    # and made the oracle's own fp32 2.3e-2 from its fp64, the kernels 4.5e-3 (d/dz) and 7.6e-3 (d/dc, fast).  Pupil
    # points with such a ray on a live row (fp64 oracle, every field, wavelength, lens) take the place of the first
    # point of the fan that has none.
    put(rad)
    near = np.zeros(P, bool)
    for b in range(n_lens):
        ab = _perturbed(a, b)
        kw = dict(kappa=ab["kappa"].double(), poly=ab["poly"].double(), kind=ab["kind"]) if rows else {}
        o = orc.trace_skew_general(*[ab[k].double() for k in ("x", "y", "z", "cx", "cy", "c", "t", "mu")], ab["mask"],
                                   aggregate=True, **kw)
        th = torch.stack(o[7]["theta_norm"] + o[7]["theta_prime_norm"]) * (np.pi / 2)      # [2S,1,F,P,W]; dead rows: pi/2
        bad = (th < NEAR_NORMAL_RAD) | ((th > np.pi / 2 - GRAZING_RAD) & (th < np.pi / 2))
        near |= bad.any(dim=0).reshape(-1, P, W).any(dim=(0, 2)).numpy()
    if near.any():
        j = int(np.flatnonzero(~near & ~out)[0])
        rad[near], th_p[near] = rad[j], th_p[j]
    put(rad)
    a["near_normal_moved"] = int(near.sum())
    return a


def _perturbed(a, b):
    """Lens b of a batch: curvatures (flat rows stay flat) and gaps of `a` perturbed by about 1 %."""
    if b == 0:
        return a
    rng = np.random.default_rng(77 + b)
    S = a["c"].shape[-1]
    out = dict(a)
    out["c"] = a["c"] * torch.from_numpy((1 + 0.01 * rng.standard_normal(S)).astype(np.float32))
    out["t"] = a["t"] * torch.from_numpy((1 + 0.01 * rng.random(S)).astype(np.float32))
    return out


_LEAVES = ("z", "cy", "c", "t", "mu")
_PER_RAY = ("z", "cy")
_ORACLE = {}


def _oracle(S, variant, P, b=None):
    """fp32 (IEEE sqrt) and fp64 oracle runs of one lens (lens b of the batch at S when b is not None): forward outputs,
    rms, sumQ and their gradients w.r.t. the launch / lens parameters.  Cached for the module."""
    key = (S, variant, P, b)
    if key in _ORACLE:
        return _ORACLE[key]
    from oracle import trace_oracle as orc
    a = _fan(S, variant, P, 1 if b is None else len(BATCH_W))
    if b is not None:
        a = _perturbed(a, b)
    names = _LEAVES + (("kappa", "poly") if a["rows"] else ())
    res = {}
    for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
        # z and cy per ray (broadcast to the fan): their gradients are kept ray by ray, see _grad_errors
        lv = {n: (a[n].to(dt).expand(a["x"].shape) if n in _PER_RAY else a[n].to(dt)).clone().requires_grad_(True)
              for n in names}
        kw = dict(kappa=lv["kappa"], poly=lv["poly"], kind=a["kind"]) if a["rows"] else {}
        o = orc.trace_skew_general(a["x"].to(dt), a["y"].to(dt), lv["z"], a["cx"].to(dt), lv["cy"], lv["c"], lv["t"],
                                   lv["mu"], a["mask"], ieee_sqrt=(dt == torch.float32), aggregate=True, **kw)
        rms = orc.compute_rms2d(o[0], o[1], o[4])
        q = orc.penalty_from_stacks(o[7], S)
        g_rms = torch.autograd.grad(rms, [lv[n] for n in names], retain_graph=True, allow_unused=True)
        g_q = torch.autograd.grad(q, [lv[n] for n in names], allow_unused=True)
        zero = lambda g, n: torch.zeros_like(lv[n]) if g is None else g         # noqa: E731
        res[tag] = dict(fwd=[t.detach() for t in o[:6]], rms=rms.item(), q=q.item(),
                        g_rms={n: zero(g, n).double() for n, g in zip(names, g_rms)},
                        g_q={n: zero(g, n).double() for n, g in zip(names, g_q)})
    # lam from the fp64 oracle (c is a lens leaf, not per ray)
    res["lam"] = float(res["f64"]["g_rms"]["c"].norm() / res["f64"]["g_q"]["c"].norm())
    res["args"] = a
    res["names"] = names
    _ORACLE[key] = res
    return res


@pytest.fixture(scope="module")
def ta():
    import torchoptics_amd
    from torchoptics_amd import _lib
    _lib.lib()
    return torchoptics_amd


def _run_gpu(ta, lenses, S, variant, pen, lam, mode, algo, weights=None):
    """The kernels on one lens (or a batch of them, stacked along dim 0): forward outputs, loss values, gradients."""
    from torchoptics_amd import ops, ray_tracing as rt
    a0 = lenses[0]
    B = len(lenses)
    names = _LEAVES + (("kappa", "poly") if a0["rows"] else ())
    per_lens = ("z", "c", "t")
    lv = {}
    for n in names:
        v = torch.cat([a[n] for a in lenses], 0) if (B > 1 and n in per_lens) else a0[n]
        lv[n] = v.to(DEV).clone().requires_grad_(True)
    kw = {}
    if a0["rows"]:
        kw = dict(kappa=lv["kappa"], poly=lv["poly"], surf_kind=torch.tensor(a0["kind"], dtype=torch.bool, device=DEV))
    ops.set_backward_algorithm(algo)
    ops.set_asph_hit_slots(HIT_SLOTS.get(variant, 4))
    try:
        out = ta.trace_skew(a0["x"].to(DEV), a0["y"].to(DEV), lv["z"], a0["cx"].to(DEV), lv["cy"], lv["c"], lv["t"], lv["mu"],
                            a0["mask"].to(DEV), True if pen else False, True, mode=mode, **kw)
        inv, route = ops.used_walk_back(out[0]), ops.backward_route(out[0])
        if B > 1:
            if pen:
                ld = rt.unsupervised_loss_batch(out, S, lam)
                rms, q = ld["rms"], ld["penalty"]
                loss = ld["loss_unsup"]
            else:
                rms = loss = rt.compute_rms2d_batch(out[0], out[1], out[4])
                q = None
            (loss * torch.tensor(weights, device=DEV)).sum().backward()
        else:
            rms = ta.compute_rms2d(out[0], out[1], out[4])
            q = rt.penalty_sum(out[6], S) if pen else None
            (rms + lam * q if pen else rms).backward()
    finally:
        ops.set_backward_algorithm("inverse")
        ops.set_asph_hit_slots(4)
    return dict(fwd=[t.detach().cpu() for t in out[:6]], inv=inv, route=route,
                rms=rms.detach().cpu().double().reshape(-1), q=None if q is None else q.detach().cpu().double().reshape(-1),
                grads={n: lv[n].grad.detach().cpu().double() for n in names})


def _check_forward(tag, got, o32, o64, exact, k):
    """Forward outputs of one lens: bit-equal to the fp32 IEEE oracle (`exact`), else the gate of
    test_gpu_asphere.test_asphere_forward_matches_oracle (fast mode x k)."""
    if exact:
        for name, g_, w_ in zip(("x", "y", "cx", "cy", "ok", "back"), got, o32):
            assert torch.equal(g_, w_), f"{tag}: {name} not bit-exact"
        return
    ok_g, ok_w, ok_32 = got[4], o64[4], o32[4]
    differ = (ok_g != ok_w).sum().item()
    assert differ <= 2 + (ok_32 != ok_w).sum().item(), f"{tag}: ok masks differ on {differ} of {ok_w.numel()} rays"
    assert (got[5] != o32[5]).sum().item() <= 2 + (o32[5] != o64[5]).sum().item(), f"{tag}: backward-ray flags"
    both = ok_g & ok_w & ok_32
    for i, tol in ((0, 2e-5), (1, 2e-5), (2, 2e-6), (3, 2e-6)):
        d = (got[i].double() - o64[i])[both].abs().max().item()
        noise = (o32[i].double() - o64[i])[both].abs().max().item()
        assert d <= tol * k + 2 * noise, f"{tag}: forward output {i}: {d:.2e} (oracle fp32 itself {noise:.2e})"
    assert not got[0][~ok_g].any(), f"{tag}: dead rays not parked"


def _gate(n, pen, noise, k, cancel=1.0):
    """Gradient bound vs fp64.  rms: test_gpu_asphere.py (lens 2e-5, launch conditions max(3 noise, 3e-5)); with the
    penalty: test_gpu_penalty.py (1e-4, 2e-3); fast mode x 10; + 2 x the oracle's own fp32-vs-fp64 distance.
    `cancel` (penalty loss only): (|g_rms| + |lam g_Q|) / |g_rms + lam g_Q| of this parameter in the fp64 oracle.  Each
    term is held to its own relative bound, so where the two cancel (d/dkappa of the 19-row aspheric lens: |sum| is
    1/156 of either term) the bound on the sum grows by that factor; it is 1.0..1.6 for most parameters."""
    if n in _PER_RAY:
        base = 2e-3 if pen else max(3 * noise, 3e-5)
    else:
        base = 1e-4 if pen else 2e-5
    return base * k * (cancel if pen else 1.0) + 2 * noise


def _reduce(n, g, like):
    """A per-ray launch-condition gradient summed to the shape of the kernel's (z [..1,1,1], cy [1,F,1,1])."""
    return g.sum(dim=(2, 3), keepdim=True).sum(dim=1, keepdim=True) if n == "z" else g.sum(dim=(2, 3), keepdim=True)


def _grad_errors(tag, got, r32, r64, pen, k, rows, S, cancel=None):
    """Per parameter: e64 vs the fp64 oracle, the oracle's own noise, and the hard gate.

    z (the reference is per ray): `noise` is the oracle's fp32-vs-fp64 distance summed ray by ray without
    cancellation, sum_rays |g32 - g64| / |sum_rays g64|, when that is larger than the distance of the sums.  d/dz is a
    sum over the fan of terms of both signs: in focus (zoom20, 20 rows and more) d rms / dz is 1e-6 against
    per-ray terms of 1e-3..1e-2, so every fp32 evaluation carries the per-ray rounding of its own operation order
    into the sum, and the oracle's autograd happening to round the same way as its fp64 twin is no bound for another
    order (the walk-back, which rebuilds each ray from the image plane, measured 1.1e-3..2.2e-3 there, the checkpoint
    kernel 6e-5, the oracle's summed noise 1e-4, its per-ray noise 1.1e-3..1.4e-3)."""
    msg = []
    for n, g in got.items():
        assert torch.isfinite(g).all(), f"{tag}: d/d{n} not finite"
        w32, w64 = r32[n], r64[n]
        if n in _PER_RAY:
            d = (w32 - w64).abs()
            w32, w64 = _reduce(n, w32, g), _reduce(n, w64, g)
            e64, noise = rel_l2(g.numpy(), w64.numpy()), rel_l2(w32.numpy(), w64.numpy())
            if n == "z":
                noise = max(noise, float(_reduce(n, d, g).norm() / w64.norm()))
        else:
            e64, noise = rel_l2(g.numpy(), w64.numpy()), rel_l2(w32.numpy(), w64.numpy())
        cn = 1.0 if cancel is None else cancel[n]
        msg.append(f"{n} {e64:.1e}/{noise:.1e}" + (f"/x{cn:.1f}" if cn > 1.05 else ""))
        assert e64 <= _gate(n, pen, noise, k, cn), \
            f"{tag} d/d{n}: vs fp64 {e64:.2e}, oracle fp32 itself {noise:.2e}, cancellation x{cn:.1f}"
        if n in ("kappa", "poly"):
            flat = [j for j in range(S) if j not in rows]
            assert g.reshape(S, -1)[flat].abs().max().item() == 0 if flat else True, f"{tag}: d/d{n} of a spherical row"
    return msg


def _cancel(parts):
    """(|a| + |b|) / |a + b| per parameter from fp64 (a, b) pairs, per-ray references summed first."""
    out = {}
    for n, (a, b) in parts.items():
        if n in _PER_RAY:
            a, b = _reduce(n, a, None), _reduce(n, b, None)
        out[n] = float((a.norm() + b.norm()) / max((a + b).norm(), 1e-300))
    return out


def _ref_grad(r, pen, lam, w=1.0):
    return {n: w * (r["g_rms"][n] + lam * r["g_q"][n] if pen else r["g_rms"][n]) for n in r["g_rms"]}


def _parts(r, lam, w=1.0):
    return {n: (w * r["g_rms"][n], w * lam * r["g_q"][n]) for n in r["g_rms"]}


def _check_losses(tag, got_rms, got_q, r, pen, k):
    r32, r64 = r["f32"], r["f64"]
    # rms: 5e-6 relative (test_gpu_penalty.py) + 2 x the oracle's own fp32-vs-fp64 distance (the fp32 spot of a long
    # lens carries the rounding of every row's positions)
    assert abs(got_rms - r64["rms"]) <= 5e-6 * k * r64["rms"] + 2 * abs(r32["rms"] - r64["rms"]), \
        f"{tag}: rms {got_rms!r} vs fp64 {r64['rms']!r} (fp32 oracle {r32['rms']!r})"
    if pen:
        assert abs(got_q - r64["q"]) <= 3e-6 * k * abs(r64["q"]) + 2 * abs(r32["q"] - r64["q"]), \
            f"{tag}: sumQ {got_q!r} vs fp64 {r64['q']!r} (fp32 oracle {r32['q']!r})"


_MODES = ("strict", "fast")
_ALGOS = ("inverse", "checkpoint")


def _family(S, P, pen, algo):
    """The kernel family the module docstring lists for a cell, in the words of ops.backward_route.  Every variant of the
    matrix stores its aspheric hits (4 or 8 slots), 'asph5' included: its launch is the unrolled walk-back, which hands the
    lens to the checkpoint kernel on the device."""
    if algo == "checkpoint":
        return "checkpoint"
    if 3 <= S <= 20 and P >= 256:
        return "walk_unrolled"
    return "checkpoint" if pen else "walk_rolled"


@pytest.mark.gpu
@pytest.mark.parametrize("algo", _ALGOS)
@pytest.mark.parametrize("mode", _MODES)
@pytest.mark.parametrize("loss", ("rms", "pen"))
@pytest.mark.parametrize("S,variant,P", LENSES, ids=[f"S{s}-{v}-P{p}" for s, v, p in LENSES])
def test_backward_instantiation_matches_fp64_oracle(ta, S, variant, P, loss, mode, algo):
    if loss == "pen" and S > 31:
        # the penalty term's per-ray row bits are a 32-bit word with one bit spare (tl_api.hip, check_problem)
        a = _fan(S, variant, P)
        with pytest.raises(RuntimeError, match="aggregate needs S <= 31"):
            _run_gpu(ta, [a], S, variant, True, 1.0, mode, algo)
        return
    r = _oracle(S, variant, P)
    a = r["args"]
    pen, k = loss == "pen", (10.0 if mode == "fast" else 1.0)
    lam = r["lam"] if pen else 0.0
    ok32 = r["f32"]["fwd"][4]
    assert ok32.float().mean().item() > 0.5
    assert S < 3 or not ok32.all(), "no dead rays: the walk-back + checkpoint merge is not reached"
    got = _run_gpu(ta, [a], S, variant, pen, lam, mode, algo)
    tag = f"S={S} {variant} P={P} {loss} {mode} {algo}"
    assert got["inv"] is (algo == "inverse"), tag
    assert got["route"] == _family(S, P, pen, algo), (tag, got["route"])
    _check_forward(tag, got["fwd"], r["f32"]["fwd"], r["f64"]["fwd"], exact=(variant == "sph" and mode == "strict"), k=k)
    _check_losses(tag, got["rms"].item(), None if got["q"] is None else got["q"].item(), r, pen, k)
    msg = _grad_errors(tag, got["grads"], _ref_grad(r["f32"], pen, lam), _ref_grad(r["f64"], pen, lam), pen, k,
                       a["rows"], S, _cancel(_parts(r["f64"], lam)) if pen else None)
    print(f"{tag}: live {int(ok32.sum())}/{ok32.numel()}, lam {lam:.3g} | e64/noise " + ", ".join(msg))


@pytest.mark.gpu
@pytest.mark.parametrize("algo", _ALGOS)
@pytest.mark.parametrize("mode", _MODES)
@pytest.mark.parametrize("loss", ("rms", "pen"))
@pytest.mark.parametrize("variant", ("sph", "asph"))
@pytest.mark.parametrize("S", BATCH_ROWS)
def test_lens_batch_matches_fp64_oracle_per_lens(ta, S, variant, loss, mode, algo):
    """B = 3 perturbed copies in one launch, weighted per-lens losses: the gradients of the per-lens parameters (z, c, t)
    against each lens's own oracle run, the shared ones (cy, mu, kappa, poly) against the weighted sum."""
    rs = [_oracle(S, variant, P_MAIN, b) for b in range(len(BATCH_W))]
    pen, k = loss == "pen", (10.0 if mode == "fast" else 1.0)
    lam = rs[0]["lam"] if pen else 0.0
    got = _run_gpu(ta, [r["args"] for r in rs], S, variant, pen, lam, mode, algo, weights=BATCH_W)
    tag = f"batch S={S} {variant} {loss} {mode} {algo}"
    assert got["inv"] is (algo == "inverse"), tag
    assert got["route"] == _family(S, P_MAIN, pen, algo), (tag, got["route"])
    msg = []
    shared = {}
    for b, (r, w) in enumerate(zip(rs, BATCH_W)):
        tb = f"{tag} lens {b}"
        _check_forward(tb, [t[b:b + 1] for t in got["fwd"]], r["f32"]["fwd"], r["f64"]["fwd"],
                       exact=(variant == "sph" and mode == "strict"), k=k)
        _check_losses(tb, got["rms"][b].item(), None if got["q"] is None else got["q"][b].item(), r, pen, k)
        ref32, ref64 = _ref_grad(r["f32"], pen, lam, w), _ref_grad(r["f64"], pen, lam, w)
        mine = {n: got["grads"][n][b:b + 1] for n in ("z", "c", "t")}
        parts = _parts(r["f64"], lam, w)
        msg += [f"{b}:" + m for m in _grad_errors(tb, mine, ref32, ref64, pen, k, r["args"]["rows"], S,
                                                  _cancel(parts) if pen else None)]
        for n in ref32:
            if n not in mine:
                acc = shared.setdefault(n, [0.0, 0.0, 0.0, 0.0])
                acc[0], acc[1] = acc[0] + ref32[n], acc[1] + ref64[n]
                acc[2], acc[3] = acc[2] + parts[n][0], acc[3] + parts[n][1]
    rest = {n: got["grads"][n] for n in shared}
    msg += _grad_errors(tag, rest, {n: v[0] for n, v in shared.items()}, {n: v[1] for n, v in shared.items()}, pen, k,
                        rs[0]["args"]["rows"], S, _cancel({n: (v[2], v[3]) for n, v in shared.items()}) if pen else None)
    print(f"{tag}: lam {lam:.3g} | e64/noise " + ", ".join(msg))


# ------------------------------------------------------------------------------------------------------------------
# CPU guard: the matrix covers what the sources instantiate
# ------------------------------------------------------------------------------------------------------------------

def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _instantiated():
    """(unrolled NS list of the release build, bucket table, TL_INVU_MIN, TL_INVU_MAX, kInvUnrollPairMin) from the sources."""
    kin, com = _read("tl_kernels.inc"), _read("tl_common.h")
    m = re.search(r"#ifdef TL_INVU_DEV.*?#else(.*?)#endif", kin, re.S)
    assert m, "the TL_INVU_DEV / release switch of launch_bwd_inv is gone"
    invu = sorted(int(n) for n in re.findall(r"TL_INVU\((\d+)\)", m.group(1)))
    b = re.search(r"tl_bwd_bucket\(int S\)\s*\{[^}]*?\{([\d,\s]+)\}", com, re.S)
    buckets = [int(v) for v in b.group(1).split(",")]
    lo = int(re.search(r"#define TL_INVU_MIN (\d+)", com).group(1))
    hi = int(re.search(r"#define TL_INVU_MAX (\d+)", com).group(1))
    pair = int(re.search(r"kInvUnrollPairMin = (\d+)", kin).group(1))
    return invu, buckets, lo, hi, pair


def test_row_matrix_covers_every_instantiation_and_boundary():
    invu, buckets, lo, hi, pair = _instantiated()
    assert invu == list(range(lo, hi + 1)), f"unrolled instantiations {invu} vs TL_INVU_MIN..MAX {lo}..{hi}"
    rows = set(ROWS)
    missing = [n for n in invu if n not in rows]
    assert not missing, f"unrolled walk-back instantiations never tested: NS = {missing}"
    # both sides of every boundary: checkpoint buckets (S = v and v + 1), the unrolled range, the lane-pair threshold
    edges = {1}
    for v in buckets:
        edges |= {v, v + 1}
    edges |= {lo - 1, lo, hi, hi + 1, pair - 1, pair}
    edges = {e for e in edges if 1 <= e <= max(buckets)}
    missing = sorted(edges - rows)
    assert not missing, f"row counts at a bucket / unroll / pair boundary not in the matrix: {missing}"
    # the small pupil (P < 256: rolled walk-back, penalty on the checkpoint kernel) on both sides of the unrolled range
    # and of the pair threshold
    small = {s for s, _, p in LENSES if p < 256}
    assert {lo, pair - 1, pair, hi} <= small, small
    assert all(p >= 256 and p % 256 for s, _, p in LENSES if p not in (P_SMALL,))
    # every lens of the matrix has aspheric variants too, and the middle aspheric row of a paired lens lies past row 12
    for S in ROWS:
        rows_a = _asph_rows(S, "asph")
        assert 0 in rows_a and S - 1 in rows_a and len(rows_a) <= 4
        if S >= pair + 2:
            assert any(pair <= j < S - 1 for j in rows_a), (S, rows_a)
    assert len(_asph_rows(20, "asph8")) == 8 and len(_asph_rows(16, "asph5")) == 5
    # the kernel family each cell asserts (_family) is tl_bwd_route's answer for the problem the host chains build there,
    # and every family of the docstring is reached with and without the penalty term where it exists
    import ctypes as C
    from torchoptics_amd import _lib, ops
    reached = set()
    for S, variant, P in LENSES:
        for pen in (False, True):
            if pen and S > 31:
                continue
            p = _lib.tl_problem()
            p.F, p.W, p.S, p.P, p.aggregate = 3, 3, S, P, int(pen)
            if variant != "sph":
                p.surf_kind = p.kappa = p.poly = p.asph_hits = 8            # (addresses: never followed)
                p.asph_hit_slots = min(HIT_SLOTS.get(variant, 4), S)
            assert ops.BACKWARD_ROUTES[_lib.lib().tl_bwd_route(C.byref(p))] == _family(S, P, pen, "inverse"), (S, variant, P, pen)
            reached.add((_family(S, P, pen, "inverse"), pen))
    assert reached == {("walk_unrolled", False), ("walk_unrolled", True), ("walk_rolled", False), ("checkpoint", True)}
