"""
Case table and fp64 reference of the optical-path-length (OPD) matrix: tests/test_opd_cases_cpu.py states on the CPU when
the reference is fit to judge, tests/test_gpu_opd_matrix.py holds the kernels to it.  No GPU import here.

What runs with an OPD seed (csrc/tl_kernels.inc): trace_fwd_kernel<false, ASPH, true> forwards, and backwards the
checkpoint kernel trace_bwd_kernel<NS, ASPH, kPenNone> of the bucket NS = tl_bwd_bucket(S) with its per-wave sums
sgn[NS+1][kWaves], written to columns NB .. NB+NS of its partial rows and summed by reduce_bwd_kernel into g_n[w][k].

Lenses and fans are those of test_gpu_kernel_matrix (_fan: zoom20 truncations, 3 fields x 3 wavelengths, a pupil 1.2 x the
entrance pupil with every 16th point 5 x further out, so every fan loses rays); n_index [1,1,1,W,S+1] follows from mu.

  ROWS         both sides of every bucket boundary of tl_bwd_bucket, S < NS and S == NS in every bucket
  variants     'sph' | 'asph' (aspheric rows first, middle, last: _asph_rows)
  pupils       777 (three chunks and a 9-lane tail) everywhere; at S = 4, 13 also 200 (less than a block), 64 (one full
               wave, three past the end) and 63
  lens batch   B = 3 at S = 5, 13: c, t perturbed (_perturbed), every index but object space scaled by 1 +- 1e-3 in lenses
               1 and 2 and mu recomputed from it, so a wrong lens offset into n_index or g_n_index shows

Losses (each in fp32 with the IEEE sqrt and in fp64, from oracle.trace_skew_general(..., n_index=...)):
  path         sum(w OPD), w a seeded weight per ray in [0, 1e-3), of both signs in half the cases: the OPD seed alone
  path+rms     path + compute_rms2d: the OPD seed and the spot seed in one adjoint
  wavefront    mean over (field, wavelength) of the variance of OPD over the fan's live rays (`wavefront`, plain torch):
               its seeds sum to zero per fan, so every gradient is a cancelling sum over rays

The fp64 run carries every leaf per ray, so the reference knows each ray's term of every gradient: its sum is the
reference gradient, `cancel` = |sum_rays |term|| / |sum_rays term| (norms over the leaf) the cancellation factor the
wavefront gates carry, and `abs_n` = sum_rays |term| of d/d n_index entry by entry.
"""
import torch

from test_gpu_kernel_matrix import _PER_RAY, _asph_rows, _fan, _perturbed   # noqa: F401  (_asph_rows: re-exported)

ROWS = (1, 2, 4, 5, 8, 9, 12, 13, 16, 17, 20, 21, 24, 25, 32)
VARIANTS = ("sph", "asph")
P_MAIN = 777
SMALL_P = (200, 64, 63)
SMALL_ROWS = (4, 13)
BATCH_ROWS = (5, 13)
BATCH_W = (0.5, 1.0, 1.5)                     # per-lens loss weights of a lens batch
BATCH_N_SCALE = (0.0, +1e-3, -1e-3)           # lens b: every index but object space times 1 + BATCH_N_SCALE[b]
LOSSES = ("path", "path+rms", "wavefront")
CANCEL_CAP = 200.0                            # wavefront: largest cancellation factor a case may carry
# _fan puts an outer point back into the fan when it survives anywhere (in any lens of a batch): see _more_dead_rays
MORE_OUT = {(2, "asph", P_MAIN, False): (8, 7.0)}     # (S, variant, P, lens batch): (first of every 16th point, factor)
HOST_CHAIN_CASES = ((5, "sph", P_MAIN), (13, "asph", P_MAIN))

CASES = ([(S, v, P_MAIN) for S in ROWS for v in VARIANTS]
         + [(S, v, P) for S in SMALL_ROWS for v in VARIANTS for P in SMALL_P])
BATCH_CASES = [(S, v) for S in BATCH_ROWS for v in VARIANTS]
LEAVES = ("z", "cy", "c", "t", "mu", "n_index")


def case_id(case):
    return "S%d-%s-P%d" % case


def n_of_mu(mu):
    """[.,1,1,W,S+1] refractive indices from the index ratios mu_k = n_k / n_{k+1}, n_0 = 1 (object space)."""
    n = [torch.ones_like(mu[..., 0])]
    for k in range(mu.shape[-1]):
        n.append(n[-1] / mu[..., k])
    return torch.stack(n, dim=-1)


def mu_of_n(n):
    return n[..., :-1] / n[..., 1:]


def signed_weights(S, variant):
    """Half the cases weigh the OPD with both signs."""
    return (S % 2 == 1) != (variant == "asph")


def path_weights(S, variant, P, shape, b=None):
    g = torch.Generator().manual_seed(7919 * S + 31 * P + (1 if variant == "asph" else 0) + 1009 * (0 if b is None else b + 1))
    w = torch.rand(shape, generator=g, dtype=torch.float64) * 1e-3
    if signed_weights(S, variant):
        w = w * (torch.randint(0, 2, shape, generator=g).double() * 2 - 1)
    return w.float()                            # the fp32 values every run uses


def wavefront(opd, ok):
    """[B]: per lens the mean over (field, wavelength) of the variance of OPD [B,F,P,W] over the fan's live rays.  Formed
    in fp64 from whatever precision the OPD comes in, so the seeds are exact functions of the OPD values given."""
    o, m = opd.double(), ok.double()
    n = m.sum(dim=2, keepdim=True)
    mean = (o * m).sum(dim=2, keepdim=True) / n
    var = (m * (o - mean) ** 2).sum(dim=2, keepdim=True) / n
    return var.mean(dim=(1, 2, 3))


def _dies_everywhere(lenses, cand, factor):
    """Which of the pupil points `cand`, sent `factor` x further out, die on every field, wavelength and lens -- also with
    0.1 % more or less of that radius (the rule of _fan: an outer ray that gets through does so at grazing angles, where
    any two fp32 evaluations of its gradient differ by per cent)."""
    from oracle import trace_oracle as orc
    P = lenses[0]["x"].shape[2]
    dead = torch.ones(len(cand), dtype=torch.bool)
    for scale in (0.999, 1.001, 1.0):
        s = torch.ones(P, dtype=torch.float64)
        s[cand] = factor * scale
        for a in lenses:
            x, y = ((a[n][:, :1, :, :1].double() * s.reshape(1, 1, P, 1)).expand(a[n].shape) for n in ("x", "y"))
            kw = dict(kappa=a["kappa"].double(), poly=a["poly"].double(), kind=a["kind"]) if a["rows"] else {}
            o = orc.trace_skew_general(x, y, *[a[k].double() for k in ("z", "cx", "cy", "c", "t", "mu")], a["mask"], **kw)
            dead &= ~o[4].any(dim=3).any(dim=1).any(dim=0)[cand]
    return dead


def _more_dead_rays(lenses, S, variant, P, batch):
    """Send further pupil points out where _fan leaves too few dead rays for this matrix.
    * The two-row aspheric lens lets most rays 5 x out through (0.9 % of the fan dead): there the every-16th points from
      8 go 7 x out (MORE_OUT) -- those of them that die everywhere.
    * P = 777 has one every-16th point in its ragged last chunk, 768, and on some fans _fan has put it back: then the
      last point of the chunk that dies everywhere 5 x (else 7 x, 10 x) out goes there, so that the 9-lane tail holds a
      dead ray.  One point: the dead fraction hardly moves."""
    from oracle import trace_oracle as orc
    scale = torch.ones(P)
    if (S, variant, P, batch) in MORE_OUT:
        first, factor = MORE_OUT[(S, variant, P, batch)]
        cand = torch.arange(first, P, 16)
        scale[cand[_dies_everywhere(lenses, cand, factor)]] = factor
    tail = (P // 256) * 256
    if P == P_MAIN:
        a = lenses[0]
        kw = dict(kappa=a["kappa"].double(), poly=a["poly"].double(), kind=a["kind"]) if a["rows"] else {}
        x, y = ((a[n][:, :1, :, :1].double() * scale.double().reshape(1, 1, P, 1)).expand(a[n].shape) for n in ("x", "y"))
        ok = orc.trace_skew_general(x, y, *[a[k].double() for k in ("z", "cx", "cy", "c", "t", "mu")], a["mask"], **kw)[4]
        if ok[:, :, tail:].all():
            cand = torch.arange(P - 1, tail, -1)
            for factor in (5.0, 7.0, 10.0):
                dies = _dies_everywhere(lenses, cand, factor)
                if dies.any():
                    scale[cand[dies][0]] = factor
                    break
    if (scale != 1).any():
        for a in lenses:
            for n in ("x", "y"):
                a[n] = (a[n][:, :1, :, :1] * scale.reshape(1, 1, P, 1)).expand(a[n].shape)


_LENSES = {}


def _lenses(S, variant, P, batch):
    """The lens of a case, or the three of a lens batch (one fan for all): CPU kernel arguments with n_index."""
    key = (S, variant, P, batch)
    if key in _LENSES:
        return _LENSES[key]
    a0 = _fan(S, variant, P, len(BATCH_W) if batch else 1)
    out = []
    for b in range(len(BATCH_W) if batch else 1):
        a = dict(_perturbed(a0, b))
        n = n_of_mu(a["mu"].double())
        if b:
            n = torch.cat((n[..., :1], n[..., 1:] * (1.0 + BATCH_N_SCALE[b])), dim=-1)
        a["n_index"] = n.float()
        a["mu"] = mu_of_n(a["n_index"].double()).float()
        out.append(a)
    _more_dead_rays(out, S, variant, P, batch)
    _LENSES[key] = out
    return out


def lens_case(S, variant, P, b=None):
    """CPU kernel arguments of one lens (lens b of the batch at S when b is not None) with n_index and the path weights."""
    a = dict(_lenses(S, variant, P, b is not None)[b or 0])
    a["w"] = path_weights(S, variant, P, a["x"].shape, b)
    return a


def leaf_names(a):
    return LEAVES + (("kappa", "poly") if a["rows"] else ())


def _to_leaf(n, g, like):
    """A per-ray gradient [..] summed over the rays to the shape of the leaf `like` (z and cy stay per ray)."""
    if n in _PER_RAY:
        return g
    if n in ("kappa", "poly"):
        return g.reshape(*like.shape, -1).sum(dim=-1)
    dims = tuple(i for i in range(like.dim()) if like.shape[i] == 1 and g.shape[i] != 1)
    return g.sum(dim=dims, keepdim=True) if dims else g


def gate_cancel(r, loss, n):
    """The cancellation factor the gate of (loss, leaf) carries: the wavefront loss's own, capped (test_opd_cases_cpu.py)."""
    return min(r["cancel"][loss][n], CANCEL_CAP) if loss == "wavefront" else 1.0


_REF = {}


def reference(S, variant, P, b=None):
    """fp32 (IEEE sqrt) and fp64 oracle runs of one case, cached: forward outputs, the three losses' gradients per leaf
    (z and cy per ray, as test_gpu_kernel_matrix keeps them), and from fp64 the per-ray bound scale of the forward OPD
    `path` = sum_k |n_k d_k| + |n_S d_image|, the cancellation factors and `abs_n`."""
    key = (S, variant, P, b)
    if key in _REF:
        return _REF[key]
    from oracle import trace_oracle as orc
    a = lens_case(S, variant, P, b)
    names = leaf_names(a)
    shape = a["x"].shape                                                  # [1,F,P,W]
    res = {"args": a, "names": names}
    for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
        per_ray = dt == torch.float64
        lv = {}
        for n in names:
            v = a[n].to(dt)
            if n in _PER_RAY:
                v = v.expand(shape)
            elif per_ray and n in ("kappa", "poly"):
                v = v.reshape(*v.shape, 1, 1, 1, 1).expand(*v.shape, *shape)
            elif per_ray:
                v = v.expand(*shape, v.shape[-1])
            lv[n] = v.clone().requires_grad_(True)
        kw = dict(kappa=lv["kappa"], poly=lv["poly"], kind=a["kind"]) if a["rows"] else {}
        o = orc.trace_skew_general(a["x"].to(dt), a["y"].to(dt), lv["z"], a["cx"].to(dt), lv["cy"], lv["c"], lv["t"],
                                   lv["mu"], a["mask"], n_index=lv["n_index"], ieee_sqrt=(dt == torch.float32), **kw)
        opd, ok = o[6], o[4]
        path = (opd * a["w"].to(dt)).sum()
        losses = {"path": path, "path+rms": path + orc.compute_rms2d(o[0], o[1], ok), "wavefront": wavefront(opd, ok)[0]}
        out = dict(fwd=[t.detach() for t in o[:7]], loss={k: float(v.detach()) for k, v in losses.items()}, grads={})
        leaves = [lv[n] for n in names]
        if per_ray:
            res["cancel"], res["abs_n"] = {}, {}
            (d_k,) = torch.autograd.grad(opd.sum(), [lv["n_index"]], retain_graph=True)      # per ray and row: d_k, d_image
            res["path"] = (d_k * lv["n_index"].detach()).abs().sum(dim=-1)
        for name, loss in losses.items():
            gs = torch.autograd.grad(loss, leaves, retain_graph=True, allow_unused=True)
            gs = [torch.zeros_like(q) if g is None else g for g, q in zip(gs, leaves)]
            out["grads"][name] = {n: _to_leaf(n, g.double(), a[n]) for n, g in zip(names, gs)}
            if per_ray:
                tot = {n: _to_leaf(n, g.abs(), a[n]) for n, g in zip(names, gs)}
                res["cancel"][name] = {}
                for n in names:
                    s, t_ = out["grads"][name][n], tot[n]
                    if n in _PER_RAY:                                     # the kernel's leaf: one z, one cy per field
                        dims = (1, 2, 3) if n == "z" else (2, 3)
                        s, t_ = s.sum(dim=dims), t_.sum(dim=dims)
                    res["cancel"][name][n] = float(t_.norm() / max(float(s.norm()), 1e-300))
                res["abs_n"][name] = tot["n_index"]
        res[tag] = out
    _REF[key] = res
    return res
