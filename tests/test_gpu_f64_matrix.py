"""
The double-precision trace kernels (tl_trace_fwd_f64 / tl_trace_bwd_f64, csrc/tl_f64.hip) against the oracle's
trace_skew_general in float64 on the CPU, over the launch shapes, layouts and edges that tests/test_gpu_f64.py does not
reach.  These kernels are the judge of the fp32 gradients at fan sizes the CPU oracle cannot take (bench.py --full), so
their own indexing has to be pinned: lens batches (every per-lens offset of lens_view and reduce_kernel), ragged pupils
(idle lanes in the wave and block sums), the gradient of cx (the cz0 fold and the skipped g_cz column), 1..32 rows, more
than one chunk per block, strided / broadcast fans, output selection and the refusals of the C entry points.

Tolerances are those of test_gpu_f64.py: per-ray outputs within 1e-11 mm, `ok` / `back` equal, gradients rel_l2 < 1e-9,
scalars (rms, moment sums) within 1e-10 relative, counts exact.  No ray is left out of a comparison.

The loss, the same on both sides, per lens b:

    w_b rms_b  +  sum_rays (x Wx + y Wy + cx Wcx + cy Wcy)  +  sum_fields Wm . (moments 0, 1, 2, 4, 5, 6)

compute_rms2d seeds the y-moments 0..2, the dense weights seed every per-ray output, the linear term seeds the x-moments
4..6 as well (and makes a ray-additive loss for the chunk test).  At P = 1 and 2 the rms term is left out: the spot of a field
is then one or two points (times W wavelengths), its variance 0 or ~1e-6 mm^2, where sqrt has no derivative (both sides
return NaN) and the closed form on the moments, M2 - 2 m M1 + m^2 M3, has lost eps y^2 / var of its digits: the moments are
seeded by the linear term alone there.  cx is a few degrees of azimuth in every case, so d/dcx and the fold of the cz0
adjoint carry signal.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import rel_l2

DEV = "cuda:0"
gpu = pytest.mark.gpu

P_LIST = (1, 2, 63, 64, 65, 255, 256, 257, 300, 1000)
# one seed per case of the sweep; lens and pupil size come from the position in the table (every P_LIST entry appears at
# least twice, with different lenses), everything else from the seed.  test_f64_case_table_covers_the_edges holds the table
# to what it is meant to cover.
SEEDS = tuple(range(100, 124))
OUT_TOL, GRAD_TOL, SUM_TOL = 1e-11, 1e-9, 1e-10
ILL_COS2 = 0.01                    # moments entry 9 counts live rays with a squared cosine below this on some row (tl_f64.hip)


@pytest.fixture(scope="module")
def ta():
    import torchoptics_amd
    from torchoptics_amd import _lib
    _lib.lib()
    return torchoptics_amd


# ------------------------------------------------------------------------------------------------------------------
# cases: dicts of float64 CPU tensors in trace_skew's shapes
# ------------------------------------------------------------------------------------------------------------------

def _mu_rows(d, W, scale=1.0):
    """mu [W,S] = n_before / n_after per row, mildly dispersive (as test_gpu_fuzz._case)."""
    nd = iter(d["nd"])
    n_rows = np.array([next(nd) * scale if ch == "G" else 1.0 for ch in d["sequence"][0]])
    lam = np.linspace(-1.0, 1.0, W) if W > 1 else np.zeros(1)
    n = 1.0 + (n_rows[None, :] - 1.0) * (1.0 + 0.01 * lam[:, None])
    n = np.concatenate([np.ones((W, 1)), n], axis=1)
    return n[:, :-1] / n[:, 1:]


def _weights(k, seed):
    """Fixed seeds of the loss: four dense [B,F,P,W] weights, moment weights [B*F,7] (the count has none), lens weights."""
    gen = torch.Generator().manual_seed(seed)
    B, F, P, W = k["B"], k["F"], k["P"], k["W"]
    k["wts"] = [torch.randn(B, F, P, W, generator=gen, dtype=torch.float64) * 1e-3 for _ in range(4)]
    k["wm"] = torch.randn(B * F, 7, generator=gen, dtype=torch.float64) * 1e-3
    k["wm"][:, 3] = 0.0
    k["wl"] = torch.linspace(0.5, 1.5, B, dtype=torch.float64) if B > 1 else torch.ones(1, dtype=torch.float64)
    return k


def _case(idx, seed=None, B=None, F=None, W=None, P=None, name=None, asph=None, fill=None, dense=None):
    """Case `idx` of the sweep (test_gpu_fuzz._case in float64, with what the fp64 kernels index per lens made per lens)."""
    import yaml_free_lenses as L
    seed = SEEDS[idx] if seed is None else seed
    rng = np.random.default_rng(seed)
    name = name or ("doublet", "cooke", "tessar")[idx % 3]
    d = L.PRESCRIPTIONS[name]
    S = len(d["c"])
    draw = dict(B=int(rng.integers(1, 5)), F=int(rng.integers(1, 5)), W=int(rng.choice([1, 3])), fill=float(rng.uniform(0.6, 1.6)),
                asph=bool(rng.integers(0, 2)), allow=bool(rng.integers(0, 2)), per_lens_dir=bool(rng.integers(0, 2)),
                dense=bool(rng.integers(0, 2)), per_lens_mu=bool(rng.integers(0, 2)), per_lens_asph=bool(rng.integers(0, 2)))
    B, F, W = B or draw["B"], F or draw["F"], W or draw["W"]
    P = P or P_LIST[idx % len(P_LIST)]
    asph = draw["asph"] if asph is None else asph
    fill = draw["fill"] if fill is None else fill
    dense = draw["dense"] if dense is None else dense
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))      # noqa: E731
    c = np.array(d["c"])[None, :] * (1 + 0.03 * rng.standard_normal((B, S)))
    t = np.array(d["t"])[None, :] * (1 + 0.03 * rng.random((B, S)))
    c[:, d["stop_idx"][0]] = 0.0
    if draw["per_lens_mu"] and B > 1:
        mu = np.stack([_mu_rows(d, W, 1 + 0.005 * rng.standard_normal()) for _ in range(B)]).reshape(B, 1, 1, W, S)
    else:
        mu = _mu_rows(d, W).reshape(1, 1, 1, W, S)
    # sequence mask: gates the backward-ray test of the row after; lenses past the first drop two rows each
    mask = np.ones((B, S), bool)
    for b in range(1, B):
        mask[b, rng.choice(S, 2, replace=False)] = False
    r = np.sqrt(rng.random(P)) * (0.5 * L.EPD * fill)
    th = rng.random(P) * 2 * np.pi
    x, y = (r * np.cos(th)).reshape(1, 1, P, 1), (r * np.sin(th)).reshape(1, 1, P, 1)
    if dense:           # a fan per (lens, field, wavelength), as ray aiming makes
        x = x * (1 + 1e-3 * rng.standard_normal((B, F, 1, W)))
        y = y * (1 + 1e-3 * rng.standard_normal((B, F, 1, W)))
    # field directions from 2 deg to 0.5 .. 1.3 x the half field of view (test_gpu_fuzz._case), turned out of the
    # meridional plane by a few degrees
    fld = np.sin(np.deg2rad(np.linspace(2.0, L.HFOV_DEG * float(rng.uniform(0.5, 1.3)), F)))
    az = np.deg2rad(rng.uniform(3.0, 12.0))
    nb = B if (draw["per_lens_dir"] and B > 1) else 1
    jit = 1 + 0.02 * rng.standard_normal((nb, 1))
    cx, cy = (fld[None, :] * np.sin(az) * jit).reshape(nb, F, 1, 1), (fld[None, :] * np.cos(az) * jit).reshape(nb, F, 1, 1)
    z = rng.uniform(2.0, 6.0, B).reshape(B, 1, 1, 1)
    k = dict(idx=idx, seed=seed, name=name, B=B, F=F, W=W, P=P, S=S, fill=fill, asph=asph, allow=draw["allow"], dense=dense,
             rms=P >= 63, x=T(x), y=T(y), z=T(z), cx=T(cx), cy=T(cy), c=T(c.reshape(B, 1, 1, 1, S)), t=T(t.reshape(B, 1, 1, 1, S)),
             mu=T(mu), mask=torch.from_numpy(mask.reshape(B, 1, 1, 1, S)), kappa=None, poly=None, kind=None)
    if asph:
        na = B if (draw["per_lens_asph"] and B > 1) else 1
        kap, pol = np.zeros((na, S)), np.zeros((na, S, 4))
        rows = [0, S - 1]
        kap[:, rows] = rng.uniform(-0.8, 0.4, (na, 2))
        pol[:, rows, 0] = rng.uniform(-3e-5, 3e-5, (na, 2))
        pol[:, rows, 1] = rng.uniform(-3e-7, 3e-7, (na, 2))
        kind = np.zeros(S, bool)
        kind[rows] = True
        k.update(kappa=T(kap if na > 1 else kap[0]), poly=T(pol if na > 1 else pol[0]), kind=torch.from_numpy(kind))
    return _weights(k, seed)


def _sub(k, sel):
    """The same case on the pupil points `sel` (a slice): the fan and the dense weights are cut, nothing else."""
    out = dict(k)
    out["x"], out["y"] = k["x"][:, :, sel], k["y"][:, :, sel]
    out["wts"] = [w[:, :, sel] for w in k["wts"]]
    out["P"] = out["x"].shape[2]
    return out


def _names(k, x_in=True):
    return (("x", "y") if x_in else ()) + ("z", "cx", "cy", "c", "t", "mu") + (("kappa", "poly") if k["asph"] else ())


def _lens(a, b):
    """Lens b of an argument that is given per lens, or the argument itself when all lenses share it."""
    return a[b:b + 1] if a.shape[0] > 1 else a


def _moment_loss(x, y, ok):
    """Moments 0..6 of one lens, [F,7], differentiable: sum y, sum ok y, sum ok y^2, sum ok, then the same three of x."""
    okd = ok.to(y.dtype)
    three = lambda q: [q.sum(dim=(2, 3))[0], (okd * q).sum(dim=(2, 3))[0], (okd * q * q).sum(dim=(2, 3))[0]]   # noqa: E731
    return torch.stack(three(y) + [okd.sum(dim=(2, 3))[0]] + three(x), dim=1)


# ------------------------------------------------------------------------------------------------------------------
# the two sides
# ------------------------------------------------------------------------------------------------------------------

def _oracle_run(k, x_in=True):
    """The oracle lens by lens (as test_gpu_batch.py): per-lens outputs [1,F,P,W], rms, the ten moments, gradients of the
    one loss (arguments shared by the lenses collect their sum through autograd)."""
    from oracle import trace_oracle as orc
    B, F, P, W = k["B"], k["F"], k["P"], k["W"]
    names = _names(k, x_in)
    lv = {n: k[n].clone().requires_grad_(True) for n in names}
    get = lambda n: lv.get(n, k[n])      # noqa: E731
    loss, fwd, rms, moments, near = 0.0, [], [], [], 0
    for b in range(B):
        extra = ()
        if k["asph"]:
            kap, pol = get("kappa"), get("poly")
            extra = (kap[b] if kap.dim() == 2 else kap, pol[b] if pol.dim() == 3 else pol, [int(v) for v in k["kind"]])
        o = orc.trace_skew_general(*[_lens(get(n), b) for n in ("x", "y", "z", "cx", "cy", "c", "t", "mu")], _lens(k["mask"], b),
                                   *extra, allow_backward_rays=k["allow"], aggregate=True)
        x, y, cx, cy, ok, back = [q.expand(1, F, P, W) for q in o[:6]]
        m = _moment_loss(x, y, ok)
        loss = loss + (k["wm"][b * F:(b + 1) * F] * m).sum()
        loss = loss + sum((q * w[b:b + 1]).sum() for q, w in zip((x, y, cx, cy), k["wts"]))
        if k["rms"]:
            r_b = orc.compute_rms2d(x, y, ok)
            loss = loss + k["wl"][b] * r_b
            rms.append(r_b.item())
        # entry 9: rays alive behind the last row (its theta is 1 for a dead ray) with a grazing row somewhere
        th = torch.stack(o[7]["theta_norm"] + o[7]["theta_prime_norm"]).detach()
        alive = (o[7]["theta_norm"][-1].detach() != 1.0).expand(1, F, P, W)
        cos2 = torch.cos(th * (np.pi / 2)).square().amin(dim=0).expand(1, F, P, W)
        near += int((alive & ((cos2 - ILL_COS2).abs() < 1e-9)).sum())
        ill = (alive & (cos2 < ILL_COS2)).double().sum(dim=(2, 3))[0]
        md = m.detach()
        moments.append(torch.cat((md, back.double().sum(dim=(2, 3))[0][:, None], torch.zeros(F, 1, dtype=torch.float64),
                                  ill[:, None]), dim=1))
        fwd.append([q.detach() for q in (x, y, cx, cy, ok, back)])
    loss.backward()
    ok_all = torch.cat([f[4] for f in fwd])
    return dict(fwd=fwd, rms=rms, moments=torch.cat(moments), grads={n: lv[n].grad for n in names},
                live=float(ok_all.double().mean()), dead=int((~ok_all).sum()), back=int(sum(f[5].sum() for f in fwd)),
                near_ill=near)


_ORACLE = {}


def _sweep_oracle(idx):
    if idx not in _ORACLE:
        k = _case(idx)
        _ORACLE[idx] = (k, _oracle_run(k))
    return _ORACLE[idx]


def _moments_of(y):
    return y._tl_spot[0]


def _kernel_run(ta, k, x_in=True, keep_on_device=False):
    """The fp64 kernels on the whole batch in one launch each way, same loss."""
    from torchoptics_amd import ray_tracing as rt
    B, F = k["B"], k["F"]
    names = _names(k, x_in)
    lv = {n: k[n].to(DEV).clone().requires_grad_(True) for n in names}
    get = lambda n: lv[n] if n in lv else k[n].to(DEV)      # noqa: E731
    kw = dict(kappa=lv["kappa"], poly=lv["poly"], surf_kind=k["kind"].to(DEV)) if k["asph"] else {}
    out = ta.trace_skew(*[get(n) for n in ("x", "y", "z", "cx", "cy", "c", "t", "mu")], k["mask"].to(DEV), False, k["allow"], **kw)
    assert all(q.dtype == torch.float64 for q in out[:4])
    mom = _moments_of(out[1])
    loss = (k["wm"].to(DEV) * mom[:, :7]).sum() + sum((q * w.to(DEV)).sum() for q, w in zip(out[:4], k["wts"]))
    rms = None
    if k["rms"]:
        if B == 1:
            rms = ta.compute_rms2d(out[0], out[1], out[4]).reshape(1)
        else:
            rms = rt.compute_rms2d_batch(out[0], out[1], out[4])
        assert rms.dtype == torch.float64
        loss = loss + (rms * k["wl"].to(DEV)).sum()
    loss.backward()
    put = (lambda q: q.detach()) if keep_on_device else (lambda q: q.detach().cpu())
    return dict(fwd=[put(q) for q in out[:6]], rms=None if rms is None else rms.detach().cpu(), moments=put(mom),
                grads={n: put(lv[n].grad) for n in names})


def _compare(tag, k, got, want):
    """Everything the kernels return against the oracle, lens by lens."""
    B, F = k["B"], k["F"]
    for b in range(B):
        g, w = [q[b:b + 1] for q in got["fwd"]], want["fwd"][b]
        # (a mask that differs on a ray within rounding of a 1e-6 threshold would be a reason to replace the seed, not to
        #  mask the ray; none of the seeds in use has one)
        assert torch.equal(g[4], w[4]), f"{tag} lens {b}: ok differs on {int((g[4] != w[4]).sum())} rays"
        assert torch.equal(g[5], w[5]), f"{tag} lens {b}: back differs on {int((g[5] != w[5]).sum())} rays"
        for i, n in enumerate(("x", "y", "cx", "cy")):
            e = (g[i] - w[i]).abs().max().item()
            assert e < OUT_TOL, f"{tag} lens {b}: {n} off by {e:.2e}"
    gm, wm = got["moments"], want["moments"]
    assert gm.shape == wm.shape == (B * F, 10)
    for j in (3, 7, 9):
        assert torch.equal(gm[:, j], wm[:, j]), f"{tag}: count in moments entry {j}: {gm[:, j].tolist()} vs {wm[:, j].tolist()}"
    assert not gm[:, 8].any(), f"{tag}: moments entry 8"
    for j in (0, 1, 2, 4, 5, 6):
        bad = (gm[:, j] - wm[:, j]).abs() > SUM_TOL * wm[:, j].abs()
        assert not bad.any(), f"{tag}: moments entry {j}: {gm[:, j].tolist()} vs {wm[:, j].tolist()}"
    if k["rms"]:
        for b in range(B):
            assert abs(got["rms"][b].item() - want["rms"][b]) <= SUM_TOL * abs(want["rms"][b]), \
                f"{tag} lens {b}: rms {got['rms'][b].item()!r} vs {want['rms'][b]!r}"
    errs = []
    for n, w in want["grads"].items():
        g = got["grads"][n]
        assert g.shape == w.shape and torch.isfinite(g).all(), (tag, n)
        assert w.abs().max().item() > 0, f"{tag}: the loss leaves d/d{n} trivial"
        e = rel_l2(g.numpy(), w.numpy())
        errs.append(f"{n} {e:.1e}")
        assert e < GRAD_TOL, f"{tag} d/d{n}: {e:.2e}"
        if w.shape[0] == B and B > 1:          # given per lens: each lens against its own rays (a small lens is not hidden)
            for b in range(B):
                e = rel_l2(g[b].numpy(), w[b].numpy())
                assert e < GRAD_TOL, f"{tag} d/d{n} of lens {b}: {e:.2e}"
        if n in ("kappa", "poly"):
            rows = g.reshape(-1, k["S"]) if n == "kappa" else g.reshape(-1, k["S"], 4)
            assert not rows[:, ~k["kind"]].any(), f"{tag}: d/d{n} of a spherical row"
    return errs


def _tag(k):
    return (f"case {k['idx']} seed {k['seed']}: {k['name']} B={k['B']} F={k['F']} W={k['W']} P={k['P']} fill={k['fill']:.2f} "
            f"asph={k['asph']} allow_back={k['allow']} dense={k['dense']}")


# ------------------------------------------------------------------------------------------------------------------
# 1. launch-shape sweep
# ------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("idx", range(len(SEEDS)))
def test_launch_shape_sweep_matches_the_fp64_oracle(ta, idx):
    k, want = _sweep_oracle(idx)
    got = _kernel_run(ta, k)
    errs = _compare(_tag(k), k, got, want)
    print(_tag(k) + f"; live {want['live']:.2f}, {want['back']} backward | " + ", ".join(errs))


# ------------------------------------------------------------------------------------------------------------------
# 2. row counts
# ------------------------------------------------------------------------------------------------------------------

ROW_COUNTS = (1, 2, 3, 20, 21, 31, 32)
P_ROWS = 257


def _asph_rows(S):
    """First, last and a middle row (test_gpu_kernel_matrix._asph_rows): at S = 32 the last row is aspheric."""
    mid = S // 2 if S < 15 else (13 + S - 1) // 2
    return sorted({0, mid, S - 1})


def _zoom_case(ta, S, asph, seed=None):
    """The first S rows of zoom20, or zoom20 and more rows behind it (zoom20_rows.lens_args), F = W = 2, a 257-point pupil
    1.2 x the design aperture.  The rows past 20 are thin weak glass menisci here, not flat air gaps: a flat air/air row
    bends no ray and would leave the last columns of the backward's accumulators zero whatever index they are written at."""
    from oracle import trace_oracle as orc
    from torchoptics_amd import prescriptions as PR
    from zoom20_rows import lens_args
    a = lens_args(ta, S, n_rays=(4, 4), rel_fields=(0.3, 0.8))
    epd = float(PR.zoom20("cpu", requires_grad=False)[1].epd.item())
    seed = 5000 + S if seed is None else seed
    rng = np.random.default_rng(seed)
    F, W, P = 2, 2, P_ROWS
    c, t, mu = a["c"].double().clone(), a["t"].double().clone(), a["mu"].double()[:, :, :, :W].clone()
    for j in range(20, S):
        c[..., j] = 0.004 * (-1.0) ** j
        mu[..., j] = 1 / 1.52 if (j - 20) % 2 == 0 else 1.52
    r = np.sqrt(rng.random(P)) * (0.5 * epd * 1.2)
    far = np.zeros(P, bool)
    far[::16] = True                   # (the 1.2 x fan alone loses no ray on these lenses: every 16th point goes 5 x further out)
    th = rng.random(P) * 2 * np.pi
    T = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64))      # noqa: E731
    s_f = a["cy"].double().reshape(-1)                       # sin(field angle), in the meridional plane
    az = np.deg2rad(7.0)
    k = dict(idx=f"S{S}", seed=seed, name="zoom20", B=1, F=F, W=W, P=P, S=S, fill=1.2, asph=asph, allow=True, dense=False, rms=True,
             x=None, y=None, z=a["z"].double().reshape(1, 1, 1, 1),
             cx=(s_f * np.sin(az)).reshape(1, F, 1, 1), cy=(s_f * np.cos(az)).reshape(1, F, 1, 1), c=c, t=t, mu=mu,
             mask=a["mask"].clone(), kappa=None, poly=None, kind=None)
    def put(far):
        rad = np.where(far, 5.0 * r, r)
        k["x"], k["y"] = T(rad * np.cos(th)).reshape(1, 1, P, 1), T(rad * np.sin(th)).reshape(1, 1, P, 1)
    if asph:
        rows = _asph_rows(S)
        kap, pol = np.zeros(S), np.zeros((S, 4))
        kap[rows] = rng.uniform(-0.5, 0.3, len(rows))
        pol[rows, 0] = rng.choice([-1.0, 1.0], len(rows)) * rng.uniform(1e-6, 1e-5, len(rows))
        pol[rows, 1] = rng.uniform(-1e-8, 1e-8, len(rows))
        kind = np.zeros(S, bool)
        kind[rows] = True
        k.update(kappa=T(kap), poly=T(pol), kind=torch.from_numpy(kind))
    # a far point that gets through somewhere does so at grazing angles, with a gradient orders of magnitude above the
    # fan's (test_gpu_kernel_matrix._fan): those go back into the fan
    put(far)
    extra = (k["kappa"], k["poly"], [int(v) for v in k["kind"]]) if asph else ()
    o = orc.trace_skew_general(*[k[n] for n in ("x", "y", "z", "cx", "cy", "c", "t", "mu")], k["mask"], *extra)
    put(far & ~o[4].expand(1, F, P, W).any(dim=3).any(dim=1)[0].numpy())
    return _weights(k, seed)


@gpu
@pytest.mark.parametrize("asph", (False, True), ids=("sph", "asph"))
@pytest.mark.parametrize("S", ROW_COUNTS)
def test_row_counts_match_the_fp64_oracle(ta, S, asph):
    k = _zoom_case(ta, S, asph)
    if asph:
        assert bool(k["kind"][S - 1]) and bool(k["kind"][0])
    want = _oracle_run(k)
    assert want["live"] > 0.5 and want["dead"] > 0
    got = _kernel_run(ta, k)
    errs = _compare(f"S={S} asph={asph}", k, got, want)
    if asph and S == 32:                        # the last element of the backward's accumulators carries signal
        assert want["grads"]["poly"][S - 1, 3].abs().item() > 0 and want["grads"]["kappa"][S - 1].abs().item() > 0
    print(f"S={S} asph={asph}: live {want['live']:.2f} | " + ", ".join(errs))


PAD_AT = (2, 3, 7)                  # identity rows of the 8-row padded lens: two in the middle, one at the end


def _padded(k):
    """`k` (5 rows) with identity rows (c = 0, t = 0, mu = 1, mask 0) at PAD_AT."""
    S = k["S"] + len(PAD_AT)
    keep = [j for j in range(S) if j not in PAD_AT]
    out = dict(k)
    out["S"] = S
    for n, fill in (("c", 0.0), ("t", 0.0), ("mu", 1.0)):
        v = torch.full((*k[n].shape[:-1], S), fill, dtype=torch.float64)
        v[..., keep] = k[n]
        out[n] = v
    m = torch.zeros((*k["mask"].shape[:-1], S), dtype=torch.bool)
    m[..., keep] = k["mask"]
    out["mask"] = m
    return out, keep


def _pad_case():
    return _case(0, seed=901, B=2, F=2, W=3, P=257, name="doublet", asph=False, fill=1.3, dense=False)


@gpu
def test_identity_padding_rows_match_the_fp64_oracle(ta):
    """A padded lens (identity rows in the middle and at the end, as in a batch of lenses of different length) against the
    oracle on the same padded rows, and against the un-padded lens: outputs within 1e-11 mm, masks equal, the gradients of
    the real rows within 1e-9, d/dc of an identity row zero to rounding (it bends no ray; its t and mu are ordinary
    parameters with an ordinary gradient, which the oracle comparison covers)."""
    k = _pad_case()
    kp, keep = _padded(k)
    got_p = _kernel_run(ta, kp)
    _compare("padded", kp, got_p, _oracle_run(kp))
    got = _kernel_run(ta, k)
    for i in range(4):
        assert (got_p["fwd"][i] - got["fwd"][i]).abs().max().item() < OUT_TOL, i
    assert torch.equal(got_p["fwd"][4], got["fwd"][4]) and torch.equal(got_p["fwd"][5], got["fwd"][5])
    assert not got["fwd"][4].all() and got["fwd"][4].double().mean() > 0.5
    for n in ("c", "mu"):
        assert rel_l2(got_p["grads"][n][..., keep].numpy(), got["grads"][n].numpy()) < GRAD_TOL, n
    for n in ("x", "y", "z", "cx", "cy"):
        assert rel_l2(got_p["grads"][n].numpy(), got["grads"][n].numpy()) < GRAD_TOL, n
    g_c = got_p["grads"]["c"]
    assert g_c[..., list(PAD_AT)].abs().max().item() <= 1e-12 * g_c.abs().max().item()


@gpu
def test_identity_padding_rows_leave_outputs_bit_equal_and_take_no_gradient(ta):
    """The padded lens gives the un-padded lens's outputs bit for bit, and exactly zero d/dc on the identity rows: the
    kernels run an identity row's tests (the flags are the oracle's) but leave the ray where it is, so the rows behind it
    start from the state they start from in the un-padded lens.  (The oracle moves the ray to the row's vertex plane and
    its padded and un-padded runs differ by 3.6e-15 mm, its d/dc of such a row is 3e-17; the kernels did the same before
    they passed such rows through.)  t and mu of an identity row are ordinary parameters with an ordinary gradient -- 0.2
    and 6 here against 2.7e2 for d/dc of the real rows -- which test_identity_padding_rows_match_the_fp64_oracle holds to
    the oracle's."""
    k = _pad_case()
    kp, keep = _padded(k)
    got_p, got = _kernel_run(ta, kp), _kernel_run(ta, k)
    worst = max((got_p["fwd"][i] - got["fwd"][i]).abs().max().item() for i in range(4))
    g_pad = got_p["grads"]["c"][..., list(PAD_AT)].abs().max().item()
    print(f"padded vs un-padded: outputs differ by at most {worst:.3e} mm, |d/dc| of identity rows at most {g_pad:.3e}")
    for i in range(6):
        assert torch.equal(got_p["fwd"][i], got["fwd"][i]), f"output {i}: {worst:.3e}"
    assert g_pad == 0.0


# ------------------------------------------------------------------------------------------------------------------
# 3. more than one chunk per block
# ------------------------------------------------------------------------------------------------------------------

P_BIG = 22101                       # 87 chunks of 256 points, the last one ragged (85 points)
SUB_STEP = 97                       # the oracle takes every 97th pupil point


def _nbx(B, F, W, S, P):
    """Blocks per (lens, field, wavelength) row of the fp64 launches, from tl_workspace_bytes_f64 =
    rows * nbx * (8 S + 3) * 8 + 256 (the backward's partials; the forward's 10 columns are fewer)."""
    from torchoptics_amd import _lib
    p = _lib.tl_problem()
    p.B, p.F, p.W, p.S, p.P = B, F, W, S, P
    nbytes = _lib.lib().tl_workspace_bytes_f64(C.byref(p))
    q, rem = divmod(nbytes - 256, B * F * W * (8 * S + 3) * 8)
    assert rem == 0 and q >= 1, (nbytes, q, rem)
    return q


@gpu
def test_more_than_one_chunk_per_block(ta):
    """B = 4, F = 4, W = 3, P = 22 101: 1.06 M rays, 87 chunks over fewer blocks (44 under today's plan: a block takes one
    or two, an uneven share, so a block's first chunk is not its index times its count), with the accumulators carried
    across chunks (every use of these kernels as a judge does; no other fp64 test does).
    (a) against the same kernels on two halves of the pupil, each at one chunk per block -- the shape the sweep holds to the
    oracle: per-ray outputs and d/dx_in, d/dy_in bit-equal, parameter gradients and moments equal to the sum of the halves
    to 1e-12 (the loss is ray-additive: dense weights and fixed moment weights, no rms);
    (b) against the oracle on every 97th pupil point: per-ray outputs and d/dx_in to the sweep's tolerances."""
    k = _case(1, seed=777, B=4, F=4, W=3, P=P_BIG, name="cooke", asph=True, fill=1.3, dense=True)
    k["rms"] = False
    B, F, W, S, P = k["B"], k["F"], k["W"], k["S"], k["P"]
    chunks = -(-P // 256)
    nbx = _nbx(B, F, W, S, P)
    assert chunks > nbx, "the launch plan gives this shape one chunk per block: the test no longer covers R >= 2"
    assert chunks % nbx, "every block has the same number of chunks: choose P so that the share is uneven"
    cuts = (0, 11008, P)                      # 43 and 44 chunks
    for p0, p1 in zip(cuts, cuts[1:]):
        assert -(-(p1 - p0) // 256) == _nbx(B, F, W, S, p1 - p0), "a half is no longer at one chunk per block"
    full = _kernel_run(ta, k, keep_on_device=True)
    assert 0.2 < full["fwd"][4].double().mean().item() < 1.0
    halves = [_kernel_run(ta, _sub(k, slice(p0, p1)), keep_on_device=True) for p0, p1 in zip(cuts, cuts[1:])]
    for i in range(6):
        assert torch.equal(full["fwd"][i], torch.cat([h["fwd"][i] for h in halves], dim=2)), f"output {i}"
    for n in ("x", "y"):
        assert torch.equal(full["grads"][n], torch.cat([h["grads"][n] for h in halves], dim=2)), f"d/d{n}_in"
    for n in _names(k, x_in=False):
        s = halves[0]["grads"][n] + halves[1]["grads"][n]
        e = rel_l2(full["grads"][n].cpu().numpy(), s.cpu().numpy())
        assert e < 1e-12, f"d/d{n}: {e:.2e}"
        assert s.abs().max().item() > 0
    ms = (halves[0]["moments"] + halves[1]["moments"]).cpu()
    mf = full["moments"].cpu()
    for j in (3, 7, 8, 9):
        assert torch.equal(mf[:, j], ms[:, j]), j
    for j in (0, 1, 2, 4, 5, 6):
        assert not ((mf[:, j] - ms[:, j]).abs() > 1e-12 * ms[:, j].abs()).any(), j
    # (b)
    sel = slice(0, None, SUB_STEP)
    ks = _sub(k, sel)
    want = _oracle_run(ks)
    for b in range(B):
        g = [q[b:b + 1, :, sel].cpu() for q in full["fwd"]]
        w = want["fwd"][b]
        assert torch.equal(g[4], w[4]) and torch.equal(g[5], w[5]), b
        for i in range(4):
            assert (g[i] - w[i]).abs().max().item() < OUT_TOL, (b, i)
        for n in ("x", "y"):
            e = rel_l2(full["grads"][n][b, :, sel].cpu().numpy(), want["grads"][n][b].numpy())
            assert e < GRAD_TOL, f"d/d{n}_in of lens {b}: {e:.2e}"


# ------------------------------------------------------------------------------------------------------------------
# 4. layouts and output selection
# ------------------------------------------------------------------------------------------------------------------

def _layout_case():
    return _case(1, seed=4242, B=2, F=2, W=3, P=300, name="cooke", asph=True, fill=1.2, dense=False)


def _same(a, b):
    for i in range(6):
        assert torch.equal(a["fwd"][i], b["fwd"][i]), f"output {i}"
    assert torch.equal(a["moments"], b["moments"])
    if a["rms"] is not None:
        assert torch.equal(a["rms"], b["rms"])


@gpu
def test_broadcast_fan_equals_the_dense_fan(ta):
    """x / y [1,1,P,1] (strides 0 over lens, field, wavelength) against the same values written out [B,F,P,W]: same
    arithmetic, so outputs, moments and parameter gradients are bit-equal; d/dx_in of the broadcast fan is the sum over
    (b, f, w) of the dense one (formed by autograd: 1e-12)."""
    k = _layout_case()
    kd = dict(k)
    kd["x"], kd["y"] = (k[n].expand(k["B"], k["F"], k["P"], k["W"]).contiguous() for n in ("x", "y"))
    a, b = _kernel_run(ta, k), _kernel_run(ta, kd)
    _same(a, b)
    for n in _names(k, x_in=False):
        assert torch.equal(a["grads"][n], b["grads"][n]), n
    for n in ("x", "y"):
        s = b["grads"][n].sum(dim=(0, 1, 3), keepdim=True)
        assert rel_l2(a["grads"][n].numpy(), s.numpy()) < 1e-12, n


@gpu
def test_dense_fan_per_row_equals_each_row_traced_alone(ta):
    """A different fan per (lens, field, wavelength), as ray aiming makes: every row of the batched launch equals that row
    traced alone (B = F = W = 1, its own fan), bit for bit, outputs and d/dx_in."""
    k = _case(1, seed=4243, B=2, F=2, W=3, P=300, name="cooke", asph=True, fill=1.2, dense=True)
    k["rms"] = False
    assert k["x"].shape == (2, 2, 300, 3)
    got = _kernel_run(ta, k)
    kap, pol = k["kappa"], k["poly"]
    for b in range(2):
        for f in range(2):
            for w in range(3):
                one = dict(k, B=1, F=1, W=1)
                for n in ("x", "y"):
                    one[n] = k[n][b:b + 1, f:f + 1, :, w:w + 1]
                for n in ("z", "c", "t", "mask"):
                    one[n] = _lens(k[n], b)
                one["mu"] = _lens(k["mu"], b)[:, :, :, w:w + 1]
                for n in ("cx", "cy"):
                    one[n] = _lens(k[n], b)[:, f:f + 1]
                one["kappa"], one["poly"] = (kap[b] if kap.dim() == 2 else kap), (pol[b] if pol.dim() == 3 else pol)
                one["wts"] = [q[b:b + 1, f:f + 1, :, w:w + 1] for q in k["wts"]]
                one["wm"] = k["wm"][b * 2 + f:b * 2 + f + 1]
                r = _kernel_run(ta, one)
                for i in range(6):
                    assert torch.equal(r["fwd"][i], got["fwd"][i][b:b + 1, f:f + 1, :, w:w + 1]), (b, f, w, i)
                for n in ("x", "y"):
                    assert torch.equal(r["grads"][n], got["grads"][n][b:b + 1, f:f + 1, :, w:w + 1]), (b, f, w, n)


@gpu
def test_non_contiguous_fan_with_odd_strides(ta):
    """The fan as a view into a larger buffer (strides 3 and 5 elements, an offset): equal to the contiguous copy bit for
    bit, the gradient lands in the view's elements and nowhere else."""
    k = _case(1, seed=4243, B=2, F=2, W=3, P=300, name="cooke", asph=True, fill=1.2, dense=True)
    B, F, P, W = 2, 2, 300, 3
    want = _kernel_run(ta, k)
    names = _names(k, x_in=False)
    base = {n: torch.zeros(B, F + 1, 3 * P + 1, W + 2, dtype=torch.float64, device=DEV) for n in ("x", "y")}
    cut = (slice(None), slice(0, F), slice(1, None, 3), slice(1, W + 1))
    for n in ("x", "y"):
        base[n][cut] = k[n].to(DEV)
        base[n].requires_grad_(True)
    views = {n: base[n][cut] for n in ("x", "y")}
    assert views["x"].stride() == ((F + 1) * (3 * P + 1) * (W + 2), (3 * P + 1) * (W + 2), 3 * (W + 2), 1) and not views["x"].is_contiguous()
    lv = {n: k[n].to(DEV).clone().requires_grad_(True) for n in names}
    out = ta.trace_skew(views["x"], views["y"], *[lv[n] for n in ("z", "cx", "cy", "c", "t", "mu")], k["mask"].to(DEV), False, k["allow"],
                        kappa=lv["kappa"], poly=lv["poly"], surf_kind=k["kind"].to(DEV))
    from torchoptics_amd import ray_tracing as rt
    mom = _moments_of(out[1])
    loss = (k["wm"].to(DEV) * mom[:, :7]).sum() + sum((q * w.to(DEV)).sum() for q, w in zip(out[:4], k["wts"]))
    loss = loss + (rt.compute_rms2d_batch(out[0], out[1], out[4]) * k["wl"].to(DEV)).sum()
    loss.backward()
    for i in range(6):
        assert torch.equal(out[i].cpu(), want["fwd"][i]), i
    for n in names:
        assert torch.equal(lv[n].grad.cpu(), want["grads"][n]), n
    for n in ("x", "y"):
        g = base[n].grad
        assert torch.equal(g[cut].cpu(), want["grads"][n]), n
        rest = g.clone()
        rest[cut] = 0.0
        assert not rest.any()                                              # nothing outside the view


@gpu
def test_moments_only_call_equals_the_full_call(ta):
    """want_rays=False (every per-ray pointer NULL): the same moments, and the same gradients of compute_rms2d through
    them, as the call that also writes the rays."""
    from torchoptics_amd import ray_tracing as rt
    k = _layout_case()
    names = _names(k, x_in=False)
    res = []
    for want_rays in (True, False):
        lv = {n: k[n].to(DEV).clone().requires_grad_(True) for n in names}
        out = ta.trace_skew(k["x"].to(DEV), k["y"].to(DEV), *[lv[n] for n in ("z", "cx", "cy", "c", "t", "mu")], k["mask"].to(DEV),
                            False, k["allow"], want_rays=want_rays, kappa=lv["kappa"], poly=lv["poly"], surf_kind=k["kind"].to(DEV))
        mom = _moments_of(out[1]) if want_rays else out
        assert mom.shape == (k["B"] * k["F"], 10) and mom.dtype == torch.float64
        n = k["P"] * k["W"]
        if want_rays:
            rms = ta.compute_rms2d(out[0], out[1], out[4])                  # lens 0, as the reference
            assert rms.item() == rt.rms_from_moments(mom[:k["F"]], n).item()
        else:
            rms = rt.rms_from_moments(mom[:k["F"]], n)
        rms.backward()
        res.append((mom.detach().cpu(), rms.item(), {n_: lv[n_].grad.cpu() for n_ in names}))
    assert torch.equal(res[0][0], res[1][0]) and res[0][1] == res[1][1]
    for n in names:
        assert torch.equal(res[0][2][n], res[1][2][n]), n
    # lens 1 is not part of compute_rms2d: its rows take exactly nothing
    assert not res[0][2]["c"][1].any() and res[0][2]["c"][0].any()


@gpu
@pytest.mark.parametrize("need", ((True, False), (False, True), (False, False)), ids=("x-only", "y-only", "neither"))
def test_fan_gradients_are_optional(ta, need):
    """requires_grad off on x and / or y (g_x_in / g_y_in NULL): the other gradients are bit-equal to the call that asks
    for both, and no gradient appears where none was asked for."""
    k = _case(1, seed=4243, B=2, F=2, W=3, P=300, name="cooke", asph=True, fill=1.2, dense=True)
    want = _kernel_run(ta, k)
    names = _names(k, x_in=False)
    lv = {n: k[n].to(DEV).clone().requires_grad_(True) for n in names}
    fan = {n: k[n].to(DEV).clone().requires_grad_(on) for n, on in zip(("x", "y"), need)}
    out = ta.trace_skew(fan["x"], fan["y"], *[lv[n] for n in ("z", "cx", "cy", "c", "t", "mu")], k["mask"].to(DEV), False, k["allow"],
                        kappa=lv["kappa"], poly=lv["poly"], surf_kind=k["kind"].to(DEV))
    from torchoptics_amd import ray_tracing as rt
    mom = _moments_of(out[1])
    loss = (k["wm"].to(DEV) * mom[:, :7]).sum() + sum((q * w.to(DEV)).sum() for q, w in zip(out[:4], k["wts"]))
    loss = loss + (rt.compute_rms2d_batch(out[0], out[1], out[4]) * k["wl"].to(DEV)).sum()
    loss.backward()
    for n in names:
        assert torch.equal(lv[n].grad.cpu(), want["grads"][n]), n
    for n, on in zip(("x", "y"), need):
        if on:
            assert torch.equal(fan[n].grad.cpu(), want["grads"][n]), n
        else:
            assert fan[n].grad is None


@gpu
def test_two_dimensional_rms_matches_the_fp64_oracle(ta):
    """compute_rms_spot_xy on the fused x- and y-moments (backward seeds 4..6 next to 0..2) against the same statistic
    formed from the oracle's rays with plain torch ops (test_gpu_parity.py::test_two_dimensional_rms_extension in fp64)."""
    from oracle import trace_oracle as orc
    from torchoptics_amd import ray_tracing as rt
    k = _case(1, seed=4244, B=1, F=3, W=3, P=300, name="cooke", asph=True, fill=1.2, dense=False)
    names = _names(k)
    lv = {n: k[n].to(DEV).clone().requires_grad_(True) for n in names}
    out = ta.trace_skew(*[lv[n] for n in ("x", "y", "z", "cx", "cy", "c", "t", "mu")], k["mask"].to(DEV), False, k["allow"],
                        kappa=lv["kappa"], poly=lv["poly"], surf_kind=k["kind"].to(DEV))
    got = rt.compute_rms_spot_xy(out[0], out[1], out[4])
    assert got.dtype == torch.float64
    got.backward()
    cl = {n: k[n].clone().requires_grad_(True) for n in names}
    o = orc.trace_skew_general(*[cl[n] for n in ("x", "y", "z", "cx", "cy", "c", "t", "mu")], k["mask"], cl["kappa"], cl["poly"],
                               [int(v) for v in k["kind"]], allow_backward_rays=k["allow"])
    x, y, ok = (q.expand(1, k["F"], k["P"], k["W"]) for q in (o[0], o[1], o[4]))
    n = k["P"] * k["W"]
    okd = ok[0].double()
    mx, my = x[0].sum(dim=(1, 2), keepdim=True) / n, y[0].sum(dim=(1, 2), keepdim=True) / n
    want = torch.sqrt((okd * ((x[0] - mx) ** 2 + (y[0] - my) ** 2)).sum(dim=(1, 2)) / n).mean()
    want.backward()
    assert torch.equal(out[4].cpu(), ok) and not ok.all()
    assert abs(got.item() - want.item()) <= SUM_TOL * want.item()
    for n_ in names:
        e = rel_l2(lv[n_].grad.cpu().numpy(), cl[n_].grad.numpy())
        assert cl[n_].grad.abs().max().item() > 0 and e < GRAD_TOL, f"d/d{n_}: {e:.2e}"


# ------------------------------------------------------------------------------------------------------------------
# 5. refusals on the C ABI
# ------------------------------------------------------------------------------------------------------------------

@gpu
def test_cabi_refusals_of_the_fp64_entry_points(ta):
    """Every bad call comes back with TL_EINVAL / TL_EWORKSPACE and a message before anything is launched (modelled on
    test_gpu_buckets.py::test_cabi_error_codes).  Every call here starts from a complete, valid problem with every buffer
    large enough, and changes one thing: a refusal that went missing would launch a valid trace, not a stray one."""
    import yaml_free_lenses as L
    from torchoptics_amd import _lib, ops
    lib = _lib.lib()
    EINVAL, EWORKSPACE = -1, -3
    d = L.PRESCRIPTIONS["singlet"]
    S, P = 3, 64
    f64 = lambda v: torch.tensor(v, dtype=torch.float64, device=DEV)        # noqa: E731
    x_e = torch.linspace(-2.0, 2.0, P, dtype=torch.float64, device=DEV).reshape(1, 1, P, 1)
    y_e = torch.linspace(-1.0, 1.5, P, dtype=torch.float64, device=DEV).reshape(1, 1, P, 1)
    z, cx, cy, c, t = f64([3.0]), f64([[0.02]]), f64([[0.05]]), f64([d["c"]]), f64([d["t"]])
    mu = f64([[[1.0, 1.0 / d["nd"][0], d["nd"][0]]]])
    m8 = torch.ones(1, S, dtype=torch.uint8, device=DEV)
    kap, pol = torch.zeros(1, S, dtype=torch.float64, device=DEV), torch.zeros(1, S, 4, dtype=torch.float64, device=DEV)
    kind = torch.tensor([[0, 1, 0]], dtype=torch.uint8, device=DEV)

    def problem(asph=False):
        return ops._problem(x_e, y_e, z, cx, cy, c, t, mu, m8, True, "strict", *((kap, pol, kind) if asph else ()))
    new = lambda *s: torch.zeros(s, dtype=torch.float64, device=DEV)        # noqa: E731
    ray = [new(1, 1, 1, P) for _ in range(4)]
    flag = [torch.zeros(1, 1, 1, P, dtype=torch.uint8, device=DEV) for _ in range(2)]
    mom = new(1, 10)
    big = new(3 * S * P + 64)                     # what a member with no meaning here is pointed at: larger than any of them
    rays = lambda **kw: _lib.rays(**dict(dict(x=ray[0], y=ray[1], cx=ray[2], cy=ray[3], ok=flag[0], back=flag[1], moments=mom), **kw))   # noqa: E731
    gr = dict(g_c=new(1, S), g_t=new(1, S), g_mu=new(1, 1, S), g_z=new(1), g_cx=new(1, 1), g_cy=new(1, 1), g_x_in=new(1, 1, 1, P),
              g_y_in=new(1, 1, 1, P))
    asph_gr = dict(g_kappa=new(1, S), g_poly=new(1, S, 4))
    sd = dict(gx=new(1, 1, 1, P) + 1e-3, gy=new(1, 1, 1, P) + 1e-3, g_moments=new(1, 10) + 1e-3)
    p = problem()
    nbytes = lib.tl_workspace_bytes_f64(C.byref(p))
    assert nbytes == (8 * S + 3) * 8 + 256          # one chunk, one block, one row: the backward's partial row
    need_f, need_b = 10 * 8, (8 * S + 3) * 8
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    st = ops._stream_ptr(torch.device(DEV))
    fwd = lambda p_, r_, n_=nbytes: lib.tl_trace_fwd_f64(None if p_ is None else C.byref(p_), r_, _lib.ptr(ws), n_, st)        # noqa: E731
    bwd = lambda p_, s_, g_, n_=nbytes: lib.tl_trace_bwd_f64(None if p_ is None else C.byref(p_), s_, g_, _lib.ptr(ws), n_, st)  # noqa: E731
    # the starting point is valid, both ways, spherical and aspheric
    pa = problem(asph=True)
    assert fwd(pa, rays()) == 0 and bwd(pa, _lib.seeds(**sd), _lib.grads(**gr, **asph_gr)) == 0
    assert fwd(p, rays()) == 0 and bwd(p, _lib.seeds(**sd), _lib.grads(**gr)) == 0
    torch.cuda.synchronize()
    assert flag[0].any() and gr["g_c"].abs().max().item() > 0 and asph_gr["g_kappa"].abs().max().item() > 0
    results = ray + [mom] + list(gr.values())
    before = [q.clone() for q in results]

    def refused(rc, code, word):
        msg = lib.tl_last_error()
        assert rc == code and msg and word in msg, (rc, code, word, msg)
    p0 = problem()
    p0.P = 0
    refused(fwd(p0, rays()), EINVAL, b"P >= 1")
    refused(bwd(p0, _lib.seeds(**sd), _lib.grads(**gr)), EINVAL, b"P >= 1")
    pg = problem()
    pg.aggregate = 1
    refused(fwd(pg, rays()), EINVAL, b"aggregate")
    refused(bwd(pg, _lib.seeds(**sd), _lib.grads(**gr)), EINVAL, b"aggregate")
    refused(fwd(p, rays(opd=big)), EINVAL, b"opd")
    refused(fwd(p, rays(stacks=big)), EINVAL, b"stacks")
    refused(bwd(p, _lib.seeds(g_opd=big, **sd), _lib.grads(**gr)), EINVAL, b"g_opd")
    refused(bwd(p, _lib.seeds(g_stacks=big, **sd), _lib.grads(**gr)), EINVAL, b"g_stacks")
    refused(bwd(p, _lib.seeds(**sd), _lib.grads(g_n_index=big, **gr)), EINVAL, b"g_n_index")
    refused(fwd(p, None), EINVAL, b"NULL")
    refused(bwd(p, None, _lib.grads(**gr)), EINVAL, b"NULL")
    refused(bwd(p, _lib.seeds(**sd), None), EINVAL, b"NULL")
    refused(fwd(None, rays()), EINVAL, b"NULL")
    refused(bwd(None, _lib.seeds(**sd), _lib.grads(**gr)), EINVAL, b"NULL")
    refused(fwd(p, rays(), need_f - 1), EWORKSPACE, b"workspace")
    refused(bwd(p, _lib.seeds(**sd), _lib.grads(**gr), need_b - 1), EWORKSPACE, b"workspace")
    assert fwd(p, rays(), need_f) == 0 and bwd(p, _lib.seeds(**sd), _lib.grads(**gr), need_b) == 0       # exactly enough is enough
    refused(bwd(pa, _lib.seeds(**sd), _lib.grads(**gr)), EINVAL, b"g_kappa")
    refused(bwd(pa, _lib.seeds(**sd), _lib.grads(g_kappa=asph_gr["g_kappa"], **gr)), EINVAL, b"g_poly")
    torch.cuda.synchronize()
    # nothing ran in between: the spherical call repeated last left what the first one left
    for a, b in zip(before, results):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------------
# 7. what the sweep's table covers (CPU, from the oracle alone)
# ------------------------------------------------------------------------------------------------------------------

def test_f64_case_table_covers_the_edges():
    cases = [_sweep_oracle(i) for i in range(len(SEEDS))]
    ks = [k for k, _ in cases]
    assert len(set(SEEDS)) == len(SEEDS) >= 24
    assert {k["P"] for k in ks} == set(P_LIST)
    assert {k["name"] for k in ks} == {"doublet", "cooke", "tessar"}
    assert {k["B"] for k in ks} == {1, 2, 3, 4} and {k["F"] for k in ks} == {1, 2, 3, 4}
    masks_differ = [k for k in ks if k["B"] >= 3 and len({tuple(m.reshape(-1).tolist()) for m in k["mask"]}) >= 3]
    assert masks_differ, "no batch of three or more lenses with differing mask rows"
    assert {k["allow"] for k in ks} == {True, False}
    assert {k["asph"] for k in ks} == {True, False}
    assert {k["W"] for k in ks} == {1, 3}
    assert {k["dense"] for k in ks} == {True, False}
    for n in ("cx", "mu"):                         # shared by the batch and per lens, both
        assert {k[n].shape[0] > 1 for k in ks if k["B"] > 1} == {True, False}, n
    assert {k["kappa"].dim() for k in ks if k["asph"] and k["B"] > 1} == {1, 2}
    assert all(bool((k["cx"] != 0).all()) for k in ks)
    dead = [r for _, r in cases if r["dead"] > 0]
    assert 3 * len(dead) >= len(cases), f"only {len(dead)} of {len(cases)} cases have dead rays"
    for k, r in cases:
        assert r["live"] >= 0.2, f"{_tag(k)}: {r['live']:.2f} of the rays live"
        assert r["near_ill"] == 0, f"{_tag(k)}: a ray within 1e-9 of the grazing count's threshold: replace the seed"
        for n, g in r["grads"].items():
            assert torch.isfinite(g).all() and g.abs().max().item() > 0, f"{_tag(k)}: d/d{n}"
    # the sequence mask matters somewhere (backward rays exist), and a lens batch has them
    assert any(r["back"] > 0 or (not k["allow"] and r["dead"] > 0) for k, r in cases)
