"""
The optical-path-length kernels against the oracle's fp64 run (tests/opd_cases.py; tests/test_opd_cases_cpu.py says when
that reference is fit to judge): trace_fwd_kernel<false, ASPH, true> and the OPD seed through every bucket of
trace_bwd_kernel<NS, ASPH, kPenNone>, its per-wave sums sgn[NS+1][kWaves], columns NB .. NB+NS of the partial rows and
the g_n[w][k] branch of reduce_bwd_kernel -- with S < NS and S == NS in every bucket, ragged and sub-block pupils, fans
that lose rays, lens batches, both arithmetic modes and both host chains.

Forward bound, per ray alive in the kernel, the fp64 and the fp32 oracle:
    |OPD - OPD_fp64| <= K u D + 2 |OPD_fp32 oracle - OPD_fp64|,   u = 2^-24,  D = sum_k |n_k d_k| + |n_S d_image| (fp64)
K is counted from the kernel's accumulation (trace_fwd_kernel), not fitted:
  strict, spherical row:  d = ((z_out + t_k) - z_in) / cz_in ; opd += n_k d.  Roundings that are not the oracle's: the
      stored z_out = z_hit - t_k and the sum z_out + t_k that undoes it (each relative to a height against a vertex plane
      that the neighbouring march reaches: charged as two roundings of a row's term each, 4), the difference, the divide
      and the product n_k d (3): 7 u |n_k d_k|, 7 u D over the rows.  An aspheric row adds n_k s with Newton's own s
      (product, the last update of s: fewer), the image plane a divide and a product (fewer).
  the running sum: S + 1 additions, each rounded relative to a partial sum <= D: (S + 1) u D.
      K_strict = S + 8.
  fast (DESIGN "Arithmetic modes": v_rcp / v_sqrt, 1 ulp = 2 u each, contraction only removes roundings): the row's and
      the image plane's divide become rcp + multiply, + 2 u of the term: + 2.  The traced state is no longer the fp32
      oracle's, so its distance does not cover it: per row three hardware square roots (cos_i, cos_t, cz) and the step's
      own divide turn the ray by <= 2 u each; a turn eps at a row moves the image point by <= eps x the path left and
      the path length by no more than that (times the sine of the angle at the image plane, <= 1): 4 x 2 u D per row.
      K_fast = K_strict + 2 + 8 S = 9 S + 10.
Strict mode is NOT bit-equal to the fp32 oracle (which sums n_k d_k with the step's own d, not the one recovered from z):
the bound is asserted in both modes, and `OPD-BND` prints the largest error / bound and how many rays differ in bits.

Gradients: relative L2 per leaf against fp64 with test_gpu_kernel_matrix._gate(n, pen=False, noise, k) -- lens leaves
(n_index among them) 2e-5, launch conditions max(3 noise, 3e-5), fast mode x 10, + 2 x the oracle's noise; the wavefront
loss times its cancellation factor (opd_cases.gate_cancel).  d/d n_index is also held entry by entry -- every k <= S of
every wavelength -- to lens gate x sum_rays |term| + 2 x the oracle's own entry distance, which is what a column
shifted by NS - S cannot pass.
"""
import pytest
import torch

import opd_cases as oc
from conftest import rel_l2
from test_gpu_kernel_matrix import _PER_RAY, _check_forward, _gate, _reduce

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
MODES = ("strict", "fast")
PER_LENS = ("z", "c", "t", "mu", "n_index")


def k_forward(S, mode):
    """K of the forward bound: see the derivation in the module docstring."""
    return S + 8 if mode == "strict" else 9 * S + 10


@pytest.fixture(scope="module")
def ta():
    import torchoptics_amd
    from torchoptics_amd import _lib
    _lib.lib()
    return torchoptics_amd


def _run(ta, refs, loss, mode, weights=(1.0,), w=None, strided=False, want_opd=True, lens=None):
    """The kernels on one lens or a batch (stacked along dim 0; x, y, cy, kappa, poly shared): forward outputs and the
    gradients of sum_b weights[b] loss_b.  `w`: path weights instead of the cases' own.  `lens`: trace only that lens of
    `refs`, with its weight."""
    from torchoptics_amd import ops, ray_tracing as rt
    if lens is not None:
        refs, weights = [refs[lens]], (weights[lens],)
    args = [r["args"] for r in refs]
    a0, B = args[0], len(args)
    names = refs[0]["names"]
    lv = {}
    for n in names:
        v = torch.cat([a[n] for a in args], 0) if (B > 1 and n in PER_LENS) else a0[n]
        lv[n] = v.to(DEV).clone().requires_grad_(True)
    x, y = a0["x"].to(DEV), a0["y"].to(DEV)
    if strided:
        _, F, P, W = x.shape
        big = [torch.full((1, F, 2 * P + 1, 2 * W), float("nan"), device=DEV) for _ in range(2)]
        big[0][:, :, 1::2, ::2], big[1][:, :, 1::2, ::2] = x, y
        x, y = big[0][:, :, 1::2, ::2], big[1][:, :, 1::2, ::2]
        assert not x.is_contiguous()
    kw = {}
    if a0["rows"]:
        kw = dict(kappa=lv["kappa"], poly=lv["poly"], surf_kind=torch.tensor(a0["kind"], dtype=torch.bool, device=DEV))
    if want_opd:
        kw.update(n_index=lv["n_index"], want_opd=True)
    out = ta.trace_skew(x, y, lv["z"], a0["cx"].to(DEV), lv["cy"], lv["c"], lv["t"], lv["mu"], a0["mask"].to(DEV), mode=mode, **kw)
    fwd = [t.detach().cpu() for t in out[:7 if want_opd else 6]]
    if not want_opd:
        return dict(fwd=fwd)
    inv = ops.used_walk_back(out[0])
    opd, ok = out[6], out[4]
    if w is None:
        w = torch.cat([a["w"] for a in args], 0)
    w = w.to(DEV)
    # lens by lens, so that a lens of a batch and the same lens traced alone go through the same torch reductions
    per = []
    for b in range(B):
        s = slice(b, b + 1)
        if loss == "wavefront":
            per.append(oc.wavefront(opd[s], ok[s])[0])
        else:
            per.append((opd[s] * w[s]).sum())
    total = sum(wt * lb for wt, lb in zip(weights, per))
    if loss == "path+rms":
        rms = ta.compute_rms2d(out[0], out[1], ok) if B == 1 else rt.compute_rms2d_batch(out[0], out[1], ok)
        total = total + (rms.reshape(-1) * torch.tensor(weights, device=DEV)).sum()
    total.backward()
    return dict(fwd=fwd, inv=inv, grads={n: lv[n].grad.detach().cpu() for n in names})


def _same_bits(tag, a, b, what):
    for key in ("fwd", "grads"):
        if key not in a or key not in b:
            continue
        items = a[key].items() if isinstance(a[key], dict) else enumerate(a[key])
        for n, t in items:
            assert torch.equal(t, b[key][n]), f"{tag}: {what}: {key} {n} changes bits"


def _check_opd(tag, got, r, S, mode):
    """OPD of one lens, element by element, against fp64; returns the line for the record."""
    o32, o64 = r["f32"]["fwd"], r["f64"]["fwd"]
    ok_g = got[4]
    dead = got[6][~ok_g]
    assert (dead == 0).all() and not torch.signbit(dead).any(), f"{tag}: OPD of a dead ray is not +0.0"
    assert torch.isfinite(got[6]).all(), f"{tag}: OPD not finite"
    both = ok_g & o64[4] & o32[4]
    err = (got[6].double() - o64[6]).abs()
    bound = k_forward(S, mode) * U * r["path"] + 2 * (o32[6].double() - o64[6]).abs()
    ratio = (err / bound)[both].max().item()
    n_bits = int((got[6] != o32[6])[both].sum())
    line = (f"OPD-BND {tag}: max err/bound {ratio:.3f} (K = {k_forward(S, mode)}, max err {err[both].max().item():.2e} mm, "
            f"path {r['path'][both].max().item():.0f} mm), {n_bits}/{int(both.sum())} rays differ in bits from the fp32 oracle")
    print(line)
    assert ratio <= 1.0, line
    return line


def _check_grads(tag, got, refs32, refs64, cancel, k, abs_n=None):
    """Per leaf: finite, then relative L2 against fp64 under the project's gate; d/d n_index also entry by entry."""
    for n, g in got.items():
        assert torch.isfinite(g).all(), f"{tag}: d/d{n} not finite"
    msg = []
    for n, g in got.items():
        g = g.double()
        w32, w64 = refs32[n], refs64[n]
        if n in _PER_RAY:
            d = (w32 - w64).abs()
            w32, w64 = _reduce(n, w32, g), _reduce(n, w64, g)
            noise = rel_l2(w32.numpy(), w64.numpy())
            if n == "z":                      # test_gpu_kernel_matrix._grad_errors: the oracle's distance summed ray by ray
                noise = max(noise, float(_reduce(n, d, g).norm() / w64.norm()))
        else:
            noise = rel_l2(w32.numpy(), w64.numpy())
        e64 = rel_l2(g.reshape(w64.shape).numpy(), w64.numpy())
        cn = cancel[n]
        gate = (_gate(n, False, noise, k) - 2 * noise) * cn + 2 * noise
        msg.append(f"{n} {e64:.1e}/{noise:.1e}" + (f"/x{cn:.1f}" if cn > 1.05 else ""))
        assert e64 <= gate, f"{tag} d/d{n}: vs fp64 {e64:.2e}, gate {gate:.2e}, oracle fp32 itself {noise:.2e}, cancellation x{cn:.1f}"
        if n == "n_index" and abs_n is not None:
            lim = (_gate(n, False, 0.0, k) * abs_n + 2 * (w32 - w64).abs()).reshape(w64.shape)
            bad = (g.reshape(w64.shape) - w64).abs() > lim
            assert not bad.any(), (f"{tag} d/dn_index: entries [.., wavelength, row] {bad.nonzero()[:4, -2:].tolist()} off: "
                                   f"{g.reshape(w64.shape)[bad][:4].tolist()} vs fp64 {w64[bad][:4].tolist()}")
    return msg


CASE_IDS = [oc.case_id(c) for c in oc.CASES]


@pytest.mark.parametrize("loss", oc.LOSSES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("S,variant,P", oc.CASES, ids=CASE_IDS)
def test_opd_case_matches_fp64_oracle(ta, S, variant, P, mode, loss):
    r = oc.reference(S, variant, P)
    k = 10.0 if mode == "fast" else 1.0
    tag = f"S={S} {variant} P={P} {loss} {mode}"
    got = _run(ta, [r], loss, mode)
    assert got["inv"] is False, f"{tag}: the walk-back does not carry the OPD seed"
    # forward
    _check_forward(tag, got["fwd"][:6], r["f32"]["fwd"][:6], r["f64"]["fwd"][:6], exact=(variant == "sph" and mode == "strict"), k=k)
    _check_opd(tag, got["fwd"], r, S, mode)
    # gradients
    cancel = {n: oc.gate_cancel(r, loss, n) for n in r["names"]}
    msg = _check_grads(tag, got["grads"], r["f32"]["grads"][loss], r["f64"]["grads"][loss], cancel, k, r["abs_n"][loss])
    print(f"OPD-GRAD {tag}: e64/noise[/cancellation] " + ", ".join(msg))
    _same_bits(tag, got, _run(ta, [r], loss, mode), "second run")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("S,variant,P", oc.CASES, ids=CASE_IDS)
def test_want_opd_leaves_the_ray_outputs_bit_identical(ta, S, variant, P, mode):
    """x, y, cx, cy, ok, back of a want_opd trace have the bits of the same trace without it.

    In fast mode an all-spherical trace without OPD runs trace_fwd_plain_kernel<2> (two rays per lane), and contraction
    fuses that body and trace_fwd_kernel<false, false, true> into different multiply-adds (measured: up to 637 of 6993
    rays differed in x, y by <= 3.1e-6 mm, masks identical).  launch_fwd therefore takes the ray outputs, flags and moments
    of such a trace from the plain kernel and has the OPD kernel write the OPD alone; each decides `ok` for itself, which
    _check_opd would show (a live ray with OPD 0, or a dead one with a path)."""
    r = oc.reference(S, variant, P)
    tag = f"S={S} {variant} P={P} {mode}"
    with_opd, plain = _run(ta, [r], "path", mode), _run(ta, [r], "path", mode, want_opd=False)
    names = ("x", "y", "cx", "cy", "ok", "back")
    diff = {n: (int((p_ != q_).sum()), (p_.double() - q_.double()).abs().max().item()) for n, p_, q_ in zip(names, plain["fwd"], with_opd["fwd"])}
    print(f"OPD-SAME {tag}: rays that differ / largest difference: " + ", ".join(f"{n} {c}/{d:.1e}" for n, (c, d) in diff.items()))
    for n, p_, q_ in zip(names, plain["fwd"], with_opd["fwd"]):
        assert torch.equal(p_, q_), f"{tag}: {n} of a want_opd trace differs in bits from the same trace without it ({diff[n]})"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("S,variant,P", oc.CASES, ids=CASE_IDS)
def test_opd_seed_of_dead_rays_changes_no_bit(ta, S, variant, P, mode):
    """NaN, inf and 1e30 as the OPD seed of dead rays: no gradient may see them."""
    r = oc.reference(S, variant, P)
    tag = f"S={S} {variant} P={P} path {mode}"
    clean = _run(ta, [r], "path", mode)
    dead = ~clean["fwd"][4]
    assert dead.any()
    w = r["args"]["w"].clone()
    w[dead] = torch.tensor([float("nan"), float("inf"), 1e30, -float("inf")]).repeat(int(dead.sum()) // 4 + 1)[:int(dead.sum())]
    got = _run(ta, [r], "path", mode, w=w)
    for n, g in got["grads"].items():
        assert torch.isfinite(g).all(), f"{tag}: d/d{n} not finite with a poisoned seed on dead rays"
        assert torch.equal(g, clean["grads"][n]), f"{tag}: d/d{n} changes bits with the OPD seed of dead rays"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("S,variant,P", [c for c in oc.CASES if c[2] == oc.P_MAIN], ids=[i for i, c in zip(CASE_IDS, oc.CASES) if c[2] == oc.P_MAIN])
def test_strided_pupil_gives_the_contiguous_bits(ta, S, variant, P, mode):
    r = oc.reference(S, variant, P)
    _same_bits(f"S={S} {variant} P={P} {mode}", _run(ta, [r], "path+rms", mode), _run(ta, [r], "path+rms", mode, strided=True),
               "x, y as strided views")


@pytest.mark.parametrize("loss", oc.LOSSES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("S,variant", oc.BATCH_CASES, ids=[f"S{s}-{v}" for s, v in oc.BATCH_CASES])
def test_lens_batch_is_held_lens_by_lens(ta, S, variant, mode, loss):
    """B = 3, per-lens z, c, t, mu and n_index in one launch: every lens against its own oracle run, the shared leaves
    against the weighted sum, and lens b's d/d n_index equal in bits to lens b traced alone."""
    rs = [oc.reference(S, variant, oc.P_MAIN, b) for b in range(len(oc.BATCH_W))]
    k = 10.0 if mode == "fast" else 1.0
    tag = f"batch S={S} {variant} {loss} {mode}"
    got = _run(ta, rs, loss, mode, weights=oc.BATCH_W)
    assert got["inv"] is False, tag
    shared32, shared64, shared_abs = {}, {}, {}
    msg = []
    for b, (r, wt) in enumerate(zip(rs, oc.BATCH_W)):
        tb = f"{tag} lens {b}"
        fwd = [t[b:b + 1] for t in got["fwd"]]
        _check_forward(tb, fwd[:6], r["f32"]["fwd"][:6], r["f64"]["fwd"][:6], exact=(variant == "sph" and mode == "strict"), k=k)
        _check_opd(tb, fwd, r, S, mode)
        r32 = {n: wt * g for n, g in r["f32"]["grads"][loss].items()}
        r64 = {n: wt * g for n, g in r["f64"]["grads"][loss].items()}
        mine = {n: got["grads"][n][b:b + 1] for n in PER_LENS}
        cancel = {n: oc.gate_cancel(r, loss, n) for n in r["names"]}
        msg += [f"{b}:" + m for m in _check_grads(tb, mine, r32, r64, cancel, k, wt * r["abs_n"][loss])]
        for n in r["names"]:
            if n not in PER_LENS:
                shared32[n] = shared32.get(n, 0) + r32[n]
                shared64[n] = shared64.get(n, 0) + r64[n]
                # sum over the lenses of each lens's sum_rays |term|, as a norm ratio against the summed gradient
                shared_abs[n] = shared_abs.get(n, 0.0) + wt * r["cancel"][loss][n] * float(
                    (_reduce(n, r["f64"]["grads"][loss][n], None) if n in _PER_RAY else r["f64"]["grads"][loss][n]).norm())
        alone = _run(ta, rs, loss, mode, weights=oc.BATCH_W, lens=b)
        assert torch.equal(alone["grads"]["n_index"], got["grads"]["n_index"][b:b + 1]), f"{tb}: d/dn_index differs in bits from the lens traced alone"
    cancel = {}
    for n in shared64:
        tot = float((_reduce(n, shared64[n], None) if n in _PER_RAY else shared64[n]).norm())
        cancel[n] = min(shared_abs[n] / max(tot, 1e-300), oc.CANCEL_CAP) if loss == "wavefront" else 1.0
    msg += _check_grads(tag, {n: got["grads"][n] for n in shared64}, shared32, shared64, cancel, k)
    print(f"OPD-GRAD {tag}: e64/noise[/cancellation] " + ", ".join(msg))


@pytest.mark.parametrize("S,variant,P", oc.HOST_CHAIN_CASES, ids=[oc.case_id(c) for c in oc.HOST_CHAIN_CASES])
def test_host_chains_agree_bit_for_bit(ta, S, variant, P):
    """The ctypes chain of ops.py and trace_cpp of csrc/tl_torch.cpp launch the same kernels with the same arguments."""
    from test_gpu_host_chain import _both
    from torchoptics_amd import ops
    assert ops.host_chain() == "cpp", "the C++ host extension (_tlx.so) is not built / does not load"
    r = oc.reference(S, variant, P)
    for mode in MODES:
        cpp, py = _both(lambda: _run(ta, [r], "path+rms", mode))
        assert cpp["inv"] is False and py["inv"] is False
        _same_bits(f"S={S} {variant} P={P} {mode}", cpp, py, "C++ and ctypes host chains")
        assert all(torch.isfinite(g).all() for g in cpp["grads"].values())
