"""
The fp32 forward trace kernels (trace_fwd_kernel<PEN, ASPH, OPD>, trace_fwd_plain_kernel<2>: csrc/tl_kernels.inc) against
the oracle's trace_skew_general in fp64, over the table of tests/fwd_cases.py: every forward kernel of the build (fwd_cases.
KERNELS), strict and fast, on an unfiltered fan, at one, at 1 and 2 and at 2 and 3 chunks per block in a batch of four lenses.

Every call goes through the C ABI (tl_trace_fwd) with the conditioning bytes and, on aspheric lenses, the hit-point buffer
attached, so one launch yields everything a forward can write: rays, flags, path length, stacks, hits, the ten moments.

  1  every output of every case against the gates of fwd_cases.py, lens by lens; the moments against fp64 sums of the
     kernel's own fp32 outputs (counts equal, sums within n 2^-53 sum |terms|);
  2  cond_flags and asph_hits, with 4 hit slots on lenses of 3 and of 5 aspheric rows over a buffer of sentinels;
  3  bit invariance: a row of the batch against that row traced alone; broadcast, dense and strided fans; moments-only,
     aggregate='sum' and x_moments calls; allow_backward_rays=False.

Found by test_forward_case_matches_fp64_oracle[r3-P33101-S5-sph-opd-fast] ("opd of a dead ray is not zero"): fast mode writes
the path length of an all-spherical lens with a second kernel, which decided `ok` for itself; it now reads the first one's.

Run with -s for the FWD-ACC lines (condensed in profiles/fwd_accuracy.txt).
"""
import ctypes as C

import pytest
import torch

import fwd_cases as fc
import test_gpu_kernel_matrix as km

DEV = "cuda:0"
gpu = pytest.mark.gpu
SENTINEL = -12345.0
PAD = 1024                          # floats behind the hit-point buffer that must stay untouched


@pytest.fixture(scope="module")
def ta():
    import torchoptics_amd
    from torchoptics_amd import _lib
    _lib.lib()
    return torchoptics_amd


def _ref(name, P, S, variant, b=0):
    """fwd_cases.reference, with at most one of the large shapes cached at a time."""
    if name in ("r2", "r3"):
        fc.free("r3" if name == "r2" else "r2")
    return fc.reference(name, P, S, variant, b)


# ------------------------------------------------------------------------------------------------------------------
# one launch through the C ABI
# ------------------------------------------------------------------------------------------------------------------

def _fan_view(v, shape, layout):
    """The pupil coordinate v [1,1,P,1] as the [B,F,P,W] view the kernel reads: strides (0,0,1,0), dense, or every second
    element along P of a larger buffer whose other elements are NaN."""
    B, F, P, W = shape
    v = v.to(DEV)
    if layout == "broadcast":
        return v.expand(B, F, P, W)
    if layout == "dense":
        return v.expand(B, F, P, W).contiguous()
    buf = torch.full((B, F, 2 * P + 1, W), float("nan"), dtype=torch.float32, device=DEV)
    buf[:, :, 1::2, :] = v
    out = buf[:, :, 1::2, :]
    assert out.stride(2) == 2 * W and out.shape == (B, F, P, W)
    return out


def run(lenses, output, mode, allow=True, x_moments=True, want_rays=True, layout="broadcast", slots=fc.HIT_SLOTS, cpu=True):
    """tl_trace_fwd on the lenses (fwd_cases.lens dictionaries) in one launch.  Returns the outputs in the form of
    fwd_cases.oracle_run, [B,F,P,W]: fwd, opd, stk [3,S,B,F,P,W], hits [slots,2,B,F,P,W] (+ hits_pad, the floats behind
    the buffer), flags, moments [B*F,10]; what the call does not write is None."""
    from torchoptics_amd import _lib, ops
    a0, B = lenses[0], len(lenses)
    F, W, S, P = a0["cy"].shape[1], a0["mu"].shape[3], a0["c"].shape[-1], a0["x"].shape[2]
    dev = torch.device(DEV)
    cat = lambda n, *tail: torch.cat([a[n].reshape(1, *tail) for a in lenses]).contiguous().to(DEV)      # noqa: E731
    x_e, y_e = _fan_view(a0["x"], (B, F, P, W), layout), _fan_view(a0["y"], (B, F, P, W), layout)
    z, cx, cy = cat("z"), a0["cx"].reshape(1, 1).to(DEV), cat("cy", F)
    c, t, mu = cat("c", S), cat("t", S), cat("mu", W, S)
    mask = torch.cat([a["mask"].reshape(1, S) for a in lenses]).to(torch.uint8).contiguous().to(DEV)
    asph = bool(a0["rows"])
    kap = pol = kind = None
    if asph:
        kap, pol = cat("kappa", S), cat("poly", S, 4)
        kind = torch.tensor([a0["kind"]] * B, dtype=torch.uint8, device=DEV)
    nidx = cat("n_index", W, S + 1) if output == "opd" else None
    n = B * F * W * P
    hits_flat = hits = cond = None
    if want_rays:
        cond = torch.full((B, F, W, P), 255, dtype=torch.uint8, device=DEV)
        if slots:
            hits_flat = torch.full((slots * 2 * n + PAD,), SENTINEL, dtype=torch.float32, device=DEV)
            hits = hits_flat[:slots * 2 * n].view(slots, 2, B, F, W, P)
    aggregate = output in ("pen", "pensum")
    prob = ops._problem(x_e, y_e, z, cx, cy, c, t, mu, mask, allow, mode, kap, pol, kind, nidx, aggregate, hits, x_moments, cond)
    assert (prob.B, prob.F, prob.W, prob.S, prob.P) == (B, F, W, S, P) and prob.cy_stride_b == (F if B > 1 else 0)
    nbytes = _lib.lib().tl_workspace_bytes(C.byref(prob))
    ws = ops._workspace(nbytes, dev)
    new = lambda dt: torch.empty((B, F, W, P), dtype=dt, device=DEV)      # noqa: E731
    fp = [new(torch.float32) for _ in range(4)] if want_rays else [None] * 4
    bp = [new(torch.uint8) for _ in range(2)] if want_rays else [None] * 2
    opd = new(torch.float32) if (want_rays and output == "opd") else None
    stk = torch.empty((3, S, B, F, W, P), dtype=torch.float32, device=DEV) if (want_rays and output == "pen") else None
    moments = torch.full((B * F, 10), float("nan"), dtype=torch.float64, device=DEV)
    out = _lib.rays(x=fp[0], y=fp[1], cx=fp[2], cy=fp[3], ok=bp[0], back=bp[1], opd=opd, stacks=stk, moments=moments)
    ops._call("tl_trace_fwd", dev, C.byref(prob), out, ws, ws.numel())
    torch.cuda.synchronize()
    put = (lambda q: None if q is None else q.cpu()) if cpu else (lambda q: q)
    sw = lambda q: None if q is None else put(q.transpose(-1, -2))      # noqa: E731   [..,W,P] -> [..,P,W]
    res = dict(fwd=None, opd=sw(opd), stk=sw(stk), hits=sw(hits), flags=sw(cond), moments=put(moments),
               hits_pad=None if hits_flat is None else put(hits_flat[slots * 2 * n:]))
    if want_rays:
        res["fwd"] = [sw(q) for q in fp] + [sw(q).bool() for q in bp]
    return res


def lens_of(got, b):
    """Lens b of a launch's outputs."""
    cut = lambda q, d: None if q is None else q.narrow(d, b, 1)      # noqa: E731
    return dict(fwd=[cut(q, 0) for q in got["fwd"]], opd=cut(got["opd"], 0), stk=cut(got["stk"], 2), hits=cut(got["hits"], 2),
                flags=cut(got["flags"], 0))


def _rows_used(ref, slots=fc.HIT_SLOTS):
    return 0 if ref["f64"]["hits"] is None else min(slots, ref["f64"]["hits"].shape[0])


MAXNORM_AMP = 2.0


def _well_conditioned(ref):
    """The rays the max-norm gate of test_gpu_kernel_matrix._check_forward is made for: amplification A_i (with the image
    plane's factor) at most MAXNORM_AMP.  That gate is "worst ray <= tol k + 2 x the fp32 oracle's worst ray", and the fan
    it has been applied to carries A_i <= 1.6 on every lens (its outer points go back into the fan when they get through).
    On the unfiltered fan the worst ray of any fp32 evaluation is the most amplified one of the set, whatever the set, and
    one evaluation's draw on it is no bound for another's: the kernels showed 7.1e-3 mm against the oracle's 1.8e-3 on a ray
    of the 5-row lens at A_i up to 6e4, and 1.6e-4 against 4.0e-5 at A_i up to 93.  Such rays are held by the per-ray gate;
    the max-norm gate stays as it is on the 97 % of the fan it was made for."""
    return ref["amp_image"] <= MAXNORM_AMP


def check_lens(tag, gb, ref, variant, mode, allow=True, ref32=None):
    """Every per-ray output of one lens against the gates of fwd_cases.py.  Returns the line for the record."""
    k = fc.K_FAST if mode == "fast" else 1.0
    f32, f64 = (ref32 or ref["f32"]), ref["f64"]
    fwd = gb["fwd"]
    ok_g, ok64, ok32 = fwd[4], f64["fwd"][4], f32["fwd"][4]
    if allow and variant == "sph" and mode == "strict":
        km._check_forward(tag, fwd, f32["fwd"], f64["fwd"], exact=True, k=k)
    elif allow:
        well = _well_conditioned(ref)
        if (ok_g & ok64 & ok32 & well).any():
            cut = lambda qs: [torch.where(well, q, torch.zeros_like(q)) for q in qs]      # noqa: E731
            km._check_forward(tag, cut(fwd), cut(f32["fwd"]), cut(f64["fwd"]), exact=False, k=k)
    # the hit points the lens has slots for; the stacks only where the call wrote them
    nh = _rows_used(ref)
    run_ = dict(gb, hits=gb["hits"][:nh] if nh else None)
    refv = dict(ref, f64=dict(f64, hits=f64["hits"][:nh] if nh else None))
    left = fc.rays_differing(run_, refv)
    cap = 2 * fc.rays_differing(f32, refv) + 2
    assert left <= cap, f"{tag}: {left} rays die elsewhere than in the fp64 oracle (the fp32 oracle allows {cap})"
    alive_g = gb["flags"] != 0
    keep = (alive_g & ref["alive"]) & (ok_g == ok64)
    rt = fc.ratios(run_, refv, k, fc.C, keep=keep)
    worst = max(rt, key=rt.get)
    assert rt[worst] <= 1.0, f"{tag}: {worst} misses its per-ray gate by {rt[worst]:.2f} x ({rt})"
    # dead rays: exact zeros, flag 0; the flags of the rest, away from the threshold
    dead = ~alive_g
    if allow:
        assert torch.equal(alive_g, ok_g), f"{tag}: flag 0 is not `dead`"
    for n, q in list(zip(("x", "y", "cx", "cy"), fwd[:4])) + ([("opd", gb["opd"])] if gb["opd"] is not None else []):
        assert not (q[dead] != 0).any(), f"{tag}: {n} of a dead ray is not zero"
    bad = (gb["flags"] != ref["flags"]) & ~ref["near"] & (alive_g == ref["alive"])
    assert not bad.any(), f"{tag}: {int(bad.sum())} conditioning flags differ from the fp64 oracle's"
    assert int((alive_g != ref["alive"]).sum()) <= cap, tag
    bits = ""
    if gb["stk"] is not None and mode == "strict":
        bits = f", strict z_RELU bit-equal to the fp32 oracle: {torch.equal(gb['stk'][0], f32['stk'][0])}"
    return (f"FWD-ACC {tag}: error / gate " + ", ".join(f"{n} {v:.3f}" for n, v in rt.items())
            + f"; left out {left} (cap {cap}){bits}")


def check_moments(tag, got, stk, x_moments=True):
    """The ten columns of a launch against fp64 sums of the launch's own per-ray outputs (fwd_cases.moments_of)."""
    x, y, _, _, ok, back = got["fwd"]
    want, bound = fc.moments_of(x, y, ok, back, got["flags"], stk)
    m = got["moments"]
    assert m.shape == want.shape and torch.isfinite(m).all(), tag
    if not x_moments:
        assert not m[:, 4:7].any(), f"{tag}: x-moments filled without x_moments"
        want[:, 4:7] = 0.0
    if stk is None:
        assert not m[:, 8].any(), f"{tag}: sum Q without the penalty term"
    for j in fc.COUNTS:
        assert torch.equal(m[:, j], want[:, j]), f"{tag}: count {j}: {m[:, j].tolist()} vs {want[:, j].tolist()}"
    worst = 0.0
    for j in fc.SUMS:
        e = (m[:, j] - want[:, j]).abs()
        assert (e <= bound[:, j]).all(), f"{tag}: moment {j}: {m[:, j].tolist()} vs {want[:, j].tolist()} (bound {bound[:, j].tolist()})"
        worst = max(worst, float((e / bound[:, j].clamp(min=1e-300)).max()))
    return worst


# ------------------------------------------------------------------------------------------------------------------
# 1. every case, output and mode against the fp64 oracle
# ------------------------------------------------------------------------------------------------------------------

def _id(case):
    return "%s-P%d-S%d-%s" % case


@gpu
@pytest.mark.parametrize("mode", fc.MODES)
@pytest.mark.parametrize("output", fc.OUTPUTS)
@pytest.mark.parametrize("case", fc.CASES, ids=_id)
def test_forward_case_matches_fp64_oracle(ta, case, output, mode):
    name, P, S, variant = case
    lenses = fc.lens(name, P, S, variant)
    tag = f"{_id(case)} {output} {mode}"
    if output in ("pen", "pensum") and S > 31:
        with pytest.raises(RuntimeError, match="aggregate needs S <= 31"):
            run(lenses, output, mode)
        return
    got = run(lenses, output, mode)
    stk = got["stk"]
    if output == "pensum":          # the stacks column 8 is rebuilt from: those of the call that writes them
        full = run(lenses, "pen", mode)
        stk = full["stk"]
        for i in range(6):
            assert torch.equal(got["fwd"][i], full["fwd"][i]), f"{tag}: output {i} differs from aggregate=True"
    lines = []
    for b in range(len(lenses)):
        ref = _ref(name, P, S, variant, b)
        lines.append(check_lens(f"{tag} lens {b}", lens_of(got, b), ref, variant, mode))
    worst = check_moments(tag, got, stk)
    print("\n".join(lines))
    print(f"FWD-ACC {tag}: moments worst error / bound {worst:.3f}")


# ------------------------------------------------------------------------------------------------------------------
# 2. cond_flags and asph_hits
# ------------------------------------------------------------------------------------------------------------------

HIT_CASES = ([("main", 777, 5, "sph")] + [("main", 777, S, v) for S, v in fc.HIT_LENSES]
             + [("r3", 33101, S, v) for S, v in fc.BIG_LENSES])


@gpu
@pytest.mark.parametrize("mode", fc.MODES)
@pytest.mark.parametrize("output", ("rays", "pen"))
@pytest.mark.parametrize("case", HIT_CASES, ids=_id)
def test_flags_and_hit_points(ta, case, output, mode):
    """What the walk-back reads instead of recomputing: one byte per ray (0 dead, 1 live, 2 live and ill-conditioned) and
    the (X, Y) of the first 4 aspheric rows, slot j = aspheric rows before the row.  A lens with 3 such rows leaves slot 3
    alone, one with 5 writes nothing for its fifth, an all-spherical lens writes nothing at all; nothing is written
    behind the buffer."""
    name, P, S, variant = case
    lenses = fc.lens(name, P, S, variant)
    tag = f"hits {_id(case)} {output} {mode}"
    got = run(lenses, output, mode)
    n_rows = len(lenses[0]["rows"])
    used = min(fc.HIT_SLOTS, n_rows)
    assert (n_rows, used) in ((0, 0), (3, 3), (5, 4))
    assert (got["hits_pad"] == SENTINEL).all(), f"{tag}: written behind the hit-point buffer"
    assert (got["hits"][used:] == SENTINEL).all(), f"{tag}: a slot the lens has no row for was written"
    lines = []
    for b in range(len(lenses)):
        ref = _ref(name, P, S, variant, b)
        gb = lens_of(got, b)
        lines.append(check_lens(f"{tag} lens {b}", gb, ref, variant, mode))
        alive = gb["flags"] != 0
        if used:
            assert not (gb["hits"][:used][:, :, alive] == SENTINEL).any(), f"{tag}: a live ray without a hit point"
    check_moments(tag, got, got["stk"])
    print("\n".join(lines))


# ------------------------------------------------------------------------------------------------------------------
# 3. bit invariance
# ------------------------------------------------------------------------------------------------------------------

def _same_bits(tag, a, b, names=("fwd", "opd", "stk", "hits", "flags")):
    """Bit equality of two launches' per-ray outputs (b may broadcast against a: one row against every row)."""
    for n in names:
        qa, qb = a[n], b[n]
        assert (qa is None) == (qb is None), (tag, n)
        for i, (u, v) in enumerate(zip(qa, qb) if n == "fwd" else [(qa, qb)] if qa is not None else []):
            if u.dtype == torch.float32:        # (NaN is a value a wrong kernel could write: compare the bits)
                u, v = u.contiguous().view(torch.int32), v.contiguous().view(torch.int32)
            assert bool((u == v).all()), f"{tag}: {n}[{i}] differs on {int((u != v).sum())} elements"


ROW_OF = (1, 2, 1)                  # the (lens, field, wavelength) of r3 that every row of the replicated launch carries


@gpu
@pytest.mark.parametrize("mode", fc.MODES)
@pytest.mark.parametrize("output", fc.OUTPUTS)
@pytest.mark.parametrize("S,variant", fc.BIG_LENSES)
def test_every_row_of_a_batch_equals_the_row_traced_alone(ta, S, variant, output, mode):
    """4 x 4 x 3 rows of 33 101 points (44 blocks of 2 and 3 chunks; two rays per lane: a full and a half round) that all
    carry one lens, field and wavelength, against that row alone (130 blocks of one chunk): per-ray outputs bit-equal,
    counts equal, moment sums within the derived bound."""
    b, f, w = ROW_OF
    a = fc.lens("r3", 33101, S, variant)[b]
    B, F, W, _ = fc.SHAPES["r3"]
    assert fc.plan_of(B, F, W, 33101) == fc.EXPECT[("r3", 33101)] and fc.plan_of(1, 1, 1, 33101) == fc.ALONE
    one = dict(a, cy=a["cy"][:, f:f + 1], mu=a["mu"][:, :, :, w:w + 1], n_index=a["n_index"][:, :, :, w:w + 1])
    rep = dict(one, cy=one["cy"].expand(1, F, 1, 1), mu=one["mu"].expand(1, 1, 1, W, S),
               n_index=one["n_index"].expand(1, 1, 1, W, S + 1))
    tag = f"rows S={S} {variant} {output} {mode}"
    alone = run([one], output, mode, cpu=False)
    full = run([rep] * B, output, mode, cpu=False)
    _same_bits(tag, full, alone)
    assert alone["fwd"][4].any() and not alone["fwd"][4].all() and (alone["flags"] == 2).any()
    m, m1 = full["moments"].cpu(), alone["moments"].cpu()
    _, bound = fc.moments_of(*[q.cpu() for q in (alone["fwd"][0], alone["fwd"][1], alone["fwd"][4], alone["fwd"][5])],
                             alone["flags"].cpu(), None if alone["stk"] is None else alone["stk"].cpu())
    for j in fc.COUNTS:
        assert (m[:, j] == W * m1[0, j]).all(), f"{tag}: count {j}"
    for j in fc.SUMS:
        # W rows of P terms each against W x (one row of P terms): both within P W 2^-53 sum |terms| of the exact sum
        assert ((m[:, j] - W * m1[0, j]).abs() <= 2 * W * W * bound[0, j]).all(), f"{tag}: moment {j}"
    assert m1[0, 3] > 0 and m1[0, 7] > 0 and m1[0, 9] > 0 and (output not in ("pen", "pensum") or m1[0, 8] > 0)


LAYOUT_CASES = [("main", 777, 7, "sph"), ("main", 777, 7, "asph")] + [("r2", 22101, S, v) for S, v in fc.BIG_LENSES]


@gpu
@pytest.mark.parametrize("mode", fc.MODES)
@pytest.mark.parametrize("output", fc.OUTPUTS)
@pytest.mark.parametrize("case", LAYOUT_CASES, ids=_id)
def test_fan_layouts_give_the_same_bits(ta, case, output, mode):
    """x_in, y_in as a broadcast [1,1,P,1], written out [B,F,P,W], and as every second element of a larger buffer."""
    name, P, S, variant = case
    lenses = fc.lens(name, P, S, variant)
    base = run(lenses, output, mode, cpu=False)
    for layout in ("dense", "strided"):
        other = run(lenses, output, mode, layout=layout, cpu=False)
        _same_bits(f"{layout} {name} S={S} {variant} {output} {mode}", other, base)
        assert torch.equal(other["moments"], base["moments"]), layout


@gpu
@pytest.mark.parametrize("mode", fc.MODES)
@pytest.mark.parametrize("variant", fc.VARIANTS)
@pytest.mark.parametrize("name,P", (("main", 777), ("r3", 33101)))
def test_moment_columns_do_not_depend_on_what_else_is_written(ta, name, P, variant, mode):
    """want_rays=False (every per-ray pointer NULL), aggregate='sum' (stacks NULL) and x_moments on or off return the
    full call's columns bit for bit; with x_moments off, columns 4..6 are exactly 0."""
    S = {"sph": 5, "asph": 7}[variant]
    lenses = fc.lens(name, P, S, variant)
    tag = f"columns {name} S={S} {variant} {mode}"
    for output in fc.OUTPUTS:
        full = run(lenses, output, mode, cpu=False)["moments"]
        assert torch.isfinite(full).all() and (full[:, 4:7] != 0).any(), tag
        only = run(lenses, output, mode, want_rays=False, cpu=False)["moments"]
        assert torch.equal(only, full), f"{tag} {output}: the moments-only call differs"
        for want_rays in (True, False):
            no_x = run(lenses, output, mode, x_moments=False, want_rays=want_rays, cpu=False)["moments"]
            assert not no_x[:, 4:7].any(), f"{tag} {output}: x-moments without x_moments"
            keep = [0, 1, 2, 3, 7, 8, 9]
            assert torch.equal(no_x[:, keep], full[:, keep]), f"{tag} {output}: x_moments changes another column"
    pen, pensum = (run(lenses, o, mode, cpu=False)["moments"] for o in ("pen", "pensum"))
    assert torch.equal(pen, pensum) and (pen[:, 8] > 0).all(), f"{tag}: aggregate='sum' differs from aggregate=True"


@gpu
@pytest.mark.parametrize("mode", fc.MODES)
@pytest.mark.parametrize("output", fc.OUTPUTS)
def test_backward_rays_not_allowed(ta, output, mode, variant="sph"):
    """allow_backward_rays=False on the 5-row lens: a ray that turns back on the way dies there, one that does so at the
    image plane keeps its y, its path length, its stacks and its flag, and loses `ok`: columns 1..3 follow `ok`, column 0
    and column 9 follow `alive`."""
    lenses = fc.lens("main", 777, 5, variant)
    a = lenses[0]
    ref = dict(args=a, f32=fc.oracle_run(a, torch.float32, False), f64=fc.oracle_run(a, torch.float64, False))
    ref["alive"], ref["min_cos2"], ref["flags"], ref["near"] = fc.conditioning(ref["f64"]["stk"])
    ref["amp"] = 1.0 / ref["min_cos2"]
    alive_only = ref["alive"] & ~ref["f64"]["fwd"][4]
    ref["amp_image"] = ref["amp"] * fc.image_amplification(ref["f64"]["fwd"][:4] + [ref["alive"]])
    ref["died_at"] = fc.died_at(ref["f64"]["stk"])
    assert int(alive_only.sum()) > 20 and not ref["f64"]["fwd"][5].any()
    tag = f"no-back {variant} {output} {mode}"
    got = run(lenses, output, mode, allow=False)
    gb = lens_of(got, 0)
    ok_g = gb["fwd"][4]
    assert not gb["fwd"][5].any(), f"{tag}: a backward flag although such rays are not allowed"
    differ = int((ok_g != ref["f64"]["fwd"][4]).sum())
    assert differ <= 2 + 2 * int((ref["f32"]["fwd"][4] != ref["f64"]["fwd"][4]).sum()), f"{tag}: ok differs on {differ} rays"
    print(check_lens(tag, gb, ref, variant, mode, allow=False))
    mine = (gb["flags"] != 0) & ~ok_g
    assert int((mine != alive_only).sum()) <= 2 and (gb["fwd"][1][mine] != 0).any(), tag
    stk = got["stk"] if output != "pensum" else run(lenses, "pen", mode, allow=False)["stk"]
    check_moments(tag, got, stk)
    m = got["moments"]
    assert (m[:, 0] != m[:, 1]).all(), f"{tag}: column 1 does not follow ok"


# ------------------------------------------------------------------------------------------------------------------
# CPU guard: the launch plan puts every shape where the table says (the full premises: test_fwd_cases_cpu.py)
# ------------------------------------------------------------------------------------------------------------------

def test_shapes_land_on_the_expected_plans():
    for (name, P), want in fc.EXPECT.items():
        B, F, W, _ = fc.SHAPES[name]
        assert fc.plan_of(B, F, W, P) == want, (name, P)
