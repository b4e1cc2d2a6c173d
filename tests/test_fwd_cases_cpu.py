"""
The premises of tests/fwd_cases.py, from the oracle and the sources alone (no GPU): the launch plans the shapes are meant to
reach, the kernel each call runs, what the unfiltered fans contain, how few rays the reference itself leaves out, the moment
helper against the oracle's closed forms, and -- the point of a gate -- that evaluations with one index or one term wrong miss
it by two orders of magnitude on every case.
"""
import os
import re

import pytest
import torch

import fwd_cases as fc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "torchoptics_amd", "csrc")
MISS = 100.0                        # a wrong evaluation misses its gate by at least this factor at its worst ray


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


# ------------------------------------------------------------------------------------------------------------------
# plans and kernels
# ------------------------------------------------------------------------------------------------------------------

def test_plan_mirror_lands_every_shape_on_expect():
    api = _read("tl_api.hip")
    m = re.search(r'env_int\("TL_FWD_BLOCKS", (\d+)\), rmax = env_int\("TL_FWD_RMAX", (\d+)\)', api)
    n = re.search(r'env_int\("TL_PLAN_FEW", (\d+)\), rwant = env_int\("TL_PLAN_R", (\d+)\)', api)
    assert m and n, "plan_fwd's defaults moved"
    assert fc.FWD_PLAN == dict(cap=int(m.group(1)), rmax=int(m.group(2)), few=int(n.group(1)), rwant=int(n.group(2)))
    assert {(name, P) for name, P, _, _ in fc.CASES} == set(fc.EXPECT)
    for (name, P), want in fc.EXPECT.items():
        B, F, W, _ = fc.SHAPES[name]
        assert fc.plan_of(B, F, W, P) == want, (name, P, fc.plan_of(B, F, W, P))
    assert fc.plan_of(1, 1, 1, 33101) == fc.ALONE
    # the ragged last chunks, and what two rays per lane make of the shares: one round, a full one, a full and a half one
    assert 22101 % 256 == 85 and 33101 % 256 == 77
    assert {-(-r // 2) for r in fc.EXPECT[("r2", 22101)][2]} == {1} and {r % 2 for r in fc.EXPECT[("r3", 33101)][2]} == {0, 1}
    for name in ("TL_FWD_BLOCKS", "TL_FWD_RMAX", "TL_PLAN_FEW", "TL_PLAN_R"):
        assert name not in os.environ, f"{name} is set: the plans of this table are the defaults'"


def _launch_fwd_chain(fast):
    """[(condition, kernels)] of launch_fwd's `if` chain as the preprocessor leaves it for TL_FAST = `fast`."""
    src = _read("tl_kernels.inc")
    body = src[src.index("static int launch_fwd("):]
    body = body[:body.index("#undef TL_FWD")]
    lines, keep = [], [True]
    for ln in body.splitlines():
        s = ln.strip()
        if s.startswith("#if TL_FAST"):
            keep.append(fast)
        elif s.startswith("#else") and len(keep) > 1:
            keep[-1] = not keep[-1]
        elif s.startswith("#endif") and len(keep) > 1:
            keep.pop()
        elif all(keep) and not s.startswith("//"):
            lines.append(ln.split("//")[0])
    text = "\n".join(lines)
    text = text[text.index("if (p.aggregate"):]
    chain = []
    for part in re.split(r"\belse\b", text):
        cond = re.match(r"\s*if \((.*?)\) (?:TL_FWD|\{|hipLaunch)", part, re.S)
        names = []
        for m in re.finditer(r"TL_FWD\((\w+), (\w+), (\w+)\)|trace_fwd_kernel<(\w+), (\w+), (\w+)>|(trace_fwd_plain_kernel<2>)", part):
            g = m.groups()
            names.append(g[6] if g[6] else "trace_fwd_kernel<%s, %s, %s>" % (g[0:3] if g[0] else g[3:6]))
        assert names, part
        chain.append((cond.group(1) if cond else None, tuple(names)))
    return chain


def test_kernel_table_matches_launch_fwd():
    seen = set()
    for mode in fc.MODES:
        chain = _launch_fwd_chain(mode == "fast")
        assert chain[-1][0] is None and all(c is not None for c, _ in chain[:-1]), chain
        for variant in fc.VARIANTS:
            for output in fc.OUTPUTS:
                env = dict(asph=variant == "asph", wopd=output == "opd", agg=output in ("pen", "pensum"))
                for cond, names in chain:
                    if cond is None or eval(cond.replace("p.aggregate", "agg").replace("&&", "and"), {}, env):
                        break
                assert fc.KERNELS[(variant, output, mode)] == names, (variant, output, mode, names)
                seen |= set(names)
    assert seen == fc.ALL_FWD_KERNELS and len(seen) == 7
    # every (variant, output, mode) is run by a case: `main` has both variants at every row count
    assert {v for _, _, _, v in fc.CASES} == set(fc.VARIANTS)
    # what the source instantiates and nothing else
    src = _read("tl_kernels.inc")
    assert "trace_fwd_plain_kernel<2>" in src and not re.search(r"trace_fwd_plain_kernel<[^2R]", src)


# ------------------------------------------------------------------------------------------------------------------
# what the fans contain, and how little the reference leaves out
# ------------------------------------------------------------------------------------------------------------------

def _case_stats(case):
    name, P, S, v = case
    B = fc.SHAPES[name][0]
    tot = dict(n=0, dead=0, back=0, flag2=0, near=0, left=0)
    for b in range(B):
        r = fc.reference(name, P, S, v, b)
        ok = r["f64"]["fwd"][4]
        tot["n"] += ok.numel()
        tot["dead"] += int((~ok).sum())
        tot["back"] += int(r["f64"]["fwd"][5].sum())
        tot["flag2"] += int((r["flags"] == 2).sum())
        tot["near"] += int(r["near"].sum())
        tot["left"] += fc.rays_differing(r["f32"], r)
    return tot


@pytest.mark.parametrize("case", fc.CASES, ids=lambda c: "%s-P%d-S%d-%s" % c)
def test_case_premises_and_wrong_evaluations(case):
    """One pass per case, so that the large shapes' references are built once and dropped."""
    name, P, S, v = case
    st = _case_stats(case)
    small = name == "edge" and P < 255
    if not small:
        assert st["dead"] > 0 and st["back"] > 0, (case, st)
        assert st["dead"] < 0.05 * st["n"], (case, st)
    if (name == "main" and S >= 5) or name in ("r2", "r3"):
        assert st["flag2"] >= 1, f"{case}: no ill-conditioned live ray ({st})"
    # the reference alone: what it would leave out of a comparison
    assert st["left"] <= fc.LEFT_OUT_CAP * st["n"], f"{case}: the fp32 oracle dies elsewhere on {st['left']} of {st['n']} rays"
    assert st["near"] <= fc.LEFT_OUT_CAP * st["n"], f"{case}: {st['near']} of {st['n']} rays near the flag's threshold"
    for b in range(fc.SHAPES[name][0]):
        _helper_matches_the_oracles_closed_forms(case, b)
    for what, miss in wrong_evaluations(case):
        assert miss >= MISS, f"{case}: '{what}' misses its gate by {miss:.1f} x only"
    if name != "main":
        fc.free(name)


def _helper_matches_the_oracles_closed_forms(case, b):
    from oracle import trace_oracle as orc
    name, P, S, v = case
    r = fc.reference(name, P, S, v, b)
    x, y, _, _, ok, back = r["f32"]["fwd"]
    m, bound = fc.moments_of(x, y, ok, back, r["flags"], r["f32"]["stk"])
    want = orc.spot_moments(y, ok)
    assert m.shape == (y.shape[1], 10) and ((m[:, :4] - want).abs() <= 2 * bound[:, :4]).all(), case
    assert torch.equal(m[:, 7], back.double().sum(dim=(2, 3))[0]) and torch.equal(m[:, 9], (r["flags"] == 2).double().sum(dim=(2, 3))[0])
    stacks = {key: list(r["f32"]["stk"][j]) for j, key in enumerate(("z_RELU", "theta_norm", "theta_prime_norm"))}
    q = float(orc.penalty_from_stacks(stacks, S)) * S
    # the oracle divides by S and sums in fp32 (pairwise): log2(n) + 2 roundings of 2^-24
    n = y[0].numel()
    assert abs(float(m[:, 8].sum()) - q) <= (n.bit_length() + 2) * 2.0 ** -24 * abs(q), (case, float(m[:, 8].sum()), q)


# ------------------------------------------------------------------------------------------------------------------
# wrong evaluations
# ------------------------------------------------------------------------------------------------------------------

def _miss(run, ref, names):
    rt = fc.ratios(run, ref, 1.0, fc.C)
    return max(rt[n] for n in names if n in rt)


def wrong_evaluations(case):
    """(what, factor by which it misses the strict gate it is held to, or inf where it breaks an equality) for every wrong
    evaluation that applies to the case.  (The fast mode's per-ray gate is K_FAST = 10 times as wide, so there the factor
    is a tenth; the moment sums and the equalities are the same in both modes.)"""
    name, P, S, v = case
    B, F, W, _ = fc.SHAPES[name]
    lenses = fc.lens(name, P, S, v)
    inf = float("inf")
    out = []
    rays = ("x", "y", "cx", "cy", "opd")
    if B > 1:
        for b in range(B):
            ref = fc.reference(name, P, S, v, b)
            wrong = fc.oracle_run(lenses[b], torch.float64, c=lenses[(b + 1) % B]["c"])
            out.append((f"lens {(b + 1) % B}'s c for lens {b}", _miss(wrong, ref, rays)))
    b = 1 if B > 1 else 0
    ref, a = fc.reference(name, P, S, v, b), lenses[b]
    f64 = ref["f64"]
    alive = int(f64["fwd"][4].sum())
    if alive:
        if F > 1:
            out.append(("field f+1's cy", _miss(fc.oracle_run(a, torch.float64, cy=a["cy"].roll(-1, 1)), ref, rays)))
        out.append(("wavelength w+1's mu", _miss(fc.oracle_run(a, torch.float64, mu=a["mu"].roll(-1, 3)), ref, rays)))
    if S > 1:
        out.append(("stack row k read as k+1", _miss(dict(f64, stk=f64["stk"].roll(-1, 1)), ref, ("zrelu", "theta", "thetap"))))
    out.append(("theta and theta' exchanged", _miss(dict(f64, stk=f64["stk"][[0, 2, 1]]), ref, ("theta", "thetap"))))
    if f64["hits"] is not None and f64["hits"].shape[0] > 1 and alive:
        out.append(("hit slot j+1 for j", _miss(dict(f64, hits=f64["hits"].roll(-1, 0)), ref, ("hits",))))
    # the moments, from the fp32 oracle's outputs as the kernel's stand-in
    x, y, _, _, ok, back = ref["f32"]["fwd"]
    stk = ref["f32"]["stk"]
    m, bound = fc.moments_of(x, y, ok, back, ref["flags"], stk)

    def moments_miss(m2, cols):
        worst = 0.0
        for j in cols:
            if j in fc.COUNTS:
                worst = max(worst, inf if not torch.equal(m2[:, j], m[:, j]) else 0.0)
            else:
                worst = max(worst, float(((m2[:, j] - m[:, j]).abs() / bound[:, j].clamp(min=1e-300)).max()))
        return worst
    if ok[:, :, -1].any():
        dup = lambda q: torch.cat((q, q[:, :, -1:]), dim=2)      # noqa: E731
        m2, _ = fc.moments_of(dup(x), dup(y), dup(ok), dup(back))
        out.append(("the clamped duplicate of the last point counted", moments_miss(m2, (0, 1, 2, 3))))
    if alive:
        m2, _ = fc.moments_of(x, y, ok, back, ref["flags"], torch.stack((torch.zeros_like(stk[0]), stk[1], stk[2])))
        out.append(("sum Q without z_RELU", moments_miss(m2, (8,))))
    return out


def test_flags_follow_alive_where_backward_rays_are_not_allowed():
    """allow_backward_rays=False on the 5-row lens: rays that turn back at the image plane lose `ok` and nothing else.
    Flags taken behind that test instead of before it break the flag comparison on each of them."""
    for v in ("sph",):
        a = fc.lens("main", 777, 5, v)[0]
        o = fc.oracle_run(a, torch.float64, False)
        alive, _, flags, _ = fc.conditioning(o["stk"])
        only = alive & ~o["fwd"][4]
        assert int(only.sum()) > 20 and (o["fwd"][1][only] != 0).all()
        wrong = torch.where(o["fwd"][4], flags, torch.zeros_like(flags))
        assert int((wrong != flags).sum()) == int(only.sum())
    back = fc.reference("main", 777, 5, "sph")["f64"]["fwd"][5]
    assert int(back.sum()) == 723                 # (allowed, they are flagged: on the way and at the image plane)


def test_c_is_four_times_the_oracles_own_ratio():
    """C against the measurement on `main` and `edge` (the large shapes: `python tests/fwd_cases.py`, 25 s): no case may
    exceed the recorded maxima, and C is 4 x them, not below 1."""
    assert fc.C == {n: max(1.0, 4.0 * v) for n, v in fc.C_MEASURED.items()} and set(fc.C) == set(fc.TOL)
    worst = fc.measure([c for c in fc.CASES if c[0] in ("main", "edge")], out=lambda s: None)
    for n, v in worst.items():
        assert v <= fc.C_MEASURED[n] * (1 + 1e-3), (n, v)
