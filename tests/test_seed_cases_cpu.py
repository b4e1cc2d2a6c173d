"""
The case table of test_gpu_seed_matrix.py (seed_cases.py) is what it claims -- no GPU.

The GPU tests hold the fp32 backward kernels to the fp64 oracle on turned fans and under dense seeds.  That says something
only if the turned fan keeps what test_gpu_kernel_matrix._fan established (who dies; fp32 and fp64 agreeing on it), if the
oracle's skew path is right (its outputs turn with the fan; its d/dcx, d/dcy agree with finite differences), if every case
carries a d/dcx well above the oracle's own rounding in which the fold of the cz0 adjoint is a large share, and if the
losses hand the kernels the seed pointers they are named after.  These are conditions on the inputs: a lens that fails one
is replaced, the condition stays.
"""
import math

import pytest
import torch

import seed_cases as sc
import test_gpu_kernel_matrix as km
from conftest import rel_l2

_IDS = [f"S{s}-{v}-P{p}" for s, v, p in sc.LENSES]
_BATCH = [(S, v, P, b) for S, v, P in sc.BATCH_LENSES for b in range(len(km.BATCH_W))]


def _ok(a, dt):
    with torch.no_grad():
        return sc.trace(a, dt)[4]


@pytest.mark.parametrize("S,variant,P", sc.LENSES, ids=_IDS)
def test_turned_fan_keeps_the_masks(S, variant, P):
    r = sc.reference(S, variant, P)
    ok64, ok32 = r["f64"]["fwd"][4], r["f32"]["fwd"][4]
    assert torch.equal(ok64, _ok(sc.fan(S, variant, P), torch.float64)), "a ray lives or dies by the turn"
    assert torch.equal(ok32, ok64), f"fp32 and fp64 masks differ on {(ok32 != ok64).sum().item()} rays"
    assert ok64.float().mean().item() > 0.5
    assert S < 3 or not ok64.all(), "no dead rays: dead-ray seeds and the walk-back + checkpoint merge are not reached"


@pytest.mark.parametrize("S,variant,P,b", _BATCH, ids=[f"S{s}-{v}-lens{b}" for s, v, _, b in _BATCH])
def test_batch_lenses_keep_the_masks(S, variant, P, b):
    r = sc.reference(S, variant, P, b)
    ok64, ok32 = r["f64"]["fwd"][4], r["f32"]["fwd"][4]
    assert torch.equal(ok32, ok64), f"fp32 and fp64 masks differ on {(ok32 != ok64).sum().item()} rays"
    assert 0.5 < ok64.float().mean().item() < 1.0


@pytest.mark.parametrize("S,variant,P", sc.LENSES, ids=_IDS)
def test_oracle_outputs_turn_with_the_fan(S, variant, P):
    """fp64: the outputs of the exactly turned fan are the unturned outputs turned by the same matrix (positions to 1e-10 mm,
    cosines to 1e-12).  This pins the oracle's skew path without its autograd."""
    a0 = sc.fan(S, variant, P)
    with torch.no_grad():
        o0 = sc.trace(a0, torch.float64)
        o1 = sc.trace(sc.turned(a0, dtype=torch.float64), torch.float64)
    co, si = math.cos(sc.AZ), math.sin(sc.AZ)
    assert torch.equal(o0[4], o1[4]) and torch.equal(o0[5], o1[5])
    for i, tol in ((0, 1e-10), (2, 1e-12)):
        u0, v0 = o0[i].expand_as(o1[i]), o0[i + 1].expand_as(o1[i + 1])
        assert (o1[i] - (u0 * co + v0 * si)).abs().max().item() <= tol, i
        assert (o1[i + 1] - (v0 * co - u0 * si)).abs().max().item() <= tol, i + 1
    assert o1[0].abs().max().item() > 1e-3 and o1[2].abs().max().item() > 1e-3      # (x and cx are not zero any more)


def test_oracle_cx_cy_gradients_match_finite_differences():
    """d/dcx, d/dcy of the fp64 oracle per field, loss rms+all on the 13-row aspheric lens, against central differences
    with the step and the bound of test_oracle_asphere.py's own check."""
    from oracle import trace_oracle as orc
    r = sc.reference(13, "asph", sc.P_MAIN)
    a, wts = r["args"], r["wts"]
    lv = {n: a[n].double().clone() for n in ("cx", "cy")}

    def loss():
        with torch.no_grad():
            o = sc.trace(a, torch.float64, lv)
            return sc.loss_of("rms+all", o[:4], wts, lambda: orc.compute_rms2d(o[0], o[1], o[4]), ok=o[4]).item()
    h = 1e-7
    for n in ("cx", "cy"):
        g = sc.summed(n, r["f64"]["grads"]["rms+all"][n])
        for f in range(a["cy"].shape[1]):
            base = lv[n][0, f, 0, 0].item()
            lv[n][0, f, 0, 0] = base + h
            lp = loss()
            lv[n][0, f, 0, 0] = base - h
            lm = loss()
            lv[n][0, f, 0, 0] = base
            fd = (lp - lm) / (2 * h)
            assert abs(g[0, f, 0, 0].item() - fd) <= 2e-5 * abs(fd) + 1e-12, (n, f, g[0, f, 0, 0].item(), fd)


def _signal(r, share, tag):
    lines = []
    for loss in r["losses"]:
        g32, g64 = r["f32"]["grads"][loss], r["f64"]["grads"][loss]
        noise = {}
        for n in r["names"]:
            w32, w64 = (sc.summed(n, g[n]) if n in sc.PER_RAY else g[n] for g in (g32, g64))
            noise[n] = rel_l2(w32.numpy(), w64.numpy())
            if n == "z" and sc.LOSSES[loss][0]:
                continue                        # d rms / dz in focus: the per-ray-noise rule of km._grad_errors
            assert noise[n] <= 1e-4, f"{tag} {loss}: the oracle's own fp32 is {noise[n]:.2e} from fp64 in d/d{n}"
        ncx, ncy = (float(sc.summed(n, g64[n]).norm()) for n in ("cx", "cy"))
        assert ncx >= 1e-3 * ncy, f"{tag} {loss}: |g_cx| {ncx:.2e} against |g_cy| {ncy:.2e}"
        for n, factor in (("cx", 100.0), ("cy", 10.0)):
            gate = km._gate("cy", False, noise[n], 1.0)
            assert share[loss][n] >= factor * gate, \
                f"{tag} {loss}: the cz0 fold is {share[loss][n]:.2e} of d/d{n}, gate {gate:.2e}"
        lines.append(f"{tag} {loss}: |g_cx| {ncx:.2e} |g_cy| {ncy:.2e}, fold share cx {share[loss]['cx']:.2e} cy "
                     f"{share[loss]['cy']:.2e}, noise " + ", ".join(f"{n} {v:.1e}" for n, v in noise.items()))
    for line in lines:
        print(line)


@pytest.mark.parametrize("S,variant,P", sc.LENSES, ids=_IDS)
def test_cases_carry_signal(S, variant, P):
    """Per lens and loss: the oracle's own fp32-vs-fp64 distance <= 1e-4 in every parameter (z under the rms has its own
    rule), |g_cx| >= 1e-3 |g_cy|, and a backward without the cz0 fold is >= 100 x the (strict) gate away in d/dcx and
    >= 10 x in d/dcy."""
    _signal(sc.reference(S, variant, P), sc.fold_share(S, variant, P), f"S={S} {variant} P={P}")


@pytest.mark.parametrize("S,variant,P,b", _BATCH, ids=[f"S{s}-{v}-lens{b}" for s, v, _, b in _BATCH])
def test_batch_cases_carry_signal(S, variant, P, b):
    _signal(sc.reference(S, variant, P, b), sc.fold_share(S, variant, P, b), f"batch S={S} {variant} lens {b}")


class _Probe(torch.autograd.Function):
    """Four per-ray outputs and a moments tensor behind set_materialize_grads(False), as the trace node has them."""
    seen = None

    @staticmethod
    def forward(ctx, v):
        ctx.set_materialize_grads(False)
        return v * 1.0, v * 2.0, v * 3.0, v * 4.0, v.sum().reshape(1)

    @staticmethod
    def backward(ctx, gx, gy, gcx, gcy, gmom):
        _Probe.seen = (gmom is not None, sum(bit for bit, g in ((1, gx), (2, gy), (4, gcx), (8, gcy)) if g is not None))
        return None


@pytest.mark.parametrize("loss", sorted(sc.LOSSES))
def test_every_loss_hands_over_the_seed_pointers_it_claims(loss):
    v = torch.ones(1, 2, 5, 3, requires_grad=True)
    x, y, cx, cy, mom = _Probe.apply(v)
    wts = sc.weights(v.shape, 1)
    _Probe.seen = None
    sc.loss_of(loss, (x, y, cx, cy), wts, lambda: mom.sum()).backward()
    assert _Probe.seen == sc.seed_bits(loss)
    want = {"rms+all": (True, 15), "all": (False, 15), "x": (False, 1), "cx": (False, 4), "y+cy": (False, 10)}
    assert sc.seed_bits(loss) == want[loss]


def test_case_table_reaches_every_route():
    invu, buckets, lo, hi, pair = km._instantiated()
    rows = set(sc.ROWS)
    assert {lo - 1, lo, hi, hi + 1, pair - 1, pair} <= rows, (lo, hi, pair, rows)
    assert sum(1 for v in buckets if any(s <= v for s in rows) and any(s > v for s in rows)) >= 2, "three checkpoint buckets"
    assert max(rows) > hi + 1 and 1 < min(rows) < lo               # rolled walk-back on both sides of the unrolled range
    assert {S for S, _, _ in sc.DENSE_LENSES} == {pair - 1, pair}
    assert {S for S, _, _ in sc.BATCH_LENSES} == {pair}
    assert all(lo <= S <= hi for S, _, p in sc.LENSES if p < 256) and any(p < 256 for _, _, p in sc.LENSES)
    assert (16, "asph5", sc.P_MAIN) in sc.LENSES and len(km._asph_rows(16, "asph5")) > 4
    assert all(s in rows for s in sc.XY_ROWS) and min(sc.XY_ROWS) == lo and max(sc.XY_ROWS) == hi + 1
    for S in sc.ROWS:
        assert {(S, v, sc.P_MAIN) for v in ("sph", "asph")} <= set(sc.LENSES)
    assert len(sc.CASES) == len(sc.LENSES) + 4 * len(sc.DENSE_LENSES) and set(sc.DENSE_LOSSES) | {"rms+all"} == set(sc.LOSSES)
