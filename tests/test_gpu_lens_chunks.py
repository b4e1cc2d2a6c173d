"""
trace_skew of a lens batch above one launch's 65 535 (lens, field, wavelength) rows, traced in lens chunks and joined
(ray_tracing._trace_skew_in_lens_chunks), beyond the one configuration test_gpu_batch.py holds it for: per-lens kappa [B,S],
poly [B,S,4] and a surf_kind tensor, the optical path length with n_index [B,1,1,W,S+1], aggregate=True (the three per-surface
stacks joined, a loss that reads one stack row), the x-moments in the rebuilt spot tag -- on both host chains.

Method (that of test_batch_above_the_grid_row_limit_is_traced_in_lens_chunks): the three padded lenses of fixture G11 cycled
with a 1e-3 jitter, F = 3, W = 3, B = 7 300, P = 16 (65 700 rows, 1.05 M rays: two chunks of 7 281 and 19 lenses).  Outputs,
per-lens losses and the gradients to c, t, mu, kappa, poly and n_index of the 16 lenses that straddle the chunk boundary equal,
bit for bit, the same lenses traced as one small batch.  Three of them are held to the fp64 oracle with the gates of
test_gpu_batch.test_batch_with_aspheric_rows_and_opd.  Two more batches guard the rank-based slicing of the chunker against a
coincidence of sizes: a shared kappa [S] whose S = 8 is no other size of the call, and F = B = 148.
"""
import pytest
import torch

from conftest import rel_l2
from test_gpu_batch import _g11

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B_BIG, F, W, P = 7300, 3, 3, 16
NB = 65535 // (F * W)                       # lenses per chunk: 7 281
PROBE = slice(NB - 8, NB + 8)               # straddles the chunk boundary
ORACLE_LENSES = (NB - 1, NB, NB + 1)        # the last lens of chunk 0, the first two of chunk 1


@pytest.fixture(params=("cpp", "python"))
def chain(request):
    from torchoptics_amd import ops
    ops.set_host_chain(request.param)
    yield request.param
    ops.set_host_chain("cpp")


_INPUTS = {}


def _inputs(n_lens, n_fields=F, n_pupil=P):
    """G11's three padded lenses cycled over n_lens with a 1e-3 jitter on c and kappa; one shared fan of n_pupil points; per-lens
    aspheric terms on a real row of each lens, the refractive indices that belong to mu, weights for the path length."""
    key = (n_lens, n_fields, n_pupil)
    if key in _INPUTS:
        return _INPUTS[key]
    g, ins, mask = _g11(DEV)
    S = ins[5].shape[-1]
    idx = torch.arange(n_lens, device=DEV) % 3
    gen = torch.Generator().manual_seed(3)
    jit = (1.0 + 1e-3 * torch.randn(n_lens, generator=gen)).to(DEV)
    kap3, pol3 = torch.zeros(3, S), torch.zeros(3, S, 4)
    kap3[0, 0], kap3[1, 3], kap3[2, 5] = -0.6, 0.4, -1.0
    pol3[0, 0, 0], pol3[2, 5, 1], pol3[1, 3, 0] = 2e-5, -2e-7, -3e-5
    mu = ins[7][idx].contiguous()
    n = [torch.ones(n_lens, 1, 1, W, device=DEV)]
    for k in range(S):
        n.append(n[-1] / mu[..., k])
    a = dict(S=S,
             # (every 256 / n_pupil-th point of lens 0's 16 x 16 polar grid from its sixth: one per ring, off both axes)
             x=ins[0][:1, :1, 5::256 // n_pupil, :1].contiguous(), y=ins[1][:1, :1, 5::256 // n_pupil, :1].contiguous(),
             z=ins[2][idx].contiguous(), cx=torch.zeros(1, 1, 1, 1, device=DEV),
             cy=(ins[4][idx].contiguous() if n_fields == F else torch.linspace(0.0, 0.42, n_fields, device=DEV).reshape(1, -1, 1, 1)),
             c=ins[5][idx] * jit.reshape(-1, 1, 1, 1, 1), t=ins[6][idx].contiguous(), mu=mu, mask=mask[idx].contiguous(),
             kappa=kap3.to(DEV)[idx] * jit.reshape(-1, 1), poly=pol3.to(DEV)[idx].contiguous(),
             kind=((kap3 != 0) | (pol3 != 0).any(dim=-1)).to(DEV)[idx].contiguous(),
             n_index=torch.stack(n, dim=-1),                                              # [n_lens,1,1,W,S+1]
             w_opd=torch.rand(n_lens, n_fields, n_pupil, W, generator=gen).to(DEV))
    _INPUTS[key] = a
    return a


_PER_LENS = ("c", "t", "mu", "kappa", "poly", "n_index")


def _xy_spot_per_lens(y, n_lens):
    """[n_lens] mean over the fields of the 2-D rms spot radius from the fused moments on y (x-moments included), in plain
    elementwise ops: the same bits whatever the batch size."""
    tag = y._tl_spot
    m, n = tag.moments.view(n_lens, -1, tag.moments.shape[-1]), tag.n_pw
    my, mx = m[..., 0] / n, m[..., 4] / n
    var = ((m[..., 2] - 2 * my * m[..., 1] + my * my * m[..., 3]) + (m[..., 6] - 2 * mx * m[..., 5] + mx * mx * m[..., 3])) / n
    r = torch.sqrt(var)
    tot = r[:, 0]
    for f in range(1, r.shape[1]):
        tot = tot + r[:, f]
    return tot / r.shape[1]


def _sum_per_lens(t):
    """[n_lens] sums over (field, pupil, wavelength) for a per-lens LOSS VALUE that is compared bit for bit between batch sizes:
    summed in fp64 and rounded to fp32, so that the order in which a reduction kernel adds the 144 terms (it may depend on the
    batch size) cannot show; its gradient is the constant 1 per element either way."""
    return t.double().sum(dim=(1, 2, 3)).float().double()


def _run(a, sel, kind_of_run, shared_kappa=None):
    """One trace_skew call on the lenses `sel` of `a` and the backward of the sum of the per-lens losses.
    'opd': aspheric rows, the path length, x_moments; 'stacks': aspheric rows, aggregate=True, a loss on one stack row."""
    import torchoptics_amd as ta
    lv = {n: a[n][sel].clone().requires_grad_(True) for n in _PER_LENS}
    n_lens = lv["c"].shape[0]
    cy = a["cy"][sel] if a["cy"].shape[0] > 1 else a["cy"]
    args = (a["x"], a["y"], a["z"][sel], a["cx"], cy, lv["c"], lv["t"], lv["mu"], a["mask"][sel])
    if shared_kappa is not None:
        lv["kappa"], lv["poly"] = shared_kappa
        kw = dict(kappa=lv["kappa"], poly=lv["poly"], surf_kind=[1, 0, 0, 1] + [0] * (a["S"] - 4))
    else:
        kw = dict(kappa=lv["kappa"], poly=lv["poly"], surf_kind=a["kind"][sel])
    if kind_of_run == "opd":
        out = ta.trace_skew(*args, n_index=lv["n_index"], want_opd=True, x_moments=True, **kw)
        assert out[1]._tl_spot.has_x and bool((out[1]._tl_spot.moments[:, 6] > 0).all())
        rms = ta.compute_rms2d_batch(out[0], out[1], out[4])
        loss = rms.double() + _xy_spot_per_lens(out[1], n_lens) + 1e-3 * _sum_per_lens(out[6] * a["w_opd"][sel])
        extra = [out[6]]
    else:
        out = ta.trace_skew(*args, aggregate=True, **kw)
        assert not out[1]._tl_spot.has_x and not bool(out[1]._tl_spot.moments[:, 4:7].any())
        row = out[6]["theta_norm"][2]                                       # one row of one stack, [n_lens,F,P,W]
        assert row.shape == out[0].shape and len(out[6]["z_RELU"]) == a["S"]
        assert out[6].q_per_lens.shape == (n_lens,)
        m8 = out[1]._tl_spot.moments.view(n_lens, -1, 10)[..., 8]           # the fused penalty sums, per lens and field
        q = (m8[:, 0] + m8[:, 1]) + m8[:, 2]
        loss = ta.compute_rms2d_batch(out[0], out[1], out[4]).double() + 0.2 * q / a["S"] + 0.1 * _sum_per_lens(row)
        extra = [torch.stack(out[6][k]) for k in ("z_RELU", "theta_norm", "theta_prime_norm")]      # [S,n_lens,F,P,W]
    loss.sum().backward()
    grads = {n: q.grad for n, q in lv.items() if q.grad is not None}
    return list(out[:6]) + extra, loss.detach(), grads, out


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


@pytest.mark.parametrize("kind_of_run", ("opd", "stacks"))
def test_chunked_batch_equals_the_small_batch_bit_for_bit(chain, kind_of_run):
    from torchoptics_amd import ops
    a = _inputs(B_BIG)
    outs, loss, grads, raw = _run(a, slice(0, B_BIG), kind_of_run)
    assert outs[0].shape == (B_BIG, F, P, W) and torch.isfinite(loss).all()
    # the joined outputs answer for their chunks: the OPD gradient keeps the checkpoint kernel, the penalty term of a 16-point
    # pupil is handed to it as a whole
    assert ops.used_walk_back(raw[0]) is (kind_of_run == "stacks") and ops.backward_route(raw[0]) == "checkpoint"
    outs_s, loss_s, grads_s, raw_s = _run(a, PROBE, kind_of_run)
    assert ops.used_walk_back(raw_s[0]) is ops.used_walk_back(raw[0]) and ops.backward_route(raw_s[0]) == "checkpoint"
    assert _same(loss[PROBE], loss_s), "per-lens losses"
    for i, (big, small) in enumerate(zip(outs, outs_s)):
        lens_axis = 0 if i < 6 or kind_of_run == "opd" else 1
        assert _same(big.narrow(lens_axis, PROBE.start, 16), small), f"output {i}"
    assert set(grads) == set(grads_s) == set(_PER_LENS) - ({"n_index"} if kind_of_run == "stacks" else set())
    for n in grads:
        assert grads[n].shape == a[n].shape and _same(grads[n][PROBE], grads_s[n]), f"d/d{n}"
        assert bool(grads[n][PROBE].any()), f"d/d{n} is all zero on the probe"


def test_chunked_batch_matches_the_fp64_oracle_on_three_lenses():
    """Lenses 7280, 7281, 7282 of the 'opd' run (aspheric rows, path length, x-moments) against trace_skew_general in fp64,
    lens by lens: the gates of test_batch_with_aspheric_rows_and_opd (forward 3e-5, path length 1e-4, gradients 1e-4)."""
    from oracle import trace_oracle as orc
    a = _inputs(B_BIG)
    outs, loss, grads, _ = _run(a, slice(0, B_BIG), "opd")
    worst = 0.0
    for b in ORACLE_LENSES:
        one = lambda n: a[n][b:b + 1].cpu().double()                                           # noqa: E731
        cb, tb = one("c").requires_grad_(True), one("t").requires_grad_(True)
        kb, pb = a["kappa"][b].cpu().double().requires_grad_(True), a["poly"][b].cpu().double().requires_grad_(True)
        o = orc.trace_skew_general(a["x"].cpu().double(), a["y"].cpu().double(), one("z"), a["cx"].cpu().double(), one("cy"), cb, tb,
                                   one("mu"), a["mask"][b:b + 1].cpu(), kb, pb, [int(v) for v in a["kind"][b]],
                                   n_index=one("n_index"))
        assert o[4].all() and torch.equal(o[4], outs[4][b:b + 1].cpu())
        for i, tol in ((0, 3e-5), (1, 3e-5), (6, 1e-4)):
            assert (o[i] - outs[i][b:b + 1].cpu().double()).abs().max().item() <= tol, (b, i)
        n = P * W
        mx, my = o[0].sum(dim=(2, 3), keepdim=True) / n, o[1].sum(dim=(2, 3), keepdim=True) / n
        xy = torch.sqrt((((o[0] - mx) ** 2 + (o[1] - my) ** 2).sum(dim=(2, 3))) / n).mean()
        lb = orc.compute_rms2d(o[0], o[1], o[4]) + xy + 1e-3 * (o[6] * a["w_opd"][b:b + 1].cpu().double()).sum()
        lb.backward()
        for name, got, want in (("c", grads["c"][b], cb.grad[0]), ("t", grads["t"][b], tb.grad[0]),
                                ("kappa", grads["kappa"][b], kb.grad), ("poly", grads["poly"][b], pb.grad)):
            if want.abs().max() == 0:
                assert got.abs().max().item() == 0, (b, name)
                continue
            e = rel_l2(got.cpu().numpy(), want.numpy())
            worst = max(worst, e / 1e-4)
            assert e <= 1e-4, (b, name, e)
    print(f"CHUNKS opd run, lenses {ORACLE_LENSES} vs the fp64 oracle: worst error over gate {worst:.2f}")


def test_shared_kappa_whose_length_is_no_other_size_of_the_call(chain):
    """kappa [S], poly [S,4] and surf_kind as a list, shared by all 7 300 lenses: S = 8 is neither B, F, W nor P, so nothing
    can slice them by mistake.  Per-lens results equal the small batch's bit for bit; the shared gradient has the leaf's shape
    and is the per-lens gradients' sum to the rounding of that fp32 sum (B 2^-24 sum |g_b|: every term rounded once)."""
    a = _inputs(B_BIG)
    S = a["S"]
    assert S not in (B_BIG, F, W, P, NB, 16)

    def shared():
        kap = torch.zeros(S, device=DEV)
        pol = torch.zeros(S, 4, device=DEV)
        kap[0], kap[3], pol[0, 0], pol[3, 1] = -0.6, 0.4, 2e-5, -2e-7
        return kap.requires_grad_(True), pol.requires_grad_(True)
    outs, loss, grads, _ = _run(a, slice(0, B_BIG), "opd", shared())
    outs_s, loss_s, grads_s, _ = _run(a, PROBE, "opd", shared())
    assert _same(loss[PROBE], loss_s)
    for i, (big, small) in enumerate(zip(outs, outs_s)):
        assert _same(big[PROBE], small), f"output {i}"
    for n in ("c", "t", "mu", "n_index"):
        assert _same(grads[n][PROBE], grads_s[n]), f"d/d{n}"
    assert grads["kappa"].shape == (S,) and grads["poly"].shape == (S, 4)
    # the same lenses with the shared values spelled out per lens: [B,S], [B,S,4]
    kap, pol = shared()
    per = dict(a, kappa=kap.detach().expand(B_BIG, S).contiguous(), poly=pol.detach().expand(B_BIG, S, 4).contiguous(),
               kind=torch.tensor([1, 0, 0, 1] + [0] * (S - 4), dtype=torch.bool, device=DEV).expand(B_BIG, S).contiguous())
    _, loss_p, grads_p, _ = _run(per, slice(0, B_BIG), "opd")
    assert _same(loss_p, loss)
    for n in ("kappa", "poly"):
        want = grads_p[n].double().sum(dim=0)
        bound = B_BIG * 2.0 ** -24 * grads_p[n].double().abs().sum(dim=0)
        assert bool(((grads[n].double() - want).abs() <= bound).all()) and bool(grads[n].any()), n


def test_as_many_fields_as_lenses(chain):
    """F = B = 148 (65 712 rows: chunks of 147 lenses and of one): cy [1,F,1,1] has the batch's length in dim 1 and must not be
    cut; the lone lens of the last chunk is a B = 1 trace."""
    n = 148
    a = _inputs(n, n_fields=n, n_pupil=4)
    assert a["cy"].shape == (1, n, 1, 1) and n * n * W > 65535
    outs, loss, grads, _ = _run(a, slice(0, n), "opd")
    assert outs[0].shape == (n, n, 4, W)
    probe = slice(n - 8, n)
    outs_s, loss_s, grads_s, _ = _run(a, probe, "opd")
    assert _same(loss[probe], loss_s)
    for i, (big, small) in enumerate(zip(outs, outs_s)):
        assert _same(big[probe], small), f"output {i}"
    for name in grads:
        assert _same(grads[name][probe], grads_s[name]), f"d/d{name}"
