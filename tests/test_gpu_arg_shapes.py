"""
The shapes trace_skew takes for its extension arguments, the same on both host chains (its docstring):

    kappa    [S], [1,S], [B,S]          poly    [S,4], [1,S,4], [B,S,4]          n_index    [1|B,1,1,W,S+1]

On fixture G11 (B = 3 padded lenses, F = 3, P = 256, W = 3) every accepted form is traced and differentiated: the gradient has
the leaf's shape, a shared form's gradient is the per-lens form's summed over the lenses -- both held to the fp64 oracle
(oracle.trace_skew_general lens by lens) with the gates this configuration already has: 1e-4 norm-relative for kappa and poly
(test_gpu_batch.test_batch_with_aspheric_rows_and_opd), 2e-5 + 2 x the oracle's own fp32-vs-fp64 distance for n_index
(test_gpu_asphere.test_gradient_through_the_optical_path_length) -- and the two chains give equal bits.  Any other shape is a
ValueError that names the argument, raised by the call itself and never inside backward (the C++ chain used to trace a kappa
[B,1,1,1,S] and then throw from at::sum_to when the gradient was summed back).
"""
import pytest
import torch

from conftest import rel_l2
from test_gpu_batch import _g11

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = 3
FORMS = ("flat", "one", "per_lens")          # kappa [S] | [1,S] | [B,S]; poly alike; n_index [1,...] | [1,...] | [B,...]


def _values():
    """The aspheric terms (rows 0 and 3: real rows of all three lenses) and the indices of lens 0, shared by every lens."""
    g, ins, mask = _g11("cpu")
    S, W = ins[5].shape[-1], ins[7].shape[3]
    kap, pol = torch.zeros(S), torch.zeros(S, 4)
    kap[0], kap[3], pol[0, 0], pol[3, 1] = -0.6, 0.4, 2e-5, -2e-7
    n = [torch.ones(1, 1, 1, W)]
    for k in range(S):
        n.append(n[-1] / ins[7][:1, ..., k])
    w_opd = torch.rand(B, 3, 256, W, generator=torch.Generator().manual_seed(11))
    return ins, mask, kap, pol, torch.stack(n, dim=-1), w_opd, [1, 0, 0, 1] + [0] * (S - 4)


def _shaped(form, kap, pol, n):
    S = kap.shape[0]
    if form == "flat":
        return kap.clone(), pol.clone(), n.clone()
    if form == "one":
        return kap.reshape(1, S).clone(), pol.reshape(1, S, 4).clone(), n.clone()
    return kap.expand(B, S).clone(), pol.expand(B, S, 4).clone(), n.expand(B, *n.shape[1:]).clone()


_REF = {}


def _oracle():
    """Per lens: d loss_b / d (kappa, poly, n_index) in fp32 (IEEE sqrt) and fp64, loss_b = rms_b + 1e-3 sum(w opd)."""
    if _REF:
        return _REF
    from oracle import trace_oracle as orc
    ins, mask, kap, pol, n, w_opd, kind = _values()
    for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
        per = []
        for b in range(B):
            one = [a[b:b + 1].to(dt) if a.shape[0] == B else a.to(dt) for a in ins]
            lv = [q.to(dt).clone().requires_grad_(True) for q in (kap, pol, n)]
            o = orc.trace_skew_general(*one, mask[b:b + 1], lv[0], lv[1], kind, n_index=lv[2], ieee_sqrt=(dt == torch.float32))
            (orc.compute_rms2d(o[0], o[1], o[4]) + 1e-3 * (o[6] * w_opd[b:b + 1].to(dt)).sum()).backward()
            per.append([q.grad.double() for q in lv])
        _REF[tag] = [torch.stack([p[i] for p in per]) for i in range(3)]         # [B, *leaf]
    return _REF


def _gpu(form, chain):
    import torchoptics_amd as ta
    from torchoptics_amd import ops
    ins, mask, kap, pol, n, w_opd, kind = _values()
    lv = [q.to(DEV).requires_grad_(True) for q in _shaped(form, kap, pol, n)]
    ops.set_host_chain(chain)
    try:
        out = ta.trace_skew(*[a.to(DEV) for a in ins], mask.to(DEV), kappa=lv[0], poly=lv[1], surf_kind=kind, n_index=lv[2],
                            want_opd=True)
        (ta.compute_rms2d_batch(out[0], out[1], out[4]).sum() + 1e-3 * (out[6] * w_opd.to(DEV)).sum()).backward()
    finally:
        ops.set_host_chain("cpp")
    return [t.detach().cpu() for t in out[:7]], lv


@pytest.mark.parametrize("form", FORMS)
def test_every_accepted_form_gives_the_leaf_a_gradient_of_its_shape(form):
    ref = _oracle()
    res = {chain: _gpu(form, chain) for chain in ("cpp", "python")}
    for (o1, l1), (o2, l2) in [(res["cpp"], res["python"])]:
        for i, (p, q) in enumerate(zip(o1, o2)):
            assert torch.equal(p, q), f"{form}: output {i} differs between the host chains"
        for name, p, q in zip(("kappa", "poly", "n_index"), l1, l2):
            assert p.grad is not None and p.grad.shape == p.shape, (form, name, None if p.grad is None else p.grad.shape)
            assert q.grad.shape == q.shape and torch.equal(p.grad, q.grad), f"{form}: d/d{name} differs between the host chains"
    worst = 0.0
    for i, name in enumerate(("kappa", "poly", "n_index")):
        got = res["cpp"][1][i].grad.cpu().double()
        w32, w64 = ref["f32"][i], ref["f64"][i]
        if form != "per_lens":                          # a shared form: the sum over the lenses
            w32, w64 = w32.sum(dim=0), w64.sum(dim=0)
        e64, noise = rel_l2(got.numpy(), w64.numpy()), rel_l2(w32.numpy(), w64.numpy())
        gate = 1e-4 if name != "n_index" else 2e-5 + 2 * noise
        worst = max(worst, e64 / gate)
        print(f"SHAPES {form} d/d{name} {tuple(got.shape)}: vs fp64 {e64:.2e}, oracle fp32 itself {noise:.2e}, e64/gate {e64 / gate:.4f}")
        assert e64 <= gate, (form, name, e64, gate)
    print(f"SHAPES {form}: worst error over gate {worst:.4f}")


def _bad_shapes(S, W):
    return [("kappa", (B, 1, 1, 1, S)), ("kappa", (1, 1, 1, 1, S)), ("kappa", (S, 1)), ("kappa", (2, S)), ("kappa", (B * S,)),
            ("poly", (B, 1, 1, 1, S, 4)), ("poly", (S * 4,)), ("poly", (4, S)), ("poly", (2, S, 4)), ("poly", (B, S * 4)),
            ("n_index", (W, S + 1)), ("n_index", (B, W, S + 1)), ("n_index", (1, 1, 1, 1, S + 1)), ("n_index", (2, 1, 1, W, S + 1)),
            ("n_index", (1, 1, W, S + 1)), ("n_index", (1, 1, 1, W, S))]


@pytest.mark.parametrize("chain", ("cpp", "python"))
def test_any_other_shape_is_refused_by_name_at_the_call(chain):
    import torchoptics_amd as ta
    from torchoptics_amd import ops
    ins, mask, kap, pol, n, w_opd, kind = _values()
    S, W = kap.shape[0], n.shape[3]
    dev = [a.to(DEV) for a in ins]
    good = dict(kappa=kap.to(DEV), poly=pol.to(DEV), n_index=n.to(DEV))
    ops.set_host_chain(chain)
    try:
        for name, shape in _bad_shapes(S, W):
            numel = 1
            for d in shape:
                numel *= d
            bad = torch.zeros(numel, device=DEV).reshape(shape).requires_grad_(True)
            kw = dict(good, **{name: bad})
            with pytest.raises(ValueError, match=name):
                ta.trace_skew(*dev, mask.to(DEV), surf_kind=kind, want_opd=True, **kw)
        # the shape the C++ chain used to trace and then fail on in backward
        with pytest.raises(ValueError, match="kappa"):
            ta.trace_skew(*dev, mask.to(DEV), kappa=kap.to(DEV).expand(B, S).reshape(B, 1, 1, 1, S).clone().requires_grad_(True),
                          poly=pol.to(DEV))
        # n_index is only looked at when the path length is asked for
        out = ta.trace_skew(*dev, mask.to(DEV), kappa=good["kappa"], poly=good["poly"], n_index=torch.zeros(2, device=DEV))
        assert len(out) == 6
    finally:
        ops.set_host_chain("cpp")
