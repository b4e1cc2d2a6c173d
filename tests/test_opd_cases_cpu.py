"""When the reference of the optical-path-length matrix (tests/opd_cases.py) is fit to judge the kernels: no GPU needed.

  * the row counts cover every bucket of tl_bwd_bucket (csrc/tl_common.h) on both sides, S < NS and S == NS in each;
  * every fan loses 1 .. 10 % of its rays, at least one of them in a wave that also holds live rays and, at P = 777, at
    least one in the ragged last chunk;
  * the fp64 oracle's OPD is exactly +0 on dead rays and every reference gradient is finite;
  * for every (case, loss, leaf) the oracle's own fp32-vs-fp64 distance is below the base gate the kernels are judged
    with (test_gpu_kernel_matrix._gate without its noise term; the wavefront loss times its cancellation factor);
  * the cancellation factor the wavefront gates carry is printed per leaf and never exceeds CANCEL_CAP: it is min(factor,
    CANCEL_CAP).  d/dz and d/dt of the variance are structurally above it on every seed -- a shift of the launch plane or
    of a gap lengthens every ray of a fan by almost the same amount, which the zero-sum seeds cancel: 340 .. 54 000 for z,
    up to 212 for t -- so those leaves are judged with a gate tighter than their own cancellation would allow.
"""
import pytest
import torch

import opd_cases as oc
from conftest import rel_l2
from test_gpu_kernel_matrix import _PER_RAY, _gate, _instantiated, _reduce

ALL = [c + (None,) for c in oc.CASES] + [(S, v, oc.P_MAIN, b) for S, v in oc.BATCH_CASES for b in range(len(oc.BATCH_W))]


def _bucket(S, buckets):
    return next(v for v in buckets if S <= v)


def test_rows_cover_every_bucket_on_both_sides():
    buckets = _instantiated()[1]
    rows = set(oc.ROWS)
    assert max(rows) == max(buckets) and 1 in rows
    for v in buckets:
        assert v in rows, f"S == NS never runs in bucket {v}"
        assert v == max(buckets) or v + 1 in rows, f"the row count just past bucket {v} is missing"
        assert any(s < v and _bucket(s, buckets) == v for s in rows), f"S < NS never runs in bucket {v}"
    cases = set(oc.CASES)
    assert all((S, v, oc.P_MAIN) in cases for S in oc.ROWS for v in oc.VARIANTS)
    assert oc.P_MAIN > 2 * 256 and oc.P_MAIN % 256 == 9                      # three chunks and a 9-lane tail
    assert oc.SMALL_P == (200, 64, 63)
    assert all((S, v, P) in cases for S in oc.SMALL_ROWS for v in oc.VARIANTS for P in oc.SMALL_P)
    # the small pupils and the lens batches run S == NS and S < NS / only S < NS (where a shifted column shows)
    assert any(_bucket(S, buckets) > S for S in oc.SMALL_ROWS) and all(_bucket(S, buckets) > S for S in oc.BATCH_ROWS)
    assert all(c in cases for c in oc.HOST_CHAIN_CASES)
    for S in oc.ROWS:
        r = oc._asph_rows(S, "asph")
        assert 0 in r and S - 1 in r
    # both signs of the path weights in half the cases
    assert sum(oc.signed_weights(S, v) for S, v, _ in oc.CASES) * 2 == len(oc.CASES)


@pytest.mark.parametrize("S,variant,P,b", ALL, ids=[oc.case_id(c[:3]) + ("" if c[3] is None else f"-lens{c[3]}") for c in ALL])
def test_reference_is_fit_to_judge(S, variant, P, b):
    r = oc.reference(S, variant, P, b)
    a = r["args"]
    ok64, ok32 = r["f64"]["fwd"][4], r["f32"]["fwd"][4]
    tag = f"S={S} {variant} P={P}" + ("" if b is None else f" lens {b}")
    dead = ~ok64
    frac = dead.float().mean().item()
    assert 0.01 <= frac <= 0.10, f"{tag}: {int(dead.sum())} dead rays of {dead.numel()}"
    # [1,F,P,W]: a wave is 64 consecutive pupil points of one (field, wavelength)
    mixed = False
    for p0 in range(0, P, 64):
        d = dead[:, :, p0:p0 + 64]
        mixed |= bool((d.any(dim=2) & (~d).any(dim=2)).any())
    assert mixed, f"{tag}: no wave holds dead and live rays"
    if P == oc.P_MAIN:
        assert dead[:, :, (P // 256) * 256:].any(), f"{tag}: no dead ray in the ragged last chunk"
    assert (ok64.sum(dim=2) >= 2).all(), f"{tag}: a fan without live rays has no variance"
    for run in ("f64", "f32"):
        opd = r[run]["fwd"][6]
        assert (opd[~r[run]["fwd"][4]] == 0).all() and not torch.signbit(opd[~r[run]["fwd"][4]]).any(), f"{tag}: OPD of dead rays ({run})"
        assert torch.isfinite(opd).all()
    assert (a["w"][dead] != 0).any()
    assert (oc.signed_weights(S, variant) and (a["w"] < 0).any()) or (a["w"] >= 0).all()
    assert torch.isfinite(r["path"]).all() and (r["path"][ok64] > 0).all()
    for loss in oc.LOSSES:
        msg = []
        for n in r["names"]:
            g32, g64 = r["f32"]["grads"][loss][n], r["f64"]["grads"][loss][n]
            assert torch.isfinite(g64).all() and torch.isfinite(g32).all(), f"{tag} {loss}: reference d/d{n} not finite"
            if n in _PER_RAY:
                g32, g64 = _reduce(n, g32, None), _reduce(n, g64, None)
            assert g64.abs().max().item() > 0, f"{tag} {loss}: d/d{n} is zero, a relative gate says nothing"
            noise = rel_l2(g32.numpy(), g64.numpy())
            cn = oc.gate_cancel(r, loss, n)
            base = _gate(n, False, noise, 1.0) - 2 * noise
            msg.append(f"{n} {noise:.1e}" + (f"/x{r['cancel'][loss][n]:.1f}" if loss == "wavefront" else ""))
            assert noise < base * cn, f"{tag} {loss} d/d{n}: the oracle's own fp32 is {noise:.2e} from fp64, base gate {base * cn:.2e}"
        print(f"OPD-REF {tag} {loss}: dead {int(dead.sum())}/{dead.numel()} | noise[/cancellation] " + ", ".join(msg))
