"""tl_pupil_position (pupil_position_kernel) at the C ABI against tests/pupil_ref.py: the strict value bit for bit against
the numpy fp32 tree for every K = 1 .. TL_MAX_SURFACES -- odd counts, whose carry no fixture reaches, included --, the fast
value and every element of the gradients against float64 within one fp32 rounding plus the counted fp64 allowance, batches
of 1, 64, 65 and 130 lenses (a second and a third block, a partly filled one), a padded batch, and the backward-only call.
Run with -s for the PUPIL-ACC lines (profiles/aim_accuracy.txt)."""
import numpy as np
import pytest
import torch

import pupil_ref as PR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BATCHES = (1, 64, 65, 130)
PADDED_B = 65                                       # the batch whose rows behind a per-lens stop are identity


def _call(c, t, n, mode, g_z=None, want_z=True):
    """tl_pupil_position on numpy inputs; returns (z or None, g_c, g_t, g_n or None) as numpy.  Every output is NaN
    beforehand."""
    from torchoptics_amd import _lib, ops
    B, K = c.shape
    dev = torch.device(DEV)
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=DEV)
    cd, td, nd = up(c), up(t), up(n)
    z = nan(B) if want_z else None
    gz = None if g_z is None else up(g_z)
    g = [nan(B, K), nan(B, K), nan(B, K + 1)] if g_z is not None else [None] * 3
    P = _lib.ptr
    with ops._on_device(dev):
        rc = _lib.lib().tl_pupil_position(0, B, K, P(cd), P(td), P(nd), P(z), P(gz), P(g[0]), P(g[1]), P(g[2]), mode,
                                          ops._stream_ptr(dev))
    _lib.check(rc, "tl_pupil_position")
    torch.cuda.synchronize()
    return tuple(None if q is None else q.cpu().numpy() for q in (z, *g))


def _worst(got, want, limit):
    assert got.shape == want.shape and np.isfinite(got).all(), "an element is not finite (or was never written)"
    err = np.abs(got.astype(np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(err == 0, 0.0, err / limit).max())


@pytest.mark.parametrize("K", range(1, 33))
def test_pupil_position_values_and_gradients(K):
    from torchoptics_amd import _lib
    assert K <= _lib.TL_MAX_SURFACES
    worst = {"z_fast": 0.0, "g_c": 0.0, "g_t": 0.0, "g_n": 0.0}
    for B in BATCHES:
        c, t, n = PR.seeded_front(K, B, 3000 + 40 * K + B, padded=B == PADDED_B)
        if B == PADDED_B and K >= 3:
            assert (c[:, -1] == 0).any() and (n[:, 1:][c == 0] == 1).all() and (t[c == 0] == 0).all()
        grads = B == 65
        g_z = (np.linspace(-1.5, 2.0, B) * np.where(np.arange(B) % 3 == 0, -1.0, 1.0)).astype(np.float32) if grads else None
        # strict: the fp32 tree, bit for bit
        zs, *gs = _call(c, t, n, _lib.MODE_STRICT, g_z)
        assert np.array_equal(zs.view(np.int32), PR.tree32(c, t, n).view(np.int32)), (K, B)
        # fast: float64 rounded once
        zf, *gf = _call(c, t, n, _lib.MODE_FAST, g_z)
        ref = PR.kernel_order(c, t, n, np.zeros(B) if g_z is None else g_z)
        z64 = PR.fast64(c, t, n)
        worst["z_fast"] = max(worst["z_fast"], _worst(zf, z64, PR.U32 * (np.abs(z64) + 2 * ref[0].e) + 2 * ref[0].e))
        if not grads:
            continue
        _, *g64 = PR.grads64(c, t, n, g_z)
        for mode, got in ((_lib.MODE_STRICT, gs), (_lib.MODE_FAST, gf)):
            for name, g, want, errs in zip(("g_c", "g_t", "g_n"), got, g64, ref[1:]):
                e = 2 * PR.stacked(errs)[1]
                worst[name] = max(worst[name], _worst(g, want, PR.U32 * (np.abs(want) + e) + e))
            # the backward-only call, as ops.pupil_position's backward makes it: the same gradient bits
            none, *only = _call(c, t, n, mode, g_z, want_z=False)
            assert none is None
            for a, b in zip(only, got):
                assert np.isfinite(a).all() and np.array_equal(a.view(np.int32), b.view(np.int32))
    print(f"PUPIL-ACC K={K}: strict z bit for bit (B {BATCHES}); largest error / bound  z_fast {worst['z_fast']:.3f} "
          f"g_c {worst['g_c']:.3f} g_t {worst['g_t']:.3f} g_n {worst['g_n']:.3f}")
    assert max(worst.values()) <= 1, (K, worst)
