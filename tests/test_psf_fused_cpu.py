"""The fused PSF (tl_psf_accumulate / tl_psf_accumulate_bwd, metrics.compute_psf(fused=True)): what can be checked without a
GPU -- the three entry points are declared, bound and exported with the ABI version unchanged; they refuse bad arguments
before any HIP call; the Python keyword raises instead of falling back; the default path is untouched."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_psf_cpu import _fan

from torchoptics_amd import _lib, metrics

NAMES = ("tl_psf_workspace_bytes", "tl_psf_accumulate", "tl_psf_accumulate_bwd")
EINVAL, EWORKSPACE = -1, -3                 # TL_EINVAL, TL_EWORKSPACE (include/tl_trace.h)
ONE = C.c_void_p(8)                         # any non-NULL pointer: never dereferenced on the paths taken here


def test_entry_points_are_declared_bound_and_exported_and_the_abi_version_stays():
    hdr = open(os.path.join(ROOT, "include", "tl_trace.h")).read()
    declared = set(re.findall(r"\b(tl_[a-z0-9_]+)\s*\(", hdr))
    dll = _lib.lib()
    for name in NAMES:
        assert name in declared and name in _lib.EXPORTS and hasattr(dll, name), name
    assert dll.tl_version() == 15 == _lib.TL_ABI_VERSION
    assert int(re.search(r"#define TL_ABI_VERSION (\d+)", hdr).group(1)) == 15
    assert C.sizeof(_lib.tl_problem) == dll.tl_problem_size() == 248


def _fwd(dll, G=3, W=3, R=1000, x=ONE, y=ONE, weight=None, ok=None, xp=ONE, yp=ONE, yc=ONE, nxh=11, ny=21, hist=ONE,
         ws=ONE, ws_bytes=1 << 30):
    return dll.tl_psf_accumulate(0, G, W, R, x, y, weight, ok, W * R, R, xp, yp, yc, nxh, ny, 0.0, -10.0, hist, ws, ws_bytes, None)


def _bwd(dll, G=3, W=3, R=1000, x=ONE, y=ONE, weight=None, ok=None, xp=ONE, yp=ONE, yc=ONE, nxh=11, ny=21, g_hist=ONE,
         gx=ONE, gy=ONE, ws=ONE, ws_bytes=1 << 30):
    return dll.tl_psf_accumulate_bwd(0, G, W, R, x, y, weight, ok, W * R, R, xp, yp, yc, nxh, ny, 0.0, -10.0, g_hist, gx, gy,
                                     None, None, None, ws, ws_bytes, None)


BAD = [dict(x=None), dict(y=None), dict(xp=None), dict(yp=None), dict(yc=None),          # null required pointer
       dict(nxh=0), dict(nxh=33), dict(ny=0), dict(ny=33),                                # bins outside 1..32
       dict(G=256, W=256),                                                                # G W > 65535
       dict(R=0), dict(R=-5),                                                             # R < 1
       dict(weight=ONE, ok=ONE)]                                                          # both weight and ok


@pytest.mark.parametrize("bad", BAD, ids=lambda d: ",".join(f"{k}={'NULL' if v is None else getattr(v, 'value', v)}" for k, v in d.items()))
def test_bad_arguments_are_refused_before_any_hip_call(bad):
    dll = _lib.lib()
    for call, name in ((_fwd, b"tl_psf_accumulate"), (_bwd, b"tl_psf_accumulate_bwd")):
        dll.tl_unsup_loss(0, 0, 3, 100.0, ONE, None, 7.0, 0.2, ONE, ONE, ONE, ONE, None)       # another call's message first
        assert call(dll, **bad) == EINVAL, (name, bad)
        msg = dll.tl_last_error()
        assert name + b":" in msg, msg
    assert _fwd(dll, hist=None) == EINVAL and b"tl_psf_accumulate" in dll.tl_last_error()
    for k in ("g_hist", "gx", "gy"):
        assert _bwd(dll, **{k: None}) == EINVAL and b"tl_psf_accumulate_bwd" in dll.tl_last_error()


def test_workspace_size_grows_with_the_fan_and_a_small_workspace_is_refused():
    dll = _lib.lib()
    sizes = [dll.tl_psf_workspace_bytes(3, 3, R, 11, 21) for R in (1 << 8, 1 << 12, 1 << 16, 1 << 20, 1 << 24)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0] > 0, sizes
    one = [dll.tl_psf_workspace_bytes(1, 1, R, 16, 32) for R in (1 << 10, 1 << 20)]
    assert one[1] > one[0] > 0
    assert sizes[-1] < (9 << 24) // 2, "the workspace must stay far below one byte per ray"
    for bad in ((0, 3, 100, 11, 21), (3, 3, 0, 11, 21), (3, 3, 100, 33, 21), (3, 3, 100, 11, 0)):
        assert dll.tl_psf_workspace_bytes(*bad) == 0
    need = dll.tl_psf_workspace_bytes(3, 3, 1 << 20, 11, 21)
    assert _fwd(dll, R=1 << 20, ws=None) == EWORKSPACE
    assert _fwd(dll, R=1 << 20, ws_bytes=16) == EWORKSPACE and b"tl_psf_accumulate" in dll.tl_last_error()
    assert _bwd(dll, R=1 << 20, ws_bytes=16) == EWORKSPACE and b"tl_psf_accumulate_bwd" in dll.tl_last_error()
    assert need >= 256


def test_fused_has_no_cpu_fallback_and_no_fp64():
    x, y = (torch.from_numpy(a).float() for a in _fan())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.compute_psf(x, y, n_bins=(21, 21), increment=0.004, fused=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.compute_psf(x.double(), y.double(), fused=True)
    xt, yt = x.permute(0, 1, 3, 2), y.permute(0, 1, 3, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.psf_from_trace(xt, yt, torch.ones_like(xt, dtype=torch.bool), fused=True)
    for n_bins in ((33, 21), (21, 33), (64, 64)):
        with pytest.raises(ValueError, match="at most 32 bins"):
            metrics.compute_psf(x, y, n_bins=n_bins, fused=True)
    metrics.compute_psf(x, y, n_bins=(33, 40))              # the default path has no such limit


def test_the_default_path_is_the_unfused_one_bit_for_bit():
    x64, y64 = (torch.from_numpy(a) for a in _fan(seed=3))
    w64 = (torch.arange(x64.shape[-1]) % 7 != 0).to(torch.float64).expand_as(x64)
    for dt in (torch.float64, torch.float32):
        x, y, w = x64.to(dt), y64.to(dt), w64.to(dt)
        for kw in (dict(n_bins=(21, 21)), dict(n_bins=(8, 10), y_extent="centred"), dict(n_bins=(15, 15), increment=0.004),
                   dict(n_bins=(21, 21), increment=0.004, weights=w, y_target=y.reshape(2, -1).mean(dim=1))):
            a = metrics.compute_psf(x, y, **kw)
            b = metrics.compute_psf(x, y, fused=False, **kw)
            for p, q in zip(a, b):
                assert np.array_equal(np.asarray(p), np.asarray(q))
            assert a[3].dtype == dt
        xt, yt = x.permute(0, 1, 3, 2), y.permute(0, 1, 3, 2)
        ok = (w != 0).permute(0, 1, 3, 2)
        a, b = metrics.psf_from_trace(xt, yt, ok), metrics.psf_from_trace(xt, yt, ok, fused=False)
        assert all(np.array_equal(np.asarray(p), np.asarray(q)) for p, q in zip(a, b))
