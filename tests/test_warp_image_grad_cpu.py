"""The fixed-point image gradient of imaging.warp_bicubic without a GPU: the contract of tl_warp_bwd_image (include/tl_trace.h)
emulated in numpy (tests/warp_image_ref.py) stays within the bound of tests/warp_image_cases.py on every shape, so the GPU
test can be passed; the bound is sharp (four wrong float64 evaluations and a fixed-point scale that ignores the data exceed
it); the `image_grad` keyword; the C entry points (declared, bound, exported, refusing bad arguments before any HIP call)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import warp_cases as wc
import warp_image_cases as wic
import warp_image_ref as wir
import warp_ref as ref
from torchoptics_amd import _lib, imaging

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
ONE = C.c_void_p(8)           # a non-NULL, aligned pointer that is never dereferenced: every call below is refused first


# --------------------------------------------------------------------------------------------- the contract and the bound

@pytest.mark.parametrize("name,signed", [(n, False) for n in wic.ALL] + [(n, True) for n in wc.SIGNED])
def test_the_emulated_contract_stays_within_the_bound_and_below_the_headroom(name, signed):
    image, x, y, gain, g_out = wic.inputs(name, signed)
    r = wic.reference(name, signed)
    got, acc = wir.emulate(image.shape, x, y, gain, g_out)
    assert int(np.abs(acc).max()) < 1 << 62, "the accumulators stay below 2^62"
    limit = wic.bound(r, gain, g_out)
    q = wc.ratio(got, r.g_image, limit)
    share = float((r.g_image_terms * wir.quantum(gain, g_out) / 2 / np.where(limit > 0, limit, 1)).max())
    print(f"WARP-IMG-ACC emulation {name}{'/signed' if signed else ''}: largest error / bound {q:.3f}  (largest share of Q in the bound {share:.3f})")
    assert q <= 1, (name, q)
    untouched = r.g_image_terms == 0
    assert (got[untouched] == 0).all() and not np.signbit(got[untouched]).any(), "no tap: exactly +0.0"


def test_the_new_shapes_are_what_they_are_for():
    r = wic.reference("sparse")
    assert (r.g_image_terms == 0).mean() >= 0.9
    r = wic.reference("pile-up")
    assert r.g_image_terms.max() >= 4096
    image, x, y, gain, g_out = wic.inputs("range")
    assert np.abs(g_out).min() < 2.0 ** -25 and np.abs(g_out).max() > 0.25
    r = wic.reference("range")
    limit = wic.bound(r, gain, g_out)
    share = r.g_image_terms * wir.quantum(gain, g_out) / 2 / limit
    assert share.max() > 5e-3, "somewhere Q is a visible share of the bound (it is below 1e-4 of it on every other shape)"
    _, x, y, _, _ = wic.inputs("outliers")
    _, xb, yb, _, _ = wic.inputs("barrel")
    assert 0 < ((x != xb) | (y != yb)).mean() < 0.03


@pytest.mark.parametrize("name", wc.MAIN)
@pytest.mark.parametrize("variant", ["alpha", "swap", "tap", "wrap"])
def test_a_wrong_float64_image_gradient_exceeds_the_bound(name, variant):
    image, x, y, gain, g_out = wic.inputs(name)
    r = wic.reference(name)
    wrong = ref.evaluate(image, x, y, gain, g_out, variant=variant).g_image
    assert (np.abs(wrong - r.g_image) > wic.bound(r, gain, g_out)).any(), (name, variant)


def test_a_fixed_scale_that_ignores_the_data_exceeds_the_bound():
    """The `range` shape with g_out times 2^-40: the scale taken from m stays within the bound, a scale fixed for |a| < 1 does
    not (its quantum is 2^40 times too coarse for these seeds)."""
    image, x, y, gain, g_out = wic.inputs("range")
    small = g_out * 2.0 ** -40
    r = ref.evaluate(image, x, y, gain, small)
    limit = wic.bound(r, gain, small)
    good, _ = wir.emulate(image.shape, x, y, gain, small)
    assert wc.ratio(good, r.g_image, limit) <= 1
    Hb = (16 * g_out.shape[1] * g_out.shape[2] - 1).bit_length()
    fixed, _ = wir.emulate(image.shape, x, y, gain, small, k=0 + Hb - 62)
    assert (np.abs(fixed - r.g_image) > limit).any()


def test_the_quantum_follows_the_contract():
    g = np.zeros((1, 4, 4, 1))
    assert wir.quantum(None, g) == 0.0
    g[0, 1, 2, 0] = -0.75                                     # 2^-1 <= m < 2^0: E = 0; 16 Ho Wo = 2^8
    assert wir.quantum(None, g) == 2.0 ** (0 + 8 - 62)
    g[0, 0, 0, 0] = 1.0                                       # 2^0 <= m < 2^1: E = 1
    assert wir.quantum(None, g) == 2.0 ** (1 + 8 - 62)
    g[0, 3, 3, 0] = np.inf                                    # left out of m
    assert wir.quantum(None, g) == 2.0 ** (1 + 8 - 62)
    assert wir.quantum(np.full((1, 4, 4, 1), 0.25), g) == 2.0 ** (-1 + 8 - 62)
    assert wir.quantum(None, np.ones((1, 3, 3, 2))) == 2.0 ** (1 + 8 - 62)     # 16 x 9 = 144 <= 2^8


# ------------------------------------------------------------------------------------------------------- Python layer

def test_the_image_grad_keyword():
    image = torch.rand((1, 5, 6, 3), requires_grad=True)
    x = torch.zeros((1, 4, 7))
    for bad in ("kernel", None, True, "Fused"):
        with pytest.raises(ValueError, match="image_grad must be 'torch' or 'fused'"):
            imaging.warp_bicubic(image, x, x, image_grad=bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        imaging.warp_bicubic(image, x, x, fused=True, image_grad="fused")              # CPU tensors: no longer "scatter"
    with pytest.raises(RuntimeError, match="image requires a gradient.*scatter"):
        imaging.warp_bicubic(image, x, x, fused=True, image_grad="torch")              # the default, as before
    for fused in (None, False):                                                        # on the CPU both are the torch path
        out = imaging.warp_bicubic(image, x, x, fused=fused, image_grad="fused")
        assert torch.equal(out, imaging.warp_bicubic(image, x, x))
    image.grad = None
    imaging.warp_bicubic(image, x, x, image_grad="fused").sum().backward()
    assert float(image.grad.sum()) == pytest.approx(4 * 7 * 3)


def test_an_output_beyond_the_headroom_is_refused_and_points_to_the_torch_path():
    image = torch.rand((1, 2, 2, 1), requires_grad=True)
    x = torch.zeros((1, 1, 1)).expand(1, 8193, 8193)                                   # 8193^2 > 2^26; no memory behind it
    with pytest.raises(RuntimeError, match=r"8193 x 8193 pixels.*2\^26.*fused=False"):
        imaging.warp_bicubic(image, x, x, fused=True, image_grad="fused")
    with pytest.raises(RuntimeError, match="no CPU fallback"):                         # without an image gradient: no such limit
        imaging.warp_bicubic(image.detach(), x, x, fused=True, image_grad="fused")


def test_set_warp_image_grad_path_takes_two_values():
    from torchoptics_amd import ops
    ops.set_warp_image_grad_path("direct")
    ops.set_warp_image_grad_path("auto")
    with pytest.raises(ValueError, match="auto"):
        ops.set_warp_image_grad_path("lds")
    assert "bwd_image" in ops.warp_counts()


# ------------------------------------------------------------------------------------------------------------------ C ABI

def _geom(B=2, H=5, W=6, Cc=3, Ho=4, Wo=7, cb=2, gb=2, gc=3):
    q = _lib.tl_warp_geom(device=0, B=B, H=H, W=W, C=Cc, Ho=Ho, Wo=Wo, coord_batch=cb, gain_batch=gb, gain_channels=gc)
    q.image_stride[:] = (H * W * Cc, W * Cc, Cc, 1)
    q.x_stride[:] = q.y_stride[:] = q.g_x_stride[:] = q.g_y_stride[:] = (Ho * Wo, Wo, 1)
    q.gain_stride[:] = q.g_gain_stride[:] = (Ho * Wo * gc, Wo * gc, gc, 1)
    return q


def test_entry_points_are_declared_bound_and_exported_and_the_abi_version_stays():
    hdr = open(os.path.join(ROOT, "include", "tl_trace.h")).read()
    declared = set(re.findall(r"\b(tl_[a-z0-9_]+)\s*\(", hdr))
    dll = _lib.lib()
    for name in ("tl_warp_bwd_image", "tl_warp_bwd_image_work_bytes"):
        assert name in declared and name in _lib.EXPORTS and hasattr(dll, name), name
        assert _lib._SIGNATURES[name][1][0] is C.POINTER(_lib.tl_warp_geom)
    assert _lib._SIGNATURES["tl_warp_bwd_image_work_bytes"][0] is C.c_size_t
    assert declared == set(_lib.EXPORTS)
    assert dll.tl_version() == _lib.TL_ABI_VERSION == 15


def test_the_workspace_grows_with_the_image_and_not_with_the_output():
    dll = _lib.lib()
    size = lambda **kw: dll.tl_warp_bwd_image_work_bytes(C.byref(_geom(**kw)))        # noqa: E731
    base = size()
    assert base >= 8 * 2 * 5 * 6 * 3
    for grow in (dict(B=4, cb=4, gb=4), dict(H=10), dict(W=12), dict(Cc=6, gc=6)):
        assert size(**grow) >= base + 8 * 2 * 5 * 6 * 3, grow                         # twice the elements: 8 more bytes each
    assert size(Ho=40, Wo=70) == base
    assert size(B=1 << 10, cb=1, gb=1, H=1 << 10, W=1 << 10) >= 8 << 30
    assert size(B=0) == 0 and dll.tl_warp_bwd_image_work_bytes(None) == 0


def test_bad_arguments_are_refused_before_any_device_call():
    dll = _lib.lib()
    big = C.c_size_t(1 << 40)

    def call(q, x=ONE, y=ONE, gain=ONE, g_out=ONE, g_image=ONE, work=ONE, work_bytes=big, flags=0):
        return dll.tl_warp_bwd_image(C.byref(q), x, y, gain, g_out, g_image, work, work_bytes, flags, None)

    def refused(rc, *words):
        msg = dll.tl_last_error()
        assert rc == EINVAL and all(w in msg for w in (b"tl_warp_bwd_image",) + words), (rc, msg, words)

    for size in ("B", "H", "W", "Cc", "Ho", "Wo"):
        refused(call(_geom(**{size: 0})), b">= 1")
    refused(call(_geom(cb=3)), b"coord_batch")
    refused(call(_geom(cb=1, gb=3)), b"gain_batch")
    refused(call(_geom(gc=2)), b"gain_channels")
    refused(call(_geom(H=(1 << 20) + 1)), b"2^20")
    for arg in ("x", "y", "g_out", "g_image", "work"):
        refused(call(_geom(), **{arg: None}), arg.encode())
    refused(call(_geom(Ho=8193, Wo=8193)), b"Ho Wo", b"2^26")
    assert call(_geom(Ho=8192, Wo=8192), work_bytes=0) == EINVAL and b"work_bytes" in dll.tl_last_error()   # 2^26 itself passes
    refused(call(_geom(B=1 << 21, cb=1, gb=1, H=1 << 20, W=1 << 20)), b"B H W C", b"2^40")
    need = dll.tl_warp_bwd_image_work_bytes(C.byref(_geom()))
    refused(call(_geom(), work_bytes=need - 1), b"work_bytes", str(need).encode())
    refused(call(_geom(), work=C.c_void_p(12)), b"work", b"aligned")
    refused(call(_geom(), flags=2), b"flags")
    refused(call(_geom(gb=7, gc=9), gain=None, g_image=None), b"g_image")             # without a gain its extents are not read
    rc = dll.tl_warp_bwd_image(None, ONE, ONE, ONE, ONE, ONE, ONE, big, 0, None)
    refused(rc, b"g is NULL")
