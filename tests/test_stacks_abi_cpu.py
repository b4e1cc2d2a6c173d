"""
The C-ABI side of the differentiable penalty stacks, without a GPU: the gradient of the per-surface stacks is a member of
the tl_seeds block both backward entry points take (ABI 15; ABI 14 had two twin entry points for it), and a stack gradient
without the penalty term is refused before any device call.
"""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GONE = ("tl_trace_bwd" + "_stacks", "tl_trace_bwd_from_outputs" + "_stacks")     # the twins of ABI 14
EINVAL = -1                                           # TL_EINVAL (include/tl_trace.h)


def _problem(_lib, aggregate):
    """A problem that passes the argument checks; its pointers are never dereferenced on the paths tested here."""
    one = 8
    p = _lib.tl_problem()
    p.F, p.P, p.W, p.S, p.B = 3, 1024, 3, 7, 1
    p.device, p.mode, p.allow_backward, p.aggregate = 0, 0, 1, aggregate
    p.x_in = p.y_in = p.z = p.cx = p.cy = p.c = p.t = p.mu = p.mask = one
    return p


def test_stack_entry_points_are_declared_and_exported():
    """g_stacks is a member of tl_seeds in the header and in _lib; the ABI-14 twins are neither declared nor exported."""
    from torchoptics_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "tl_trace.h")).read()
    declared = set(re.findall(r"\b(tl_[a-z0-9_]+)\s*\(", hdr))
    dll = _lib.lib()
    body = re.search(r"typedef struct tl_seeds \{(.*?)\} tl_seeds;", hdr, re.S)
    assert body and re.search(r"\bconst float \*g_stacks;", body.group(1))
    assert "g_stacks" in [n for n, _ in _lib.tl_seeds._fields_]
    for name in GONE:
        assert name not in declared and name not in _lib.EXPORTS, name
        assert not hasattr(dll, name), name
    # both backward calls take the block
    for name in ("tl_trace_bwd", "tl_trace_bwd_from_outputs"):
        assert name in declared and name in _lib.EXPORTS and hasattr(dll, name), name
        assert _lib._SIGNATURES[name][1][1] is C.POINTER(_lib.tl_seeds), name


def test_abi_version_and_problem_layout():
    from torchoptics_amd import _lib
    dll = _lib.lib()
    assert dll.tl_version() == _lib.TL_ABI_VERSION == 15
    assert dll.tl_problem_size() == C.sizeof(_lib.tl_problem) == 248


def test_stack_gradient_without_aggregate_is_refused_before_any_device_call():
    from torchoptics_amd import _lib
    dll = _lib.lib()
    p = _problem(_lib, aggregate=0)
    ws = C.c_void_p(16)
    g = _lib.tl_seeds(g_moments=8, g_stacks=8)
    out = _lib.tl_grads(g_c=8, g_t=8, g_mu=8, g_z=8, g_cx=8, g_cy=8)
    rc = dll.tl_trace_bwd(C.byref(p), g, out, ws, 1 << 30, None)
    assert rc == EINVAL
    assert b"g_stacks" in dll.tl_last_error()
    fwd = _lib.tl_rays(x=8, y=8, cx=8, cy=8, ok=8)
    rc = dll.tl_trace_bwd_from_outputs(C.byref(p), g, fwd, out, ws, 1 << 30, None)
    assert rc == EINVAL
    assert b"g_stacks" in dll.tl_last_error()
