"""
The C-ABI side of the differentiable penalty stacks (ABI 14), without a GPU: the two backward entry points that take a
gradient of the per-surface stacks are declared and exported, and a stack gradient without the penalty term is refused
before any device call.
"""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tl_trace_bwd_stacks", "tl_trace_bwd_from_outputs_stacks")
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
    from torchoptics_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "tl_trace.h")).read()
    declared = set(re.findall(r"\b(tl_[a-z0-9_]+)\s*\(", hdr))
    dll = _lib.lib()
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS, name
        assert hasattr(dll, name), name
    # after g_stacks, exactly the argument lists of the existing two calls
    for name, base in zip(NEW, ("tl_trace_bwd", "tl_trace_bwd_from_outputs")):
        args, base_args = _lib._SIGNATURES[name][1], _lib._SIGNATURES[base][1]
        assert [args[0]] + args[2:] == base_args, name


def test_abi_version_and_problem_layout():
    from torchoptics_amd import _lib
    dll = _lib.lib()
    assert dll.tl_version() == _lib.TL_ABI_VERSION == 14
    assert dll.tl_problem_size() == C.sizeof(_lib.tl_problem) == 248


def test_stack_gradient_without_aggregate_is_refused_before_any_device_call():
    from torchoptics_amd import _lib
    dll = _lib.lib()
    one = C.c_void_p(8)
    p = _problem(_lib, aggregate=0)
    ws = C.c_void_p(16)
    # g_stacks, gx, gy, gcx, gcy, g_moments, g_opd, g_c, g_t, g_mu, g_z, g_cx, g_cy, g_kappa, g_poly, g_n, g_xin, g_yin
    rc = dll.tl_trace_bwd_stacks(C.byref(p), one, None, None, None, None, one, None, one, one, one, one, one, one,
                                 None, None, None, None, None, ws, 1 << 30, None)
    assert rc == EINVAL
    assert b"g_stacks" in dll.tl_last_error()
    # g_stacks, gx, gy, gcx, gcy, g_moments, x, y, cx, cy, ok, moments_fwd, g_c, g_t, g_mu, g_z, g_cx, g_cy, g_kappa,
    # g_poly, g_xin, g_yin
    rc = dll.tl_trace_bwd_from_outputs_stacks(C.byref(p), one, None, None, None, None, one, one, one, one, one, one, None,
                                              one, one, one, one, one, one, None, None, None, None, ws, 1 << 30, None)
    assert rc == EINVAL
    assert b"g_stacks" in dll.tl_last_error()
