"""
Iterated ray aiming without a GPU: the fp64 restatement (aim_iter_ref.py) reproduces the reference's one-step aimed fan
(fixture G6) and converges on the caller's lenses, and tl_ray_aim_iter is declared, exported and refuses bad arguments
before any device call.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1                                           # TL_EINVAL (include/tl_trace.h)


def _cpu(name, **kw):
    import yaml_free_lenses as L
    lens, specs, _ = L.build(name, "cpu", grad=False, **kw)
    return lens, specs


def test_restatement_at_one_step_reproduces_the_reference_fixture():
    """G6: the reference's own aimed pupil coordinates of the Cooke triplet (16 x 16, fields 0 / 0.707 / 1, C d F)."""
    import aim_iter_ref as R
    from torchoptics_amd import ray_tracing as rt
    g = load_golden("G6_cooke_aim1")
    lens, specs = _cpu("cooke")
    inp = R.inputs(lens, specs, (0., 0.707, 1.), (656.3, 587.6, 486.1))
    xp, yp = rt.circle(None, 16, 16, "cpu")
    x, y = R.aimed_fan(R.aim(inp, 1), xp, yp, specs.epd)
    assert x.shape == g["in_x"].shape
    assert np.abs(x.numpy() - g["in_x"]).max() <= 2e-5
    assert np.abs(y.numpy() - g["in_y"]).max() <= 2e-5


@pytest.mark.parametrize("name", ["cooke", "doublet"])
def test_meridional_error_converges_by_four_steps(name):
    import aim_iter_ref as R
    lens, specs = _cpu(name)
    inp = R.inputs(lens, specs, (0.5, 0.707, 1.), (587.6,))
    err = [R.residual(inp, n)[:, :, :2].abs().max().item() for n in (1, 2, 3, 4)]
    assert err[3] < 1e-9, err
    assert err[1] < err[0] and err[2] < err[1], err            # each step helps while it is above the noise
    if name == "cooke":
        assert err[0] >= 5e-3                                  # one step leaves the pupil mis-aimed


def test_sagittal_step_takes_its_own_partial_after_the_first():
    """Tessar at epd 12, hfov 30, field 0.707: with d xs/d xp from step 2 on, the sagittal error keeps falling
    (the reference's d(xs + ys)/dp diverges there)."""
    import aim_iter_ref as R
    lens, specs = _cpu("tessar", epd=12.0, hfov_deg=30.0)
    inp = R.inputs(lens, specs, (0.707,), (587.6,))
    err = [R.residual(inp, n)[:, :, 2].abs().max().item() for n in (1, 2, 3, 4)]
    assert err[3] < 1e-10 and err[3] < err[2] < err[1], err


def test_iterated_aiming_entry_point_is_declared_and_exported():
    from torchoptics_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "tl_trace.h")).read()
    declared = set(re.findall(r"\b(tl_[a-z0-9_]+)\s*\(", hdr))
    assert "tl_ray_aim_iter" in declared and "tl_ray_aim_iter" in _lib.EXPORTS
    assert hasattr(_lib.lib(), "tl_ray_aim_iter")
    assert int(re.search(r"#define TL_MAX_AIM_ITER (\d+)", hdr).group(1)) == _lib.TL_MAX_AIM_ITER == 16
    # tl_ray_aim's arguments, with n_iter, tee_ref and rs before the outputs
    args, base = _lib._SIGNATURES["tl_ray_aim_iter"][1], _lib._SIGNATURES["tl_ray_aim"][1]
    assert args[:18] == base[:18] and args[21:] == base[18:]
    assert args[18] == C.c_int32 and args[19:21] == [C.c_void_p, C.c_void_p]


def _call(dll, n_iter=2, null=None):
    one = C.c_void_p(8)                                   # any non-NULL pointer: never dereferenced on these paths
    ptrs = {k: one for k in ("c", "t", "n", "n_d", "mask", "z", "hfov", "fields", "epd", "xs", "ys", "yo")}
    if null:
        ptrs[null] = None
    p = ptrs
    return dll.tl_ray_aim_iter(0, 2, 3, 3, 4, p["c"], p["t"], p["n"], p["n_d"], p["mask"], None, None, None, p["z"], p["hfov"],
                               p["fields"], p["epd"], 1, n_iter, None, None, p["xs"], p["ys"], p["yo"], None)


@pytest.mark.parametrize("n_iter", [0, -1, 17, 1 << 20])
def test_iteration_count_out_of_range_is_refused(n_iter):
    from torchoptics_amd import _lib
    dll = _lib.lib()
    assert _call(dll, n_iter=n_iter) == EINVAL
    assert b"n_iter" in dll.tl_last_error()


@pytest.mark.parametrize("null", ["c", "t", "n", "n_d", "mask", "z", "hfov", "fields", "epd", "xs", "ys", "yo"])
def test_null_required_pointer_is_refused(null):
    from torchoptics_amd import _lib
    dll = _lib.lib()
    assert _call(dll, null=null) == EINVAL
    assert b"tl_ray_aim_iter" in dll.tl_last_error()


def test_python_refuses_more_steps_than_the_kernel_takes():
    import torchoptics_amd as ta
    lens, specs = _cpu("cooke")
    tr = ta.RayTracer(mode="circular", n_rays=(4, 4), n_ray_aiming_iter=17, default_device="cpu")
    with pytest.raises(ValueError, match="n_ray_aiming_iter"):
        tr.ray_aiming(specs, lens, True)
