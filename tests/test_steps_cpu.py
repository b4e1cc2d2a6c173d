"""What tests/test_gpu_steps_graph.py holds on the GPU, as far as it can be held without one.

* Every step of tests/step_cases.py that has a torch path runs with fused=False on the CPU: the same bits twice, and input
  sets A and B differ in every tensor it returns (the GPU tests' A / B / A replays would be vacuous otherwise).
* Warm-call host traffic, the CPU-side proxy of the GPU suite's sync-free check: `torch.tensor`, `torch.as_tensor` of a host
  sequence and `torch.from_numpy` are counted, and the SECOND call of every function that a captured step goes through builds
  no tensor from host data -- its constants are cached (lens_modeling.const_tensor, the tables kept on the geometry objects)
  and its argument checks are decided on host values.
* Those argument checks still raise the ValueErrors they raised when they read the device.
"""
import numpy as np
import pytest
import torch

import step_cases
from torchoptics_amd import imaging, lens_modeling as lm, paraxial


# ------------------------------------------------------------------------------------------------ the steps on the CPU
def _run(name, which):
    case = step_cases.build(name, "cpu", False)
    case.load(which)
    return case, [t.clone() for t in case.step()]


@pytest.mark.parametrize("name", step_cases.TORCH_PATH)
def test_a_step_gives_the_same_bits_twice_and_other_bits_on_other_inputs(name):
    case, first = _run(name, "A")
    again = [t.clone() for t in case.step()]                     # the same leaves, a second step: nothing carries over
    _, fresh = _run(name, "A")                                   # fresh leaves
    _, other = _run(name, "B")
    assert len(first) == len(case.names)
    for what, a, b, c, d in zip(case.names, first, again, fresh, other):
        assert a.shape == d.shape and a.dtype == d.dtype, what
        assert torch.equal(a, b), f"{name}: {what} changed on the second step"
        assert torch.equal(a, c), f"{name}: {what} differs between two builds"
        assert torch.isfinite(a).all() and torch.isfinite(d).all(), f"{name}: {what} is not finite"
        assert not torch.equal(a, d), f"{name}: {what} is the same on input sets A and B"


def test_loading_a_set_writes_the_leaves_in_place():
    case = step_cases.build("focus", "cpu", False)
    ptrs = {k: (t.data_ptr(), t.stride()) for k, t in case.leaves.items()}
    case.load("B")
    for k, t in case.leaves.items():
        assert (t.data_ptr(), t.stride()) == ptrs[k] and torch.equal(t.detach(), case.sets["B"][k])
        assert t.is_leaf and t.requires_grad and t.stride(2) == 1          # the tracer's layout: rays contiguous


# ---------------------------------------------------------------------------------------------- warm-call host traffic
class _HostTensors:
    """Counts the tensors built from host data while it is installed: torch.tensor, torch.from_numpy, and torch.as_tensor
    of anything that is not a tensor already."""

    def __init__(self, monkeypatch):
        self.calls = []
        for name in ("tensor", "from_numpy", "as_tensor"):
            monkeypatch.setattr(torch, name, self._counted(name, getattr(torch, name)))

    def _counted(self, name, fn):
        def wrapper(data, *args, **kwargs):
            if not (name == "as_tensor" and torch.is_tensor(data)):
                self.calls.append(name)
            return fn(data, *args, **kwargs)
        return wrapper


def _values(seed, shape):
    return torch.from_numpy(np.random.default_rng(seed).random(shape).astype(np.float32))


def _radial_map():
    v = _values(1, (2, 3))
    return lambda: imaging.radial_map(v, (0.4, 0.7, 1.0), (6, 9), v0=1.0)


def _distortion_grid():
    d = _values(2, (2, 3)) * 0.01
    return lambda: imaging.distortion_grid(d, [0.4, 0.7, 1.0], (6, 9))


def _grid_from_fields(index_map):
    k = _values(3, (3, 2, 5, 5))
    return lambda: imaging.psf_grid_from_fields(k, (3, 1) if index_map is None else (2, 2), index_map)


def _grid_from_trace():
    case = step_cases.build("psf_grid", "cpu", False)
    return case.step


def _ms_ssim_torch():
    a, b = _values(4, (1, 12, 14, 2)), _values(5, (1, 12, 14, 2))
    return lambda: imaging._ms_ssim_torch(a, b, 1.0, (0.4, 0.6), 5, 1.5, 0.01, 0.03)


def _aspheric_scale():
    st = lm.Structure(stop_idx=np.array([0]), sequence=np.array(["AGA"]), default_device="cpu")
    lens = lm.Lens(st, _values(6, (3,)), _values(7, (3,)), torch.tensor([1.5]), torch.tensor([50.0]),
                   poly=_values(8, (3, 4)) * 1e-4)
    return lambda: lens.scale(2.0).poly


def _last_curvature():
    import yaml_free_lenses as L
    lens, _, _ = L.build("cooke", "cpu", grad=False)
    c, t, nd = lens.flat_c_but_last, lens.flat_t, lens.flat_nd
    return lambda: paraxial.compute_last_curvature(lens.structure, c, t, nd)


WARM_CALLS = {
    "radial_map": _radial_map,
    "distortion_grid": _distortion_grid,
    "psf_grid_from_fields": lambda: _grid_from_fields(None),
    "psf_grid_from_fields-index_map": lambda: _grid_from_fields([[2, 1], [1, 0]]),
    "psf_grid_from_fields-index_map-array": lambda: _grid_from_fields(np.array([[2, 1], [1, 0]])),
    "psf_grid_from_trace-torch": _grid_from_trace,
    "ms_ssim_torch": _ms_ssim_torch,
    "aspheric-poly-scale": _aspheric_scale,
    "compute_last_curvature": _last_curvature,
}


@pytest.mark.parametrize("name", list(WARM_CALLS))
def test_the_second_call_builds_no_tensor_from_host_data(name, monkeypatch):
    call = WARM_CALLS[name]()
    first = call()
    counter = _HostTensors(monkeypatch)
    second = call()
    assert counter.calls == [], f"{name}: the warm call built tensors from host data: {counter.calls}"
    for a, b in zip(first if isinstance(first, tuple) else (first,), second if isinstance(second, tuple) else (second,)):
        assert torch.equal(a, b)


def test_the_counter_sees_a_cold_call(monkeypatch):
    """The detector detects: a first call with new constants does build tensors from host data."""
    v = _values(9, (1, 2))
    counter = _HostTensors(monkeypatch)
    imaging.radial_map(v, (0.123, 0.987), (3, 4))
    assert "tensor" in counter.calls
    torch.as_tensor(v)
    n = len(counter.calls)
    torch.as_tensor([1.0])
    assert len(counter.calls) == n + 1


# ------------------------------------------------------------------------------------------------ the argument checks
@pytest.mark.parametrize("fields", [(0.7, 0.4, 1.0), (0.4, 0.4, 1.0), (0.0, 0.5, 1.0), (-0.1, 0.5, 1.0), (1e-50, 0.5, 1.0)])
@pytest.mark.parametrize("kind", ["tuple", "array", "tensor"])
def test_radial_map_refuses_unsorted_or_non_positive_fields_on_the_host(fields, kind):
    given = {"tuple": fields, "array": np.asarray(fields), "tensor": torch.tensor(fields, dtype=torch.float64)}[kind]
    with pytest.raises(ValueError, match="fields must be ascending and > 0"):
        imaging.radial_map(_values(1, (2, 3)), given, (6, 9))
    with pytest.raises(ValueError, match="fields must be ascending and > 0"):
        imaging.distortion_grid(_values(1, (2, 3)), given, (6, 9))


def test_radial_map_checks_the_fields_in_the_dtype_of_the_values():
    """1e-50 is 0 in float32 (refused above) and positive in float64; two fields that differ by less than an fp32 ulp are one."""
    out = imaging.radial_map(_values(1, (2, 3)).double(), (1e-50, 0.5, 1.0), (6, 9))
    assert out.dtype == torch.float64 and torch.isfinite(out).all()
    with pytest.raises(ValueError, match="fields must be ascending and > 0"):
        imaging.radial_map(_values(1, (2, 2)), (0.5, 0.5 + 1e-9), (6, 9))


def test_radial_map_counts_the_fields_on_the_host():
    with pytest.raises(ValueError, match="hold 3 samples per lens, fields 2"):
        imaging.radial_map(_values(1, (2, 3)), (0.5, 1.0), (6, 9))
    with pytest.raises(ValueError, match="fields 0"):
        imaging.radial_map(_values(1, (2, 0)), (), (6, 9))


def test_radial_map_gives_the_bits_of_the_fields_rounded_once():
    """The cached device copy is the host values rounded once to the dtype of `values`: what torch.as_tensor gave."""
    v, fields = _values(11, (2, 3, 2)), (0.1, 0.7, 1.0)
    f = torch.as_tensor(fields, dtype=torch.float32)
    got = imaging.radial_map(v, fields, (5, 7), v0=1.0)
    assert torch.equal(got, imaging.radial_map(v, f, (5, 7), v0=1.0))
    assert torch.equal(got, imaging.radial_map(v, np.asarray(fields), (5, 7), v0=1.0))


@pytest.mark.parametrize("index_map, message", [([[0, 1], [2, 3]], "names a field that does not exist"),
                                                 ([[0, -1], [1, 2]], "names a field that does not exist"),
                                                 ([[0, 1, 2]], "must hold 2 x 2 entries")])
@pytest.mark.parametrize("kind", ["list", "array", "tensor"])
def test_psf_grid_from_fields_checks_the_index_map_on_the_host(index_map, message, kind):
    given = {"list": index_map, "array": np.asarray(index_map), "tensor": torch.tensor(index_map)}[kind]
    with pytest.raises(ValueError, match=message):
        imaging.psf_grid_from_fields(_values(3, (3, 2, 5, 5)), (2, 2), given)


def test_psf_grid_from_fields_gathers_by_the_map_and_views_the_identity():
    k = _values(3, (3, 2, 5, 5))
    got = imaging.psf_grid_from_fields(k, (2, 2), [[2, 1], [1, 0]])
    assert torch.equal(got, k[[2, 1, 1, 0]].permute(0, 2, 3, 1).unsqueeze(0))
    same = imaging.psf_grid_from_fields(k, (3, 1), np.arange(3).reshape(3, 1))
    assert same.data_ptr() == k.data_ptr()
