"""metrics.compute_distortion, compute_relative_illumination and compute_ray_aiming_error on the device against their fp64
restatement (tests/metrics_ref.py), case by case of tests/metrics_cases.py and in both arithmetic modes: every value within
an absolute gate, the gradient of sum(w metric) to every leaf (c, t, nd, v, kappa, poly) within a rel-L2 gate, the shapes, the
rows of a padded batch against the single-lens calls, and for the case with dead rays the fields that report exactly 1 and
their exactly zero gradient.  The gates come from the restatement's own fp32 noise (metrics_cases.py); nothing here is
measured on the code under test.  Run with -s for the METRICS-ACC lines (profiles/metrics_accuracy.txt)."""
import numpy as np
import pytest
import torch

import metrics_cases as MC
import metrics_ref as MR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPE = {"dist": lambda B, F, W: (B, F), "ri": lambda B, F, W: (B, F, W), "aim": lambda B, F, W: (B, F, 2, 1)}


@pytest.fixture(scope="module", autouse=True)
def _library():
    from torchoptics_amd import _lib
    _lib.lib()


def _metric(spec, mode, weights=None):
    """The product's metric of a case in `mode`: (value, {leaf: flat gradient of sum(weights value), fp64 numpy} or None)."""
    import torchoptics_amd as ta
    from torchoptics_amd import ops
    lens, specs, leaves = MC.build(spec, DEV, grad=weights is not None)
    vig_fn = MR.linear_vig if spec["vig"] else None
    fields = list(spec["fields"])
    before = ops.get_default_mode()
    ops.set_default_mode(mode)
    try:
        if spec["metric"] == "dist":
            value = ta.metrics.compute_distortion(specs, lens, fields, DEV)
        elif spec["metric"] == "ri":
            value = ta.metrics.compute_relative_illumination(specs, lens, fields, vig_fn, spec["n_iter"], spec["wavelengths"], DEV)
        else:
            value = ta.metrics.compute_ray_aiming_error(specs, lens, fields, vig_fn, spec["n_iter"], spec["aim_mode"], DEV)
        grads = None
        if weights is not None:
            (torch.as_tensor(weights).to(DEV, torch.float32) * value).sum().backward()
            grads = {n: (torch.zeros_like(v) if v.grad is None else v.grad).detach().cpu().double().numpy()
                     for n, v in leaves.items()}
    finally:
        ops.set_default_mode(before)
    return value, grads


@pytest.mark.parametrize("mode", MC.MODES)
@pytest.mark.parametrize("name", MC.NAMES)
def test_metric_against_the_fp64_restatement(name, mode):
    spec, ref = MC.CASES[name], MC.reference(name)
    if not isinstance(ref["value"], np.ndarray):                       # a stop at row 0: the integer 0, nothing traced
        got, _ = _metric(spec, mode)
        assert isinstance(got, int) and got == ref["value"] == 0
        print(f"METRICS-ACC {name} {mode}: the integer 0")
        return
    w = MR.weights(ref["value"].shape, MC.seed_of(name)).numpy() if spec["grad"] else None
    got, grads = _metric(spec, mode, w)
    B, F, W = len(MC.build(spec, "cpu")[0]), len(spec["fields"]), len(spec["wavelengths"])
    assert tuple(got.shape) == SHAPE[spec["metric"]](B, F, W) == ref["value"].shape and got.dtype == torch.float32
    got = got.detach().cpu().numpy()
    if grads is not None:
        assert set(grads) == set(ref["grads"])
        for leaf, g in grads.items():
            assert g.shape == ref["grads"][leaf].shape, leaf
    err = MC.errors(got, grads, ref)
    ratio = {k: e / MC.gate(name, mode, k) for k, e in err.items()}
    print(f"METRICS-ACC {name} {mode}: " + ", ".join(
        f"{'values' if k is None else 'd/d' + k} {err[k]:.3e} / {MC.gate(name, mode, k):.3e} = {ratio[k]:.3f}" for k in err))
    if name in MC.DEAD:
        # the fields with a dead ray (or a dead ray on axis at their wavelength) report exactly 1, the others do not
        valid = ref["valid"]
        assert (got[~valid] == 1.0).all()
        assert (got[:, 1:][valid[:, 1:]] != 1.0).all()
    for b, (_, single) in enumerate(MC.singles(spec)):
        one, _ = _metric(single, mode)
        e = MC.abs_err(got[b], one.detach().cpu().numpy()[0])
        print(f"METRICS-ACC {name} {mode}: row {b} against the single-lens call {e:.3e} / {MC.gate(name, mode):.3e}")
        assert e <= MC.gate(name, mode), (name, b, e)
    assert max(ratio.values()) <= 1, (name, mode, ratio)


@pytest.mark.parametrize("mode", MC.MODES)
def test_fields_that_report_one_have_no_gradient(mode):
    name = MC.DEAD[0]
    ref = MC.reference(name)
    got, grads = _metric(MC.CASES[name], mode, (~ref["valid"]).astype(np.float64))
    assert (got.detach().cpu().numpy()[~ref["valid"]] == 1.0).all()
    for leaf, g in grads.items():
        assert (g == 0).all(), leaf
