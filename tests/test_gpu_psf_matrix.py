"""The fused PSF kernels (csrc/tl_psf.hip behind ops.PsfAccumulateFunction) on the GPU, across launch plans, instantiations,
weight kinds, strides and partial gradients: every element of hist, gx and gy against the float64 reference of
tests/psf_ref.py within the bounds that tests/psf_cases.py derives from the kernels' roundings (and that
tests/test_psf_cases_cpu.py holds to be sufficient and sharp); the three per-grid gradients against the float64 sums of the
kernel's own gx, gy.  The lines "PSF-BND ..." are kept in profiles/psf_fused_accuracy.txt; "PSF-GRID ..." is for the record."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import psf_cases as pc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALL = pc.RESULTS + pc.GRID
_RUNS = {}


@pytest.fixture(scope="module")
def ops():
    from torchoptics_amd import _lib, ops
    _lib.lib()
    return ops


def _clean(ops, name):
    """The op on a case as it stands in the table: run once, shared, never changed."""
    if name not in _RUNS:
        a = pc.inputs(name)
        _RUNS[name] = pc.run(ops, pc.tensors(a, DEV), a)
    return _RUNS[name]


def _assert_same_bits(got, want, names=ALL, what=""):
    for k in names:
        assert pc.same_bits(got[k], want[k]), f"{what}: {k} differs"


def _held(label, got, r, a):
    """Print the line of a run and hold every result to its bound."""
    q, s, rel = pc.ratios(got, r, a), pc.grid_ratios(got, a), pc.grid_rel(got, r)
    G, W, R = a.shape
    pl = pc.plan(G, W, R, a.nxh, a.ny)
    print(f"PSF-BND {label} {G}x{W}x{R} {a.ny}x{a.nxh} <{pl.nxp}> nb={pl.nb} rpl={pl.rpl}: largest error / bound "
          f"hist {q['hist']:.3f} gx {q['gx']:.3f} gy {q['gy']:.3f}; per-grid / sum tolerance "
          + " ".join(f"{k} {v:.3f}" for k, v in s.items()))
    print(f"PSF-GRID {label}: relative to the float64 reference " + " ".join(f"{k} {v:.2e}" for k, v in rel.items()))
    for k in ALL:
        assert got[k].dtype == np.float32 and np.isfinite(got[k]).all(), k
    assert max(q.values()) <= 1.0, (label, q)
    assert max(s.values()) <= 1.0, (label, s)


# --------------------------------------------------------------------------------------------------------- 1. every case
@pytest.mark.parametrize("name", list(pc.CASES))
def test_every_case_within_its_bounds_and_the_same_bits_twice(ops, name):
    a, r = pc.inputs(name), pc.reference(name)
    got = _clean(ops, name)
    again = pc.run(ops, pc.tensors(a, DEV), a)
    _assert_same_bits(again, got, what=name)
    assert got["hist"].shape == a.shape[:2] + (a.ny, a.nxh) and got["gx"].shape == got["gy"].shape == a.shape
    _held(name, got, r, a)
    if name == "dead-channel":
        c = pc.DEAD_CHANNEL
        assert not got["hist"][c].any() and not got["gx"][c].any() and not got["gy"][c].any()
        assert got["hist"][0, 0].all() and got["gx"][0, 0].any()


# ---------------------------------------------------------------------------------------------- 2. all eight instantiations
@pytest.mark.parametrize("nxh", pc.SWEEP_NXH)
def test_every_instantiation_of_the_backward(ops, nxh):
    a, r = pc.sweep_inputs(nxh), pc.reference(("sweep", nxh))
    got = pc.run(ops, pc.tensors(a, DEV), a)
    assert got["g_hist"].shape == a.T.shape and np.array_equal(got["g_hist"], a.T), "the backward was handed another g_hist"
    _held(f"nxh={nxh}", got, r, a)


# ------------------------------------------------------------------------------------------------------- 3. weight kinds
def test_bytes_bools_and_floats_of_0_and_1_give_the_same_bits(ops):
    a = pc.inputs("block-edge")
    live = a.weight != 0
    runs = []
    for w in (live.astype(np.float32), live, live.astype(np.uint8)):
        t = pc.tensors(a, DEV)
        t["weight"] = torch.from_numpy(w).to(DEV)
        runs.append(pc.run(ops, t, a))
    _assert_same_bits(runs[1], runs[0], what="bool")
    _assert_same_bits(runs[2], runs[0], what="uint8")
    r = pc.evaluate(a, weight=live)
    _held("block-edge 0/1 weights", runs[0], r, a)


def test_half_the_weights_give_half_the_result_and_negated_weights_the_negative(ops):
    a = pc.inputs("block-edge")
    full = _clean(ops, "block-edge")
    for factor in (0.5, -1.0):
        t = pc.tensors(a, DEV)
        t["weight"] = t["weight"] * factor
        got = pc.run(ops, t, a)
        for k in ALL:
            assert np.array_equal(got[k], np.float32(factor) * full[k]), (factor, k)
    neg = pc.tensors(a, DEV)
    neg["weight"] = -neg["weight"].abs()                      # every weight negative: the bound stands on absolute values
    w = -np.abs(a.weight)
    _held("block-edge negative weights", pc.run(ops, neg, a), pc.evaluate(a, weight=w), a)


# ------------------------------------------------------------------------------------- 4. dead rays with hostile coordinates
@pytest.mark.parametrize("name", ["block-edge", "plan-3"])
def test_a_ray_of_weight_0_contributes_nothing_whatever_its_coordinates(ops, name):
    a = pc.inputs(name)
    clean = _clean(ops, name)
    dead = torch.from_numpy(a.weight == 0).to(DEV)
    assert dead.any()
    for bad in (float("nan"), float("inf"), 1e30):
        t = pc.tensors(a, DEV)
        t["x"][dead] = bad
        t["y"][dead] = bad
        got = pc.run(ops, t, a)
        _assert_same_bits(got, clean, what=f"{name} {bad}")
        assert not got["gx"][a.weight == 0].any() and not got["gy"][a.weight == 0].any()
        assert all(np.isfinite(got[k]).all() for k in ALL)


def test_live_rays_far_off_the_grid_add_exactly_nothing(ops):
    """Live rays 50 pixels past the last column, 5000 pixels past the last row, and 5000 and 50: a Gaussian underflows to 0,
    so the result is the one with those rays at weight 0, and their gradients are 0."""
    a = pc.inputs("block-edge")
    G, W, R = a.shape
    far = (np.arange(G * W * R).reshape(a.shape) % 5 == 1) & (a.weight != 0)
    far[..., R - 1] = a.weight[..., R - 1] != 0                # the lone ray of the second block too
    kind = np.arange(G * W * R).reshape(a.shape) % 3
    px, py = a.x_pitch[:, None, None].astype(np.float64), a.y_pitch[:, None, None].astype(np.float64)
    off_x, off_y = np.array([50.0, 0.0, 5000.0])[kind], np.array([0.0, 5000.0, 50.0])[kind]
    x = np.where(far & (off_x > 0), (a.x_first + a.nxh - 1 + off_x) * px, a.x).astype(np.float32)
    y = np.where(far & (off_y > 0), a.y_centre[:, None, None] + (a.y_first + a.ny - 1 + off_y) * py, a.y).astype(np.float32)
    t = pc.tensors(a, DEV)
    t["x"], t["y"] = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    got = pc.run(ops, t, a)
    t0 = pc.tensors(a, DEV)
    t0["weight"] = torch.from_numpy(np.where(far, np.float32(0), a.weight)).to(DEV)
    want = pc.run(ops, t0, a)
    for k in ALL:
        assert np.isfinite(got[k]).all() and np.array_equal(got[k], want[k]), k
    assert far.sum() > 100 and not got["gx"][far].any() and not got["gy"][far].any()
    assert got["gx"][~far & (a.weight != 0)].all()


# ------------------------------------------------------------------------------------------------------------ 5. strides
def test_a_strided_x_is_read_in_place_and_gives_the_bits_of_the_contiguous_run(ops):
    a = pc.inputs("block-edge")
    G, W, R = a.shape
    clean = _clean(ops, "block-edge")
    t = pc.tensors(a, DEV)
    r0 = 3 if ((W + 2) * (R + 5) + (R + 5)) % 2 == 0 else 2
    big = torch.zeros((G + 1, W + 2, R + 5), device=DEV).requires_grad_(True)
    with torch.no_grad():
        big[1:, 1:W + 1, r0:r0 + R] = t["x"]
    xv = big[1:, 1:W + 1, r0:r0 + R]
    assert xv.storage_offset() % 2 == 1 and xv.stride() == ((W + 2) * (R + 5), R + 5, 1) and xv.stride(0) != W * xv.stride(1)
    wbig = torch.zeros((G, W + 1, R + 2), device=DEV)
    wbig[:, :W, 1:R + 1] = t["weight"]
    t["x"], t["weight"] = xv, wbig[:, :W, 1:R + 1]
    assert t["y"].is_contiguous() and not t["weight"].is_contiguous()
    got = pc.run(ops, t, a)
    assert got["saved_x_ptr"] == xv.data_ptr(), "a strided x with contiguous rays must reach the kernel without a copy"
    _assert_same_bits(got, clean, what="strided")
    g = big.grad.cpu().numpy()
    assert np.array_equal(g[1:, 1:W + 1, r0:r0 + R], clean["gx"])
    g[1:, 1:W + 1, r0:r0 + R] = 0
    assert not g.any()


def test_an_expanded_x_is_copied_and_still_right(ops):
    a = pc.inputs("block-edge")
    G, W, R = a.shape
    t = pc.tensors(a, DEV)
    leaf = t["x"][:, :1, :].clone().requires_grad_(True)
    t["x"] = leaf.expand(G, W, R)
    assert t["x"].stride(1) == 0
    got = pc.run(ops, t, a)
    assert got["saved_x_ptr"] != leaf.data_ptr()
    b = SimpleNamespace(**vars(a))
    b.x = np.ascontiguousarray(np.broadcast_to(a.x[:, :1, :], a.shape))
    want = pc.run(ops, pc.tensors(b, DEV), b)
    _assert_same_bits(got, want, what="expanded")
    _held("block-edge expanded x", got, pc.evaluate(b), b)
    both = got["gx"].astype(np.float64)
    assert np.abs(leaf.grad.cpu().numpy()[:, 0] - both.sum(1)).max() <= 2 * pc.U * np.abs(both).sum(1).max()


# -------------------------------------------------------------------------------------------------- 6. partial gradients
@pytest.mark.parametrize("needs", [("y_centre",), ("x_pitch", "x"), ("x",)], ids=lambda n: "+".join(n))
def test_a_gradient_that_is_asked_for_alone_has_the_bits_of_the_full_run(ops, needs):
    a = pc.inputs("block-edge")
    full = _clean(ops, "block-edge")
    got = pc.run(ops, pc.tensors(a, DEV), a, needs=needs)
    assert pc.same_bits(got["hist"], full["hist"])
    for n, k in zip(pc.LEAVES, ("gx", "gy") + pc.GRID):
        if n in needs:
            assert pc.same_bits(got[k], full[k]), k
        else:
            assert got[k] is None, k
