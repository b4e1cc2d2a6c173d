"""The premises of tests/test_gpu_spot_kernels.py, checked without a GPU: the inputs of tests/spot_cases.py make every moment
exact in fp64, its restatement of the launch plan of tl_spot_moments reaches every path the GPU tests claim to reach (with the
plan's constants read from csrc/tl_api.hip, so that a change there fails here), and the coincident-ray moments really drive the
closed form below zero in plain fp64."""
import os
import re

import numpy as np
import pytest
import torch

import spot_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plan_constants():
    """(cap, rmax, few, rwant, kBlock, unroll) as csrc/tl_api.hip states them."""
    with open(os.path.join(ROOT, "torchoptics_amd", "csrc", "tl_api.hip")) as f:
        src = f.read()
    block = int(re.search(r"constexpr int kBlock = (\d+);", src).group(1))
    few, rwant = (int(v) for v in re.search(r"Plan make_plan\(int P, int FW, int cap, int rmax, int few = (\d+), int rwant = (\d+)\)",
                                            src).groups())
    spot = src[src.index("int tl_spot_moments("):]
    cap, rmax = (int(v) for v in re.search(r"const Plan pl = make_plan\(P, F \* W, (\d+), (\d+)\);", spot).groups())
    last, step = (int(v) for v in re.search(r"for \(; i \+ (\d+) \* kBlock < count; i \+= (\d+) \* kBlock\)", src).groups())
    assert step == last + 1
    return cap, rmax, few, rwant, block, step


def test_plan_constants_are_the_ones_the_case_list_was_derived_for():
    assert _plan_constants() == (4096, 64, 2048, 8, 256, 8)


def _plans():
    cap, rmax, few, rwant, block, unroll = _plan_constants()
    out = {}
    for F, W, P in sc.SHAPES:
        nbx, R = sc.make_plan(P, F * W, cap, rmax, few, rwant, block)
        out[(F, W, P)] = (nbx, R, sc.block_chunks(P, nbx, R, block), sc.uncapped_blocks(P, F * W, few, rwant, block),
                          sc.sum_rows_trips(W * nbx, unroll, block))
    return out


def test_the_shapes_reach_every_path_of_the_launch_plan():
    cap, rmax, few, rwant, block, unroll = _plan_constants()
    plans = _plans()
    # R = 1 with one partial chunk, with full chunks only, with full chunks and a partial one
    for P, want in ((1, [1]), (63, [63]), (255, [255]), (256, [256]), (257, [256, 1]), (1000, [256, 256, 256, 232])):
        nbx, R, chunks, _, _ = plans[(3, 3, P)]
        assert R == 1 and [c[0] for c in chunks] == want
    # R > 1, the last block's share one partial chunk and the rest past the pupil
    nbx, R, chunks, wanted, _ = plans[(8, 8, 49169)]
    assert (nbx, R) == (33, 6) and wanted == nbx and chunks[-1] == [17, 0, 0, 0, 0, 0] and all(c == [256] * 6 for c in chunks[:-1])
    # the cap: fewer blocks than the plan wanted, and one block with no chunk at all
    nbx, R, chunks, wanted, _ = plans[(16, 16, 33001)]
    assert (nbx, R) == (16, 9) and wanted == 17 and wanted * 256 > cap >= nbx * 256
    assert chunks[15] == [0] * 9 and chunks[14] == [256, 256, 233, 0, 0, 0, 0, 0, 0]
    # sum_rows: the unrolled loop once for every thread, then a tail for thread 0 only / for the first 55 threads
    nbx, R, _, _, (big, tail) = plans[(1, 1, 524291)]
    assert (nbx, R) == (2049, 1) and 1 * nbx > (unroll - 1) * block
    assert big == [1] * block and tail == [1] + [0] * (block - 1)
    nbx, R, _, _, (big, tail) = plans[(1, 3, 179203)]
    assert (nbx, R) == (701, 1) and 3 * nbx == 2103
    assert big == [1] * block and tail == [1] * 55 + [0] * (block - 55)
    # no other shape enters the unrolled loop, and none needs the rmax branch
    for (F, W, P), (nbx, R, _, _, (big, _)) in plans.items():
        assert R <= rmax
        if (F, W, P) not in ((1, 1, 524291), (1, 3, 179203)):
            assert max(big) == 0
    # the restated planner covers every ray exactly once
    for (F, W, P), (nbx, R, chunks, _, _) in plans.items():
        assert sum(sum(c) for c in chunks) == P


@pytest.mark.parametrize("shape", sc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_reference_moments_are_exact(shape):
    """The fp64 sums equal the int64 sums of the underlying integers bit for bit: nothing was rounded, so any order of
    summation gives the same fp64 number and the GPU tests may ask for equality."""
    F, W, P = shape
    assert P * W <= sc.MAX_RAYS
    for expanded in (False, True):
        ky, kx, ok = sc.ints(F, W, P, expanded)
        x, y, okf = sc.rays(F, W, P, expanded)
        assert torch.equal((y[0].double() * sc.SCALE).to(torch.int64), ky) and torch.equal((x[0].double() * sc.SCALE).to(torch.int64), kx)
        mi = sc.integer_moments(ky, kx, ok)
        assert int(mi.abs().max()) < 2 ** 46
        assert torch.equal(sc.reference_moments(x, y, okf), mi.double() * sc.UNITS)
        dead = (~ok).sum((1, 2))
        assert int(dead.max()) >= 1 and not bool(ok[0, 0, 0])
        if P * W >= 1000:
            frac = dead.double() / (P * W)
            assert 0.03 < float(frac.min()) and float(frac.max()) < 0.33
        if not expanded:
            assert int(ky[~ok].abs().max()) == 0 and int(kx[~ok].abs().max()) == 0        # dead rays at the origin
    # the columns can be told apart: no two of the seven moments of a field are equal but sum y = sum ok y
    m = sc.reference_moments(x, y, okf)
    if P * W >= 63:
        for a in range(7):
            for b in range(a + 1, 7):
                assert ((m[:, a] != m[:, b]).all()) or (a, b) == (0, 1) or (a, b) == (4, 5), (a, b)


def test_dead_rays_off_the_origin_tell_the_sum_over_all_rays_from_the_sum_over_live_ones():
    x, y, ok = sc.rays(3, 3, 257, dead_at_zero=False)
    m = sc.reference_moments(x, y, ok)
    assert (m[:, 0] != m[:, 1]).all() and (m[:, 4] != m[:, 5]).all()
    ky, kx, okb = sc.ints(3, 3, 257, dead_at_zero=False)
    assert torch.equal(m, sc.integer_moments(ky, kx, okb).double() * sc.UNITS)


def test_seed_formula_is_exact_before_its_one_rounding():
    """g0 + ok (g1 + 2 y g2) in fp64 equals the integer evaluation in units of 2^-18, so the reference gradient is the exact
    value rounded to fp32 once."""
    F, W, P = 3, 3, 1000
    ky, kx, ok = sc.ints(F, W, P)
    x, y, okf = sc.rays(F, W, P)
    g = sc.seeds(F)
    gi = (g * 256).to(torch.int64)
    assert torch.equal(gi.double() / 256, g) and int(gi.abs().max()) < 1024
    q = gi.reshape(F, 1, 1, sc.NMOM)
    exact = q[..., 0] * 1024 + ok.to(torch.int64) * (q[..., 1] * 1024 + 2 * ky * q[..., 2])          # units of 2^-18
    assert int(exact.abs().max()) < 2 ** 53
    gx, gy = sc.reference_seeds(x, y, okf, g)
    assert torch.equal(gy[0], (exact.double() / 2 ** 18).float())
    assert gx.shape == gy.shape == y.shape


def test_layouts_keep_the_values_and_change_the_strides():
    x, y, ok = sc.rays(3, 3, 63)
    for layout in sc.LAYOUTS:
        for which, t in (("x", x), ("y", y), ("ok", ok)):
            v = sc.lay_out(t, layout, which)
            assert v.shape == t.shape
            if not (layout == "y_expanded" and which == "y"):
                assert torch.equal(v, t)
    assert sc.lay_out(y, "fwp", "y").stride()[2:] == (1, 63)
    assert sc.lay_out(y, "slice", "y").stride() == (5 * 126 * 3, 126 * 3, 6, 1)
    assert sc.lay_out(y, "y_expanded", "y").stride(3) == 0
    assert sc.lay_out(ok, "ok_contiguous", "ok").is_contiguous() and not sc.lay_out(y, "ok_contiguous", "y").is_contiguous()
    assert not sc.lay_out(x, "x_fwp", "x").is_contiguous() and sc.lay_out(y, "x_fwp", "y").is_contiguous()


def test_coincident_rays_drive_the_closed_form_below_zero():
    """The teeth of the degenerate-field test: on these very moments, plain fp64 evaluation of M2 - 2 m M1 + m^2 M3 is negative
    for at least 5 % of the values (sqrt of it is NaN), although all rays of a field coincide -- over the one-n launches taken
    together and in the launch that mixes every n.  (Up to 32 copies of an fp32 square sum without any rounding in fp64: n = 3,
    5, 7 are exactly 0 in every order of summation and stand for the fields that must stay untouched.)"""
    sets = sc.coincident_sets()
    assert [name for name, _, _ in sets] == ["n3", "n5", "n7", "n48", "n777", "mixed"]
    neg = {}
    for name, m, n in sets:
        assert m.shape == (sc.COINCIDENT_LENSES, sc.NMOM)
        var = sc.closed_form_variance(m, float(n))
        neg[name] = var < 0
        # what is not negative is rounding noise as well: within the bound the GPU test holds the kernels to
        assert (np.abs(var) <= 16 * 2.0 ** -53 * m[:, 2] / n).all(), name
    assert np.concatenate([neg[k] for k in ("n3", "n5", "n7", "n48", "n777")]).mean() >= 0.05
    assert neg["mixed"].mean() >= 0.05
    assert neg["n48"].mean() >= 0.05 and neg["n777"].mean() >= 0.05 and not neg["n3"].any()
