"""The ray-aiming cases and bounds of tests/aim_cases.py and the pupil-position references of tests/pupil_ref.py, judged on
the CPU from the references alone: every case reaches its branch and decides nothing on a knife edge, the allowance A holds
an fp64 evaluation in the kernel's own order of operations (sufficient), ten deliberately wrong evaluations exceed the bound
(sharp), and the numpy fp32 tree is the torch chain bit for bit.  Run with -s for the ratios."""
import numpy as np
import pytest
import torch

import aim_cases as C
import aim_iter_ref as R
import pupil_ref
from conftest import assert_matches_fixture, load_golden


# ------------------------------------------------------------------ the conditions on the cases
@pytest.mark.parametrize("name", C.CASES)
def test_no_decision_on_a_knife_edge(name):
    """The live / dead pattern of the tee rays, step by step, is the same with h / 2, h and 2 h, and with the autograd
    Jacobian (which looks at the centre ray alone)."""
    inp, tee_ref, rs = C.inputs(name)
    for n_iter in C.N_ITERS:
        ref = C.reference(name, n_iter)
        for h in (C.H / 2, 2 * C.H):
            other = R.aim_detail(inp, n_iter, tee_ref, rs, jacobian="central", h=h)
            assert all(torch.equal(a, b) for a, b in zip(ref["dead"], other["dead"])), (name, n_iter, h)
        auto = C.reference(name, n_iter, "autograd")
        assert all(torch.equal(a, b) for a, b in zip(ref["dead"], auto["dead"])), (name, n_iter)
        assert torch.isfinite(torch.stack(ref["map"])).all()


def test_every_case_reaches_its_branch():
    for name in C.CASES:
        a = C.arrays(name)
        B, K = a["c"].shape
        for n_iter in C.N_ITERS:
            dead = torch.stack(C.reference(name, n_iter)["dead"])
            if name in C.DEAD_TEE:
                assert dead.any() and not dead.all(), name
            elif name == "back-marginal":
                assert dead.all() and not C.reference(name, n_iter)["ok_m"].any()
                assert np.array_equal(C.want(name, n_iter), np.stack([np.ones((1, 4, 1)), np.ones((1, 4, 1)), np.zeros((1, 4, 1))]))
            else:
                assert not dead.any(), name
        if name in C.ASPHERIC:
            kind = a["kind"].astype(bool)
            assert kind.any() and not kind.all() and a["mask"][kind].all()
            assert (a["poly"][kind] != 0).any() and (a["kappa"][kind] != 0).any()
        else:
            assert a["kind"] is None
    # back-mixed: under allow_backward = 0 exactly the bottom tee ray of the two outer fields takes no step, at every step;
    # the marginal ray lives; under 1 everything lives
    for n_iter in C.N_ITERS:
        r = C.reference("back-mixed", n_iter)
        assert r["ok_m"].all()
        for dead in r["dead"]:
            assert dead[0, :, :, 0].tolist() == [[False] * 3, [False] * 3, [True, False, False], [True, False, False]]
        assert not torch.stack(C.reference("back-mixed-allow", n_iter)["dead"]).any()
        assert np.abs(C.want("back-mixed", n_iter) - C.want("back-mixed-allow", n_iter)).max() > 1e-3
    # the shapes the table promises
    shapes = {n: C.arrays(n)["n"].shape + (len(C.arrays(n)["fields"]),) for n in C.CASES}
    assert shapes["cooke-f3w1"] == (1, 4, 1, 3) and shapes["batch6"] == (6, 4, 3, 4) and shapes["k1"][1] == 1
    assert shapes["k32"][1:3] == (32, 2) and shapes["mixed-kinds"][0] == 3 and shapes["tee-rs"][0] == 2
    b6 = C.arrays("batch6")
    assert not b6["mask"][1, 2:].any() and (b6["c"][1, 2:] == 0).all() and (b6["t"][1, 2:] == 0).all() and (b6["n"][1, 2:] == 1).all()
    assert b6["mask"][0].all() and len({tuple(r) for r in b6["c"].tolist()}) == 6
    mk = C.arrays("mixed-kinds")
    assert mk["kind"].tolist() == [[0, 1, 0, 0, 0], [0] * 5, [0, 1, 0, 0, 0]] and mk["poly"][2, 1, 3] != 0
    assert (mk["poly"][0, 1] != mk["poly"][2, 1]).all() or (mk["poly"][0, 1, 2:] == 0).all()
    tee = C.TEE_REF
    assert (tee[0] != tee[1]).all() and (tee[:, :, 0] != -tee[:, :, 1]).all() and (tee[:, :, 2] != 1).all() and C.RS[0] != C.RS[1]
    assert len({tuple(r) for r in tee.reshape(-1, 3).tolist()}) == 8


# ------------------------------------------------------------------ the bound: sufficient
@pytest.mark.parametrize("name", C.CASES)
def test_allowance_holds_the_kernel_ordered_evaluation(name):
    """An fp64 evaluation in the kernel's order of operations differs from the oracle-ordered restatement by less than A,
    element by element; and what the central difference costs against autograd, from the reference alone."""
    inp, tee_ref, rs = C.inputs(name)
    for n_iter in C.N_ITERS:
        got = R.aim_kernel_order(inp, n_iter, tee_ref, rs)
        q = C.ratio(got, C.want(name, n_iter), C.allowance(name, n_iter))
        trunc = C.truncation(name, n_iter).reshape(3, -1).max(axis=1)
        print(f"AIM-SUFFICIENT {name} N={n_iter}: kernel order / A  x_scale {q[0]:.2e} y_scale {q[1]:.2e} y_offset {q[2]:.2e}"
              f"   A <= {C.allowance(name, n_iter).max():.2e}   central - autograd <= {trunc.max():.2e}")
        assert (q <= 1).all(), (name, n_iter, q)


# ------------------------------------------------------------------ the bound: sharp
SHARP = {"sum-jacobian": ("batch6",), "sagittal-y0": ("tee-rs",), "mu-fp64": ("batch6", "k32"), "rs-f-line": ("batch6",),
         "dead-steps": ("back-mixed", "cooke_wide"), "no-a10": ("mixed-kinds",), "next-wavelength": ("batch6", "k32"),
         "next-lens-poly": ("mixed-kinds",), "next-lens-rs": ("tee-rs",), "ignore-allow-backward": ("back-mixed",)}


@pytest.mark.parametrize("wrong", R.WRONG)
def test_a_wrong_evaluation_exceeds_the_bound(wrong):
    worst = 0.0
    for name in SHARP[wrong]:
        inp, tee_ref, rs = C.inputs(name)
        got = R.aim_kernel_order(inp, 2, tee_ref, rs, wrong=wrong)
        q = C.ratio(got.astype(np.float32), C.want(name, 2), C.bound(name, 2))
        print(f"AIM-SHARP {wrong} on {name} N=2: error / bound  x_scale {q[0]:.3g} y_scale {q[1]:.3g} y_offset {q[2]:.3g}")
        worst = max(worst, q.max())
    assert worst > 1, (wrong, worst)


def test_the_right_evaluation_rounded_to_fp32_is_within_the_bound():
    for name in ("batch6", "mixed-kinds", "tee-rs", "back-mixed"):
        inp, tee_ref, rs = C.inputs(name)
        got = R.aim_kernel_order(inp, 2, tee_ref, rs).astype(np.float32)
        assert (C.ratio(got, C.want(name, 2), C.bound(name, 2)) <= 1).all()


# ------------------------------------------------------------------ the pupil-position references
def _torch_chain32(c, t, n):
    from torchoptics_amd import paraxial
    m = paraxial.reduce_abcd(paraxial.interface_propagation_abcd(torch.tensor(c), torch.tensor(t), torch.tensor(n)))
    return (m[:, 0, 1] / m[:, 0, 0]).numpy()


@pytest.mark.parametrize("K", range(1, 33))
def test_fp32_tree_is_the_torch_chain_bit_for_bit(K):
    c, t, n = pupil_ref.seeded_front(K, 20, 1000 + K, padded=K % 4 == 0)
    got, want = pupil_ref.tree32(c, t, n), _torch_chain32(c, t, n)
    assert want.dtype == np.float32 and np.isfinite(want).all()
    assert np.array_equal(got.view(np.int32), want.view(np.int32))


def test_fp32_tree_on_the_paraxial_fixture():
    import yaml_free_lenses as L
    from torchoptics_amd import paraxial
    g9 = load_golden("G9_paraxial")
    for name in ("doublet", "cooke", "tessar"):
        lens, _, _ = L.build(name, "cpu", grad=False)
        front = lens.up_to_stop()
        c, t, n = front.c.numpy(), front.t.numpy(), paraxial._with_air_in_front(front.nd).numpy()
        got = pupil_ref.tree32(c, t, n)
        assert np.array_equal(got.view(np.int32), paraxial.compute_pupil_position(lens).numpy().view(np.int32))
        assert_matches_fixture(got, g9[name][2:3], 0, rtol=2e-6, what="pupil position")


@pytest.mark.parametrize("K", (1, 2, 3, 7, 16, 31, 32))
def test_pupil_allowance_holds_the_kernel_ordered_evaluation(K):
    """The float64 evaluation in the kernel's order against float64 autograd: inside twice the error bound, element by
    element, value and gradients; and the bound is small against one fp32 rounding wherever the element is not itself
    small by cancellation."""
    c, t, n = pupil_ref.seeded_front(K, 65, 2000 + K, padded=True)
    g_z = np.linspace(-1.5, 2.0, 65)
    z64, *g64 = pupil_ref.grads64(c, t, n, g_z)
    z, *g = pupil_ref.kernel_order(c, t, n, g_z)
    assert np.array_equal(pupil_ref.fast64(c, t, n), z64)
    worst = float((np.abs(z.v - z64) / (2 * z.e)).max())
    assert (np.abs(z.v - z64) <= 2 * z.e).all() and (2 * z.e <= 1e-2 * pupil_ref.U32 * np.abs(z64)).all()
    for errs, want in zip(g, g64):
        v, e = pupil_ref.stacked(errs)
        assert v.shape == want.shape and (np.abs(v - want) <= 2 * e).all()
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = max(worst, float(np.where(e > 0, np.abs(v - want) / (2 * e), 0.0).max()))
    print(f"PUPIL-SUFFICIENT K={K}: kernel order / allowance {worst:.3f}")
