"""The case table of the metrics matrix (tests/metrics_cases.py) and its restatement (tests/metrics_ref.py), on the CPU:
the premises of the cases, four physical properties that a mere copy of the product's formulas would not have, and the
sharpness of the gates -- every wrong restatement of metrics_ref.WRONG misses the gate of a case."""
import math

import numpy as np
import pytest
import torch

import metrics_cases as MC
import metrics_ref as MR


# ---------------------------------------------------------------------------------------------------------------- premises
def test_the_table_holds_what_it_says():
    specs = MC.CASES
    assert len(MC.NAMES) == len(set(MC.NAMES)) == 7 + 18 + 4 + 2 + 36 + 1
    assert MC.DEAD == ("ri-cooke_wide-dead",)
    assert sum(s["metric"] == "aim" and s["grad"] for s in specs.values()) == 1
    assert {s["n_iter"] for s in specs.values() if s["metric"] == "ri" and s["vig"]} == {1, 3}
    assert any(s["metric"] == "ri" and len(s["wavelengths"]) == 1 for s in specs.values())
    lens, _, _ = MC.build(specs["dist-batch3"], "cpu")
    assert sorted(lens.structure.mask.sum(axis=1).tolist()) == [5, 7, 8] and len(set(lens.structure.stop_idx.tolist())) == 2
    assert MC.build(specs["dist-singlet"], "cpu")[0].structure.stop_idx.tolist() == [0]
    lens, _, leaves = MC.build(specs["dist-dg-asph"], "cpu")
    assert "kappa" in leaves and (lens.kappa != 0).sum() == 2


@pytest.mark.parametrize("name", MC.NAMES)
def test_every_reference_ray_is_alive_in_both_twins(name):
    r64, r32 = MC.reference(name), MC.reference(name, torch.float32)
    if name == "aim-singlet":
        assert r64["value"] == 0 and isinstance(r64["value"], int) and r32["value"] == 0
        return
    assert np.isfinite(r64["value"]).all() and np.isfinite(r32["value"]).all()
    for g in (r64["grads"] or {}).values():
        assert np.isfinite(g).all()
    if name in MC.DEAD:
        # the one case with dead rays: the same rays die in both twins, and fields of both kinds exist
        assert np.array_equal(r64["ok"], r32["ok"]) and np.array_equal(r64["valid"], r32["valid"])
        assert r64["valid"].any() and not r64["valid"].all() and r64["valid"][:, 0].all()
        assert (r64["value"][~r64["valid"]] == 1.0).all()
    else:
        assert r64["ok"].all() and r32["ok"].all()
        if r64["valid"] is not None:
            assert r64["valid"].all()


def test_dead_fields_report_one_with_zero_gradient():
    name = MC.DEAD[0]
    spec = MC.CASES[name]
    lens, specs, _ = MC.build(spec, "cpu")
    S = MR.System(lens, specs)
    ri, valid, _ = MC.evaluate(spec, S)
    g = MR.leaf_gradients(S, ri, (~valid).double())
    assert all((v == 0).all() for v in g.values())


def test_batch_rows_of_the_restatement_are_its_single_lens_runs():
    for name in ("dist-batch3", "ri-batch3-N1"):
        spec, ref = MC.CASES[name], MC.reference(name)
        for b, (_, single) in enumerate(MC.singles(spec)):
            one = MC.run(single, name)
            assert np.abs(one["value"][0] - ref["value"][b]).max() < 1e-12


def test_the_aimed_fan_of_the_restatement_is_aim_iter_ref_s():
    """Without a vignetting function the fan is one for all fields, and aim_iter_ref.aimed_fan builds the same one."""
    import aim_iter_ref as AR
    lens, specs, _ = MC.build(MC.CASES["ri-batch3-N3"], "cpu")
    S = MR.System(lens, specs)
    xs, ys = [0.0, 0.0, 1.0], [1.0, -1.0, 0.0]
    m = S.aim_map(MC.FIELDS_RI, [MR.LINES[w] for w in MC.CDF], 3, False)
    x, y = S.vignette(MC.FIELDS_RI, xs, ys, False)
    half = (S.epd / 2).reshape(-1, 1, 1, 1)
    want = AR.aimed_fan(tuple(a[:, :, 0, :] for a in m), xs, ys, specs.epd)
    assert torch.equal(torch.clamp(x * m[0], -2, 2) * half, want[0]) and torch.equal(torch.clamp(y * m[1] + m[2], -2, 2) * half, want[1])
    assert (m[1] != 1).any() and (m[2] != 0).any()


def test_the_measured_constants_are_the_table_s():
    """C_MEASURED and C_CASE against measure() on this table: no case exceeds the recorded maxima, and none of them is
    recorded looser than twice what the table gives."""
    worst, _, table = MC.measure(out=lambda s: None)
    assert set(worst) == set(MC.C_MEASURED)
    for (name, leaf), c in MC.C_CASE.items():
        assert 0.5 * c <= table[(name, leaf)] <= c * (1 + 1e-3), (name, leaf)
    for key, c in MC.C_MEASURED.items():
        assert 0.5 * c <= worst[key] <= c * (1 + 1e-3), key
    # a case has its own constant only where it would set the kind's alone: at least twice the rest of the table
    for (name, leaf), c in MC.C_CASE.items():
        assert c > 2 * MC.C_MEASURED[(MC.CASES[name]["metric"], leaf)]


# ----------------------------------------------------------------------------------------------------------------- physics
def _system(lens_name, hfov=None, fields=MC.FIELDS_DIST, **kw):
    spec = MC._spec("dist", lens_name, fields, hfov=hfov, **kw)
    lens, specs, _ = MC.build(spec, "cpu")
    return MR.System(lens, specs)


def test_distortion_vanishes_as_the_square_of_the_field():
    """Third-order distortion: d(2h) / d(h) -> 4 towards the axis -- only with the right EFL and defocus term (a wrong
    EFL leaves a constant, a wrong defocus a term that does not vanish)."""
    S = _system("singlet", hfov=10.0)
    with torch.no_grad():
        d = MR.distortion(S, (0.125, 0.25, 0.5))[0][0].numpy()
    r = d[1:] / d[:-1]
    print(f"METRICS-PHYS d(2h)/d(h) of the singlet at 10 degrees: {r}")
    # 4.0015 and 4.0057: the fifth-order term, quartering with the field.  (Further in, the fp32 rounding of the field
    # sines that the tracer is fed -- and this restatement with it -- shows: 4.002 at 0.0625, where d is 2e-5.)
    assert abs(r[1] - 4) < 0.01 and abs(r[0] - 4) < 0.0025
    for wrong in ("no-defocus", "last-gap-in"):
        with torch.no_grad():
            dw = MR.distortion(S, (0.0625, 0.125), wrong)[0][0].numpy()
        assert abs(dw[1] / dw[0] - 4) > 0.1, wrong


@pytest.mark.parametrize("lens_name", ["cooke", "dg-asph"])
def test_distortion_and_illumination_do_not_change_with_the_scale_of_the_lens(lens_name):
    """c / k, t k, epd k (and the aspheric terms with their powers of k): the same angles everywhere.  k = 2 keeps every
    fp32 input exact, so the two runs differ by fp64 rounding only."""
    from torchoptics_amd import lens_modeling as lm
    spec = MC._spec("ri", lens_name, MC.FIELDS_RI, wavelengths=MC.CDF, n_iter=1)
    lens, specs, _ = MC.build(spec, "cpu")
    big = lm.Lens(lens.structure, lens.c / 2, lens.t * 2, lens.nd, lens.v,
                  *((lens.kappa, lens.poly / torch.tensor([8.0, 32.0, 128.0, 512.0])) if lens.kappa is not None else ()))
    big_specs = lm.Specs(specs.structure, specs.epd * 2, specs.hfov)
    with torch.no_grad():
        a, b = MR.System(lens, specs), MR.System(big, big_specs)
        assert (MR.distortion(a, MC.FIELDS_DIST)[0] - MR.distortion(b, MC.FIELDS_DIST)[0]).abs().max().item() < 1e-11
        assert (MR.relative_illumination(a, MC.FIELDS_RI, MC.CDF, 1)[0]
                - MR.relative_illumination(b, MC.FIELDS_RI, MC.CDF, 1)[0]).abs().max().item() < 1e-11


@pytest.mark.parametrize("lens_name", ["singlet", "doublet", "cooke", "tessar", "dg-asph", "batch3"])
def test_efl_is_what_a_paraxial_ray_sees(lens_name):
    """EFL = -h / u' of a ray that enters parallel to the axis at a small height h, to O(h^2): the error quarters when h
    halves, and at h = 0.05 mm it is below 1e-5 of the focal length."""
    S = _system(lens_name)
    err = []
    with torch.no_grad():
        efl = S.first_order()[0]
        for h in (0.1, 0.05):
            S._z = torch.zeros(S.B, dtype=S.dtype)                       # launched at the first vertex plane
            try:
                y = (h / (S.epd / 2)).reshape(S.B, 1, 1, 1)
                _, _, _, cy, ok, _ = S.trace(S.full(), torch.zeros_like(y), y, torch.zeros(S.B, 1, 1, 1, dtype=S.dtype),
                                             S.mu_of(S.indices([MR.LINES["d"]])))
            finally:
                S._z = None
            cy = cy.reshape(S.B)
            assert ok.all()
            err.append(((-h / (cy / torch.sqrt(1 - cy * cy)) - efl) / efl).numpy())
    print(f"METRICS-PHYS {lens_name}: EFL {efl.numpy()}, ray - matrix at h = 0.1, 0.05: {err[0]}, {err[1]}")
    assert np.abs(err[1]).max() < 1e-5
    assert np.allclose(err[0] / err[1], 4.0, atol=0.02)


# |three-ray illumination - area ratio of the rim's image| measured here (d line, three aiming steps, 720 rim points) at
# fields 0.5 / 1: doublet 1.4e-5 / 1.1e-4, Cooke 1.3e-6 / 1.4e-3, Tessar 5.6e-5 / 5.3e-3.  The three rays span an ellipse;
# the true image of the pupil in direction space is egg-shaped off axis, so the two agree to parts in a thousand, not to
# rounding.  The tolerance is twice the largest.
RIM_TOL = 0.011


@pytest.mark.parametrize("lens_name", ["doublet", "cooke", "tessar"])
def test_three_ray_illumination_is_the_area_of_the_pupil_in_direction_space(lens_name):
    n_rim = 720
    spec = MC._spec("ri", lens_name, MC.FIELDS_RI, n_iter=3)
    lens, specs, _ = MC.build(spec, "cpu")
    S = MR.System(lens, specs)
    with torch.no_grad():
        ri = MR.relative_illumination(S, MC.FIELDS_RI, ("d",), 3)[0][0, :, 0].numpy()
        th = torch.arange(n_rim, dtype=torch.float64) * (2 * math.pi / n_rim)
        m = S.aim_map(MC.FIELDS_RI, [MR.LINES["d"]], 3, False)
        x = (torch.cos(th).reshape(1, 1, -1, 1) * m[0]).expand(1, 3, n_rim, 1)
        y = (torch.sin(th).reshape(1, 1, -1, 1) * m[1] + m[2]).expand(1, 3, n_rim, 1)
        _, _, cx, cy, ok, _ = S.trace(S.full(), x, y, S.sines(MC.FIELDS_RI).reshape(1, 3, 1, 1), S.mu_of(S.indices([MR.LINES["d"]])))
        assert ok.all()
        cx, cy = cx[0, :, :, 0].numpy(), cy[0, :, :, 0].numpy()
    area = 0.5 * np.abs((cx * np.roll(cy, -1, axis=1) - np.roll(cx, -1, axis=1) * cy).sum(axis=1))      # shoelace
    rim = area / area[0]
    print(f"METRICS-PHYS {lens_name}: three rays {ri}, rim polygon {rim}, difference {ri - rim}")
    assert np.abs(ri - rim).max() < RIM_TOL
    assert abs(rim[0] - 1) == 0 and (rim[1:] < 1).all()


# --------------------------------------------------------------------------------------------------------------- sharpness
# wrong restatement -> the cases that catch it (value gate unless a leaf is named)
CATCHES = {
    "no-defocus": [("dist-cooke-10deg", None), ("dist-tessar", None)],
    "last-gap-in": [("dist-cooke", None)],
    "sin-for-tan": [("dist-cooke-10deg", None)],
    "per-wavelength-axis": [("ri-cooke-N1", None)],
    "sagittal-cy": [("ri-tessar-N0", None)],
    "swap-upper-lower": [("ri-doublet-N3", None)],
    "f-line": [("dist-doublet", None), ("aim-cooke-N0-real", None), ("ri-cooke-w1", None)],
    "unvignetted-height": [("aim-tessar-N3-real-vig", None), ("aim-dg-N1-paraxial-vig", None)],
    "z-detached": [("dist-cooke", "c"), ("ri-tessar-N1", "t"), ("aim-cooke-N1-real", "c")],
    "neighbour-last": [("dist-batch3", None)],
}


def test_every_wrong_restatement_is_listed():
    assert set(CATCHES) == set(MR.WRONG)


@pytest.mark.parametrize("wrong", MR.WRONG)
def test_a_wrong_restatement_misses_the_gate(wrong):
    """Against the WIDEST gate of the case, the fast mode's."""
    for name, leaf in CATCHES[wrong]:
        bad = MC.run(MC.CASES[name], name, wrong=wrong)
        e = MC.errors(bad["value"], bad["grads"], MC.reference(name))[leaf]
        g = MC.gate(name, "fast", leaf)
        print(f"METRICS-SHARP {wrong} on {name} ({'values' if leaf is None else 'd/d' + leaf}): error / fast gate {e / g:.1f}")
        assert e > 2 * g, (wrong, name, leaf, e, g)
