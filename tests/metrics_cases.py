"""
The case table of tests/test_gpu_metrics_matrix.py and its references (CPU only; checked by tests/test_metrics_cases_cpu.py).

compute_distortion, compute_relative_illumination and compute_ray_aiming_error (torchoptics_amd/metrics.py) reach the trace
kernels as nothing else does: one chief ray per (lens, field) seeded through y and cy together; three tee rays seeded through
cx and cy alone, behind a torch.where; aimed fans of three points through tl_aim_fan, with and without a vignetting function;
a lens cut at its stop, whose image plane is the stop plane and whose marginal ray sits in a denominator; padded batches with
a per-lens last row.  Every case is a handful of rays:

  dist-*   fields (0.25, 0.5, 0.75, 1), d line: the four yaml lenses at 25 degrees (the singlet's stop is row 0), the Cooke
           triplet at 10 degrees and fields (0.05, 0.1, 0.2) -- d = 1e-5 .. 1e-4, where (y - y_ref) / y_ref cancels --, the
           double Gauss with aspheric rows (kappa and poly take gradients), and doublet + Cooke + Tessar as one padded batch
           (5, 7 and 8 rows: per-lens last, defocus, EFL)
  ri-*     fields (0, 0.5, 1), lines C, d, F: the same lenses and the batch at n_ray_aiming_iter 0, 1, 3; Cooke and Tessar
           under the linear vignetting function with factors (0.3, 0.1, 0.2) at N = 1 (the op sequence) and N = 3 (the kernel
           with tee_ref); the Cooke triplet at epd 12 and 32 degrees, where tee rays die (`dead`); the Cooke triplet on the d
           line alone (W = 1)
  aim-*    fields (0.5, 0.707, 1): Cooke, Tessar and the spherical double Gauss at N = 0, 1, 3, 'real' and 'paraxial', with
           and without the vignetting function; the singlet, which returns the integer 0.  aim-cooke-N1-real takes gradients.

Every case runs in strict and in fast mode (the default mode of torchoptics_amd.ops).

THE GATES.  Values are compared element by element in ABSOLUTE terms (a distortion of 1e-5 has no meaningful relative error),
gradients per leaf as rel-L2 of sum(w metric) with the seeded weights of metrics_ref.weights.  The gate of an output kind is

    max(4 C_MEASURED[kind], FLOOR) (x K_FAST in fast mode)

with C_MEASURED the worst distance of the restatement's fp32 twin from its fp64 run over the whole table, measured on the CPU
from the reference alone (`python tests/metrics_cases.py`, profiles/metrics_accuracy.txt); the factor 4 is for the kernels'
operation order, K_FAST = 10 as in fwd_cases.py.  FLOOR is four fp32 ulps of the quantity's scale: all three metrics are
differences of ratios near 1, and a rel-L2 is relative already.  A (metric, leaf) whose noise one case dominates gets that
case its own constant (C_CASE) and the rest of the table a tighter one.

What the cases found (profiles/metrics_accuracy.txt): every value and every valid mask was inside its gate at once, the
distortion 3.0e-7 absolute at most in either mode, so the fp32 ABCD product behind EFL, BFL and y_ref costs nothing that the
fp32 trace of y does not cost already.  One gradient missed: dist-dg-asph in strict mode, d/d poly 1.035e-5 against a gate
of 7.7e-6, with the walk-back backward -- its reconstructed state at the front aspheric row is off by a few 1e-6, which the
polynomial terms multiply by their order (a4 .. a10: 2.6e-6, 5.6e-6, 8.7e-6, 1.2e-5), and the difference y - y_ref does not
average over one chief ray per field.  The checkpoint backward gives 1.9e-6 there; compute_distortion takes it now.  The
case closest to its gate after that is ri-cooke_wide-dead, strict, d/d t: 0.61 of it.
"""
import dataclasses
import zlib

import numpy as np
import torch

import metrics_ref as MR

MODES = ("strict", "fast")
K_FAST = 10.0
FLOOR = 4 * 2.0 ** -23
CDF = ("C", "d", "F")
FIELDS_DIST, FIELDS_RI, FIELDS_AIM = (0.25, 0.5, 0.75, 1.0), (0.0, 0.5, 1.0), (0.5, 0.707, 1.0)
VIG = (0.3, 0.1, 0.2)                       # vig_up, vig_down, vig_x: unequal on purpose
BATCH3 = ("doublet", "cooke", "tessar")


def _spec(metric, lens, fields, **kw):
    s = dict(metric=metric, lens=lens, fields=fields, hfov=None, wavelengths=("d",), n_iter=1, vig=False, aim_mode="real",
             grad=metric != "aim", dead=False)
    s.update(kw)
    return s


CASES = {}
for _l in ("singlet", "doublet", "cooke", "tessar"):
    CASES[f"dist-{_l}"] = _spec("dist", _l, FIELDS_DIST)
CASES["dist-cooke-10deg"] = _spec("dist", "cooke", (0.05, 0.1, 0.2), hfov=10.0)
CASES["dist-dg-asph"] = _spec("dist", "dg-asph", FIELDS_DIST)
CASES["dist-batch3"] = _spec("dist", "batch3", FIELDS_DIST)
for _l in ("singlet", "doublet", "cooke", "tessar", "dg-asph", "batch3"):
    for _n in (0, 1, 3):
        CASES[f"ri-{_l}-N{_n}"] = _spec("ri", _l, FIELDS_RI, wavelengths=CDF, n_iter=_n)
for _l in ("cooke", "tessar"):
    for _n in (1, 3):
        CASES[f"ri-{_l}-vig-N{_n}"] = _spec("ri", _l, FIELDS_RI, wavelengths=CDF, n_iter=_n, vig=True)
CASES["ri-cooke_wide-dead"] = _spec("ri", "cooke_wide", FIELDS_RI, wavelengths=CDF, n_iter=1, dead=True)
CASES["ri-cooke-w1"] = _spec("ri", "cooke", FIELDS_RI, wavelengths=("d",), n_iter=1)
for _l in ("cooke", "tessar", "dg"):
    for _n in (0, 1, 3):
        for _m in ("real", "paraxial"):
            for _v in (False, True):
                CASES[f"aim-{_l}-N{_n}-{_m}{'-vig' if _v else ''}"] = _spec("aim", _l, FIELDS_AIM, n_iter=_n, aim_mode=_m, vig=_v)
CASES["aim-cooke-N1-real"]["grad"] = True
CASES["aim-singlet"] = _spec("aim", "singlet", FIELDS_AIM)
NAMES = tuple(CASES)
DEAD = tuple(n for n, s in CASES.items() if s["dead"])

# The fp32 twin's worst distance from the fp64 restatement over the table (`python tests/metrics_cases.py`): values absolute,
# gradients rel-L2 per (metric, leaf).  C_CASE: the cases that would otherwise set a (metric, leaf) constant alone.
C_MEASURED = {
    "dist": 3.7426e-07, ("dist", "c"): 6.8626e-06, ("dist", "t"): 1.2464e-05, ("dist", "nd"): 7.2184e-06,
    ("dist", "v"): 4.3686e-10, ("dist", "kappa"): 3.6401e-07, ("dist", "poly"): 1.9294e-06,
    "ri": 1.3724e-06, ("ri", "c"): 1.7226e-05, ("ri", "t"): 1.4441e-05, ("ri", "nd"): 1.9025e-05, ("ri", "v"): 1.3489e-06,
    ("ri", "kappa"): 1.5320e-06, ("ri", "poly"): 3.3100e-06,
    "aim": 6.8252e-07, ("aim", "c"): 4.3331e-07, ("aim", "t"): 6.6443e-07, ("aim", "nd"): 1.4128e-06, ("aim", "v"): 0.0}
# dist-cooke-10deg: d is 1e-5 .. 2e-4 there and its gradient a difference of the gradients of y and y_ref, fifty times its
# size; dist-singlet: d/d nd of the one glass, four times the next lens'
C_CASE = {("dist-cooke-10deg", "c"): 3.5656e-04, ("dist-cooke-10deg", "t"): 1.8476e-04, ("dist-cooke-10deg", "nd"): 4.5295e-04,
          ("dist-singlet", "nd"): 2.8000e-05}


# ------------------------------------------------------------------------------------------------------------------
# lenses
# ------------------------------------------------------------------------------------------------------------------

def build(spec, device, grad=False):
    """(lens, specs, leaves) of a case on `device`; leaves are the flat c, t, nd, v (kappa, poly) the Lens is made of."""
    import yaml_free_lenses as L
    from torchoptics_amd import lens_modeling as lm, prescriptions as P
    name = spec["lens"]
    if name in L.PRESCRIPTIONS:
        lens, specs, leaves = L.build(name, device, hfov_deg=spec["hfov"] or L.HFOV_DEG, grad=grad)
    elif name == "cooke_wide":                                   # aim_cases.py: tee rays that miss or are totally reflected
        lens, specs, leaves = L.build("cooke", device, epd=12.0, hfov_deg=32.0, grad=grad)
    elif name in ("dg", "dg-asph"):
        lens, specs, leaves = P.double_gauss(device, requires_grad=grad, aspheres=name == "dg-asph")
    elif name == "batch3":                                       # as tests/test_gpu_batch.py builds its padded batch
        ps = [L.PRESCRIPTIONS[n] for n in BATCH3]
        st = lm.Structure(stop_idx=np.array(sum((p["stop_idx"] for p in ps), [])),
                          sequence=np.array(sum((p["sequence"] for p in ps), [])), default_device=device)
        leaves = {k: torch.tensor(sum((p[k] for p in ps), []), dtype=torch.float32, device=device, requires_grad=grad)
                  for k in ("c", "t", "nd", "v")}
        lens = lm.Lens(st, leaves["c"], leaves["t"], leaves["nd"], leaves["v"])
        specs = lm.Specs(st, torch.tensor([L.EPD] * 3, dtype=torch.float32, device=device),
                         torch.tensor([np.deg2rad(L.HFOV_DEG)] * 3, dtype=torch.float32, device=device))
    else:
        raise KeyError(name)
    if spec["vig"]:
        up, down, vx = (torch.full((len(lens),), v, dtype=torch.float32, device=device) for v in VIG)
        specs = dataclasses.replace(specs, vig_up=up, vig_down=down, vig_x=vx)
    return lens, specs, leaves


def singles(spec):
    """The single-lens cases a batch case is made of: [(lens name, spec)]."""
    return [(n, dict(spec, lens=n)) for n in BATCH3] if spec["lens"] == "batch3" else []


# ------------------------------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------------------------------

def seed_of(name):
    return zlib.crc32(name.encode())


def evaluate(spec, S, wrong=None):
    """(value, valid or None, ok or None) of the restatement on the system S."""
    if spec["metric"] == "dist":
        d, ok = MR.distortion(S, spec["fields"], wrong)
        return d, None, ok
    if spec["metric"] == "ri":
        return MR.relative_illumination(S, spec["fields"], spec["wavelengths"], spec["n_iter"], spec["vig"], wrong)
    e, ok = MR.ray_aiming_error(S, spec["fields"], spec["n_iter"], spec["vig"], spec["aim_mode"], wrong)
    return e, None, ok


def run(spec, name, dtype=torch.float64, wrong=None):
    """One evaluation: dict(value fp64 numpy (or the integer 0), valid, ok (numpy bool or None), grads {leaf: flat fp64
    numpy} or None)."""
    lens, specs, _ = build(spec, "cpu")
    S = MR.System(lens, specs, dtype)
    value, valid, ok = evaluate(spec, S, wrong)
    if not torch.is_tensor(value):
        return dict(value=value, valid=None, ok=None, grads=None)
    grads = MR.leaf_gradients(S, value, MR.weights(value.shape, seed_of(name))) if spec["grad"] else None
    return dict(value=value.detach().double().numpy(), valid=None if valid is None else valid.numpy(),
                ok=None if ok is None else ok.numpy(), grads=grads)


_REF = {}


def reference(name, dtype=torch.float64):
    """The restatement of a case in `dtype`: computed once, never changed."""
    key = (name, dtype)
    if key not in _REF:
        _REF[key] = run(CASES[name], name, dtype)
    return _REF[key]


# ------------------------------------------------------------------------------------------------------------------
# gates
# ------------------------------------------------------------------------------------------------------------------

def abs_err(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.isfinite(got).all(), "an element is not finite"
    return float(np.abs(got - want).max())


def rel_l2(got, want):
    got, want = np.asarray(got, dtype=np.float64).ravel(), np.asarray(want, dtype=np.float64).ravel()
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.isfinite(got).all(), "an element is not finite"
    nw = np.linalg.norm(want)
    return float(np.linalg.norm(got - want) / nw) if nw > 0 else float(np.linalg.norm(got))


def constant(name, leaf=None):
    """The measured noise constant behind a gate: the case's own if it has one, else its (metric[, leaf]) kind's."""
    metric = CASES[name]["metric"]
    key = metric if leaf is None else (metric, leaf)
    return C_CASE.get((name, leaf), C_MEASURED[key])


def gate(name, mode, leaf=None):
    """The gate of a case's values (leaf None: absolute) or of one leaf's gradient (rel-L2) in `mode`."""
    return max(4.0 * constant(name, leaf), FLOOR) * (K_FAST if mode == "fast" else 1.0)


def errors(got_value, got_grads, ref):
    """{None: absolute error of the values, leaf: rel-L2 of its gradient} of a run against the reference `ref`."""
    out = {None: abs_err(got_value, ref["value"])}
    if ref["grads"] is not None and got_grads is not None:
        for leaf, want in ref["grads"].items():
            out[leaf] = rel_l2(got_grads[leaf], want)
    return out


# ------------------------------------------------------------------------------------------------------------------
# the measurement behind C_MEASURED
# ------------------------------------------------------------------------------------------------------------------

def measure(out=print):
    """The fp32 twin against the fp64 restatement, case by case; returns ({kind: worst}, {kind: case that set it},
    {(case, kind): value})."""
    worst, where, table = {}, {}, {}
    for name, spec in CASES.items():
        r64, r32 = reference(name), reference(name, torch.float32)
        if not isinstance(r64["value"], np.ndarray):
            out(f"{name}: the integer {r64['value']}")
            continue
        e = errors(r32["value"], r32["grads"], r64)
        alive = "all alive" if (r64["ok"].all() and r32["ok"].all()) else f"dead rays {int((~r64['ok']).sum())}/{int((~r32['ok']).sum())}"
        out(f"{name}: {alive}; |value| {np.abs(r64['value']).min():.3e} .. {np.abs(r64['value']).max():.3e}; "
            + ", ".join(f"{'value' if k is None else 'd/d' + k} {v:.3e}" for k, v in e.items()))
        for k, v in e.items():
            key = spec["metric"] if k is None else (spec["metric"], k)
            table[(name, k)] = v
            if (name, k) in C_CASE:
                out(f"    own constant of ({name}, {k}): {v:.4e}")
            elif v > worst.get(key, -1.0):
                worst[key], where[key] = v, name
    for key in worst:
        second = max([v for (n, k), v in table.items() if n != where[key] and (n, k) not in C_CASE
                      and (CASES[n]["metric"] if k is None else (CASES[n]["metric"], k)) == key], default=0.0)
        out(f"worst {key}: {worst[key]:.4e} at {where[key]} (next: {second:.4e})")
    out("C_MEASURED = {" + ", ".join(f"{k!r}: {v:.4e}" for k, v in worst.items()) + "}")
    return worst, where, table


if __name__ == "__main__":
    measure()
