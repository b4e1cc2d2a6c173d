"""The cases the through-focus MTF kernels (tl_tfmtf_sums, tl_tfmtf_seed) are held on, shared by tests/test_gpu_tfmtf.py and
tests/test_tfmtf_cpu.py: the fourteen seeded fans of tests/focus_cases.py with their direction cosines, their live rule (ok != 0
and 1 - cx^2 - cy^2 > 0), the "poisoned" directions and their memory layouts, at the frequencies (0, 10, 25, 50) cycles / mm,
tangential and sagittal (J = 8), on the 16 planes -0.125 + z / 32 (exact in binary), which bracket the fans' foci at shifts of
about 0.04 to 0.33.  The two many-rows cases take J = 2 (25 cycles / mm, tangential and sagittal) and Z = 2."""
import numpy as np

import enclosed_cases as EC
import focus_cases as FC

SHAPES = FC.SHAPES
CASES = FC.CASES
FREQUENCIES = (0.0, 10.0, 25.0, 50.0)
DIRECTIONS = ("tangential", "sagittal")
PLANES = (-0.125, 2.0 ** -5, 16)
KEYS = ("x", "y", "cx", "cy")
rays, place, given_centre = FC.rays, FC.place, EC.given_centre


def frequencies_of(name):
    return (25.0,) if name.startswith("many-rows") else FREQUENCIES


def planes_of(name):
    return (0.0625, 2.0 ** -4, 2) if name.startswith("many-rows") else PLANES


def seeds(name, J, Z):
    """Dense seeds of both signs: g_sums [B,F,W,J,Z,2] (float64)."""
    B, F, W, _ = SHAPES[name]
    return np.random.default_rng(29 + sum(map(ord, name)) + J + Z).standard_normal((B, F, W, J, Z, 2))


def two_rays(a=0.05, zeta=0.0625, x0=0.25, y0=3.0):
    """Two live rays with slopes (0, +-a) through (x0, y0) at the shift zeta, given at the shift 0 (float32 [1,1,2,1]); and what
    the ROUNDED inputs say: (the half difference of the slopes v, the shift at which the two rays cross) in float64."""
    v = np.array([a, -a], np.float64)
    cy = (v / np.sqrt(1 + v * v)).astype(np.float32).reshape(1, 1, 2, 1)
    y = (y0 - zeta * v).astype(np.float32).reshape(1, 1, 2, 1)
    r = dict(x=np.full_like(y, x0), y=y, cx=np.zeros_like(y), cy=cy, ok=np.ones(y.shape, bool))
    c = cy.astype(np.float64).ravel()
    vr = c / np.sqrt(1 - c * c)
    yr = y.astype(np.float64).ravel()
    return r, float(vr[0] - vr[1]) / 2, float(-(yr[0] - yr[1]) / (vr[0] - vr[1]))


def point_fan(P=96, zeta=0.09375, seed=5):
    """P live rays that all pass through (0.5, 4) at the shift zeta (a plane of PLANES), up to the float32 rounding of their
    coordinates at the shift 0."""
    rng = np.random.default_rng(seed)
    u, v = 0.2 * (rng.random(P) - 0.5), 0.2 * (rng.random(P) - 0.5) + 0.1
    cz = 1 / np.sqrt(1 + u * u + v * v)
    sh = (1, 1, P, 1)
    r = dict(x=(0.5 - zeta * u).reshape(sh), y=(4.0 - zeta * v).reshape(sh), cx=(u * cz).reshape(sh), cy=(v * cz).reshape(sh))
    return dict({k: a.astype(np.float32) for k, a in r.items()}, ok=np.ones(sh, bool))
