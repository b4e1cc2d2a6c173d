"""The cases the MTF kernels (tl_mtf_sums, tl_mtf_seed) are held on, shared by tests/test_gpu_mtf.py and tests/test_mtf_cpu.py: the
fourteen seeded fans of tests/focus_cases.py as tests/enclosed_cases.py hands them out (spots 0.02 - 0.07 mm across at image
heights of millimetres, dead rays among them, their shapes and memory layouts; a ray is live iff ok != 0), at the frequencies
5 k cycles / mm, k = 0 .. 15, tangential and sagittal: 32 vectors, two launches.  The curve runs from exactly 1 through ~0.8 at
10 cycles / mm to ~0.05 - 0.15 at 75.  The two many-rows cases take J = 2: 15 cycles / mm tangential and sagittal."""
import numpy as np

import enclosed_cases as EC

SHAPES = EC.SHAPES
CASES = EC.CASES
FREQUENCIES = tuple(5.0 * k for k in range(16))
DIRECTIONS = ("tangential", "sagittal")
rays, place, given_centre = EC.rays, EC.place, EC.given_centre


def frequencies_of(name):
    return (15.0,) if name.startswith("many-rows") else FREQUENCIES


def seeds(name, J):
    """Dense seeds of both signs: g_sums [B,F,W,J,2] (float64)."""
    B, F, W, _ = SHAPES[name]
    return np.random.default_rng(23 + sum(map(ord, name)) + J).standard_normal((B, F, W, J, 2))


def two_rays(a=0.004):
    """Two live rays at y = 9 +- a, x = 0.25 (float32 [1,1,2,1]) and the half distance of the ROUNDED coordinates (float64)."""
    y = np.array([9.0 + a, 9.0 - a], np.float32).reshape(1, 1, 2, 1)
    x = np.full_like(y, 0.25)
    return dict(x=x, y=y, ok=np.ones(y.shape, bool)), (float(y[0, 0, 0, 0]) - float(y[0, 0, 1, 0])) / 2


def comb(N=64, d=2.0 ** -10, y0=8.0):
    """N live rays at spacing d from y = y0 (exact in float32), x = -0.5: the Dirichlet kernel."""
    y = (y0 + d * np.arange(N)).astype(np.float32).reshape(1, 1, N, 1)
    assert np.array_equal(y.astype(np.float64).ravel(), y0 + d * np.arange(N))
    return dict(x=np.full_like(y, -0.5), y=y, ok=np.ones(y.shape, bool))


def dirichlet(nu, N=64, d=2.0 ** -10):
    nu = np.asarray(nu, np.float64)
    den = N * np.sin(np.pi * nu * d)
    return np.where(den == 0, 1.0, np.abs(np.sin(N * np.pi * nu * d) / np.where(den == 0, 1.0, den)))


def bracket(v, live):
    """(lower, upper) of the MTF at the phases v = 2 pi nu (coordinate - its live mean) [.., P, ..] summed over axis 2:
    1 - m2 / 2 <= MTF <= sqrt((1 - m2 / 2 + m4 / 24)^2 + (m3 / 6)^2), m_k = mean |v|^k over the live rays."""
    n = np.maximum(live.sum(axis=2), 1)
    m = {k: np.where(live, np.abs(v) ** k, 0.0).sum(axis=2) / n for k in (2, 3, 4)}
    return 1 - m[2] / 2, np.sqrt((1 - m[2] / 2 + m[4] / 24) ** 2 + (m[3] / 6) ** 2)
