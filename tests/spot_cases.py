"""The shapes, layouts, inputs and reference of the spot-metric kernel tests, shared by tests/test_gpu_spot_kernels.py (the
kernels behind tl_spot_moments, tl_spot_seed, tl_spot_rms, tl_unsup_loss, tl_unsup_loss_bwd) and tests/test_spot_cases_cpu.py
(the premises, checked without a GPU), plus a Python statement of how the host plans the launch of tl_spot_moments
(csrc/tl_api.hip: make_plan, sum_rows), written from the definition.

Inputs are dyadic: y = k / 1024, x = k' / 1024 with integers |k|, |k'| <= 8192, exact in fp32.  Every moment
(sum y, sum ok y, sum ok y^2, sum ok, and the same in x) is then an integer multiple of 2^-20 below 2^46 for up to 2^20 rays
per field: exact in fp64 IN ANY SUMMATION ORDER.  The reference is a torch fp64 sum on the CPU and the tolerance is zero.
Gradient seeds are multiples of 2^-8 below 4, so g0 + ok (g1 + 2 y g2) is a multiple of 2^-18 below 72: 25 bits, exact in
fp64 with or without FMA contraction, and rounded to fp32 once.

Why each shape is there (kBlock = 256 pupil points per chunk, make_plan(P, F W, cap 4096, rmax 64, few 2048, rwant 8)):
    (3, 3, P), P = 1, 63, 255, 256, 257, 1000   R = 1: one chunk per block, the last one partial (or the only one)
    (8, 8, 49169)     193 chunks, R = 6, 33 blocks per row: the last block holds ONE chunk of 17 rays and five past the pupil
    (16, 16, 33001)   129 chunks: 17 blocks per row would be 4352 > cap, so 16 blocks of R = 9; block 14 holds three chunks
                      (the last of 233 rays), block 15 none at all
    (1, 1, 524291)    2049 chunks = 2049 partial rows of one field: every thread of sum_rows takes one unrolled trip of eight,
                      thread 0 alone one trip of the tail loop
    (1, 3, 179203)    701 chunks, count = 3 x 701 = 2103 partial rows over three wavelengths: one unrolled trip, then the tail
                      loop for threads 0..54 only
The rmax = 64 branch (more chunks than 64 per block under the cap: 4096 x 64 x 256 > 67 M elements) is left out: a test of
that size does not belong in a suite that runs for every change.
"""
import functools

import numpy as np
import torch

NMOM = 10
SCALE = 1024                # y = k / SCALE
KMAX = 8192                 # |k| <= KMAX
MAX_RAYS = 1 << 20          # rays per field for which every moment is still exact

SHAPES = [(3, 3, 1), (3, 3, 63), (3, 3, 255), (3, 3, 256), (3, 3, 257), (3, 3, 1000),
          (8, 8, 49169), (16, 16, 33001), (1, 1, 524291), (1, 3, 179203)]

# how x, y, ok [1,F,P,W] reach SpotMomentsFunction
LAYOUTS = ["contiguous",        # [1,F,P,W] dense: s_p = W, s_w = 1
           "fwp",               # [1,F,W,P] storage permuted to [1,F,P,W]: s_p = 1, s_w = P (what the trace and tl_aim_fan produce)
           "slice",             # fields 1..F of F + 2 and every second pupil point of 2 P: dense in no dimension but w
           "ok_contiguous",     # y, x as "fwp", ok dense: ok goes through empty_strided(...).copy_()
           "x_fwp",             # y, ok dense, x as "fwp": x goes through empty_strided(...).copy_()
           "y_expanded",        # y [1,F,P,1] expanded over W (stride 0): made dense by the op
           "x_none"]            # compute_rms2d's call: no x


def make_plan(P, FW, cap, rmax, few, rwant, block=256):
    """(nbx, R) of csrc/tl_api.hip: make_plan -- blocks per (f, w) row and chunks of `block` pupil points per block."""
    chunks = (P + block - 1) // block
    r = min(max(chunks * FW // few, 1), rwant)
    nbx = (chunks + r - 1) // r
    if nbx * FW > cap:
        nbx = (cap + FW - 1) // FW
    nbx = min(nbx, chunks)
    if nbx * rmax < chunks:
        nbx = (chunks + rmax - 1) // rmax
    nbx = max(nbx, 1)
    return nbx, (chunks + nbx - 1) // nbx


def uncapped_blocks(P, FW, few, rwant, block=256):
    """Blocks per row that make_plan wants before the cap: ceil(chunks / r)."""
    chunks = (P + block - 1) // block
    r = min(max(chunks * FW // few, 1), rwant)
    return (chunks + r - 1) // r


def block_chunks(P, nbx, R, block=256):
    """Rays in each of the R chunks of each of the nbx blocks of one row (0 = the chunk lies past the pupil): block bx takes
    the chunks bx R ... bx R + R - 1 (spot_moments_kernel)."""
    return [[max(0, min(block, P - (bx * R + r) * block)) for r in range(R)] for bx in range(nbx)]


def sum_rows_trips(count, unroll, block=256):
    """(trips of the unrolled loop, trips of the tail loop) of every thread of sum_rows over one run of `count` partial rows:
    a thread starts at its index, takes `unroll` rows `block` apart per unrolled trip while the last of them is in range,
    then single rows."""
    big, tail = [], []
    for t in range(block):
        i, nb, nt = t, 0, 0
        while i + (unroll - 1) * block < count:
            i, nb = i + unroll * block, nb + 1
        while i < count:
            i, nt = i + block, nt + 1
        big.append(nb)
        tail.append(nt)
    return big, tail


@functools.lru_cache(maxsize=2)
def ints(F, W, P, expanded=False, dead_at_zero=True):
    """The integers behind one case: (ky, kx, ok), each [F,P,W] (int64, int64, bool).  5-30 % of the rays of a field are dead
    (ray 0 of field 0 always); a dead ray sits at the origin like the trace's, unless dead_at_zero=False (sum y != sum ok y
    then); every field has its own offset in y and another in x, so that no two fields and no two columns share a moment.
    `expanded`: y does not depend on w."""
    assert P * W <= MAX_RAYS
    rng = np.random.default_rng(1000003 * F + 1009 * W + P)
    f = np.arange(F)
    off_y = (257 * (f % 13) - 1500)[:, None, None]
    off_x = (1200 - 311 * (f % 11))[:, None, None]
    ky = rng.integers(-4096, 4097, size=(F, P, 1 if expanded else W)) + off_y
    ky = np.broadcast_to(ky, (F, P, W)).copy()
    kx = rng.integers(-4096, 4097, size=(F, P, W)) + off_x
    frac = rng.uniform(0.05, 0.30, size=F)[:, None, None]
    ok = rng.random(size=(F, P, W)) >= frac
    ok[0, 0, 0] = False
    if dead_at_zero and not expanded:            # (an expanded y cannot be zero at one w only)
        ky[~ok] = 0
        kx[~ok] = 0
    assert np.abs(ky).max() <= KMAX and np.abs(kx).max() <= KMAX
    return torch.from_numpy(ky), torch.from_numpy(kx), torch.from_numpy(ok)


def rays(F, W, P, expanded=False, dead_at_zero=True):
    """(x, y, ok) [1,F,P,W] float32, float32, bool on the CPU."""
    ky, kx, ok = ints(F, W, P, expanded, dead_at_zero)
    return (kx.to(torch.float32) / SCALE)[None], (ky.to(torch.float32) / SCALE)[None], ok[None]


def reference_moments(x, y, ok):
    """[F, NMOM] fp64: the sums of tl_spot_moments on the CPU (x may be None: its columns are 0)."""
    yd, okd = y[0].double(), ok[0].double()
    m = torch.zeros(y.shape[1], NMOM, dtype=torch.float64)
    m[:, 0], m[:, 1], m[:, 2], m[:, 3] = yd.sum((1, 2)), (okd * yd).sum((1, 2)), (okd * yd * yd).sum((1, 2)), okd.sum((1, 2))
    if x is not None:
        xd = x[0].double()
        m[:, 4], m[:, 5], m[:, 6] = xd.sum((1, 2)), (okd * xd).sum((1, 2)), (okd * xd * xd).sum((1, 2))
    return m


def integer_moments(ky, kx, ok):
    """The same sums in int64: columns 0, 1, 4, 5 in units of 1 / SCALE, columns 2, 6 in units of 1 / SCALE^2, column 3 a count."""
    o = ok.to(torch.int64)
    m = torch.zeros(ky.shape[0], NMOM, dtype=torch.int64)
    m[:, 0], m[:, 1], m[:, 2], m[:, 3] = ky.sum((1, 2)), (o * ky).sum((1, 2)), (o * ky * ky).sum((1, 2)), o.sum((1, 2))
    m[:, 4], m[:, 5], m[:, 6] = kx.sum((1, 2)), (o * kx).sum((1, 2)), (o * kx * kx).sum((1, 2))
    return m


UNITS = torch.tensor([1 / SCALE, 1 / SCALE, 1 / SCALE ** 2, 1.0, 1 / SCALE, 1 / SCALE, 1 / SCALE ** 2, 0.0, 0.0, 0.0],
                     dtype=torch.float64)


def seeds(F, seed=7):
    """g_moments [F, NMOM] fp64: multiples of 2^-8, |g| < 4, every column filled (7-9 must be ignored)."""
    rng = np.random.default_rng(seed + F)
    return torch.from_numpy(rng.integers(-1023, 1024, size=(F, NMOM)).astype(np.float64) / 256)


def reference_seeds(x, y, ok, g):
    """(gx, gy) [1,F,P,W] float32: d(sum g . moments) / d(x, y) evaluated in fp64 and rounded once (tl_spot_seed)."""
    okd = ok.double()
    q = g.reshape(1, -1, 1, 1, NMOM)
    gy = (q[..., 0] + okd * (q[..., 1] + 2.0 * y.double() * q[..., 2])).float()
    gx = None if x is None else (q[..., 4] + okd * (q[..., 5] + 2.0 * x.double() * q[..., 6])).float()
    return gx, gy


def lay_out(t, layout, which):
    """The [1,F,P,W] tensor `t` (which = 'x' | 'y' | 'ok') as `layout` presents it: same values, other strides."""
    def fwp(a):
        return a.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
    if layout in ("contiguous", "x_none"):
        return t.contiguous()
    if layout == "fwp":
        return fwp(t)
    if layout == "slice":
        _, F, P, W = t.shape
        big = torch.full((1, F + 2, 2 * P, W), 3, dtype=t.dtype, device=t.device)          # (what lies between the rays must not be read)
        big[:, 1:-1, ::2] = t
        return big[:, 1:-1, ::2]
    if layout == "ok_contiguous":
        return t.contiguous() if which == "ok" else fwp(t)
    if layout == "x_fwp":
        return fwp(t) if which == "x" else t.contiguous()
    if layout == "y_expanded":
        return t[..., :1].contiguous().expand(t.shape) if which == "y" else t.contiguous()
    raise ValueError(layout)


# ------------------------------------------------------------------------------------------ coincident rays (degenerate fields)
COINCIDENT_N = (3, 5, 7, 48, 777)
COINCIDENT_LENSES = 2048


def coincident_values(seed=20261019):
    """COINCIDENT_LENSES fp32 values (as float64) between 0.1 and 30 mm, either sign."""
    rng = np.random.default_rng(seed)
    v = rng.uniform(0.1, 30.0, size=COINCIDENT_LENSES) * rng.choice([-1.0, 1.0], size=COINCIDENT_LENSES)
    return v.astype(np.float32).astype(np.float64)


RUN = 48                    # rays in one running sum


def run_sum(values):
    """The fp64 sum of `values`: running sums over runs of RUN, the runs added pairwise.  No kernel's order -- chosen so that
    the sums round (more than 32 copies of a 48-bit square do) yet stay within a few ulp; the GPU test
    test_coincident_rays_end_to_end covers the kernels' own order."""
    parts = [np.cumsum(values[i:i + RUN])[-1] for i in range(0, len(values), RUN)]
    while len(parts) > 1:
        parts = [parts[i] + parts[i + 1] if i + 1 < len(parts) else parts[i] for i in range(0, len(parts), 2)]
    return parts[0]


def coincident_moments(n_live, n_all, v):
    """[len(v), NMOM] fp64 numpy: the moments of fields of n_all rays at the fp32 value v[b], n_live[b] of them alive -- all
    rays of a field coincide, so its variance is exactly 0.  The sums of v and v v (the product of two fp32 values is exact in
    fp64) are formed by run_sum."""
    n_live = np.broadcast_to(np.asarray(n_live), v.shape)
    m = np.zeros((len(v), NMOM))
    for b, (nl, val) in enumerate(zip(n_live, v)):
        m[b, 0] = run_sum(np.full(n_all, val))
        m[b, 1] = run_sum(np.full(nl, val))
        m[b, 2] = run_sum(np.full(nl, val * val))
        m[b, 3] = nl
    return m


@functools.lru_cache(maxsize=1)
def coincident_sets():
    """[(name, moments [2048, NMOM], n_per_field)]: one launch per n with n live rays per lens (n_per_field = n), and one
    launch that mixes every n (lens b has COINCIDENT_N[b % 5] live rays of n_per_field = 777; its dead rays sit at the same
    point, so the centroid is that point and the variance is exactly 0 as well)."""
    v = coincident_values()
    out = [(f"n{n}", coincident_moments(n, n, v), n) for n in COINCIDENT_N]
    mixed = np.array([COINCIDENT_N[b % len(COINCIDENT_N)] for b in range(len(v))])
    out.append(("mixed", coincident_moments(mixed, max(COINCIDENT_N), v), max(COINCIDENT_N)))
    return out


def closed_form_variance(m, n):
    """var = (M2 - 2 m M1 + m^2 M3) / n, m = M0 / n, in plain fp64 (numpy): what every closed form of the project evaluates."""
    mean = m[:, 0] / n
    return (m[:, 2] - 2.0 * mean * m[:, 1] + mean * mean * m[:, 3]) / n
