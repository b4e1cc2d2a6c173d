// tl_psf.hip -- the PSF soft histogram of a ray fan and its adjoint, plain (tl_psf_accumulate, tl_psf_accumulate_bwd of
// include/tl_trace.h; metrics.compute_psf(fused=True)) and rotated (tl_psf_rot_accumulate, tl_psf_rot_accumulate_bwd;
// imaging.psf_grid_from_trace(fused=True)).
//
//   hist[g,w,i,j] = sum_r wt_r Gy_i(r) Gx_j(r),   Gx_j = exp(-2 (u - (x_first + j))^2),  u = x / x_pitch[g]
//                                                 Gy_i = exp(-2 (v - (y_first + i))^2),  v = (y - y_centre[g]) / y_pitch[g]
//
// is a [ny, R] x [R, nx] product whose operands never leave registers.
// ONE BODY, TWO LOADS.  The plain call reads fan g for grid g (load_ray).  The rotated call has G grids read K fans: grid g
//   reads the fan src[g], centred on y_centre[src[g]] and turned by (c[g], s[g]) (load_src, then rotate).  Both are load_live
//   and end in to_pitch; everything behind the load -- add_batch and store_tile of the forward, ray_adjoint of the backward
//   -- is written once, which is what lets the rotated kernels give the bits of the plain ones at the four right angles.
// Forward: one wave takes 64 consecutive rays with one coalesced load, then feeds them two at a time (lane half h takes ray
//   s + 32 h of the 64) to v_mfma_f32_32x32x2_f32 with A = wt Gy (row = lane & 31) and B = Gx (column = lane & 31): each lane
//   evaluates the two exponentials of its (row, ray) and (column, ray).  The accumulator is an exact k-ordered fp32 FMA chain;
//   a chain is closed after the 64 rays of one load and added to the wave's fp64 totals (16 v_add_f64 against 32 MFMAs of 64
//   cycles).  The four waves of a block are added in fp64 in a fixed order and the block writes ONE fp32 partial tile;
//   psf_reduce_kernel sums the partials in a fixed order in fp64 and rounds once.  No atomics: the same bits on every run.
// Backward: one ray per lane (rotated: one SOURCE ray, which walks the grids of its fan); g_hist (wave-uniform) is copied into
//   the workspace with rows padded with zeros to a multiple of 4 columns and read through the scalar cache, so the inner
//   product over j is unrolled with no predicate.
#include "tl_common.h"

#include <stdio.h>

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr float kC = -2.885390081777927f;       // -2 log2(e): exp(-2 d^2) = exp2(kC d^2)
constexpr int kRowFold = 32768;                 // rotated: rows per grid-y; row = blockIdx.z kRowFold + blockIdx.y
constexpr int64_t kRotMaxRows = 1 << 20;        // rotated: G W and K W
constexpr int64_t kRotMaxWork = (int64_t)1 << 36;

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float uload(const float *__restrict__ q, const int i)
{
    return ((const __attribute__((address_space(4))) float *)(unsigned long long)q)[i];
}

__device__ __forceinline__ float gauss(const float d) { return __builtin_amdgcn_exp2f(kC * d * d); }

// x, y, weight / ok: K fans [K, W, R] by the strides s_g, s_w.  x_pitch, y_pitch [G]; y_centre [K].  The plain call leaves
// src, c and s null and K = G.
struct PsfIn {
    const float *x, *y, *weight;
    const uint8_t *ok;
    int64_t s_g, s_w, R;
    const float *x_pitch, *y_pitch, *y_centre;
    int W, nx, ny;
    float x_first, y_first;
    const int32_t *src;
    const float *c, *s;
    int G, K;
};

// The load both kinds of call share: the live ray r of a fan, centred, as make(x, y - yc, wt) gives it; past the end of the
// fan or at weight 0 it is `dead`, and nothing of the ray is read.
template <class T, class F>
__device__ __forceinline__ T load_live(const PsfIn &in, const int64_t off, const int64_t r, const float yc, const T dead, F make)
{
    T q = dead;
    if (r < in.R) {
        const float wt = in.weight ? in.weight[off + r] : (in.ok ? (in.ok[off + r] ? 1.f : 0.f) : 1.f);
        if (wt != 0.f) q = make(in.x[off + r], in.y[off + r] - yc, wt);                 // (a NaN weight is kept: it shows)
    }
    return q;
}

// One ray in pitch units.  u, v are carried as a rounded quotient and its remainder (u + ul = x / x_pitch to ~2^-48): a ray
// ten pixels from the centre has ulp(u) = 1e-6 pixels, and that rounding alone, random from ray to ray, was the largest error
// of the sums over rays that cancel (g_y_centre = -sum gy_r: 1e-6 relative against 1e-7 with the remainder).  The distance to
// a pixel centre is then (u - a) + ul: the difference of two nearby numbers is exact, so the error is an ulp of the DISTANCE.
struct Ray { float x, yc, u, v, ul, vl, wt; };

__device__ __forceinline__ Ray to_pitch(const float x, const float yc, const float wt, const float px, const float py)
{
    Ray o;
    o.x = x;
    o.yc = yc;
    o.u = x / px;
    o.v = yc / py;
    o.ul = __builtin_fmaf(-o.u, px, x) / px;
    o.vl = __builtin_fmaf(-o.v, py, yc) / py;
    o.wt = wt;
    return o;
}

// The plain load: straight to pitch units; a dead ray is (0, 0, weight 0) with no division made, so it adds exactly 0
// whatever the pitches are.
__device__ __forceinline__ Ray load_ray(const PsfIn &in, const int64_t off, const int64_t r, const float yc, const float px,
                                        const float py)
{
    return load_live(in, off, r, yc, Ray{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f},
                     [=](float x, float eta, float wt) { return to_pitch(x, eta, wt, px, py); });
}

// The rotated load: the source ray, (0, 0, weight 0) when dead, which rotate() turns for each grid that reads it and takes
// to pitch units, a dead one as the zeros it is.
struct SrcRay { float xi, eta, wt; };

__device__ __forceinline__ SrcRay load_src(const PsfIn &in, const int64_t off, const int64_t r, const float yc)
{
    return load_live(in, off, r, yc, SrcRay{0.f, 0.f, 0.f}, [](float xi, float eta, float wt) { return SrcRay{xi, eta, wt}; });
}

// x' = c xi + s eta, y' = -s xi + c eta (one product and one fma each)
__device__ __forceinline__ Ray rotate(const SrcRay &q, const float c, const float s, const float px, const float py)
{
    return to_pitch(__builtin_fmaf(c, q.xi, s * q.eta), __builtin_fmaf(c, q.eta, -(s * q.xi)), q.wt, px, py);
}

// Forward, 64 loaded rays (one per lane) -> the MFMA chain of this batch, closed and added to the wave's totals.
__device__ __forceinline__ void add_batch(const PsfIn &in, const Ray &q, double tot[16])
{
    const int idx = threadIdx.x & 31, src0 = threadIdx.x & 32;
    const float ax = in.x_first + (float)idx, ay = in.y_first + (float)idx;
    f32x16 acc = {0};
#pragma unroll
    for (int s = 0; s < 32; ++s) {
        const float us = __shfl(q.u, src0 + s, 64), vs = __shfl(q.v, src0 + s, 64), ws = __shfl(q.wt, src0 + s, 64);
        const float uls = __shfl(q.ul, src0 + s, 64), vls = __shfl(q.vl, src0 + s, 64);
        const float a = ws * gauss((vs - ay) + vls), bb = gauss((us - ax) + uls);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bb, acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) tot[r] += (double)acc[r];
}

// Forward, the totals of the four waves -> LDS -> the block's partial tile out[ny, nx], added in fp64 in wave order.
__device__ __forceinline__ void store_tile(const PsfIn &in, const double tot[16], double (&tile)[kWaves][16][64],
                                           float *__restrict__ out)
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int r = 0; r < 16; ++r) tile[tid >> 6][r][tid & 63] = tot[r];
    __syncthreads();
    for (int e = tid; e < 16 * 64; e += kBlock) {
        const int r = e >> 6, l = e & 63;
        const int row = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5), col = l & 31;     // C/D map of the 32x32 MFMA
        if (row < in.ny && col < in.nx) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < kWaves; ++k) s += tile[k][r][l];
            out[row * in.nx + col] = (float)s;
        }
    }
}

// grid (nbx, rows in y, rows / kRowFold in z), kBlock threads: row gw = blockIdx.z kRowFold + blockIdx.y (the plain launch puts
// all its G W <= 65535 rows in y, so its z is 0); wave `wv` of block bx takes the 64-ray batches [(bx kWaves + wv) nb, ... + nb).
// (The error texts name psf_fwd_kernel<true> psf_rot_fwd_kernel.)
template <bool ROT>
__global__ __launch_bounds__(kBlock) void psf_fwd_kernel(const PsfIn in, float *__restrict__ part, const int nb)
{
    __shared__ double tile[kWaves][16][64];
    const int gw = blockIdx.z * kRowFold + blockIdx.y;
    if (gw >= in.G * in.W) return;                                      // block-uniform, before any barrier
    const int g = gw / in.W, w = gw - g * in.W, k = ROT ? in.src[g] : g;
    const int64_t off = (int64_t)k * in.s_g + (int64_t)w * in.s_w;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const float px = in.x_pitch[g], py = in.y_pitch[g], yc = in.y_centre[k];
    const float cg = ROT ? in.c[g] : 1.f, sg = ROT ? in.s[g] : 0.f;
    const int64_t batch0 = ((int64_t)blockIdx.x * kWaves + wv) * nb;
    double tot[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) tot[r] = 0.0;
    for (int b = 0; b < nb; ++b) {
        const int64_t r0 = (batch0 + b) * 64;
        if (r0 >= in.R) break;                                          // wave-uniform
        const int64_t r = r0 + lane;
        add_batch(in, ROT ? rotate(load_src(in, off, r, yc), cg, sg, px, py) : load_ray(in, off, r, yc, px, py), tot);
    }
    store_tile(in, tot, tile, part + ((size_t)gw * gridDim.x + blockIdx.x) * (size_t)(in.ny * in.nx));
}

// hist[gw, bin] = sum over the nbx partials, fp64, fixed order, rounded once.  grid (ceil(nbins / 64), G W), block (64, 4):
// slice z sums the partials k = z, z + 4, ... (four interleaved accumulators), then the slices are added in order.
__global__ __launch_bounds__(256) void psf_reduce_kernel(const float *__restrict__ part, float *__restrict__ hist, const int nbx,
                                                         const int nbins)
{
    __shared__ double sl[4][64];
    const int bin = blockIdx.x * 64 + threadIdx.x, z = threadIdx.y, gw = blockIdx.y;
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    if (bin < nbins) {
        const float *__restrict__ p = part + (size_t)gw * nbx * nbins + bin;
        int k = z;
        for (; k + 12 < nbx; k += 16) {
#pragma unroll
            for (int q = 0; q < 4; ++q) a[q] += (double)p[(size_t)(k + 4 * q) * nbins];
        }
        for (int q = 0; k < nbx; k += 4, ++q) a[q] += (double)p[(size_t)k * nbins];
    }
    sl[z][threadIdx.x] = (a[0] + a[1]) + (a[2] + a[3]);
    __syncthreads();
    if (z == 0 && bin < nbins)
        hist[(size_t)gw * nbins + bin] = (float)((sl[0][threadIdx.x] + sl[1][threadIdx.x]) + (sl[2][threadIdx.x] + sl[3][threadIdx.x]));
}

// g_hist [G W, ny, nx] -> gpad [G W, ny, nxp], columns nx..nxp-1 zero
__global__ void psf_pad_kernel(const float *__restrict__ g_hist, float *__restrict__ gpad, const int rows, const int nx,
                               const int nxp)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * nxp) return;
    const int row = i / nxp, col = i - row * nxp;
    gpad[i] = col < nx ? g_hist[(size_t)row * nx + col] : 0.f;
}

// a + b over the wave in a fixed tree; lane 0 holds the sum
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
    return v;
}

// Backward, one ray against the padded seed gp [ny, NXP] of its (grid, channel):
//   A = sum_ij g_ij Gy_i Gx'_j,  Bq = sum_ij g_ij Gy'_i Gx_j  (derivatives to u and v; the caller scales by wt / pitch)
template <int NXP>
__device__ __forceinline__ void ray_adjoint(const Ray &q, const float *__restrict__ gp, const int ny, const float x_first,
                                            const float y_first, float &A, float &Bq)
{
    float Gx[NXP], Gd[NXP];
#pragma unroll
    for (int j = 0; j < NXP; ++j) {
        const float d = (q.u - (x_first + (float)j)) + q.ul;
        Gx[j] = gauss(d);
        Gd[j] = -4.f * d * Gx[j];
    }
    A = 0.f;
    Bq = 0.f;
    for (int i = 0; i < ny; ++i) {
        const float d = (q.v - (y_first + (float)i)) + q.vl;
        const float Gy = gauss(d), Gyd = -4.f * d * Gy;
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int j = 0; j < NXP; ++j) {
            const float gij = uload(gp, i * NXP + j);
            s1 = __builtin_fmaf(gij, Gd[j], s1);
            s2 = __builtin_fmaf(gij, Gx[j], s2);
        }
        A = __builtin_fmaf(Gy, s1, A);
        Bq = __builtin_fmaf(Gyd, s2, Bq);
    }
}

// grid (nbx, G W), kBlock threads, lane t of block bx takes rays (bx rpl + k) kBlock + t, k < rpl.
// part [G W, nbx, 3] doubles: the block's sums of gx_r x_r, gy_r (y_r - y_centre), gy_r (psf_bwd_reduce_kernel finishes them)
template <int NXP>
__global__ __launch_bounds__(kBlock) void psf_bwd_kernel(const PsfIn in, const float *__restrict__ gpad, float *__restrict__ gx,
                                                         float *__restrict__ gy, double *__restrict__ part, const int rpl)
{
    __shared__ double red[kWaves][3];
    const int gw = blockIdx.y, g = gw / in.W, w = gw - g * in.W;
    const int64_t off = (int64_t)g * in.s_g + (int64_t)w * in.s_w;
    const int tid = threadIdx.x;
    const float px = in.x_pitch[g], py = in.y_pitch[g], yc = in.y_centre[g];
    const float *__restrict__ gp = gpad + (size_t)gw * in.ny * NXP;
    double s_xp = 0.0, s_yp = 0.0, s_yc = 0.0;
    for (int k = 0; k < rpl; ++k) {
        const int64_t r = ((int64_t)blockIdx.x * rpl + k) * kBlock + tid;
        if (r >= in.R) break;
        const Ray q = load_ray(in, off, r, yc, px, py);
        float A, Bq;
        ray_adjoint<NXP>(q, gp, in.ny, in.x_first, in.y_first, A, Bq);
        const bool live = q.wt != 0.f;
        const float gxr = live ? q.wt * A / px : 0.f, gyr = live ? q.wt * Bq / py : 0.f;
        gx[off + r] = gxr;
        gy[off + r] = gyr;
        s_xp += (double)gxr * (double)q.x;
        s_yp += (double)gyr * (double)q.yc;
        s_yc += (double)gyr;
    }
    s_xp = wave_sum(s_xp);
    s_yp = wave_sum(s_yp);
    s_yc = wave_sum(s_yc);
    if ((tid & 63) == 0) {
        red[tid >> 6][0] = s_xp;
        red[tid >> 6][1] = s_yp;
        red[tid >> 6][2] = s_yc;
    }
    __syncthreads();
    if (tid < 3) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < kWaves; ++k) s += red[k][tid];
        part[((size_t)gw * gridDim.x + blockIdx.x) * 3 + tid] = s;
    }
}

// grid (nbx, min(K W, kRowFold), ceil(K W / kRowFold)): one lane per SOURCE ray, lane t of block bx takes rays
// (bx rpl + q) kBlock + t, q < rpl, and walks the grids of its fan in list order: the adjoint of every grid is turned back by
// (c, s) and summed, the first term assigned.  gpad [G W, ny, NXP] as psf_pad_kernel leaves it.
// part [K W, nbx, 3] doubles, slot 2 only: the block's sum of gy (psf_bwd_reduce_kernel finishes g_y_centre).
template <int NXP>
__global__ __launch_bounds__(kBlock) void psf_rot_bwd_kernel(const PsfIn in, const int32_t *__restrict__ field_start,
                                                             const int32_t *__restrict__ field_grids,
                                                             const float *__restrict__ gpad, float *__restrict__ gx,
                                                             float *__restrict__ gy, double *__restrict__ part, const int rpl)
{
    __shared__ double red[kWaves];
    const int kw = blockIdx.z * kRowFold + blockIdx.y;
    if (kw >= in.K * in.W) return;                                      // block-uniform, before any barrier
    const int k = kw / in.W, w = kw - k * in.W;
    const int64_t off = (int64_t)k * in.s_g + (int64_t)w * in.s_w;
    const int tid = threadIdx.x;
    const float yc = in.y_centre[k];
    const int n0 = field_start[k], n1 = field_start[k + 1];
    const int ny = in.ny;
    double s_yc = 0.0;
    for (int it = 0; it < rpl; ++it) {
        const int64_t r = ((int64_t)blockIdx.x * rpl + it) * kBlock + tid;
        if (r >= in.R) break;
        const SrcRay sr = load_src(in, off, r, yc);
        float gxi = 0.f, geta = 0.f;
        for (int n = n0; n < n1; ++n) {                                 // wave-uniform
            const int g = field_grids[n];
            const float cg = in.c[g], sg = in.s[g], px = in.x_pitch[g], py = in.y_pitch[g];
            const Ray q = rotate(sr, cg, sg, px, py);
            float A, Bq;
            ray_adjoint<NXP>(q, gpad + ((size_t)g * in.W + w) * ny * NXP, ny, in.x_first, in.y_first, A, Bq);
            const float gxr = q.wt * A / px, gyr = q.wt * Bq / py;
            const float txi = __builtin_fmaf(cg, gxr, -(sg * gyr)), teta = __builtin_fmaf(cg, gyr, sg * gxr);
            gxi = n == n0 ? txi : gxi + txi;
            geta = n == n0 ? teta : geta + teta;
        }
        const bool live = sr.wt != 0.f;
        gxi = live ? gxi : 0.f;
        geta = live ? geta : 0.f;
        gx[off + r] = gxi;
        gy[off + r] = geta;
        s_yc += (double)geta;
    }
    s_yc = wave_sum(s_yc);
    if ((tid & 63) == 0) red[tid >> 6] = s_yc;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < kWaves; ++q) s += red[q];
        part[((size_t)kw * gridDim.x + blockIdx.x) * 3 + 2] = s;
    }
}

// g_x_pitch[g] = -(sum gx_r x_r) / x_pitch,  g_y_pitch[g] = -(sum gy_r (y_r - y_centre)) / y_pitch,  g_y_centre[g] = -sum gy_r:
// one wave per (g, q); lane l sums the partials l, l + 64, ... of the grid's W nbx in order, then the fixed tree.
__global__ __launch_bounds__(64) void psf_bwd_reduce_kernel(const double *__restrict__ part, const int n_per_grid,
                                                            const float *__restrict__ x_pitch, const float *__restrict__ y_pitch,
                                                            float *g_x_pitch, float *g_y_pitch, float *g_y_centre)
{
    const int g = blockIdx.x / 3, q = blockIdx.x - 3 * g;
    float *const dst = q == 0 ? g_x_pitch : (q == 1 ? g_y_pitch : g_y_centre);
    if (!dst) return;
    const double *__restrict__ p = part + (size_t)g * n_per_grid * 3 + q;
    double s = 0.0;
    for (int k = threadIdx.x; k < n_per_grid; k += 64) s += p[(size_t)k * 3];
    s = wave_sum(s);
    if (threadIdx.x == 0) {
        const double div = q == 0 ? (double)x_pitch[g] : (q == 1 ? (double)y_pitch[g] : 1.0);
        dst[g] = (float)(-s / div);
    }
}

// ---------------------------------------------------------------------------------------------------------------- host

struct PsfPlan {
    int nb, nbx_fwd;        // forward: 64-ray batches per wave, blocks per (g, w)
    int rpl, nbx_bwd;       // backward: rays per lane, blocks per (g, w)
    int nxp;                // g_hist columns padded to a multiple of 4
    size_t fwd_bytes, gpad_bytes, bwd_bytes;
};

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Forward: MFMA-bound, one round of ~1024 blocks (4 waves per SIMD) whatever the size, so the partials stay << 1 B per ray.
// Backward: VALU-bound, ~2048 blocks.
PsfPlan psf_plan(int G, int W, int64_t R, int nx, int ny)
{
    PsfPlan pl;
    const int64_t GW = (int64_t)G * W, batches = cdiv(R, 64);
    int64_t nb = cdiv(batches * GW, (int64_t)kWaves * 1024);
    nb = nb < 1 ? 1 : (nb > 256 ? 256 : nb);
    pl.nb = (int)nb;
    pl.nbx_fwd = (int)cdiv(batches, kWaves * nb);
    int64_t rpl = cdiv(R * GW, (int64_t)kBlock * 2048);
    rpl = rpl < 1 ? 1 : (rpl > 64 ? 64 : rpl);
    pl.rpl = (int)rpl;
    pl.nbx_bwd = (int)cdiv(R, kBlock * rpl);
    pl.nxp = (nx + 3) & ~3;
    pl.fwd_bytes = (size_t)GW * pl.nbx_fwd * ny * nx * sizeof(float);
    pl.gpad_bytes = (((size_t)GW * ny * pl.nxp * sizeof(float)) + 255u) & ~(size_t)255u;
    pl.bwd_bytes = pl.gpad_bytes + (size_t)GW * pl.nbx_bwd * 3 * sizeof(double);
    return pl;
}

struct RotPlan {
    PsfPlan f, b;           // forward over the G W grid rows, backward over the K W source rows (b.gpad_bytes is f's)
    size_t fwd_bytes, bwd_bytes;
};

RotPlan psf_rot_plan(int G, int K, int W, int64_t R, int nx, int ny)
{
    RotPlan pl;
    pl.f = psf_plan(G, W, R, nx, ny);
    pl.b = psf_plan(K, W, R, nx, ny);
    pl.fwd_bytes = pl.f.fwd_bytes;
    pl.bwd_bytes = pl.f.gpad_bytes + (size_t)K * W * pl.b.nbx_bwd * 3 * sizeof(double);
    return pl;
}

// f(std::integral_constant<int, NXP>) for the instantiation that takes nxp padded columns (a multiple of 4 in 4..32)
template <class F>
void with_nxp(int nxp, F f)
{
    switch (nxp) {
    case 4: f(std::integral_constant<int, 4>()); break;
    case 8: f(std::integral_constant<int, 8>()); break;
    case 12: f(std::integral_constant<int, 12>()); break;
    case 16: f(std::integral_constant<int, 16>()); break;
    case 20: f(std::integral_constant<int, 20>()); break;
    case 24: f(std::integral_constant<int, 24>()); break;
    case 28: f(std::integral_constant<int, 28>()); break;
    default: f(std::integral_constant<int, 32>()); break;
    }
}

// Everything that can be refused without a HIP call.  rot: the rotated pair, with its tables and its wider limits;
// missing: what is wrong with the entry point's own pointers, or null.
int check_args(const char *fn, const PsfIn &in, bool rot, const char *missing)
{
    char msg[256];
    const int64_t GW = (int64_t)in.G * in.W, KW = (int64_t)in.K * in.W, max_rows = rot ? kRotMaxRows : 65535;
    const char *what = missing;
    if (!in.x || !in.y || !in.x_pitch || !in.y_pitch || !in.y_centre || (rot && (!in.src || !in.c || !in.s)))
        what = "a required pointer is NULL";
    else if (in.nx < 1 || in.nx > 32 || in.ny < 1 || in.ny > 32)
        what = rot ? "nx and ny must be in 1..32" : "nxh and ny must be in 1..32";
    else if (in.G < 1 || in.K < 1 || in.W < 1 || GW > max_rows || KW > max_rows)
        what = rot ? "G, K and W must be >= 1 and G*W, K*W <= 1048576" : "G and W must be >= 1 and G*W <= 65535";
    else if (in.R < 1) what = "R must be >= 1";
    else if (rot && (in.R > kRotMaxWork / GW || in.R > kRotMaxWork / KW)) what = "G*W*R and K*W*R must be <= 2^36";
    else if (in.weight && in.ok) what = "give weight or ok, not both";
    if (!what) return TL_OK;
    snprintf(msg, sizeof(msg), "%s: %s", fn, what);
    return tl_host::fail(TL_EINVAL, msg);
}

// The workspace of the call, then its device.
int enter(const char *fn, int device, const void *workspace, size_t have, size_t need)
{
    char msg[96];
    if (workspace && have >= need) return tl_host::use_device(device);
    snprintf(msg, sizeof(msg), "workspace too small for %s", fn);
    return tl_host::fail(TL_EWORKSPACE, msg);
}

// The rows of a launch: kRowFold per grid-y and the rest in z for the rotated pair, all in y for the plain one.
inline int row_fold(bool rot) { return rot ? kRowFold : 65535; }
inline dim3 fold_rows(int nbx, int rows, int fold) { return dim3(nbx, rows < fold ? rows : fold, (rows + fold - 1) / fold); }

// Both forward entry points; the plain one is the rotated one without tables and with K = G.
int accumulate(const char *fn, bool rot, int device, const PsfIn &in, float *hist, void *workspace, size_t workspace_bytes,
               hipStream_t st)
{
    int rc = check_args(fn, in, rot, hist ? nullptr : "hist is NULL");
    if (rc) return rc;
    const PsfPlan pl = psf_plan(in.G, in.W, in.R, in.nx, in.ny);             // (RotPlan.f: the forward runs over the G W grid rows)
    if ((rc = enter(fn, device, workspace, workspace_bytes, pl.fwd_bytes))) return rc;
    const int GW = in.G * in.W, nbins = in.ny * in.nx, fold = row_fold(rot);
    const dim3 grid = fold_rows(pl.nbx_fwd, GW, fold);
    if (rot) hipLaunchKernelGGL(psf_fwd_kernel<true>, grid, dim3(kBlock), 0, st, in, (float *)workspace, pl.nb);
    else hipLaunchKernelGGL(psf_fwd_kernel<false>, grid, dim3(kBlock), 0, st, in, (float *)workspace, pl.nb);
    if ((rc = tl_host::launched(rot ? "psf_rot_fwd_kernel launch" : "psf_fwd_kernel launch"))) return rc;
    for (int row0 = 0; row0 < GW; row0 += fold) {            // psf_reduce_kernel takes its rows in grid-y alone
        const int rows = GW - row0 < fold ? GW - row0 : fold;
        hipLaunchKernelGGL(psf_reduce_kernel, dim3((nbins + 63) / 64, rows), dim3(64, 4), 0, st,
                           (const float *)workspace + (size_t)row0 * pl.nbx_fwd * nbins, hist + (size_t)row0 * nbins, pl.nbx_fwd,
                           nbins);
        if ((rc = tl_host::launched("psf_reduce_kernel launch"))) return rc;
    }
    return TL_OK;
}

// Both backward entry points.  rot: field_start and field_grids are the fans' grid lists and g_x_pitch, g_y_pitch are null
// (psf_bwd_reduce_kernel returns at once for a quantity without a destination, before it reads a pitch).
int accumulate_bwd(const char *fn, bool rot, int device, const PsfIn &in, const int32_t *field_start, const int32_t *field_grids,
                   const float *g_hist, float *gx, float *gy, float *g_x_pitch, float *g_y_pitch, float *g_y_centre,
                   void *workspace, size_t workspace_bytes, hipStream_t st)
{
    const bool have = g_hist && gx && gy && (!rot || (field_start && field_grids));
    const char *missing = rot ? "field_start, field_grids, g_hist, gx or gy is NULL" : "g_hist, gx or gy is NULL";
    int rc = check_args(fn, in, rot, have ? nullptr : missing);
    if (rc) return rc;
    const RotPlan pl = psf_rot_plan(in.G, in.K, in.W, in.R, in.nx, in.ny);
    if ((rc = enter(fn, device, workspace, workspace_bytes, pl.bwd_bytes))) return rc;
    const int rows = in.G * in.W * in.ny, nxp = pl.f.nxp;
    float *gpad = (float *)workspace;
    double *part = (double *)((char *)workspace + pl.f.gpad_bytes);
    const dim3 grid = fold_rows(pl.b.nbx_bwd, in.K * in.W, row_fold(rot));
    hipLaunchKernelGGL(psf_pad_kernel, dim3((rows * nxp + 255) / 256), dim3(256), 0, st, g_hist, gpad, rows, in.nx, nxp);
    if ((rc = tl_host::launched("psf_pad_kernel launch"))) return rc;
    with_nxp(nxp, [&](auto n) {
        constexpr int NXP = decltype(n)::value;
        if (rot) hipLaunchKernelGGL(psf_rot_bwd_kernel<NXP>, grid, dim3(kBlock), 0, st, in, field_start, field_grids, gpad, gx, gy, part,
                                    pl.b.rpl);
        else hipLaunchKernelGGL(psf_bwd_kernel<NXP>, grid, dim3(kBlock), 0, st, in, gpad, gx, gy, part, pl.b.rpl);
    });
    if ((rc = tl_host::launched(rot ? "psf_rot_bwd_kernel launch" : "psf_bwd_kernel launch"))) return rc;
    if (!g_x_pitch && !g_y_pitch && !g_y_centre) return TL_OK;
    hipLaunchKernelGGL(psf_bwd_reduce_kernel, dim3(in.K * 3), dim3(64), 0, st, (const double *)part, in.W * pl.b.nbx_bwd,
                       rot ? nullptr : in.x_pitch, rot ? nullptr : in.y_pitch, g_x_pitch, g_y_pitch, g_y_centre);
    return tl_host::launched("psf_bwd_reduce_kernel launch");
}

}  // namespace

extern "C" {

size_t tl_psf_workspace_bytes(int32_t G, int32_t W, int64_t R, int32_t nxh, int32_t ny)
{
    if (G < 1 || W < 1 || R < 1 || nxh < 1 || nxh > 32 || ny < 1 || ny > 32) return 0;
    const PsfPlan pl = psf_plan(G, W, R, nxh, ny);
    return (pl.fwd_bytes > pl.bwd_bytes ? pl.fwd_bytes : pl.bwd_bytes) + 256;
}

int tl_psf_accumulate(int32_t device, int32_t G, int32_t W, int64_t R, const float *x, const float *y, const float *weight,
                      const uint8_t *ok, int64_t s_g, int64_t s_w, const float *x_pitch, const float *y_pitch,
                      const float *y_centre, int32_t nxh, int32_t ny, float x_first, float y_first, float *hist,
                      void *workspace, size_t workspace_bytes, void *stream)
{
    const PsfIn in = {x, y, weight, ok, s_g, s_w, R, x_pitch, y_pitch, y_centre, W, nxh, ny, x_first, y_first,
                      nullptr, nullptr, nullptr, G, G};
    return accumulate("tl_psf_accumulate", false, device, in, hist, workspace, workspace_bytes, (hipStream_t)stream);
}

int tl_psf_accumulate_bwd(int32_t device, int32_t G, int32_t W, int64_t R, const float *x, const float *y, const float *weight,
                          const uint8_t *ok, int64_t s_g, int64_t s_w, const float *x_pitch, const float *y_pitch,
                          const float *y_centre, int32_t nxh, int32_t ny, float x_first, float y_first, const float *g_hist,
                          float *gx, float *gy, float *g_x_pitch, float *g_y_pitch, float *g_y_centre, void *workspace,
                          size_t workspace_bytes, void *stream)
{
    const PsfIn in = {x, y, weight, ok, s_g, s_w, R, x_pitch, y_pitch, y_centre, W, nxh, ny, x_first, y_first,
                      nullptr, nullptr, nullptr, G, G};
    return accumulate_bwd("tl_psf_accumulate_bwd", false, device, in, nullptr, nullptr, g_hist, gx, gy, g_x_pitch, g_y_pitch,
                          g_y_centre, workspace, workspace_bytes, (hipStream_t)stream);
}

size_t tl_psf_rot_workspace_bytes(int32_t G, int32_t K, int32_t W, int64_t R, int32_t nx, int32_t ny)
{
    if (G < 1 || K < 1 || W < 1 || R < 1 || nx < 1 || nx > 32 || ny < 1 || ny > 32 || (int64_t)G * W > kRotMaxRows
        || (int64_t)K * W > kRotMaxRows || R > kRotMaxWork / ((int64_t)G * W) || R > kRotMaxWork / ((int64_t)K * W))
        return 0;
    const RotPlan pl = psf_rot_plan(G, K, W, R, nx, ny);
    return (pl.fwd_bytes > pl.bwd_bytes ? pl.fwd_bytes : pl.bwd_bytes) + 256;
}

int tl_psf_rot_accumulate(int32_t device, int32_t G, int32_t K, int32_t W, int64_t R, const float *x, const float *y,
                          const float *weight, const uint8_t *ok, int64_t s_g, int64_t s_w, const int32_t *src, const float *c,
                          const float *s, const float *x_pitch, const float *y_pitch, const float *y_centre, int32_t nx,
                          int32_t ny, float x_first, float y_first, float *hist, void *workspace, size_t workspace_bytes,
                          void *stream)
{
    const PsfIn in = {x, y, weight, ok, s_g, s_w, R, x_pitch, y_pitch, y_centre, W, nx, ny, x_first, y_first, src, c, s, G, K};
    return accumulate("tl_psf_rot_accumulate", true, device, in, hist, workspace, workspace_bytes, (hipStream_t)stream);
}

int tl_psf_rot_accumulate_bwd(int32_t device, int32_t G, int32_t K, int32_t W, int64_t R, const float *x, const float *y,
                              const float *weight, const uint8_t *ok, int64_t s_g, int64_t s_w, const int32_t *src,
                              const float *c, const float *s, const float *x_pitch, const float *y_pitch,
                              const float *y_centre, int32_t nx, int32_t ny, float x_first, float y_first,
                              const int32_t *field_start, const int32_t *field_grids, const float *g_hist, float *gx, float *gy,
                              float *g_y_centre, void *workspace, size_t workspace_bytes, void *stream)
{
    const PsfIn in = {x, y, weight, ok, s_g, s_w, R, x_pitch, y_pitch, y_centre, W, nx, ny, x_first, y_first, src, c, s, G, K};
    return accumulate_bwd("tl_psf_rot_accumulate_bwd", true, device, in, field_start, field_grids, g_hist, gx, gy, nullptr, nullptr,
                          g_y_centre, workspace, workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
