// tl_psf.hip -- the PSF soft histogram of a ray fan and its adjoint (tl_psf_accumulate, tl_psf_accumulate_bwd of
// include/tl_trace.h; metrics.compute_psf(fused=True) stands on them).
//
//   hist[g,w,i,j] = sum_r wt_r Gy_i(r) Gx_j(r),   Gx_j = exp(-2 (u - (x_first + j))^2),  u = x / x_pitch[g]
//                                                 Gy_i = exp(-2 (v - (y_first + i))^2),  v = (y - y_centre[g]) / y_pitch[g]
//
// is a [ny, R] x [R, nxh] product whose operands never leave registers.
// Forward: one wave takes 64 consecutive rays with one coalesced load, then feeds them two at a time (lane half h takes ray
//   s + 32 h of the 64) to v_mfma_f32_32x32x2_f32 with A = wt Gy (row = lane & 31) and B = Gx (column = lane & 31): each lane
//   evaluates the two exponentials of its (row, ray) and (column, ray).  The accumulator is an exact k-ordered fp32 FMA chain;
//   a chain is closed after the 64 rays of one load and added to the wave's fp64 totals (16 v_add_f64 against 32 MFMAs of 64
//   cycles).  The four waves of a block are added in fp64 in a fixed order and the block writes ONE fp32 partial tile;
//   psf_reduce_kernel sums the partials in a fixed order in fp64 and rounds once.  No atomics: the same bits on every run.
// Backward: one ray per lane; g_hist (wave-uniform) is copied into the workspace with rows padded with zeros to a multiple
//   of 4 columns and read through the scalar cache, so the inner product over j is unrolled with no predicate.
// The rotated grid (tl_psf_rot_accumulate, tl_psf_rot_accumulate_bwd; imaging.psf_grid_from_trace(fused=True)) is the same
//   pair with the fan lookup src[g] and the rotation (c[g], s[g]) in the load, further down.
#include "tl_common.h"

#include <stdio.h>

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr float kC = -2.885390081777927f;       // -2 log2(e): exp(-2 d^2) = exp2(kC d^2)

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float uload(const float *__restrict__ q, const int i)
{
    return ((const __attribute__((address_space(4))) float *)(unsigned long long)q)[i];
}

__device__ __forceinline__ float gauss(const float d) { return __builtin_amdgcn_exp2f(kC * d * d); }

struct PsfIn {
    const float *x, *y, *weight;
    const uint8_t *ok;
    int64_t s_g, s_w, R;
    const float *x_pitch, *y_pitch, *y_centre;
    int W, nxh, ny;
    float x_first, y_first;
};

// One ray in pitch units; a ray past the end of the fan or with weight 0 is (0, 0, weight 0): it adds exactly 0.
// u, v are carried as a rounded quotient and its remainder (u + ul = x / x_pitch to ~2^-48): a ray ten pixels from the centre
// has ulp(u) = 1e-6 pixels, and that rounding alone, random from ray to ray, was the largest error of the sums over rays that
// cancel (g_y_centre = -sum gy_r: 1e-6 relative against 1e-7 with the remainder).  The distance to a pixel centre is then
// (u - a) + ul: the difference of two nearby numbers is exact, so the error is an ulp of the DISTANCE.
struct Ray { float x, yc, u, v, ul, vl, wt; };

__device__ __forceinline__ Ray load_ray(const PsfIn &in, const int64_t off, const int64_t r, const float px, const float py,
                                        const float yc)
{
    Ray q = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (r < in.R) {
        const float wt = in.weight ? in.weight[off + r] : (in.ok ? (in.ok[off + r] ? 1.f : 0.f) : 1.f);
        if (wt != 0.f) {                 // (a NaN weight is kept: it shows)
            q.x = in.x[off + r];
            q.yc = in.y[off + r] - yc;
            q.u = q.x / px;
            q.v = q.yc / py;
            q.ul = __builtin_fmaf(-q.u, px, q.x) / px;
            q.vl = __builtin_fmaf(-q.v, py, q.yc) / py;
            q.wt = wt;
        }
    }
    return q;
}

// grid (nbx, G W), kBlock threads; wave `wv` of block bx takes the 64-ray batches [(bx kWaves + wv) nb, ... + nb)
__global__ __launch_bounds__(kBlock) void psf_fwd_kernel(const PsfIn in, float *__restrict__ part, const int nb)
{
    __shared__ double tile[kWaves][16][64];
    const int gw = blockIdx.y, g = gw / in.W, w = gw - g * in.W;
    const int64_t off = (int64_t)g * in.s_g + (int64_t)w * in.s_w;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int idx = lane & 31, src0 = lane & 32;
    const float px = in.x_pitch[g], py = in.y_pitch[g], yc = in.y_centre[g];
    const float ax = in.x_first + (float)idx, ay = in.y_first + (float)idx;
    const int64_t batch0 = ((int64_t)blockIdx.x * kWaves + wv) * nb;
    double tot[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) tot[r] = 0.0;
    for (int b = 0; b < nb; ++b) {
        const int64_t r0 = (batch0 + b) * 64;
        if (r0 >= in.R) break;                                      // wave-uniform
        const Ray q = load_ray(in, off, r0 + lane, px, py, yc);
        f32x16 acc = {0};
#pragma unroll
        for (int s = 0; s < 32; ++s) {
            const float us = __shfl(q.u, src0 + s, 64), vs = __shfl(q.v, src0 + s, 64), ws = __shfl(q.wt, src0 + s, 64);
            const float uls = __shfl(q.ul, src0 + s, 64), vls = __shfl(q.vl, src0 + s, 64);
            const float a = ws * gauss((vs - ay) + vls), bb = gauss((us - ax) + uls);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bb, acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) tot[r] += (double)acc[r];       // the chain of this batch's 64 rays is closed
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) tile[wv][r][lane] = tot[r];
    __syncthreads();
    float *__restrict__ out = part + ((size_t)gw * gridDim.x + blockIdx.x) * (size_t)(in.ny * in.nxh);
    for (int e = tid; e < 16 * 64; e += kBlock) {
        const int r = e >> 6, l = e & 63;
        const int row = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5), col = l & 31;     // C/D map of the 32x32 MFMA
        if (row < in.ny && col < in.nxh) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < kWaves; ++k) s += tile[k][r][l];
            out[row * in.nxh + col] = (float)s;
        }
    }
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

// g_hist [G W, ny, nxh] -> gpad [G W, ny, nxp], columns nxh..nxp-1 zero
__global__ void psf_pad_kernel(const float *__restrict__ g_hist, float *__restrict__ gpad, const int rows, const int nxh,
                               const int nxp)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * nxp) return;
    const int row = i / nxp, col = i - row * nxp;
    gpad[i] = col < nxh ? g_hist[(size_t)row * nxh + col] : 0.f;
}

// a + b over the wave in a fixed tree; lane 0 holds the sum
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
    return v;
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
    const int ny = in.ny;
    double s_xp = 0.0, s_yp = 0.0, s_yc = 0.0;
    for (int k = 0; k < rpl; ++k) {
        const int64_t r = ((int64_t)blockIdx.x * rpl + k) * kBlock + tid;
        if (r >= in.R) break;
        const Ray q = load_ray(in, off, r, px, py, yc);
        float Gx[NXP], Gd[NXP];
#pragma unroll
        for (int j = 0; j < NXP; ++j) {
            const float d = (q.u - (in.x_first + (float)j)) + q.ul;
            Gx[j] = gauss(d);
            Gd[j] = -4.f * d * Gx[j];
        }
        float A = 0.f, Bq = 0.f;
        for (int i = 0; i < ny; ++i) {
            const float d = (q.v - (in.y_first + (float)i)) + q.vl;
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

struct PsfPlan {
    int nb, nbx_fwd;        // forward: 64-ray batches per wave, blocks per (g, w)
    int rpl, nbx_bwd;       // backward: rays per lane, blocks per (g, w)
    int nxp;                // g_hist columns padded to a multiple of 4
    size_t fwd_bytes, gpad_bytes, bwd_bytes;
};

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Forward: MFMA-bound, one round of ~1024 blocks (4 waves per SIMD) whatever the size, so the partials stay << 1 B per ray.
// Backward: VALU-bound, ~2048 blocks.
PsfPlan psf_plan(int G, int W, int64_t R, int nxh, int ny)
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
    pl.nxp = (nxh + 3) & ~3;
    pl.fwd_bytes = (size_t)GW * pl.nbx_fwd * ny * nxh * sizeof(float);
    pl.gpad_bytes = (((size_t)GW * ny * pl.nxp * sizeof(float)) + 255u) & ~(size_t)255u;
    pl.bwd_bytes = pl.gpad_bytes + (size_t)GW * pl.nbx_bwd * 3 * sizeof(double);
    return pl;
}

int check_args(const char *fn, int32_t G, int32_t W, int64_t R, const float *x, const float *y, const float *weight,
               const uint8_t *ok, const float *x_pitch, const float *y_pitch, const float *y_centre, int32_t nxh, int32_t ny)
{
    static thread_local char msg[256];
    const char *what = nullptr;
    if (!x || !y || !x_pitch || !y_pitch || !y_centre) what = "a required pointer is NULL";
    else if (nxh < 1 || nxh > 32 || ny < 1 || ny > 32) what = "nxh and ny must be in 1..32";
    else if (G < 1 || W < 1 || (int64_t)G * W > 65535) what = "G and W must be >= 1 and G*W <= 65535";
    else if (R < 1) what = "R must be >= 1";
    else if (weight && ok) what = "give weight or ok, not both";
    if (!what) return TL_OK;
    snprintf(msg, sizeof(msg), "%s: %s", fn, what);
    return tl_host::fail(TL_EINVAL, msg);
}

template <int NXP>
void launch_bwd(const PsfIn &in, const PsfPlan &pl, int GW, const float *gpad, float *gx, float *gy, double *part, hipStream_t st)
{
    hipLaunchKernelGGL(psf_bwd_kernel<NXP>, dim3(pl.nbx_bwd, GW), dim3(kBlock), 0, st, in, gpad, gx, gy, part, pl.rpl);
}

// ------------------------------------------------------------------------------------------------------------------------
// The rotated PSF grid (tl_psf_rot_*): G grids read K fans, grid g the fan src[g] turned by (c[g], s[g]) about the fan's
// centre.  The rotation and the fan lookup sit in the load; everything after it is the arithmetic of the kernels above.

constexpr int kRowFold = 32768;                 // rows per grid-y; row = blockIdx.z kRowFold + blockIdx.y
constexpr int64_t kRotMaxRows = 1 << 20;        // G W and K W
constexpr int64_t kRotMaxWork = (int64_t)1 << 36;

struct RotIn {
    const float *x, *y, *weight;
    const uint8_t *ok;
    int64_t s_g, s_w, R;
    const int32_t *src;
    const float *c, *s, *x_pitch, *y_pitch, *y_centre;
    int G, K, W, nx, ny;
    float x_first, y_first;
};

// A source ray, centred: (0, 0, weight 0) past the end of the fan or at weight 0 -- dropped before any rotation.
struct SrcRay { float xi, eta, wt; };

__device__ __forceinline__ SrcRay load_src(const RotIn &in, const int64_t off, const int64_t r, const float yc)
{
    SrcRay q = {0.f, 0.f, 0.f};
    if (r < in.R) {
        const float wt = in.weight ? in.weight[off + r] : (in.ok ? (in.ok[off + r] ? 1.f : 0.f) : 1.f);
        if (wt != 0.f) {
            q.xi = in.x[off + r];
            q.eta = in.y[off + r] - yc;
            q.wt = wt;
        }
    }
    return q;
}

// x' = c xi + s eta, y' = -s xi + c eta (one product and one fma each), then pitch units as load_ray carries them
__device__ __forceinline__ Ray rotate(const SrcRay &q, const float c, const float s, const float px, const float py)
{
    Ray o;
    o.x = __builtin_fmaf(c, q.xi, s * q.eta);
    o.yc = __builtin_fmaf(c, q.eta, -(s * q.xi));
    o.u = o.x / px;
    o.v = o.yc / py;
    o.ul = __builtin_fmaf(-o.u, px, o.x) / px;
    o.vl = __builtin_fmaf(-o.v, py, o.yc) / py;
    o.wt = q.wt;
    return o;
}

// grid (nbx, min(G W, kRowFold), ceil(G W / kRowFold)); otherwise psf_fwd_kernel
__global__ __launch_bounds__(kBlock) void psf_rot_fwd_kernel(const RotIn in, float *__restrict__ part, const int nb)
{
    __shared__ double tile[kWaves][16][64];
    const int gw = blockIdx.z * kRowFold + blockIdx.y;
    if (gw >= in.G * in.W) return;                                      // block-uniform, before any barrier
    const int g = gw / in.W, w = gw - g * in.W, k = in.src[g];
    const int64_t off = (int64_t)k * in.s_g + (int64_t)w * in.s_w;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int idx = lane & 31, src0 = lane & 32;
    const float px = in.x_pitch[g], py = in.y_pitch[g], yc = in.y_centre[k], cg = in.c[g], sg = in.s[g];
    const float ax = in.x_first + (float)idx, ay = in.y_first + (float)idx;
    const int64_t batch0 = ((int64_t)blockIdx.x * kWaves + wv) * nb;
    double tot[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) tot[r] = 0.0;
    for (int b = 0; b < nb; ++b) {
        const int64_t r0 = (batch0 + b) * 64;
        if (r0 >= in.R) break;                                      // wave-uniform
        const Ray q = rotate(load_src(in, off, r0 + lane, yc), cg, sg, px, py);
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
#pragma unroll
    for (int r = 0; r < 16; ++r) tile[wv][r][lane] = tot[r];
    __syncthreads();
    float *__restrict__ out = part + ((size_t)gw * gridDim.x + blockIdx.x) * (size_t)(in.ny * in.nx);
    for (int e = tid; e < 16 * 64; e += kBlock) {
        const int r = e >> 6, l = e & 63;
        const int row = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5), col = l & 31;     // C/D map of the 32x32 MFMA
        if (row < in.ny && col < in.nx) {
            double s = 0.0;
#pragma unroll
            for (int kk = 0; kk < kWaves; ++kk) s += tile[kk][r][l];
            out[row * in.nx + col] = (float)s;
        }
    }
}

// grid (nbx, min(K W, kRowFold), ceil(K W / kRowFold)): one lane per SOURCE ray, lane t of block bx takes rays
// (bx rpl + q) kBlock + t, q < rpl, and walks the grids of its fan in list order.  gpad [G W, ny, NXP] as psf_pad_kernel
// leaves it.  part [K W, nbx, 3] doubles, slot 2 only: the block's sum of gy (psf_bwd_reduce_kernel finishes g_y_centre).
template <int NXP>
__global__ __launch_bounds__(kBlock) void psf_rot_bwd_kernel(const RotIn in, const int32_t *__restrict__ field_start,
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
            const float *__restrict__ gp = gpad + ((size_t)g * in.W + w) * ny * NXP;
            const Ray q = rotate(sr, cg, sg, px, py);
            float Gx[NXP], Gd[NXP];
#pragma unroll
            for (int j = 0; j < NXP; ++j) {
                const float d = (q.u - (in.x_first + (float)j)) + q.ul;
                Gx[j] = gauss(d);
                Gd[j] = -4.f * d * Gx[j];
            }
            float A = 0.f, Bq = 0.f;
            for (int i = 0; i < ny; ++i) {
                const float d = (q.v - (in.y_first + (float)i)) + q.vl;
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

int check_rot_args(const char *fn, int32_t G, int32_t K, int32_t W, int64_t R, const float *x, const float *y, const float *weight,
                   const uint8_t *ok, const int32_t *src, const float *c, const float *s, const float *x_pitch,
                   const float *y_pitch, const float *y_centre, int32_t nx, int32_t ny)
{
    static thread_local char msg[256];
    const char *what = nullptr;
    if (!x || !y || !src || !c || !s || !x_pitch || !y_pitch || !y_centre) what = "a required pointer is NULL";
    else if (nx < 1 || nx > 32 || ny < 1 || ny > 32) what = "nx and ny must be in 1..32";
    else if (G < 1 || K < 1 || W < 1 || (int64_t)G * W > kRotMaxRows || (int64_t)K * W > kRotMaxRows)
        what = "G, K and W must be >= 1 and G*W, K*W <= 1048576";
    else if (R < 1) what = "R must be >= 1";
    else if (R > kRotMaxWork / ((int64_t)G * W) || R > kRotMaxWork / ((int64_t)K * W)) what = "G*W*R and K*W*R must be <= 2^36";
    else if (weight && ok) what = "give weight or ok, not both";
    if (!what) return TL_OK;
    snprintf(msg, sizeof(msg), "%s: %s", fn, what);
    return tl_host::fail(TL_EINVAL, msg);
}

inline dim3 fold_rows(int nbx, int rows) { return dim3(nbx, rows < kRowFold ? rows : kRowFold, (rows + kRowFold - 1) / kRowFold); }

template <int NXP>
void launch_rot_bwd(const RotIn &in, const RotPlan &pl, const int32_t *field_start, const int32_t *field_grids, const float *gpad,
                    float *gx, float *gy, double *part, hipStream_t st)
{
    hipLaunchKernelGGL(psf_rot_bwd_kernel<NXP>, fold_rows(pl.b.nbx_bwd, in.K * in.W), dim3(kBlock), 0, st, in, field_start,
                       field_grids, gpad, gx, gy, part, pl.b.rpl);
}

}  // namespace

extern "C" {

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
    const int rc = check_rot_args("tl_psf_rot_accumulate", G, K, W, R, x, y, weight, ok, src, c, s, x_pitch, y_pitch, y_centre, nx, ny);
    if (rc) return rc;
    if (!hist) return tl_host::fail(TL_EINVAL, "tl_psf_rot_accumulate: hist is NULL");
    const RotPlan pl = psf_rot_plan(G, K, W, R, nx, ny);
    if (!workspace || workspace_bytes < pl.fwd_bytes)
        return tl_host::fail(TL_EWORKSPACE, "workspace too small for tl_psf_rot_accumulate");
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return tl_host::hip_fail(e, "hipSetDevice");
    hipStream_t st = (hipStream_t)stream;
    const RotIn in = {x, y, weight, ok, s_g, s_w, R, src, c, s, x_pitch, y_pitch, y_centre, G, K, W, nx, ny, x_first, y_first};
    const int GW = G * W, nbins = ny * nx;
    hipLaunchKernelGGL(psf_rot_fwd_kernel, fold_rows(pl.f.nbx_fwd, GW), dim3(kBlock), 0, st, in, (float *)workspace, pl.f.nb);
    int herr = (int)hipGetLastError();
    if (herr) return tl_host::hip_fail(herr, "psf_rot_fwd_kernel launch");
    for (int row0 = 0; row0 < GW; row0 += kRowFold) {        // psf_reduce_kernel as it is, kRowFold rows at a time
        const int rows = GW - row0 < kRowFold ? GW - row0 : kRowFold;
        hipLaunchKernelGGL(psf_reduce_kernel, dim3((nbins + 63) / 64, rows), dim3(64, 4), 0, st,
                           (const float *)workspace + (size_t)row0 * pl.f.nbx_fwd * nbins, hist + (size_t)row0 * nbins,
                           pl.f.nbx_fwd, nbins);
        herr = (int)hipGetLastError();
        if (herr) return tl_host::hip_fail(herr, "psf_reduce_kernel launch");
    }
    return TL_OK;
}

int tl_psf_rot_accumulate_bwd(int32_t device, int32_t G, int32_t K, int32_t W, int64_t R, const float *x, const float *y,
                              const float *weight, const uint8_t *ok, int64_t s_g, int64_t s_w, const int32_t *src,
                              const float *c, const float *s, const float *x_pitch, const float *y_pitch,
                              const float *y_centre, int32_t nx, int32_t ny, float x_first, float y_first,
                              const int32_t *field_start, const int32_t *field_grids, const float *g_hist, float *gx, float *gy,
                              float *g_y_centre, void *workspace, size_t workspace_bytes, void *stream)
{
    const int rc = check_rot_args("tl_psf_rot_accumulate_bwd", G, K, W, R, x, y, weight, ok, src, c, s, x_pitch, y_pitch, y_centre,
                                  nx, ny);
    if (rc) return rc;
    if (!field_start || !field_grids || !g_hist || !gx || !gy)
        return tl_host::fail(TL_EINVAL, "tl_psf_rot_accumulate_bwd: field_start, field_grids, g_hist, gx or gy is NULL");
    const RotPlan pl = psf_rot_plan(G, K, W, R, nx, ny);
    if (!workspace || workspace_bytes < pl.bwd_bytes)
        return tl_host::fail(TL_EWORKSPACE, "workspace too small for tl_psf_rot_accumulate_bwd");
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return tl_host::hip_fail(e, "hipSetDevice");
    hipStream_t st = (hipStream_t)stream;
    const RotIn in = {x, y, weight, ok, s_g, s_w, R, src, c, s, x_pitch, y_pitch, y_centre, G, K, W, nx, ny, x_first, y_first};
    const int rows = G * W * ny, nxp = pl.f.nxp;
    float *gpad = (float *)workspace;
    double *part = (double *)((char *)workspace + pl.f.gpad_bytes);
    hipLaunchKernelGGL(psf_pad_kernel, dim3((rows * nxp + 255) / 256), dim3(256), 0, st, g_hist, gpad, rows, nx, nxp);
    int herr = (int)hipGetLastError();
    if (herr) return tl_host::hip_fail(herr, "psf_pad_kernel launch");
    switch (nxp) {
    case 4: launch_rot_bwd<4>(in, pl, field_start, field_grids, gpad, gx, gy, part, st); break;
    case 8: launch_rot_bwd<8>(in, pl, field_start, field_grids, gpad, gx, gy, part, st); break;
    case 12: launch_rot_bwd<12>(in, pl, field_start, field_grids, gpad, gx, gy, part, st); break;
    case 16: launch_rot_bwd<16>(in, pl, field_start, field_grids, gpad, gx, gy, part, st); break;
    case 20: launch_rot_bwd<20>(in, pl, field_start, field_grids, gpad, gx, gy, part, st); break;
    case 24: launch_rot_bwd<24>(in, pl, field_start, field_grids, gpad, gx, gy, part, st); break;
    case 28: launch_rot_bwd<28>(in, pl, field_start, field_grids, gpad, gx, gy, part, st); break;
    default: launch_rot_bwd<32>(in, pl, field_start, field_grids, gpad, gx, gy, part, st); break;
    }
    herr = (int)hipGetLastError();
    if (herr) return tl_host::hip_fail(herr, "psf_rot_bwd_kernel launch");
    if (g_y_centre) {       // psf_bwd_reduce_kernel as it is: only its third quantity has a destination, the others return
        hipLaunchKernelGGL(psf_bwd_reduce_kernel, dim3(K * 3), dim3(64), 0, st, (const double *)part, W * pl.b.nbx_bwd,
                           (const float *)nullptr, (const float *)nullptr, (float *)nullptr, (float *)nullptr, g_y_centre);
        herr = (int)hipGetLastError();
        if (herr) return tl_host::hip_fail(herr, "psf_bwd_reduce_kernel launch");
    }
    return TL_OK;
}

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
    const int rc = check_args("tl_psf_accumulate", G, W, R, x, y, weight, ok, x_pitch, y_pitch, y_centre, nxh, ny);
    if (rc) return rc;
    if (!hist) return tl_host::fail(TL_EINVAL, "tl_psf_accumulate: hist is NULL");
    const PsfPlan pl = psf_plan(G, W, R, nxh, ny);
    if (!workspace || workspace_bytes < pl.fwd_bytes) return tl_host::fail(TL_EWORKSPACE, "workspace too small for tl_psf_accumulate");
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return tl_host::hip_fail(e, "hipSetDevice");
    hipStream_t st = (hipStream_t)stream;
    const PsfIn in = {x, y, weight, ok, s_g, s_w, R, x_pitch, y_pitch, y_centre, W, nxh, ny, x_first, y_first};
    const int GW = G * W, nbins = ny * nxh;
    hipLaunchKernelGGL(psf_fwd_kernel, dim3(pl.nbx_fwd, GW), dim3(kBlock), 0, st, in, (float *)workspace, pl.nb);
    int herr = (int)hipGetLastError();
    if (herr) return tl_host::hip_fail(herr, "psf_fwd_kernel launch");
    hipLaunchKernelGGL(psf_reduce_kernel, dim3((nbins + 63) / 64, GW), dim3(64, 4), 0, st, (const float *)workspace, hist,
                       pl.nbx_fwd, nbins);
    herr = (int)hipGetLastError();
    if (herr) return tl_host::hip_fail(herr, "psf_reduce_kernel launch");
    return TL_OK;
}

int tl_psf_accumulate_bwd(int32_t device, int32_t G, int32_t W, int64_t R, const float *x, const float *y, const float *weight,
                          const uint8_t *ok, int64_t s_g, int64_t s_w, const float *x_pitch, const float *y_pitch,
                          const float *y_centre, int32_t nxh, int32_t ny, float x_first, float y_first, const float *g_hist,
                          float *gx, float *gy, float *g_x_pitch, float *g_y_pitch, float *g_y_centre, void *workspace,
                          size_t workspace_bytes, void *stream)
{
    const int rc = check_args("tl_psf_accumulate_bwd", G, W, R, x, y, weight, ok, x_pitch, y_pitch, y_centre, nxh, ny);
    if (rc) return rc;
    if (!g_hist || !gx || !gy) return tl_host::fail(TL_EINVAL, "tl_psf_accumulate_bwd: g_hist, gx or gy is NULL");
    const PsfPlan pl = psf_plan(G, W, R, nxh, ny);
    if (!workspace || workspace_bytes < pl.bwd_bytes)
        return tl_host::fail(TL_EWORKSPACE, "workspace too small for tl_psf_accumulate_bwd");
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return tl_host::hip_fail(e, "hipSetDevice");
    hipStream_t st = (hipStream_t)stream;
    const PsfIn in = {x, y, weight, ok, s_g, s_w, R, x_pitch, y_pitch, y_centre, W, nxh, ny, x_first, y_first};
    const int GW = G * W, rows = GW * ny;
    float *gpad = (float *)workspace;
    double *part = (double *)((char *)workspace + pl.gpad_bytes);
    hipLaunchKernelGGL(psf_pad_kernel, dim3((rows * pl.nxp + 255) / 256), dim3(256), 0, st, g_hist, gpad, rows, nxh, pl.nxp);
    int herr = (int)hipGetLastError();
    if (herr) return tl_host::hip_fail(herr, "psf_pad_kernel launch");
    switch (pl.nxp) {
    case 4: launch_bwd<4>(in, pl, GW, gpad, gx, gy, part, st); break;
    case 8: launch_bwd<8>(in, pl, GW, gpad, gx, gy, part, st); break;
    case 12: launch_bwd<12>(in, pl, GW, gpad, gx, gy, part, st); break;
    case 16: launch_bwd<16>(in, pl, GW, gpad, gx, gy, part, st); break;
    case 20: launch_bwd<20>(in, pl, GW, gpad, gx, gy, part, st); break;
    case 24: launch_bwd<24>(in, pl, GW, gpad, gx, gy, part, st); break;
    case 28: launch_bwd<28>(in, pl, GW, gpad, gx, gy, part, st); break;
    default: launch_bwd<32>(in, pl, GW, gpad, gx, gy, part, st); break;
    }
    herr = (int)hipGetLastError();
    if (herr) return tl_host::hip_fail(herr, "psf_bwd_kernel launch");
    if (g_x_pitch || g_y_pitch || g_y_centre) {
        hipLaunchKernelGGL(psf_bwd_reduce_kernel, dim3(G * 3), dim3(64), 0, st, (const double *)part, W * pl.nbx_bwd, x_pitch,
                           y_pitch, g_x_pitch, g_y_pitch, g_y_centre);
        herr = (int)hipGetLastError();
        if (herr) return tl_host::hip_fail(herr, "psf_bwd_reduce_kernel launch");
    }
    return TL_OK;
}

}  // extern "C"
