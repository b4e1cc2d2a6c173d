// tl_mtf.hip -- the geometric OTF of a traced fan as Fourier sums over the spot, and its seeds (tl_mtf_sums, tl_mtf_seed of
// include/tl_trace.h; metrics.otf_sums / metrics.geometric_mtf stand on them).
//
// Per row (f, w), over the LIVE rays (ok != 0), with the row's origin o and the frequency vectors (nu_x, nu_y)_j, j < J:
//   dx = (double)x - o_x,  dy = (double)y - o_y
//   u  = nu_x dx + nu_y dy                      two products, one sum: cycles
//   r  = u - rint(u)                            exact in fp64, |r| <= 1/2
//   sums[j] = (C_j, S_j) = (sum cos(2 pi r), sum sin(2 pi r))      sincospi(2 r): the factor 2 is exact, pi never multiplies in
// Every operation is in fp64 from the fp32 inputs and nothing is contracted (contract(off)).  An image height of 9 mm at 75
// cycles / mm is a phase of ~700 cycles: fp32 anywhere in u leaves nothing of it.  nu = 0 gives u = 0, r = 0 and the term (1, 0)
// exactly, so C = n and S = 0 without a rounding.  A dead ray is excluded by a select: whatever it holds reaches no sum.
//
// LAYOUT AND PLAN are the enclosed-energy kernels' (tl_enclosed.hip), restated here: grid (nbx, rows of this launch), 256 lanes;
// block bx of a row takes the rays [bx R 1024, (bx + 1) R 1024); where the ray stride is 1 and the row's base addresses are
// aligned a lane takes four consecutive rays with 16-byte loads (ok as one dword), otherwise one ray at a time.  The 2 J running
// sums are a static register array of the compile-time bucket JB = 4 / 8 / 16 >= J; the frequency vectors travel in a by-value
// kernel argument, so nothing is uploaded, and are staged in LDS, read wave-uniformly (a broadcast); slots from J on hold 0 and
// their sums are never stored.  A butterfly over the wave, the four waves added in order through LDS, one partial per block in the
// workspace, mtf_reduce_kernel adds a row's partials in order.  No atomics: the same bits on every run, and a column's bits do
// not depend on which other columns the call holds.
// SEED.  mtf_seed_kernel walks the rays the same way, the row's 2 J seeds (gC_j, gS_j) staged in LDS next to the frequencies:
//   q_j = gS_j cos(2 pi r_j) - gC_j sin(2 pi r_j),   gx = 2 pi sum_j nu_xj q_j,   gy = 2 pi sum_j nu_yj q_j,
// the sums over j = 0 .. J - 1 in that order in fp64, times 2 pi, rounded once to fp32 at the store.  Dead rays get zeros.  The
// modulus of the OTF does not depend on the origin, so there is no gradient to it and nothing to reduce.
#include "tl_common.h"

#include <math.h>
#include <stdio.h>

#include <algorithm>

namespace {

constexpr int kBlock = 256;
constexpr int kVec = 4;                         // rays per lane and load on the aligned path
constexpr int kChunk = kBlock * kVec;           // rays a block takes per step: the unit of the plan
constexpr int kMaxY = 65535;                    // rows per launch (grid y)
constexpr int kMaxJ = 16;                       // frequency vectors per call (the largest register bucket)
constexpr int64_t kTargetBlocks = 2048;         // 256 CUs x 8 blocks of 4 waves
constexpr int64_t kMaxDim = ((int64_t)1 << 31) - 1;
constexpr double kTwoPi = 6.283185307179586476925286766559;

struct Rays {
    const float *x, *y;
    const uint8_t *ok;
    int64_t s_f, s_p, s_w;
};

struct Freq { double nx[kMaxJ], ny[kMaxJ]; };   // cycles per unit of x; slots from J on hold 0

struct Plan { int nbx, R; };                    // blocks per row, steps of kChunk rays per block

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

Plan mtf_plan(int64_t rows, int64_t P)
{
    const int64_t chunks = cdiv(P, kChunk);
    const int64_t want = std::max<int64_t>(1, cdiv(kTargetBlocks, rows));
    const int64_t R = cdiv(chunks, std::min(chunks, want));
    return {(int)cdiv(chunks, R), (int)R};
}

__device__ __forceinline__ bool aligned_to(const void *p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1u)) == 0; }

// body(o, xs, ys, oks) on every ray of [first, last) that this lane owns: four consecutive rays at element offset o on the
// aligned path, one elsewhere (the arrays' length says which)
template <class Body>
__device__ __forceinline__ void walk_rays(const float *__restrict__ x, const float *__restrict__ y, const uint8_t *__restrict__ ok,
                                          int64_t s_p, bool vec, int64_t first, int64_t last, int64_t P, Body &&body)
{
    if (vec) {                                              // (uniform over the block)
        for (int64_t ip = first + kVec * (int64_t)threadIdx.x; ip < last; ip += kChunk) {
            if (ip + kVec <= P) {
                const float4 x4 = *reinterpret_cast<const float4 *>(x + ip), y4 = *reinterpret_cast<const float4 *>(y + ip);
                const unsigned o4 = *reinterpret_cast<const unsigned *>(ok + ip);
                const float xs[kVec] = {x4.x, x4.y, x4.z, x4.w}, ys[kVec] = {y4.x, y4.y, y4.z, y4.w};
                const unsigned oks[kVec] = {o4 & 0xffu, o4 & 0xff00u, o4 & 0xff0000u, o4 & 0xff000000u};
                body(ip, xs, ys, oks);
            } else {                                        // the last one to three rays of the row
                for (int64_t q = ip; q < P; ++q) {
                    const float xs[1] = {x[q]}, ys[1] = {y[q]};
                    const unsigned oks[1] = {ok[q]};
                    body(q, xs, ys, oks);
                }
            }
        }
    } else {
        for (int64_t ip = first + threadIdx.x; ip < last; ip += kBlock) {
            const int64_t o = ip * s_p;
            const float xs[1] = {x[o]}, ys[1] = {y[o]};
            const unsigned oks[1] = {ok[o]};
            body(o, xs, ys, oks);
        }
    }
}

// part[(row nbx + bx) n + j] = the block's sum of m[j], j < n <= N: a butterfly over the wave, the four waves in order
template <int N>
__device__ __forceinline__ void block_partial(const double (&m)[N], double *__restrict__ part, int row, int nbx, int n)
{
    __shared__ double red[kBlock / 64][N];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        double v = m[j];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) red[wv][j] = v;
    }
    __syncthreads();
    if ((int)threadIdx.x < n) {
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < kBlock / 64; ++q) s += red[q][threadIdx.x];
        part[((int64_t)row * nbx + blockIdx.x) * n + threadIdx.x] = s;
    }
}

struct RowBase {
    const float *x, *y;
    const uint8_t *ok;
    int64_t off;
    int row;
};

__device__ __forceinline__ RowBase row_base(const Rays &r, int W, int row0)
{
    const int row = row0 + (int)blockIdx.y;
    const int f = row / W, w = row - f * W;
    const int64_t off = f * r.s_f + w * r.s_w;
    return {r.x + off, r.y + off, r.ok + off, off, row};
}

// (cos, sin)(2 pi r) of the phase u = nu_x dx + nu_y dy cycles, r = u - rint(u): the term of the definition
__device__ __forceinline__ void term(double nx, double ny, double dx, double dy, double *c, double *s)
{
#pragma clang fp contract(off)
    const double u = nx * dx + ny * dy;
    const double r = u - rint(u);
    sincospi(2.0 * r, s, c);
}

// m[2 j], m[2 j + 1] = (C_j, S_j) of the block's rays, j < JB; the first 2 J of them go to the block's partial
template <int JB>
__global__ __launch_bounds__(kBlock) void mtf_sums_kernel(Rays r, int64_t P, int W, int row0, const double *__restrict__ origin,
                                                          Freq fq, int J, double *__restrict__ part, int nbx, int R)
{
#pragma clang fp contract(off)
    const RowBase b = row_base(r, W, row0);
    const double o_x = origin[2 * (int64_t)b.row], o_y = origin[2 * (int64_t)b.row + 1];
    const int64_t first = (int64_t)blockIdx.x * R * kChunk;
    const int64_t last = std::min(first + (int64_t)R * kChunk, P);
    // read from LDS (one address per wave: a broadcast) the frequencies cost no register between uses
    __shared__ double nx[JB], ny[JB];
    if ((int)threadIdx.x < JB) {
        nx[threadIdx.x] = fq.nx[threadIdx.x];
        ny[threadIdx.x] = fq.ny[threadIdx.x];
    }
    __syncthreads();
    double m[2 * JB];
#pragma unroll
    for (int k = 0; k < 2 * JB; ++k) m[k] = 0.0;
    const bool vec = r.s_p == 1 && aligned_to(b.x, 16) && aligned_to(b.y, 16) && aligned_to(b.ok, 4);
    walk_rays(b.x, b.y, b.ok, r.s_p, vec, first, last, P, [&](int64_t, const auto &xs, const auto &ys, const auto &oks) {
        constexpr int N = sizeof(xs) / sizeof(xs[0]);
        double dx[N], dy[N];
        bool live[N];
#pragma unroll
        for (int i = 0; i < N; ++i) {
            live[i] = oks[i] != 0u;
            // a dead ray is the ray at 0 that is not counted: nothing of what it holds reaches a sum
            dx[i] = (live[i] ? (double)xs[i] : 0.0) - o_x;
            dy[i] = (live[i] ? (double)ys[i] : 0.0) - o_y;
        }
#pragma unroll
        for (int j = 0; j < JB; ++j) {
#pragma unroll
            for (int i = 0; i < N; ++i) {
                double c, s;
                term(nx[j], ny[j], dx[i], dy[i], &c, &s);
                m[2 * j] += live[i] ? c : 0.0;
                m[2 * j + 1] += live[i] ? s : 0.0;
            }
            __builtin_amdgcn_sched_barrier(0);              // one frequency per scheduling region: the next one's terms stay behind it
        }
    });
    block_partial(m, part, b.row, nbx, 2 * J);
}

// out[row][j] = the row's nbx partials added in order
__global__ __launch_bounds__(kBlock) void mtf_reduce_kernel(const double *__restrict__ part, double *__restrict__ out,
                                                            int64_t total, int nbx, int n)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= total) return;
    const int64_t row = i / n;
    const double *p = part + row * nbx * n + (i - row * n);
    double s = 0.0;
    for (int b = 0; b < nbx; ++b) s += p[(int64_t)b * n];
    out[i] = s;
}

__global__ __launch_bounds__(kBlock) void mtf_seed_kernel(Rays r, int64_t P, int W, int row0, const double *__restrict__ origin,
                                                          Freq fq, int J, const double *__restrict__ g_sums, float *gx_all,
                                                          float *gy_all, int R)
{
#pragma clang fp contract(off)
    const RowBase b = row_base(r, W, row0);
    const double o_x = origin[2 * (int64_t)b.row], o_y = origin[2 * (int64_t)b.row + 1];
    float *__restrict__ gx = gx_all ? gx_all + b.off : nullptr, *__restrict__ gy = gy_all ? gy_all + b.off : nullptr;
    __shared__ double nx[kMaxJ], ny[kMaxJ], gC[kMaxJ], gS[kMaxJ];      // (no register array is indexed by j here: a plain loop to J)
    if ((int)threadIdx.x < J) {
        nx[threadIdx.x] = fq.nx[threadIdx.x];
        ny[threadIdx.x] = fq.ny[threadIdx.x];
        gC[threadIdx.x] = g_sums[((int64_t)b.row * J + threadIdx.x) * 2];
        gS[threadIdx.x] = g_sums[((int64_t)b.row * J + threadIdx.x) * 2 + 1];
    }
    __syncthreads();
    const int64_t first = (int64_t)blockIdx.x * R * kChunk;
    const int64_t last = std::min(first + (int64_t)R * kChunk, P);
    // (a NULL output is aligned)
    const bool vec = r.s_p == 1 && aligned_to(b.x, 16) && aligned_to(b.y, 16) && aligned_to(b.ok, 4) && aligned_to(gx, 16)
                     && aligned_to(gy, 16);
    walk_rays(b.x, b.y, b.ok, r.s_p, vec, first, last, P, [&](int64_t o, const auto &xs, const auto &ys, const auto &oks) {
        constexpr int N = sizeof(xs) / sizeof(xs[0]);
        double dx[N], dy[N], ax[N], ay[N];
        bool live[N];
#pragma unroll
        for (int i = 0; i < N; ++i) {
            live[i] = oks[i] != 0u;
            dx[i] = (live[i] ? (double)xs[i] : 0.0) - o_x;
            dy[i] = (live[i] ? (double)ys[i] : 0.0) - o_y;
            ax[i] = ay[i] = 0.0;
        }
#pragma unroll 1
        for (int j = 0; j < J; ++j) {
#pragma unroll
            for (int i = 0; i < N; ++i) {
                double c, s;
                term(nx[j], ny[j], dx[i], dy[i], &c, &s);
                const double q = gS[j] * c - gC[j] * s;
                ax[i] += nx[j] * q;
                ay[i] += ny[j] * q;
            }
        }
        float ox[N], oy[N];
#pragma unroll
        for (int i = 0; i < N; ++i) {
            ox[i] = live[i] ? (float)(kTwoPi * ax[i]) : 0.0f;
            oy[i] = live[i] ? (float)(kTwoPi * ay[i]) : 0.0f;
        }
        if constexpr (N == kVec) {
            if (gx) *reinterpret_cast<float4 *>(gx + o) = make_float4(ox[0], ox[1], ox[2], ox[3]);
            if (gy) *reinterpret_cast<float4 *>(gy + o) = make_float4(oy[0], oy[1], oy[2], oy[3]);
        } else {
            if (gx) gx[o] = ox[0];
            if (gy) gy[o] = oy[0];
        }
    });
}

struct Checked { int rc; Freq fq; };

// the argument check the calls share; `name` opens the message.  Sizes, pointers, then the frequency vectors (host) into
// the kernel argument, then the workspace: everything before the first HIP call.
Checked check_call(const char *name, int64_t F, int64_t P, int64_t W, const Rays &r, const char *missing, const double *nu_x,
                   const double *nu_y, int J, const void *ws, size_t ws_bytes)
{
    static thread_local char msg[200];
    Checked c = {TL_OK, {}};
    int code = TL_EINVAL;
    const char *what = nullptr;
    if (F < 1 || P < 1 || W < 1) what = "F, P and W must be at least 1";
    else if (F > kMaxDim || W > kMaxDim || F * W > kMaxDim || P > kMaxDim) what = "F W and P must stay below 2^31";
    else if (!r.x || !r.y || !r.ok) what = "x, y and ok are required";
    else if (missing) what = missing;
    else if (J < 1 || J > kMaxJ) what = "J must be 1 .. 16";
    else if (!nu_x || !nu_y) what = "nu_x and nu_y (host) are required";
    else {
        for (int j = 0; j < J && !what; ++j) {
            if (!(std::isfinite(nu_x[j]) && std::isfinite(nu_y[j]))) what = "every frequency must be finite";
            c.fq.nx[j] = nu_x[j];
            c.fq.ny[j] = nu_y[j];
        }
        if (!what && !(ws && ws_bytes >= tl_mtf_workspace_bytes(F, P, W, J))) {
            what = "workspace NULL or below tl_mtf_workspace_bytes";
            code = TL_EWORKSPACE;
        }
    }
    if (what) {
        snprintf(msg, sizeof msg, "%s: %s", name, what);
        c.rc = tl_host::fail(code, msg);
    }
    return c;
}

template <int JB>
void launch_sums(dim3 grid, hipStream_t st, const Rays &r, int64_t P, int W, int row0, const double *origin, const Freq &fq, int J,
                 double *part, const Plan &pl)
{
    hipLaunchKernelGGL((mtf_sums_kernel<JB>), grid, dim3(kBlock), 0, st, r, P, W, row0, origin, fq, J, part, pl.nbx, pl.R);
}

// the launcher of the register bucket JB = 4 / 8 / 16 that holds J
using SumsLauncher = void (*)(dim3, hipStream_t, const Rays &, int64_t, int, int, const double *, const Freq &, int, double *, const Plan &);
SumsLauncher sums_launcher(int J) { return J <= 4 ? launch_sums<4> : J <= 8 ? launch_sums<8> : launch_sums<16>; }

}  // namespace

extern "C" {

size_t tl_mtf_workspace_bytes(int64_t F, int64_t P, int64_t W, int J)
{
    if (F < 1 || P < 1 || W < 1 || F > kMaxDim || W > kMaxDim || F * W > kMaxDim || P > kMaxDim || J < 1 || J > kMaxJ) return 0;
    return (size_t)(F * W) * (size_t)mtf_plan(F * W, P).nbx * (size_t)(2 * J) * sizeof(double);
}

int tl_mtf_sums(int32_t device, int64_t F, int64_t P, int64_t W, const float *x, const float *y, const uint8_t *ok, int64_t s_f,
                int64_t s_p, int64_t s_w, const double *origin, const double *nu_x, const double *nu_y, int J, double *sums,
                void *workspace, size_t workspace_bytes, void *stream)
{
    const Rays r = {x, y, ok, s_f, s_p, s_w};
    const Checked c = check_call("tl_mtf_sums", F, P, W, r, !origin ? "the origin pointer is NULL" : !sums ? "the sums pointer is NULL" : nullptr,
                                 nu_x, nu_y, J, workspace, workspace_bytes);
    if (c.rc) return c.rc;
    if (const int rc = tl_host::use_device(device)) return rc;
    const int64_t rows = F * W;
    const Plan pl = mtf_plan(rows, P);
    hipStream_t st = (hipStream_t)stream;
    for (int64_t row0 = 0; row0 < rows; row0 += kMaxY) {
        const int ny = (int)std::min<int64_t>(kMaxY, rows - row0);
        sums_launcher(J)(dim3(pl.nbx, ny), st, r, P, (int)W, (int)row0, origin, c.fq, J, (double *)workspace, pl);
        if (const int rc = tl_host::launched("mtf_sums_kernel launch")) return rc;
    }
    const int64_t total = rows * 2 * J;
    hipLaunchKernelGGL(mtf_reduce_kernel, dim3((unsigned)cdiv(total, kBlock)), dim3(kBlock), 0, st, (const double *)workspace, sums,
                       total, pl.nbx, 2 * J);
    return tl_host::launched("mtf_reduce_kernel launch");
}

int tl_mtf_seed(int32_t device, int64_t F, int64_t P, int64_t W, const float *x, const float *y, const uint8_t *ok, int64_t s_f,
                int64_t s_p, int64_t s_w, const double *origin, const double *nu_x, const double *nu_y, int J, const double *g_sums,
                float *gx, float *gy, void *workspace, size_t workspace_bytes, void *stream)
{
    const Rays r = {x, y, ok, s_f, s_p, s_w};
    const Checked c = check_call("tl_mtf_seed", F, P, W, r, !origin ? "the origin pointer is NULL" : !g_sums ? "the g_sums pointer is NULL" :
                                 !gx && !gy ? "gx and gy are both NULL" : nullptr, nu_x, nu_y, J, workspace, workspace_bytes);
    if (c.rc) return c.rc;
    if (const int rc = tl_host::use_device(device)) return rc;
    const int64_t rows = F * W;
    const Plan pl = mtf_plan(rows, P);
    for (int64_t row0 = 0; row0 < rows; row0 += kMaxY) {
        const int ny = (int)std::min<int64_t>(kMaxY, rows - row0);
        hipLaunchKernelGGL(mtf_seed_kernel, dim3(pl.nbx, ny), dim3(kBlock), 0, (hipStream_t)stream, r, P, (int)W, (int)row0, origin,
                           c.fq, J, g_sums, gx, gy, pl.R);
        if (const int rc = tl_host::launched("mtf_seed_kernel launch")) return rc;
    }
    return TL_OK;
}

}  // extern "C"
