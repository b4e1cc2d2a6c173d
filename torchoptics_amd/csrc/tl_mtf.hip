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
// LAYOUT, PLAN, PARTIALS AND REDUCE are the row frame's (tl_rows.h).  The 2 J running sums are a static register array of the
// compile-time bucket JB = 4 / 8 / 16 >= J; the frequency vectors travel in a by-value kernel argument, so nothing is uploaded,
// and are staged in LDS, read wave-uniformly (a broadcast); slots from J on hold 0 and their sums are never stored.  A column's
// bits do not depend on which other columns the call holds.
// SEED.  mtf_seed_kernel walks the rays the same way, the row's 2 J seeds (gC_j, gS_j) staged in LDS next to the frequencies:
//   q_j = gS_j cos(2 pi r_j) - gC_j sin(2 pi r_j),   gx = 2 pi sum_j nu_xj q_j,   gy = 2 pi sum_j nu_yj q_j,
// the sums over j = 0 .. J - 1 in that order in fp64, times 2 pi, rounded once to fp32 at the store.  Dead rays get zeros.  The
// modulus of the OTF does not depend on the origin, so there is no gradient to it and nothing to reduce.
#include "tl_rows.h"

#include <math.h>

namespace {

constexpr int kMaxJ = 16;                       // frequency vectors per call (the largest register bucket)
constexpr double kTwoPi = 6.283185307179586476925286766559;

struct Rays {
    const float *x, *y;
    const uint8_t *ok;
    int64_t s_f, s_p, s_w;
};

struct Freq { double nx[kMaxJ], ny[kMaxJ]; };   // cycles per unit of x; slots from J on hold 0

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

__global__ __launch_bounds__(kBlock) void mtf_reduce_kernel(const double *__restrict__ part, double *__restrict__ out,
                                                            int64_t total, int nbx, int n)
{
    reduce_rows(part, out, total, nbx, n);
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
    Checked c = {TL_OK, {}};
    const char *what = nullptr;
    if (const char *bad = size_fault(F, P, W)) what = bad;
    else if (!r.x || !r.y || !r.ok) what = "x, y and ok are required";
    else if (missing) what = missing;
    else if (J < 1 || J > kMaxJ) what = "J must be 1 .. 16";
    else if (!nu_x || !nu_y) what = "nu_x and nu_y (host) are required";
    for (int j = 0; j < J && !what; ++j) {
        if (!(std::isfinite(nu_x[j]) && std::isfinite(nu_y[j]))) what = "every frequency must be finite";
        c.fq.nx[j] = nu_x[j];
        c.fq.ny[j] = nu_y[j];
    }
    c.rc = what ? refuse(name, what) : check_workspace(name, ws, ws_bytes, tl_mtf_workspace_bytes(F, P, W, J), "tl_mtf_workspace_bytes");
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
    if (size_fault(F, P, W) || J < 1 || J > kMaxJ) return 0;
    return (size_t)(F * W) * (size_t)row_plan(F * W, P).nbx * (size_t)(2 * J) * sizeof(double);
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
    const Plan pl = row_plan(rows, P);
    hipStream_t st = (hipStream_t)stream;
    if (const int rc = launch_rows(rows, pl.nbx, "mtf_sums_kernel launch", [&](dim3 grid, int row0) {
            sums_launcher(J)(grid, st, r, P, (int)W, row0, origin, c.fq, J, (double *)workspace, pl);
        }))
        return rc;
    return launch_reduce(mtf_reduce_kernel, "mtf_reduce_kernel launch", (const double *)workspace, sums, rows, pl.nbx, 2 * J, st);
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
    const Plan pl = row_plan(F * W, P);
    return launch_rows(F * W, pl.nbx, "mtf_seed_kernel launch", [&](dim3 grid, int row0) {
        hipLaunchKernelGGL(mtf_seed_kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, r, P, (int)W, row0, origin, c.fq, J, g_sums,
                           gx, gy, pl.R);
    });
}

}  // extern "C"
