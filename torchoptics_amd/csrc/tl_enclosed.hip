// tl_enclosed.hip -- encircled / ensquared energy of a traced fan and its seeds (tl_enclosed_centroid, tl_enclosed_sums,
// tl_enclosed_seed of include/tl_trace.h; metrics.enclosed_energy / metrics.spot_centroid stand on them).
//
// Per row (f, w), over the LIVE rays (ok != 0), with the row's centre c, dx = x - c_x, dy = y - c_y:
//   S = (n, sum x, sum y)                                                       tl_enclosed_centroid
//   sums[k] = sum e_k,   circle: e_k = sigma((R_k - rho) inv_k), rho = sqrt(dx^2 + dy^2)
//                        square: e_k = sigma((R_k - |dx|) inv_k) sigma((R_k - |dy|) inv_k)          tl_enclosed_sums
//   sigma(u) = t^2 (3 - 2 t), t = (u + 1) / 2 clamped to [0, 1]: 0 below the band, 1 above it, C1 at both ends.
// Every difference, product, root and sum is in fp64 from the fp32 inputs and nothing is contracted (contract(off)): a ray's
// term has the bits of the definition evaluated in any IEEE fp64 arithmetic, only the ORDER of the sums is this file's.  The
// centre sits at millimetres while a spot measures microns, and (R - rho) inv amplifies rho's error by rho inv: fp32 would
// leave nothing of a band of a few microns.
//
// LAYOUT, PLAN, PARTIALS AND REDUCE are the row frame's (tl_rows.h).  The K running sums are a static register array of the
// compile-time bucket KB = 8 / 16 / 32 >= K; radii and 1 / softness travel in a by-value kernel argument, so nothing is uploaded,
// and are staged in LDS, read wave-uniformly (a broadcast).
// SEED.  enclosed_seed_kernel walks the rays the same way: the K seeds of the row staged in LDS next to the radii, per ray the sum over
// k of g_k d e_k / d(x, y) in fp64, rounded once to fp32 at the store; the centre's gradient is minus the sum of those over the
// row, through partials and the same reduce.  Dead rays get zeros.
#include "tl_rows.h"

#include <math.h>

namespace {

constexpr int kMaxK = 32;                       // radii per call
constexpr int kCircle = 0, kSquare = 1;

struct Rays {
    const float *x, *y;
    const uint8_t *ok;
    int64_t s_f, s_p, s_w;
};

struct Edge { double R[kMaxK], inv[kMaxK]; };   // radii and 1 / softness; slots from K on hold 0 and are never stored

// t of the edge: (u + 1) / 2 clamped to [0, 1]
__device__ __forceinline__ double edge_t(double u)
{
#pragma clang fp contract(off)
    return fmin(fmax(0.5 * (u + 1.0), 0.0), 1.0);               // (min / max, not selects: no lane mask per term to keep)
}
__device__ __forceinline__ double sigma(double t)
{
#pragma clang fp contract(off)
    return t * t * (3.0 - 2.0 * t);
}
__device__ __forceinline__ double dsigma(double t)                              // d sigma / du
{
#pragma clang fp contract(off)
    return 3.0 * t * (1.0 - t);
}

// The first KB radii and 1 / softness from the kernel argument into LDS, then a barrier.  Read from there (one address per
// wave: a broadcast) they cost no register between uses; held in scalar registers 2 KB doubles overflow the scalar file.
template <int KB>
__device__ __forceinline__ void stage_edge(const Edge &e, double *eR, double *eI)
{
    if ((int)threadIdx.x < KB) {
        eR[threadIdx.x] = e.R[threadIdx.x];
        eI[threadIdx.x] = e.inv[threadIdx.x];
    }
    __syncthreads();
}

__global__ __launch_bounds__(kBlock) void enclosed_centroid_kernel(Rays r, int64_t P, int W, int row0, double *__restrict__ part,
                                                                   int nbx, int R)
{
    const RowBase b = row_base(r, W, row0);
    const int64_t first = (int64_t)blockIdx.x * R * kChunk;
    const int64_t last = std::min(first + (int64_t)R * kChunk, P);
    double m[3] = {0.0, 0.0, 0.0};
    const bool vec = r.s_p == 1 && aligned_to(b.x, 16) && aligned_to(b.y, 16) && aligned_to(b.ok, 4);
    walk_rays(b.x, b.y, b.ok, r.s_p, vec, first, last, P, [&](int64_t, const auto &xs, const auto &ys, const auto &oks) {
        constexpr int N = sizeof(xs) / sizeof(xs[0]);
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const bool live = oks[j] != 0u;
            m[0] += live ? 1.0 : 0.0;
            m[1] += live ? (double)xs[j] : 0.0;
            m[2] += live ? (double)ys[j] : 0.0;
        }
    });
    block_partial(m, part, b.row, nbx, 3);
}

template <int KB, int SHAPE>
__global__ __launch_bounds__(kBlock) void enclosed_sums_kernel(Rays r, int64_t P, int W, int row0, const double *__restrict__ centre,
                                                               Edge e, int K, double *__restrict__ part, int nbx, int R)
{
#pragma clang fp contract(off)
    const RowBase b = row_base(r, W, row0);
    const double c_x = centre[2 * (int64_t)b.row], c_y = centre[2 * (int64_t)b.row + 1];
    const int64_t first = (int64_t)blockIdx.x * R * kChunk;
    const int64_t last = std::min(first + (int64_t)R * kChunk, P);
    __shared__ double eR[KB], eI[KB];
    stage_edge<KB>(e, eR, eI);
    double m[KB];
#pragma unroll
    for (int k = 0; k < KB; ++k) m[k] = 0.0;
    const bool vec = r.s_p == 1 && aligned_to(b.x, 16) && aligned_to(b.y, 16) && aligned_to(b.ok, 4);
    walk_rays(b.x, b.y, b.ok, r.s_p, vec, first, last, P, [&](int64_t, const auto &xs, const auto &ys, const auto &oks) {
        constexpr int N = sizeof(xs) / sizeof(xs[0]);
        double a[N], q[N];                                  // circle: a = rho; square: a = |dx|, q = |dy|
        bool live[N];
#pragma unroll
        for (int j = 0; j < N; ++j) {
            live[j] = oks[j] != 0u;
            // a dead ray is the ray at the origin that is not counted: nothing of what it holds reaches a sum
            const double dx = (live[j] ? (double)xs[j] : 0.0) - c_x, dy = (live[j] ? (double)ys[j] : 0.0) - c_y;
            if (SHAPE == kCircle) { a[j] = sqrt(dx * dx + dy * dy); q[j] = 0.0; }
            else { a[j] = fabs(dx); q[j] = fabs(dy); }
        }
#pragma unroll
        for (int k = 0; k < KB; ++k) {
#pragma unroll
            for (int j = 0; j < N; ++j) {
                double t = sigma(edge_t((eR[k] - a[j]) * eI[k]));
                if (SHAPE == kSquare) t = t * sigma(edge_t((eR[k] - q[j]) * eI[k]));
                m[k] += live[j] ? t : 0.0;
            }
            __builtin_amdgcn_sched_barrier(0);              // one radius per scheduling region: the loads of the next stay behind it
        }
    });
    block_partial(m, part, b.row, nbx, K);
}

__global__ __launch_bounds__(kBlock) void enclosed_reduce_kernel(const double *__restrict__ part, double *__restrict__ out,
                                                                 int64_t total, int nbx, int n)
{
    reduce_rows(part, out, total, nbx, n);
}

template <int SHAPE>
__global__ __launch_bounds__(kBlock) void enclosed_seed_kernel(Rays r, int64_t P, int W, int row0, const double *__restrict__ centre,
                                                               Edge e, int K, const double *__restrict__ g_sums,
                                                               const double *__restrict__ g_lin, float *gx_all, float *gy_all,
                                                               double *__restrict__ part, int nbx, int R)
{
#pragma clang fp contract(off)
    const RowBase b = row_base(r, W, row0);
    const double c_x = centre[2 * (int64_t)b.row], c_y = centre[2 * (int64_t)b.row + 1];
    const double l_x = g_lin ? g_lin[2 * (int64_t)b.row] : 0.0, l_y = g_lin ? g_lin[2 * (int64_t)b.row + 1] : 0.0;
    float *__restrict__ gx = gx_all ? gx_all + b.off : nullptr, *__restrict__ gy = gy_all ? gy_all + b.off : nullptr;
    __shared__ double eR[kMaxK], eI[kMaxK], g[kMaxK];       // (no register array is indexed by k here: a plain loop to K)
    if ((int)threadIdx.x < K) g[threadIdx.x] = g_sums[(int64_t)b.row * K + threadIdx.x];
    stage_edge<kMaxK>(e, eR, eI);
    const int64_t first = (int64_t)blockIdx.x * R * kChunk;
    const int64_t last = std::min(first + (int64_t)R * kChunk, P);
    double m[2] = {0.0, 0.0};                               // the centre's gradient: minus the rays' edge terms
    // (a NULL output is aligned)
    const bool vec = r.s_p == 1 && aligned_to(b.x, 16) && aligned_to(b.y, 16) && aligned_to(b.ok, 4) && aligned_to(gx, 16)
                     && aligned_to(gy, 16);
    walk_rays(b.x, b.y, b.ok, r.s_p, vec, first, last, P, [&](int64_t o, const auto &xs, const auto &ys, const auto &oks) {
        constexpr int N = sizeof(xs) / sizeof(xs[0]);
        double dx[N], dy[N], a[N], q[N], sx[N], sy[N];
        bool live[N];
#pragma unroll
        for (int j = 0; j < N; ++j) {
            live[j] = oks[j] != 0u;
            dx[j] = (live[j] ? (double)xs[j] : 0.0) - c_x;
            dy[j] = (live[j] ? (double)ys[j] : 0.0) - c_y;
            if (SHAPE == kCircle) { a[j] = sqrt(dx[j] * dx[j] + dy[j] * dy[j]); q[j] = 0.0; }
            else { a[j] = fabs(dx[j]); q[j] = fabs(dy[j]); }
            sx[j] = sy[j] = 0.0;
        }
#pragma unroll 1
        for (int k = 0; k < K; ++k) {
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const double ta = edge_t((eR[k] - a[j]) * eI[k]);
                if (SHAPE == kCircle) {
                    sx[j] += g[k] * (dsigma(ta) * eI[k]);
                } else {
                    const double tq = edge_t((eR[k] - q[j]) * eI[k]);
                    sx[j] += g[k] * (dsigma(ta) * sigma(tq) * eI[k]);
                    sy[j] += g[k] * (sigma(ta) * dsigma(tq) * eI[k]);
                }
            }
        }
        float ox[N], oy[N];
#pragma unroll
        for (int j = 0; j < N; ++j) {
            double ex, ey;                                  // d(sum_k g_k e_k) / d(x, y) of this ray
            if (SHAPE == kCircle) {
                const double s = a[j] > 0.0 ? sx[j] / a[j] : 0.0;
                ex = -(s * dx[j]);
                ey = -(s * dy[j]);
            } else {
                ex = dx[j] > 0.0 ? -sx[j] : dx[j] < 0.0 ? sx[j] : 0.0;
                ey = dy[j] > 0.0 ? -sy[j] : dy[j] < 0.0 ? sy[j] : 0.0;
            }
            m[0] -= live[j] ? ex : 0.0;
            m[1] -= live[j] ? ey : 0.0;
            ox[j] = live[j] ? (float)(ex + l_x) : 0.0f;
            oy[j] = live[j] ? (float)(ey + l_y) : 0.0f;
        }
        if constexpr (N == kVec) {
            if (gx) *reinterpret_cast<float4 *>(gx + o) = make_float4(ox[0], ox[1], ox[2], ox[3]);
            if (gy) *reinterpret_cast<float4 *>(gy + o) = make_float4(oy[0], oy[1], oy[2], oy[3]);
        } else {
            if (gx) gx[o] = ox[0];
            if (gy) gy[o] = oy[0];
        }
    });
    if (part) block_partial(m, part, b.row, nbx, 2);
}

struct Checked { int rc; Edge e; };

// the argument check the calls share; `name` opens the message
int check_rays(const char *name, int64_t F, int64_t P, int64_t W, const Rays &r, const char *missing)
{
    if (const char *what = size_fault(F, P, W)) return refuse(name, what);
    if (!r.x || !r.y || !r.ok) return refuse(name, "x, y and ok are required");
    if (missing) return refuse(name, missing);
    return TL_OK;
}

// radii and 1 / softness (host) into the kernel argument; refuses what the definition excludes
Checked check_edge(const char *name, const double *radii, const double *inv_soft, int K, int shape)
{
    Checked c = {TL_OK, {}};
    const char *what = nullptr;
    if (K < 1 || K > kMaxK) what = "K must be 1 .. 32";
    else if (shape != kCircle && shape != kSquare) what = "shape must be 0 (circle) or 1 (square)";
    else if (!radii || !inv_soft) what = "radii and inv_soft (host) are required";
    for (int k = 0; k < K && !what; ++k) {
        if (!(std::isfinite(radii[k]) && radii[k] > 0.0)) what = "every radius must be finite and positive";
        else if (!(std::isfinite(inv_soft[k]) && inv_soft[k] > 0.0)) what = "every softness must be finite and positive";
        else if (k > 0 && !(radii[k] > radii[k - 1])) what = "the radii must be strictly increasing";
        c.e.R[k] = radii[k];
        c.e.inv[k] = inv_soft[k];
    }
    if (what) c.rc = refuse(name, what);
    return c;
}

// everything before the first HIP call: rays, edge, workspace, in that order
Checked check_call(const char *name, int64_t F, int64_t P, int64_t W, const Rays &r, const char *missing, const double *radii,
                   const double *inv_soft, int K, int shape, const void *ws, size_t ws_bytes)
{
    Checked c = {check_rays(name, F, P, W, r, missing), {}};
    if (!c.rc) c = check_edge(name, radii, inv_soft, K, shape);
    if (!c.rc) c.rc = check_workspace(name, ws, ws_bytes, tl_enclosed_workspace_bytes(F, P, W, K), "tl_enclosed_workspace_bytes");
    return c;
}

int reduce(const double *part, double *out, int64_t rows, int nbx, int n, hipStream_t st)
{
    return launch_reduce(enclosed_reduce_kernel, "enclosed_reduce_kernel launch", part, out, rows, nbx, n, st);
}

template <int KB, int SHAPE>
void launch_sums(dim3 grid, hipStream_t st, const Rays &r, int64_t P, int W, int row0, const double *centre, const Edge &e, int K,
                 double *part, const Plan &pl)
{
    hipLaunchKernelGGL((enclosed_sums_kernel<KB, SHAPE>), grid, dim3(kBlock), 0, st, r, P, W, row0, centre, e, K, part, pl.nbx, pl.R);
}

template <int SHAPE>
void launch_seed(dim3 grid, hipStream_t st, const Rays &r, int64_t P, int W, int row0, const double *centre, const Edge &e, int K,
                 const double *g_sums, const double *g_lin, float *gx, float *gy, double *part, const Plan &pl)
{
    hipLaunchKernelGGL((enclosed_seed_kernel<SHAPE>), grid, dim3(kBlock), 0, st, r, P, W, row0, centre, e, K, g_sums, g_lin, gx,
                       gy, part, pl.nbx, pl.R);
}

// the launcher of the register bucket KB = 8 / 16 / 32 that holds K, for the shape
using SumsLauncher = void (*)(dim3, hipStream_t, const Rays &, int64_t, int, int, const double *, const Edge &, int, double *, const Plan &);
SumsLauncher sums_launcher(int K, int shape)
{
    const bool circle = shape == kCircle;
    if (K <= 8) return circle ? launch_sums<8, kCircle> : launch_sums<8, kSquare>;
    if (K <= 16) return circle ? launch_sums<16, kCircle> : launch_sums<16, kSquare>;
    return circle ? launch_sums<32, kCircle> : launch_sums<32, kSquare>;
}

}  // namespace

extern "C" {

size_t tl_enclosed_workspace_bytes(int64_t F, int64_t P, int64_t W, int K)
{
    if (size_fault(F, P, W) || K < 1 || K > kMaxK) return 0;
    return (size_t)(F * W) * (size_t)row_plan(F * W, P).nbx * (size_t)std::max(K, 3) * sizeof(double);
}

int tl_enclosed_centroid(int32_t device, int64_t F, int64_t P, int64_t W, const float *x, const float *y, const uint8_t *ok,
                         int64_t s_f, int64_t s_p, int64_t s_w, double *S, void *workspace, size_t workspace_bytes, void *stream)
{
    static const char *name = "tl_enclosed_centroid";
    const Rays r = {x, y, ok, s_f, s_p, s_w};
    if (const int rc = check_rays(name, F, P, W, r, S ? nullptr : "the S pointer is NULL")) return rc;
    if (const int rc = check_workspace(name, workspace, workspace_bytes, tl_enclosed_workspace_bytes(F, P, W, 1), "tl_enclosed_workspace_bytes"))
        return rc;
    if (const int rc = tl_host::use_device(device)) return rc;
    const int64_t rows = F * W;
    const Plan pl = row_plan(rows, P);
    hipStream_t st = (hipStream_t)stream;
    if (const int rc = launch_rows(rows, pl.nbx, "enclosed_centroid_kernel launch", [&](dim3 grid, int row0) {
            hipLaunchKernelGGL(enclosed_centroid_kernel, grid, dim3(kBlock), 0, st, r, P, (int)W, row0, (double *)workspace, pl.nbx, pl.R);
        }))
        return rc;
    return reduce((const double *)workspace, S, rows, pl.nbx, 3, st);
}

int tl_enclosed_sums(int32_t device, int64_t F, int64_t P, int64_t W, const float *x, const float *y, const uint8_t *ok,
                     int64_t s_f, int64_t s_p, int64_t s_w, const double *centre, const double *radii, const double *inv_soft,
                     int K, int shape, double *sums, void *workspace, size_t workspace_bytes, void *stream)
{
    const Rays r = {x, y, ok, s_f, s_p, s_w};
    const Checked c = check_call("tl_enclosed_sums", F, P, W, r, !centre ? "the centre pointer is NULL" : !sums ? "the sums pointer is NULL" : nullptr,
                                 radii, inv_soft, K, shape, workspace, workspace_bytes);
    if (c.rc) return c.rc;
    if (const int rc = tl_host::use_device(device)) return rc;
    const int64_t rows = F * W;
    const Plan pl = row_plan(rows, P);
    hipStream_t st = (hipStream_t)stream;
    if (const int rc = launch_rows(rows, pl.nbx, "enclosed_sums_kernel launch", [&](dim3 grid, int row0) {
            sums_launcher(K, shape)(grid, st, r, P, (int)W, row0, centre, c.e, K, (double *)workspace, pl);
        }))
        return rc;
    return reduce((const double *)workspace, sums, rows, pl.nbx, K, st);
}

int tl_enclosed_seed(int32_t device, int64_t F, int64_t P, int64_t W, const float *x, const float *y, const uint8_t *ok,
                     int64_t s_f, int64_t s_p, int64_t s_w, const double *centre, const double *radii, const double *inv_soft,
                     int K, int shape, const double *g_sums, const double *g_lin, float *gx, float *gy, double *g_centre,
                     void *workspace, size_t workspace_bytes, void *stream)
{
    const Rays r = {x, y, ok, s_f, s_p, s_w};
    const Checked c = check_call("tl_enclosed_seed", F, P, W, r, !centre ? "the centre pointer is NULL" : !g_sums ? "the g_sums pointer is NULL" :
                                 !gx && !gy && !g_centre ? "gx, gy and g_centre are all NULL" : nullptr, radii, inv_soft, K, shape,
                                 workspace, workspace_bytes);
    if (c.rc) return c.rc;
    if (const int rc = tl_host::use_device(device)) return rc;
    const int64_t rows = F * W;
    const Plan pl = row_plan(rows, P);
    hipStream_t st = (hipStream_t)stream;
    double *part = g_centre ? (double *)workspace : nullptr;
    if (const int rc = launch_rows(rows, pl.nbx, "enclosed_seed_kernel launch", [&](dim3 grid, int row0) {
            (shape == kCircle ? launch_seed<kCircle> : launch_seed<kSquare>)(grid, st, r, P, (int)W, row0, centre, c.e, K, g_sums, g_lin,
                                                                             gx, gy, part, pl);
        }))
        return rc;
    return g_centre ? reduce(part, g_centre, rows, pl.nbx, 2, st) : TL_OK;
}

}  // extern "C"
