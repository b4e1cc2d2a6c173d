// tl_focus.hip -- the through-focus spot moments of a traced fan and their seeds (tl_focus_moments, tl_focus_seed of
// include/tl_trace.h; metrics.focus_moments / metrics.through_focus stand on them).
//
// Behind the last surface a ray is a straight line: at a plane shifted by d it lands at (x + d u, y + d v), u = cx / cz,
// v = cy / cz.  The mean square radius of a spot is a parabola in d, and its three coefficients are second moments of
// (x, y, u, v).  Per row (f, w) the forward sums, over the LIVE rays (ok != 0 and s = 1 - cx^2 - cy^2 > 0),
//   (1, x, y, u, v, x^2, y^2, u^2, v^2, x u, y v)
// with cz = sqrt(s), u, v, every product and every sum in fp64 from the fp32 inputs: the raw second moment of y is ~4e5 times
// the variance the finish extracts from it, so fp32 products would leave nothing.  Nothing is contracted (contract(off)): a
// ray's eleven terms have the bits of the definition evaluated in any IEEE fp64 arithmetic, only the ORDER of the sums is
// this file's.
//
// FORWARD.  focus_moments_kernel: layout, plan, partials and reduce are the row frame's (tl_rows.h), with five base addresses to
// be aligned for the 16-byte path and eleven fp64 accumulators per lane: one partial of eleven doubles per block.
// SEED.  focus_seed_kernel: one lane per four rays (the same two load paths), the eleven seeds of the row read once
// (wave-uniform), everything in fp64, one rounding to fp32 at the store.  Dead rays get zeros.
#include "tl_rows.h"

namespace {

constexpr int kNF = 11;                         // moments per row

struct Rays {
    const float *x, *y, *cx, *cy;
    const uint8_t *ok;
    int64_t s_f, s_p, s_w;
};

// the eleven terms of one ray, added to m
__device__ __forceinline__ void add_ray(double (&m)[kNF], float xf, float yf, float cxf, float cyf, unsigned okb)
{
#pragma clang fp contract(off)
    const double cx = (double)cxf, cy = (double)cyf;
    const double s = 1.0 - cx * cx - cy * cy;
    const bool live = okb != 0u && s > 0.0;                 // (NaN > 0 is false)
    // a dead ray is the ray (0, 0, 0, 0) that is not counted: every term +0.0, whatever its coordinates hold
    const double cz = sqrt(live ? s : 1.0);
    const double x = live ? (double)xf : 0.0, y = live ? (double)yf : 0.0;
    const double u = (live ? cx : 0.0) / cz, v = (live ? cy : 0.0) / cz;
    m[0] += live ? 1.0 : 0.0;
    m[1] += x; m[2] += y; m[3] += u; m[4] += v;
    m[5] += x * x; m[6] += y * y; m[7] += u * u; m[8] += v * v;
    m[9] += x * u; m[10] += y * v;
}

__global__ __launch_bounds__(kBlock) void focus_moments_kernel(Rays r, int64_t P, int W, int row0, double *__restrict__ part,
                                                               int nbx, int R)
{
    const int row = row0 + (int)blockIdx.y;
    const int f = row / W, w = row - f * W;
    const int64_t off = f * r.s_f + w * r.s_w;
    const float *__restrict__ x = r.x + off, *__restrict__ y = r.y + off, *__restrict__ cx = r.cx + off, *__restrict__ cy = r.cy + off;
    const uint8_t *__restrict__ ok = r.ok + off;
    const int64_t first = (int64_t)blockIdx.x * R * kChunk;
    const int64_t last = std::min(first + (int64_t)R * kChunk, P);
    double m[kNF];
#pragma unroll
    for (int j = 0; j < kNF; ++j) m[j] = 0.0;
    const bool vec = r.s_p == 1 && aligned_to(x, 16) && aligned_to(y, 16) && aligned_to(cx, 16) && aligned_to(cy, 16) && aligned_to(ok, 4);
    if (vec) {                                              // (uniform over the block)
        for (int64_t ip = first + kVec * (int64_t)threadIdx.x; ip < last; ip += kChunk) {
            if (ip + kVec <= P) {
                const float4 x4 = *reinterpret_cast<const float4 *>(x + ip), y4 = *reinterpret_cast<const float4 *>(y + ip);
                const float4 cx4 = *reinterpret_cast<const float4 *>(cx + ip), cy4 = *reinterpret_cast<const float4 *>(cy + ip);
                const unsigned o4 = *reinterpret_cast<const unsigned *>(ok + ip);
                add_ray(m, x4.x, y4.x, cx4.x, cy4.x, o4 & 0xffu);
                add_ray(m, x4.y, y4.y, cx4.y, cy4.y, o4 & 0xff00u);
                add_ray(m, x4.z, y4.z, cx4.z, cy4.z, o4 & 0xff0000u);
                add_ray(m, x4.w, y4.w, cx4.w, cy4.w, o4 & 0xff000000u);
            } else {                                        // the last one to three rays of the row
                for (int64_t q = ip; q < P; ++q) add_ray(m, x[q], y[q], cx[q], cy[q], ok[q]);
            }
        }
    } else {
        for (int64_t ip = first + threadIdx.x; ip < last; ip += kBlock) {
            const int64_t o = ip * r.s_p;
            add_ray(m, x[o], y[o], cx[o], cy[o], ok[o]);
        }
    }
    block_partial(m, part, row, nbx, kNF);
}

// (kNF as a literal: the division by it folds)
__global__ __launch_bounds__(kBlock) void focus_reduce_kernel(const double *__restrict__ part, double *__restrict__ moments,
                                                              int64_t total, int nbx)
{
    reduce_rows(part, moments, total, nbx, kNF);
}

struct Seeds { float *gx, *gy, *gcx, *gcy; };

__device__ __forceinline__ void seed_ray(const double (&g)[kNF], float xf, float yf, float cxf, float cyf, unsigned okb,
                                         float &ox, float &oy, float &ocx, float &ocy)
{
#pragma clang fp contract(off)
    const double cx = (double)cxf, cy = (double)cyf;
    const double cx2 = cx * cx, cy2 = cy * cy;
    const double s = 1.0 - cx2 - cy2;
    ox = oy = ocx = ocy = 0.0f;
    if (okb != 0u && s > 0.0) {
        const double x = (double)xf, y = (double)yf;
        const double cz = sqrt(s);
        const double u = cx / cz, v = cy / cz;
        const double gu = g[3] + 2.0 * u * g[7] + x * g[9];
        const double gv = g[4] + 2.0 * v * g[8] + y * g[10];
        const double cz3 = cz * cz * cz, cxy = cx * cy;
        ox = (float)(g[1] + 2.0 * x * g[5] + u * g[9]);
        oy = (float)(g[2] + 2.0 * y * g[6] + v * g[10]);
        ocx = (float)((gu * (1.0 - cy2) + gv * cxy) / cz3);
        ocy = (float)((gu * cxy + gv * (1.0 - cx2)) / cz3);
    }
}

__global__ __launch_bounds__(kBlock) void focus_seed_kernel(Rays r, int64_t P, int W, int row0, const double *__restrict__ gmom,
                                                            Seeds out)
{
    const int row = row0 + (int)blockIdx.y;
    const int f = row / W, w = row - f * W;
    const int64_t off = f * r.s_f + w * r.s_w;
    const float *__restrict__ x = r.x + off, *__restrict__ y = r.y + off, *__restrict__ cx = r.cx + off, *__restrict__ cy = r.cy + off;
    const uint8_t *__restrict__ ok = r.ok + off;
    float *__restrict__ gx = out.gx ? out.gx + off : nullptr, *__restrict__ gy = out.gy ? out.gy + off : nullptr;
    float *__restrict__ gcx = out.gcx ? out.gcx + off : nullptr, *__restrict__ gcy = out.gcy ? out.gcy + off : nullptr;
    double g[kNF];
#pragma unroll
    for (int j = 0; j < kNF; ++j) g[j] = gmom[(int64_t)row * kNF + j];
    const int64_t first = (int64_t)blockIdx.x * kChunk;
    // (a NULL output is aligned)
    const bool vec = r.s_p == 1 && aligned_to(x, 16) && aligned_to(y, 16) && aligned_to(cx, 16) && aligned_to(cy, 16) && aligned_to(ok, 4)
                     && aligned_to(gx, 16) && aligned_to(gy, 16) && aligned_to(gcx, 16) && aligned_to(gcy, 16);
    const int64_t ip = first + kVec * (int64_t)threadIdx.x;
    if (vec && ip + kVec <= P) {
        const float4 x4 = *reinterpret_cast<const float4 *>(x + ip), y4 = *reinterpret_cast<const float4 *>(y + ip);
        const float4 cx4 = *reinterpret_cast<const float4 *>(cx + ip), cy4 = *reinterpret_cast<const float4 *>(cy + ip);
        const unsigned o4 = *reinterpret_cast<const unsigned *>(ok + ip);
        float4 a, b, c, d;
        seed_ray(g, x4.x, y4.x, cx4.x, cy4.x, o4 & 0xffu, a.x, b.x, c.x, d.x);
        seed_ray(g, x4.y, y4.y, cx4.y, cy4.y, o4 & 0xff00u, a.y, b.y, c.y, d.y);
        seed_ray(g, x4.z, y4.z, cx4.z, cy4.z, o4 & 0xff0000u, a.z, b.z, c.z, d.z);
        seed_ray(g, x4.w, y4.w, cx4.w, cy4.w, o4 & 0xff000000u, a.w, b.w, c.w, d.w);
        if (gx) *reinterpret_cast<float4 *>(gx + ip) = a;
        if (gy) *reinterpret_cast<float4 *>(gy + ip) = b;
        if (gcx) *reinterpret_cast<float4 *>(gcx + ip) = c;
        if (gcy) *reinterpret_cast<float4 *>(gcy + ip) = d;
        return;
    }
    // one ray at a time: the whole row on the strided path (lanes along the rays), the last one to three on the aligned one
    for (int j = 0; j < kVec; ++j) {
        const int64_t q = vec ? ip + j : first + (int64_t)j * kBlock + threadIdx.x;
        if (q >= P) continue;
        const int64_t o = q * r.s_p;
        float a, b, c, d;
        seed_ray(g, x[o], y[o], cx[o], cy[o], ok[o], a, b, c, d);
        if (gx) gx[o] = a;
        if (gy) gy[o] = b;
        if (gcx) gcx[o] = c;
        if (gcy) gcy[o] = d;
    }
}

// the argument check both calls share; `name` opens the message
int check_rays(const char *name, int64_t F, int64_t P, int64_t W, const Rays &r, const void *moments)
{
    if (const char *what = size_fault(F, P, W)) return refuse(name, what);
    if (!r.x || !r.y || !r.cx || !r.cy || !r.ok) return refuse(name, "x, y, cx, cy and ok are required");
    if (!moments) return refuse(name, "the moments pointer is NULL");
    return TL_OK;
}

}  // namespace

extern "C" {

size_t tl_focus_workspace_bytes(int64_t F, int64_t P, int64_t W)
{
    if (size_fault(F, P, W)) return 0;
    return (size_t)(F * W) * (size_t)row_plan(F * W, P).nbx * kNF * sizeof(double);
}

int tl_focus_moments(int32_t device, int64_t F, int64_t P, int64_t W, const float *x, const float *y, const float *cx,
                     const float *cy, const uint8_t *ok, int64_t s_f, int64_t s_p, int64_t s_w, double *moments,
                     void *workspace, size_t workspace_bytes, void *stream)
{
    static const char *name = "tl_focus_moments";
    const Rays r = {x, y, cx, cy, ok, s_f, s_p, s_w};
    if (const int rc = check_rays(name, F, P, W, r, moments)) return rc;
    if (const int rc = check_workspace(name, workspace, workspace_bytes, tl_focus_workspace_bytes(F, P, W), "tl_focus_workspace_bytes"))
        return rc;
    if (const int rc = tl_host::use_device(device)) return rc;
    const int64_t rows = F * W;
    const Plan pl = row_plan(rows, P);
    hipStream_t st = (hipStream_t)stream;
    if (const int rc = launch_rows(rows, pl.nbx, "focus_moments_kernel launch", [&](dim3 grid, int row0) {
            hipLaunchKernelGGL(focus_moments_kernel, grid, dim3(kBlock), 0, st, r, P, (int)W, row0, (double *)workspace, pl.nbx, pl.R);
        }))
        return rc;
    hipLaunchKernelGGL(focus_reduce_kernel, dim3((unsigned)cdiv(rows * kNF, kBlock)), dim3(kBlock), 0, st, (const double *)workspace,
                       moments, rows * kNF, pl.nbx);
    return tl_host::launched("focus_reduce_kernel launch");
}

int tl_focus_seed(int32_t device, int64_t F, int64_t P, int64_t W, const float *x, const float *y, const float *cx,
                  const float *cy, const uint8_t *ok, int64_t s_f, int64_t s_p, int64_t s_w, const double *g_moments,
                  float *gx, float *gy, float *gcx, float *gcy, void *stream)
{
    const Rays r = {x, y, cx, cy, ok, s_f, s_p, s_w};
    if (const int rc = check_rays("tl_focus_seed", F, P, W, r, g_moments)) return rc;
    if (!gx && !gy && !gcx && !gcy) return refuse("tl_focus_seed", "gx, gy, gcx and gcy are all NULL");
    if (const int rc = tl_host::use_device(device)) return rc;
    const Seeds out = {gx, gy, gcx, gcy};
    return launch_rows(F * W, cdiv(P, kChunk), "focus_seed_kernel launch", [&](dim3 grid, int row0) {
        hipLaunchKernelGGL(focus_seed_kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, r, P, (int)W, row0, g_moments, out);
    });
}

}  // extern "C"
