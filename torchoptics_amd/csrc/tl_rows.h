// tl_rows.h -- the row frame of the spot merits: tl_focus.hip, tl_enclosed.hip, tl_zfit.hip, tl_mtf.hip and tl_tfmtf.hip include
// it, nothing else does.  Each of them sums per-ray terms over the rays of a ROW (one field f and wavelength w of the F x W the call holds)
// in fp64; what a ray's terms are is the unit's, everything around them is defined here, once.
//
// LAYOUT AND PLAN.  A ray array is read at f s_f + i s_p + w s_w (elements).  Grid (nbx, rows of this launch), 256 lanes; rows
// beyond 65535 go in further launches (grid y), back to back on the stream.  Block bx of a row takes the rays
// [bx R 1024, (bx + 1) R 1024): where the ray stride is 1 and the row's base addresses are aligned a lane takes four consecutive
// rays with 16-byte loads (ok as one dword) and strides by 1024, otherwise one ray at a time, striding by 256; the last one to
// three rays of an aligned row go one at a time.  row_plan aims at ~2048 blocks (8 per CU) whatever the size, so the partials stay
// far below a byte per ray.  Each lane keeps its running sums in a static register array.
// PARTIALS AND REDUCE.  A butterfly over the wave, the four waves added in order through LDS, one partial per block in the
// workspace (block_partial); the unit's *_reduce_kernel then adds a row's nbx partials in order (reduce_rows).  No atomics: the
// same bits on every run, and a sum's bits depend on nothing but its row's rays and the plan.
// HOST.  The checks refuse with "<entry point>: <what>" before the first HIP call; sizes first, then what the unit adds, the
// workspace last.
#pragma once
#include "tl_common.h"

#include <stdio.h>

#include <algorithm>

namespace {

constexpr int kBlock = 256;
constexpr int kVec = 4;                         // rays per lane and load on the aligned path
constexpr int kChunk = kBlock * kVec;           // rays a block takes per step: the unit of the plan
constexpr int kMaxY = 65535;                    // rows per launch (grid y)
constexpr int64_t kTargetBlocks = 2048;         // 256 CUs x 8 blocks of 4 waves
constexpr int64_t kMaxDim = ((int64_t)1 << 31) - 1;

struct Plan { int nbx, R; };                    // blocks per row, steps of kChunk rays per block

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

Plan row_plan(int64_t rows, int64_t P)
{
    const int64_t chunks = cdiv(P, kChunk);
    const int64_t want = std::max<int64_t>(1, cdiv(kTargetBlocks, rows));
    const int64_t R = cdiv(chunks, std::min(chunks, want));
    return {(int)cdiv(chunks, R), (int)R};
}

// ---------------------------------------------------------------------------------------------------------------- the device
__device__ __forceinline__ bool aligned_to(const void *p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1u)) == 0; }

// the row of this block and where its (x, y, ok) rays start; Rays: the unit's kernel argument {x, y, ok, s_f, s_p, s_w, ..}
struct RowBase {
    const float *x, *y;
    const uint8_t *ok;
    int64_t off;
    int row;
};

template <class Rays>
__device__ __forceinline__ RowBase row_base(const Rays &r, int W, int row0)
{
    const int row = row0 + (int)blockIdx.y;
    const int f = row / W, w = row - f * W;
    const int64_t off = f * r.s_f + w * r.s_w;
    return {r.x + off, r.y + off, r.ok + off, off, row};
}

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

// the same for a unit that reads the direction cosines too: Rays {x, y, cx, cy, ok, s_f, s_p, s_w, ..}
struct RowBase5 {
    const float *x, *y, *cx, *cy;
    const uint8_t *ok;
    int64_t off;
    int row;
};

template <class Rays>
__device__ __forceinline__ RowBase5 row_base5(const Rays &r, int W, int row0)
{
    const int row = row0 + (int)blockIdx.y;
    const int f = row / W, w = row - f * W;
    const int64_t off = f * r.s_f + w * r.s_w;
    return {r.x + off, r.y + off, r.cx + off, r.cy + off, r.ok + off, off, row};
}

// whether the row's five bases take the 16-byte path (s_p == 1 is the caller's to add)
__device__ __forceinline__ bool aligned_row(const RowBase5 &b)
{
    return aligned_to(b.x, 16) && aligned_to(b.y, 16) && aligned_to(b.cx, 16) && aligned_to(b.cy, 16) && aligned_to(b.ok, 4);
}

// walk_rays over five arrays: body(o, xs, ys, cxs, cys, oks), the same rays to the same lanes in the same order
template <class Body>
__device__ __forceinline__ void walk_rays5(const RowBase5 &b, int64_t s_p, bool vec, int64_t first, int64_t last, int64_t P, Body &&body)
{
    const float *__restrict__ x = b.x, *__restrict__ y = b.y, *__restrict__ cx = b.cx, *__restrict__ cy = b.cy;
    const uint8_t *__restrict__ ok = b.ok;
    if (vec) {                                              // (uniform over the block)
        for (int64_t ip = first + kVec * (int64_t)threadIdx.x; ip < last; ip += kChunk) {
            if (ip + kVec <= P) {
                const float4 x4 = *reinterpret_cast<const float4 *>(x + ip), y4 = *reinterpret_cast<const float4 *>(y + ip);
                const float4 c4 = *reinterpret_cast<const float4 *>(cx + ip), d4 = *reinterpret_cast<const float4 *>(cy + ip);
                const unsigned o4 = *reinterpret_cast<const unsigned *>(ok + ip);
                const float xs[kVec] = {x4.x, x4.y, x4.z, x4.w}, ys[kVec] = {y4.x, y4.y, y4.z, y4.w};
                const float cxs[kVec] = {c4.x, c4.y, c4.z, c4.w}, cys[kVec] = {d4.x, d4.y, d4.z, d4.w};
                const unsigned oks[kVec] = {o4 & 0xffu, o4 & 0xff00u, o4 & 0xff0000u, o4 & 0xff000000u};
                body(ip, xs, ys, cxs, cys, oks);
            } else {                                        // the last one to three rays of the row
                for (int64_t q = ip; q < P; ++q) {
                    const float xs[1] = {x[q]}, ys[1] = {y[q]}, cxs[1] = {cx[q]}, cys[1] = {cy[q]};
                    const unsigned oks[1] = {ok[q]};
                    body(q, xs, ys, cxs, cys, oks);
                }
            }
        }
    } else {
        for (int64_t ip = first + threadIdx.x; ip < last; ip += kBlock) {
            const int64_t o = ip * s_p;
            const float xs[1] = {x[o]}, ys[1] = {y[o]}, cxs[1] = {cx[o]}, cys[1] = {cy[o]};
            const unsigned oks[1] = {ok[o]};
            body(o, xs, ys, cxs, cys, oks);
        }
    }
}

// part[(row nbx + bx) stride + base + j] = the block's sum of m[j], j < n <= N: a butterfly over the wave, the four waves in
// order.  stride: the doubles a block's partial holds, of which this call stores n from `base` on.
template <int N>
__device__ __forceinline__ void block_partial(const double (&m)[N], double *__restrict__ part, int row, int nbx, int n, int stride,
                                              int base)
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
        part[((int64_t)row * nbx + blockIdx.x) * stride + base + threadIdx.x] = s;
    }
}

template <int N>
__device__ __forceinline__ void block_partial(const double (&m)[N], double *__restrict__ part, int row, int nbx, int n)
{
    block_partial(m, part, row, nbx, n, n, 0);
}

// out[row][j] = the row's nbx partials of n doubles added in order: the body of every unit's *_reduce_kernel
__device__ __forceinline__ void reduce_rows(const double *__restrict__ part, double *__restrict__ out, int64_t total, int nbx, int n)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= total) return;
    const int64_t row = i / n;
    const double *p = part + row * nbx * n + (i - row * n);
    double s = 0.0;
    for (int b = 0; b < nbx; ++b) s += p[(int64_t)b * n];
    out[i] = s;
}

// the same ordered sum for one slot of partials that hold `stride` doubles per block (a unit whose output is not laid out as its
// partials are maps an output element to its slot and calls this)
__device__ __forceinline__ double reduce_slot(const double *__restrict__ part, int64_t row, int nbx, int stride, int slot)
{
    const double *p = part + row * nbx * stride + slot;
    double s = 0.0;
    for (int b = 0; b < nbx; ++b) s += p[(int64_t)b * stride];
    return s;
}

// ------------------------------------------------------------------------------------------------------------------ the host
// what is wrong with the sizes, or nullptr: the *_workspace_bytes answer 0 where the checks refuse
inline const char *size_fault(int64_t F, int64_t P, int64_t W)
{
    if (F < 1 || P < 1 || W < 1) return "F, P and W must be at least 1";
    if (F > kMaxDim || W > kMaxDim || F * W > kMaxDim || P > kMaxDim) return "F W and P must stay below 2^31";
    return nullptr;
}

// the refusal "<name>: <what>" as the calling thread's message; returns code
int refuse(const char *name, const char *what, int code = TL_EINVAL)
{
    char msg[200];                                          // (fail copies it)
    snprintf(msg, sizeof msg, "%s: %s", name, what);
    return tl_host::fail(code, msg);
}

// `sizer`: the name of the unit's tl_*_workspace_bytes, which gave `need`
int check_workspace(const char *name, const void *ws, size_t bytes, size_t need, const char *sizer)
{
    if (ws && bytes >= need) return TL_OK;
    char what[80];
    snprintf(what, sizeof what, "workspace NULL or below %s", sizer);
    return refuse(name, what, TL_EWORKSPACE);
}

// launch(grid, row0) for every kMaxY rows, grid = (nbx, rows of the launch); `what` names the launch in a HIP error
template <class Launch>
int launch_rows(int64_t rows, int64_t nbx, const char *what, Launch &&launch)
{
    for (int64_t row0 = 0; row0 < rows; row0 += kMaxY) {
        launch(dim3((unsigned)nbx, (unsigned)std::min<int64_t>(kMaxY, rows - row0)), (int)row0);
        if (const int rc = tl_host::launched(what)) return rc;
    }
    return TL_OK;
}

using ReduceKernel = void (*)(const double *, double *, int64_t, int, int);

int launch_reduce(ReduceKernel kernel, const char *what, const double *part, double *out, int64_t rows, int nbx, int n, hipStream_t st)
{
    const int64_t total = rows * n;
    hipLaunchKernelGGL(kernel, dim3((unsigned)cdiv(total, kBlock)), dim3(kBlock), 0, st, part, out, total, nbx, n);
    return tl_host::launched(what);
}

}  // namespace
