// tl_warp.hip -- bicubic resampling of an image at per-pixel source coordinates, and its gradients to the coordinates and
// the gain (tl_warp_fwd, tl_warp_bwd of include/tl_trace.h; imaging.warp_bicubic(fused=True) stands on them).
//
//   xc = clamp(x, -1, 1),  u = (xc + 1) / 2 (W - 1),  j0 = floor(u),  t = u - j0,  columns clip(j0 - 1 .. j0 + 2, 0, W - 1)
//   rows likewise from y and H;   out[b,yo,xo,c] = gain  sum_i sum_j wy_i wx_j image[b, row_i, col_j, c]
//
// with the cubic convolution weights of alpha = -0.75 (Horner form in axis_taps below).  A latency-bound gather with trivial
// arithmetic: one lane per output pixel, lanes along xo (pixel index = yo Wo + xo over the whole output, so a narrow output
// still fills its waves), the lens index in grid y.  The four row and four column offsets and the eight weights are computed
// once per pixel; the channels are a loop inside the lane (16 loads in flight per lane, never 16 x C); no LDS, no workspace.
//
// ADDRESSING.  floor(u) is converted to an integer (0 when u is NaN: the conversion of a NaN is never executed), then all
// four integer indices per axis, j0 included, are clipped into [0, n - 1], and the image is addressed only through those
// clipped integers.  So no coordinate value -- infinities and NaN included -- can form an address outside the image.  The
// clamp is written with comparisons, which a NaN fails: a NaN coordinate stays NaN through u and t, makes all eight weights
// NaN and with them this pixel's output and this pixel's gradients, and nothing else.
//
// Backward: one launch gives g_x, g_y and (when asked) g_gain.  It recomputes offsets, weights and derivative weights and
// gathers the same 16 taps; it needs g_out, the image, the coordinates and the gain, not the forward output.  Every sum it
// needs -- over the channels, over the lenses when coordinates or gain are shared by the batch, over the channels of a
// [..,1] gain -- is taken inside one lane in a fixed order, b outer and c inner: no atomics, no workspace, the same bits on
// every run.  With nothing shared the lens index is grid y; otherwise the lane loops over the lenses.  A gain shared by the
// batch but not by the channels keeps its C running sums in g_gain itself (the lane that owns the pixel stores, then reads,
// adds and stores its own element again: program order, one lane, no other writer).
//
// The gradient to the image is a scatter: tl_warp_bwd_image at the end of this file, with its own contract (64-bit fixed-point
// integer atomics on a scale taken from the data, so the same bits in any order).
#include "tl_common.h"

#include <limits.h>

#include <stdio.h>

#include <algorithm>

namespace {

constexpr int kBlock = 256;
constexpr int kMaxY = 65535;                    // lenses per launch (grid y)
constexpr int kMaxEdge = 1 << 20;               // H, W, Ho, Wo
constexpr float kA = -0.75f;                    // the reference's alpha

struct Geo {
    int B, H, W, C, Ho, Wo, cb, gb, gc;
    int64_t im_s[4], x_s[3], y_s[3], gn_s[4], gx_s[3], gy_s[3], gg_s[4];
};

// One axis of one pixel: element offsets of the four taps, weights, derivative weights (d/du), and whether the clamp passes
// the gradient (-1 <= x <= 1, torch's convention; true for NaN, whose gradient is NaN anyway).
// Roundings: xc + 1 and the product with (n - 1)/2 (exact for n <= 2^24) are the only two in u; t = u - floor(u) is exact.
// Each cubic is a Horner form of three steps (<= 6 roundings, 3 with contraction), each derivative one of two steps (<= 4).
__device__ __forceinline__ void axis_taps(const float x, const int n, const int64_t stride, int64_t off[4], float w[4], float dw[4],
                                          bool &pass)
{
    const float xc = x < -1.f ? -1.f : (x > 1.f ? 1.f : x);                    // NaN fails both comparisons and stays
    const float u = (xc + 1.f) * (0.5f * (float)(n - 1));
    const float fl = floorf(u);
    const float t = u - fl;
    const int j0 = (u == u) ? (int)fl : 0;                                     // u is in [0, n - 1] or NaN
#pragma unroll
    for (int k = 0; k < 4; ++k) off[k] = (int64_t)min(max(j0 - 1 + k, 0), n - 1) * stride;
    const float tt = t * t;
    w[0] = ((kA * t - 2.f * kA) * t + kA) * t;
    w[1] = ((kA + 2.f) * t - (kA + 3.f)) * tt + 1.f;
    w[2] = ((-(kA + 2.f) * t + (2.f * kA + 3.f)) * t - kA) * t;
    w[3] = (kA - kA * t) * tt;
    dw[0] = (3.f * kA * t - 4.f * kA) * t + kA;
    dw[1] = (3.f * (kA + 2.f) * t - 2.f * (kA + 3.f)) * t;
    dw[2] = (-3.f * (kA + 2.f) * t + 2.f * (2.f * kA + 3.f)) * t - kA;
    dw[3] = (-3.f * kA * t + 2.f * kA) * t;
    pass = !(x < -1.f) && !(x > 1.f);
}

// grid (ceil(Ho Wo / 256), lenses of this launch)
__global__ __launch_bounds__(kBlock) void warp_fwd_kernel(const Geo g, const float *__restrict__ image, const float *__restrict__ x,
                                                          const float *__restrict__ y, const float *__restrict__ gain,
                                                          float *__restrict__ out, const int b0)
{
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= (int64_t)g.Ho * g.Wo) return;
    const int yo = (int)(p / g.Wo), xo = (int)(p - (int64_t)yo * g.Wo);
    const int b = b0 + blockIdx.y, bc = g.cb == 1 ? 0 : b;
    int64_t ro[4], co[4];
    float wy[4], wx[4], dwy[4], dwx[4];
    bool pass;
    axis_taps(x[(int64_t)bc * g.x_s[0] + (int64_t)yo * g.x_s[1] + (int64_t)xo * g.x_s[2]], g.W, g.im_s[2], co, wx, dwx, pass);
    axis_taps(y[(int64_t)bc * g.y_s[0] + (int64_t)yo * g.y_s[1] + (int64_t)xo * g.y_s[2]], g.H, g.im_s[1], ro, wy, dwy, pass);
    const float *__restrict__ im = image + (int64_t)b * g.im_s[0];
    const float *__restrict__ gp = gain ? gain + (int64_t)(g.gb == 1 ? 0 : b) * g.gn_s[0] + (int64_t)yo * g.gn_s[1]
                                                 + (int64_t)xo * g.gn_s[2] : nullptr;
    const int64_t gcs = g.gc == 1 ? 0 : g.gn_s[3];
    float *__restrict__ o = out + (((size_t)b * g.Ho + yo) * g.Wo + xo) * g.C;
#pragma unroll 1
    for (int c = 0; c < g.C; ++c) {
        const float *__restrict__ q = im + (int64_t)c * g.im_s[3];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float *__restrict__ r = q + ro[i];
            float row = wx[0] * r[co[0]];
            row = __builtin_fmaf(wx[1], r[co[1]], row);
            row = __builtin_fmaf(wx[2], r[co[2]], row);
            row = __builtin_fmaf(wx[3], r[co[3]], row);
            s = i == 0 ? wy[0] * row : __builtin_fmaf(wy[i], row, s);
        }
        if (gp) s *= gp[(int64_t)c * gcs];
        o[c] = s;
    }
}

// grid (ceil(Ho Wo / 256), lenses of this launch), or (.., 1) with nb = B when the lane loops over the lenses
__global__ __launch_bounds__(kBlock) void warp_bwd_kernel(const Geo g, const float *__restrict__ image, const float *__restrict__ x,
                                                          const float *__restrict__ y, const float *__restrict__ gain,
                                                          const float *__restrict__ g_out, float *__restrict__ g_x,
                                                          float *__restrict__ g_y, float *__restrict__ g_gain, const int b0,
                                                          const int nb)
{
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= (int64_t)g.Ho * g.Wo) return;
    const int yo = (int)(p / g.Wo), xo = (int)(p - (int64_t)yo * g.Wo);
    const int first = b0 + (nb == 1 ? (int)blockIdx.y : 0);
    const float fx = 0.5f * (float)(g.W - 1), fy = 0.5f * (float)(g.H - 1);
    const int64_t x_at = (int64_t)yo * g.x_s[1] + (int64_t)xo * g.x_s[2], y_at = (int64_t)yo * g.y_s[1] + (int64_t)xo * g.y_s[2];
    const int64_t gx_at = (int64_t)yo * g.gx_s[1] + (int64_t)xo * g.gx_s[2], gy_at = (int64_t)yo * g.gy_s[1] + (int64_t)xo * g.gy_s[2];
    const int64_t gn_at = (int64_t)yo * g.gn_s[1] + (int64_t)xo * g.gn_s[2], gg_at = (int64_t)yo * g.gg_s[1] + (int64_t)xo * g.gg_s[2];
    const int64_t gcs = g.gc == 1 ? 0 : g.gn_s[3];
    int64_t ro[4], co[4];
    float wy[4], wx[4], dwy[4], dwx[4];
    bool pass_x = false, pass_y = false;
    float gx = 0.f, gy = 0.f, gsum = 0.f;
    for (int b = first; b < first + nb; ++b) {
        if (b == first || g.cb != 1) {
            const int64_t bc = g.cb == 1 ? 0 : b;
            axis_taps(x[bc * g.x_s[0] + x_at], g.W, g.im_s[2], co, wx, dwx, pass_x);
            axis_taps(y[bc * g.y_s[0] + y_at], g.H, g.im_s[1], ro, wy, dwy, pass_y);
            gx = gy = 0.f;
        }
        if (g.gb != 1) gsum = 0.f;
        const float *__restrict__ im = image + (int64_t)b * g.im_s[0];
        const float *__restrict__ go = g_out + (((size_t)b * g.Ho + yo) * g.Wo + xo) * g.C;
        const float *__restrict__ gp = gain ? gain + (int64_t)(g.gb == 1 ? 0 : b) * g.gn_s[0] + gn_at : nullptr;
        float *gg = g_gain ? g_gain + (int64_t)(g.gb == 1 ? 0 : b) * g.gg_s[0] + gg_at : nullptr;   // (not restrict: read back)
#pragma unroll 1
        for (int c = 0; c < g.C; ++c) {
            const float *__restrict__ q = im + (int64_t)c * g.im_s[3];
            float s = 0.f, sx = 0.f, sy = 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float *__restrict__ r = q + ro[i];
                const float v0 = r[co[0]], v1 = r[co[1]], v2 = r[co[2]], v3 = r[co[3]];
                float row = wx[0] * v0, drow = dwx[0] * v0;
                row = __builtin_fmaf(wx[1], v1, row);
                drow = __builtin_fmaf(dwx[1], v1, drow);
                row = __builtin_fmaf(wx[2], v2, row);
                drow = __builtin_fmaf(dwx[2], v2, drow);
                row = __builtin_fmaf(wx[3], v3, row);
                drow = __builtin_fmaf(dwx[3], v3, drow);
                s = i == 0 ? wy[0] * row : __builtin_fmaf(wy[i], row, s);
                sx = i == 0 ? wy[0] * drow : __builtin_fmaf(wy[i], drow, sx);
                sy = i == 0 ? dwy[0] * row : __builtin_fmaf(dwy[i], row, sy);
            }
            const float gv = go[c];
            const float a = gp ? gv * gp[(int64_t)c * gcs] : gv;
            gx = __builtin_fmaf(a, sx, gx);
            gy = __builtin_fmaf(a, sy, gy);
            if (gg) {
                if (g.gc == 1) {
                    gsum = __builtin_fmaf(gv, s, gsum);
                } else {
                    float *at = gg + (int64_t)c * g.gg_s[3];
                    float v = gv * s;
                    if (g.gb == 1 && b != first) v += *at;
                    *at = v;
                }
            }
        }
        if (gg && g.gc == 1 && (g.gb != 1 || b == first + nb - 1)) *gg = gsum;
        if (g_x && (g.cb != 1 || b == first + nb - 1)) {
            const int64_t bc = g.cb == 1 ? 0 : b;
            g_x[bc * g.gx_s[0] + gx_at] = pass_x ? gx * fx : 0.f;
            g_y[bc * g.gy_s[0] + gy_at] = pass_y ? gy * fy : 0.f;
        }
    }
}

// ------------------------------------------------------------------------------------------------ the gradient to the image
//
//   g_image[b,r,q,c] = sum over output pixels and taps (i,j) with (row_i, col_j) = (r,q) of wy_i wx_j a,   a = g_out gain
//
// A scatter: many output pixels add into one source pixel.  Float atomics would make the sum depend on the arrival order.
// Integer addition is associative, so every contribution is converted to a 64-bit fixed-point integer on ONE scale for the
// whole call and added with plain integer atomics: the same bits in any order, grouping, launch plan and run.
//
// THE SCALE.  m = the largest finite |a| of the call (a as the fp32 product g_out gain; pre-pass, integer atomicMax on the
// bit pattern, which orders non-negative floats); E with 2^(E-1) <= m < 2^E; Hb = ceil(log2(16 Ho Wo)); the quantum is
// Q = 2^(E + Hb - 62).  Ho Wo <= 2^26, so Hb <= 30 and Q <= 2^(E-32): the error is ABSOLUTE, on the scale of the largest
// seed, at least 2^-32 of it; it is not relative per pixel.
// ONE CONTRIBUTION.  The fp32 product (wy_i wx_j) a, times 1/Q in fp64 (a power of two: exact), rounded to the nearest int64.
// NO OVERFLOW.  |wy wx| <= 1 and |a| < 2^E, so |contribution| <= 2^(62-Hb); at most 16 Ho Wo <= 2^Hb contributions reach one
// address (16 taps of every output pixel of one lens), so |sum| <= 2^62.  (The fp32 Horner forms can exceed 1 by an ulp
// next to t = 0 or 1; the spare bit between 2^62 and 2^63 holds that with room to spare.)  The LDS box below holds partial
// sums of the same contributions, so the same bound holds there.
// THE RESULT.  fp32(sum Q), rounded once (the int64 is narrowed with a sticky bit first, so the conversion through fp64 does
// not round twice).  A source pixel that no tap reaches is +0.0; m = 0 or no finite a gives zeros.
// NON-FINITE.  A non-finite a, or a NaN coordinate (NaN weights; taps = the clipped indices around j0 = 0, as in axis_taps),
// is left out of m and of the sums and sets the bit of its destination element in a flag plane instead; a flagged element
// comes out NaN, every other element keeps the bits of the clean run.
//
// WORKSPACE (tl_warp_bwd_image_work_bytes): [0, 256) word 0 = the bits of m | int64 accumulators, PLANAR [B,C,H,W], so that
// neighbouring columns of one channel are neighbouring 8-byte words | one flag bit per element of g_image in its own
// (channel-last) order.  Cleared by warp_image_clear_kernel at the head of the call -- a kernel, not hipMemsetAsync: recorded
// into a HIP graph, the memset node cleared the region on the graph's first launch only and filled it with its own 64-bit
// destination address on every later one (tests/test_gpu_steps_graph.py: the second replay of a captured warp step).
//
// SCATTER KERNEL.  One lane per output pixel, a block owns a tile of 32 x 8 output pixels (lanes along xo), the lens in
// grid y.  Taps and weights are axis_taps' (with stride 1 the offsets are the clipped indices).  Privatised in LDS: the block
// takes a box origin from its smallest clipped row and column (LDS atomicMin: block-uniform); contributions that land in
// the 16 x 48 source box at that origin are added in LDS (6 KiB: occupancy is not limited by it), the others go straight to
// the global accumulator; after a barrier the block adds its non-zero box entries to global memory, consecutive lanes on
// consecutive columns of a row.  The channels loop through the same box.  For a smooth map of magnification near 1 this
// replaces 16 global atomics per pixel and channel by about 1.7; for an arbitrary map everything takes the direct path.
// flags bit 0 skips the box altogether (the A/B switch; the same contributions, so the same bits).
constexpr int kTileX = 32, kTileY = 8;          // kTileX kTileY = kBlock
constexpr int kBoxH = 16, kBoxW = 48;
constexpr int64_t kMaxPixels = (int64_t)1 << 26;
constexpr int64_t kMaxElements = (int64_t)1 << 40;
constexpr size_t kWorkHead = 256;
constexpr unsigned kInfBits = 0x7f800000u;
static_assert(kTileX * kTileY == kBlock, "one lane per output pixel of the tile");

typedef unsigned long long u64;

// k with Q = 2^k, from the bits of m (> 0, finite)
__device__ __forceinline__ int quantum_exponent(const unsigned mbits, const int Hb)
{
    const int e = (int)(mbits >> 23);
    const int E = e ? e - 126 : (32 - __clz((int)mbits)) - 149;       // subnormal m: highest set bit p, 2^(p-149) <= m < 2^(p-148)
    return E + Hb - 62;
}

__device__ __forceinline__ double pow2(const int k) { return __longlong_as_double((long long)(k + 1023) << 52); }   // |k| < 1023

// grid-stride over the 8-byte words of the workspace: the clear at the head of tl_warp_bwd_image
__global__ __launch_bounds__(kBlock) void warp_image_clear_kernel(u64 *__restrict__ work, const int64_t words)
{
    for (int64_t at = (int64_t)blockIdx.x * kBlock + threadIdx.x; at < words; at += (int64_t)gridDim.x * kBlock) work[at] = 0;
}

// grid-stride over the B Ho Wo output pixels of the call; one atomic per block at the most
__global__ __launch_bounds__(kBlock) void warp_image_max_kernel(const Geo g, const float *__restrict__ gain,
                                                                const float *__restrict__ g_out, unsigned *__restrict__ m, const int64_t n)
{
    __shared__ unsigned wave_best[kBlock / 64];
    const int64_t pixels = (int64_t)g.Ho * g.Wo;
    const int64_t gcs = g.gc == 1 ? 0 : g.gn_s[3];
    unsigned best = 0;
    for (int64_t at = (int64_t)blockIdx.x * kBlock + threadIdx.x; at < n; at += (int64_t)gridDim.x * kBlock) {
        const int64_t b = at / pixels, p = at - b * pixels;
        const int yo = (int)(p / g.Wo), xo = (int)(p - (int64_t)yo * g.Wo);
        const float *__restrict__ go = g_out + at * g.C;
        const float *__restrict__ gp = gain ? gain + (g.gb == 1 ? 0 : b) * g.gn_s[0] + (int64_t)yo * g.gn_s[1] + (int64_t)xo * g.gn_s[2]
                                            : nullptr;
        for (int c = 0; c < g.C; ++c) {
            const float a = gp ? go[c] * gp[(int64_t)c * gcs] : go[c];
            const unsigned bits = __float_as_uint(a) & 0x7fffffffu;
            if (bits < kInfBits) best = max(best, bits);
        }
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) best = max(best, (unsigned)__shfl_xor((int)best, off));
    if ((threadIdx.x & 63) == 0) wave_best[threadIdx.x / 64] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 1; k < kBlock / 64; ++k) best = max(best, wave_best[k]);
        // one word for the whole call: a block adds its atomic only when it would raise the word it sees (a stale view costs
        // an atomic, never the maximum), so the traffic to that one address dies out as m settles
        if (best > __hip_atomic_load(m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(m, best);
    }
}

// grid (tiles of 32 x 8 output pixels, lenses of this launch)
__global__ __launch_bounds__(kBlock) void warp_image_scatter_kernel(const Geo g, const float *__restrict__ x, const float *__restrict__ y,
                                                                    const float *__restrict__ gain, const float *__restrict__ g_out,
                                                                    const unsigned *__restrict__ m, u64 *__restrict__ acc,
                                                                    unsigned *__restrict__ flags, const int Hb, const int direct,
                                                                    const int b0)
{
    __shared__ u64 box[kBoxH * kBoxW];
    __shared__ int origin[2];
    const unsigned mbits = *m;
    const double inv_q = mbits ? pow2(-quantum_exponent(mbits, Hb)) : 0.0;      // m = 0: every finite contribution is 0
    const int tiles_x = (g.Wo + kTileX - 1) / kTileX;
    const int ty = (int)(blockIdx.x / tiles_x), tx = (int)(blockIdx.x - (unsigned)ty * tiles_x);
    const int xo = tx * kTileX + (threadIdx.x & (kTileX - 1)), yo = ty * kTileY + (threadIdx.x / kTileX);
    const bool active = xo < g.Wo && yo < g.Ho;
    const int b = b0 + blockIdx.y, bc = g.cb == 1 ? 0 : b;
    int64_t ri[4] = {0, 0, 0, 0}, ci[4] = {0, 0, 0, 0};
    float wy[4], wx[4], dw[4], w[16];
    bool pass, w_finite = false;
    if (active) {
        axis_taps(x[(int64_t)bc * g.x_s[0] + (int64_t)yo * g.x_s[1] + (int64_t)xo * g.x_s[2]], g.W, 1, ci, wx, dw, pass);
        axis_taps(y[(int64_t)bc * g.y_s[0] + (int64_t)yo * g.y_s[1] + (int64_t)xo * g.y_s[2]], g.H, 1, ri, wy, dw, pass);
        w_finite = wx[0] == wx[0] && wy[0] == wy[0];      // a NaN coordinate makes all four weights of its axis NaN
#pragma unroll
        for (int k = 0; k < 16; ++k) w[k] = wy[k / 4] * wx[k % 4];
    }
    int r0 = 0, c0 = 0;
    if (!direct) {
        if (threadIdx.x == 0) origin[0] = origin[1] = INT_MAX;
        for (int e = threadIdx.x; e < kBoxH * kBoxW; e += kBlock) box[e] = 0;
        __syncthreads();
        if (active) {                                  // tap 0 is the smallest clipped index of the pixel
            atomicMin(&origin[0], (int)ri[0]);
            atomicMin(&origin[1], (int)ci[0]);
        }
        __syncthreads();
        r0 = origin[0];
        c0 = origin[1];
    }
    // per tap row / column: its place in the box (rows as multiples of the box width), or -1 when it is outside; and the
    // row's offset in a plane of the global accumulator.  Only clipped indices (0 <= r < H, 0 <= q < W) enter any of them.
    int box_r[4], box_c[4];
    int64_t row_at[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int dr = (int)ri[k] - r0, dc = (int)ci[k] - c0;                       // >= 0: the origin is the smallest
        box_r[k] = !direct && (unsigned)dr < (unsigned)kBoxH ? dr * kBoxW : -1;
        box_c[k] = !direct && (unsigned)dc < (unsigned)kBoxW ? dc : -1;
        row_at[k] = ri[k] * g.W;
    }
    const float *__restrict__ go = g_out + (((size_t)b * g.Ho + yo) * g.Wo + xo) * g.C;               // read only when active
    const float *__restrict__ gp = gain ? gain + (int64_t)(g.gb == 1 ? 0 : b) * g.gn_s[0] + (int64_t)yo * g.gn_s[1]
                                                 + (int64_t)xo * g.gn_s[2] : nullptr;
    const int64_t gcs = g.gc == 1 ? 0 : g.gn_s[3];
    const int64_t plane_size = (int64_t)g.H * g.W;
#pragma unroll 1
    for (int c = 0; c < g.C; ++c) {
        u64 *__restrict__ plane = acc + ((int64_t)b * g.C + c) * plane_size;
        if (active) {
            const float a = gp ? go[c] * gp[(int64_t)c * gcs] : go[c];
            if (w_finite && (__float_as_uint(a) & 0x7fffffffu) < kInfBits) {
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    const int i = k / 4, j = k % 4;
                    const long long v = __double2ll_rn((double)(w[k] * a) * inv_q);
                    if ((box_r[i] | box_c[j]) >= 0) atomicAdd(&box[box_r[i] + box_c[j]], (u64)v);     // both inside the box
                    else if (v != 0) atomicAdd(&plane[row_at[i] + ci[j]], (u64)v);
                }
            } else {                                   // non-finite: mark the 16 destination elements, add nothing
                for (int k = 0; k < 16; ++k) {
                    const int64_t e = (((int64_t)b * plane_size + row_at[k / 4] + ci[k % 4]) * g.C) + c;
                    atomicOr(&flags[e >> 5], 1u << (unsigned)(e & 31));
                }
            }
        }
        if (!direct) {
            __syncthreads();
            for (int e = threadIdx.x; e < kBoxH * kBoxW; e += kBlock) {          // consecutive lanes: consecutive columns of a row
                const u64 v = box[e];
                if (v == 0) continue;
                box[e] = 0;
                const int r = r0 + e / kBoxW, q = c0 + e % kBoxW;
                if (r < g.H && q < g.W) atomicAdd(&plane[(int64_t)r * g.W + q], v);
            }
            __syncthreads();
        }
    }
}

// grid-stride over the n = B H W C elements of g_image
__global__ __launch_bounds__(kBlock) void warp_image_final_kernel(const Geo g, const unsigned *__restrict__ m, const u64 *__restrict__ acc,
                                                                  const unsigned *__restrict__ flags, float *__restrict__ g_image,
                                                                  const int Hb, const int64_t n)
{
    const unsigned mbits = *m;
    const double q2048 = mbits ? pow2(quantum_exponent(mbits, Hb) + 11) : 0.0;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < n; e += (int64_t)gridDim.x * kBlock) {
        int64_t t = e / g.C;
        const int c = (int)(e - t * g.C);
        const int q = (int)(t % g.W);
        t /= g.W;
        const int r = (int)(t % g.H);
        const int64_t b = t / g.H;
        const long long s = (long long)acc[((b * g.C + c) * g.H + r) * g.W + q];
        // 53 bits and a sticky bit (round to odd): the two conversions below then round sum Q once, to fp32
        const long long hi = (s >> 11) | (long long)((s & 0x7ff) != 0);
        float v = s == 0 ? 0.f : (float)((double)hi * q2048);
        if ((flags[e >> 5] >> (unsigned)(e & 31)) & 1u) v = __uint_as_float(0x7fc00000u);
        g_image[e] = v;
    }
}

int64_t image_elements(const tl_warp_geom *g) { return (int64_t)g->B * g->H * g->W * g->C; }   // after the size checks only

bool image_sizes_ok(const tl_warp_geom *g)
{
    if (g->B < 1 || g->H < 1 || g->W < 1 || g->C < 1 || g->H > kMaxEdge || g->W > kMaxEdge) return false;
    return (int64_t)g->H * g->W <= kMaxElements && (int64_t)g->B * g->C <= kMaxElements / ((int64_t)g->H * g->W);
}

size_t image_work_bytes(const int64_t n)
{
    const size_t raw = kWorkHead + (size_t)n * sizeof(u64) + (size_t)((n + 31) / 32) * sizeof(unsigned);
    return (raw + 255) / 256 * 256;
}

// Everything that can be refused without a HIP call.
int check_geom(const char *fn, const tl_warp_geom *g, bool has_gain)
{
    static thread_local char msg[256];
    const char *what = nullptr;
    if (!g) what = "g is NULL";
    else if (g->B < 1 || g->H < 1 || g->W < 1 || g->C < 1 || g->Ho < 1 || g->Wo < 1)
        what = "B, H, W, C, Ho, Wo must be >= 1";
    else if (g->H > kMaxEdge || g->W > kMaxEdge || g->Ho > kMaxEdge || g->Wo > kMaxEdge)
        what = "H, W, Ho, Wo must be <= 2^20";
    else if ((int64_t)g->Ho * g->Wo > 0x7fffffff) what = "Ho Wo must be < 2^31";
    else if (g->coord_batch != 1 && g->coord_batch != g->B) what = "coord_batch must be 1 or B";
    else if (has_gain && g->gain_batch != 1 && g->gain_batch != g->B) what = "gain_batch must be 1 or B";
    else if (has_gain && g->gain_channels != 1 && g->gain_channels != g->C) what = "gain_channels must be 1 or C";
    if (!what) return TL_OK;
    snprintf(msg, sizeof(msg), "%s: %s", fn, what);
    return tl_host::fail(TL_EINVAL, msg);
}

Geo make_geo(const tl_warp_geom *g)
{
    Geo q;
    q.B = g->B; q.H = g->H; q.W = g->W; q.C = g->C; q.Ho = g->Ho; q.Wo = g->Wo;
    q.cb = g->coord_batch; q.gb = g->gain_batch; q.gc = g->gain_channels;
    for (int k = 0; k < 4; ++k) { q.im_s[k] = g->image_stride[k]; q.gn_s[k] = g->gain_stride[k]; q.gg_s[k] = g->g_gain_stride[k]; }
    for (int k = 0; k < 3; ++k) {
        q.x_s[k] = g->x_stride[k]; q.y_s[k] = g->y_stride[k]; q.gx_s[k] = g->g_x_stride[k]; q.gy_s[k] = g->g_y_stride[k];
    }
    return q;
}

}  // namespace

extern "C" {

int tl_warp_fwd(const tl_warp_geom *g, const float *image, const float *x, const float *y, const float *gain, float *out,
                void *stream)
{
    const int rc = check_geom("tl_warp_fwd", g, gain != nullptr);
    if (rc) return rc;
    if (!image) return tl_host::fail(TL_EINVAL, "tl_warp_fwd: image is NULL");
    if (!x || !y) return tl_host::fail(TL_EINVAL, "tl_warp_fwd: x or y is NULL");
    if (!out) return tl_host::fail(TL_EINVAL, "tl_warp_fwd: out is NULL");
    if (const int rc = tl_host::use_device(g->device)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const Geo q = make_geo(g);
    const unsigned blocks = (unsigned)(((int64_t)g->Ho * g->Wo + kBlock - 1) / kBlock);
    for (int b0 = 0; b0 < g->B; b0 += kMaxY) {
        hipLaunchKernelGGL(warp_fwd_kernel, dim3(blocks, std::min(kMaxY, g->B - b0)), dim3(kBlock), 0, st, q, image, x, y, gain, out, b0);
        if (const int rc = tl_host::launched("warp_fwd_kernel launch")) return rc;
    }
    return TL_OK;
}

int tl_warp_bwd(const tl_warp_geom *g, const float *image, const float *x, const float *y, const float *gain, const float *g_out,
                float *g_x, float *g_y, float *g_gain, void *stream)
{
    const int rc = check_geom("tl_warp_bwd", g, gain != nullptr);
    if (rc) return rc;
    if (!image) return tl_host::fail(TL_EINVAL, "tl_warp_bwd: image is NULL");
    if (!x || !y) return tl_host::fail(TL_EINVAL, "tl_warp_bwd: x or y is NULL");
    if (!g_out) return tl_host::fail(TL_EINVAL, "tl_warp_bwd: g_out is NULL");
    if ((g_x == nullptr) != (g_y == nullptr)) return tl_host::fail(TL_EINVAL, "tl_warp_bwd: g_x and g_y go together, one of them is NULL");
    if (!g_x && !g_gain) return tl_host::fail(TL_EINVAL, "tl_warp_bwd: g_x, g_y and g_gain are all NULL: nothing to compute");
    if (g_gain && !gain) return tl_host::fail(TL_EINVAL, "tl_warp_bwd: g_gain is asked for but gain is NULL");
    if (const int rc = tl_host::use_device(g->device)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const Geo q = make_geo(g);
    const unsigned blocks = (unsigned)(((int64_t)g->Ho * g->Wo + kBlock - 1) / kBlock);
    const bool in_lane = g->B > 1 && ((g_x && g->coord_batch == 1) || (g_gain && g->gain_batch == 1));
    if (in_lane) {                                  // something is shared by the batch: the lane sums over the lenses
        hipLaunchKernelGGL(warp_bwd_kernel, dim3(blocks, 1), dim3(kBlock), 0, st, q, image, x, y, gain, g_out, g_x, g_y, g_gain, 0, g->B);
        return tl_host::launched("warp_bwd_kernel launch");
    }
    for (int b0 = 0; b0 < g->B; b0 += kMaxY) {
        hipLaunchKernelGGL(warp_bwd_kernel, dim3(blocks, std::min(kMaxY, g->B - b0)), dim3(kBlock), 0, st, q, image, x, y, gain, g_out,
                           g_x, g_y, g_gain, b0, 1);
        if (const int rc = tl_host::launched("warp_bwd_kernel launch")) return rc;
    }
    return TL_OK;
}

size_t tl_warp_bwd_image_work_bytes(const tl_warp_geom *g)
{
    return g && image_sizes_ok(g) ? image_work_bytes(image_elements(g)) : 0;
}

int tl_warp_bwd_image(const tl_warp_geom *g, const float *x, const float *y, const float *gain, const float *g_out, float *g_image,
                      void *work, size_t work_bytes, int flags, void *stream)
{
    const int rc = check_geom("tl_warp_bwd_image", g, gain != nullptr);
    if (rc) return rc;
    if (!x || !y) return tl_host::fail(TL_EINVAL, "tl_warp_bwd_image: x or y is NULL");
    if (!g_out) return tl_host::fail(TL_EINVAL, "tl_warp_bwd_image: g_out is NULL");
    if (!g_image) return tl_host::fail(TL_EINVAL, "tl_warp_bwd_image: g_image is NULL");
    if ((int64_t)g->Ho * g->Wo > kMaxPixels)
        return tl_host::fail(TL_EINVAL, "tl_warp_bwd_image: Ho Wo must be <= 2^26 (the headroom of the 64-bit accumulators)");
    if (!image_sizes_ok(g)) return tl_host::fail(TL_EINVAL, "tl_warp_bwd_image: B H W C must be <= 2^40");
    if (flags & ~1) return tl_host::fail(TL_EINVAL, "tl_warp_bwd_image: flags has bits other than bit 0 (direct atomics) set");
    const int64_t n = image_elements(g);
    const size_t need = image_work_bytes(n);
    if (!work) return tl_host::fail(TL_EINVAL, "tl_warp_bwd_image: work is NULL");
    if ((uintptr_t)work % 8) return tl_host::fail(TL_EINVAL, "tl_warp_bwd_image: work must be aligned to 8 bytes");
    if (work_bytes < need) {
        static thread_local char msg[160];
        snprintf(msg, sizeof(msg), "tl_warp_bwd_image: work_bytes is %zu, tl_warp_bwd_image_work_bytes asks for %zu", work_bytes, need);
        return tl_host::fail(TL_EINVAL, msg);
    }
    if (const int rc = tl_host::use_device(g->device)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const Geo q = make_geo(g);
    unsigned *m = (unsigned *)work;
    u64 *acc = (u64 *)((char *)work + kWorkHead);
    unsigned *marks = (unsigned *)(acc + n);
    const int64_t pixels = (int64_t)g->Ho * g->Wo;
    int Hb = 0;                                          // ceil(log2(16 Ho Wo)), in integers
    while (((int64_t)1 << Hb) < 16 * pixels) ++Hb;
    const int64_t words = (int64_t)(need / sizeof(u64));             // need is a multiple of 256, work is aligned to 8 bytes
    const unsigned cblocks = (unsigned)std::min<int64_t>((words + kBlock - 1) / kBlock, (int64_t)1 << 16);
    hipLaunchKernelGGL(warp_image_clear_kernel, dim3(cblocks), dim3(kBlock), 0, st, (u64 *)work, words);
    if (const int rc = tl_host::launched("warp_image_clear_kernel launch")) return rc;
    const unsigned tiles = (unsigned)((g->Wo + kTileX - 1) / kTileX) * (unsigned)((g->Ho + kTileY - 1) / kTileY);
    const int64_t all = (int64_t)g->B * pixels;                       // <= 2^31 2^26
    const unsigned mblocks = (unsigned)std::min<int64_t>((all + kBlock - 1) / kBlock, 2048);
    hipLaunchKernelGGL(warp_image_max_kernel, dim3(mblocks), dim3(kBlock), 0, st, q, gain, g_out, m, all);
    if (const int rc = tl_host::launched("warp_image_max_kernel launch")) return rc;
    for (int b0 = 0; b0 < g->B; b0 += kMaxY) {
        hipLaunchKernelGGL(warp_image_scatter_kernel, dim3(tiles, std::min(kMaxY, g->B - b0)), dim3(kBlock), 0, st, q, x, y, gain, g_out,
                           m, acc, marks, Hb, flags & 1, b0);
        if (const int rc = tl_host::launched("warp_image_scatter_kernel launch")) return rc;
    }
    const unsigned fblocks = (unsigned)std::min<int64_t>((n + kBlock - 1) / kBlock, (int64_t)1 << 20);
    hipLaunchKernelGGL(warp_image_final_kernel, dim3(fblocks), dim3(kBlock), 0, st, q, m, acc, marks, g_image, Hb, n);
    return tl_host::launched("warp_image_final_kernel launch");
}

}  // extern "C"
