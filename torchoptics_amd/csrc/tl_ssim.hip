// tl_ssim.hip -- the structural similarity of two images under a separable Gaussian window, per lens, and its gradients to both
// images (tl_ssim_fwd, tl_ssim_bwd of include/tl_trace.h; imaging.ssim(fused=True) stands on them), and the multi-scale pyramid
// of it (tl_ms_ssim_fwd, tl_ms_ssim_bwd; imaging.ms_ssim(fused=True)).
//
// LAYOUT.  The kernels come first: ssim_fwd_kernel<K, Q> and ssim_bwd_kernel<K, MS> serve both pairs of entry points, the finish,
// pooling and pyramid-finish kernels one each.  Below them ONE host path: both public geometries are read into one description
// (Desc; `pyramid` marks the multi-scale calls, the single scale is not a pyramid of one level), over which stand one fault
// function, one maker of a level's Geo, one buffer check and, per direction, one helper that cuts B into launches, dispatches
// on K and checks each launch.  The four entry points differ in what they check and in the levels they walk, not in how they launch.
//
//   mu_a = w*a,  mu_b = w*b,  va = w*a^2 - mu_a^2,  vb = w*b^2 - mu_b^2,  cab = w*ab - mu_a mu_b      (valid window, w (x) w)
//   S = (2 mu_a mu_b + C1)(2 cab + C2) / ((mu_a^2 + mu_b^2 + C1)(va + vb + C2)),   ssim[b] = mean of S over Hm x Wm x C
//
// FORWARD.  One workgroup of 256 lanes per tile of 32 x 16 map pixels per lens.  The channels go in chunks of up to 4: per
// chunk the tile plus its K - 1 halo of a and b (at most 42 x 26 pixels) is loaded into LDS, the lanes running along each
// row's (pixel, channel) span -- for a dense channels-last image that is one contiguous run of memory, so C = 3 coalesces
// like C = 4 -- with all of a three-channel chunk's loads of both images in flight at once, and stored PLANAR per channel
// (plane pitch = 12 mod 32 banks, so the three or four channels of neighbouring pixels that one store instruction carries
// fall on different banks).  Then per channel, with register blocking along the filter in both passes (K + 1 values give TWO outputs) and every LDS read 8 bytes
// wide (ds_read_b64: twice the bytes per LDS cycle of a 4-byte read):
//   horizontal pass   lane (row r, column pair x, x + 1): the five window sums of a', b', a'^2, b'^2, a'b' along the row from
//                     K + 1 consecutive values of each raw plane, into five planes stored TRANSPOSED, [x][r] with a pitch of
//                     26 (the stores of a wave fall two to a bank, which a 4-byte store hides);
//   vertical pass     lane (column x, row pair): the five sums down the column from K + 1 consecutive values of the
//                     transposed plane (lanes 26 words apart: 26 l mod 64 are 32 different even banks, no conflict), then S
//                     and the partial maps of the two pixels.
// CENTRING.  a' = a - a0, b' = b - b0 with a0, b0 the tile's first pixel of that image and channel.  Variances and the
// covariance do not change under a shift, and w*a'^2 - (w*a')^2 no longer subtracts two numbers of size mu^2 to get one of
// size C2 = 9e-4 L^2: on a smooth or flat image a' is small against a.  The means get the constant back, mu_a = a0 + w*a'.
// PARTIAL MAPS (each dense channels-last [B,Hm,Wm,C], written only when its pointer is given; unscaled, so the forward does
// not depend on the seed):  ds = dS/d va = dS/d vb = -S / (va + vb + C2) (stored once per wanted side),
// dc = dS/d cab = 2 (2 mu_a mu_b + C1) / (B1 B2),  dm_a = dS/d mu_a - 2 mu_a ds - mu_b dc (raw second moments held fixed).
// REDUCTION.  Each lane adds its S values in fp64 (channels outer, its two rows inner), the wave adds by a butterfly, lane 0
// of the block adds the four waves in order: one double per (lens, tile) in the workspace.  ssim_finish_kernel adds the
// tiles of a lens in fp64, strided over 256 lanes and then by a tree: every order is fixed, there is no atomic anywhere, so
// the result has the same bits on every run.
//
// BACKWARD (once per image that needs a gradient, the caller swaps the roles):
//   g_p[b,y,x,c] = g[b] / (Hm Wm C) sum_{i,j} w_i w_j (dm + 2 p[y,x] ds + q[y,x] dc)[y - i, x - j]    (0 outside the map)
// One workgroup per tile of 32 x 16 INPUT pixels: the three maps over the tile plus halo go to LDS the same way (zero outside
// the map: the full correlation), the same two passes run over the three of them, and the lane combines with its own p and q
// read straight from memory.  A gather in a fixed order: no atomics, no workspace, the same bits on every run.
#include "tl_common.h"

#include <stdio.h>

#include <algorithm>

namespace {

constexpr int kBlock = 256;
constexpr int kMaxY = 65535;                    // lenses per launch (grid y)
constexpr int kMaxEdge = 1 << 20;               // H, W
constexpr int kMaxK = 11;
constexpr int kTX = 32, kTY = 16;               // tile: lanes along x, two rows per lane in the vertical pass
constexpr int kHX = kTX + kMaxK - 1;            // 42: pitch of a raw row
constexpr int kHY = kTY + kMaxK - 1;            // 26
constexpr int kPlane = 1100;                    // >= kHX kHY = 1092, = 12 mod 32, even (8-byte reads of row pairs)
constexpr int kCh = 4;                          // channels per chunk
constexpr int kHPlane = kHY * kTX;              // one plane of the horizontal pass, stored TRANSPOSED: [x][r], pitch kHY
constexpr int64_t kMaxTiles = (int64_t)1 << 22;
static_assert(kPlane >= kHX * kHY && kPlane % 32 == 12, "raw plane pitch");
static_assert(kHX % 2 == 0 && kHY % 2 == 0 && kPlane % 2 == 0 && kHPlane % 2 == 0 && kMaxK % 2 == 1, "float2 reads are aligned");
static_assert(kTX * kTY == 2 * kBlock, "two map rows per lane");

// K + 1 consecutive floats from an 8-byte aligned LDS address, as (K + 1) / 2 eight-byte reads
template <int K>
__device__ __forceinline__ void read_run(const float *__restrict__ at, float out[K + 1])
{
    const float2 *__restrict__ p = reinterpret_cast<const float2 *>(at);
#pragma unroll
    for (int k = 0; k < (K + 1) / 2; ++k) {
        const float2 t = p[k];
        out[2 * k] = t.x;
        out[2 * k + 1] = t.y;
    }
}

struct Geo {
    int B, H, W, C, Hm, Wm, tiles_x;
    float w[kMaxK], C1, C2;
    int64_t a_s[4], b_s[4], g_s[4];
};

__host__ __device__ constexpr int fwd_lds_floats(int nch) { return 2 * nch * kPlane + 5 * kHPlane + 8; }
__host__ __device__ constexpr int bwd_lds_floats(int nch) { return 3 * nch * kPlane + 3 * kHPlane; }
static_assert(fwd_lds_floats(kCh) * 4 <= 65536 && bwd_lds_floats(kCh) * 4 <= 65536, "LDS per workgroup stays below 64 KiB");

// The lanes of the block run along the (row, pixel, channel) elements of the tile plus halo, nc channels from c0:
// plane[c][r][x] = src(oy + r, ox + x, c0 + c), or 0 where that lies outside the source (ox, oy may be negative in the
// backward; limit_y / limit_x bound the source).  Consecutive lanes take consecutive (pixel, channel) of a row, which is
// consecutive memory in a dense channels-last source.  N sources of one geometry go together (the two images; the three maps):
// N kLoads loads per lane are issued before the first is stored, so their latencies overlap -- the whole chunk of a
// three-channel tile is one round trip to memory.  The two divisions are multiplies: e / span is exact while e span < 2^24
// (e < 26 span, span <= 168) and the product stays below 2^32; j / nc is exact for j < 168, nc <= 4.
constexpr int kLoads = 13;
struct Source {
    const float *p;                                 // at (lens, 0, 0, 0)
    int64_t s_y, s_x, s_c;
};
template <int N>
__device__ __forceinline__ void load_planes(float *__restrict__ planes, const int plane_step, const Source (&src)[N], const int oy,
                                            const int ox, const int rows, const int cols, const int limit_y, const int limit_x,
                                            const int c0, const int nc)
{
    const int span = cols * nc, total = rows * span;
    const unsigned inv_nc = 65536u / (unsigned)nc + 1u, inv_span = (1u << 24) / (unsigned)span + 1u;
    for (int e0 = threadIdx.x; e0 < total; e0 += kBlock * kLoads) {
        float v[N][kLoads];
        int at[kLoads];
#pragma unroll
        for (int u = 0; u < kLoads; ++u) {
            const int e = e0 + u * kBlock;
            at[u] = -1;
#pragma unroll
            for (int n = 0; n < N; ++n) v[n][u] = 0.f;
            if (e < total) {
                const int r = (int)(((unsigned)e * inv_span) >> 24), j = e - r * span;
                const int x = (int)(((unsigned)j * inv_nc) >> 16), c = j - x * nc;
                const int y = oy + r, sx = ox + x;
                at[u] = c * kPlane + r * kHX + x;
                if (y >= 0 && y < limit_y && sx >= 0 && sx < limit_x) {
#pragma unroll
                    for (int n = 0; n < N; ++n)
                        v[n][u] = src[n].p[(int64_t)y * src[n].s_y + (int64_t)sx * src[n].s_x + (int64_t)(c0 + c) * src[n].s_c];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kLoads; ++u)
            if (at[u] >= 0) {
#pragma unroll
                for (int n = 0; n < N; ++n) planes[n * plane_step + at[u]] = v[n][u];
            }
    }
}

// What the forward sums.  kSsimAll: S over the map and all channels, one partial per (lens, tile) -- tl_ssim_fwd.  The two
// others are the terms of the multi-scale pyramid, one partial per (lens, tile, CHANNEL): kCsChan the contrast-structure
// factor CS = (2 cab + C2) / (va + vb + C2), whose partial maps are ds = -CS / B2, dc = 2 / B2, dm_p = -2 mu_p ds - mu_q dc
// (CS does not depend on the means otherwise), kSsimChan S itself.  A NULL ds_a / ds_b is skipped (the pyramid keeps ds once).
enum Quantity { kSsimAll = 0, kCsChan = 1, kSsimChan = 2 };

// grid (tiles of the map, lenses of this launch); dynamic LDS = fwd_lds_floats(min(C, 4)) floats
template <int K, int Q>
__global__ __launch_bounds__(kBlock) void ssim_fwd_kernel(const Geo g, const float *__restrict__ a, const float *__restrict__ b,
                                                          float *__restrict__ dm_a, float *__restrict__ ds_a, float *__restrict__ dm_b,
                                                          float *__restrict__ ds_b, float *__restrict__ dc, double *__restrict__ part,
                                                          const int b0)
{
    extern __shared__ __align__(16) float lds[];
    const int nch = min(g.C, kCh);
    float *raw_a = lds, *raw_b = lds + nch * kPlane, *hbuf = lds + 2 * nch * kPlane;
    double *wave_sum = (double *)(hbuf + 5 * kHPlane);                       // 4 doubles; the offset is a multiple of 8 bytes
    const int ty = (int)blockIdx.x / g.tiles_x, tx = (int)blockIdx.x - ty * g.tiles_x;
    const int y0 = ty * kTY, x0 = tx * kTX;
    const int th = min(kTY, g.Hm - y0), tw = min(kTX, g.Wm - x0);              // map pixels of this tile
    const int rows = th + K - 1, cols = tw + K - 1;                            // input pixels: all inside the image
    const int lens = b0 + blockIdx.y;
    const Source images[2] = {{a + (int64_t)lens * g.a_s[0], g.a_s[1], g.a_s[2], g.a_s[3]},
                              {b + (int64_t)lens * g.b_s[0], g.b_s[1], g.b_s[2], g.b_s[3]}};
    const int vx = threadIdx.x & (kTX - 1), vy = (threadIdx.x / kTX) * 2;      // vertical pass: column, first of two rows
    float w[K];
#pragma unroll
    for (int k = 0; k < K; ++k) w[k] = g.w[k];
    double acc = 0.0;
    for (int c0 = 0; c0 < g.C; c0 += kCh) {
        const int nc = min(kCh, g.C - c0);
        __syncthreads();                                                       // the last chunk's readers are done
        load_planes<2>(raw_a, nch * kPlane, images, y0, x0, rows, cols, g.H, g.W, c0, nc);      // raw_b = raw_a + nch kPlane
        __syncthreads();
        for (int c = 0; c < nc; ++c) {
            const float *__restrict__ pa = raw_a + c * kPlane, *__restrict__ pb = raw_b + c * kPlane;
            const float a0 = pa[0], b0v = pb[0];                               // the centring constants (a broadcast read)
            // a lane takes a row r and the column PAIR x, x + 1 (x even): K + 1 values of each image in 8-byte reads.  Columns
            // up to x + K <= 41 stay inside the raw row; what lies beyond the tile's own columns only reaches column x + 1
            // >= tw of the result, which nobody reads.
            for (int it = threadIdx.x; it < rows * (kTX / 2); it += kBlock) {
                const int r = it / (kTX / 2), x = (it & (kTX / 2 - 1)) * 2;
                if (x >= tw) continue;
                float av[K + 1], bv[K + 1];
                read_run<K>(pa + r * kHX + x, av);
                read_run<K>(pb + r * kHX + x, bv);
#pragma unroll
                for (int k = 0; k <= K; ++k) {
                    av[k] -= a0;
                    bv[k] -= b0v;
                }
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    float sa = 0.f, sb = 0.f, saa = 0.f, sbb = 0.f, sab = 0.f;
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        const float wa = w[k] * av[k + half], wb = w[k] * bv[k + half];
                        sa += wa;
                        sb += wb;
                        saa = __builtin_fmaf(wa, av[k + half], saa);
                        sbb = __builtin_fmaf(wb, bv[k + half], sbb);
                        sab = __builtin_fmaf(wa, bv[k + half], sab);
                    }
                    float *__restrict__ h = hbuf + (x + half) * kHY + r;
                    h[0] = sa;
                    h[kHPlane] = sb;
                    h[2 * kHPlane] = saa;
                    h[3 * kHPlane] = sbb;
                    h[4 * kHPlane] = sab;
                }
            }
            __syncthreads();
            if (vx < tw && vy < th) {
                float s0[5], s1[5];
#pragma unroll
                for (int m = 0; m < 5; ++m) {
                    float v[K + 1];
                    read_run<K>(hbuf + m * kHPlane + vx * kHY + vy, v);        // rows vy .. vy + K <= 25 of column vx (vy is even)
                    float u0 = 0.f, u1 = 0.f;
#pragma unroll
                    for (int k = 0; k <= K; ++k) {
                        if (k < K) u0 = __builtin_fmaf(w[k], v[k], u0);
                        if (k > 0) u1 = __builtin_fmaf(w[k - 1], v[k], u1);
                    }
                    s0[m] = u0;
                    s1[m] = u1;
                }
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    if (vy + half >= th) break;                               // the second row of an odd tile: sums of stale rows, dropped
                    const float *s = half ? s1 : s0;
                    const float ma = s[0], mb = s[1];                          // centred means
                    const float va = s[2] - ma * ma, vb = s[3] - mb * mb, cab = s[4] - ma * mb;
                    const float mua = a0 + ma, mub = b0v + mb;
                    const float A1 = 2.f * mua * mub + g.C1, A2 = 2.f * cab + g.C2;
                    const float B1 = mua * mua + mub * mub + g.C1, B2 = va + vb + g.C2;
                    const float rB1 = 1.f / B1, rB2 = 1.f / B2;
                    if constexpr (Q == kCsChan) {
                        const float V = A2 * rB2;
                        acc += (double)V;
                        if (dc) {
                            const size_t at = (((size_t)lens * g.Hm + (y0 + vy + half)) * g.Wm + (x0 + vx)) * g.C + (c0 + c);
                            const float ds = -V * rB2;
                            const float dcv = 2.f * rB2;
                            dc[at] = dcv;
                            if (ds_a) ds_a[at] = ds;
                            if (ds_b) ds_b[at] = ds;
                            if (dm_a) dm_a[at] = -2.f * mua * ds - mub * dcv;
                            if (dm_b) dm_b[at] = -2.f * mub * ds - mua * dcv;
                        }
                        continue;
                    }
                    const float S = (A1 * A2) * (rB1 * rB2);
                    acc += (double)S;
                    if (dc) {
                        const size_t at = (((size_t)lens * g.Hm + (y0 + vy + half)) * g.Wm + (x0 + vx)) * g.C + (c0 + c);
                        const float ds = -S * rB2;
                        const float dcv = 2.f * A1 * (rB1 * rB2);
                        const float t = 2.f * A2 * (rB1 * rB2);                // dS/d mu_a = t mu_b - 2 mu_a S / B1
                        const float u = 2.f * S * rB1;
                        dc[at] = dcv;
                        if (dm_a) {
                            dm_a[at] = (t * mub - u * mua) - 2.f * mua * ds - mub * dcv;
                            if (Q == kSsimAll || ds_a) ds_a[at] = ds;
                        }
                        if (dm_b) {
                            dm_b[at] = (t * mua - u * mub) - 2.f * mub * ds - mua * dcv;
                            if (Q == kSsimAll || ds_b) ds_b[at] = ds;
                        }
                    }
                }
            }
            if constexpr (Q != kSsimAll) {                                     // this channel's partial: wave butterfly, then the four waves
#pragma unroll
                for (int off = 32; off; off >>= 1) acc += __shfl_xor(acc, off);
                if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = acc;
                acc = 0.0;
            }
            __syncthreads();                                                   // hbuf is rewritten by the next channel
            if constexpr (Q != kSsimAll) {                                     // wave_sum is next written two barriers from here
                if (threadIdx.x == 0)
                    part[((size_t)lens * ((size_t)gridDim.x) + blockIdx.x) * g.C + (c0 + c)] =
                        ((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3];
            }
        }
    }
    if constexpr (Q != kSsimAll) return;
#pragma unroll
    for (int off = 32; off; off >>= 1) acc += __shfl_xor(acc, off);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0)
        part[(size_t)lens * ((size_t)gridDim.x) + blockIdx.x] = ((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3];
}

// grid (lenses): value[b] = (sum of the lens's tile partials, in a fixed order) / (Hm Wm C)
__global__ __launch_bounds__(kBlock) void ssim_finish_kernel(const double *__restrict__ part, float *__restrict__ value, const int tiles,
                                                             const double count)
{
    __shared__ double s[kBlock];
    const double *__restrict__ p = part + (size_t)blockIdx.x * tiles;
    double acc = 0.0;
    for (int t = threadIdx.x; t < tiles; t += kBlock) acc += p[t];
    s[threadIdx.x] = acc;
    __syncthreads();
    for (int n = kBlock / 2; n; n >>= 1) {
        if ((int)threadIdx.x < n) s[threadIdx.x] += s[threadIdx.x + n];
        __syncthreads();
    }
    if (threadIdx.x == 0) value[blockIdx.x] = (float)(s[0] / count);
}

// The backward of one level of the multi-scale pyramid (MS): the seed of lens and channel is g_value[b] / C factor[b,c,level]
// / (Hm Wm) with factor = d ms / d v_level from the finish kernel, and, where `coarse` is given (the gradient to the next level's
// image, dense channels-last [B,Hc,Wc,C]), the store adds the adjoint of the 2 x 2 mean: a quarter of the coarse pixel
// (y / 2, x / 2), twice that per axis on which this pixel is the doubled last row or column of an odd side.
struct Pyramid {
    const double *factor;                           // [B, C, levels]
    const float *coarse;                            // or NULL on the coarsest level
    int level, levels, Hc, Wc;
};

// grid (tiles of the image, lenses of this launch); dynamic LDS = bwd_lds_floats(min(C, 4)) floats
template <int K, bool MS>
__global__ __launch_bounds__(kBlock) void ssim_bwd_kernel(const Geo g, const float *__restrict__ p, const float *__restrict__ q,
                                                          const float *__restrict__ dm, const float *__restrict__ ds,
                                                          const float *__restrict__ dc, const float *__restrict__ g_value,
                                                          float *__restrict__ g_p, const int b0, const Pyramid pyr)
{
    extern __shared__ __align__(16) float lds[];
    const int nch = min(g.C, kCh);
    float *hbuf = lds + 3 * nch * kPlane;
    const int ty = (int)blockIdx.x / g.tiles_x, tx = (int)blockIdx.x - ty * g.tiles_x;
    const int y0 = ty * kTY, x0 = tx * kTX;
    const int th = min(kTY, g.H - y0), tw = min(kTX, g.W - x0);                // input pixels of this tile
    const int rows = th + K - 1, cols = tw + K - 1;                            // map pixels from (y0 - K + 1, x0 - K + 1): zero outside
    const int lens = b0 + blockIdx.y;
    const int64_t ms_x = g.C, ms_y = (int64_t)g.Wm * g.C;
    const size_t map_at = (size_t)lens * g.Hm * g.Wm * g.C;
    const Source maps[3] = {{dm + map_at, ms_y, ms_x, 1}, {ds + map_at, ms_y, ms_x, 1}, {dc + map_at, ms_y, ms_x, 1}};
    const int vx = threadIdx.x & (kTX - 1), vy = (threadIdx.x / kTX) * 2;
    float scale = 0.f;
    if constexpr (!MS) scale = (float)((double)g_value[lens] / ((double)g.Hm * (double)g.Wm * (double)g.C));
    float w[K];
#pragma unroll
    for (int k = 0; k < K; ++k) w[k] = g.w[k];
    for (int c0 = 0; c0 < g.C; c0 += kCh) {
        const int nc = min(kCh, g.C - c0);
        __syncthreads();
        load_planes<3>(lds, nch * kPlane, maps, y0 - (K - 1), x0 - (K - 1), rows, cols, g.Hm, g.Wm, c0, nc);
        __syncthreads();
        for (int c = 0; c < nc; ++c) {
            // this lane's own p and q, asked for now and used after the two passes
            float pv[2] = {0.f, 0.f}, qv[2] = {0.f, 0.f}, up[2] = {0.f, 0.f};
#pragma unroll
            for (int half = 0; half < 2; ++half)
                if (vx < tw && vy + half < th) {
                    const int64_t y = y0 + vy + half, x = x0 + vx, ch = c0 + c;
                    pv[half] = p[(int64_t)lens * g.a_s[0] + y * g.a_s[1] + x * g.a_s[2] + ch * g.a_s[3]];
                    qv[half] = q[(int64_t)lens * g.b_s[0] + y * g.b_s[1] + x * g.b_s[2] + ch * g.b_s[3]];
                    if constexpr (MS) {
                        if (pyr.coarse) {
                            const float weight = (((g.H & 1) && y == g.H - 1) ? 2.f : 1.f) * (((g.W & 1) && x == g.W - 1) ? 0.5f : 0.25f);
                            up[half] = weight * pyr.coarse[(((size_t)lens * pyr.Hc + (y >> 1)) * pyr.Wc + (x >> 1)) * g.C + ch];
                        }
                    }
                }
            if constexpr (MS)
                scale = (float)((double)g_value[lens] / (double)g.C * pyr.factor[((size_t)lens * g.C + (c0 + c)) * pyr.levels + pyr.level]
                                / ((double)g.Hm * (double)g.Wm));
            // raw column x + K - 1 - j is map column x0 + x - j: the window runs backwards along the row
            // (a row and a column pair per lane, as in the forward)
            for (int it = threadIdx.x; it < rows * (kTX / 2); it += kBlock) {
                const int r = it / (kTX / 2), x = (it & (kTX / 2 - 1)) * 2;
                if (x >= tw) continue;
#pragma unroll
                for (int m = 0; m < 3; ++m) {
                    float v[K + 1];
                    read_run<K>(lds + (m * nch + c) * kPlane + r * kHX + x, v);
                    float u0 = 0.f, u1 = 0.f;
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        u0 = __builtin_fmaf(w[K - 1 - k], v[k], u0);
                        u1 = __builtin_fmaf(w[K - 1 - k], v[k + 1], u1);
                    }
                    hbuf[m * kHPlane + x * kHY + r] = u0;
                    hbuf[m * kHPlane + (x + 1) * kHY + r] = u1;
                }
            }
            __syncthreads();
            if (vx < tw && vy < th) {
                float s0[3], s1[3];
#pragma unroll
                for (int m = 0; m < 3; ++m) {
                    float v[K + 1];
                    read_run<K>(hbuf + m * kHPlane + vx * kHY + vy, v);
                    float u0 = 0.f, u1 = 0.f;
#pragma unroll
                    for (int k = 0; k <= K; ++k) {
                        if (k < K) u0 = __builtin_fmaf(w[K - 1 - k], v[k], u0);
                        if (k > 0) u1 = __builtin_fmaf(w[K - k], v[k], u1);
                    }
                    s0[m] = u0;
                    s1[m] = u1;
                }
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    if (vy + half >= th) break;
                    const float *s = half ? s1 : s0;
                    const int64_t y = y0 + vy + half, x = x0 + vx, ch = c0 + c;
                    const float v = __builtin_fmaf(qv[half], s[2], __builtin_fmaf(2.f * pv[half], s[1], s[0]));
                    if constexpr (MS)
                        g_p[(int64_t)lens * g.g_s[0] + y * g.g_s[1] + x * g.g_s[2] + ch * g.g_s[3]] = __builtin_fmaf(v, scale, up[half]);
                    else
                        g_p[(int64_t)lens * g.g_s[0] + y * g.g_s[1] + x * g.g_s[2] + ch * g.g_s[3]] = v * scale;
                }
            }
            __syncthreads();
        }
    }
}

constexpr int kMaxLevels = 8;

// The 2 x 2 mean with stride 2 of both images in one launch: out[y', x'] = 1/4 sum in[min(2y' + dy, H - 1), min(2x' + dx, W - 1)]
// (the last row or column of an odd side counts twice).  grid (blocks over the Ho Wo C elements of a pooled image, lenses of this
// launch): consecutive lanes take consecutive (pixel, channel) of the dense channels-last output.  s_a, s_b: the strides of the inputs.
struct PoolGeo {
    int H, W, C, Ho, Wo;
    int64_t a_s[4], b_s[4];
};
__global__ __launch_bounds__(kBlock) void ms_pool_kernel(const PoolGeo g, const float *__restrict__ a, const float *__restrict__ b,
                                                         float *__restrict__ out_a, float *__restrict__ out_b, const int b0)
{
    const unsigned n = (unsigned)g.Ho * (unsigned)g.Wo * (unsigned)g.C;        // < 2^31 (checked on the host)
    const unsigned e = blockIdx.x * (unsigned)kBlock + threadIdx.x;
    if (e >= n) return;
    const int lens = b0 + blockIdx.y;
    const unsigned pix = e / (unsigned)g.C, c = e - pix * (unsigned)g.C;
    const int yo = (int)(pix / (unsigned)g.Wo), xo = (int)(pix - (unsigned)yo * (unsigned)g.Wo);
    const int64_t y0 = 2 * yo, y1 = min(2 * yo + 1, g.H - 1), x0 = 2 * xo, x1 = min(2 * xo + 1, g.W - 1);
    const float *pa = a + (int64_t)lens * g.a_s[0] + (int64_t)c * g.a_s[3], *pb = b + (int64_t)lens * g.b_s[0] + (int64_t)c * g.b_s[3];
    const float a00 = pa[y0 * g.a_s[1] + x0 * g.a_s[2]], a01 = pa[y0 * g.a_s[1] + x1 * g.a_s[2]];
    const float a10 = pa[y1 * g.a_s[1] + x0 * g.a_s[2]], a11 = pa[y1 * g.a_s[1] + x1 * g.a_s[2]];
    const float b00 = pb[y0 * g.b_s[1] + x0 * g.b_s[2]], b01 = pb[y0 * g.b_s[1] + x1 * g.b_s[2]];
    const float b10 = pb[y1 * g.b_s[1] + x0 * g.b_s[2]], b11 = pb[y1 * g.b_s[1] + x1 * g.b_s[2]];
    const size_t at = (size_t)lens * n + e;
    out_a[at] = 0.25f * ((a00 + a01) + (a10 + a11));
    out_b[at] = 0.25f * ((b00 + b01) + (b10 + b11));
}

// grid (lenses): per channel and level the tile partials are added in fp64, strided over the 256 lanes and then by a tree (a
// fixed order), v = sum / (Hm Wm); then lane 0 forms ms[c] = prod_k max(v_k, 0)^p_k, value = mean_c ms[c] and the backward
// factors d ms / d v_k = p_k ms / v_k -- exactly 0 for every level of a (lens, channel) of which any term is <= 0 -- in fp64.
struct FinishPlan {
    int M, C;
    int tiles[kMaxLevels];
    unsigned long long part_at[kMaxLevels];
    double count[kMaxLevels], power[kMaxLevels];
};
__global__ __launch_bounds__(kBlock) void ms_finish_kernel(const FinishPlan f, const double *__restrict__ part, float *__restrict__ value,
                                                           float *__restrict__ terms, double *__restrict__ factor)
{
    __shared__ double s[kBlock];
    const size_t lens = blockIdx.x;
    double total = 0.0;                                                        // lane 0's
    for (int c = 0; c < f.C; ++c) {
        double v[kMaxLevels];
        for (int k = 0; k < f.M; ++k) {
            const double *__restrict__ p = part + f.part_at[k] + lens * (size_t)f.tiles[k] * f.C + c;
            double acc = 0.0;
            for (int t = threadIdx.x; t < f.tiles[k]; t += kBlock) acc += p[(size_t)t * f.C];
            __syncthreads();                                                   // lane 0 has read the last sum
            s[threadIdx.x] = acc;
            __syncthreads();
            for (int n = kBlock / 2; n; n >>= 1) {
                if ((int)threadIdx.x < n) s[threadIdx.x] += s[threadIdx.x + n];
                __syncthreads();
            }
            v[k] = s[0] / f.count[k];
        }
        if (threadIdx.x == 0) {
            bool positive = true;
            double ms = 1.0;
            for (int k = 0; k < f.M; ++k) {
                positive = positive && v[k] > 0.0;
                ms *= pow(fmax(v[k], 0.0), f.power[k]);
            }
            for (int k = 0; k < f.M; ++k) {
                const size_t at = (lens * f.C + c) * f.M + k;
                terms[at] = (float)v[k];
                factor[at] = positive ? f.power[k] * ms / v[k] : 0.0;
            }
            total += ms;
        }
    }
    if (threadIdx.x == 0) value[lens] = (float)(total / (double)f.C);
}

// ------------------------------------------------------------------------------------------------------------------- host
//
// What both public geometries come to (two adapters fill it; the members keep the callers' meaning).  `pyramid` marks
// tl_ms_ssim_*: the single scale is NOT a pyramid of one level -- that sums per channel, clamps a negative mean and seeds
// and stores differently -- so everything below asks `pyramid`, never `levels == 1`.
struct Desc {
    bool given, pyramid;                            // given: the caller's g was not NULL
    int device, B, H, W, C, K, flags, levels;
    float C1, C2;
    const float *window, *power;
    const int64_t *a_s, *b_s, *g_s;
};
template <typename G>
Desc desc_of(const G *g, bool pyramid)
{
    Desc d{};
    d.pyramid = pyramid;
    if (!g) return d;
    d.given = true; d.device = g->device; d.B = g->B; d.H = g->H; d.W = g->W; d.C = g->C; d.K = g->K; d.flags = g->flags;
    d.C1 = g->C1; d.C2 = g->C2; d.window = g->window;
    d.a_s = g->a_stride; d.b_s = g->b_stride; d.g_s = g->g_stride;
    return d;
}
Desc desc_of(const tl_ssim_geom *g) { return desc_of(g, false); }
Desc desc_of(const tl_ms_ssim_geom *g)
{
    Desc d = desc_of(g, true);
    if (g) { d.levels = g->levels; d.power = g->power; }
    return d;
}

int64_t tiles_of(int n_y, int n_x) { return (int64_t)((n_y + kTY - 1) / kTY) * ((n_x + kTX - 1) / kTX); }

thread_local char t_what[160];                      // a fault that carries numbers; refuse() copies it before the next one

// Everything about the geometry that can be refused without a HIP call, in the order each entry point documents; nullptr
// when it is fine.
const char *geom_fault(const Desc &d)
{
    if (!d.given) return "g is NULL";
    if (d.B < 1 || d.H < 1 || d.W < 1 || d.C < 1) return "B, H, W, C must be >= 1";
    if (d.K < 3 || d.K > kMaxK || d.K % 2 == 0) return "K must be odd, 3 <= K <= 11";
    if (d.pyramid && (d.levels < 1 || d.levels > kMaxLevels)) return "levels must be 1 .. 8";
    if (!d.pyramid && (d.H < d.K || d.W < d.K)) return "H and W must be >= K (the window is valid only)";
    if (d.H > kMaxEdge || d.W > kMaxEdge) return "H and W must be <= 2^20";
    if (tiles_of(d.H, d.W) > kMaxTiles) return "H W must fit 2^22 tiles of 16 x 32 pixels";
    if (d.pyramid && (int64_t)d.H * d.W * d.C >= ((int64_t)1 << 31)) return "H W C must be below 2^31";
    if (d.flags & ~3) return "flags has bits other than bit 0 (maps of a) and bit 1 (maps of b) set";
    int h = d.H, w = d.W;
    for (int k = 0; k < d.levels; ++k, h = (h + 1) / 2, w = (w + 1) / 2)           // no level without a pyramid
        if (h < d.K || w < d.K) {
            snprintf(t_what, sizeof(t_what), "level %d is %d x %d, every level must be >= K = %d on both sides", k, h, w, d.K);
            return t_what;
        }
    return nullptr;
}

// `name` (work, keep) NULL, misaligned, or its size `size_name` below what `planner` asks; nullptr when it is fine
const char *buffer_fault(const char *name, const void *at, const char *size_name, size_t given, const char *planner, size_t need)
{
    if (!at)
        snprintf(t_what, sizeof(t_what), "%s is NULL", name);
    else if ((uintptr_t)at % 8)
        snprintf(t_what, sizeof(t_what), "%s must be aligned to 8 bytes", name);
    else if (given < need)
        snprintf(t_what, sizeof(t_what), "%s is %zu, %s asks for %zu", size_name, given, planner, need);
    else
        return nullptr;
    return t_what;
}

int refuse(const char *fn, const char *what)
{
    char msg[256];
    snprintf(msg, sizeof(msg), "%s: %s", fn, what);
    return tl_host::fail(TL_EINVAL, msg);
}

// the single scale's workspace: one double per (lens, tile of the map)
size_t work_bytes(const Desc &d)
{
    const size_t raw = (size_t)d.B * (size_t)tiles_of(d.H - d.K + 1, d.W - d.K + 1) * sizeof(double);
    return (raw + 255) / 256 * 256;
}

// The pyramid.  tl_ms_ssim_fwd: per level k = 0 .. M - 1, [pool level k - 1 -> k for both images], the term forward of level
// k (kCsChan below the top, kSsimChan on it); then ONE finish launch.  tl_ms_ssim_bwd: per level from the coarsest to the
// finest one ssim_bwd_kernel<K, true>, which adds the unpooled gradient of the level above in its store.  Every launch goes
// on the stream back to back.  KEEP (floats): [ factor: B C M doubles | pooled a, levels 1 .. M - 1 | pooled b | the maps
// dm_a (flags bit 0), dm_b (bit 1), ds, dc (either bit), each all levels one after the other ], every image and map dense
// channels-last.  WORK: forward, the tile partials, one double per (level, lens, tile, channel); backward, the gradients to
// the pooled images of levels 1 .. M - 1.
struct Level {
    int H, W, Hm, Wm;
    int64_t tiles;                                  // of the map
    size_t part_at, image_at, map_at;               // doubles into the partials; floats into one pooled pyramid / one map
};
struct Plan {
    int M, n_maps;
    Level lv[kMaxLevels];
    size_t part_doubles, image_floats, map_floats, factor_floats, keep_floats, work_bytes;
};
Plan make_plan(const Desc &d)
{
    Plan p{};
    p.M = d.levels;
    p.n_maps = (d.flags & 3) == 3 ? 4 : (d.flags & 3) ? 3 : 0;
    int h = d.H, w = d.W;
    for (int k = 0; k < p.M; ++k, h = (h + 1) / 2, w = (w + 1) / 2) {
        Level &l = p.lv[k];
        l.H = h; l.W = w; l.Hm = h - d.K + 1; l.Wm = w - d.K + 1;
        l.tiles = tiles_of(l.Hm, l.Wm);
        l.part_at = p.part_doubles; l.image_at = p.image_floats; l.map_at = p.map_floats;
        p.part_doubles += (size_t)d.B * (size_t)l.tiles * (size_t)d.C;
        if (k > 0) p.image_floats += (size_t)d.B * h * w * d.C;
        p.map_floats += (size_t)d.B * l.Hm * l.Wm * d.C;
    }
    p.factor_floats = 2 * (size_t)d.B * d.C * p.M;
    p.keep_floats = p.factor_floats + 2 * p.image_floats + (size_t)p.n_maps * p.map_floats;
    p.work_bytes = (std::max(p.part_doubles * sizeof(double), p.image_floats * sizeof(float)) + 255) / 256 * 256;
    return p;
}

// the slots of the maps in KEEP after the factors and the two pooled pyramids: dm_a, dm_b (as far as kept), ds, dc
struct Maps { float *dm_a, *dm_b, *ds, *dc; };
Maps maps_of(const Desc &d, const Plan &p, float *keep)
{
    float *at = keep + p.factor_floats + 2 * p.image_floats;
    Maps m{nullptr, nullptr, nullptr, nullptr};
    if (d.flags & 1) { m.dm_a = at; at += p.map_floats; }
    if (d.flags & 2) { m.dm_b = at; at += p.map_floats; }
    if (d.flags & 3) { m.ds = at; m.dc = at + p.map_floats; }
    return m;
}

// The Geo of one level of h x w pixels.  n_x: the columns that the launch tiles (of the map in the forward, of the image in
// the backward).  callers: the images are the caller's and lie at its strides (level 0); otherwise dense channels-last.
Geo make_geo(const Desc &d, int h, int w, int n_x, bool callers)
{
    Geo q;
    q.B = d.B; q.H = h; q.W = w; q.C = d.C; q.Hm = h - d.K + 1; q.Wm = w - d.K + 1;
    q.tiles_x = (n_x + kTX - 1) / kTX;
    for (int k = 0; k < kMaxK; ++k) q.w[k] = k < d.K ? d.window[k] : 0.f;
    q.C1 = d.C1; q.C2 = d.C2;
    const int64_t dense[4] = {(int64_t)h * w * d.C, (int64_t)w * d.C, d.C, 1};
    const int64_t *a_s = callers ? d.a_s : dense, *b_s = callers ? d.b_s : dense, *g_s = callers ? d.g_s : dense;
    for (int k = 0; k < 4; ++k) { q.a_s[k] = a_s[k]; q.b_s[k] = b_s[k]; q.g_s[k] = g_s[k]; }
    return q;
}

template <typename F>
void for_k(int K, F &&f)
{
    switch (K) {
    case 3: f(std::integral_constant<int, 3>()); break;
    case 5: f(std::integral_constant<int, 5>()); break;
    case 7: f(std::integral_constant<int, 7>()); break;
    case 9: f(std::integral_constant<int, 9>()); break;
    default: f(std::integral_constant<int, 11>()); break;
    }
}

// B cut into launches of at most 65535 lenses: launch(first lens, lenses), checked under the name `what`; the first launch
// that fails ends it.
template <typename F>
int for_lens_chunks(int B, const char *what, F &&launch)
{
    for (int b0 = 0; b0 < B; b0 += kMaxY) {
        launch(b0, (unsigned)std::min(kMaxY, B - b0));
        if (const int rc = tl_host::launched(what)) return rc;
    }
    return TL_OK;
}

// The forward of one level over all lenses, summing `what`.  A NULL map is not written.
struct FwdOut { float *dm_a, *ds_a, *dm_b, *ds_b, *dc; double *part; };
int launch_fwd(const Desc &d, const Geo &q, Quantity what, const float *a, const float *b, const FwdOut &o, const char *name, hipStream_t st)
{
    const unsigned tiles = (unsigned)tiles_of(q.Hm, q.Wm);
    const size_t lds = (size_t)fwd_lds_floats(std::min(d.C, kCh)) * sizeof(float);
    return for_lens_chunks(d.B, name, [&](int b0, unsigned lenses) {
        for_k(d.K, [&](auto kk) {
            constexpr int K = decltype(kk)::value;
            auto *kernel = what == kSsimAll ? ssim_fwd_kernel<K, kSsimAll> : what == kCsChan ? ssim_fwd_kernel<K, kCsChan> : ssim_fwd_kernel<K, kSsimChan>;
            hipLaunchKernelGGL(kernel, dim3(tiles, lenses), dim3(kBlock), lds, st, q, a, b, o.dm_a, o.ds_a, o.dm_b, o.ds_b, o.dc, o.part, b0);
        });
    });
}

// The backward of one level over all lenses: of the single scale (ms false, pyr unused) or of a level of the pyramid.
int launch_bwd(const Desc &d, const Geo &q, bool ms, const Pyramid &pyr, const float *p, const float *q_image, const float *dm,
               const float *ds, const float *dc, const float *g_value, float *g_p, const char *name, hipStream_t st)
{
    const unsigned tiles = (unsigned)tiles_of(q.H, q.W);
    const size_t lds = (size_t)bwd_lds_floats(std::min(d.C, kCh)) * sizeof(float);
    return for_lens_chunks(d.B, name, [&](int b0, unsigned lenses) {
        for_k(d.K, [&](auto kk) {
            constexpr int K = decltype(kk)::value;
            auto *kernel = ms ? ssim_bwd_kernel<K, true> : ssim_bwd_kernel<K, false>;
            hipLaunchKernelGGL(kernel, dim3(tiles, lenses), dim3(kBlock), lds, st, q, p, q_image, dm, ds, dc, g_value, g_p, b0, pyr);
        });
    });
}

}  // namespace

extern "C" {

size_t tl_ssim_work_bytes(const tl_ssim_geom *g) { const Desc d = desc_of(g); return geom_fault(d) ? 0 : work_bytes(d); }

size_t tl_ssim_maps_elems(const tl_ssim_geom *g)
{
    return geom_fault(desc_of(g)) ? 0 : (size_t)g->B * (size_t)(g->H - g->K + 1) * (size_t)(g->W - g->K + 1) * (size_t)g->C;
}

int tl_ssim_fwd(const tl_ssim_geom *g, const float *a, const float *b, float *value, float *dm_a, float *ds_a, float *dm_b,
                float *ds_b, float *dc, void *work, size_t work_bytes_given, void *stream)
{
    const char *fn = "tl_ssim_fwd";
    const Desc d = desc_of(g);
    if (const char *what = geom_fault(d)) return refuse(fn, what);
    if (!a) return refuse(fn, "a is NULL");
    if (!b) return refuse(fn, "b is NULL");
    if (!value) return refuse(fn, "value is NULL");
    if ((d.flags & 1) && !dm_a) return refuse(fn, "flags bit 0 asks for the maps of a, dm_a is NULL");
    if ((d.flags & 1) && !ds_a) return refuse(fn, "flags bit 0 asks for the maps of a, ds_a is NULL");
    if ((d.flags & 2) && !dm_b) return refuse(fn, "flags bit 1 asks for the maps of b, dm_b is NULL");
    if ((d.flags & 2) && !ds_b) return refuse(fn, "flags bit 1 asks for the maps of b, ds_b is NULL");
    if ((d.flags & 3) && !dc) return refuse(fn, "flags asks for partial maps, dc is NULL");
    if (const char *what = buffer_fault("work", work, "work_bytes", work_bytes_given, "tl_ssim_work_bytes", work_bytes(d)))
        return refuse(fn, what);
    if (const int rc = tl_host::use_device(d.device)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const Geo q = make_geo(d, d.H, d.W, d.W - d.K + 1, true);
    // a map that the flags do not ask for is not written, whatever its pointer
    const FwdOut out{(d.flags & 1) ? dm_a : nullptr, (d.flags & 1) ? ds_a : nullptr, (d.flags & 2) ? dm_b : nullptr,
                     (d.flags & 2) ? ds_b : nullptr, (d.flags & 3) ? dc : nullptr, (double *)work};
    if (const int rc = launch_fwd(d, q, kSsimAll, a, b, out, "ssim_fwd_kernel launch", st)) return rc;
    hipLaunchKernelGGL(ssim_finish_kernel, dim3((unsigned)d.B), dim3(kBlock), 0, st, out.part, value, (int)tiles_of(q.Hm, q.Wm),
                       (double)q.Hm * (double)q.Wm * (double)d.C);
    return tl_host::launched("ssim_finish_kernel launch");
}

int tl_ssim_bwd(const tl_ssim_geom *g, const float *p, const float *q, const float *dm, const float *ds, const float *dc,
                const float *g_value, float *g_p, void *stream)
{
    const char *fn = "tl_ssim_bwd";
    const Desc d = desc_of(g);
    if (const char *what = geom_fault(d)) return refuse(fn, what);
    if (!p) return refuse(fn, "p is NULL");
    if (!q) return refuse(fn, "q is NULL");
    if (!dm) return refuse(fn, "dm is NULL");
    if (!ds) return refuse(fn, "ds is NULL");
    if (!dc) return refuse(fn, "dc is NULL");
    if (!g_value) return refuse(fn, "g_value is NULL");
    if (!g_p) return refuse(fn, "g_p is NULL");
    if (const int rc = tl_host::use_device(d.device)) return rc;
    return launch_bwd(d, make_geo(d, d.H, d.W, d.W, true), false, Pyramid{}, p, q, dm, ds, dc, g_value, g_p, "ssim_bwd_kernel launch",
                      (hipStream_t)stream);
}

size_t tl_ms_ssim_work_bytes(const tl_ms_ssim_geom *g) { const Desc d = desc_of(g); return geom_fault(d) ? 0 : make_plan(d).work_bytes; }

size_t tl_ms_ssim_keep_elems(const tl_ms_ssim_geom *g) { const Desc d = desc_of(g); return geom_fault(d) ? 0 : make_plan(d).keep_floats; }

int tl_ms_ssim_fwd(const tl_ms_ssim_geom *g, const float *a, const float *b, float *value, float *terms, float *keep,
                   size_t keep_elems, void *work, size_t work_bytes_given, void *stream)
{
    const char *fn = "tl_ms_ssim_fwd";
    const Desc d = desc_of(g);
    if (const char *what = geom_fault(d)) return refuse(fn, what);
    if (!a) return refuse(fn, "a is NULL");
    if (!b) return refuse(fn, "b is NULL");
    if (!value) return refuse(fn, "value is NULL");
    if (!terms) return refuse(fn, "terms is NULL");
    const Plan plan = make_plan(d);
    if (const char *what = buffer_fault("keep", keep, "keep_elems", keep_elems, "tl_ms_ssim_keep_elems", plan.keep_floats))
        return refuse(fn, what);
    if (const char *what = buffer_fault("work", work, "work_bytes", work_bytes_given, "tl_ms_ssim_work_bytes", plan.work_bytes))
        return refuse(fn, what);
    if (const int rc = tl_host::use_device(d.device)) return rc;
    hipStream_t st = (hipStream_t)stream;
    double *factor = (double *)keep, *part = (double *)work;
    float *pool_a = keep + plan.factor_floats, *pool_b = pool_a + plan.image_floats;
    const Maps maps = maps_of(d, plan, keep);
    FinishPlan fin{};
    fin.M = plan.M; fin.C = d.C;
    for (int k = 0; k < plan.M; ++k) {
        const Level &l = plan.lv[k];
        fin.tiles[k] = (int)l.tiles; fin.part_at[k] = l.part_at;
        fin.count[k] = (double)l.Hm * (double)l.Wm; fin.power[k] = (double)d.power[k];
        const float *pa = k ? pool_a + l.image_at : a, *pb = k ? pool_b + l.image_at : b;      // levels >= 1: dense, in KEEP
        if (k) {                                                                   // level k - 1 -> level k
            const Level &from = plan.lv[k - 1];
            const Geo src = make_geo(d, from.H, from.W, from.W, k == 1);               // for the strides of level k - 1
            PoolGeo pg{from.H, from.W, d.C, l.H, l.W, {}, {}};
            for (int i = 0; i < 4; ++i) { pg.a_s[i] = src.a_s[i]; pg.b_s[i] = src.b_s[i]; }
            const float *src_a = k == 1 ? a : pool_a + from.image_at, *src_b = k == 1 ? b : pool_b + from.image_at;
            const unsigned blocks = (unsigned)(((size_t)l.H * l.W * d.C + kBlock - 1) / kBlock);
            const int rc = for_lens_chunks(d.B, "ms_pool_kernel launch", [&](int b0, unsigned lenses) {
                hipLaunchKernelGGL(ms_pool_kernel, dim3(blocks, lenses), dim3(kBlock), 0, st, pg, src_a, src_b, pool_a + l.image_at,
                                   pool_b + l.image_at, b0);
            });
            if (rc) return rc;
        }
        // ds is kept once: the kernel writes it through ds_a when a's maps are kept, through ds_b otherwise
        float *dm_a = maps.dm_a ? maps.dm_a + l.map_at : nullptr, *dm_b = maps.dm_b ? maps.dm_b + l.map_at : nullptr;
        float *ds = maps.ds ? maps.ds + l.map_at : nullptr, *dc = maps.dc ? maps.dc + l.map_at : nullptr;
        const FwdOut out{dm_a, dm_a ? ds : nullptr, dm_b, dm_a ? nullptr : ds, dc, part + l.part_at};
        if (const int rc = launch_fwd(d, make_geo(d, l.H, l.W, l.Wm, k == 0), k < plan.M - 1 ? kCsChan : kSsimChan, pa, pb, out,
                                      "ssim_fwd_kernel launch (pyramid)", st))
            return rc;
    }
    hipLaunchKernelGGL(ms_finish_kernel, dim3((unsigned)d.B), dim3(kBlock), 0, st, fin, part, value, terms, factor);
    return tl_host::launched("ms_finish_kernel launch");
}

int tl_ms_ssim_bwd(const tl_ms_ssim_geom *g, const float *p, const float *q, const float *keep, size_t keep_elems,
                   const float *g_value, float *g_p, int which, void *work, size_t work_bytes_given, void *stream)
{
    const char *fn = "tl_ms_ssim_bwd";
    const Desc d = desc_of(g);
    if (const char *what = geom_fault(d)) return refuse(fn, what);
    if (!p) return refuse(fn, "p is NULL");
    if (!q) return refuse(fn, "q is NULL");
    if (!g_value) return refuse(fn, "g_value is NULL");
    if (!g_p) return refuse(fn, "g_p is NULL");
    if (which != 0 && which != 1) return refuse(fn, "which must be 0 (p is a) or 1 (p is b)");
    if (!(d.flags & (1 << which))) return refuse(fn, "which names an image whose maps flags did not keep");
    const Plan plan = make_plan(d);
    if (const char *what = buffer_fault("keep", keep, "keep_elems", keep_elems, "tl_ms_ssim_keep_elems", plan.keep_floats))
        return refuse(fn, what);
    if (const char *what = buffer_fault("work", work, "work_bytes", work_bytes_given, "tl_ms_ssim_work_bytes", plan.work_bytes))
        return refuse(fn, what);
    if (const int rc = tl_host::use_device(d.device)) return rc;
    const float *pool_a = keep + plan.factor_floats, *pool_b = pool_a + plan.image_floats;
    const float *pool_p = which ? pool_b : pool_a, *pool_q = which ? pool_a : pool_b;
    const Maps maps = maps_of(d, plan, const_cast<float *>(keep));
    const float *dm = which ? maps.dm_b : maps.dm_a;
    float *grads = (float *)work;                                                  // of the pooled images, levels 1 .. M - 1
    for (int k = plan.M - 1; k >= 0; --k) {
        const Level &l = plan.lv[k];
        Pyramid pyr{(const double *)keep, nullptr, k, plan.M, 0, 0};
        if (k < plan.M - 1) {
            pyr.coarse = grads + plan.lv[k + 1].image_at;
            pyr.Hc = plan.lv[k + 1].H; pyr.Wc = plan.lv[k + 1].W;
        }
        const int rc = launch_bwd(d, make_geo(d, l.H, l.W, l.W, k == 0), true, pyr, k ? pool_p + l.image_at : p, k ? pool_q + l.image_at : q,
                                  dm + l.map_at, maps.ds + l.map_at, maps.dc + l.map_at, g_value, k ? grads + l.image_at : g_p,
                                  "ssim_bwd_kernel launch (pyramid)", (hipStream_t)stream);
        if (rc) return rc;
    }
    return TL_OK;
}

}  // extern "C"
