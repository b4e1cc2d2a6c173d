// tl_ssim.hip -- the structural similarity of two images under a separable Gaussian window, per lens, and its gradients to both
// images (tl_ssim_fwd, tl_ssim_bwd of include/tl_trace.h; imaging.ssim(fused=True) stands on them).
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

int64_t tiles_of(int n_y, int n_x) { return (int64_t)((n_y + kTY - 1) / kTY) * ((n_x + kTX - 1) / kTX); }

// Everything about the geometry that can be refused without a HIP call; nullptr when it is fine.
const char *geom_fault(const tl_ssim_geom *g)
{
    if (!g) return "g is NULL";
    if (g->B < 1 || g->H < 1 || g->W < 1 || g->C < 1) return "B, H, W, C must be >= 1";
    if (g->K < 3 || g->K > kMaxK || g->K % 2 == 0) return "K must be odd, 3 <= K <= 11";
    if (g->H < g->K || g->W < g->K) return "H and W must be >= K (the window is valid only)";
    if (g->H > kMaxEdge || g->W > kMaxEdge) return "H and W must be <= 2^20";
    if (tiles_of(g->H, g->W) > kMaxTiles) return "H W must fit 2^22 tiles of 16 x 32 pixels";
    if (g->flags & ~3) return "flags has bits other than bit 0 (maps of a) and bit 1 (maps of b) set";
    return nullptr;
}

int refuse(const char *fn, const char *what)
{
    static thread_local char msg[256];
    snprintf(msg, sizeof(msg), "%s: %s", fn, what);
    return tl_host::fail(TL_EINVAL, msg);
}

size_t work_bytes(const tl_ssim_geom *g)
{
    const size_t raw = (size_t)g->B * (size_t)tiles_of(g->H - g->K + 1, g->W - g->K + 1) * sizeof(double);
    return (raw + 255) / 256 * 256;
}

// n_x: the columns that the launch tiles (of the map in the forward, of the image in the backward)
Geo make_geo(const tl_ssim_geom *g, int n_x)
{
    Geo q;
    q.B = g->B; q.H = g->H; q.W = g->W; q.C = g->C;
    q.Hm = g->H - g->K + 1; q.Wm = g->W - g->K + 1;
    q.tiles_x = (n_x + kTX - 1) / kTX;
    for (int k = 0; k < kMaxK; ++k) q.w[k] = k < g->K ? g->window[k] : 0.f;
    q.C1 = g->C1; q.C2 = g->C2;
    for (int k = 0; k < 4; ++k) { q.a_s[k] = g->a_stride[k]; q.b_s[k] = g->b_stride[k]; q.g_s[k] = g->g_stride[k]; }
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

// ------------------------------------------------------------------------------------------------- the multi-scale pyramid
//
// tl_ms_ssim_fwd: per level k = 0 .. M - 1, [pool level k - 1 -> k for both images], the term forward of level k (kCsChan
// below the top, kSsimChan on it); then ONE finish launch.  tl_ms_ssim_bwd: per level from the coarsest to the finest one
// ssim_bwd_kernel<K, true>, which adds the unpooled gradient of the level above in its store.  Every launch goes on the stream
// back to back.  KEEP (floats): [ factor: B C M doubles | pooled a, levels 1 .. M - 1 | pooled b | the maps dm_a (flags bit
// 0), dm_b (bit 1), ds, dc (either bit), each all levels one after the other ], every image and map dense channels-last.
// WORK: forward, the tile partials, one double per (level, lens, tile, channel); backward, the gradients to the pooled
// images of levels 1 .. M - 1.
constexpr int kMaxLevels = 8;

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

const char *ms_geom_fault(const tl_ms_ssim_geom *g)
{
    static thread_local char msg[160];
    if (!g) return "g is NULL";
    if (g->B < 1 || g->H < 1 || g->W < 1 || g->C < 1) return "B, H, W, C must be >= 1";
    if (g->K < 3 || g->K > kMaxK || g->K % 2 == 0) return "K must be odd, 3 <= K <= 11";
    if (g->levels < 1 || g->levels > kMaxLevels) return "levels must be 1 .. 8";
    if (g->H > kMaxEdge || g->W > kMaxEdge) return "H and W must be <= 2^20";
    if (tiles_of(g->H, g->W) > kMaxTiles) return "H W must fit 2^22 tiles of 16 x 32 pixels";
    if ((int64_t)g->H * g->W * g->C >= ((int64_t)1 << 31)) return "H W C must be below 2^31";
    if (g->flags & ~3) return "flags has bits other than bit 0 (maps of a) and bit 1 (maps of b) set";
    int h = g->H, w = g->W;
    for (int k = 0; k < g->levels; ++k, h = (h + 1) / 2, w = (w + 1) / 2)
        if (h < g->K || w < g->K) {
            snprintf(msg, sizeof(msg), "level %d is %d x %d, every level must be >= K = %d on both sides", k, h, w, g->K);
            return msg;
        }
    return nullptr;
}

Plan make_plan(const tl_ms_ssim_geom *g)
{
    Plan p{};
    p.M = g->levels;
    p.n_maps = (g->flags & 3) == 3 ? 4 : (g->flags & 3) ? 3 : 0;
    int h = g->H, w = g->W;
    for (int k = 0; k < p.M; ++k, h = (h + 1) / 2, w = (w + 1) / 2) {
        Level &l = p.lv[k];
        l.H = h; l.W = w; l.Hm = h - g->K + 1; l.Wm = w - g->K + 1;
        l.tiles = tiles_of(l.Hm, l.Wm);
        l.part_at = p.part_doubles; l.image_at = p.image_floats; l.map_at = p.map_floats;
        p.part_doubles += (size_t)g->B * (size_t)l.tiles * (size_t)g->C;
        if (k > 0) p.image_floats += (size_t)g->B * h * w * g->C;
        p.map_floats += (size_t)g->B * l.Hm * l.Wm * g->C;
    }
    p.factor_floats = 2 * (size_t)g->B * g->C * p.M;
    p.keep_floats = p.factor_floats + 2 * p.image_floats + (size_t)p.n_maps * p.map_floats;
    p.work_bytes = (std::max(p.part_doubles * sizeof(double), p.image_floats * sizeof(float)) + 255) / 256 * 256;
    return p;
}

Geo level_geo(const tl_ms_ssim_geom *g, const Level &l, int n_x)
{
    Geo q;
    q.B = g->B; q.H = l.H; q.W = l.W; q.C = g->C; q.Hm = l.Hm; q.Wm = l.Wm;
    q.tiles_x = (n_x + kTX - 1) / kTX;
    for (int k = 0; k < kMaxK; ++k) q.w[k] = k < g->K ? g->window[k] : 0.f;
    q.C1 = g->C1; q.C2 = g->C2;
    const int64_t dense[4] = {(int64_t)l.H * l.W * g->C, (int64_t)l.W * g->C, g->C, 1};
    for (int k = 0; k < 4; ++k) q.a_s[k] = q.b_s[k] = q.g_s[k] = dense[k];
    return q;
}

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

// the slots of the maps in KEEP after the factors and the two pooled pyramids: dm_a, dm_b (as far as kept), ds, dc
struct Maps { float *dm_a, *dm_b, *ds, *dc; };
Maps maps_of(const tl_ms_ssim_geom *g, const Plan &p, float *keep)
{
    float *at = keep + p.factor_floats + 2 * p.image_floats;
    Maps m{nullptr, nullptr, nullptr, nullptr};
    if (g->flags & 1) { m.dm_a = at; at += p.map_floats; }
    if (g->flags & 2) { m.dm_b = at; at += p.map_floats; }
    if (g->flags & 3) { m.ds = at; m.dc = at + p.map_floats; }
    return m;
}

}  // namespace

extern "C" {

size_t tl_ssim_work_bytes(const tl_ssim_geom *g) { return geom_fault(g) ? 0 : work_bytes(g); }

size_t tl_ssim_maps_elems(const tl_ssim_geom *g)
{
    return geom_fault(g) ? 0 : (size_t)g->B * (size_t)(g->H - g->K + 1) * (size_t)(g->W - g->K + 1) * (size_t)g->C;
}

int tl_ssim_fwd(const tl_ssim_geom *g, const float *a, const float *b, float *value, float *dm_a, float *ds_a, float *dm_b,
                float *ds_b, float *dc, void *work, size_t work_bytes_given, void *stream)
{
    if (const char *what = geom_fault(g)) return refuse("tl_ssim_fwd", what);
    if (!a) return refuse("tl_ssim_fwd", "a is NULL");
    if (!b) return refuse("tl_ssim_fwd", "b is NULL");
    if (!value) return refuse("tl_ssim_fwd", "value is NULL");
    if ((g->flags & 1) && !dm_a) return refuse("tl_ssim_fwd", "flags bit 0 asks for the maps of a, dm_a is NULL");
    if ((g->flags & 1) && !ds_a) return refuse("tl_ssim_fwd", "flags bit 0 asks for the maps of a, ds_a is NULL");
    if ((g->flags & 2) && !dm_b) return refuse("tl_ssim_fwd", "flags bit 1 asks for the maps of b, dm_b is NULL");
    if ((g->flags & 2) && !ds_b) return refuse("tl_ssim_fwd", "flags bit 1 asks for the maps of b, ds_b is NULL");
    if ((g->flags & 3) && !dc) return refuse("tl_ssim_fwd", "flags asks for partial maps, dc is NULL");
    const size_t need = work_bytes(g);
    if (!work) return refuse("tl_ssim_fwd", "work is NULL");
    if ((uintptr_t)work % 8) return refuse("tl_ssim_fwd", "work must be aligned to 8 bytes");
    if (work_bytes_given < need) {
        char what[128];
        snprintf(what, sizeof(what), "work_bytes is %zu, tl_ssim_work_bytes asks for %zu", work_bytes_given, need);
        return refuse("tl_ssim_fwd", what);
    }
    if (const int rc = tl_host::use_device(g->device)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int Hm = g->H - g->K + 1, Wm = g->W - g->K + 1;
    const Geo q = make_geo(g, Wm);
    const unsigned tiles = (unsigned)tiles_of(Hm, Wm);
    const size_t lds = (size_t)fwd_lds_floats(std::min(g->C, kCh)) * sizeof(float);
    // a map that the flags do not ask for is not written, whatever its pointer
    float *ma = (g->flags & 1) ? dm_a : nullptr, *sa = (g->flags & 1) ? ds_a : nullptr;
    float *mb = (g->flags & 2) ? dm_b : nullptr, *sb = (g->flags & 2) ? ds_b : nullptr;
    float *cc = (g->flags & 3) ? dc : nullptr;
    double *part = (double *)work;
    int rc = TL_OK;
    for (int b0 = 0; b0 < g->B && rc == TL_OK; b0 += kMaxY) {
        const dim3 grid(tiles, std::min(kMaxY, g->B - b0));
        for_k(g->K, [&](auto k) {
            hipLaunchKernelGGL((ssim_fwd_kernel<decltype(k)::value, kSsimAll>), grid, dim3(kBlock), lds, st, q, a, b, ma, sa, mb, sb, cc, part, b0);
        });
        rc = tl_host::launched("ssim_fwd_kernel launch");
    }
    if (rc) return rc;
    hipLaunchKernelGGL(ssim_finish_kernel, dim3((unsigned)g->B), dim3(kBlock), 0, st, part, value, (int)tiles,
                       (double)Hm * (double)Wm * (double)g->C);
    return tl_host::launched("ssim_finish_kernel launch");
}

int tl_ssim_bwd(const tl_ssim_geom *g, const float *p, const float *q, const float *dm, const float *ds, const float *dc,
                const float *g_value, float *g_p, void *stream)
{
    if (const char *what = geom_fault(g)) return refuse("tl_ssim_bwd", what);
    if (!p) return refuse("tl_ssim_bwd", "p is NULL");
    if (!q) return refuse("tl_ssim_bwd", "q is NULL");
    if (!dm) return refuse("tl_ssim_bwd", "dm is NULL");
    if (!ds) return refuse("tl_ssim_bwd", "ds is NULL");
    if (!dc) return refuse("tl_ssim_bwd", "dc is NULL");
    if (!g_value) return refuse("tl_ssim_bwd", "g_value is NULL");
    if (!g_p) return refuse("tl_ssim_bwd", "g_p is NULL");
    if (const int rc = tl_host::use_device(g->device)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const Geo geo = make_geo(g, g->W);
    const unsigned tiles = (unsigned)tiles_of(g->H, g->W);
    const size_t lds = (size_t)bwd_lds_floats(std::min(g->C, kCh)) * sizeof(float);
    for (int b0 = 0; b0 < g->B; b0 += kMaxY) {
        const dim3 grid(tiles, std::min(kMaxY, g->B - b0));
        for_k(g->K, [&](auto k) {
            hipLaunchKernelGGL((ssim_bwd_kernel<decltype(k)::value, false>), grid, dim3(kBlock), lds, st, geo, p, q, dm, ds, dc, g_value, g_p, b0,
                               Pyramid{});
        });
        if (const int rc = tl_host::launched("ssim_bwd_kernel launch")) return rc;
    }
    return TL_OK;
}

size_t tl_ms_ssim_work_bytes(const tl_ms_ssim_geom *g) { return ms_geom_fault(g) ? 0 : make_plan(g).work_bytes; }

size_t tl_ms_ssim_keep_elems(const tl_ms_ssim_geom *g) { return ms_geom_fault(g) ? 0 : make_plan(g).keep_floats; }

static const char *ms_buffers_fault(const Plan &plan, const void *keep, size_t keep_elems, const void *work, size_t work_bytes_given,
                                    const char *planner_keep, const char *planner_work)
{
    static thread_local char what[160];
    if (!keep) return "keep is NULL";
    if ((uintptr_t)keep % 8) return "keep must be aligned to 8 bytes";
    if (keep_elems < plan.keep_floats) {
        snprintf(what, sizeof(what), "keep_elems is %zu, %s asks for %zu", keep_elems, planner_keep, plan.keep_floats);
        return what;
    }
    if (!work) return "work is NULL";
    if ((uintptr_t)work % 8) return "work must be aligned to 8 bytes";
    if (work_bytes_given < plan.work_bytes) {
        snprintf(what, sizeof(what), "work_bytes is %zu, %s asks for %zu", work_bytes_given, planner_work, plan.work_bytes);
        return what;
    }
    return nullptr;
}

int tl_ms_ssim_fwd(const tl_ms_ssim_geom *g, const float *a, const float *b, float *value, float *terms, float *keep,
                   size_t keep_elems, void *work, size_t work_bytes_given, void *stream)
{
    const char *fn = "tl_ms_ssim_fwd";
    if (const char *what = ms_geom_fault(g)) return refuse(fn, what);
    if (!a) return refuse(fn, "a is NULL");
    if (!b) return refuse(fn, "b is NULL");
    if (!value) return refuse(fn, "value is NULL");
    if (!terms) return refuse(fn, "terms is NULL");
    const Plan plan = make_plan(g);
    if (const char *what = ms_buffers_fault(plan, keep, keep_elems, work, work_bytes_given, "tl_ms_ssim_keep_elems", "tl_ms_ssim_work_bytes"))
        return refuse(fn, what);
    if (const int rc = tl_host::use_device(g->device)) return rc;
    hipStream_t st = (hipStream_t)stream;
    double *factor = (double *)keep, *part = (double *)work;
    float *pool_a = keep + plan.factor_floats, *pool_b = pool_a + plan.image_floats;
    const Maps maps = maps_of(g, plan, keep);
    const size_t lds = (size_t)fwd_lds_floats(std::min(g->C, kCh)) * sizeof(float);
    FinishPlan fin{};
    fin.M = plan.M; fin.C = g->C;
    for (int k = 0; k < plan.M; ++k) {
        const Level &l = plan.lv[k];
        fin.tiles[k] = (int)l.tiles; fin.part_at[k] = l.part_at;
        fin.count[k] = (double)l.Hm * (double)l.Wm; fin.power[k] = (double)g->power[k];
        Geo q = level_geo(g, l, l.Wm);
        const float *pa = pool_a + l.image_at, *pb = pool_b + l.image_at;          // levels >= 1: dense, in KEEP
        if (k == 0) {
            pa = a; pb = b;
            for (int d = 0; d < 4; ++d) { q.a_s[d] = g->a_stride[d]; q.b_s[d] = g->b_stride[d]; }
        } else {                                                                   // level k - 1 -> level k
            const Level &from = plan.lv[k - 1];
            PoolGeo pg{from.H, from.W, g->C, l.H, l.W, {}, {}};
            const int64_t dense[4] = {(int64_t)from.H * from.W * g->C, (int64_t)from.W * g->C, g->C, 1};
            for (int d = 0; d < 4; ++d) { pg.a_s[d] = k == 1 ? g->a_stride[d] : dense[d]; pg.b_s[d] = k == 1 ? g->b_stride[d] : dense[d]; }
            const float *src_a = k == 1 ? a : pool_a + from.image_at, *src_b = k == 1 ? b : pool_b + from.image_at;
            const unsigned blocks = (unsigned)(((size_t)l.H * l.W * g->C + kBlock - 1) / kBlock);
            for (int b0 = 0; b0 < g->B; b0 += kMaxY) {
                hipLaunchKernelGGL(ms_pool_kernel, dim3(blocks, std::min(kMaxY, g->B - b0)), dim3(kBlock), 0, st, pg, src_a, src_b,
                                   pool_a + l.image_at, pool_b + l.image_at, b0);
                if (const int rc = tl_host::launched("ms_pool_kernel launch")) return rc;
            }
        }
        // ds is kept once: the kernel writes it through ds_a when a's maps are kept, through ds_b otherwise
        float *dm_a = maps.dm_a ? maps.dm_a + l.map_at : nullptr, *dm_b = maps.dm_b ? maps.dm_b + l.map_at : nullptr;
        float *ds = maps.ds ? maps.ds + l.map_at : nullptr, *dc = maps.dc ? maps.dc + l.map_at : nullptr;
        float *ds_a = dm_a ? ds : nullptr, *ds_b = dm_a ? nullptr : ds;
        for (int b0 = 0; b0 < g->B; b0 += kMaxY) {
            const dim3 grid((unsigned)l.tiles, std::min(kMaxY, g->B - b0));
            for_k(g->K, [&](auto kk) {
                constexpr int K = decltype(kk)::value;
                if (k < plan.M - 1)
                    hipLaunchKernelGGL((ssim_fwd_kernel<K, kCsChan>), grid, dim3(kBlock), lds, st, q, pa, pb, dm_a, ds_a, dm_b, ds_b, dc,
                                       part + l.part_at, b0);
                else
                    hipLaunchKernelGGL((ssim_fwd_kernel<K, kSsimChan>), grid, dim3(kBlock), lds, st, q, pa, pb, dm_a, ds_a, dm_b, ds_b, dc,
                                       part + l.part_at, b0);
            });
            if (const int rc = tl_host::launched("ssim_fwd_kernel launch (pyramid)")) return rc;
        }
    }
    hipLaunchKernelGGL(ms_finish_kernel, dim3((unsigned)g->B), dim3(kBlock), 0, st, fin, part, value, terms, factor);
    return tl_host::launched("ms_finish_kernel launch");
}

int tl_ms_ssim_bwd(const tl_ms_ssim_geom *g, const float *p, const float *q, const float *keep, size_t keep_elems,
                   const float *g_value, float *g_p, int which, void *work, size_t work_bytes_given, void *stream)
{
    const char *fn = "tl_ms_ssim_bwd";
    if (const char *what = ms_geom_fault(g)) return refuse(fn, what);
    if (!p) return refuse(fn, "p is NULL");
    if (!q) return refuse(fn, "q is NULL");
    if (!g_value) return refuse(fn, "g_value is NULL");
    if (!g_p) return refuse(fn, "g_p is NULL");
    if (which != 0 && which != 1) return refuse(fn, "which must be 0 (p is a) or 1 (p is b)");
    if (!(g->flags & (1 << which))) return refuse(fn, "which names an image whose maps flags did not keep");
    const Plan plan = make_plan(g);
    if (const char *what = ms_buffers_fault(plan, keep, keep_elems, work, work_bytes_given, "tl_ms_ssim_keep_elems", "tl_ms_ssim_work_bytes"))
        return refuse(fn, what);
    if (const int rc = tl_host::use_device(g->device)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const float *pool_a = keep + plan.factor_floats, *pool_b = pool_a + plan.image_floats;
    const float *pool_p = which ? pool_b : pool_a, *pool_q = which ? pool_a : pool_b;
    const Maps maps = maps_of(g, plan, const_cast<float *>(keep));
    const float *dm = which ? maps.dm_b : maps.dm_a;
    float *grads = (float *)work;                                                  // of the pooled images, levels 1 .. M - 1
    const size_t lds = (size_t)bwd_lds_floats(std::min(g->C, kCh)) * sizeof(float);
    for (int k = plan.M - 1; k >= 0; --k) {
        const Level &l = plan.lv[k];
        Geo geo = level_geo(g, l, l.W);
        const float *pp = pool_p + l.image_at, *qq = pool_q + l.image_at;
        float *out = grads + l.image_at;
        if (k == 0) {
            pp = p; qq = q; out = g_p;
            for (int d = 0; d < 4; ++d) { geo.a_s[d] = g->a_stride[d]; geo.b_s[d] = g->b_stride[d]; geo.g_s[d] = g->g_stride[d]; }
        }
        Pyramid pyr{(const double *)keep, nullptr, k, plan.M, 0, 0};
        if (k < plan.M - 1) {
            pyr.coarse = grads + plan.lv[k + 1].image_at;
            pyr.Hc = plan.lv[k + 1].H; pyr.Wc = plan.lv[k + 1].W;
        }
        const unsigned tiles = (unsigned)tiles_of(l.H, l.W);
        for (int b0 = 0; b0 < g->B; b0 += kMaxY) {
            const dim3 grid(tiles, std::min(kMaxY, g->B - b0));
            for_k(g->K, [&](auto kk) {
                hipLaunchKernelGGL((ssim_bwd_kernel<decltype(kk)::value, true>), grid, dim3(kBlock), lds, st, geo, pp, qq, dm + l.map_at,
                                   maps.ds + l.map_at, maps.dc + l.map_at, g_value, out, b0, pyr);
            });
            if (const int rc = tl_host::launched("ssim_bwd_kernel launch (pyramid)")) return rc;
        }
    }
    return TL_OK;
}

}  // extern "C"
