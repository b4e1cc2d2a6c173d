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

// grid (tiles of the map, lenses of this launch); dynamic LDS = fwd_lds_floats(min(C, 4)) floats
template <int K>
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
                            ds_a[at] = ds;
                        }
                        if (dm_b) {
                            dm_b[at] = (t * mua - u * mub) - 2.f * mub * ds - mua * dcv;
                            ds_b[at] = ds;
                        }
                    }
                }
            }
            __syncthreads();                                                   // hbuf is rewritten by the next channel
        }
    }
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

// grid (tiles of the image, lenses of this launch); dynamic LDS = bwd_lds_floats(min(C, 4)) floats
template <int K>
__global__ __launch_bounds__(kBlock) void ssim_bwd_kernel(const Geo g, const float *__restrict__ p, const float *__restrict__ q,
                                                          const float *__restrict__ dm, const float *__restrict__ ds,
                                                          const float *__restrict__ dc, const float *__restrict__ g_value,
                                                          float *__restrict__ g_p, const int b0)
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
    const float scale = (float)((double)g_value[lens] / ((double)g.Hm * (double)g.Wm * (double)g.C));
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
            float pv[2] = {0.f, 0.f}, qv[2] = {0.f, 0.f};
#pragma unroll
            for (int half = 0; half < 2; ++half)
                if (vx < tw && vy + half < th) {
                    const int64_t y = y0 + vy + half, x = x0 + vx, ch = c0 + c;
                    pv[half] = p[(int64_t)lens * g.a_s[0] + y * g.a_s[1] + x * g.a_s[2] + ch * g.a_s[3]];
                    qv[half] = q[(int64_t)lens * g.b_s[0] + y * g.b_s[1] + x * g.b_s[2] + ch * g.b_s[3]];
                }
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
            hipLaunchKernelGGL(ssim_fwd_kernel<decltype(k)::value>, grid, dim3(kBlock), lds, st, q, a, b, ma, sa, mb, sb, cc, part, b0);
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
            hipLaunchKernelGGL(ssim_bwd_kernel<decltype(k)::value>, grid, dim3(kBlock), lds, st, geo, p, q, dm, ds, dc, g_value, g_p, b0);
        });
        if (const int rc = tl_host::launched("ssim_bwd_kernel launch")) return rc;
    }
    return TL_OK;
}

}  // extern "C"
