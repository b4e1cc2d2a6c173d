// tl_svola.hip -- the spatially varying overlap-add PSF convolution and its two adjoints (tl_svola_fwd, tl_svola_bwd_psf,
// tl_svola_bwd_image of include/tl_trace.h; imaging.svola_convolution(fused=True) stands on them).
//
//   out[b,y,x,c] = sum_n w_n(y + oh, x + ow) sum_{i,j} psfs[b,n,i,j,c] P[b, y + a - i, x + b - j, c]
//
// (P = the image under symmetric reflection, a = kh/2, b = kw/2, w_n = wr[i][r] wc[j][q] the normalised window of patch n).
// The patch edges cut the frame into cells inside which the set of covering patches is constant.  The host cuts every cell
// of the central H x W into tiles of <= 32 x 32 pixels; one block takes one tile of one (b, c), so the covering patches and
// with them every PSF tap are block-uniform: the taps are scalar loads, the tile plus its halo lives in LDS (the reflection
// is resolved in the index while loading, no padded image exists in memory), and a thread owns a column of 4 output rows so
// that one LDS read feeds 4 FMAs per covering patch.
// Forward:       one accumulator set per covering patch, out = sum_n w_n acc_n.
// Backward, PSF: same tiles; a thread owns taps (i, j) and sweeps the tile's pixels from LDS against w_n g_out of up to four
//                covering patches at a time; per-tile partials go to the workspace and svola_psf_reduce_kernel adds them in
//                a fixed order in fp64 and rounds once (no atomics: the same bits on every run).
// Backward, image: the correlation of w_n g_out with the PSFs on the frame extended by the halo, over plain 32 x 32 tiles
//                (the patches that reach into a tile's halo are block-uniform too; w_n is 0 outside its patch), then
//                svola_fold_kernel lets every image pixel gather its own value and those of its mirror images.
#include "tl_common.h"

#include <stdio.h>

#include <algorithm>
#include <vector>

namespace {

constexpr int kBlock = 256;
constexpr int kTile = 32;                       // tile edge, pixels
constexpr int kMaxK = 31;                       // PSF edge, taps
constexpr int kRows = kTile + kMaxK - 1;        // LDS image of a tile plus halo
constexpr int kPitch = kRows + 1;
constexpr int kMaxSeg = 96;                     // tile rows / columns per launch (kernel argument space)
constexpr int kMaxGrid = 128;                   // patches per axis
constexpr int kMaxZ = 65535;

// One tile edge along an axis: `len` pixels from `start`, covered by the patches lo .. lo + n - 1 of that axis.
struct Seg {
    int32_t start;
    uint16_t lo;
    uint8_t len, n;
};

struct Tiles { Seg rows[kMaxSeg], cols[kMaxSeg]; };

// Per patch row / column: the first tile edge it covers and how many (they are consecutive).
struct PatchSegs { uint16_t first_r[kMaxGrid], cnt_r[kMaxGrid], first_c[kMaxGrid], cnt_c[kMaxGrid]; };

struct Geo {
    int B, H, W, C, pb, gh, gw, kh, kw, oh, ow;
    int64_t im_s[4], psf_s[5], gpsf_s[5];
};

__device__ __forceinline__ float uload(const float *__restrict__ q, const int64_t i)
{
    return ((const __attribute__((address_space(4))) float *)(unsigned long long)q)[i];
}

__device__ __forceinline__ int reflect(int i, const int n)      // -1-i -> i, n+i -> n-1-i; clamped: never out of bounds
{
    i = i < 0 ? -1 - i : (i >= n ? 2 * n - 1 - i : i);
    return min(max(i, 0), n - 1);
}

// tile[r][q] = image[reflect(ys + r), reflect(xs + q)] for r < rows, q < cols
__device__ __forceinline__ void stage_image(float *__restrict__ tile, const float *__restrict__ img, const Geo &g, const int ys,
                                            const int xs, const int rows, const int cols)
{
    for (int e = threadIdx.x; e < rows * cols; e += kBlock) {
        const int r = e / cols, q = e - r * cols;
        tile[r * kPitch + q] = img[(int64_t)reflect(ys + r, g.H) * g.im_s[1] + (int64_t)reflect(xs + q, g.W) * g.im_s[2]];
    }
}

// acc[k] = sum_{i,j} psf[i][j] tile[ty + k + u(i)][tx + v(j)], k < 4:  FLIP: u = kh-1-i, v = kw-1-j (convolution);  else u = i,
// v = j (correlation).  The taps are wave-uniform scalar loads; the four rows slide down the column, one LDS read per tap.
template <bool FLIP>
__device__ __forceinline__ void conv4(const float *__restrict__ tile, const float *__restrict__ pk, const int64_t s_i,
                                      const int64_t s_j, const int kh, const int kw, const int ty, const int tx, float acc[4])
{
    acc[0] = acc[1] = acc[2] = acc[3] = 0.f;
    for (int v = 0; v < kw; ++v) {
        const float *__restrict__ col = tile + ty * kPitch + tx + v;
        const int64_t oj = (int64_t)(FLIP ? kw - 1 - v : v) * s_j;
        float w0 = col[0], w1 = col[kPitch], w2 = col[2 * kPitch];
        for (int u = 0; u < kh; ++u) {
            const float w3 = col[(u + 3) * kPitch];
            const float t = uload(pk, (int64_t)(FLIP ? kh - 1 - u : u) * s_i + oj);
            acc[0] = __builtin_fmaf(t, w0, acc[0]);
            acc[1] = __builtin_fmaf(t, w1, acc[1]);
            acc[2] = __builtin_fmaf(t, w2, acc[2]);
            acc[3] = __builtin_fmaf(t, w3, acc[3]);
            w0 = w1;
            w1 = w2;
            w2 = w3;
        }
    }
}

// grid (tile columns, tile rows, lenses of this launch x C)
__global__ __launch_bounds__(kBlock) void svola_fwd_kernel(const Geo g, const Tiles tl, const double *__restrict__ wr,
                                                           const double *__restrict__ wc, const float *__restrict__ image,
                                                           const float *__restrict__ psfs, float *__restrict__ out, const int b0)
{
    __shared__ float tile[kRows * kPitch];
    const Seg sy = tl.rows[blockIdx.y], sx = tl.cols[blockIdx.x];
    const int b = b0 + blockIdx.z / g.C, c = blockIdx.z % g.C;
    const int a = g.kh >> 1, hb = g.kw >> 1, th = sy.len, tw = sx.len, y0 = sy.start, x0 = sx.start;
    const int Ih = g.H + 2 * g.oh, Iw = g.W + 2 * g.ow;
    stage_image(tile, image + (int64_t)b * g.im_s[0] + (int64_t)c * g.im_s[3], g, y0 - a, x0 - hb, th + 2 * a, tw + 2 * hb);
    __syncthreads();
    const int tid = threadIdx.x, tx = tid % tw, ty = 4 * (tid / tw);
    if (ty >= th) return;
    float o[4] = {0.f, 0.f, 0.f, 0.f};
    const float *__restrict__ pb = psfs + (g.pb == 1 ? 0 : (int64_t)b * g.psf_s[0]) + (int64_t)c * g.psf_s[4];
    for (int pi = 0; pi < sy.n; ++pi) {
        for (int pj = 0; pj < sx.n; ++pj) {
            const int n = (sy.lo + pi) * g.gw + sx.lo + pj;
            float acc[4];
            conv4<true>(tile, pb + (int64_t)n * g.psf_s[1], g.psf_s[2], g.psf_s[3], g.kh, g.kw, ty, tx, acc);
            const double wq = wc[(size_t)(sx.lo + pj) * Iw + x0 + tx + g.ow];
            const double *__restrict__ wrow = wr + (size_t)(sy.lo + pi) * Ih + y0 + ty + g.oh;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (ty + k < th) o[k] = __builtin_fmaf((float)(wrow[k] * wq), acc[k], o[k]);
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (ty + k < th) out[(((size_t)b * g.H + y0 + ty + k) * g.W + x0 + tx) * g.C + c] = o[k];
}

// Same grid.  part [B C][N][slots][kh kw]: the slot of a tile within patch n is (its row among the tile rows the patch covers)
// x slots_c + (its column among the tile columns the patch covers).
__global__ __launch_bounds__(kBlock) void svola_bwd_psf_kernel(const Geo g, const Tiles tl, const PatchSegs ps,
                                                               const double *__restrict__ wr, const double *__restrict__ wc,
                                                               const float *__restrict__ image, const float *__restrict__ g_out,
                                                               float *__restrict__ part, const int b0, const int row_base,
                                                               const int col_base, const int slots_c, const int slots)
{
    __shared__ float tile[kRows * kPitch];
    __shared__ float4 wg[kTile * kTile];
    const Seg sy = tl.rows[blockIdx.y], sx = tl.cols[blockIdx.x];
    const int b = b0 + blockIdx.z / g.C, c = blockIdx.z % g.C;
    const int a = g.kh >> 1, hb = g.kw >> 1, th = sy.len, tw = sx.len, y0 = sy.start, x0 = sx.start;
    const int Ih = g.H + 2 * g.oh, Iw = g.W + 2 * g.ow, ntaps = g.kh * g.kw, N = g.gh * g.gw;
    const int tid = threadIdx.x, ncover = sy.n * sx.n;
    stage_image(tile, image + (int64_t)b * g.im_s[0] + (int64_t)c * g.im_s[3], g, y0 - a, x0 - hb, th + 2 * a, tw + 2 * hb);
    for (int m0 = 0; m0 < ncover; m0 += 4) {
        __syncthreads();
        for (int e = tid; e < th * tw; e += kBlock) {
            const int y = e / tw, x = e - y * tw;
            const float go = g_out[(((size_t)b * g.H + y0 + y) * g.W + x0 + x) * g.C + c];
            float v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int m = m0 + k;
                v[k] = 0.f;
                if (m < ncover) {
                    const int pi = sy.lo + m / sx.n, pj = sx.lo + m % sx.n;
                    v[k] = (float)(wr[(size_t)pi * Ih + y0 + y + g.oh] * wc[(size_t)pj * Iw + x0 + x + g.ow]) * go;
                }
            }
            wg[e] = make_float4(v[0], v[1], v[2], v[3]);
        }
        __syncthreads();
        for (int e = tid; e < ntaps; e += kBlock) {
            const int i = e / g.kw, j = e - i * g.kw;
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
            for (int y = 0; y < th; ++y) {
                const float *__restrict__ row = tile + (y + 2 * a - i) * kPitch + 2 * hb - j;
                const float4 *__restrict__ wrow = wg + y * tw;
                for (int x = 0; x < tw; ++x) {
                    const float p = row[x];
                    const float4 w = wrow[x];
                    acc[0] = __builtin_fmaf(w.x, p, acc[0]);
                    acc[1] = __builtin_fmaf(w.y, p, acc[1]);
                    acc[2] = __builtin_fmaf(w.z, p, acc[2]);
                    acc[3] = __builtin_fmaf(w.w, p, acc[3]);
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int m = m0 + k;
                if (m < ncover) {
                    const int pi = sy.lo + m / sx.n, pj = sx.lo + m % sx.n;
                    const int slot = (row_base + (int)blockIdx.y - ps.first_r[pi]) * slots_c
                                     + (col_base + (int)blockIdx.x - ps.first_c[pj]);
                    part[((((size_t)b * g.C + c) * N + pi * g.gw + pj) * slots + slot) * ntaps + e] = acc[k];
                }
            }
        }
    }
}

// g_psfs[bp,n,i,j,c] = sum over the lenses folded into bp and the tiles of patch n, fp64, fixed order, rounded once.
// grid (ceil(kh kw / 64), N, psf_batch C), 64 threads
__global__ __launch_bounds__(64) void svola_psf_reduce_kernel(const Geo g, const PatchSegs ps, const float *__restrict__ part,
                                                              float *__restrict__ g_psfs, const int slots_c, const int slots)
{
    const int ntaps = g.kh * g.kw, N = g.gh * g.gw;
    const int e = blockIdx.x * 64 + threadIdx.x, n = blockIdx.y, bp = blockIdx.z / g.C, c = blockIdx.z % g.C;
    if (e >= ntaps) return;
    const int nr = ps.cnt_r[n / g.gw], nc = ps.cnt_c[n % g.gw];
    const int fold = g.pb == 1 ? g.B : 1;
    double s = 0.0;
    for (int f = 0; f < fold; ++f) {
        const int b = g.pb == 1 ? f : bp;
        const float *__restrict__ p = part + ((((size_t)b * g.C + c) * N + n) * slots) * ntaps + e;
        for (int sr = 0; sr < nr; ++sr)
            for (int sc = 0; sc < nc; ++sc) s += (double)p[(size_t)(sr * slots_c + sc) * ntaps];
    }
    const int i = e / g.kw, j = e - i * g.kw;
    g_psfs[(int64_t)bp * g.gpsf_s[0] + (int64_t)n * g.gpsf_s[1] + (int64_t)i * g.gpsf_s[2] + (int64_t)j * g.gpsf_s[3]
           + (int64_t)c * g.gpsf_s[4]] = (float)s;
}

// ext [B C][H + 2a][W + 2b]: ext(e_r, e_c) = sum_n sum_{i,j} psfs[n,i,j] (w_n g_out)[e_r - a + i, e_c - b + j] for the extended
// image coordinates e_r in [-a, H + a), e_c in [-b, W + b).  Tiles are plain 32 x 32 pieces of that frame; Seg.start is the
// extended coordinate, Seg.lo / n the patches that reach the tile's halo.  grid as the forward's.
__global__ __launch_bounds__(kBlock) void svola_bwd_image_kernel(const Geo g, const Tiles tl, const double *__restrict__ wr,
                                                                 const double *__restrict__ wc, const float *__restrict__ psfs,
                                                                 const float *__restrict__ g_out, float *__restrict__ ext,
                                                                 const int b0)
{
    __shared__ float tile[kRows * kPitch];
    const Seg sy = tl.rows[blockIdx.y], sx = tl.cols[blockIdx.x];
    const int b = b0 + blockIdx.z / g.C, c = blockIdx.z % g.C;
    const int a = g.kh >> 1, hb = g.kw >> 1, th = sy.len, tw = sx.len, y0 = sy.start, x0 = sx.start;
    const int Ih = g.H + 2 * g.oh, Iw = g.W + 2 * g.ow, rows = th + 2 * a, cols = tw + 2 * hb;
    const int tid = threadIdx.x, tx = tid % tw, ty = 4 * (tid / tw);
    const float *__restrict__ pb = psfs + (g.pb == 1 ? 0 : (int64_t)b * g.psf_s[0]) + (int64_t)c * g.psf_s[4];
    float o[4] = {0.f, 0.f, 0.f, 0.f};
    for (int pi = sy.lo; pi < sy.lo + sy.n; ++pi) {
        for (int pj = sx.lo; pj < sx.lo + sx.n; ++pj) {
            __syncthreads();
            for (int e = tid; e < rows * cols; e += kBlock) {
                const int r = e / cols, q = e - r * cols;
                const int Y = y0 - a + r, X = x0 - hb + q;
                float v = 0.f;
                if (Y >= 0 && Y < g.H && X >= 0 && X < g.W) {
                    const double w = wr[(size_t)pi * Ih + Y + g.oh] * wc[(size_t)pj * Iw + X + g.ow];
                    if (w != 0.0) v = (float)w * g_out[(((size_t)b * g.H + Y) * g.W + X) * g.C + c];
                }
                tile[r * kPitch + q] = v;
            }
            __syncthreads();
            if (ty < th) {
                float acc[4];
                conv4<false>(tile, pb + (int64_t)(pi * g.gw + pj) * g.psf_s[1], g.psf_s[2], g.psf_s[3], g.kh, g.kw, ty, tx, acc);
#pragma unroll
                for (int k = 0; k < 4; ++k) o[k] += acc[k];
            }
        }
    }
    if (ty >= th) return;
    const int Eh = g.H + 2 * a, Ew = g.W + 2 * hb;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (ty + k < th) ext[(((size_t)b * g.C + c) * Eh + y0 + a + ty + k) * Ew + x0 + hb + tx] = o[k];
}

// g_image[b,y,x,c] = ext at (y, x) and at the mirror images of y (-1-y when y < a, 2H-1-y when y >= H-a) and of x, summed in
// a fixed order: the adjoint of the symmetric reflection as a gather.  One thread per element of [B,H,W,C].
__global__ __launch_bounds__(kBlock) void svola_fold_kernel(const Geo g, const float *__restrict__ ext, float *__restrict__ g_image,
                                                            const size_t total)
{
    const size_t e = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= total) return;
    const int a = g.kh >> 1, hb = g.kw >> 1, Eh = g.H + 2 * a, Ew = g.W + 2 * hb;
    const int c = (int)(e % g.C);
    const size_t px = e / g.C;
    const int x = (int)(px % g.W), y = (int)((px / g.W) % g.H), b = (int)(px / ((size_t)g.W * g.H));
    const int ry[3] = {y, -1 - y, 2 * g.H - 1 - y}, rx[3] = {x, -1 - x, 2 * g.W - 1 - x};
    const bool row_on[3] = {true, y < a, y >= g.H - a}, col_on[3] = {true, x < hb, x >= g.W - hb};
    const float *__restrict__ p = ext + ((size_t)b * g.C + c) * Eh * Ew;
    float s = 0.f;
#pragma unroll
    for (int u = 0; u < 3; ++u) {
#pragma unroll
        for (int v = 0; v < 3; ++v)
            if (row_on[u] && col_on[v]) s += p[(size_t)(ry[u] + a) * Ew + rx[v] + hb];
    }
    g_image[e] = s;
}

// ---------------------------------------------------------------------------------------------------------------- host

struct Plan {
    std::vector<Seg> rows, cols;            // tiles of the central H x W between the patch edges
    std::vector<Seg> erows, ecols;          // plain tiles of the extended frame (image backward)
    PatchSegs ps;
    int slots_r, slots_c;
    size_t psf_bytes, ext_bytes;
};

// The tile edges of one axis.  len = H (W), o = overlap, p0 / p1 [gn] = patch bounds in the frame.  False: a pixel of the
// centre lies in no patch.
bool cut_axis(int len, int o, int gn, const int32_t *p0, const int32_t *p1, std::vector<Seg> &segs, uint16_t *first, uint16_t *cnt)
{
    std::vector<int> lines = {o, o + len};
    for (int i = 0; i < gn; ++i) {
        if (p0[i] > o && p0[i] < o + len) lines.push_back(p0[i]);
        if (p1[i] > o && p1[i] < o + len) lines.push_back(p1[i]);
    }
    std::sort(lines.begin(), lines.end());
    lines.erase(std::unique(lines.begin(), lines.end()), lines.end());
    for (int i = 0; i < gn; ++i) first[i] = cnt[i] = 0;
    for (size_t k = 0; k + 1 < lines.size(); ++k) {
        const int s = lines[k], e = lines[k + 1];
        int lo = -1, hi = -1;
        for (int i = 0; i < gn; ++i)
            if (p0[i] <= s && p1[i] >= e) {
                if (lo < 0) lo = i;
                hi = i;
            }
        if (lo < 0) return false;
        const int pieces = (e - s + kTile - 1) / kTile;         // (<= 2^15 + 257 tile edges per axis: H, W <= 2^20, gh, gw <= 128)
        for (int q = 0; q < pieces; ++q) {
            const int t0 = s + (int)((int64_t)(e - s) * q / pieces), t1 = s + (int)((int64_t)(e - s) * (q + 1) / pieces);
            for (int i = lo; i <= hi; ++i) {
                if (!cnt[i]) first[i] = (uint16_t)segs.size();
                ++cnt[i];
            }
            segs.push_back(Seg{t0 - o, (uint16_t)lo, (uint8_t)(t1 - t0), (uint8_t)(hi - lo + 1)});
        }
    }
    return true;
}

// Plain tiles of [-halo, len + halo) with the patches whose rows meet the outputs [start - halo, start + n + halo) of a tile.
void cut_extended(int len, int o, int halo, int gn, const int32_t *p0, const int32_t *p1, std::vector<Seg> &segs)
{
    for (int s = -halo; s < len + halo; s += kTile) {
        const int n = std::min(kTile, len + halo - s);
        const int y_lo = std::max(s - halo, 0) + o, y_hi = std::min(s + n - 1 + halo, len - 1) + o;     // frame rows, inclusive
        int lo = -1, hi = -1;
        for (int i = 0; i < gn; ++i)
            if (p0[i] <= y_hi && p1[i] > y_lo) {
                if (lo < 0) lo = i;
                hi = i;
            }
        if (lo < 0) lo = hi = 0;
        segs.push_back(Seg{s, (uint16_t)lo, (uint8_t)n, (uint8_t)(hi - lo + 1)});
    }
}

const char *check_axis(int len, int o, int gn, const int32_t *p0, const int32_t *p1)
{
    const int pl = len / gn + 2 * o;
    for (int i = 0; i < gn; ++i) {
        if (p0[i] < 0 || p1[i] > len + 2 * o || p1[i] - p0[i] != pl) return "patch bounds outside the frame or not one patch long";
        if (i && p0[i] < p0[i - 1]) return "patch bounds decrease";
    }
    return nullptr;
}

// Everything that can be refused without a HIP call; fills the plan.
int make_plan(const char *fn, const tl_svola_geom *g, const int32_t *r0, const int32_t *r1, const int32_t *c0, const int32_t *c1,
              Plan &pl)
{
    static thread_local char msg[256];
    const char *arg = "", *what = nullptr;
    if (!g) what = "g is NULL";
    else if (!r0 || !r1 || !c0 || !c1) what = "r0, r1, c0 or c1 is NULL";
    else if (g->B < 1 || g->H < 1 || g->W < 1 || g->C < 1 || g->C > kMaxZ || g->H > (1 << 20) || g->W > (1 << 20))
        what = "B, H, W, C must be >= 1, C <= 65535 and H, W <= 2^20";
    else if (g->kh < 1 || g->kh > kMaxK || !(g->kh & 1)) what = "kh must be odd and <= 31";
    else if (g->kw < 1 || g->kw > kMaxK || !(g->kw & 1)) what = "kw must be odd and <= 31";
    else if (g->oh < 0 || g->oh + g->kh / 2 > g->H) what = "oh + kh/2 must not exceed H";
    else if (g->ow < 0 || g->ow + g->kw / 2 > g->W) what = "ow + kw/2 must not exceed W";
    else if (g->gh < 1 || g->gh > kMaxGrid || g->gw < 1 || g->gw > kMaxGrid) what = "gh and gw must be in 1..128";
    else if (g->psf_batch != 1 && g->psf_batch != g->B) what = "psf_batch must be 1 or B";
    else if ((what = check_axis(g->H, g->oh, g->gh, r0, r1))) arg = "r0/r1: ";
    else if ((what = check_axis(g->W, g->ow, g->gw, c0, c1))) arg = "c0/c1: ";
    else if (!cut_axis(g->H, g->oh, g->gh, r0, r1, pl.rows, pl.ps.first_r, pl.ps.cnt_r)) {
        arg = "r0/r1: ";
        what = "a row of the image lies in no patch";
    } else if (!cut_axis(g->W, g->ow, g->gw, c0, c1, pl.cols, pl.ps.first_c, pl.ps.cnt_c)) {
        arg = "c0/c1: ";
        what = "a column of the image lies in no patch";
    }
    if (what) {
        snprintf(msg, sizeof(msg), "%s: %s%s", fn, arg, what);
        return tl_host::fail(TL_EINVAL, msg);
    }
    cut_extended(g->H, g->oh, g->kh / 2, g->gh, r0, r1, pl.erows);
    cut_extended(g->W, g->ow, g->kw / 2, g->gw, c0, c1, pl.ecols);
    pl.slots_r = pl.slots_c = 1;
    for (int i = 0; i < g->gh; ++i) pl.slots_r = std::max<int>(pl.slots_r, pl.ps.cnt_r[i]);
    for (int j = 0; j < g->gw; ++j) pl.slots_c = std::max<int>(pl.slots_c, pl.ps.cnt_c[j]);
    pl.psf_bytes = (size_t)g->B * g->C * g->gh * g->gw * pl.slots_r * pl.slots_c * g->kh * g->kw * sizeof(float);
    pl.ext_bytes = (size_t)g->B * g->C * (g->H + 2 * (g->kh / 2)) * (g->W + 2 * (g->kw / 2)) * sizeof(float);
    return TL_OK;
}

Geo make_geo(const tl_svola_geom *g)
{
    Geo q;
    q.B = g->B; q.H = g->H; q.W = g->W; q.C = g->C; q.pb = g->psf_batch;
    q.gh = g->gh; q.gw = g->gw; q.kh = g->kh; q.kw = g->kw; q.oh = g->oh; q.ow = g->ow;
    for (int k = 0; k < 4; ++k) q.im_s[k] = g->image_stride[k];
    for (int k = 0; k < 5; ++k) { q.psf_s[k] = g->psfs_stride[k]; q.gpsf_s[k] = g->g_psfs_stride[k]; }
    return q;
}

// fn(tiles, row_base, col_base, n_rows, n_cols, b0, nb) launches one chunk of <= kMaxSeg x kMaxSeg tiles and <= 65535 / C
// lenses; every launch is checked as `what`
template <class F>
int for_chunks(const std::vector<Seg> &rows, const std::vector<Seg> &cols, int B, int C, const char *what, F fn)
{
    const int bmax = std::max(1, kMaxZ / C);
    Tiles tl;
    for (size_t rb = 0; rb < rows.size(); rb += kMaxSeg) {
        const int nr = (int)std::min<size_t>(kMaxSeg, rows.size() - rb);
        for (size_t cb = 0; cb < cols.size(); cb += kMaxSeg) {
            const int nc = (int)std::min<size_t>(kMaxSeg, cols.size() - cb);
            for (int k = 0; k < kMaxSeg; ++k) {
                tl.rows[k] = rows[rb + std::min(k, nr - 1)];
                tl.cols[k] = cols[cb + std::min(k, nc - 1)];
            }
            for (int b0 = 0; b0 < B; b0 += bmax) {
                fn(tl, (int)rb, (int)cb, nr, nc, b0, std::min(bmax, B - b0));
                if (const int rc = tl_host::launched(what)) return rc;
            }
        }
    }
    return TL_OK;
}

}  // namespace

extern "C" {

size_t tl_svola_workspace_bytes(const tl_svola_geom *g, const int32_t *r0, const int32_t *r1, const int32_t *c0, const int32_t *c1)
{
    Plan pl;
    if (make_plan("tl_svola_workspace_bytes", g, r0, r1, c0, c1, pl)) return 0;
    return std::max(pl.psf_bytes, pl.ext_bytes) + 256;
}

int tl_svola_fwd(const tl_svola_geom *g, const int32_t *r0, const int32_t *r1, const int32_t *c0, const int32_t *c1,
                 const double *wr, const double *wc, const float *image, const float *psfs, float *out, void *stream)
{
    Plan pl;
    const int rc = make_plan("tl_svola_fwd", g, r0, r1, c0, c1, pl);
    if (rc) return rc;
    if (!wr || !wc || !image || !psfs || !out) return tl_host::fail(TL_EINVAL, "tl_svola_fwd: wr, wc, image, psfs or out is NULL");
    if (const int rc = tl_host::use_device(g->device)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const Geo q = make_geo(g);
    return for_chunks(pl.rows, pl.cols, g->B, g->C, "svola_fwd_kernel launch",
                      [&](const Tiles &tl, int, int, int nr, int nc, int b0, int nb) {
        hipLaunchKernelGGL(svola_fwd_kernel, dim3(nc, nr, nb * g->C), dim3(kBlock), 0, st, q, tl, wr, wc, image, psfs, out, b0);
    });
}

int tl_svola_bwd_psf(const tl_svola_geom *g, const int32_t *r0, const int32_t *r1, const int32_t *c0, const int32_t *c1,
                     const double *wr, const double *wc, const float *image, const float *g_out, float *g_psfs,
                     void *workspace, size_t workspace_bytes, void *stream)
{
    Plan pl;
    int rc = make_plan("tl_svola_bwd_psf", g, r0, r1, c0, c1, pl);
    if (rc) return rc;
    if (!wr || !wc || !image || !g_out || !g_psfs)
        return tl_host::fail(TL_EINVAL, "tl_svola_bwd_psf: wr, wc, image, g_out or g_psfs is NULL");
    if (!workspace || workspace_bytes < pl.psf_bytes) return tl_host::fail(TL_EWORKSPACE, "workspace too small for tl_svola_bwd_psf");
    if ((rc = tl_host::use_device(g->device))) return rc;
    hipStream_t st = (hipStream_t)stream;
    const Geo q = make_geo(g);
    float *part = (float *)workspace;
    const int slots = pl.slots_r * pl.slots_c;
    rc = for_chunks(pl.rows, pl.cols, g->B, g->C, "svola_bwd_psf_kernel launch",
                    [&](const Tiles &tl, int rb, int cb, int nr, int nc, int b0, int nb) {
        hipLaunchKernelGGL(svola_bwd_psf_kernel, dim3(nc, nr, nb * g->C), dim3(kBlock), 0, st, q, tl, pl.ps, wr, wc, image, g_out,
                           part, b0, rb, cb, pl.slots_c, slots);
    });
    if (rc) return rc;
    const int ntaps = g->kh * g->kw, N = g->gh * g->gw;
    const int bmax = std::max(1, kMaxZ / g->C);
    for (int bp0 = 0; bp0 < g->psf_batch; bp0 += bmax) {            // (a lens of the batch per z only when psfs are per lens)
        const int nb = std::min(bmax, g->psf_batch - bp0);
        hipLaunchKernelGGL(svola_psf_reduce_kernel, dim3((ntaps + 63) / 64, N, nb * g->C), dim3(64), 0, st, q, pl.ps,
                           (const float *)part + (size_t)bp0 * g->C * N * slots * ntaps,
                           g_psfs + (int64_t)bp0 * g->g_psfs_stride[0], pl.slots_c, slots);
        if ((rc = tl_host::launched("svola_psf_reduce_kernel launch"))) return rc;
    }
    return TL_OK;
}

int tl_svola_bwd_image(const tl_svola_geom *g, const int32_t *r0, const int32_t *r1, const int32_t *c0, const int32_t *c1,
                       const double *wr, const double *wc, const float *psfs, const float *g_out, float *g_image,
                       void *workspace, size_t workspace_bytes, void *stream)
{
    Plan pl;
    int rc = make_plan("tl_svola_bwd_image", g, r0, r1, c0, c1, pl);
    if (rc) return rc;
    if (!wr || !wc || !psfs || !g_out || !g_image)
        return tl_host::fail(TL_EINVAL, "tl_svola_bwd_image: wr, wc, psfs, g_out or g_image is NULL");
    if (!workspace || workspace_bytes < pl.ext_bytes) return tl_host::fail(TL_EWORKSPACE, "workspace too small for tl_svola_bwd_image");
    if ((rc = tl_host::use_device(g->device))) return rc;
    hipStream_t st = (hipStream_t)stream;
    const Geo q = make_geo(g);
    float *ext = (float *)workspace;
    rc = for_chunks(pl.erows, pl.ecols, g->B, g->C, "svola_bwd_image_kernel launch",
                    [&](const Tiles &tl, int, int, int nr, int nc, int b0, int nb) {
        hipLaunchKernelGGL(svola_bwd_image_kernel, dim3(nc, nr, nb * g->C), dim3(kBlock), 0, st, q, tl, wr, wc, psfs, g_out, ext, b0);
    });
    if (rc) return rc;
    const size_t total = (size_t)g->B * g->H * g->W * g->C;
    const size_t blocks = (total + kBlock - 1) / kBlock;
    if (blocks > 0x7fffffffu) return tl_host::fail(TL_EINVAL, "tl_svola_bwd_image: the image has too many elements");
    hipLaunchKernelGGL(svola_fold_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, st, q, (const float *)ext, g_image, total);
    return tl_host::launched("svola_fold_kernel launch");
}

}  // extern "C"
