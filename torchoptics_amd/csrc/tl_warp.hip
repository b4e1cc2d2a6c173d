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
// The gradient to the image is a scatter and is not a kernel here.
#include "tl_common.h"

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
    hipError_t e = hipSetDevice(g->device);
    if (e != hipSuccess) return tl_host::hip_fail(e, "hipSetDevice");
    hipStream_t st = (hipStream_t)stream;
    const Geo q = make_geo(g);
    const unsigned blocks = (unsigned)(((int64_t)g->Ho * g->Wo + kBlock - 1) / kBlock);
    for (int b0 = 0; b0 < g->B; b0 += kMaxY) {
        hipLaunchKernelGGL(warp_fwd_kernel, dim3(blocks, std::min(kMaxY, g->B - b0)), dim3(kBlock), 0, st, q, image, x, y, gain, out, b0);
        const int herr = (int)hipGetLastError();
        if (herr) return tl_host::hip_fail(herr, "warp_fwd_kernel launch");
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
    hipError_t e = hipSetDevice(g->device);
    if (e != hipSuccess) return tl_host::hip_fail(e, "hipSetDevice");
    hipStream_t st = (hipStream_t)stream;
    const Geo q = make_geo(g);
    const unsigned blocks = (unsigned)(((int64_t)g->Ho * g->Wo + kBlock - 1) / kBlock);
    const bool in_lane = g->B > 1 && ((g_x && g->coord_batch == 1) || (g_gain && g->gain_batch == 1));
    if (in_lane) {                                  // something is shared by the batch: the lane sums over the lenses
        hipLaunchKernelGGL(warp_bwd_kernel, dim3(blocks, 1), dim3(kBlock), 0, st, q, image, x, y, gain, g_out, g_x, g_y, g_gain, 0, g->B);
        const int herr = (int)hipGetLastError();
        if (herr) return tl_host::hip_fail(herr, "warp_bwd_kernel launch");
        return TL_OK;
    }
    for (int b0 = 0; b0 < g->B; b0 += kMaxY) {
        hipLaunchKernelGGL(warp_bwd_kernel, dim3(blocks, std::min(kMaxY, g->B - b0)), dim3(kBlock), 0, st, q, image, x, y, gain, g_out,
                           g_x, g_y, g_gain, b0, 1);
        const int herr = (int)hipGetLastError();
        if (herr) return tl_host::hip_fail(herr, "warp_bwd_kernel launch");
    }
    return TL_OK;
}

}  // extern "C"
