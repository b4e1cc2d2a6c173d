// tl_tfmtf.hip -- the geometric OTF of a traced fan at equally spaced focal planes, from one pass over the rays, and its seeds
// (tl_tfmtf_sums, tl_tfmtf_seed of include/tl_trace.h; metrics.otf_sums_through_focus / metrics.through_focus_mtf stand on them).
//
// Behind the last surface a ray is a line: at a plane shifted by d it lands at (x + d u, y + d v), u = cx / cz, v = cy / cz, so its
// phase there is a + d b.  Per row (f, w), over the LIVE rays (ok != 0 and s = 1 - cx^2 - cy^2 > 0, tl_focus_moments' rule), with
// the row's origin o, the frequency vectors (nu_x, nu_y)_j, the first shift d0 and the step dd:
//   cz = sqrt(s),  u = cx / cz,  v = cy / cz,  dx = x - o_x,  dy = y - o_y
//   a  = nu_x dx + nu_y dy                         cycles
//   b  = nu_x u  + nu_y v                          cycles per unit of shift
//   p0 = a + d0 b,  r0 = p0 - rint(p0),  (c_0, s_0) = sincospi(2 r0)        plane 0
//   q  = dd b,      rq = q - rint(q),    (cr, sr)   = sincospi(2 rq)        the rotor
//   (c_z, s_z) = (c_{z-1} cr - s_{z-1} sr,  s_{z-1} cr + c_{z-1} sr)        z = 1 .. Z - 1: plane z lies at d0 + z dd
//   sums[j, z] = (C_jz, S_jz) = (sum c_z, sum s_z)
// Every operation is in fp64 from the fp32 inputs and nothing is contracted (contract(off)): two sincospi per ray and frequency
// instead of Z, and no phase is ever rounded to fp32.  nu = 0 gives a = b = 0, the term (1, 0) and the rotor (1, 0): C = n and
// S = 0 at every plane without a rounding.  A dead ray is excluded by a select.  With d0 = 0 plane 0 is tl_mtf_sums' term, bit
// for bit (a + 0 b = a), and lanes, order, partials and reduce are the same: the same sums where the live rules agree.
//
// FORWARD.  Layout, plan, partials and the ordered reduce are the row frame's (tl_rows.h, the five-array walk).  A launch holds
// the 2 JB ZB running sums of JB vectors x ZB planes in a static register array; the buckets are ZB = 1 / 2 / 4 / 8 / 16 >= Z with
// JB = 1 / 2 / 4 / 8 / 16 >= J, at most 32 / ZB: up to 32 columns (64 fp64 sums).  J > JB goes in further launches back to back, each reading the rays
// again and starting at vector j0; every launch holds all Z planes, so a column's recurrence never depends on the bucket.  The
// rays of a lane are taken one at a time (a rolled loop: the sincospi bodies appear 2 JB times, not 8 JB times, in the code).
// Frequencies, d0 and dd travel by value in the kernel argument and are staged in LDS; nothing is uploaded.  A block's partial holds
// every launch's 2 JB ZB sums; tfmtf_reduce_kernel adds the partials of the slot an output element has, in block order.
// SEED.  One pass: the row's J Z seed pairs (gC, gS)_jz and the Z shifts d0 + z dd in LDS, plain loops over j and z that run the
// same recurrence.  Q_jz = gS c_z - gC s_z;  gx = 2 pi sum_j nu_xj sum_z Q_jz,  gu = 2 pi sum_j nu_xj sum_z (d0 + z dd) Q_jz,  gy, gv
// with nu_y; then gcx = (gu (1 - cy^2) + gv cx cy) / cz^3, gcy = (gu cx cy + gv (1 - cx^2)) / cz^3.  fp64, one rounding at the store.
#include "tl_rows.h"

#include <math.h>

namespace {

constexpr int kMaxJ = 16;                       // frequency vectors per call
constexpr int kMaxZ = 16;                       // focal planes per call
constexpr int kCols = 32;                       // (vector, plane) columns a launch holds in registers at the most
constexpr double kTwoPi = 6.283185307179586476925286766559;

struct Rays {
    const float *x, *y, *cx, *cy;
    const uint8_t *ok;
    int64_t s_f, s_p, s_w;
};

struct Freq { double nx[kMaxJ], ny[kMaxJ], d0, dd; };       // slots from J on hold 0; dd = 0 where Z = 1

struct Seeds { float *gx, *gy, *gcx, *gcy; };

constexpr int zb_of(int Z) { return Z <= 1 ? 1 : Z <= 2 ? 2 : Z <= 4 ? 4 : Z <= 8 ? 8 : 16; }
constexpr int jb_cap(int ZB) { return kCols / ZB > kMaxJ ? kMaxJ : kCols / ZB; }       // the vectors that fit beside ZB planes
// the vector bucket of a call: 1 / 2 / 4 / 8 / 16 >= J, at most jb_cap: a call of few vectors pays for no empty slots
constexpr int jb_of(int ZB, int J) { const int need = J <= 1 ? 1 : J <= 2 ? 2 : J <= 4 ? 4 : J <= 8 ? 8 : 16; return need < jb_cap(ZB) ? need : jb_cap(ZB); }
// doubles of one block's partial: every launch's 2 JB ZB sums
inline int partial_doubles(int J, int Z) { return (int)cdiv(J, jb_of(zb_of(Z), J)) * 2 * jb_of(zb_of(Z), J) * zb_of(Z); }

// what of a ray every frequency shares: the offsets from the origin, the slopes, whether it counts
struct Line { double dx, dy, u, v; bool live; };

__device__ __forceinline__ Line line_of(float xf, float yf, float cxf, float cyf, unsigned okb, double o_x, double o_y)
{
#pragma clang fp contract(off)
    const double cx = (double)cxf, cy = (double)cyf;
    const double s = 1.0 - cx * cx - cy * cy;
    const bool live = okb != 0u && s > 0.0;                 // (NaN > 0 is false)
    // a dead ray is the ray at 0 along the axis that is not counted: nothing of what it holds reaches a sum
    const double cz = sqrt(live ? s : 1.0);
    return {(live ? (double)xf : 0.0) - o_x, (live ? (double)yf : 0.0) - o_y, (live ? cx : 0.0) / cz, (live ? cy : 0.0) / cz, live};
}

// plane 0's term (c, s) and the rotor (cr, sr) of one ray and frequency vector
__device__ __forceinline__ void start(double nx, double ny, const Line &l, double d0, double dd, double *c, double *s, double *cr, double *sr)
{
#pragma clang fp contract(off)
    const double a = nx * l.dx + ny * l.dy;
    const double b = nx * l.u + ny * l.v;
    const double p0 = a + d0 * b;
    const double r0 = p0 - rint(p0);
    sincospi(2.0 * r0, s, c);
    const double q = dd * b;
    const double rq = q - rint(q);
    sincospi(2.0 * rq, sr, cr);
}

__device__ __forceinline__ void rotate(double &c, double &s, double cr, double sr)
{
#pragma clang fp contract(off)
    const double cn = c * cr - s * sr, sn = s * cr + c * sr;
    c = cn;
    s = sn;
}

// ray i of the one or four a lane holds, by selects: the loop over them stays rolled and indexes no register array
template <class T, int N>
__device__ __forceinline__ T pick(const T (&a)[N], int i)
{
    if constexpr (N == 1) return a[0];
    else return i == 0 ? a[0] : i == 1 ? a[1] : i == 2 ? a[2] : a[3];
}

// m[2 (jl ZB + z)], m[.. + 1] = (C, S) of vector j0 + jl at plane z over the block's rays
template <int JB, int ZB>
__global__ __launch_bounds__(kBlock) void tfmtf_sums_kernel(Rays r, int64_t P, int W, int row0, const double *__restrict__ origin,
                                                            Freq fq, int j0, double *__restrict__ part, int nbx, int R, int stride,
                                                            int base)
{
#pragma clang fp contract(off)
    const RowBase5 b = row_base5(r, W, row0);
    const double o_x = origin[2 * (int64_t)b.row], o_y = origin[2 * (int64_t)b.row + 1];
    const int64_t first = (int64_t)blockIdx.x * R * kChunk;
    const int64_t last = std::min(first + (int64_t)R * kChunk, P);
    __shared__ double nx[JB], ny[JB], sh[2];                // read wave-uniformly: a broadcast, no register between uses
    if ((int)threadIdx.x < JB) {
        nx[threadIdx.x] = fq.nx[j0 + threadIdx.x];          // (j0 + JB <= 16: JB divides 16 and j0 is a multiple of it; slots from J on hold 0)
        ny[threadIdx.x] = fq.ny[j0 + threadIdx.x];
    }
    if (threadIdx.x == 0) {
        sh[0] = fq.d0;
        sh[1] = fq.dd;
    }
    __syncthreads();
    double m[2 * JB * ZB];
#pragma unroll
    for (int k = 0; k < 2 * JB * ZB; ++k) m[k] = 0.0;
    const bool vec = r.s_p == 1 && aligned_row(b);
    walk_rays5(b, r.s_p, vec, first, last, P,
               [&](int64_t, const auto &xs, const auto &ys, const auto &cxs, const auto &cys, const auto &oks) {
        constexpr int N = sizeof(xs) / sizeof(xs[0]);
#pragma unroll 1
        for (int i = 0; i < N; ++i) {                       // one ray at a time, in ray order
            const Line l = line_of(pick(xs, i), pick(ys, i), pick(cxs, i), pick(cys, i), pick(oks, i), o_x, o_y);
#pragma unroll
            for (int j = 0; j < JB; ++j) {
                double c, s, cr, sr;
                start(nx[j], ny[j], l, sh[0], sh[1], &c, &s, &cr, &sr);
                // the select that excludes a dead ray, once: its rotor is (1, 0) (b = 0), so it adds +0.0 at every plane
                c = l.live ? c : 0.0;
                s = l.live ? s : 0.0;
#pragma unroll
                for (int z = 0; z < ZB; ++z) {
                    m[2 * (j * ZB + z)] += c;
                    m[2 * (j * ZB + z) + 1] += s;
                    if (z + 1 < ZB) rotate(c, s, cr, sr);
                }
                __builtin_amdgcn_sched_barrier(0);          // one vector per scheduling region: the next one's terms stay behind it
            }
        }
    });
    block_partial(m, part, b.row, nbx, 2 * JB * ZB, stride, base);
}

// sums[row, j, z, k] from the partial slot it has: launch j / JB, then (j % JB, z, k) at the bucket's plane stride ZB
__global__ __launch_bounds__(kBlock) void tfmtf_reduce_kernel(const double *__restrict__ part, double *__restrict__ out, int64_t total,
                                                              int nbx, int J, int Z, int JB, int ZB, int stride)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= total) return;
    const int n = 2 * J * Z;
    const int64_t row = i / n;
    const int e = (int)(i - row * n);
    const int j = e / (2 * Z), z = (e >> 1) % Z, k = e & 1;
    out[i] = reduce_slot(part, row, nbx, stride, (j / JB) * (2 * JB * ZB) + 2 * ((j % JB) * ZB + z) + k);
}

__global__ __launch_bounds__(kBlock) void tfmtf_seed_kernel(Rays r, int64_t P, int W, int row0, const double *__restrict__ origin,
                                                            Freq fq, int J, int Z, const double *__restrict__ g_sums, Seeds out, int R)
{
#pragma clang fp contract(off)
    const RowBase5 b = row_base5(r, W, row0);
    const double o_x = origin[2 * (int64_t)b.row], o_y = origin[2 * (int64_t)b.row + 1];
    float *__restrict__ gx = out.gx ? out.gx + b.off : nullptr, *__restrict__ gy = out.gy ? out.gy + b.off : nullptr;
    float *__restrict__ gcx = out.gcx ? out.gcx + b.off : nullptr, *__restrict__ gcy = out.gcy ? out.gcy + b.off : nullptr;
    // (no register array is indexed by j or z here: plain loops to J and Z)
    __shared__ double nx[kMaxJ], ny[kMaxJ], del[kMaxZ], sh[2], gC[kMaxJ * kMaxZ], gS[kMaxJ * kMaxZ];
    if ((int)threadIdx.x < J) {
        nx[threadIdx.x] = fq.nx[threadIdx.x];
        ny[threadIdx.x] = fq.ny[threadIdx.x];
    }
    if ((int)threadIdx.x < Z) del[threadIdx.x] = fq.d0 + (double)threadIdx.x * fq.dd;      // the plane's shift: a product, a sum
    if (threadIdx.x == 0) {
        sh[0] = fq.d0;
        sh[1] = fq.dd;
    }
    if ((int)threadIdx.x < J * Z) {                         // (J Z <= 256 lanes)
        gC[threadIdx.x] = g_sums[((int64_t)b.row * J * Z + threadIdx.x) * 2];
        gS[threadIdx.x] = g_sums[((int64_t)b.row * J * Z + threadIdx.x) * 2 + 1];
    }
    __syncthreads();
    const int64_t first = (int64_t)blockIdx.x * R * kChunk;
    const int64_t last = std::min(first + (int64_t)R * kChunk, P);
    // (a NULL output is aligned)
    const bool vec = r.s_p == 1 && aligned_row(b) && aligned_to(gx, 16) && aligned_to(gy, 16) && aligned_to(gcx, 16) && aligned_to(gcy, 16);
    walk_rays5(b, r.s_p, vec, first, last, P,
               [&](int64_t o, const auto &xs, const auto &ys, const auto &cxs, const auto &cys, const auto &oks) {
        constexpr int N = sizeof(xs) / sizeof(xs[0]);
        Line l[N];
        double ax[N], ay[N], au[N], av[N];
#pragma unroll
        for (int i = 0; i < N; ++i) {
            l[i] = line_of(xs[i], ys[i], cxs[i], cys[i], oks[i], o_x, o_y);
            ax[i] = ay[i] = au[i] = av[i] = 0.0;
        }
#pragma unroll 1
        for (int j = 0; j < J; ++j) {
            double c[N], s[N], cr[N], sr[N], aq[N], ad[N];
#pragma unroll
            for (int i = 0; i < N; ++i) {
                start(nx[j], ny[j], l[i], sh[0], sh[1], &c[i], &s[i], &cr[i], &sr[i]);
                aq[i] = ad[i] = 0.0;
                __builtin_amdgcn_sched_barrier(0);          // one ray per scheduling region: the lane masks of the next one's sincospi stay behind it
            }
#pragma unroll 1
            for (int z = 0; z < Z; ++z) {
                const double gc = gC[j * Z + z], gs = gS[j * Z + z], d = del[z];
#pragma unroll
                for (int i = 0; i < N; ++i) {
                    const double q = gs * c[i] - gc * s[i];
                    aq[i] += q;
                    ad[i] += d * q;
                    rotate(c[i], s[i], cr[i], sr[i]);       // (the one after the last plane is not used)
                }
            }
#pragma unroll
            for (int i = 0; i < N; ++i) {
                ax[i] += nx[j] * aq[i];
                ay[i] += ny[j] * aq[i];
                au[i] += nx[j] * ad[i];
                av[i] += ny[j] * ad[i];
            }
        }
        float ox[N], oy[N], ocx[N], ocy[N];
#pragma unroll
        for (int i = 0; i < N; ++i) {
            // the slopes' seeds pass to the cosines: du/dcx = (1 - cy^2) / cz^3, du/dcy = dv/dcx = cx cy / cz^3, dv/dcy = (1 - cx^2) / cz^3
            const double cx = l[i].live ? (double)cxs[i] : 0.0, cy = l[i].live ? (double)cys[i] : 0.0;
            const double cx2 = cx * cx, cy2 = cy * cy;
            const double cz = sqrt(1.0 - cx2 - cy2);
            const double cz3 = cz * cz * cz, cxy = cx * cy;
            const double gu = kTwoPi * au[i], gv = kTwoPi * av[i];
            ox[i] = l[i].live ? (float)(kTwoPi * ax[i]) : 0.0f;
            oy[i] = l[i].live ? (float)(kTwoPi * ay[i]) : 0.0f;
            ocx[i] = l[i].live ? (float)((gu * (1.0 - cy2) + gv * cxy) / cz3) : 0.0f;
            ocy[i] = l[i].live ? (float)((gu * cxy + gv * (1.0 - cx2)) / cz3) : 0.0f;
        }
        if constexpr (N == kVec) {
            if (gx) *reinterpret_cast<float4 *>(gx + o) = make_float4(ox[0], ox[1], ox[2], ox[3]);
            if (gy) *reinterpret_cast<float4 *>(gy + o) = make_float4(oy[0], oy[1], oy[2], oy[3]);
            if (gcx) *reinterpret_cast<float4 *>(gcx + o) = make_float4(ocx[0], ocx[1], ocx[2], ocx[3]);
            if (gcy) *reinterpret_cast<float4 *>(gcy + o) = make_float4(ocy[0], ocy[1], ocy[2], ocy[3]);
        } else {
            if (gx) gx[o] = ox[0];
            if (gy) gy[o] = oy[0];
            if (gcx) gcx[o] = ocx[0];
            if (gcy) gcy[o] = ocy[0];
        }
    });
}

struct Checked { int rc; Freq fq; };

// the argument check the calls share; `name` opens the message.  Sizes, pointers, the counts, then the frequency vectors and the
// shifts (host) into the kernel argument, then the workspace: everything before the first HIP call.
Checked check_call(const char *name, int64_t F, int64_t P, int64_t W, const Rays &r, const char *missing, const double *nu_x,
                   const double *nu_y, int J, double shift_first, double shift_step, int Z, const void *ws, size_t ws_bytes)
{
    Checked c = {TL_OK, {}};
    const char *what = nullptr;
    if (const char *bad = size_fault(F, P, W)) what = bad;
    else if (!r.x || !r.y || !r.cx || !r.cy || !r.ok) what = "x, y, cx, cy and ok are required";
    else if (missing) what = missing;
    else if (J < 1 || J > kMaxJ) what = "J must be 1 .. 16";
    else if (Z < 1 || Z > kMaxZ) what = "Z must be 1 .. 16";
    else if (!nu_x || !nu_y) what = "nu_x and nu_y (host) are required";
    for (int j = 0; j < J && !what; ++j) {
        if (!(std::isfinite(nu_x[j]) && std::isfinite(nu_y[j]))) what = "every frequency must be finite";
        c.fq.nx[j] = nu_x[j];
        c.fq.ny[j] = nu_y[j];
    }
    if (!what && !(std::isfinite(shift_first) && (Z == 1 || std::isfinite(shift_step)))) what = "shift_first and shift_step must be finite";
    c.fq.d0 = shift_first;
    c.fq.dd = Z == 1 ? 0.0 : shift_step;                    // one plane: the step is ignored
    c.rc = what ? refuse(name, what)
                : check_workspace(name, ws, ws_bytes, tl_tfmtf_workspace_bytes(F, P, W, J, Z), "tl_tfmtf_workspace_bytes");
    return c;
}

template <int JB, int ZB>
void launch_sums(dim3 grid, hipStream_t st, const Rays &r, int64_t P, int W, int row0, const double *origin, const Freq &fq, int j0,
                 double *part, const Plan &pl, int stride, int base)
{
    hipLaunchKernelGGL((tfmtf_sums_kernel<JB, ZB>), grid, dim3(kBlock), 0, st, r, P, W, row0, origin, fq, j0, part, pl.nbx, pl.R,
                       stride, base);
}

// the launcher of the bucket JB x ZB (JB <= jb_cap(ZB): only those are instantiated)
using SumsLauncher = void (*)(dim3, hipStream_t, const Rays &, int64_t, int, int, const double *, const Freq &, int, double *,
                              const Plan &, int, int);
template <int ZB>
SumsLauncher vector_bucket(int JB)
{
    if constexpr (jb_cap(ZB) >= 16) if (JB == 16) return launch_sums<16, ZB>;
    if constexpr (jb_cap(ZB) >= 8) if (JB == 8) return launch_sums<8, ZB>;
    if constexpr (jb_cap(ZB) >= 4) if (JB == 4) return launch_sums<4, ZB>;
    if (JB == 2) return launch_sums<2, ZB>;
    return launch_sums<1, ZB>;
}
SumsLauncher sums_launcher(int JB, int ZB)
{
    return ZB == 1 ? vector_bucket<1>(JB) : ZB == 2 ? vector_bucket<2>(JB) : ZB == 4 ? vector_bucket<4>(JB) : ZB == 8 ? vector_bucket<8>(JB)
                                                                                                          : vector_bucket<16>(JB);
}

}  // namespace

extern "C" {

size_t tl_tfmtf_workspace_bytes(int64_t F, int64_t P, int64_t W, int J, int Z)
{
    if (size_fault(F, P, W) || J < 1 || J > kMaxJ || Z < 1 || Z > kMaxZ) return 0;
    return (size_t)(F * W) * (size_t)row_plan(F * W, P).nbx * (size_t)partial_doubles(J, Z) * sizeof(double);
}

int tl_tfmtf_sums(int32_t device, int64_t F, int64_t P, int64_t W, const float *x, const float *y, const float *cx, const float *cy,
                  const uint8_t *ok, int64_t s_f, int64_t s_p, int64_t s_w, const double *origin, const double *nu_x,
                  const double *nu_y, int J, double shift_first, double shift_step, int Z, double *sums, void *workspace,
                  size_t workspace_bytes, void *stream)
{
    const Rays r = {x, y, cx, cy, ok, s_f, s_p, s_w};
    const Checked c = check_call("tl_tfmtf_sums", F, P, W, r, !origin ? "the origin pointer is NULL" : !sums ? "the sums pointer is NULL" : nullptr,
                                 nu_x, nu_y, J, shift_first, shift_step, Z, workspace, workspace_bytes);
    if (c.rc) return c.rc;
    if (const int rc = tl_host::use_device(device)) return rc;
    const int64_t rows = F * W;
    const Plan pl = row_plan(rows, P);
    hipStream_t st = (hipStream_t)stream;
    const int ZB = zb_of(Z), JB = jb_of(ZB, J), stride = partial_doubles(J, Z);
    for (int j0 = 0; j0 < J; j0 += JB) {                    // J > JB: further launches, each reading the rays again
        if (const int rc = launch_rows(rows, pl.nbx, "tfmtf_sums_kernel launch", [&](dim3 grid, int row0) {
                sums_launcher(JB, ZB)(grid, st, r, P, (int)W, row0, origin, c.fq, j0, (double *)workspace, pl, stride, (j0 / JB) * 2 * JB * ZB);
            }))
            return rc;
    }
    const int64_t total = rows * 2 * J * Z;
    hipLaunchKernelGGL(tfmtf_reduce_kernel, dim3((unsigned)cdiv(total, kBlock)), dim3(kBlock), 0, st, (const double *)workspace, sums,
                       total, pl.nbx, J, Z, JB, ZB, stride);
    return tl_host::launched("tfmtf_reduce_kernel launch");
}

int tl_tfmtf_seed(int32_t device, int64_t F, int64_t P, int64_t W, const float *x, const float *y, const float *cx, const float *cy,
                  const uint8_t *ok, int64_t s_f, int64_t s_p, int64_t s_w, const double *origin, const double *nu_x,
                  const double *nu_y, int J, double shift_first, double shift_step, int Z, const double *g_sums, float *gx, float *gy,
                  float *gcx, float *gcy, void *workspace, size_t workspace_bytes, void *stream)
{
    const Rays r = {x, y, cx, cy, ok, s_f, s_p, s_w};
    const Checked c = check_call("tl_tfmtf_seed", F, P, W, r, !origin ? "the origin pointer is NULL" : !g_sums ? "the g_sums pointer is NULL" :
                                 !gx && !gy && !gcx && !gcy ? "gx, gy, gcx and gcy are all NULL" : nullptr, nu_x, nu_y, J, shift_first,
                                 shift_step, Z, workspace, workspace_bytes);
    if (c.rc) return c.rc;
    if (const int rc = tl_host::use_device(device)) return rc;
    const Plan pl = row_plan(F * W, P);
    const Seeds out = {gx, gy, gcx, gcy};
    return launch_rows(F * W, pl.nbx, "tfmtf_seed_kernel launch", [&](dim3 grid, int row0) {
        hipLaunchKernelGGL(tfmtf_seed_kernel, grid, dim3(kBlock), 0, (hipStream_t)stream, r, P, (int)W, row0, origin, c.fq, J, Z, g_sums,
                           out, pl.R);
    });
}

}  // extern "C"
