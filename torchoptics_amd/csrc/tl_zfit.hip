// tl_zfit.hip -- the Zernike wavefront fit of a traced fan from its transverse ray errors (tl_zfit_moments, tl_zfit_solve,
// tl_zfit_seed of include/tl_trace.h; metrics.zernike_moments / metrics.zernike_fit stand on them).
//
// The transverse ray error is the gradient of the wavefront over the pupil, so the Zernike coefficients a of W follow from the
// linear least-squares fit of the spot (x, y) against the gradients of the Noll-indexed polynomials Z_2 .. Z_{J+1} (orthonormal
// over the unit disc, order <= N, J = (N+1)(N+2)/2 - 1) at every ray's pupil coordinates (p, q): the normal equations G a = b with
//   G_jk = sum grad Z_j . grad Z_k,      b_j = sum x dZ_j/dp + y dZ_j/dq            over the LIVE rays (ok != 0).
// The Z_j are polynomials in (p, q), so G and b are linear in the monomial sums
//   mu_ab = sum p^a q^b (a + b <= 2N - 2),   xi_ab = sum x p^a q^b,  eta_ab = sum y p^a q^b (a + b <= N - 1),   sum x^2, sum y^2:
// K(N) = 3 N^2 + 2 per row, formed in fp64 from the fp32 inputs, uncontracted (contract(off)): p^0 = 1, p^k = p^(k-1) p, a term is
// (p^a q^b) and then times x, so a ray's terms have the bits of the definition in any IEEE fp64 arithmetic and only the ORDER of
// the sums is this file's.  Triangle index of (a, b): tri = (a + b)(a + b + 1) / 2 + b; a row's K sums are mu, xi, eta, sum x^2,
// sum y^2 in that order.
//
// MOMENTS.  zfit_moments_kernel<N, PART>: layout, plan, partials and reduce are the row frame's (tl_rows.h).
// PART 0 holds all K accumulators (order 5: 77 of them in 230 VGPRs, two waves per SIMD); order 6 goes as PART 1 (the 66 mu) and
// PART 2 (xi, eta, sum x^2, sum y^2: 44) in two launches, as 110 fp64 accumulators would leave one wave per SIMD.  The pupil coordinates have a stride triple of their own (0 over f and w
// for a shared pupil).
// SOLVE.  zfit_factor_kernel<N>: one wave per row, fp64, LDS.  G_m and b_m over the monomials of degree 1 .. N from the moments,
// G' = C^T G_m C and b' = C^T b_m with C the INTEGER monomial coefficients of the unnormalised Z_j (a constexpr table from the
// closed form; the Noll norms sqrt(n + 1), sqrt(2 (n + 1)) cancel in the scaled system and enter the coefficients at the end),
// G^ = D'^-1/2 G' D'^-1/2, its Cholesky factor in natural order, the validity rule (2n >= J, every D' > 0, every pivot -- the
// value whose root is the factor's diagonal -- above 2^-30), a = G^-1 b, q = sum (x^2 + y^2) - b . a.  zfit_adjoint_kernel<N>
// solves the backward's system from the stored factor and turns b_bar into the monomial coefficients the seed kernel evaluates.
// SEED.  zfit_seed_kernel<N>: one lane per four rays, the row's J + 1 numbers read once, the two polynomials by Horner in fp64,
// one rounding to fp32 at the store.  Dead rays and invalid rows get zeros.
#include "tl_rows.h"

namespace {

constexpr int kMinN = 2, kMaxN = 6, kMaxJ = 27;
constexpr double kPivotFloor = 9.313225746154785e-10;       // 2^-30 (ZFIT_PIVOT_FLOOR)

constexpr int n_coef(int N) { return (N + 1) * (N + 2) / 2 - 1; }
constexpr int n_mu(int N) { return N * (2 * N - 1); }          // a + b <= 2N - 2
constexpr int n_xi(int N) { return N * (N + 1) / 2; }          // a + b <= N - 1
constexpr int n_mom(int N) { return 3 * N * N + 2; }
__host__ __device__ constexpr int tri(int a, int b) { return (a + b) * (a + b + 1) / 2 + b; }

// The integer monomial coefficients of the unnormalised Zernike polynomials j = 2 .. 28 (Noll), the squares of their norms and
// the exponents of the monomials of degree 1 .. 6 (degree-major, b ascending: index tri(a, b) - 1).  Order N uses the leading
// n_coef(N) rows and columns.
struct ZTable {
    int c[kMaxJ][kMaxJ];                        // c[monomial][j - 2]
    int norm2[kMaxJ];
    int ea[kMaxJ], eb[kMaxJ];
};

constexpr int fact(int n) { return n <= 1 ? 1 : n * fact(n - 1); }
constexpr int binom(int n, int k) { return fact(n) / (fact(k) * fact(n - k)); }

constexpr ZTable make_table()
{
    ZTable t{};
    for (int d = 1; d <= kMaxN; ++d)
        for (int b = 0; b <= d; ++b) { t.ea[tri(d - b, b) - 1] = d - b; t.eb[tri(d - b, b) - 1] = b; }
    for (int j = 2; j <= kMaxJ + 1; ++j) {
        int n = 0;
        while ((n + 1) * (n + 2) / 2 < j) ++n;
        const int k = j - n * (n + 1) / 2;
        const int m = n % 2 == 0 ? 2 * (k / 2) : 2 * ((k - 1) / 2) + 1;
        const bool sine = m != 0 && j % 2 == 1;
        t.norm2[j - 2] = m == 0 ? n + 1 : 2 * (n + 1);
        for (int s = 0; s <= (n - m) / 2; ++s) {
            const int rc = (s % 2 ? -1 : 1) * fact(n - s) / (fact(s) * fact((n + m) / 2 - s) * fact((n - m) / 2 - s));
            const int tt = (n - m) / 2 - s;     // rho^(m + 2 tt) cos / sin (m theta) = (p^2 + q^2)^tt Re / Im (p + i q)^m
            for (int u = 0; u <= tt; ++u)
                for (int h = sine ? 1 : 0; h <= m; h += 2) {
                    const int a = 2 * (tt - u) + m - h, b = 2 * u + h;
                    if (a + b == 0) continue;
                    t.c[tri(a, b) - 1][j - 2] += rc * binom(tt, u) * binom(m, h) * ((h / 2) % 2 ? -1 : 1);
                }
        }
    }
    return t;
}

__device__ const ZTable kZ = make_table();

struct Rays {
    const float *x, *y;
    const uint8_t *ok;
    int64_t s_f, s_p, s_w;
    const float *px, *py;
    int64_t ps_f, ps_p, ps_w;
};

// accumulators and first moment of a part: 0 all, 1 the mu, 2 xi, eta, sum x^2, sum y^2
constexpr int part_size(int N, int part) { return part == 0 ? n_mom(N) : part == 1 ? n_mu(N) : n_mom(N) - n_mu(N); }
constexpr int part_base(int N, int part) { return part == 2 ? n_mu(N) : 0; }

// the terms of one ray, added to m
template <int N, int PART>
__device__ __forceinline__ void add_ray(double (&m)[part_size(N, PART)], float xf, float yf, float pf, float qf, unsigned okb)
{
#pragma clang fp contract(off)
    const bool live = okb != 0u;
    // a dead ray is the ray (0, 0) at the pupil's centre that is not counted: every term +0.0, whatever its coordinates hold
    const double x = live ? (double)xf : 0.0, y = live ? (double)yf : 0.0;
    const double p = live ? (double)pf : 0.0, q = live ? (double)qf : 0.0;
    constexpr int D = PART == 2 ? N : 2 * N - 1;            // powers 0 .. D - 1
    double pp[D], qq[D];
    pp[0] = qq[0] = 1.0;
#pragma unroll
    for (int k = 1; k < D; ++k) { pp[k] = pp[k - 1] * p; qq[k] = qq[k - 1] * q; }
    if (PART != 2) {
        m[0] += live ? 1.0 : 0.0;
#pragma unroll
        for (int d = 1; d <= 2 * N - 2; ++d)
#pragma unroll
            for (int b = 0; b <= d; ++b) m[tri(d - b, b)] += pp[d - b] * qq[b];
    }
    if (PART != 1) {
        constexpr int o = PART == 0 ? n_mu(N) : 0;
#pragma unroll
        for (int d = 0; d <= N - 1; ++d)
#pragma unroll
            for (int b = 0; b <= d; ++b) {
                const double t = pp[d - b] * qq[b];
                m[o + tri(d - b, b)] += t * x;
                m[o + n_xi(N) + tri(d - b, b)] += t * y;
            }
        m[o + 2 * n_xi(N)] += x * x;
        m[o + 2 * n_xi(N) + 1] += y * y;
    }
}

template <int N, int PART>
__global__ __launch_bounds__(kBlock) void zfit_moments_kernel(Rays r, int64_t P, int W, int row0, double *__restrict__ part, int nbx,
                                                              int R)
{
    constexpr int KP = part_size(N, PART);
    const int row = row0 + (int)blockIdx.y;
    const int f = row / W, w = row - f * W;
    const int64_t off = f * r.s_f + w * r.s_w, poff = f * r.ps_f + w * r.ps_w;
    const float *__restrict__ x = r.x + off, *__restrict__ y = r.y + off;
    const float *__restrict__ px = r.px + poff, *__restrict__ py = r.py + poff;
    const uint8_t *__restrict__ ok = r.ok + off;
    const int64_t first = (int64_t)blockIdx.x * R * kChunk;
    const int64_t last = std::min(first + (int64_t)R * kChunk, P);
    double m[KP];
#pragma unroll
    for (int j = 0; j < KP; ++j) m[j] = 0.0;
    const bool vec = r.s_p == 1 && r.ps_p == 1 && aligned_to(x, 16) && aligned_to(y, 16) && aligned_to(px, 16) && aligned_to(py, 16)
                     && aligned_to(ok, 4);
    if (vec) {                                              // (uniform over the block)
        for (int64_t ip = first + kVec * (int64_t)threadIdx.x; ip < last; ip += kChunk) {
            if (ip + kVec <= P) {
                const float4 x4 = *reinterpret_cast<const float4 *>(x + ip), y4 = *reinterpret_cast<const float4 *>(y + ip);
                const float4 p4 = *reinterpret_cast<const float4 *>(px + ip), q4 = *reinterpret_cast<const float4 *>(py + ip);
                const unsigned o4 = *reinterpret_cast<const unsigned *>(ok + ip);
                add_ray<N, PART>(m, x4.x, y4.x, p4.x, q4.x, o4 & 0xffu);
                add_ray<N, PART>(m, x4.y, y4.y, p4.y, q4.y, o4 & 0xff00u);
                add_ray<N, PART>(m, x4.z, y4.z, p4.z, q4.z, o4 & 0xff0000u);
                add_ray<N, PART>(m, x4.w, y4.w, p4.w, q4.w, o4 & 0xff000000u);
            } else {                                        // the last one to three rays of the row
                for (int64_t i = ip; i < P; ++i) add_ray<N, PART>(m, x[i], y[i], px[i], py[i], ok[i]);
            }
        }
    } else {
        for (int64_t ip = first + threadIdx.x; ip < last; ip += kBlock) {
            const int64_t o = ip * r.s_p, po = ip * r.ps_p;
            add_ray<N, PART>(m, x[o], y[o], px[po], py[po], ok[o]);
        }
    }
    block_partial(m, part, row, nbx, KP, n_mom(N), part_base(N, PART));
}

__global__ __launch_bounds__(kBlock) void zfit_reduce_kernel(const double *__restrict__ part, double *__restrict__ moments,
                                                             int64_t total, int nbx, int K)
{
    reduce_rows(part, moments, total, nbx, K);
}

// ------------------------------------------------------------------------------------------------------------------ the solve
// L L^T s = t in place in s (J entries in LDS), by one lane; L is the lower triangle of the J x J array
template <int J>
__device__ __forceinline__ void chol_solve(const double *L, double *s)
{
#pragma clang fp contract(off)
    #pragma unroll 1
    for (int i = 0; i < J; ++i) {
        double v = s[i];
        #pragma unroll 1
        for (int k = 0; k < i; ++k) v -= L[i * J + k] * s[k];
        s[i] = v / L[i * J + i];
    }
    #pragma unroll 1
    for (int i = J - 1; i >= 0; --i) {
        double v = s[i];
        #pragma unroll 1
        for (int k = i + 1; k < J; ++k) v -= L[k * J + i] * s[k];
        s[i] = v / L[i * J + i];
    }
}

// factor[row]: the J x J scaled Cholesky factor (lower triangle), then the J numbers 1 / (norm_j sqrt(D'_j))
template <int N>
__global__ __launch_bounds__(64) void zfit_factor_kernel(const double *__restrict__ moments, int64_t row0, double *__restrict__ a_out,
                                                         double *__restrict__ q_out, uint8_t *__restrict__ valid_out,
                                                         double *__restrict__ factor)
{
#pragma clang fp contract(off)
    constexpr int J = n_coef(N), K = n_mom(N);
    __shared__ double mom[K], A[J * J], H[J * J], bm[J], s[J], isd[J];
    const int64_t row = row0 + blockIdx.x;
    const int tid = threadIdx.x;
    #pragma unroll 1
    for (int i = tid; i < K; i += 64) mom[i] = moments[row * K + i];
    __syncthreads();
    #pragma unroll 1
    for (int e = tid; e < J * J; e += 64) {                  // G_m over the monomials
        const int i = e / J, k = e - i * J;
        const int a = kZ.ea[i], b = kZ.eb[i], c = kZ.ea[k], d = kZ.eb[k];
        double v = 0.0;
        if (a * c) v += (double)(a * c) * mom[tri(a + c - 2, b + d)];
        if (b * d) v += (double)(b * d) * mom[tri(a + c, b + d - 2)];
        A[e] = v;
    }
    if (tid < J) {                                           // b_m
        const int a = kZ.ea[tid], b = kZ.eb[tid];
        double v = 0.0;
        if (a) v += (double)a * mom[n_mu(N) + tri(a - 1, b)];
        if (b) v += (double)b * mom[n_mu(N) + n_xi(N) + tri(a, b - 1)];
        bm[tid] = v;
    }
    __syncthreads();
    #pragma unroll 1
    for (int e = tid; e < J * J; e += 64) {                  // H = G_m C
        const int i = e / J, j = e - i * J;
        double v = 0.0;
        #pragma unroll 1
        for (int k = 0; k < J; ++k) v += A[i * J + k] * (double)kZ.c[k][j];
        H[e] = v;
    }
    if (tid < J) {                                           // b' = C^T b_m
        double v = 0.0;
        #pragma unroll 1
        for (int i = 0; i < J; ++i) v += (double)kZ.c[i][tid] * bm[i];
        s[tid] = v;
    }
    __syncthreads();
    #pragma unroll 1
    for (int e = tid; e < J * J; e += 64) {                  // G' = C^T H
        const int j = e / J, l = e - j * J;
        double v = 0.0;
        #pragma unroll 1
        for (int i = 0; i < J; ++i) v += (double)kZ.c[i][j] * H[i * J + l];
        A[e] = v;
    }
    __syncthreads();
    bool good = 2.0 * mom[0] >= (double)J;                   // 2n equations for J unknowns: fewer leave G singular, whatever rounding says
    #pragma unroll 1
    for (int j = 0; j < J; ++j) good = good && A[j * J + j] > 0.0;          // (NaN > 0 is false)
    if (tid < J) isd[tid] = good ? 1.0 / sqrt(A[tid * J + tid]) : 1.0;
    __syncthreads();
    #pragma unroll 1
    for (int e = tid; e < J * J; e += 64) {                  // G^ = D'^-1/2 G' D'^-1/2, the identity for a row that is out already
        const int j = e / J, l = e - j * J;
        H[e] = good ? A[e] * isd[j] * isd[l] : (j == l ? 1.0 : 0.0);
    }
    if (tid < J) s[tid] *= isd[tid];
    __syncthreads();
    #pragma unroll 1
    for (int k = 0; k < J; ++k) {                            // Cholesky, natural order, in place in H (lower triangle)
        const double piv = H[k * J + k];
        const bool fine = piv > kPivotFloor;
        good = good && fine;
        const double lkk = sqrt(fine ? piv : 1.0);
        __syncthreads();
        #pragma unroll 1
        for (int i = k + tid; i < J; i += 64) H[i * J + k] = i == k ? lkk : H[i * J + k] / lkk;
        __syncthreads();
        const int n = J - 1 - k;                             // the trailing lower triangle
        #pragma unroll 1
        for (int e = tid; e < n * n; e += 64) {
            const int i = k + 1 + e / n, j = k + 1 + e % n;
            if (j <= i) H[i * J + j] -= H[i * J + k] * H[j * J + k];
        }
        __syncthreads();
    }
    if (tid < J) bm[tid] = s[tid];                           // b^ kept for b . a
    __syncthreads();
    if (tid == 0) chol_solve<J>(H, s);
    __syncthreads();
    if (tid < J) {
        isd[tid] = isd[tid] / sqrt((double)kZ.norm2[tid]);
        a_out[row * J + tid] = good ? s[tid] * isd[tid] : 0.0;
        factor[row * (J * J + J) + J * J + tid] = isd[tid];
    }
    #pragma unroll 1
    for (int e = tid; e < J * J; e += 64) factor[row * (J * J + J) + e] = H[e];
    if (tid == 0) {
        double v = 0.0;
        #pragma unroll 1
        for (int j = 0; j < J; ++j) v += bm[j] * s[j];
        q_out[row] = good ? mom[K - 2] + mom[K - 1] - v : 0.0;          // q = sum (x^2 + y^2) - b . a
        valid_out[row] = good ? 1 : 0;
    }
}

// coef[row]: the J monomial coefficients of sum_j b_bar_j Z_j, then 2 q_bar; zeros for an invalid row
template <int N>
__global__ __launch_bounds__(64) void zfit_adjoint_kernel(const double *__restrict__ factor, const double *__restrict__ a,
                                                          const uint8_t *__restrict__ valid, const double *__restrict__ g_a,
                                                          const double *__restrict__ g_q, int64_t row0, double *__restrict__ coef)
{
#pragma clang fp contract(off)
    constexpr int J = n_coef(N);
    __shared__ double L[J * J], s[J], isd[J];
    const int64_t row = row0 + blockIdx.x;
    const int tid = threadIdx.x;
    const bool good = valid[row] != 0;
    const double gq = g_q[row];
    #pragma unroll 1
    for (int e = tid; e < J * J; e += 64) L[e] = good ? factor[row * (J * J + J) + e] : (e / J == e % J ? 1.0 : 0.0);
    if (tid < J) {
        isd[tid] = good ? factor[row * (J * J + J) + J * J + tid] : 0.0;
        s[tid] = good ? isd[tid] * g_a[row * J + tid] : 0.0;
    }
    __syncthreads();
    if (tid == 0) chol_solve<J>(L, s);
    __syncthreads();
    double bbar = 0.0;
    if (tid < J) bbar = (s[tid] * isd[tid] - 2.0 * gq * a[row * J + tid]) * sqrt((double)kZ.norm2[tid]);
    __syncthreads();
    if (tid < J) s[tid] = bbar;
    __syncthreads();
    if (tid < J) {
        double v = 0.0;
        #pragma unroll 1
        for (int j = 0; j < J; ++j) v += (double)kZ.c[tid][j] * s[j];
        coef[row * (J + 1) + tid] = good ? v : 0.0;
    }
    if (tid == 0) coef[row * (J + 1) + J] = good ? 2.0 * gq : 0.0;
}

// ------------------------------------------------------------------------------------------------------------------- the seed
// dp[a][b] = (a + 1) c_(a+1, b), dq[a][b] = (b + 1) c_(a, b+1): the two gradient polynomials of degree N - 1, by Horner
template <int N>
__device__ __forceinline__ void seed_ray(const double (&dp)[N][N], const double (&dq)[N][N], double q2, float xf, float yf, float pf,
                                         float qf, unsigned okb, float &ox, float &oy)
{
#pragma clang fp contract(off)
    ox = oy = 0.0f;
    if (okb != 0u) {
        const double x = (double)xf, y = (double)yf, p = (double)pf, q = (double)qf;
        double gx = 0.0, gy = 0.0;
#pragma unroll
        for (int a = N - 1; a >= 0; --a) {
            double ix = dp[a][N - 1 - a], iy = dq[a][N - 1 - a];
#pragma unroll
            for (int b = N - 2 - a; b >= 0; --b) { ix = ix * q + dp[a][b]; iy = iy * q + dq[a][b]; }
            gx = gx * p + ix;
            gy = gy * p + iy;
        }
        ox = (float)(q2 * x + gx);
        oy = (float)(q2 * y + gy);
    }
}

template <int N>
__global__ __launch_bounds__(kBlock) void zfit_seed_kernel(Rays r, int64_t P, int W, int row0, const double *__restrict__ coef,
                                                           float *gx_out, float *gy_out)
{
#pragma clang fp contract(off)
    constexpr int J = n_coef(N);
    const int row = row0 + (int)blockIdx.y;
    const int f = row / W, w = row - f * W;
    const int64_t off = f * r.s_f + w * r.s_w, poff = f * r.ps_f + w * r.ps_w;
    const float *__restrict__ x = r.x + off, *__restrict__ y = r.y + off;
    const float *__restrict__ px = r.px + poff, *__restrict__ py = r.py + poff;
    const uint8_t *__restrict__ ok = r.ok + off;
    float *__restrict__ gx = gx_out ? gx_out + off : nullptr, *__restrict__ gy = gy_out ? gy_out + off : nullptr;
    double dp[N][N], dq[N][N];
#pragma unroll
    for (int a = 0; a < N; ++a)
#pragma unroll
        for (int b = 0; b < N; ++b) {
            const bool in = a + b <= N - 1;                 // (compile-time after unrolling)
            dp[a][b] = in ? (double)(a + 1) * coef[(int64_t)row * (J + 1) + tri(a + 1, b) - 1] : 0.0;
            dq[a][b] = in ? (double)(b + 1) * coef[(int64_t)row * (J + 1) + tri(a, b + 1) - 1] : 0.0;
        }
    const double q2 = coef[(int64_t)row * (J + 1) + J];
    const int64_t first = (int64_t)blockIdx.x * kChunk;
    // (a NULL output is aligned)
    const bool vec = r.s_p == 1 && r.ps_p == 1 && aligned_to(x, 16) && aligned_to(y, 16) && aligned_to(px, 16) && aligned_to(py, 16)
                     && aligned_to(ok, 4) && aligned_to(gx, 16) && aligned_to(gy, 16);
    const int64_t ip = first + kVec * (int64_t)threadIdx.x;
    if (vec && ip + kVec <= P) {
        const float4 x4 = *reinterpret_cast<const float4 *>(x + ip), y4 = *reinterpret_cast<const float4 *>(y + ip);
        const float4 p4 = *reinterpret_cast<const float4 *>(px + ip), q4 = *reinterpret_cast<const float4 *>(py + ip);
        const unsigned o4 = *reinterpret_cast<const unsigned *>(ok + ip);
        float4 u, v;
        seed_ray<N>(dp, dq, q2, x4.x, y4.x, p4.x, q4.x, o4 & 0xffu, u.x, v.x);
        seed_ray<N>(dp, dq, q2, x4.y, y4.y, p4.y, q4.y, o4 & 0xff00u, u.y, v.y);
        seed_ray<N>(dp, dq, q2, x4.z, y4.z, p4.z, q4.z, o4 & 0xff0000u, u.z, v.z);
        seed_ray<N>(dp, dq, q2, x4.w, y4.w, p4.w, q4.w, o4 & 0xff000000u, u.w, v.w);
        if (gx) *reinterpret_cast<float4 *>(gx + ip) = u;
        if (gy) *reinterpret_cast<float4 *>(gy + ip) = v;
        return;
    }
    // one ray at a time: the whole row on the strided path (lanes along the rays), the last one to three on the aligned one
    for (int j = 0; j < kVec; ++j) {
        const int64_t i = vec ? ip + j : first + (int64_t)j * kBlock + threadIdx.x;
        if (i >= P) continue;
        const int64_t o = i * r.s_p, po = i * r.ps_p;
        float u, v;
        seed_ray<N>(dp, dq, q2, x[o], y[o], px[po], py[po], ok[o], u, v);
        if (gx) gx[o] = u;
        if (gy) gy[o] = v;
    }
}

// ------------------------------------------------------------------------------------------------------------------- the host
// the argument check the ray calls share; `name` opens the message
int check_rays(const char *name, int64_t F, int64_t P, int64_t W, int order, const Rays &r, const void *table)
{
    if (const char *what = size_fault(F, P, W)) return refuse(name, what);
    if (order < kMinN || order > kMaxN) return refuse(name, "the order must be 2 .. 6");
    if (!r.x || !r.y || !r.ok || !r.px || !r.py) return refuse(name, "x, y, ok, px and py are required");
    if (!table) return refuse(name, "the moments / coefficients pointer is NULL");
    return TL_OK;
}

template <int N, int PART>
void launch_moments(dim3 grid, const Rays &r, int64_t P, int W, int row0, double *part, Plan pl, hipStream_t st)
{
    hipLaunchKernelGGL((zfit_moments_kernel<N, PART>), grid, dim3(kBlock), 0, st, r, P, W, row0, part, pl.nbx, pl.R);
}

template <int N>
void launch_moments_of(dim3 grid, const Rays &r, int64_t P, int W, int row0, double *part, Plan pl, hipStream_t st)
{
    if constexpr (N >= 6) {                               // 110 accumulators in one kernel would leave one wave per SIMD: two launches
        launch_moments<N, 1>(grid, r, P, W, row0, part, pl, st);
        launch_moments<N, 2>(grid, r, P, W, row0, part, pl, st);
    } else {
        launch_moments<N, 0>(grid, r, P, W, row0, part, pl, st);
    }
}

#define ZFIT_ORDERS(CALL) \
    switch (order) {      \
    case 2: CALL(2); break; \
    case 3: CALL(3); break; \
    case 4: CALL(4); break; \
    case 5: CALL(5); break; \
    default: CALL(6); break; \
    }

}  // namespace

extern "C" {

size_t tl_zfit_workspace_bytes(int64_t F, int64_t P, int64_t W, int order)
{
    if (size_fault(F, P, W) || order < kMinN || order > kMaxN) return 0;
    return (size_t)(F * W) * (size_t)row_plan(F * W, P).nbx * n_mom(order) * sizeof(double);
}

int tl_zfit_moments(int32_t device, int64_t F, int64_t P, int64_t W, int order, const float *x, const float *y, const uint8_t *ok,
                    int64_t s_f, int64_t s_p, int64_t s_w, const float *px, const float *py, int64_t ps_f, int64_t ps_p,
                    int64_t ps_w, double *moments, void *workspace, size_t workspace_bytes, void *stream)
{
    static const char *name = "tl_zfit_moments";
    const Rays r = {x, y, ok, s_f, s_p, s_w, px, py, ps_f, ps_p, ps_w};
    if (const int rc = check_rays(name, F, P, W, order, r, moments)) return rc;
    if (const int rc = check_workspace(name, workspace, workspace_bytes, tl_zfit_workspace_bytes(F, P, W, order), "tl_zfit_workspace_bytes"))
        return rc;
    if (const int rc = tl_host::use_device(device)) return rc;
    const int64_t rows = F * W;
    const Plan pl = row_plan(rows, P);
    hipStream_t st = (hipStream_t)stream;
    if (const int rc = launch_rows(rows, pl.nbx, "zfit_moments_kernel launch", [&](dim3 grid, int row0) {
#define CALL(N) launch_moments_of<N>(grid, r, P, (int)W, row0, (double *)workspace, pl, st)
            ZFIT_ORDERS(CALL)
#undef CALL
        }))
        return rc;
    return launch_reduce(zfit_reduce_kernel, "zfit_reduce_kernel launch", (const double *)workspace, moments, rows, pl.nbx, n_mom(order), st);
}

int tl_zfit_solve(int32_t device, int64_t rows, int order, const double *moments, const double *g_a, const double *g_q, double *a,
                  double *q, uint8_t *valid, double *factor, double *coef, void *stream)
{
    const char *name = "tl_zfit_solve";
    if (rows < 1 || rows > kMaxDim) return refuse(name, "rows must be 1 .. 2^31 - 1");
    if (order < kMinN || order > kMaxN) return refuse(name, "the order must be 2 .. 6");
    if (!a || !valid || !factor) return refuse(name, "a, valid and factor are required");
    if (moments ? !q : (!g_a || !g_q || !coef))
        return refuse(name, "moments and q (the fit), or g_a, g_q and coef (its adjoint) are required");
    if (const int rc = tl_host::use_device(device)) return rc;
    hipStream_t st = (hipStream_t)stream;
    for (int64_t row0 = 0; row0 < rows; row0 += kMaxY) {
        const unsigned nb = (unsigned)std::min<int64_t>(kMaxY, rows - row0);
        if (moments) {
#define CALL(N) hipLaunchKernelGGL(zfit_factor_kernel<N>, dim3(nb), dim3(64), 0, st, moments, row0, a, q, valid, factor)
            ZFIT_ORDERS(CALL)
#undef CALL
        } else {
#define CALL(N) hipLaunchKernelGGL(zfit_adjoint_kernel<N>, dim3(nb), dim3(64), 0, st, (const double *)factor, (const double *)a, \
                                   (const uint8_t *)valid, g_a, g_q, row0, coef)
            ZFIT_ORDERS(CALL)
#undef CALL
        }
        if (const int rc = tl_host::launched("zfit solve kernel launch")) return rc;
    }
    return TL_OK;
}

int tl_zfit_seed(int32_t device, int64_t F, int64_t P, int64_t W, int order, const float *x, const float *y, const uint8_t *ok,
                 int64_t s_f, int64_t s_p, int64_t s_w, const float *px, const float *py, int64_t ps_f, int64_t ps_p, int64_t ps_w,
                 const double *coef, float *gx, float *gy, void *stream)
{
    const Rays r = {x, y, ok, s_f, s_p, s_w, px, py, ps_f, ps_p, ps_w};
    if (const int rc = check_rays("tl_zfit_seed", F, P, W, order, r, coef)) return rc;
    if (!gx && !gy) return refuse("tl_zfit_seed", "gx and gy are both NULL");
    if (const int rc = tl_host::use_device(device)) return rc;
    return launch_rows(F * W, cdiv(P, kChunk), "zfit_seed_kernel launch", [&](dim3 grid, int row0) {
#define CALL(N) hipLaunchKernelGGL(zfit_seed_kernel<N>, grid, dim3(kBlock), 0, (hipStream_t)stream, r, P, (int)W, row0, coef, gx, gy)
        ZFIT_ORDERS(CALL)
#undef CALL
    });
}

}  // extern "C"
