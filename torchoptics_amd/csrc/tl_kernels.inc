// tl_kernels.inc -- device code of the fused sequential ray tracer for gfx950 (CDNA4).
//
// Included once per arithmetic mode (tl_strict.hip, tl_fast.hip) with
//   TL_NS    : namespace name for the mode; TL_API_NS: namespace of its entry points (tl_common.h, TL_DECLARE_MODE)
//   TL_FAST  : 0 = strict (TU built with -ffp-contract=off, IEEE sqrt / divide)
//              1 = fast   (TU built with -ffp-contract=fast, hardware rcp / rsq / sqrt)
//
// Mapping: one ray per lane.  blockIdx.y = f*W + w, so the field and the wavelength are
// wave-uniform: c[k], t[k], mu[w][k], mask[k], cy[f] come through the scalar cache into
// SGPRs (s_load), not VGPRs or LDS.  blockIdx.x walks the pupil dimension in chunks of
// kBlock*R consecutive points; lane i of a wave owns point base+i, so every global access
// is a 256-byte contiguous wave access.
//
// The arithmetic follows SURVEY.md Appendix A (= ray_tracing_lite.py:525-571, 594-675)
// operation by operation; comments cite the reference line each group restates.
//
// Kernels (launchers at the end of the file):
//   trace_fwd_kernel<PEN, ASPH, OPD>   forward, every feature; trace_fwd_plain_kernel<2> = the all-spherical
//                                      forward of FAST mode, two rays per lane
//   trace_bwd_inv_kernel<ASPH>         backward, default: walks each ray back from the forward's outputs
//   trace_bwd_inv_unrolled_kernel<NS>  the same with the surface loop unrolled (all-spherical lenses of 3..20 rows)
//   trace_bwd_kernel<NS, ASPH, PEN>    backward, checkpoint algorithm (re-trace + reverse): penalty term,
//                                      allow_backward_rays = False, per-ray input gradients, and the
//                                      on-device fallback of the walk-back

namespace TL_NS {

constexpr float kEps = 1e-6f;     // ray_tracing_lite.py:530,552
// A live ray whose smallest cos^2 (incidence or refraction, any surface) is below this is "ill-conditioned":
// fp32 rounding is amplified by ~1/cos^2 there, so only a bit-faithful re-trace reproduces the reference's
// autograd to 1e-5.  The forward kernel counts such rays (moment 9); the backward picks its algorithm by it.
constexpr float kCondThr = 0.01f;

// sum over the fields of moment 9 (wave-uniform scalar loads)
__device__ __forceinline__ bool ill_conditioned(const double *__restrict__ mom, const int F)
{
    double n = 0.0;
    for (int f = 0; f < F; ++f) n += mom[(size_t)f * TL_NMOM + 9];
    return n > 0.0;
}

// Does the checkpoint kernel have to redo the walk-back launch?  Either the forward counted an
// ill-conditioned live ray (fb_mom, known before the walk-back starts: that launch retires at once), or the
// walk-back itself met a non-finite adjoint and wrote this call's token into the workspace word fb_poison.
// The token is unique per call, so the word never needs clearing (a memset node costs 6 us per step); stale
// or uninitialised contents that happen to equal it would only cost an unnecessary, still exact, fallback.
__device__ __forceinline__ bool fallback_needed(const double *__restrict__ fb_mom,
                                                const unsigned *__restrict__ fb_poison, const unsigned fb_token,
                                                const int F)
{
    return (fb_mom && ill_conditioned(fb_mom, F)) || (fb_poison && *fb_poison == fb_token);
}
constexpr int kBlock = 256;       // 4 waves: one per SIMD of a CU
constexpr int kWaves = kBlock / 64;

// Bit k = (flags[k] != 0) for the S <= 32 rows of a u8 array (sequence mask, surface kind).  gfx950 has no
// scalar byte load, so `flags[k]` inside the surface loop is a VECTOR load of a uniform value whose latency
// sits on every surface of every ray; read the bytes once per wave instead and keep the word in an SGPR.
__device__ __forceinline__ unsigned row_bits(const uint8_t *__restrict__ flags, const int S)
{
    const int lane = threadIdx.x & 63;
    return (unsigned)__ballot(flags != nullptr && lane < S && flags[lane < S ? lane : 0] != 0);
}

// Wave-uniform loads of the prescription (c, t, mu, kappa, poly, n: never written by any kernel).  Read through the
// CONSTANT address space they are always scalar loads (s_load into SGPRs).  Read through a plain global pointer they are
// scalar only while the compiler can prove that no store of the kernel clobbers them: one store through an unrelated
// pointer inside the row loop (the per-row hit points of an aspheric lens, the penalty stacks) and every row's c, t, mu
// became a VECTOR load with a full s_waitcnt vmcnt(0) at the top of the row -- 10 % of the forward kernel on a lens
// with aspheric rows (ISA of trace_fwd_kernel<false,true,false>, round 3).  On AMDGPU the constant and the global
// address space are the same memory with the same pointer representation.
__device__ __forceinline__ float uload(const float *__restrict__ q, const int i)
{
    return ((const __attribute__((address_space(4))) float *)(unsigned long long)q)[i];
}
__device__ __forceinline__ double uload64(const double *__restrict__ q, const int i)
{
    return ((const __attribute__((address_space(4))) double *)(unsigned long long)q)[i];
}

// ------------------------------------------------------------------ math policy
// STRICT (TL_FAST = 0, TU built with -ffp-contract=off) promises the reference's fp32 operation order for the
// FORWARD trace (ray_tracing_lite.py:525-571, 594-675), where every rounding is pinned by the oracle.
// TL_REVERSE_CONTRACT: the reverse sweeps -- step_vals, step_adjoint, step_bwd_asph and the whole walk-back
// kernel -- have no reference operation order to follow (the reference differentiates by autograd over a
// different graph), so unfused multiplies and adds only cost instructions there.  Those function bodies carry
// `#pragma clang fp contract(fast)`: -21 % on the walk-back kernel, -15 % on the checkpoint kernel, gradients
// move by 1e-8 relative (fewer roundings, not more).  The forward sweep INSIDE the checkpoint kernel
// (step_fwd) stays unfused: it has to reproduce the forward kernel bit for bit.
#if TL_FAST
__device__ __forceinline__ float tl_sqrt(float v) { return __builtin_amdgcn_sqrtf(v); }
__device__ __forceinline__ float tl_div(float a, float b) { return a * __builtin_amdgcn_rcpf(b); }
#else
// Correctly rounded sqrt for the value range of LIVE rays (cos^2 terms in [1e-6, ~1]): v_sqrt_f32
// is within 1 ulp, so the exact result is s, s-1ulp or s+1ulp; pick it from the signs of the exact
// residuals x - s_dn*s and x - s_up*s (one FMA each).  This is the fix-up LLVM's own f32 sqrt
// expansion uses, minus its scaling of inputs below 2^-96 and its 0/inf/NaN class select, which live
// rays never need (dead lanes may compute garbage, see step_fwd<LEAN>): 9 instructions instead of 16.
// Bit-equality with the IEEE oracle is asserted by tests/test_gpu_parity.py on every fixture.
__device__ __forceinline__ float tl_sqrt_fixup(float x)
{
    float s = __builtin_amdgcn_sqrtf(x);
    const float s_dn = __int_as_float(__float_as_int(s) - 1);
    const float s_up = __int_as_float(__float_as_int(s) + 1);
    const float r_dn = __builtin_fmaf(-s_dn, s, x);
    const float r_up = __builtin_fmaf(-s_up, s, x);
    s = (r_dn <= 0.0f) ? s_dn : s;
    s = (r_up > 0.0f) ? s_up : s;
    return s;
}
#ifndef TL_STRICT_LEAN_ARITH
#define TL_STRICT_LEAN_ARITH 1
#endif
#if TL_STRICT_LEAN_ARITH
// (r3) The same two results -- correctly rounded sqrt and quotient -- in 8 instructions each instead of 9 and 11:
// * sqrt: LLVM's OTHER f32 expansion (AMDGPU lowerFSQRTF32, the branch it takes when v_sqrt cannot be used): v_rsq, then
//   s = x y, h = y/2, one coupled Newton step on both, and the final residual correction d = x - s^2, s += d h.
// * divide: LLVM's expansion of a / b without its v_div_scale x2 / v_div_fixup wrapping, which only rescales operands near
//   the ends of the exponent range and patches inf / nan / denormal results -- the operands here are cos-like sums and
//   lengths in mm, ~1e-6 .. 1e3: rcp, one Newton step on it, q = a r, two residual corrections.
// Both are bit-identical to the IEEE results on the operand ranges of the trace: tests/test_gpu_arith.py compares them
// with numpy's correctly rounded float32 sqrt and division on 2^26 operands (tl_selftest_arith), and every strict parity
// test of the forward still asserts bit-equality with the IEEE oracle.
__device__ __forceinline__ float tl_sqrt(float x)
{
    const float y = __builtin_amdgcn_rsqf(x);
    float s = x * y;
    float h = 0.5f * y;
    const float e = __builtin_fmaf(-h, s, 0.5f);
    h = __builtin_fmaf(h, e, h);
    s = __builtin_fmaf(s, e, s);
    const float d = __builtin_fmaf(-s, s, x);
    return __builtin_fmaf(d, h, s);
}
__device__ __forceinline__ float tl_div(float a, float b)
{
    float r = __builtin_amdgcn_rcpf(b);
    const float e = __builtin_fmaf(-b, r, 1.0f);
    r = __builtin_fmaf(e, r, r);
    float q = a * r;
    const float e2 = __builtin_fmaf(-b, q, a);
    q = __builtin_fmaf(e2, r, q);
    const float e3 = __builtin_fmaf(-b, q, a);
    return __builtin_fmaf(e3, r, q);
}
#else
__device__ __forceinline__ float tl_sqrt(float x) { return tl_sqrt_fixup(x); }
__device__ __forceinline__ float tl_div(float a, float b) { return a / b; }        // correctly rounded
#endif
#endif
__device__ __forceinline__ float tl_sqrt_any(float v) { return __builtin_sqrtf(v); }   // full-range, IEEE
__device__ __forceinline__ float tl_sqrt_hw(float v) { return __builtin_amdgcn_sqrtf(v); }   // hardware, 1 ulp
// reciprocals of the adjoint sweep (gradients only; never feed the forward values)
#if !TL_FAST
// strict: hardware estimate + one Newton step (~0.5 ulp and, unlike the raw v_rcp/v_rsq, unbiased).
// Gradients that are small residuals of large per-ray terms (d/dcy of a distortion-free lens cancels
// to ~1e-3 of its terms) amplify any per-ray BIAS by that factor: measured 6.7e-4 -> 7.6e-5 on
// g_cy at cfg3 for +3 % kernel time; c, t, mu are ~1e-7 either way.
__device__ __forceinline__ float tl_rcp(float v)
{
    const float r = __builtin_amdgcn_rcpf(v);
    return __builtin_fmaf(r, __builtin_fmaf(-v, r, 1.0f), r);
}
__device__ __forceinline__ float tl_rsq(float v)
{
    const float r = __builtin_amdgcn_rsqf(v);
    const float e = __builtin_fmaf(-(v * r), r, 1.0f);
    return __builtin_fmaf(0.5f * r, e, r);
}
#else
__device__ __forceinline__ float tl_rcp(float v) { return __builtin_amdgcn_rcpf(v); }
__device__ __forceinline__ float tl_rsq(float v) { return __builtin_amdgcn_rsqf(v); }
#endif

// 1/sqrt(v) and sqrt(v) together.  Strict: one Newton step shared by both (r1 = r (1 + e/2), s1 = v r (1 + e/2) with
// e = 1 - v r^2): five instructions after the v_rsq instead of the six of tl_rsq followed by v * r.
__device__ __forceinline__ void tl_rsq_sqrt(const float v, float &r_out, float &s_out)
{
    const float r = __builtin_amdgcn_rsqf(v);
    const float s0 = v * r;
#if TL_FAST
    r_out = r; s_out = s0;
#else
    const float he = 0.5f * __builtin_fmaf(-s0, r, 1.0f);
    r_out = __builtin_fmaf(r, he, r);
    s_out = __builtin_fmaf(s0, he, s0);
#endif
}

// Reciprocals that only the ADJOINT reads (1/cz_out, 1/(cz + cos_i) in the walk-back kernels): the hardware's 1-ulp
// v_rcp_f32 as it is, in both modes.  The Newton-refined tl_rcp / tl_rsq stay wherever a value feeds the reconstruction
// of the ray (an error there travels down the whole path and biases the residual-type gradients d/dz, d/dcy); an
// error here scales one term of one row by 1 +- 6e-8.  Measured: -4 % on the walk-back, every gradient group of the
// live check unchanged to its printed digits (tools/sessions/r2_s50.txt).
__device__ __forceinline__ float tl_rcp_adj(float v) { return __builtin_amdgcn_rcpf(v); }

struct Ray { float x, y, z, cx, cy, cz; };
struct Adj { float x, y, z, cx, cy, cz; };

// One surface: intersect -> propagate -> retire -> refract -> flag -> retire -> shift.
// `check_back` = (k > 0) && mask[k-1]   (ray_tracing_lite.py:626-628)
//
// LEAN = false : the reference's data flow literally, including reset_bad_rays after the miss
//                test and after the refraction test (dead rays parked at (0,0,0,0,0,1)).
// LEAN = true  : the same arithmetic for every ray that is still alive, but dead lanes are left
//                to compute garbage (possibly NaN) instead of being reset; `ok` is sticky and
//                `back` is only ever updated under `ok`, so nothing a dead lane computes can reach
//                a flag, and the caller masks the dead lanes' values once at the end.  Saves the
//                14 v_cndmask per surface that the literal form spends on lanes that are alive.
template <bool LEAN>
__device__ __forceinline__ void step_fwd(Ray &r, bool &ok, bool &back, const float c, const float t,
                                         const float mu, const bool check_back, const bool allow_back,
                                         float &cos2_i_raw, float &cos2_t_raw, float &cos_i_out, float &cos_t_out)
{
    // find_marching_distance_spherical :532-543
    const float e = -((r.x * r.cx + r.y * r.cy) + r.z * r.cz);
    const float mz = r.z + e * r.cz;
    const float m2 = ((r.x * r.x + r.y * r.y) + r.z * r.z) - e * e;
    const float tmp = c * m2 - 2.0f * mz;
    const float cos2 = r.cz * r.cz - c * tmp;
    const bool miss = (cos2 - kEps) < 0.0f;
    const float cos_i = tl_sqrt(LEAN ? cos2 : (miss ? 1.0f : cos2));
    const float d = e + tl_div(tmp, r.cz + cos_i);
    // update_ray_coordinates :518-521
    const float dz = d * r.cz;
    const float x1 = r.x + d * r.cx;
    const float y1 = r.y + d * r.cy;
    const float z1 = r.z + dz;
    // :619-620
    ok = ok && !miss;
    const float x2 = (LEAN || ok) ? x1 : 0.0f, y2 = (LEAN || ok) ? y1 : 0.0f, z2 = (LEAN || ok) ? z1 : 0.0f;
    const float cx2 = (LEAN || ok) ? r.cx : 0.0f, cy2 = (LEAN || ok) ? r.cy : 0.0f;
    // apply_snell_spherical :554-568 (cos_i is NOT reset for retired rays)
    const float cos2_t = 1.0f - (mu * mu) * (1.0f - cos_i * cos_i);
    const bool tir = (cos2_t - kEps) < 0.0f;
    const float cos_t = tl_sqrt(LEAN ? cos2_t : (tir ? 1.0f : cos2_t));
    const float g = cos_t - mu * cos_i;
    const float gc = g * c;
    const float cx3 = mu * cx2 - gc * x2;
    const float cy3 = mu * cy2 - gc * y2;
    const float czsq = 1.0f - (cx3 * cx3 + cy3 * cy3);
    const bool fail = tir || ((czsq - kEps) < 0.0f);
    const float cz3 = tl_sqrt(LEAN ? czsq : (fail ? 1.0f : czsq));
    // :626-632 (ok after the miss test, before the refraction test)
    // (branch-free on purpose: a uniform branch here splits the surface step into basic blocks and pins
    // the scalar loads of c, t, mu next to their first use, with the scalar-cache latency exposed)
    {
        const bool hit = check_back && (dz < 0.0f) && ok;
        back = back || (allow_back && hit);
        ok = ok && !(hit && !allow_back);
    }
    // :635-639
    ok = ok && !fail;
    r.x = (LEAN || ok) ? x2 : 0.0f;
    r.y = (LEAN || ok) ? y2 : 0.0f;
    r.z = ((LEAN || ok) ? z2 : 0.0f) - t;
    r.cx = (LEAN || ok) ? cx3 : 0.0f;
    r.cy = (LEAN || ok) ? cy3 : 0.0f;
    r.cz = (LEAN || ok) ? cz3 : 1.0f;
    cos2_i_raw = cos2;
    cos2_t_raw = cos2_t;
    cos_i_out = cos_i;          // sqrt of the two, as the step itself took them (LEAN: of the raw values)
    cos_t_out = cos_t;
}

template <bool LEAN>
__device__ __forceinline__ void step_fwd(Ray &r, bool &ok, bool &back, const float c, const float t,
                                         const float mu, const bool check_back, const bool allow_back,
                                         float &cos2_i_raw, float &cos2_t_raw)
{
    float u0, u1;
    step_fwd<LEAN>(r, ok, back, c, t, mu, check_back, allow_back, cos2_i_raw, cos2_t_raw, u0, u1);
}

template <bool LEAN>
__device__ __forceinline__ void step_fwd(Ray &r, bool &ok, bool &back, const float c, const float t,
                                         const float mu, const bool check_back, const bool allow_back)
{
    float u0, u1;
    step_fwd<LEAN>(r, ok, back, c, t, mu, check_back, allow_back, u0, u1);
}

// ------------------------------------------------------------------ penalty term (aggregate=True)
// Per surface, after the shift to the next vertex (ray_tracing_lite.py:641-657):
//   zRELU = max(z, 0);  theta = acos(clamp(sqrt(cos2_i), -1+1e-7, 1-1e-7)) / (pi/2), theta' likewise from
//   cos2_t; theta = theta' = 1 for rays that are not ok after the surface (their z is -t: parked rays).
// The caller sums them per ray: Q_ray = (sum theta + sum theta' + sum zRELU) / n_sequence, NaN -> 0
// (optics_simulator_lite.py:441-448).
constexpr float kAcosHi = (float)(1.0 - 1e-7);
constexpr float kHalfPi = (float)(0.5 * 3.141592653589793);
constexpr float kPenS2Min = 1.7881393e-7f;      // 3 2^-24: sin^2 above which sqrt(1 - sin^2) rounds to <= kAcosHi = 1 - 2^-23

// acos on [0, 1]: sqrt(1 - x) times a degree-7 polynomial (Abramowitz & Stegun 4.4.46, |error| <= 2e-8 -- a fifth of
// an fp32 ulp of pi/2; the sqrt factor carries the singularity at 1, so the relative error stays small where the
// penalty's angles live, near normal incidence).  12 instructions; libm's acosf plus the IEEE divide by pi/2 and the
// full-range sqrt that used to stand here were ~50, twice per row: as much as the whole surface step.
__device__ __forceinline__ float acos_01(const float x)
{
    float p = -0.0012624911f;
    p = __builtin_fmaf(p, x, 0.0066700901f);
    p = __builtin_fmaf(p, x, -0.0170881256f);
    p = __builtin_fmaf(p, x, 0.0308918810f);
    p = __builtin_fmaf(p, x, -0.0501743046f);
    p = __builtin_fmaf(p, x, 0.0889789874f);
    p = __builtin_fmaf(p, x, -0.2145988016f);
    p = __builtin_fmaf(p, x, 1.5707963050f);
    return tl_sqrt_hw(1.0f - x) * p;
}
// theta / (pi/2) from the cosine u = sqrt(cos2) >= 0 of a ray that is ok (the clamp's lower bound -1 + 1e-7 cannot bind)
__device__ __forceinline__ float theta_from_cos(const float u)
{
    return acos_01(fminf(u, kAcosHi)) * (1.0f / kHalfPi);
}
__device__ __forceinline__ float theta_norm(const float cos2) { return theta_from_cos(tl_sqrt(cos2)); }

// Upstream gradient of the three penalty quantities of one row of one ray: z_RELU, theta_norm, theta_prime_norm.  The
// fused seed gq (moment 8: the per-ray sum of all three) enters them alike (pen_seed); a per-ray seed from the stacks
// (PEN == kPenRay, tl_seeds.g_stacks) adds its own value to each.
struct PenSeed { float z, th, thp; };
__device__ __forceinline__ PenSeed pen_seed(const float g) { return PenSeed{g, g, g}; }

// Forward intermediates of one (live-branch) surface step that its adjoint needs.
struct StepVals {
    float e, m2, tmp, cos2;           // intersection: e = -(r.d), m2 = |r|^2 - e^2, tmp = c m2 - 2 mz, cos2 = cos_i^2
    float cos_i, r_i;                 // cos of incidence and its reciprocal
    float inv_den, q, d;              // 1/(cz + cos_i), tmp/(cz + cos_i), marching distance d = e + q
    float x1, y1;                     // hit point
    float s2, cos_t, r_t;             // 1 - cos_i^2, cos of refraction and its reciprocal
    float g, gc;                      // cos_t - mu cos_i, g c
    float cx3, cy3, r_z;              // outgoing direction cosines, 1 / cz_out
};

// Recompute them from the state entering the surface (checkpoint algorithm).
__device__ __forceinline__ StepVals step_vals(const Ray &in, const float c, const float mu)
{
#pragma clang fp contract(fast)       // reverse sweep: see TL_REVERSE_CONTRACT above
    StepVals v;
    v.e = -((in.x * in.cx + in.y * in.cy) + in.z * in.cz);
    const float mz = in.z + v.e * in.cz;
    v.m2 = ((in.x * in.x + in.y * in.y) + in.z * in.z) - v.e * v.e;
    v.tmp = c * v.m2 - 2.0f * mz;
    v.cos2 = in.cz * in.cz - c * v.tmp;
    // 1/sqrt once (v_rsq_f32), sqrt by one multiply: the adjoint needs both cos and 1/cos
    v.r_i = tl_rsq(v.cos2);
    v.cos_i = v.cos2 * v.r_i;
    v.inv_den = tl_rcp(in.cz + v.cos_i);
    v.q = v.tmp * v.inv_den;
    v.d = v.e + v.q;
    v.x1 = in.x + v.d * in.cx;
    v.y1 = in.y + v.d * in.cy;
    v.s2 = 1.0f - v.cos_i * v.cos_i;
    const float cos2_t = 1.0f - (mu * mu) * v.s2;
    v.r_t = tl_rsq(cos2_t);
    v.cos_t = cos2_t * v.r_t;
    v.g = v.cos_t - mu * v.cos_i;
    v.gc = v.g * c;
    v.cx3 = mu * in.cx - v.gc * v.x1;
    v.cy3 = mu * in.cy - v.gc * v.y1;
    v.r_z = tl_rsq(1.0f - (v.cx3 * v.cx3 + v.cy3 * v.cy3));      // 1 / cz3
    return v;
}

// Adjoint of step_fwd for a ray that is alive after the step (every `where` of the
// reference passes through, so only the smooth branch is differentiated; rays that fail
// anywhere have exactly zero gradient and are masked by the caller).
// in : state entering the surface     v : forward intermediates     a : adjoint of the state leaving it (in/out)
// PEN: gq = upstream gradients of zRELU, theta and theta' at this surface (PenSeed), zpos = the
// ray's z leaving the surface is > 0 (zRELU active).  theta = acos(u)/h with u = cos_i:
// d theta/d cos2_i = -1/(2 h u sqrt(1-u^2)), zero where the clamp at 1-1e-7 is active; for theta'
// 1 - cos_t^2 = mu^2 (1 - cos_i^2).
// WALK (walk-back kernels): u and u' are the cosines the walk has reconstructed (v.cos_i, v.cos_t) -- it has no
// bit-equal forward to take them from.  Rays within a few ulp of the clamp (incidence within ~5e-4 rad of the normal)
// may then sit on the other side of it than in the forward: the same kind of difference PyTorch's own fp32 and fp64
// autograd show there (DESIGN.md "Penalty term").
template <bool PEN, bool WALK = false>
__device__ __forceinline__ void step_adjoint(const Ray &in, const float c, const float mu, const StepVals &v, Adj &a,
                                             float &g_c, float &g_t, float &g_mu, const PenSeed gq = PenSeed{},
                                             const bool zpos = false, const float b_d_opd = 0.0f)
{
#pragma clang fp contract(fast)
    // (Written out with the factors of 2 and 1/2 folded by hand -- the compiler may contract a*b+c but not
    //  re-associate, and every row of every ray pays for each of these instructions: 13 fewer than the literal
    //  transcription of the chain rule, same values to rounding.)
    // ---- reverse: z5 = z4 - t   (zRELU of the penalty term acts on z5)
    if (PEN && zpos) a.z += gq.z;
    g_t = -a.z;
    // cz3 = sqrt(1 - (cx3^2 + cy3^2)):  d cz3 = -(cx3 dcx3 + cy3 dcy3) / cz3
    const float b_cz_r = a.cz * v.r_z;
    const float b_cx3 = a.cx - v.cx3 * b_cz_r;
    const float b_cy3 = a.cy - v.cy3 * b_cz_r;
    // cx3 = mu*cx - (g*c)*x1
    float b_mu = b_cx3 * in.cx + b_cy3 * in.cy;
    const float b_gc = -(b_cx3 * v.x1 + b_cy3 * v.y1);
    const float b_x1 = a.x - v.gc * b_cx3;
    const float b_y1 = a.y - v.gc * b_cy3;
    float b_c = b_gc * v.g;
    const float b_g = b_gc * c;
    // g = cos_t - mu*cos_i ; cos_t = sqrt(cos2_t) ; cos2_t = 1 - mu^2 (1 - cos_i^2).   w = 2 * (adjoint of cos2_t)
    float w = b_g * v.r_t;
    float pen_cos2_x2 = 0.0f;
    if (PEN) {
        // d theta/d cos2 = -1/(2 h u sqrt(1-u^2)) explodes (~2000) towards normal incidence and is cut to
        // zero by the clamp at u = 1-1e-7, so a 1-ulp difference in u flips a huge term.  Use exactly
        // what PyTorch's autograd uses: the FORWARD's u = sqrt(cos2) (bit-equal here in strict mode, not
        // the rsq-recomputed cos_i), 1-u*u formed from it, and clamp's inclusive pass-through mask.
        // 1 / (u sqrt(1 - u^2)) = rsq(u^2 (1 - u^2)): one hardware v_rsq_f32, unrefined -- only this adjoint term reads it
        // (WALK: sin^2 of incidence as the walk formed it, from the small quantities themselves -- v.s2 -- rather than
        //  1 - u^2, whose relative error grows like 1/sin^2 towards normal incidence, exactly where this factor is large)
        //  The clamp is then decided on that sine too -- u = fp32 sqrt(1 - s2) rounds to <= 1 - 2^-23 exactly when
        //  s2 > 3 2^-24, kPenS2Min -- so that the decision and the value it guards cannot disagree.)
        const float gh = -gq.th * (1.0f / kHalfPi);                    // 2 * (0.5 / (pi/2)): twice the adjoint
        const float ght = -gq.thp * (1.0f / kHalfPi);                  // ... of theta'
        if (WALK) {
            const float s2t = (mu * mu) * v.s2;                        // sin^2 on the refraction side
            pen_cos2_x2 = (v.s2 > kPenS2Min) ? gh * __builtin_amdgcn_rsqf((1.0f - v.s2) * v.s2) : 0.0f;
            w += (s2t > kPenS2Min) ? ght * __builtin_amdgcn_rsqf((1.0f - s2t) * s2t) : 0.0f;
        } else {
            const float u = tl_sqrt(v.cos2);
            const float uu = u * u, s2f = 1.0f - uu;
            pen_cos2_x2 = (u <= kAcosHi) ? gh * __builtin_amdgcn_rsqf(uu * s2f) : 0.0f;
            const float ut = tl_sqrt(1.0f - (mu * mu) * s2f);           // the forward's cos_t
            const float utt = ut * ut;
            w += (ut <= kAcosHi) ? ght * __builtin_amdgcn_rsqf(utt * (1.0f - utt)) : 0.0f;
        }
    }
    const float mw = mu * w;
    b_mu -= b_g * v.cos_i;
    b_mu -= v.s2 * mw;
    float b_cos_i = mu * (mw * v.cos_i - b_g);
    // x1 = x + d*cx ; y1 = y + d*cy ; z1 = z + d*cz
    // b_d_opd: upstream gradient of the optical path length times n_k (OPD = sum_k n_k d_k)
    const float b_d = ((b_x1 * in.cx + b_y1 * in.cy) + a.z * in.cz) + b_d_opd;
    float bx = b_x1, by = b_y1, bz = a.z;
    float bcx = mu * b_cx3 + b_x1 * v.d;
    float bcy = mu * b_cy3 + b_y1 * v.d;
    float bcz = a.z * v.d;
    // d = e + tmp / (cz + cos_i)
    float b_tmp = b_d * v.inv_den;
    const float b_den = -(b_tmp * v.q);
    bcz += b_den;
    b_cos_i += b_den;
    // cos_i = sqrt(cos2) ; cos2 = cz^2 - c*tmp.   b2 = 2 * (adjoint of cos2)
    const float b2 = b_cos_i * v.r_i + pen_cos2_x2;
    const float b_cos2 = 0.5f * b2;
    bcz += in.cz * b2;
    b_c -= v.tmp * b_cos2;
    b_tmp -= c * b_cos2;
    // tmp = c*m2 - 2*mz
    b_c += v.m2 * b_tmp;
    const float b_mz = -2.0f * b_tmp;
    const float b_m2_x2 = -(c * b_mz);                  // 2 * (adjoint of m2) = 2 c b_tmp
    // m2 = x^2 + y^2 + z^2 - e^2 ; mz = z + e*cz
    bx += in.x * b_m2_x2;
    by += in.y * b_m2_x2;
    bz += in.z * b_m2_x2 + b_mz;
    const float b_e = (b_d + b_mz * in.cz) - v.e * b_m2_x2;
    bcz += b_mz * v.e;
    // e = -(x*cx + y*cy + z*cz)
    a.x = bx - b_e * in.cx;
    a.y = by - b_e * in.cy;
    a.z = bz - b_e * in.cz;
    a.cx = bcx - b_e * in.x;
    a.cy = bcy - b_e * in.y;
    a.cz = bcz - b_e * in.z;
    g_c = b_c;
    g_mu = b_mu;
}

template <bool PEN>
__device__ __forceinline__ void step_bwd(const Ray &in, const float c, const float mu, Adj &a,
                                         float &g_c, float &g_t, float &g_mu, const PenSeed gq = PenSeed{},
                                         const bool zpos = false, const float b_d_opd = 0.0f, float *d_out = nullptr)
{
    const StepVals v = step_vals(in, c, mu);
    step_adjoint<PEN>(in, c, mu, v, a, g_c, g_t, g_mu, gq, zpos, b_d_opd);
    if (d_out) *d_out = v.d;
}

// ================================================================== aspheric rows (extension)
// Not in the reference (its only intersection is the closed-form sphere): conic + even polynomial
//   sag(rho) = c rho/(1 + sqrt(1 - (1+kappa) c^2 rho)) + a4 rho^2 + a6 rho^3 + a8 rho^4 + a10 rho^5
// intersected by Newton on the ray parameter s from the closed-form sphere hit, refracted with the
// vector form of Snell's law at the aspheric normal.  Defined by oracle/trace_oracle.py
// (trace_skew_general); rows with surf_kind == 0 never come here.
constexpr int kNewtonMax = 8;        // oracle: NEWTON_ITERS
constexpr float kNewtonTol = 1e-6f;  // oracle: NEWTON_TOL  |F| <= tol (1 + |z_hit|)
// Forward: when does the ray count as converged at the LAST EVALUATED point?  The step that follows (ds = -F / F', applied
// without another evaluation of the sag) leaves an error of F^2 |F'' / (2 F')|, and |F'' / (2 F')| -- the curvature of the
// sag ALONG the ray -- is bounded by the surface's own curvature: |c| + kNewtonCurv (0.1 / mm of allowance for the
// aspheric terms; for the near-paraxial rays of a real lens it is 10-100 times smaller, the slope enters squared).  The
// ray is accepted when that PREDICTED error is below a tenth of the oracle's acceptance tolerance kNewtonTol:
//     F^2 (|c| + kNewtonCurv) <= kNewtonAccept (1 + |z|),    kNewtonAccept = 1e-7.
// Waiting for |F| <= kNewtonTol BEFORE the last step, as the first version did, only spent one more evaluation.
#ifndef TL_NEWTON_ACCEPT
#define TL_NEWTON_ACCEPT 1e-7f
#endif
constexpr float kNewtonAccept = TL_NEWTON_ACCEPT;
constexpr float kNewtonCurv = 0.1f;

// Reciprocals INSIDE the Newton iteration of step_fwd_asph (starting point, residual, slope, steps): the hardware's 1-ulp
// estimates as they are -- every error there is measured by the next residual and removed by the next step (the last step
// included: ds = -F / F' is applied to a residual of <= 1e-3 mm, a 1e-7 relative error of it is 1e-10 mm).  The slope that
// gives the normal and the normalisation of that normal keep the refined forms.
#ifndef TL_ASPH_RAW_RECIP
#define TL_ASPH_RAW_RECIP 1
#endif
#if TL_ASPH_RAW_RECIP
#define TL_ASPH_RCP(v_) __builtin_amdgcn_rcpf(v_)
#define TL_ASPH_RSQ(v_) __builtin_amdgcn_rsqf(v_)
#else
#define TL_ASPH_RCP(v_) tl_rcp(v_)
#define TL_ASPH_RSQ(v_) tl_rsq(v_)
#endif

struct Asph { float c, kappa, a0, a1, a2, a3; };

__device__ __forceinline__ Asph load_asph(const tl_problem &p, const int k)
{
    Asph A;
    A.c = uload(p.c, k); A.kappa = uload(p.kappa, k);
    A.a0 = uload(p.poly, 4 * k); A.a1 = uload(p.poly, 4 * k + 1); A.a2 = uload(p.poly, 4 * k + 2); A.a3 = uload(p.poly, 4 * k + 3);
    return A;
}

// Forward step at an aspheric row (lean form: dead lanes are not reset, see step_fwd<true>).
// `live_in` = this lane holds a ray that is alive on entry (drives the convergence vote).
// Returns the marching distance s through `d_out` (for the optical path length).
// Arithmetic: aspheric rows have no reference operation order to reproduce (the reference has no aspheres; the oracle
// iterates to the root in its own arithmetic), so the promise here is the ROOT to rounding level, not an operation
// order: the sphere guess, the iterates and the converged sag / normal use v_rsq / v_rcp with one Newton refinement
// (~0.5 ulp) and contraction in both modes; only the refraction's square roots keep the mode's tl_sqrt.
__device__ __forceinline__ void step_fwd_asph(Ray &r, bool &ok, bool &back, const Asph &A, const float t,
                                              const float mu, const bool check_back, const bool allow_back,
                                              const bool live_in, float &d_out, float &cos2_i_raw, float &cos2_t_raw)
{
    float s, X, Y, rho, Z, dsag, F;
    bool miss0, bad;
    {
#pragma clang fp contract(fast)
        // Starting point: the closed-form hit on the CONIC part of the surface (the same quadratic as
        // find_marching_distance_spherical :532-543 with z^2 weighted by 1 + kappa: c (x^2 + y^2 + K z^2) - 2 z = 0 along
        // the ray), so that the first residual is the polynomial part of the sag alone.
        const float K = 1.0f + A.kappa;
        const float e = -((r.x * r.cx + r.y * r.cy) + K * (r.z * r.cz));          // -(r . d)_K
        const float dd = (r.cx * r.cx + r.cy * r.cy) + K * (r.cz * r.cz);          // (d . d)_K  (1 for a sphere)
        const float rr = (r.x * r.x + r.y * r.y) + K * (r.z * r.z);                // (r . r)_K
        const float bq = A.c * e + r.cz;                                           // -B of  A s^2 + 2 B s + C = 0
        const float cq = A.c * rr - 2.0f * r.z;                                    //  C,  A = c dd
        const float cos2 = bq * bq - (A.c * dd) * cq;                              // discriminant / 4 (cos^2 of incidence on a sphere)
        miss0 = (cos2 - kEps) < 0.0f;
        s = miss0 ? 0.0f : cq * TL_ASPH_RCP(bq + cos2 * TL_ASPH_RSQ(miss0 ? 1.0f : cos2));   // the root nearer the vertex plane
        // Newton on the ray parameter: every lane takes the same steps, and the wave leaves as soon as all of its live
        // lanes sit inside the tolerance AT THE POINT JUST EVALUATED.  That point's residual and slope then give the
        // last correction for free -- ds = -F / F', quadratic convergence: it lands on rounding level -- applied to the
        // hit point along the ray WITHOUT another evaluation of the sag (only the slope for the normal is taken again,
        // below): one evaluation per row on a mild asphere, two on a strong one, where the first version of this loop
        // spent two and three and then one more on the point after the last step.
        const float kc2 = ((1.0f + A.kappa) * A.c) * A.c;
        const float kq = fabsf(A.c) + kNewtonCurv;
        float Fp;
#pragma unroll 1
        for (int it = 0;; ++it) {
            X = r.x + s * r.cx; Y = r.y + s * r.cy;
            rho = X * X + Y * Y;
            const float q2 = 1.0f - kc2 * rho;
            const float rq = TL_ASPH_RSQ(q2);
            const float sag = (A.c * rho) * TL_ASPH_RCP(1.0f + q2 * rq) + (rho * rho) * (A.a0 + rho * (A.a1 + rho * (A.a2 + rho * A.a3)));
            dsag = 0.5f * A.c * rq + rho * (2.0f * A.a0 + rho * (3.0f * A.a1 + rho * (4.0f * A.a2 + rho * (5.0f * A.a3))));
            Z = r.z + s * r.cz;
            F = Z - sag;
            Fp = r.cz - dsag * (2.0f * (X * r.cx + Y * r.cy));
            bad = (q2 - kEps) < 0.0f;
            const bool pending = live_in && !miss0 && !bad && !((F * F) * kq <= kNewtonAccept * (1.0f + fabsf(Z)));
            if (__ballot(pending) == 0ull || it == kNewtonMax) break;
            s = s - F * TL_ASPH_RCP(Fp);
        }
        const bool conv_ = (F * F) * kq <= kNewtonAccept * (1.0f + fabsf(Z));
        const float ds = conv_ ? -F * TL_ASPH_RCP(Fp) : 0.0f;       // the last correction (lanes that did not converge are misses)
        s += ds;
        X += ds * r.cx; Y += ds * r.cy; Z += ds * r.cz;
        rho = X * X + Y * Y;
        // the slope at the corrected point (the normal is linear in it, and a strong asphere's slope moves by
        // sag'' drho ~ 1e-6 over the last step: 1e-5 rad of normal, 1e-4 mm at the image): a third of an evaluation
        dsag = 0.5f * A.c * tl_rsq(1.0f - kc2 * rho) + rho * (2.0f * A.a0 + rho * (3.0f * A.a1 + rho * (4.0f * A.a2 + rho * (5.0f * A.a3))));
    }
    const float dz = s * r.cz;
    const bool conv = (F * F) * (fabsf(A.c) + kNewtonCurv) <= kNewtonAccept * (1.0f + fabsf(Z));
    const bool miss = miss0 || bad || !conv;
    ok = ok && !miss;
    // vector Snell at n = (-m X, -m Y, 1)/sqrt(1 + m^2 rho), m = 2 dsag
    const float m = 2.0f * dsag;
    const float inv_n = tl_rsq(1.0f + (m * m) * rho);
    const float nx = -(m * X) * inv_n, ny = -(m * Y) * inv_n;
    const float cos_i = (r.cx * nx + r.cy * ny) + r.cz * inv_n;
    const float cos2_t = 1.0f - (mu * mu) * (1.0f - cos_i * cos_i);
    const bool tir = (cos2_t - kEps) < 0.0f;
    const float cos_t = tl_sqrt(cos2_t);
    const float g = cos_t - mu * cos_i;
    const float cx3 = mu * r.cx + g * nx;
    const float cy3 = mu * r.cy + g * ny;
    const float czsq = 1.0f - (cx3 * cx3 + cy3 * cy3);
    const bool fail = tir || ((czsq - kEps) < 0.0f);
    if (check_back) {
        const bool hit = (dz < 0.0f) && ok;
        if (allow_back) back = back || hit; else ok = ok && !hit;
    }
    ok = ok && !fail;
    r.x = X; r.y = Y; r.z = Z - t;
    r.cx = cx3; r.cy = cy3; r.cz = tl_sqrt(czsq);
    d_out = s;
    cos2_i_raw = cos_i * cos_i;          // conditioning of the ray at this row (see kCondThr)
    cos2_t_raw = cos2_t;
}

// Values of an aspheric row at its converged hit that the row's adjoint (asph_adjoint) reads.  The checkpoint kernel
// recomputes them from the state entering the row (asph_vals); the walk-back kernel has most of them already when it
// has undone the refraction at the hit, and fills the struct itself.
struct AsphVals {
    float s;                          // marching distance
    float X, Y, rho;                  // hit point, rho = X^2 + Y^2
    float rq, q;                      // 1/q and q = sqrt(1 - (1+kappa) c^2 rho)
    float dsag, m, inv_n, nx, ny;     // d sag / d rho, m = 2 dsag, unit normal (nx, ny, inv_n)
    float cos_i, s2, r_t, cos_t, g;   // cos of incidence, 1 - cos_i^2, 1/cos_t, cos of refraction, cos_t - mu cos_i
    float cx3, cy3, r_z;              // outgoing direction cosines, 1 / cz_out
};

// The converged ray parameter s is recovered from the stored hit point (`zout` = z leaving the step, i.e. Z - t)
// instead of re-running Newton.
__device__ __forceinline__ AsphVals asph_vals(const Ray &in, const float zout, const Asph &A, const float t, const float mu)
{
#pragma clang fp contract(fast)
    AsphVals v;
    v.s = (zout + t - in.z) * tl_rcp(in.cz);
    v.X = in.x + v.s * in.cx; v.Y = in.y + v.s * in.cy;
    v.rho = v.X * v.X + v.Y * v.Y;
    const float K = 1.0f + A.kappa;
    const float q2 = 1.0f - (K * (A.c * A.c)) * v.rho;
    v.rq = tl_rsq(q2);                 // 1/q
    v.q = q2 * v.rq;
    v.dsag = 0.5f * A.c * v.rq + v.rho * (2.0f * A.a0 + v.rho * (3.0f * A.a1 + v.rho * (4.0f * A.a2 + v.rho * (5.0f * A.a3))));
    v.m = 2.0f * v.dsag;
    v.inv_n = tl_rsq(1.0f + (v.m * v.m) * v.rho);
    v.nx = -(v.m * v.X) * v.inv_n; v.ny = -(v.m * v.Y) * v.inv_n;
    v.cos_i = (in.cx * v.nx + in.cy * v.ny) + in.cz * v.inv_n;
    v.s2 = 1.0f - v.cos_i * v.cos_i;
    const float cos2_t = 1.0f - (mu * mu) * v.s2;
    v.r_t = tl_rsq(cos2_t);
    v.cos_t = cos2_t * v.r_t;
    v.g = v.cos_t - mu * v.cos_i;
    v.cx3 = mu * in.cx + v.g * v.nx;
    v.cy3 = mu * in.cy + v.g * v.ny;
    v.r_z = tl_rsq(1.0f - (v.cx3 * v.cx3 + v.cy3 * v.cy3));
    return v;
}

// Adjoint of step_fwd_asph for a ray alive after the step.  ds/d(anything) comes from the implicit function theorem
// on F(s; .) = 0, so the Newton iterations are never differentiated.  g_asph = (d/dkappa, d/da4, d/da6, d/da8, d/da10).
// PEN: gq = upstream gradients of this row's zRELU, theta and theta' (see step_adjoint), zpos = zRELU active.
// b_s_opd: upstream gradient of the optical path length times n_k.
template <bool PEN = false, bool WALK = false>
__device__ __forceinline__ void asph_adjoint(const Ray &in, const Asph &A, const float mu, const AsphVals &v, Adj &a,
                                             float &g_c, float &g_t, float &g_mu, float g_asph[5], const PenSeed gq = PenSeed{},
                                             const bool zpos = false, const float b_s_opd = 0.0f)
{
#pragma clang fp contract(fast)
    const float s = v.s, X = v.X, Y = v.Y, rho = v.rho, rq = v.rq, q = v.q, dsag = v.dsag, m = v.m, inv_n = v.inv_n;
    const float nx = v.nx, ny = v.ny, nz = v.inv_n, cos_i = v.cos_i, s2 = v.s2, r_t = v.r_t, cos_t = v.cos_t, g = v.g;
    const float cx3 = v.cx3, cy3 = v.cy3, r_z = v.r_z;
    const float K = 1.0f + A.kappa;
    const float c2 = A.c * A.c, c3 = c2 * A.c;
    const float rq3 = rq * rq * rq;
    const float rho2 = rho * rho, rho3 = rho2 * rho, rho4 = rho2 * rho2;
    const float sag2 = 0.25f * K * c3 * rq3 + (2.0f * A.a0 + rho * (6.0f * A.a1 + rho * (12.0f * A.a2 + rho * (20.0f * A.a3))));
    // ---- reverse
    if (PEN && zpos) a.z += gq.z;
    g_t = -a.z;
    const float b_czsq = a.cz * (0.5f * r_z);
    const float b_cx3 = a.cx - 2.0f * cx3 * b_czsq;
    const float b_cy3 = a.cy - 2.0f * cy3 * b_czsq;
    float b_mu = b_cx3 * in.cx + b_cy3 * in.cy;
    const float b_g = b_cx3 * nx + b_cy3 * ny;
    float b_nx = g * b_cx3, b_ny = g * b_cy3;
    float bcx = mu * b_cx3, bcy = mu * b_cy3;
    float b_cos2_t = b_g * (0.5f * r_t);
    float pen_cos2_i = 0.0f;
    if (PEN) {
        // theta = acos(clamp(sqrt(cos_i^2)))/h, theta' likewise from cos2_t: d theta/d cos2 = -1/(2 h u sqrt(1-u^2)),
        // zero where the clamp at 1 - 1e-7 is active (step_adjoint has the spherical twin)
        // (1 - u^2 = s2 and 1 - cos_t^2 = mu^2 s2: the sines as they were formed, not re-derived from the cosines)
        // (WALK: the clamps decided on the sines, as in step_adjoint)
        const float hh = 0.5f / kHalfPi;
        const float u = fabsf(cos_i);
        const float s2t = (mu * mu) * s2;
        pen_cos2_i = (WALK ? s2 > kPenS2Min : u <= kAcosHi) ? -gq.th * hh * tl_rsq(s2) * tl_rcp(u) : 0.0f;
        b_cos2_t += (WALK ? s2t > kPenS2Min : cos_t <= kAcosHi) ? -gq.thp * hh * tl_rsq(s2t) * r_t : 0.0f;
    }
    b_mu -= b_g * cos_i + 2.0f * mu * s2 * b_cos2_t;
    const float b_cos_i = (-b_g * mu + 2.0f * (mu * mu) * cos_i * b_cos2_t) + 2.0f * cos_i * pen_cos2_i;
    bcx += b_cos_i * nx;
    bcy += b_cos_i * ny;
    float bcz = b_cos_i * nz;
    b_nx += b_cos_i * in.cx;
    b_ny += b_cos_i * in.cy;
    const float b_nz = b_cos_i * in.cz;
    // n = (-m X, -m Y, 1) inv_n
    const float b_invn = -m * (b_nx * X + b_ny * Y) + b_nz;
    float b_m = -inv_n * (b_nx * X + b_ny * Y);
    float bX = a.x - (m * inv_n) * b_nx;
    float bY = a.y - (m * inv_n) * b_ny;
    const float b_n2 = -0.5f * (inv_n * inv_n * inv_n) * b_invn;
    b_m += 2.0f * m * rho * b_n2;
    float b_rho = (m * m) * b_n2;
    const float b_dsag = 2.0f * b_m;
    b_rho += sag2 * b_dsag;
    float b_c = b_dsag * (0.5f * rq3);
    float b_kap = b_dsag * (0.25f * c3 * rho * rq3);
    float b_a0 = b_dsag * (2.0f * rho), b_a1 = b_dsag * (3.0f * rho2), b_a2 = b_dsag * (4.0f * rho3),
          b_a3 = b_dsag * (5.0f * rho4);
    bX += 2.0f * X * b_rho;
    bY += 2.0f * Y * b_rho;
    // X = x + s cx ; Y = y + s cy ; Z = z + s cz
    const float bZ = a.z;
    float bx = bX, by = bY, bz = bZ;
    bcx += bX * s;
    bcy += bY * s;
    bcz += bZ * s;
    const float b_s = ((bX * in.cx + bY * in.cy) + bZ * in.cz) + b_s_opd;
    // implicit function theorem on F = z + s cz - sag(rho(s)):  lambda = -b_s / F'
    const float Fp = in.cz - dsag * (2.0f * (X * in.cx + Y * in.cy));
    const float lam = -b_s * tl_rcp(Fp);
    const float lx = -lam * dsag * (2.0f * X), ly = -lam * dsag * (2.0f * Y);
    bz += lam;
    bcz += lam * s;
    bx += lx;
    by += ly;
    bcx += lx * s;
    bcy += ly * s;
    const float r1q = tl_rcp(1.0f + q);                    // 1/(1+q)
    b_c -= lam * rho * rq * r1q;                           // dF/dc   = -rho / (q (1+q))
    b_kap -= lam * (0.5f * c3 * rho2 * rq * r1q * r1q);    // dF/dk   = -c^3 rho^2 / (2 q (1+q)^2)
    b_a0 -= lam * rho2;
    b_a1 -= lam * rho3;
    b_a2 -= lam * rho4;
    b_a3 -= lam * (rho4 * rho);
    a.x = bx; a.y = by; a.z = bz; a.cx = bcx; a.cy = bcy; a.cz = bcz;
    g_c = b_c; g_mu = b_mu;
    g_asph[0] = b_kap; g_asph[1] = b_a0; g_asph[2] = b_a1; g_asph[3] = b_a2; g_asph[4] = b_a3;
}

// checkpoint kernel (and the rolled walk-back): values from the entering state, then the adjoint.  *s_out = the
// marching distance s.
template <bool PEN = false>
__device__ __forceinline__ void step_bwd_asph(const Ray &in, const float zout, const Asph &A, const float t,
                                              const float mu, Adj &a, float &g_c, float &g_t, float &g_mu,
                                              float g_asph[5], const PenSeed gq = PenSeed{}, const bool zpos = false,
                                              const float b_s_opd = 0.0f, float *s_out = nullptr)
{
    const AsphVals v = asph_vals(in, zout, A, t, mu);
    if (s_out) *s_out = v.s;
    asph_adjoint<PEN>(in, A, mu, v, a, g_c, g_t, g_mu, g_asph, gq, zpos, b_s_opd);
}

__device__ __forceinline__ float wave_sum_f32(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Walk-back: intersection of the line q + s d (s signed, negative when walking against d) with an aspheric
// row whose vertex is the origin of the frame of q.  Same scheme as step_fwd_asph -- closed-form sphere hit,
// then Newton steps with a wave-uniform count, leaving one step after every live lane passed the acceptance
// test -- but with the reverse sweep's arithmetic (v_rsq / v_rcp, contraction): nothing here has to
// reproduce the forward bit for bit.  A live lane still pending after kNewtonMax steps returns NaN, which
// reaches the entrance adjoint and hands the launch to the checkpoint kernel.
__device__ __forceinline__ void hit_asph(const Asph &A, const float qx, const float qy, const float qz,
                                         const float ddx, const float ddy, const float ddz, const bool live,
                                         float &HX, float &HY, float &HZ, float &S_)
{
#pragma clang fp contract(fast)
    const float e = -((qx * ddx + qy * ddy) + qz * ddz);
    const float mz = qz + e * ddz;
    const float m2 = ((qx * qx + qy * qy) + qz * qz) - e * e;
    const float tmp = A.c * m2 - 2.0f * mz;
    const float cos2 = ddz * ddz - A.c * tmp;
    float s = e + tmp * tl_rcp(ddz + cos2 * tl_rsq(cos2));
    const float kc2 = ((1.0f + A.kappa) * A.c) * A.c;
    bool pending = false;
#pragma unroll 1
    for (int it = 0; it < kNewtonMax; ++it) {
        const float X = qx + s * ddx, Y = qy + s * ddy;
        const float rho = X * X + Y * Y;
        const float q2 = 1.0f - kc2 * rho;
        const float rq = tl_rsq(q2);                                     // 1/q
        const float sag = (A.c * rho) * tl_rcp(1.0f + q2 * rq) + (rho * rho) * (A.a0 + rho * (A.a1 + rho * (A.a2 + rho * A.a3)));
        const float dsag = 0.5f * A.c * rq + rho * (2.0f * A.a0 + rho * (3.0f * A.a1 + rho * (4.0f * A.a2 + rho * (5.0f * A.a3))));
        const float zh = qz + s * ddz;
        const float F = zh - sag;
        const float Fp = ddz - dsag * (2.0f * (X * ddx + Y * ddy));
        pending = live && !(fabsf(F) <= kNewtonTol * (1.0f + fabsf(zh)));
        s = s - F * tl_rcp(Fp);
        if (__ballot(pending) == 0ull) break;
    }
    HX = pending ? __builtin_nanf("") : qx + s * ddx;
    HY = qy + s * ddy; HZ = qz + s * ddz;
    S_ = s;
}

// Transposed sum over the four lanes of a quad: lane 0 gets the sum of a, lane 1 of b, lanes 2 and 3 of c.
// Three DPP adds (each lane sends what its partner keeps), not six: a DPP operand costs about four plain
// VALU issues on gfx950 (measured: 6 DPP adds per surface = 6-8 % of the whole walk-back kernel).
template <int CTRL>
__device__ __forceinline__ float quad_perm(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}
__device__ __forceinline__ float quad_term_sums(float a, float b, float c, bool odd, bool hi)
{
    float x = odd ? b : a;                          // kept across the lane^1 exchange
    x += quad_perm<0xB1>(odd ? a : b);              // quad_perm:[1,0,3,2]: even a0+a1 | odd b1+b0
    const float m = c + quad_perm<0xB1>(c);         // c0+c1 on both lanes of the pair
    float z = hi ? m : x;                           // kept across the lane^2 exchange
    z += quad_perm<0x4E>(hi ? x : m);               // quad_perm:[2,3,0,1]
    return z;
}

// ------------------------------------------------------------------ reductions
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Which pupil points a block traces: the P points are cut into chunks of kBlock consecutive points (one per
// lane) and block b of the nbx = gridDim.x blocks of its (f, w) takes chunks [b*n/nbx, (b+1)*n/nbx): any grid
// size divides the work to within one chunk (the launch plan is not tied to an integer number of rays per lane).
#define TL_BLOCK_CHUNKS(P_)                                                                         \
    const int64_t nchunk_ = ((int64_t)(P_) + kBlock - 1) / kBlock;                                  \
    const int64_t c0 = (int64_t)blockIdx.x * nchunk_ / gridDim.x;                                   \
    const int R = (int)((int64_t)(blockIdx.x + 1) * nchunk_ / gridDim.x - c0)

// Scan map of the penalty walk-back: one byte per (row of the grid, 256-ray chunk, wave of the block) = "this wave holds a
// ray of that chunk which the walk-back left to the checkpoint pass" (dead on the way, or flagged ill-conditioned).
// Written by trace_bwd_inv_unrolled_kernel<.., PEN = true> next to the ok bytes it reads anyway, read by the selective
// pass of trace_bwd_kernel queued behind it: 64 chunks per look instead of a pass over every ray's ok byte (48 us at
// 16.8 M rays, most of it load latency).  It lives in the workspace right below the 256-byte slack that holds the poison
// word (tl_scanmap_bytes in tl_common.h is part of tl_workspace_bytes), so both kernels find it from that pointer.
__device__ __forceinline__ uint8_t *tl_scanmap(const unsigned *poison, const int rows, const int64_t nchunks)
{
    return (uint8_t *)poison + 64 - 256 - tl_scanmap_bytes(rows, nchunks);
}

// ------------------------------------------------------------------ lens batch
// blockIdx.y = (b F + f) W + w: lens b, field f, wavelength w.  `fw` (that row) addresses the per-ray outputs
// [B,F,W][P] and the block partials; `gf` = b F + f is the row of the per-field moments [B,F][TL_NMOM]; inside the
// kernel `p` is the problem of lens b alone (lens_view: every per-lens pointer advanced to that lens' slice), so the
// row code below is written for one lens.  All of it is wave-uniform scalar arithmetic, once per block.
__host__ __device__ __forceinline__ int tl_lenses(const tl_problem &p) { return p.B > 0 ? p.B : 1; }

__device__ __forceinline__ tl_problem lens_view(tl_problem p, const int b)
{
    const int64_t S = p.S, W = p.W;
    p.x_in += b * p.xs_b;
    p.y_in += b * p.ys_b;
    p.z += b;
    p.cx += b * p.cx_stride_b;
    p.cy += b * p.cy_stride_b;
    p.c += b * S;
    p.t += b * S;
    p.mu += b * W * S;
    p.mask += b * S;
    if (p.surf_kind) { p.kappa += b * S; p.poly += b * S * TL_MAX_POLY; p.surf_kind += b * S; }
    if (p.n_index) p.n_index += b * W * (S + 1);
    return p;
}
#define TL_LENS_ROW(PA_)                                                                            \
    const int fw = blockIdx.y;                                                                      \
    const int gf = fw / (PA_).W, w = fw - gf * (PA_).W;                                             \
    const int lens_ = gf / (PA_).F, f = gf - lens_ * (PA_).F;                                       \
    const tl_problem p = lens_view(PA_, lens_)

// ------------------------------------------------------------------ block stages shared by the trace kernels
// A stage that several kernels have is written once where every instantiation keeps the instruction stream it had with
// the stage in place (tools/isa_compare.py; record: profiles/kernels_shared_stages.txt).  An inline function is simplified
// on its own before it is inlined, so that holds for few of them: store_moment_partials here; the walk-backs' shared
// stages are macros (in front of trace_bwd_inv_kernel).  The field-row prologue (z0 .. yoff), the forward's image plane
// and the backward's moment seeds moved instructions in every shared form and stay written out per kernel.

// Epilogue of the forward kernels: the lane sums of a block -> its row of moment partials, stored [column][block].
__device__ __forceinline__ void store_moment_partials(const double (&m)[TL_NMOM], double *__restrict__ part, const int fw)
{
    __shared__ double red[kWaves][TL_NMOM];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < TL_NMOM; ++j) {
        const double v = wave_sum(m[j]);
        if (lane == 0) red[wv][j] = v;
    }
    __syncthreads();
    if (threadIdx.x < TL_NMOM) {
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < kWaves; ++q) s += red[q][threadIdx.x];
        part[(size_t)threadIdx.x * ((size_t)gridDim.y * gridDim.x) + ((size_t)fw * gridDim.x + blockIdx.x)] = s;   // [column][block]
    }
}

// ------------------------------------------------------------------ forward kernel
// grid (NBX, F*W), block kBlock; each thread traces R rays.
// part : [gridDim.y * gridDim.x][TL_NMOM] per-block moment partials (or nullptr)
// PEN : also evaluate the penalty-term quantities per surface;
//       stk (nullable): [3][S][F*W*P] per-surface stacks z_RELU | theta_norm | theta_prime_norm.
// ASPH: the lens has Newton rows (p.surf_kind != NULL).   OPD: accumulate the optical path length.
// Compile-time switches, so the reference's all-spherical path carries no per-surface branch or
// scalar load for features it does not use (measured: -13..18 % forward time vs run-time tests).
// the hit (X, Y) of this ray on aspheric row k_ -> slot j = number of aspheric rows before k_ (wave-uniform)
#define TL_STORE_HIT(k_)                                                                            \
    if (hits && valid) {                                                                            \
        const int j_ = __popc(kbits & ((1u << (k_)) - 1u));                                         \
        if (j_ < hit_slots) {                                                                       \
            float *h_ = hits + ((size_t)(2 * j_) * n_rays_all + ((size_t)fw * p.P + (size_t)ip));   \
            h_[0] = ray.x;                                                                          \
            h_[n_rays_all] = ray.y;                                                                 \
        }                                                                                           \
    }
template <bool PEN, bool ASPH, bool OPD>
__global__ __launch_bounds__(kBlock) void trace_fwd_kernel(
    const tl_problem pa, float *__restrict__ ox, float *__restrict__ oy, float *__restrict__ ocx,
    float *__restrict__ ocy, uint8_t *__restrict__ ook, uint8_t *__restrict__ oback,
    float *__restrict__ oopd, float *__restrict__ stk, double *__restrict__ part)
{
    // Fast mode, all-spherical lens: this instantiation only ever writes the path length behind trace_fwd_plain_kernel
    // (launch_fwd), and `ook` then holds that kernel's ok bytes, to be read: under contraction the two bodies round
    // differently, and a ray within rounding of a miss must not be dead in `ok` and carry a path length.
    constexpr bool kOkIn = TL_FAST && OPD && !ASPH && !PEN;
    TL_LENS_ROW(pa);
    TL_BLOCK_CHUNKS(p.P);
    const int S = p.S;
    const float z0 = p.z[0];
    const float cx0 = p.cx[f * p.cx_stride], cy0 = p.cy[f * p.cy_stride];
    const float cz0 = tl_sqrt((1.0f - cx0 * cx0) - cy0 * cy0);   // :609
    const float *__restrict__ mu_w = p.mu + (size_t)w * S;
    const float *__restrict__ n_w = OPD ? p.n_index + (size_t)w * (S + 1) : nullptr;
    const bool allow_back = p.allow_backward != 0;
    const unsigned mbits = row_bits(p.mask, S), kbits = ASPH ? row_bits(p.surf_kind, S) : 0u;
    const int64_t xoff = f * p.xs_f + w * p.xs_w, yoff = f * p.ys_f + w * p.ys_w;
    const bool want_x = p.moments_x != 0;                     // wave-uniform
    // ASPH: hit points of the aspheric rows for the walk-back kernel ([slot][X|Y][all rays of the launch])
    float *__restrict__ hits = ASPH ? p.asph_hits : nullptr;
    const int hit_slots = ASPH ? p.asph_hit_slots : 0;
    const size_t n_rays_all = (size_t)gridDim.y * p.P;
    // ASPH: which optional outputs are there, as bits of ONE scalar that is made opaque per ray below.  As plain pointer
    // tests they are hoisted out of the ray loop as nine wave-uniform booleans of two SGPRs each, and with the aspheric
    // rows' pointers that is more than the scalar file holds (13 spills to VGPR lanes, re-read per ray).  What is still
    // spilled with PEN or OPD is written before the ray loop and read after it.
    const unsigned out_bits_all = !ASPH ? 0u : (unsigned)__builtin_amdgcn_readfirstlane((int)(
        (ox ? 1u : 0u) | (oy ? 2u : 0u) | (ocx ? 4u : 0u) | (ocy ? 8u : 0u) | (ook ? 16u : 0u) | (oback ? 32u : 0u) |
        (p.cond_flags ? 64u : 0u) | (part ? 128u : 0u) | (want_x ? 256u : 0u) | (oopd ? 512u : 0u)));

    // per-lane sums: the value moments in fp64, the three counts (ok, back, ill-conditioned) as integers
    double m[TL_NMOM];
#pragma unroll
    for (int j = 0; j < TL_NMOM; ++j) m[j] = 0.0;
    int n_ok = 0, n_back = 0, n_ill = 0;

    // Software pipeline over the rays of this lane: the inputs of ray r+1 are requested before ray r is
    // traced, so their HBM latency (~900 cycles) overlaps the trace, and -- because vmcnt retires loads
    // and stores in issue order -- waiting for them never waits for the stores of ray r.  The prefetch is
    // UNCONDITIONAL (index clamped to a valid point, the last round re-reads its own): behind a branch
    // the compiler cannot count the loads in flight and waits for vmcnt(0) at the top of the surface
    // loop, i.e. for the prefetch it has just issued.  Lanes past the end trace a duplicate of the last
    // point; everything that leaves them is masked by `valid`.
    const int64_t ip_last = (int64_t)p.P - 1;
    const int64_t ip0 = c0 * kBlock + threadIdx.x;
    float x_nxt = p.x_in[xoff + (ip0 < ip_last ? ip0 : ip_last) * p.xs_p];
    float y_nxt = p.y_in[yoff + (ip0 < ip_last ? ip0 : ip_last) * p.ys_p];
    for (int r = 0; r < R; ++r) {
        const int64_t ip = (c0 + r) * kBlock + threadIdx.x;
        const bool valid = ip < p.P;
        unsigned out_bits = out_bits_all;
        if (ASPH) asm("" : "+s"(out_bits) : "s"(r));
        auto has = [&](const unsigned bit, const bool there) { return ASPH ? (out_bits & bit) != 0 : there; };
        Ray ray;
        ray.x = x_nxt;
        ray.y = y_nxt;
        {
            const int64_t ipn = ip + ((r + 1 < R) ? kBlock : 0);
            const int64_t ipc = ipn < ip_last ? ipn : ip_last;
            x_nxt = p.x_in[xoff + ipc * p.xs_p];
            y_nxt = p.y_in[yoff + ipc * p.ys_p];
        }
        ray.z = z0; ray.cx = cx0; ray.cy = cy0; ray.cz = cz0;
        bool ok = true, back = false;
        float opd = 0.0f;
        float s_th = 0.0f, s_thp = 0.0f, s_zr = 0.0f;      // PEN: per-ray sums over the surfaces
        float min_cos2 = 1.0f;                              // conditioning of this ray (see kCondThr)
        // One basic block per surface: the three scalar loads sit at its top and are waited for once.  (The
        // early exit is part of the loop condition, not a `break`: with a second exit edge the compiler
        // turns these wave-uniform loads into vector loads.)
        // (a wave whose 64 lanes are all past the end of the pupil -- small fans: P = 64 fills one wave of four --
        //  has nothing to trace)
        bool wave_live = __ballot(valid) != 0ull;
        for (int k = 0; k < S && wave_live; ++k) {
            const float ck = uload(p.c, k), tk = uload(p.t, k), muk = uload(mu_w, k);
            const bool chk = ((mbits << 1) >> k) & 1u;           // mask[k-1], false for k = 0
            if (PEN) {
                float c2i, c2t, th, thp;
                if (ASPH && ((kbits >> k) & 1u)) {     // wave-uniform branch
                    float d;
                    step_fwd_asph(ray, ok, back, load_asph(p, k), tk, muk, chk, allow_back, ok && valid, d, c2i, c2t);
                    th = theta_norm(c2i);
                    thp = theta_norm(c2t);
                    TL_STORE_HIT(k);
                } else {
                    float ui, ut;                      // the step's own sqrt(cos2): no second square root for the angles
                    step_fwd<true>(ray, ok, back, ck, tk, muk, chk, allow_back, c2i, c2t, ui, ut);
                    th = theta_from_cos(ui);
                    thp = theta_from_cos(ut);
                }
                th = ok ? th : 1.0f;
                thp = ok ? thp : 1.0f;
                const float zr = fmaxf(ok ? ray.z : -tk, 0.0f);      // parked rays sit at z = 0 - t
                s_th += th; s_thp += thp; s_zr += zr;
                min_cos2 = ok ? fminf(min_cos2, fminf(c2i, c2t)) : min_cos2;     // conditioning count, as below
                if (stk && valid) {
                    const size_t n = (size_t)gridDim.y * p.P, o = (size_t)fw * p.P + ip;
                    stk[(0 * (size_t)S + k) * n + o] = zr;
                    stk[(1 * (size_t)S + k) * n + o] = th;
                    stk[(2 * (size_t)S + k) * n + o] = thp;
                }
                continue;                                  // no early exit: dead rays still add theta = 1
            }
            float c2i, c2t;
            if (ASPH && ((kbits >> k) & 1u)) {         // wave-uniform branch
                float d;
                step_fwd_asph(ray, ok, back, load_asph(p, k), tk, muk, chk, allow_back, ok && valid, d, c2i, c2t);
                if (OPD) opd += uload(n_w, k) * d;
                TL_STORE_HIT(k);
            } else if (OPD) {
                const float z_in = ray.z, cz_in = ray.cz;
                step_fwd<true>(ray, ok, back, ck, tk, muk, chk, allow_back, c2i, c2t);
                opd += uload(n_w, k) * tl_div((ray.z + tk) - z_in, cz_in);     // d = dz / cz
            } else {
                step_fwd<true>(ray, ok, back, ck, tk, muk, chk, allow_back, c2i, c2t);
            }
            // every row type feeds the conditioning count (moment 9): the backward picks its algorithm by it
            min_cos2 = fminf(min_cos2, fminf(c2i, c2t));
            wave_live = __ballot(ok && valid) != 0ull;   // whole wave retired: nothing left to do
        }
        // image plane :660-670.  A ray retired on the way is parked at (0,0,.,0,0,1) by the
        // reference and therefore lands at exactly x = y = cx = cy = 0: apply that once, here.
        const float dz = -ray.z;
        const float dist = tl_div(dz, ray.cz);
        const bool alive = ok;
        const float xo = ok ? ray.x + dist * ray.cx : 0.0f;
        const float yo = ok ? ray.y + dist * ray.cy : 0.0f;
        ray.cx = ok ? ray.cx : 0.0f;
        ray.cy = ok ? ray.cy : 0.0f;
        {
            const bool hit = (dz < 0.0f) && ok && ((mbits >> (S - 1)) & 1u);
            if (allow_back) back = back || hit; else ok = ok && !hit;
        }
        if (valid) {
            const int64_t o = (int64_t)fw * p.P + ip;
            if (has(1u, ox != nullptr)) ox[o] = xo;
            if (has(2u, oy != nullptr)) oy[o] = yo;
            if (has(4u, ocx != nullptr)) ocx[o] = ray.cx;
            if (has(8u, ocy != nullptr)) ocy[o] = ray.cy;
            if (!kOkIn && has(16u, ook != nullptr)) ook[o] = ok ? 1 : 0;
            if (has(32u, oback != nullptr)) oback[o] = back ? 1 : 0;
            if (has(64u, p.cond_flags != nullptr)) p.cond_flags[o] = alive ? (min_cos2 < kCondThr ? 2 : 1) : 0;  // 2: the rays moment 9 counts
            // kOkIn: a ray that the kernel before this one gave up has no path length, whatever this one makes of it
            // (a ray that only lost `ok` at the image plane, where backward rays are not allowed, keeps its own)
            const bool path = (kOkIn && ook) ? alive && (ook[o] != 0 || (!allow_back && !ok)) : alive;
            if (OPD && has(512u, oopd != nullptr)) oopd[o] = path ? opd + uload(n_w, S) * dist : 0.0f;
            if (has(128u, part != nullptr)) {
                // (ok differs from alive only where backward rays are not allowed; the squares are exact in fp64)
                const double yd = (double)yo, ykd = (double)(ok ? yo : 0.0f);
                m[0] += yd; m[1] += ykd; m[2] = __builtin_fma(ykd, ykd, m[2]);
                n_ok += ok ? 1 : 0; n_back += back ? 1 : 0;
                n_ill += (alive && min_cos2 < kCondThr) ? 1 : 0;
                if (has(256u, want_x)) {           // compute_rms2d reads y only (:684-701); the 2-D spot radius asks for these
                    const double xd = (double)xo, xkd = (double)(ok ? xo : 0.0f);
                    m[4] += xd; m[5] += xkd; m[6] = __builtin_fma(xkd, xkd, m[6]);
                }
                if (PEN) {
                    const float q = (s_th + s_thp) + s_zr;
                    m[8] += (q != q) ? 0.0 : (double)q;        // NaN -> 0 (optics_simulator_lite.py:446)
                }
            }
        }
    }
    if (part) {
        m[3] = (double)n_ok; m[7] = (double)n_back; m[9] = (double)n_ill;
        store_moment_partials(m, part, fw);
    }
}

// ------------------------------------------------------------------ forward kernel, all-spherical fast path
// Same results as trace_fwd_kernel<false,false,false> (same per-ray operations, same summation order of
// the moments), but every lane carries RPL independent rays through the surface loop together: the
// scalar side of a surface (three s_load + wait, loop control, mask bits) is paid once per RPL rays and
// the two dependent FMA chains interleave in one wave.
template <int RPL>
__global__ __launch_bounds__(kBlock) void trace_fwd_plain_kernel(
    const tl_problem pa, float *__restrict__ ox, float *__restrict__ oy, float *__restrict__ ocx,
    float *__restrict__ ocy, uint8_t *__restrict__ ook, uint8_t *__restrict__ oback,
    double *__restrict__ part)
{
    TL_LENS_ROW(pa);
    TL_BLOCK_CHUNKS(p.P);
    const int S = p.S;
    const float z0 = p.z[0];
    const float cx0 = p.cx[f * p.cx_stride], cy0 = p.cy[f * p.cy_stride];
    const float cz0 = tl_sqrt((1.0f - cx0 * cx0) - cy0 * cy0);
    const float *__restrict__ mu_w = p.mu + (size_t)w * S;
    const bool allow_back = p.allow_backward != 0;
    const unsigned mbits = row_bits(p.mask, S);
    const int64_t xoff = f * p.xs_f + w * p.xs_w, yoff = f * p.ys_f + w * p.ys_w;
    const bool want_x = p.moments_x != 0;

    double m[TL_NMOM];
#pragma unroll
    for (int j = 0; j < TL_NMOM; ++j) m[j] = 0.0;
    int n_ok = 0, n_back = 0, n_ill = 0;

    // round j traces rays r = j*RPL + q, q < RPL, of this lane; its inputs were requested during round j-1
    // (unconditional, clamped prefetch: see trace_fwd_kernel)
    const int rounds = (R + RPL - 1) / RPL;
    const int64_t ip_last = (int64_t)p.P - 1;
    const int64_t ip_base = c0 * kBlock + threadIdx.x;
    float x_nxt[RPL], y_nxt[RPL];
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int64_t i = ip_base + (int64_t)(q < R ? q : 0) * kBlock;
        const int64_t ic = i < ip_last ? i : ip_last;
        x_nxt[q] = p.x_in[xoff + ic * p.xs_p];
        y_nxt[q] = p.y_in[yoff + ic * p.ys_p];
    }
    for (int j = 0; j < rounds; ++j) {
        Ray ray[RPL];
        bool ok[RPL], back[RPL], valid[RPL];
        float min_cos2[RPL];
        int64_t ip[RPL];
#pragma unroll
        for (int q = 0; q < RPL; ++q) {
            const int r = j * RPL + q;
            ip[q] = ip_base + (int64_t)r * kBlock;
            valid[q] = (r < R) && (ip[q] < p.P);
            ray[q].x = x_nxt[q]; ray[q].y = y_nxt[q];
            ray[q].z = z0; ray[q].cx = cx0; ray[q].cy = cy0; ray[q].cz = cz0;
            ok[q] = true; back[q] = false; min_cos2[q] = 1.0f;
            const int rn = r + RPL;
            const int64_t i = ip_base + (int64_t)(rn < R ? rn : (r < R ? r : 0)) * kBlock;
            const int64_t ic = i < ip_last ? i : ip_last;
            x_nxt[q] = p.x_in[xoff + ic * p.xs_p];
            y_nxt[q] = p.y_in[yoff + ic * p.ys_p];
        }
        bool any_valid = false;
#pragma unroll
        for (int q = 0; q < RPL; ++q) any_valid = any_valid || valid[q];
        bool wave_live = __ballot(any_valid) != 0ull;             // all lanes past the end of the pupil: nothing to trace
        for (int k = 0; k < S && wave_live; ++k) {
            const float ck = uload(p.c, k), tk = uload(p.t, k), muk = uload(mu_w, k);
            const bool chk = ((mbits << 1) >> k) & 1u;
            bool any = false;
#pragma unroll
            for (int q = 0; q < RPL; ++q) {
                float c2i, c2t;
                step_fwd<true>(ray[q], ok[q], back[q], ck, tk, muk, chk, allow_back, c2i, c2t);
                min_cos2[q] = fminf(min_cos2[q], fminf(c2i, c2t));
                any = any || (ok[q] && valid[q]);
            }
            wave_live = __ballot(any) != 0ull;
        }
#pragma unroll
        for (int q = 0; q < RPL; ++q) {
            const float dz = -ray[q].z;
            const float dist = tl_div(dz, ray[q].cz);
            const bool alive = ok[q];
            const float xo = alive ? ray[q].x + dist * ray[q].cx : 0.0f;
            const float yo = alive ? ray[q].y + dist * ray[q].cy : 0.0f;
            const float cxo = alive ? ray[q].cx : 0.0f, cyo = alive ? ray[q].cy : 0.0f;
            {
                const bool hit = (dz < 0.0f) && ok[q] && ((mbits >> (S - 1)) & 1u);
                if (allow_back) back[q] = back[q] || hit; else ok[q] = ok[q] && !hit;
            }
            if (valid[q]) {
                const int64_t o = (int64_t)fw * p.P + ip[q];
                if (ox) ox[o] = xo;
                if (oy) oy[o] = yo;
                if (ocx) ocx[o] = cxo;
                if (ocy) ocy[o] = cyo;
                if (ook) ook[o] = ok[q] ? 1 : 0;
                if (oback) oback[o] = back[q] ? 1 : 0;
                if (p.cond_flags) p.cond_flags[o] = alive ? (min_cos2[q] < kCondThr ? 2 : 1) : 0;
                if (part) {
                    const double yd = (double)yo, ykd = (double)(ok[q] ? yo : 0.0f);
                    m[0] += yd; m[1] += ykd; m[2] = __builtin_fma(ykd, ykd, m[2]);
                    n_ok += ok[q] ? 1 : 0; n_back += back[q] ? 1 : 0;
                    n_ill += (alive && min_cos2[q] < kCondThr) ? 1 : 0;
                    if (want_x) {
                        const double xd = (double)xo, xkd = (double)(ok[q] ? xo : 0.0f);
                        m[4] += xd; m[5] += xkd; m[6] = __builtin_fma(xkd, xkd, m[6]);
                    }
                }
            }
        }
    }
    if (part) {
        m[3] = (double)n_ok; m[7] = (double)n_back; m[9] = (double)n_ill;
        store_moment_partials(m, part, fw);
    }
}

// ------------------------------------------------------------------ backward kernel
// NS = compile-time bound on the surface rows (S <= NS); the surface loops are fully
// unrolled so the per-surface checkpoints (state entering each surface, 6 floats) live in VGPRs.
// The 3*NS per-lane gradient accumulators live in LDS instead: every lane owns one private
// 4-byte slot per accumulator (slot [j][tid]: consecutive lanes -> consecutive banks, conflict
// free) and updates it with a plain ds_read / v_add / ds_write (no other lane ever touches the
// slot, so no atomic is needed -- and ds_add_f32 measured ~200 cycles per wave-instruction on
// gfx950, 3x slower end to end).  That frees 3*NS VGPRs per lane, which is what lets 4 waves per
// SIMD stay resident at NS = 12.
// part : [nblocks][tl_bwd_row(NS, asph)] doubles: g_c[NS] | g_t[NS] | g_mu[NS] | g_z | g_cx | g_cy [| g_kappa[NS] | g_poly[NS][4]] | g_n[NS+1]
#ifndef TL_BWD_WAVES
#define TL_BWD_WAVES(NS) ((NS) <= 12 ? 4 : (NS) <= 16 ? 3 : (NS) <= 24 ? 2 : 1)   // waves per SIMD that VGPRs + LDS allow
#endif
// PEN (all-spherical only): also back-propagate the penalty term.  Unlike the spot loss, the penalty
// keeps gradient for rays that die LATER: theta_k / zRELU_k of the surfaces a ray passed alive were
// computed before it was parked, so the reverse sweep starts, per ray, at its last live surface
// (`live` bit k = ok after surface k); parked rays only feed d/dt_k through zRELU = max(-t_k, 0).
// PEN is tri-state (PenMode): kPenNone; kPenUniform, the fused seed gq of moment 8 for every row and ray; kPenRay, gq plus
// the per-ray seeds of the stacks (gstk: [3][S][rows of the grid * P], the layout of tl_trace_fwd's `stacks`), read row
// by row inside the reverse sweep.  A ray that died on the way is differentiated whenever a stack seed is given, even
// with gq = 0 (a loss on the stacks alone).  gstk is NULL and never read for the other two.
enum PenMode : int { kPenNone = 0, kPenUniform = 1, kPenRay = 2 };
template <int NS, bool ASPH, int PEN>
__global__ __launch_bounds__(kBlock, TL_BWD_WAVES(NS)) void trace_bwd_kernel(
    const tl_problem pa, const float *__restrict__ gx, const float *__restrict__ gy,
    const float *__restrict__ gcx, const float *__restrict__ gcy, const double *__restrict__ gmom,
    float *__restrict__ gxin, float *__restrict__ gyin, double *__restrict__ part,
    const double *__restrict__ fb_mom, const unsigned *__restrict__ fb_poison, const unsigned fb_token,
    const float *__restrict__ gopd, const uint8_t *__restrict__ dead_ok, const float *__restrict__ gstk)
{
    constexpr bool PENB = PEN != kPenNone, STK = PEN == kPenRay;
    // launched as the fallback of a walk-back kernel (fb_poison given): run only when that launch did not do the job --
    // or, for the penalty term (dead_ok = the forward's ok bytes: 0 dead, 1 live), over exactly the rays the walk-back cannot take:
    // those that died on the way still carry the gradient of the rows they passed alive.  Waves none of whose rays
    // died skip the chunk after reading its ok bytes.
    // Likewise for ill-conditioned rays when the forward left their flags (pa.cond_flags: dead_ok then holds 2 for them): the
    // walk-back took every other ray, this launch takes the flagged ones.  Without flags, one such ray hands the whole
    // launch over (fallback_needed).
    bool only_rest = false;                          // selective pass: only the rays the walk-back left out
    bool take_ill = false;                           // ... among them the flagged ones (wave-uniform)
    if (fb_poison) {
        const bool ill = fb_mom && ill_conditioned(fb_mom, pa.F * tl_lenses(pa));
        if (*fb_poison != fb_token && !(ill && !pa.cond_flags)) {
            take_ill = ill && dead_ok;
            if (!(PEN && dead_ok) && !take_ill) return;
            only_rest = true;
        }
    }
    constexpr int NB = (ASPH ? 8 : 3) * NS + 3;      // + g_kappa[NS] | g_poly[NS][4] when ASPH
    // columns NB .. NB+NS: g_n[NS+1] (gradient through the optical path length); tl_bwd_row(NS, ASPH) columns in all
    __shared__ float sacc[3 * NS][kBlock];
    __shared__ double red[kWaves][4];
    __shared__ float sasph[ASPH ? 5 * NS : 1][kWaves];   // per-wave sums of the aspheric-coefficient gradients
    // gopd (nullable): upstream gradient of the optical path length OPD = sum_k n_k d_k + n_S d_image per ray.  It
    // enters the adjoint of every marching distance (b_d += gopd n_k) and gives d/dn_k = sum_rays gopd d_k, kept as
    // per-wave sums here (a wave sum per row and ray: this optional path is not tuned)
    __shared__ float sgn[NS + 1][kWaves];
    const int tid = threadIdx.x;
    TL_LENS_ROW(pa);
    TL_BLOCK_CHUNKS(p.P);
    const float *__restrict__ n_w = gopd ? p.n_index + (size_t)w * (p.S + 1) : nullptr;
    const int S = p.S;
    const float z0 = p.z[0];
    const float cx0 = p.cx[f * p.cx_stride], cy0 = p.cy[f * p.cy_stride];
    const float cz0 = tl_sqrt((1.0f - cx0 * cx0) - cy0 * cy0);
    const float *__restrict__ mu_w = p.mu + (size_t)w * S;
    const bool allow_back = p.allow_backward != 0;
    const unsigned mbits = row_bits(p.mask, S), kbits = ASPH ? row_bits(p.surf_kind, S) : 0u;
    const int64_t xoff = f * p.xs_f + w * p.xs_w, yoff = f * p.ys_f + w * p.ys_w;

    // upstream gradient of the moments of this field (wave-uniform)
    double gm0 = 0, gm1 = 0, gm2 = 0, gm4 = 0, gm5 = 0, gm6 = 0;
    if (gmom) {
        const double *q = gmom + (size_t)gf * TL_NMOM;
        gm0 = q[0]; gm1 = q[1]; gm2 = q[2]; gm4 = q[4]; gm5 = q[5]; gm6 = q[6];
    }
    const float gq = (PEN && gmom) ? (float)gmom[(size_t)gf * TL_NMOM + 8] : 0.0f;

    if (PEN && only_rest) {
        // Selective pass behind a penalty walk-back: a block none of whose waves was left a ray (the scan map says so; every
        // block of a healthy fan) writes its row of zero partials and leaves -- no accumulators to clear, no sums to form
        const uint8_t *__restrict__ sc = tl_scanmap(fb_poison, (int)gridDim.y, nchunk_) + ((size_t)fw * nchunk_ + c0) * kWaves;
        int any = 0;
        for (int j = tid; j < R * kWaves; j += kBlock) any |= sc[j];
        if (__syncthreads_or(any) == 0) {
            const size_t nrows_ = (size_t)gridDim.y * gridDim.x;
            double *row = part + ((size_t)fw * gridDim.x + blockIdx.x);
            for (int j = tid; j < tl_bwd_row(NS, ASPH); j += kBlock) row[(size_t)j * nrows_] = 0.0;
            return;
        }
    }
#pragma unroll
    for (int j = 0; j < 3 * NS; ++j) sacc[j][tid] = 0.0f;      // own slots only: no barrier needed
    if (ASPH && (tid & 63) == 0)
        for (int j = 0; j < 5 * NS; ++j) sasph[j][tid >> 6] = 0.0f;   // touched by lane 0 of this wave only
    if ((tid & 63) == 0)
        for (int j = 0; j <= NS; ++j) sgn[j][tid >> 6] = 0.0f;        // likewise
    // entrance adjoints summed per lane in fp64: g_z and g_cy are small residuals (~1e-3) of large per-ray
    // terms, so the fp32 rounding of a running sum over the rays of a lane would show up 1000-fold
    double acc_z = 0.0, acc_cx = 0.0, acc_cy = 0.0, acc_cz = 0.0;

    // inputs of ray r+1 are requested before ray r is processed (see trace_fwd_kernel)
    const int64_t ip0 = c0 * kBlock + tid;
    float x_nxt = (ip0 < p.P && !only_rest) ? p.x_in[xoff + ip0 * p.xs_p] : 0.0f;
    float y_nxt = (ip0 < p.P && !only_rest) ? p.y_in[yoff + ip0 * p.ys_p] : 0.0f;
    unsigned long long look = 0ull;      // selective pass: bit j = chunk look_r0 + j holds a ray of this wave to take (scalar)
    int look_r0 = -64, look_n = 64;
    // PEN: the walk-back in front of this launch left the scan map (tl_scanmap): one byte per chunk and wave
    const uint8_t *__restrict__ scan = (PEN && only_rest) ? tl_scanmap(fb_poison, (int)gridDim.y, nchunk_) + ((size_t)fw * nchunk_ + c0) * kWaves
                                                                + __builtin_amdgcn_readfirstlane(tid >> 6) : nullptr;
    for (int r = 0; r < R; ++r) {
        if (only_rest) {
            if (r >= look_r0 + look_n) {
                look_r0 = r;
                if (PEN) {
                    // 64 chunks per look: lane j reads this wave's byte of chunk r + j
                    const int j = tid & 63;
                    const uint8_t b = (r + j < R) ? scan[(size_t)(r + j) * kWaves] : (uint8_t)0;
                    look = __ballot(b != 0);
                } else {
                    // no scan map (ill-conditioned rays behind a walk-back without the penalty term): one look covers eight
                    // chunks with eight independent ok-byte loads and keeps one scalar mask (with one chunk's byte per loop
                    // trip the pass was bound by the latency of a single load per wave: 64 trips of ~1 us)
                    look = 0ull;
                    look_n = 8;
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int64_t ipj = (c0 + r + j) * kBlock + tid;
                        const bool vj = (r + j < R) && (ipj < p.P);
                        const uint8_t b = dead_ok[vj ? (int64_t)fw * p.P + ipj : 0];
                        const bool tj = vj && (take_ill && b == 2);
                        look |= (__ballot(tj) != 0ull ? 1ull : 0ull) << j;
                    }
                }
            }
            if (((look >> (r - look_r0)) & 1ull) == 0ull) continue;
        }
        const int64_t ip = (c0 + r) * kBlock + tid;
        const bool valid = ip < p.P;
        Ray ray;
        ray.x = x_nxt;
        ray.y = y_nxt;
        if (only_rest) {                 // (no prefetch across skipped chunks: the few chunks taken load on demand)
            ray.x = valid ? p.x_in[xoff + ip * p.xs_p] : 0.0f;
            ray.y = valid ? p.y_in[yoff + ip * p.ys_p] : 0.0f;
        } else {
            const int64_t ipn = ip + kBlock;
            const bool more = (r + 1 < R) && (ipn < p.P);
            x_nxt = more ? p.x_in[xoff + ipn * p.xs_p] : 0.0f;
            y_nxt = more ? p.y_in[yoff + ipn * p.ys_p] : 0.0f;
        }
        // a wave whose 64 lanes are all past the end of the pupil (small fans: P = 64 fills one wave of four)
        if (__ballot(valid) == 0ull) continue;
        // `take`: this lane's ray is this launch's to differentiate
        bool take = valid;
        if (only_rest) {
            const uint8_t okb = dead_ok[valid ? (int64_t)fw * p.P + ip : 0];
            take = valid && ((PEN && okb == 0) || (take_ill && okb == 2));
        }
        ray.z = z0; ray.cx = cx0; ray.cy = cy0; ray.cz = cz0;
        bool ok = true, back = false;
        unsigned live = 0u;             // PEN: bit k = ray ok after surface k

        Ray ck[NS];                     // state entering each surface
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            if (k < S) {
                ck[k] = ray;
                const bool chk = ((mbits << 1) >> k) & 1u;       // mask[k-1], false for k = 0
                if (ASPH && ((kbits >> k) & 1u)) {
                    float d, u0, u1;
                    step_fwd_asph(ray, ok, back, load_asph(p, k), uload(p.t, k), uload(mu_w, k), chk, allow_back, ok && valid, d, u0, u1);
                } else {
                    step_fwd<true>(ray, ok, back, uload(p.c, k), uload(p.t, k), uload(mu_w, k), chk, allow_back);
                }
                if (PEN) live |= ((ok && take) ? 1u : 0u) << k;
            }
        }
        const float z_last = ray.z;          // z leaving the last surface (before the image transfer)
        const bool alive = ok && take;       // alive after the last surface: gradient flows
        const float dz = -ray.z;
        const float inv_cz = tl_rcp(ray.cz);
        const float dist = tl_div(dz, ray.cz);      // same value as the forward kernel: the seed needs y bit-equal
        const float xo = ray.x + dist * ray.cx;
        const float yo = ray.y + dist * ray.cy;
        if (!allow_back) ok = ok && !((dz < 0.0f) && ok && ((mbits >> (S - 1)) & 1u));

        const int64_t o = (int64_t)fw * p.P + ip;
        if (__ballot(PEN ? (take && (STK || gq != 0.0f)) || alive : alive) == 0ull) {   // wave-uniform: nothing to differentiate
            if (take) { if (gxin) gxin[o] = 0.0f; if (gyin) gyin[o] = 0.0f; }
            continue;
        }
        // ---- seeds
        float sx = (gx && valid) ? gx[o] : 0.0f;
        float sy = (gy && valid) ? gy[o] : 0.0f;
        const float scx = (gcx && valid) ? gcx[o] : 0.0f;
        const float scy = (gcy && valid) ? gcy[o] : 0.0f;
        if (gmom) {
            const double okd = ok ? 1.0 : 0.0;
            sy += (float)(gm0 + okd * (gm1 + 2.0 * (double)yo * gm2));
            sx += (float)(gm4 + okd * (gm5 + 2.0 * (double)xo * gm6));
        }
        // ---- image plane adjoint: xo = x + dist*cx ; dist = -z/cz ; OPD += n_S dist
        const float go = (gopd && alive) ? gopd[o] : 0.0f;         // failed rays have OPD = 0: no gradient
        Adj a;
        const float b_dist = (sx * ray.cx + sy * ray.cy) + (gopd ? go * uload(n_w, S) : 0.0f);
        a.x = sx; a.y = sy;
        a.cx = scx + sx * dist;
        a.cy = scy + sy * dist;
        a.z = -b_dist * inv_cz;
        a.cz = -b_dist * dist * inv_cz;
        if (PEN && !alive) { a.x = a.y = a.z = a.cx = a.cy = a.cz = 0.0f; }
        if (gopd) {
            // a select, not go * dist with go = 0: a dead lane's dist may be NaN (LEAN re-trace), and 0 * NaN is NaN
            const float v = wave_sum_f32(alive ? go * dist : 0.0f);
            if ((tid & 63) == 0) sgn[S][tid >> 6] += v;
        }
        // ---- reverse sweep (dead lanes carry garbage, masked where it leaves the lane)
#pragma unroll
        for (int k = NS - 1; k >= 0; --k) {
            if (k < S) {
                float g_c, g_t, g_mu;
                const bool lk = PEN ? ((live >> k) & 1u) != 0u : alive;
                // fetch this surface's three accumulators now: the LDS latency overlaps the adjoint below
                const float s_c = sacc[k][tid], s_t = sacc[NS + k][tid], s_mu = sacc[2 * NS + k][tid];
                const float zout = (k + 1 < NS && k + 1 < S) ? ck[k + 1 < NS ? k + 1 : k].z : z_last;
                const float b_d_opd = gopd ? go * uload(n_w, k) : 0.0f;
                float d_k = 0.0f;                                  // marching distance of this row (gopd only)
                PenSeed sk = pen_seed(gq);                         // this row's seeds of zRELU, theta, theta'
                if (STK && take) {
                    const size_t n_st = (size_t)gridDim.y * p.P;
                    const float *__restrict__ q = gstk + ((size_t)k * n_st + (size_t)o);
                    sk.z += q[0];
                    sk.th += q[(size_t)S * n_st];
                    sk.thp += q[2 * (size_t)S * n_st];
                }
                if (ASPH && ((kbits >> k) & 1u)) {
                    float ga[5];
                    step_bwd_asph<PENB>(ck[k], zout, load_asph(p, k), uload(p.t, k), uload(mu_w, k), a, g_c, g_t, g_mu, ga, sk, zout > 0.0f,
                                        b_d_opd, gopd ? &d_k : nullptr);
#pragma unroll
                    for (int j = 0; j < 5; ++j) {
                        const float v = wave_sum_f32(lk ? ga[j] : 0.0f);
                        if ((tid & 63) == 0) sasph[5 * k + j][tid >> 6] += v;
                    }
                } else {
                    step_bwd<PENB>(ck[k], uload(p.c, k), uload(mu_w, k), a, g_c, g_t, g_mu, sk, zout > 0.0f, b_d_opd, gopd ? &d_k : nullptr);
                }
                if (PEN && !lk) { a.x = a.y = a.z = a.cx = a.cy = a.cz = 0.0f; }     // parked after k: nothing flows below
                if (gopd) {
                    const float v = wave_sum_f32(alive ? go * d_k : 0.0f);     // (spherical and aspheric rows alike)
                    if ((tid & 63) == 0) sgn[k][tid >> 6] += v;
                }
                if (lk) {
                    sacc[k][tid] = s_c + g_c;
                    sacc[NS + k][tid] = s_t + g_t;
                    sacc[2 * NS + k][tid] = s_mu + g_mu;
                } else if (PEN && take && -uload(p.t, k) > 0.0f) {
                    sacc[NS + k][tid] = s_t - sk.z;   // parked ray: zRELU_k = max(0 - t_k, 0)
                }
            }
        }
        // ---- entrance.  cz0 = sqrt(1 - cx0^2 - cy0^2) is the same for every ray of the block, so
        // d(cz0)/d(cx0,cy0) is applied ONCE to the summed adjoint, in fp64, in the epilogue: a per-ray
        // multiply by an fp32 1/cz0 would put the same rounding error into every term, and the two
        // sums cancel to ~1e-3 of their size for a well-corrected lens (measured 6.7e-4 error in g_cy).
        const bool l0 = PEN ? (live & 1u) != 0u : alive;      // the entrance adjoint exists
        if (l0) {
            acc_z += (double)a.z;
            acc_cx += (double)a.cx;
            acc_cy += (double)a.cy;
            acc_cz += (double)a.cz;
        }
        if (take) {         // (selective pass: the walk-back kernel wrote the per-ray input gradients of the rays it took)
            if (gxin) gxin[o] = l0 ? a.x : 0.0f;
            if (gyin) gyin[o] = l0 ? a.y : 0.0f;
        }
    }

    // ---- block reduction (fixed order => bitwise reproducible)
    const int lane = tid & 63, wv = tid >> 6;
    {
        const double a0 = wave_sum(acc_z), a1 = wave_sum(acc_cx), a2 = wave_sum(acc_cy);
        const double a3 = wave_sum(acc_cz);
        if (lane == 0) { red[wv][0] = a0; red[wv][1] = a1; red[wv][2] = a2; red[wv][3] = a3; }
    }
    __syncthreads();
    // partials are stored [column][block] (the reduction kernels then read each column as one contiguous run)
    const size_t nrows_ = (size_t)gridDim.y * gridDim.x;
    double *row = part + ((size_t)fw * gridDim.x + blockIdx.x);
    // wave wv reduces accumulator rows wv, wv+4, ...: 4 conflict-free LDS reads + a wave sum each
    for (int j = wv; j < 3 * NS; j += kWaves) {
        double v = (double)sacc[j][lane] + (double)sacc[j][lane + 64];
        v += (double)sacc[j][lane + 128];
        v += (double)sacc[j][lane + 192];
        v = wave_sum(v);
        if (lane == 0) row[(size_t)(j) * nrows_] = v;
    }
    if (tid < 3) {
        double v = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
        if (tid > 0) {      // g_cx, g_cy: add  S_cz * d(cz0)/d(c{x,y}0) = -S_cz * c{x,y}0 / cz0, in fp64
            const double s_cz = ((red[0][3] + red[1][3]) + red[2][3]) + red[3][3];
            const double cxd = (double)cx0, cyd = (double)cy0;
            v -= s_cz * (tid == 1 ? cxd : cyd) / sqrt((1.0 - cxd * cxd) - cyd * cyd);
        }
        row[(size_t)(3 * NS + tid) * nrows_] = v;
    }
    if (ASPH) {
        // g_kappa[k] -> column 3NS+3+k ; g_poly[k][j] -> column 4NS+3+4k+j   (sasph row 5k+{0,1..4})
        for (int j = tid; j < 5 * NS; j += kBlock) {
            const int k = j / 5, jj = j - 5 * k;
            const double v = (((double)sasph[j][0] + (double)sasph[j][1]) + (double)sasph[j][2]) + (double)sasph[j][3];
            row[(size_t)(jj == 0 ? 3 * NS + 3 + k : 4 * NS + 3 + 4 * k + (jj - 1)) * nrows_] = v;
        }
    }
    if (gopd && tid <= NS)        // g_n[k] -> column NB + k
        row[(size_t)(NB + tid) * nrows_] = (((double)sgn[tid][0] + (double)sgn[tid][1]) + (double)sgn[tid][2]) + (double)sgn[tid][3];
}

// a wave-uniform double, moved from vector to scalar registers
__device__ __forceinline__ double uniform_f64(const double v)
{
    const long long b = __double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)b);
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)((unsigned long long)b >> 32));
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// ------------------------------------------------------------------ stages shared by the two walk-back kernels
// Macros: as inline functions each of them changed the register assignment or the instruction order of walk-back
// instantiations (profiles/kernels_shared_stages.txt); expanded in place they are the code that was there.
// TL_HIT: intersect the line (q, d) with a sphere of curvature c whose vertex is the origin (closed form of
// find_marching_distance_spherical; the signed distance DB is negative when walking against d); COS = cosine between d
// and the normal at the hit, RCOS its reciprocal.  AFTER_COS_ names what else is formed from the intermediates:
// TL_HIT_PLAIN nothing, TL_HIT_S2T the caller's `s2t` (PEN: sin^2 on the refraction side, see
// trace_bwd_inv_unrolled_kernel).
#define TL_HIT_PLAIN(c_, ddx, ddy, tmp_)
#define TL_HIT_S2T(c_, ddx, ddy, tmp_) if (PEN) s2t = ((ddx) * (ddx) + (ddy) * (ddy)) + (c_) * tmp_;
#define TL_HIT(AFTER_COS_, c_, qx_, qy_, qz_, ddx, ddy, ddz, HX, HY, HZ, COS, RCOS, DB)  \
        {                                                                                \
            const float e_ = -(((qx_) * (ddx) + (qy_) * (ddy)) + (qz_) * (ddz));         \
            const float mz_ = (qz_) + e_ * (ddz);                                        \
            const float m2_ = (((qx_) * (qx_) + (qy_) * (qy_)) + (qz_) * (qz_)) - e_ * e_; \
            const float tmp_ = (c_) * m2_ - 2.0f * mz_;                                  \
            const float cos2_ = (ddz) * (ddz) - (c_) * tmp_;                             \
            tl_rsq_sqrt(cos2_, RCOS, COS);                                               \
            AFTER_COS_(c_, ddx, ddy, tmp_)                                               \
            DB = e_ + tmp_ * tl_rcp((ddz) + COS);                                        \
            HX = (qx_) + DB * (ddx); HY = (qy_) + DB * (ddy); HZ = (qz_) + DB * (ddz);   \
        }

// TL_WALK_ENTRANCE_SUMS declares the entrance adjoints of a lane, summed over its rays in fp64 (see trace_bwd_kernel):
// acc_z, acc_cx, acc_cy.  The cz term is folded into cx and cy per ray (cz0 = sqrt(1 - cx0^2 - cy0^2): d cz0 / d cx0 =
// -cx0 / cz0), which saves a fourth fp64 sum; k_cx, k_cy are wave-uniform: moved to SGPRs, they cost no vector register.
#define TL_WALK_ENTRANCE_SUMS(cx0_, cy0_)                                                                            \
    const double rcz0_ = 1.0 / sqrt((1.0 - (double)(cx0_) * (double)(cx0_)) - (double)(cy0_) * (double)(cy0_));      \
    const double k_cx = uniform_f64(-(double)(cx0_) * rcz0_), k_cy = uniform_f64(-(double)(cy0_) * rcz0_);           \
    double acc_z = 0.0, acc_cx = 0.0, acc_cy = 0.0
// TL_WALK_ENTRANCE_ADD: one ray's adjoint `a` at the entrance.  Every term of the sweep is linear in the adjoint, so
// anything non-finite on the way (cannot happen for a ray the forward kept and called well-conditioned, short of a
// pathological prescription) is still there: flag it, and the checkpoint kernel redoes the launch bit-faithfully.
// (A plain store: an atomic here makes the compiler treat every later load of the prescription as clobbered and turn
// the per-surface scalar loads into vector loads, +4 % on the whole kernel.)
#define TL_WALK_ENTRANCE_ADD(a_)                                                                                     \
        const float fin_ = (((a_).x + (a_).y) + ((a_).z + (a_).cz)) + ((a_).cx + (a_).cy);                           \
        if (!(fin_ - fin_ == 0.0f)) *poison = token;                                                                 \
        acc_z += (double)(a_).z;                                                                                     \
        acc_cx += (double)(a_).cx + k_cx * (double)(a_).cz;                                                          \
        acc_cy += (double)(a_).cy + k_cy * (double)(a_).cz

// TL_WALK_STORE_PARTIALS: block reduction of the walk-backs (fixed order).  The entrance sums go through `red`; of the
// quad-transposed rows sacc_dyn[ROWS_][kBlock] (lane q of a quad holds term q: g_c, g_t, g_mu) wave wv reduces rows wv,
// wv+4, ...: lane, lane+64, ... hold the same term (64 = 0 mod 4), the butterfly over lane bits 2..5 leaves each lane
// with the total of its own term.  Declares `row`, this block's row of partials, and `nrows_`: partials are stored
// [column][block] (the reduction kernels then read each column as one contiguous run).  Reads `lane`, `wv`, `tid`.
#define TL_WALK_STORE_PARTIALS(ROWS_)                                                                                \
    {                                                                                                                \
        const double a0 = wave_sum(acc_z), a1 = wave_sum(acc_cx), a2 = wave_sum(acc_cy);                             \
        if (lane == 0) { red[wv][0] = a0; red[wv][1] = a1; red[wv][2] = a2; }                                        \
    }                                                                                                                \
    __syncthreads();                                                                                                 \
    const size_t nrows_ = (size_t)gridDim.y * gridDim.x;                                                             \
    double *row = part + ((size_t)fw * gridDim.x + blockIdx.x);                                                      \
    for (int k = wv; k < (ROWS_); k += kWaves) {                                                                     \
        const float *q = sacc_dyn + (size_t)k * kBlock;                                                              \
        double v = (double)q[lane] + (double)q[lane + 64];                                                           \
        v += (double)q[lane + 128];                                                                                  \
        v += (double)q[lane + 192];                                                                                  \
        _Pragma("unroll") for (int o = 32; o >= 4; o >>= 1) v += __shfl_xor(v, o, 64);                               \
        if (lane < 3) row[(size_t)(lane * (ROWS_) + k) * nrows_] = v;                                                \
    }                                                                                                                \
    if (tid < 3) row[(size_t)(3 * (ROWS_) + tid) * nrows_] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid]

// ------------------------------------------------------------------ checkpoint-free backward
// Alternative to trace_bwd_kernel for lenses with allow_backward_rays (no penalty term):
// instead of re-tracing the ray forwards and keeping the state entering every surface in registers,
// start from the forward kernel's per-ray OUTPUT (x, y, cx, cy, ok at the image plane) and walk the ray
// backwards: at surface k undo the refraction (Snell with 1/mu at the same normal), then intersect the
// incoming line with surface k-1 in closed form to get the state that entered surface k, and apply the
// same adjoint step (step_bwd).  Geometric optics is reversible, so the reconstructed states equal the
// forward ones up to rounding (~1e-7 relative per surface), which only perturbs the GRADIENT at that
// level; the seed uses the forward's own y.  No per-surface checkpoints -> ~70 VGPRs (6-7 waves per SIMD,
// SGPR-limited, instead of 4), no correctly rounded re-derivation in strict mode, one rolled loop for any S.
// LDS: S*kBlock floats of dynamic shared memory (quad-transposed accumulators, see below).
// ASPH: the lens has aspheric rows.  There the normal comes from the sag derivative, the refraction is undone
// with the vector form of Snell's law, the previous hit is found by Newton (hit_asph) when row k-1 is aspheric,
// and the adjoint is step_bwd_asph (which only needs the entering state and the z leaving the row).
// part: [nblocks][3S+3] doubles, or [nblocks][8S+3] with ASPH (g_kappa[S] | g_poly[S][4] appended).
#ifndef TL_ASPH_INV_WAVES
#define TL_ASPH_INV_WAVES 5      // waves per SIMD the aspheric walk-back is register-allocated for: 96 VGPRs + 68 B of scratch beat the
                                 // compiler's own 113 VGPRs / 4 waves by 6 % (cfg3a, both modes); 6 waves (80 VGPRs) lose it again
#endif
template <bool ASPH>
__global__ __launch_bounds__(kBlock, ASPH ? TL_ASPH_INV_WAVES : 1) void trace_bwd_inv_kernel(
    const tl_problem pa, const float *__restrict__ gx, const float *__restrict__ gy,
    const float *__restrict__ gcx, const float *__restrict__ gcy, const double *__restrict__ gmom,
    const float *__restrict__ fx, const float *__restrict__ fy, const float *__restrict__ fcx,
    const float *__restrict__ fcy, const uint8_t *__restrict__ fok, const double *__restrict__ fmom,
    float *__restrict__ gxin, float *__restrict__ gyin, double *__restrict__ part, const int /*unused, see below*/,
    unsigned *__restrict__ poison, const unsigned token)
{
#pragma clang fp contract(fast)       // see TL_REVERSE_CONTRACT above
    // (The unused int -- once a plan hint, launched as 0 -- keeps this kernel's argument layout: without it the register-
    //  bound <true> instantiation is allocated differently and loses 3 (strict) / 6 (fast) instructions, unmeasured.  The
    //  other trace kernels dropped theirs with the same opcodes in the same order; profiles/kernels_shared_stages.txt.)
    // the forward saw an ill-conditioned live ray: the checkpoint kernel (launched next to this one) does
    // the whole batch bit-faithfully instead, and this launch retires at once
    // -- unless it also left per-ray flags (pa.cond_flags; `fok` is then that array: 0 dead, 1 live, 2 live and
    // ill-conditioned): the flagged rays alone go to the checkpoint kernel and this launch walks back the bytes == 1.
    if (fmom && !pa.cond_flags && ill_conditioned(fmom, pa.F * tl_lenses(pa))) return;
    // accumulators of g_c, g_t, g_mu: [S][kBlock] floats, ONE slot per lane and surface row.  The four
    // lanes of a quad add their three terms with DPP (no LDS traffic, quad_term_sums) and lane q of the quad
    // keeps term q (0: g_c, 1: g_t, 2: g_mu, 3: idle), so a row costs one conflict-free read-add-write instead of three and
    // 1 KB of LDS instead of 3 KB: S=11 runs at 7 waves per SIMD instead of 4, S=20 at 7 instead of 2.
    extern __shared__ float sacc_dyn[];
    const bool q_odd = (threadIdx.x & 1) != 0, q_hi = (threadIdx.x & 2) != 0;
    __shared__ double red[kWaves][3];
    __shared__ float sasph[ASPH ? 5 * TL_MAX_SURFACES : 1][kWaves];   // per-wave sums of the aspheric-coefficient gradients
    const int tid = threadIdx.x;
    TL_LENS_ROW(pa);
    TL_BLOCK_CHUNKS(p.P);
    const int S = p.S;
    const unsigned kbits = ASPH ? row_bits(p.surf_kind, S) : 0u;
    if (ASPH && (tid & 63) == 0)
        for (int j = 0; j < 5 * S; ++j) sasph[j][tid >> 6] = 0.0f;    // touched by lane 0 of this wave only
    const float z0 = p.z[0];
    const float cx0 = p.cx[f * p.cx_stride], cy0 = p.cy[f * p.cy_stride];
    const float cz0 = tl_sqrt_any((1.0f - cx0 * cx0) - cy0 * cy0);
    const float *__restrict__ mu_w = p.mu + (size_t)w * S;
    const int64_t xoff = f * p.xs_f + w * p.xs_w, yoff = f * p.ys_f + w * p.ys_w;
    double gm0 = 0, gm1 = 0, gm2 = 0, gm4 = 0, gm5 = 0, gm6 = 0;
    if (gmom) {
        const double *q = gmom + (size_t)gf * TL_NMOM;
        gm0 = q[0]; gm1 = q[1]; gm2 = q[2]; gm4 = q[4]; gm5 = q[5]; gm6 = q[6];
    }
    for (int j = 0; j < S; ++j) sacc_dyn[j * kBlock + tid] = 0.0f;         // own slots only: no barrier needed
    TL_WALK_ENTRANCE_SUMS(cx0, cy0);
    // 1/mu[k] is wave-uniform: computed once per block into LDS instead of once per ray and surface
    __shared__ float s_inv_mu[TL_MAX_SURFACES];
    if (tid < S) s_inv_mu[tid] = 1.0f / uload(mu_w, tid);
    __syncthreads();

    // software pipeline: the forward outputs of ray r+1 are requested before ray r is walked back.  (Not with aspheric
    // rows: that variant is register-bound -- five VGPRs of prefetched state are five more dwords of scratch -- and
    // its Newton rows leave the other waves time to cover the load.)
    const int64_t ipf = c0 * kBlock + tid;
    const int64_t of = (int64_t)fw * p.P + ipf;
    bool a_nxt = !ASPH && (ipf < p.P) && fok[ipf < p.P ? of : 0] == 1;
    float x_nxt = a_nxt ? fx[of] : 0.0f, y_nxt = a_nxt ? fy[of] : 0.0f;
    float cx_nxt = a_nxt ? fcx[of] : 0.0f, cy_nxt = a_nxt ? fcy[of] : 0.0f;
    for (int r = 0; r < R; ++r) {
        const int64_t ip = (c0 + r) * kBlock + tid;
        const bool valid = ip < p.P;
        const int64_t o = (int64_t)fw * p.P + ip;
        bool alive = a_nxt;
        float xi = x_nxt, yi = y_nxt;
        // direction leaving the last surface (dead lanes: a harmless axial ray)
        float dx = cx_nxt, dy = cy_nxt;
        if (ASPH) {
            alive = valid && fok[valid ? o : 0] == 1;
            xi = yi = dx = dy = 0.0f;
            if (valid) { xi = fx[o]; yi = fy[o]; dx = fcx[o]; dy = fcy[o]; }
            xi = alive ? xi : 0.0f; yi = alive ? yi : 0.0f; dx = alive ? dx : 0.0f; dy = alive ? dy : 0.0f;
        } else {
            const int64_t ipn = ip + kBlock, on = o + kBlock;
            const bool more = (r + 1 < R) && (ipn < p.P);
            a_nxt = more && fok[more ? on : 0] == 1;
            x_nxt = a_nxt ? fx[on] : 0.0f; y_nxt = a_nxt ? fy[on] : 0.0f;
            cx_nxt = a_nxt ? fcx[on] : 0.0f; cy_nxt = a_nxt ? fcy[on] : 0.0f;
        }
        if (__ballot(alive) == 0ull) {
            if (valid) { if (gxin) gxin[o] = 0.0f; if (gyin) gyin[o] = 0.0f; }
            continue;
        }
        float dz = tl_sqrt_hw(1.0f - (dx * dx + dy * dy));
        // ---- seeds (same as trace_bwd_kernel; the forward's own x, y)
        float sx = (gx && alive) ? gx[o] : 0.0f;
        float sy = (gy && alive) ? gy[o] : 0.0f;
        const float scx = (gcx && alive) ? gcx[o] : 0.0f;
        const float scy = (gcy && alive) ? gcy[o] : 0.0f;
        if (gmom) {                                                    // ok = 1 for every lane that matters;
            sy += alive ? (float)(gm0 + (gm1 + 2.0 * (double)yi * gm2)) : 0.0f;   // dead lanes walk an axial ray
            sx += alive ? (float)(gm4 + (gm5 + 2.0 * (double)xi * gm6)) : 0.0f;   // with zero seeds: exact zeros
        }
        // ---- walk back from the image plane (TL_HIT: the closed-form hit on a spherical row)
        Adj a;
        float hx, hy, hz, cos_t, r_t;                 // hit on surface k (frame k), refraction-side cosine there
        {
            const float tl = uload(p.t, S - 1);
            const float qx = alive ? xi : 0.0f, qy = alive ? yi : 0.0f;
            float db;
            if (ASPH && ((kbits >> (S - 1)) & 1u)) {
                hit_asph(load_asph(p, S - 1), qx, qy, tl, dx, dy, dz, alive, hx, hy, hz, db);
                cos_t = r_t = 1.0f;                                // recomputed from the aspheric normal below
            } else {
                TL_HIT(TL_HIT_PLAIN, uload(p.c, S - 1), qx, qy, tl, dx, dy, dz, hx, hy, hz, cos_t, r_t, db);
            }
            // image-plane adjoint: x_img = x_S + dist*cx', dist = -z_S/cz' = -db
            const float dist = -db, inv_cz = tl_rcp(dz);
            const float b_dist = sx * dx + sy * dy;
            a.x = sx; a.y = sy;
            a.cx = scx + sx * dist;
            a.cy = scy + sy * dist;
            a.z = -b_dist * inv_cz;
            a.cz = -b_dist * dist * inv_cz;
        }
        for (int k = S - 1; k >= 0; --k) {
            const float c = uload(p.c, k), mu = uload(mu_w, k);
            const bool asph_k = ASPH && ((kbits >> k) & 1u);        // wave-uniform
            const float inv_mu = s_inv_mu[k];
            const float zout = hz - uload(p.t, k);                         // z leaving row k (what step_bwd_asph wants)
            StepVals v;
            float ix, iy, iz;
            if (asph_k) {
                // ---- aspheric normal at the hit, refraction undone with the vector form of Snell's law
                const Asph A = load_asph(p, k);
                const float rho = hx * hx + hy * hy;
                const float rq = tl_rsq(1.0f - (((1.0f + A.kappa) * A.c) * A.c) * rho);
                const float dsag = 0.5f * A.c * rq + rho * (2.0f * A.a0 + rho * (3.0f * A.a1 + rho * (4.0f * A.a2 + rho * (5.0f * A.a3))));
                const float m = 2.0f * dsag;
                const float nz = tl_rsq(1.0f + (m * m) * rho);
                const float nx = -(m * hx) * nz, ny = -(m * hy) * nz;
                const float ct = (dx * nx + dy * ny) + dz * nz;     // refraction-side cosine
                const float ci2 = 1.0f - (inv_mu * inv_mu) * (1.0f - ct * ct);
                const float g = ct - mu * (ci2 * tl_rsq(ci2));      // cx3 = mu cx + g nx
                ix = (dx - g * nx) * inv_mu; iy = (dy - g * ny) * inv_mu; iz = (dz - g * nz) * inv_mu;
            } else {
                v.x1 = hx; v.y1 = hy;
                v.cos_t = cos_t; v.r_t = r_t;
                v.cx3 = dx; v.cy3 = dy; v.r_z = tl_rcp_adj(dz);   // the direction leaving surface k
                // ---- undo the refraction at the hit point: n = (-c X, -c Y, 1 - c Z), d_in = (d_out - g n) / mu
                v.s2 = (inv_mu * inv_mu) * (1.0f - cos_t * cos_t); // sin^2 of incidence (Snell)
                v.cos2 = 1.0f - v.s2;
                tl_rsq_sqrt(v.cos2, v.r_i, v.cos_i);
                v.g = cos_t - mu * v.cos_i;                        // the forward's g
                v.gc = v.g * c;
                ix = (dx + v.gc * hx) * inv_mu; iy = (dy + v.gc * hy) * inv_mu; iz = ((dz - v.g) + v.gc * hz) * inv_mu;
            }
            // ---- state that entered surface k (frame k), and the hit on surface k-1 for the next round
            Ray in;
            if (k == 0) {                                          // exactly the launch conditions
                in.x = valid ? p.x_in[xoff + ip * p.xs_p] : 0.0f;
                in.y = valid ? p.y_in[yoff + ip * p.ys_p] : 0.0f;
                in.z = z0; in.cx = cx0; in.cy = cy0; in.cz = cz0;
                v.d = (hz - z0) * tl_rcp(cz0);                     // z1 = z + d cz
            } else if (!ASPH) {
                // all-spherical lens: the forward step's e, m2, tmp, q and the back-intersection with surface k-1
                // share one dot product and one |h|^2 (see trace_bwd_inv_unrolled_kernel)
                const float tp = uload(p.t, k - 1), cp = uload(p.c, k - 1);
                const float ehi = -((hx * ix + hy * iy) + hz * iz);
                const float hh = (hx * hx + hy * hy) + hz * hz;
                const float hzs = hz + tp;
                const float e_ = ehi - tp * iz;
                const float m2_ = (hh + tp * (hz + hzs)) - e_ * e_;
                const float mz_ = hzs + e_ * iz;
                const float tmp_ = cp * m2_ - 2.0f * mz_;
                const float cos2_ = iz * iz - cp * tmp_;
                tl_rsq_sqrt(cos2_, r_t, cos_t);
                const float db = e_ + tmp_ * tl_rcp(iz + cos_t);
                const float px = hx + db * ix, py = hy + db * iy, pz = hzs + db * iz;
                v.d = -db;
                v.e = ehi - db;
                v.q = -ehi;
                v.m2 = hh - ehi * ehi;
                v.tmp = c * v.m2 - 2.0f * (hz + ehi * iz);
                in.x = px; in.y = py; in.z = pz - tp;
                in.cx = ix; in.cy = iy; in.cz = iz;
                hx = px; hy = py; hz = pz;                         // hit on surface k-1, frame k-1
            } else {
                const float tp = uload(p.t, k - 1);
                float px, py, pz, db;
                const float hzs = hz + tp;
                if (ASPH && ((kbits >> (k - 1)) & 1u)) {
                    hit_asph(load_asph(p, k - 1), hx, hy, hzs, ix, iy, iz, alive, px, py, pz, db);
                } else {
                    TL_HIT(TL_HIT_PLAIN, uload(p.c, k - 1), hx, hy, hzs, ix, iy, iz, px, py, pz, cos_t, r_t, db);
                }
                in.x = px; in.y = py; in.z = pz - tp;
                in.cx = ix; in.cy = iy; in.cz = iz;
                hx = px; hy = py; hz = pz;                         // hit on surface k-1, frame k-1
                v.d = -db;
            }
            // ---- adjoint of the forward step k at that state
            float g_c, g_t, g_mu;
            if (asph_k) {
                float ga[5];
                step_bwd_asph(in, zout, load_asph(p, k), uload(p.t, k), mu, a, g_c, g_t, g_mu, ga);
                // wave sums of the five coefficient terms (dead lanes: exact zeros).  Two transposed quad sums
                // leave term j on lane j of every quad (ga0..2 in u, ga3..4 in w), then four butterfly steps over
                // the quads: 8 cross-lane moves + 6 DPP adds instead of 30 moves for five plain wave sums.
                float u = quad_term_sums(ga[0], ga[1], ga[2], q_odd, q_hi);
                float w2 = quad_term_sums(ga[3], ga[4], 0.0f, q_odd, q_hi);
#pragma unroll
                for (int o = 32; o >= 4; o >>= 1) {
                    u += __shfl_xor(u, o, 64);
                    w2 += __shfl_xor(w2, o, 64);
                }
                const int ln = tid & 63;
                if (ln < 3) sasph[5 * k + ln][tid >> 6] += u;
                if (ln < 2) sasph[5 * k + 3 + ln][tid >> 6] += w2;
            } else {
                // the few intersection quantities the adjoint needs besides what the walk already knows
                if (ASPH || k == 0) {
                    v.e = -((in.x * in.cx + in.y * in.cy) + in.z * in.cz);
                    const float mz = in.z + v.e * in.cz;
                    v.m2 = ((in.x * in.x + in.y * in.y) + in.z * in.z) - v.e * v.e;
                    v.tmp = c * v.m2 - 2.0f * mz;
                    v.q = v.d - v.e;
                }
                v.inv_den = tl_rcp_adj(in.cz + v.cos_i);
                step_adjoint<false>(in, c, mu, v, a, g_c, g_t, g_mu);
            }
            // no per-lane mask: a dead lane's terms are exact zeros (zero seeds), and a non-finite term shows
            // up in the entrance adjoint below, where it sends the whole launch to the checkpoint kernel
            sacc_dyn[k * kBlock + tid] += quad_term_sums(g_c, g_t, g_mu, q_odd, q_hi);
            dx = ix; dy = iy; dz = iz;                             // the ray between surfaces k-1 and k
        }
        TL_WALK_ENTRANCE_ADD(a);
        if (valid) {
            if (gxin) gxin[o] = a.x;
            if (gyin) gyin[o] = a.y;
        }
    }
    // ---- block reduction (fixed order)
    const int lane = tid & 63, wv = tid >> 6;
    TL_WALK_STORE_PARTIALS(S);
    if (ASPH) {
        // g_kappa[k] -> column 3S+3+k ; g_poly[k][j] -> column 4S+3+4k+j   (sasph row 5k+{0,1..4})
        for (int j = tid; j < 5 * S; j += kBlock) {
            const int k = j / 5, jj = j - 5 * k;
            const double v = (((double)sasph[j][0] + (double)sasph[j][1]) + (double)sasph[j][2]) + (double)sasph[j][3];
            row[(size_t)(jj == 0 ? 3 * S + 3 + k : 4 * S + 3 + 4 * k + (jj - 1)) * nrows_] = v;
        }
    }
}

// ------------------------------------------------------------------ walk-back, surface loop unrolled
// Same algorithm and same outputs as trace_bwd_inv_kernel<false> for an all-spherical lens of EXACTLY NS rows, with
// the row loop instantiated row by row, so that what the rolled loop has to keep in LDS, re-select and rotate every
// row can stay where it is:
//  * the g_c sum of every row lives in a VGPR of the lane across its rays, the g_t and g_mu sums in two private LDS
//    slots per row and lane at compile-time offsets ([2 NS][kBlock] floats of dynamic LDS; plain ds_read / v_add /
//    ds_write, no conflicts).  The rolled loop cannot index registers by a run-time k: there every row pays three
//    DPP adds and four selects (quad_term_sums; a DPP operand costs ~2.5 plain issues, tools/valu_probe.hip) plus
//    the ~13 register copies that rotate the carried state.  The sums meet the quad-transposed layout once per
//    block, in the epilogue;
//  * the row parameters {c, t, mu, 1/mu} come from an LDS copy of the prescription, one ds_read_b128 per row,
//    requested one row ahead.  As VGPR operands they also avoid the SGPR-source issue penalty of back-to-back VALU
//    instructions (tools/valu_probe2.hip);
//  * no prefetch of the next ray's forward outputs (five registers): at 6 waves per SIMD the other waves cover
//    the load latency, and 80 VGPRs is what 6 waves allow.
// Measured (profiles/r02_ab_walkback_variants.txt): -8 % (strict) / -12 % (fast) on the 11-row double Gauss, -5 % on the
// 7-row Cooke triplet; from ~13 rows up the 2 NS KB of LDS per block cost more waves than the unrolling wins
// (20 rows: equal; hence the pair-shared slots from 13 rows on, below); launch_bwd_inv uses it for
// kInvUnrollMin <= S <= kInvUnrollMax and the rolled kernel otherwise.
// Four compiler habits the code below works around, each measured on this kernel:
//  * a `#pragma unroll` loop promotes the per-row arrays to <NS x float> VECTORS before it unrolls, and vector-typed
//    registers with their tuple copies cost 8-20 VGPRs per row: hence static_for_down with a std::integral_constant;
//  * whatever depends on the row alone (mu^2, 2c ...; uniform, but computed by the VALU, so a VGPR each) is hoisted
//    out of the ray loop, +5 VGPRs per row: hence the LDS index laundered through an empty asm that "reads" the
//    carried state (NOT volatile: that would be a memory clobber and turn the scalar loads into vector loads);
//  * (ASPH) whatever is affine in the ray index or invariant in the ray loop gets a register of its own across the loop:
//    a running pointer per array and plane, a lane mask per row-kind test, base + lane per array in a VGPR pair; on an
//    aspheric lens that was 116 SGPRs spilled to VGPR lanes and read back per ray and row: hence the chunk offset, the
//    row bits and the lane's byte offset laundered once per ray (at the top of the ray loop);
//  * g_c, g_t, g_mu feed nothing but the sums, so they are sunk to the END of the ray together with the ~20
//    intermediates each row needs for them (scratch spills from NS = 3 on; __builtin_amdgcn_sched_barrier is no
//    help, the order is lost before the machine scheduler): hence the empty volatile asm at the end of a row that
//    consumes the sum and the carried state, which keeps its place in the instruction stream like a store would.
// Rows 13..20 (kInvUnrollPairMin..kInvUnrollMax): the two lanes of a pair share one slot per row and term (one DPP
// add each before the read-add-write, both lanes storing the same sum), 1 KB of LDS per row instead of 2, and the
// kernel is allocated for 5 waves (96 VGPRs: 20 g_c sums fit) -- 20 KB x 5 blocks per CU.
constexpr int kInvUnrollMin = TL_INVU_MIN, kInvUnrollPairMin = 13, kInvUnrollMax = TL_INVU_MAX;
#ifndef TL_INVU_ASPH_WAVES
#define TL_INVU_ASPH_WAVES 4     // waves per SIMD the variants with aspheric rows are register-allocated for (128 VGPRs: no scratch up to 12 rows)
#endif
#ifndef TL_INVU_PEN_WAVES
#define TL_INVU_PEN_WAVES 5      // ... and the all-spherical variant that carries the penalty seed
#endif
constexpr int inv_unroll_waves(int ns, bool asph, bool pen)
{
    return asph ? TL_INVU_ASPH_WAVES : pen ? TL_INVU_PEN_WAVES : (ns < kInvUnrollPairMin ? 6 : 5);
}

template <class T> struct row_index { static constexpr int value = 0; };
template <int K> struct row_index<std::integral_constant<int, K>> { static constexpr int value = K; };
// f(N-1), f(N-2), ... f(0) with the index as a std::integral_constant
template <int N, class F>
__device__ __forceinline__ void static_for_down(F &f)
{
    if constexpr (N > 0) {
        f(std::integral_constant<int, N - 1>{});
        static_for_down<N - 1>(f);
    }
}

// z = sag(rho) of an aspheric row at a STORED hit point (tl_problem.asph_hits), with 1/q and q = sqrt(1 - (1+kappa) c^2 rho)
// for the normal the row takes next.  Reverse-sweep arithmetic (v_rsq / v_rcp + one Newton step, contraction).
__device__ __forceinline__ float sag_at(const Asph &A, const float rho, float &rq_out, float &q_out)
{
#pragma clang fp contract(fast)
    const float q2 = 1.0f - (((1.0f + A.kappa) * A.c) * A.c) * rho;
    const float rq = tl_rsq(q2);
    const float q = q2 * rq;
    rq_out = rq; q_out = q;
    return (A.c * rho) * tl_rcp(1.0f + q) + (rho * rho) * (A.a0 + rho * (A.a1 + rho * (A.a2 + rho * A.a3)));
}

// ASPH: the lens has aspheric rows AND the forward left their hit points in tl_problem.asph_hits.  Every row is then
//   a wave-uniform choice between the spherical code above and an aspheric one: normal from the sag derivative at the
//   hit, refraction undone with the vector form of Snell's law, adjoint = asph_adjoint fed with what the walk already
//   has (no second evaluation of the normal, no recovery of s from z).  The hit on an aspheric row k-1 is READ, not
//   searched: the forward stored (X, Y) there, z = sag(X, Y), and the distance along the incoming line is a dot
//   product -- no Newton iteration on the reversed ray, however strong the asphere (trace_bwd_inv_kernel<true> spends
//   >= 2 iterations + a vote per aspheric row), and the reconstruction is re-anchored on exact forward values at every
//   aspheric row.  The five coefficient terms of an aspheric row are quad-transposed (two quad_term_sums) into two
//   private LDS slots per lane and slot row: no wave-wide butterfly per ray.  A lens with more aspheric rows than
//   hit slots flags the poison word and leaves the launch to the checkpoint kernel.
// PEN: the penalty seed gq (upstream gradient of moment 8) enters every row's adjoint (step_adjoint<true, WALK>,
//   asph_adjoint<true>) for rays that are ALIVE at the image plane; rays that died on the way keep the gradient of
//   the rows they passed alive, which only a forward re-trace can give: the checkpoint kernel queued behind this one
//   runs over exactly those rays (selective pass, whole waves skipped where every ray lived) and the reduction adds
//   the two partial arrays.
// PEN (PenMode, see trace_bwd_kernel) == kPenRay: the live rays add their per-ray stack seeds (gstk, see trace_bwd_kernel)
//   to gq, row by row: three loads per row, issued at the top of the row so that the walk of the row hides them.  Dead lanes
//   take zero seeds; rays that died on the way reach the checkpoint pass through the scan map, as above.
template <int NS, bool ASPH, int PEN>
__global__ __launch_bounds__(kBlock, inv_unroll_waves(NS, ASPH, PEN != kPenNone)) void trace_bwd_inv_unrolled_kernel(
    const tl_problem pa, const float *__restrict__ gx, const float *__restrict__ gy,
    const float *__restrict__ gcx, const float *__restrict__ gcy, const double *__restrict__ gmom,
    const float *__restrict__ fx, const float *__restrict__ fy, const float *__restrict__ fcx,
    const float *__restrict__ fcy, const uint8_t *__restrict__ fok, const double *__restrict__ fmom,
    float *__restrict__ gxin, float *__restrict__ gyin, double *__restrict__ part,
    unsigned *__restrict__ poison, const unsigned token, const float *__restrict__ gstk)
{
#pragma clang fp contract(fast)       // see TL_REVERSE_CONTRACT above
    constexpr bool PENB = PEN != kPenNone, STK = PEN == kPenRay;
    // no per-ray flags in `fok` (see trace_bwd_inv_kernel): the checkpoint kernel does this batch
    if (fmom && !pa.cond_flags && ill_conditioned(fmom, pa.F * tl_lenses(pa))) return;
    extern __shared__ float sacc_dyn[];                         // [2 NS][SLOTS]: g_t rows, then g_mu rows [; ASPH: [2 slots][kBlock]]
    constexpr bool PAIR = NS >= kInvUnrollPairMin;              // lanes 2j, 2j+1 share slot j
    constexpr int SLOTS = PAIR ? kBlock / 2 : kBlock;
    const int slot = PAIR ? (int)(threadIdx.x >> 1) : (int)threadIdx.x;
    float *const sasph_dyn = sacc_dyn + 2 * NS * SLOTS;         // ASPH: coefficient terms, [2 hit_slots][kBlock]
    __shared__ double red[kWaves][3];
    __shared__ float4 s_row[NS];                                // {c, t, mu, 1/mu} of this (f, w)
    __shared__ float4 s_poly[ASPH ? NS : 1];                    // a4, a6, a8, a10
    __shared__ float s_kappa[ASPH ? NS : 1];
    const bool q_odd = (threadIdx.x & 1) != 0, q_hi = (threadIdx.x & 2) != 0;
    const int tid = threadIdx.x;
    TL_LENS_ROW(pa);
    TL_BLOCK_CHUNKS(p.P);
    const unsigned kbits_all = ASPH ? row_bits(p.surf_kind, NS) : 0u;
    const int hit_slots = ASPH ? p.asph_hit_slots : 0;
    const float *__restrict__ hits = ASPH ? p.asph_hits : nullptr;
    const size_t n_rays_all = (size_t)gridDim.y * p.P;
    if (ASPH && (hits == nullptr || __popc(kbits_all) > hit_slots)) {      // (block-uniform) not enough hit slots for this lens
        if (tid == 0) *poison = token;
        return;
    }
    const float z0 = p.z[0];
    const float cx0 = p.cx[f * p.cx_stride], cy0 = p.cy[f * p.cy_stride];
    const float cz0 = tl_sqrt_any((1.0f - cx0 * cx0) - cy0 * cy0);
    const float *__restrict__ mu_w = p.mu + (size_t)w * NS;
    const int64_t xoff = f * p.xs_f + w * p.xs_w, yoff = f * p.ys_f + w * p.ys_w;
    // the six fp64 seed factors of this field.  ASPH: re-read per ray through the scalar cache instead (uload64 below):
    // held across the row code they are 12 SGPRs which the aspheric rows need
    const double *const gm_f = gmom ? gmom + (size_t)gf * TL_NMOM : nullptr;
    double gm0 = 0, gm1 = 0, gm2 = 0, gm4 = 0, gm5 = 0, gm6 = 0;
    if (!ASPH && gmom) { gm0 = gm_f[0]; gm1 = gm_f[1]; gm2 = gm_f[2]; gm4 = gm_f[4]; gm5 = gm_f[5]; gm6 = gm_f[6]; }
    const float gq = (PEN && gmom) ? (float)gmom[(size_t)gf * TL_NMOM + 8] : 0.0f;
    // which of the optional per-ray seed arrays are there (none on the moment-seeded path), as bits of one scalar
    const unsigned seed_bits = !ASPH ? 0u : (unsigned)__builtin_amdgcn_readfirstlane(
        (int)((gx ? 1u : 0u) | (gy ? 2u : 0u) | (gcx ? 4u : 0u) | (gcy ? 8u : 0u)));
    float r_c[NS];                                              // the g_c sums of this lane
#pragma unroll
    for (int j = 0; j < NS; ++j) r_c[j] = 0.0f;
    for (int j = 0; j < 2 * NS; ++j) sacc_dyn[j * SLOTS + slot] = 0.0f;   // own slots only: no barrier needed
    if (ASPH)
        for (int j = 0; j < 2 * hit_slots; ++j) sasph_dyn[j * kBlock + tid] = 0.0f;
    TL_WALK_ENTRANCE_SUMS(cx0, cy0);
    if (tid < NS) {
        s_row[tid] = make_float4(uload(p.c, tid), uload(p.t, tid), uload(mu_w, tid), 1.0f / uload(mu_w, tid));
        if (ASPH) {
            s_kappa[tid] = p.kappa[tid];
            s_poly[tid] = make_float4(p.poly[4 * tid], p.poly[4 * tid + 1], p.poly[4 * tid + 2], p.poly[4 * tid + 3]);
        }
    }
    __syncthreads();
    // PEN: this wave's column of the scan map (see tl_scanmap), from the first chunk of this block on
    // (the wave index through readfirstlane: the pointer is wave-uniform and stays in SGPRs)
    uint8_t *__restrict__ scanmap = PEN ? tl_scanmap(poison, (int)gridDim.y, nchunk_) + ((size_t)fw * nchunk_ + c0) * kWaves
                                              + __builtin_amdgcn_readfirstlane(tid >> 6) : nullptr;

    for (int r = 0; r < R; ++r) {
        // Addresses: a wave-uniform base per ray chunk (SGPRs) + the lane's 32-bit index, the `saddr` form of the
        // global loads -- no 64-bit per-lane pointers carried through the row code (8 VGPRs).  The forward's outputs
        // are read under `valid` alone, not under the ok byte just loaded: one memory latency per ray, not two.
        const int64_t chunk = (c0 + r) * kBlock;                                   // first ray of this chunk
        const int64_t left = p.P - chunk;
        const unsigned rem = left < (int64_t)kBlock ? (unsigned)left : (unsigned)kBlock;
        const unsigned ut = (unsigned)tid;
        const bool valid = ut < rem;
        // `ob`, the element offset of this chunk in every [B,F,W][P] array, is the ONE quantity that advances per ray: each
        // address below is formed from it where it is used (base + ob [+ a uniform plane offset], scalar adds).  The empty
        // asm hides how it depends on r: otherwise loop strength reduction keeps a running 64-bit pointer per array and
        // plane, 32 of them on an aspheric lens, advanced in the latch and spilled to VGPR lanes.  The row bits, the plane
        // stride, the seed-factor pointer and the seed bits go through it too, so that what depends on them alone (the
        // per-row kind tests, k * stride, the factors) is evaluated where it is used, on the scalar unit, and not hoisted
        // out of the ray loop into SGPRs held across it (a wave-uniform bool held there is a lane mask: two SGPRs each).
        // (NOT volatile: see the header.)  The all-spherical variants keep their code to the instruction.
        int64_t ob = (int64_t)fw * p.P + chunk;
        unsigned kbits = kbits_all;
        const double *gm = gm_f;
        size_t nra = n_rays_all;
        unsigned sbits = seed_bits;
        if (ASPH) asm("" : "+s"(ob), "+s"(kbits), "+s"(gm), "+s"(nra), "+s"(sbits));
        // this lane's element of a [P] row at a wave-uniform address.  ASPH: the lane part as a 32-bit BYTE offset, which
        // selects the `saddr` form of the load (uniform base in SGPRs + one VGPR); indexed by element, the lane part is
        // widened first and every load forms a 64-bit address in a VGPR pair
        unsigned ut4 = ut * 4u;
        if (ASPH) asm("" : "+v"(ut4) : "s"(r));       // (or base + lane is kept per array across the ray loop, a VGPR pair each)
        auto LD = [&](const float *q) { return ASPH ? *(const float *)((const char *)q + ut4) : q[ut]; };
        bool alive = false;
        float xi = 0.0f, yi = 0.0f, dx = 0.0f, dy = 0.0f;       // position at the image plane, direction leaving row S-1
        float sx = 0.0f, sy = 0.0f, scx = 0.0f, scy = 0.0f;     // seeds (same as trace_bwd_kernel; the forward's own x, y)
        if (valid) {
            alive = ((fok + ob)[ut] & 1) != 0;                          // (2: ill-conditioned, the checkpoint pass takes it.  `& 1`,
                                                                        //  not `== 1`: that form costs 2 VGPRs and 32 B of scratch at NS = 11)
            xi = LD(fx + ob); yi = LD(fy + ob); dx = LD(fcx + ob); dy = LD(fcy + ob);
            if (ASPH ? (sbits & 1u) != 0 : gx != nullptr) sx = LD(gx + ob);
            if (ASPH ? (sbits & 2u) != 0 : gy != nullptr) sy = LD(gy + ob);
            if (ASPH ? (sbits & 4u) != 0 : gcx != nullptr) scx = LD(gcx + ob);
            if (ASPH ? (sbits & 8u) != 0 : gcy != nullptr) scy = LD(gcy + ob);
        }
        // dead lanes: a harmless axial ray with zero seeds; its terms are exact zeros.  No wave-level skip here: a
        // second path through the loop makes the allocator keep two copies of every register sum and shuffle them
        // with ~100 moves per ray
        xi = alive ? xi : 0.0f; yi = alive ? yi : 0.0f; dx = alive ? dx : 0.0f; dy = alive ? dy : 0.0f;
        sx = alive ? sx : 0.0f; sy = alive ? sy : 0.0f; scx = alive ? scx : 0.0f; scy = alive ? scy : 0.0f;
        if (PEN) {              // the scan map for the checkpoint pass behind this launch: does this wave leave it a ray of this chunk?
            const unsigned long long rest = __ballot(valid && !alive);
            if ((tid & 63) == 0) scanmap[(size_t)r * kWaves] = rest != 0ull ? 1 : 0;
        }
        const float gq_l = (PEN && alive) ? gq : 0.0f;          // PEN: rays that died on the way belong to the checkpoint pass
        float dz = tl_sqrt_hw(1.0f - (dx * dx + dy * dy));
        if (gmom) {
            if (ASPH) {
                gm0 = uload64(gm, 0); gm1 = uload64(gm, 1); gm2 = uload64(gm, 2);
                gm4 = uload64(gm, 4); gm5 = uload64(gm, 5); gm6 = uload64(gm, 6);
            }
            sy += alive ? (float)(gm0 + (gm1 + 2.0 * (double)yi * gm2)) : 0.0f;
            sx += alive ? (float)(gm4 + (gm5 + 2.0 * (double)xi * gm6)) : 0.0f;
        }
        // the stored hit of this lane's ray on the aspheric row with `below_` aspheric rows before it
#define TL_LOAD_HIT(below_, PX, PY)                                                      \
        {                                                                                \
            const float *hp_ = hits + ((size_t)(2 * (below_)) * nra + (size_t)ob);       \
            PX = 0.0f; PY = 0.0f;                                                        \
            if (valid) { PX = LD(hp_); PY = LD(hp_ + nra); }                             \
            PX = alive ? PX : 0.0f; PY = alive ? PY : 0.0f;                              \
        }
        Adj a;
        float4 rk_next;                               // parameters of the row about to be walked
        float hx, hy, hz, cos_t, r_t;                 // hit on surface k (frame k); spherical row: refraction-side cosine
                                                      // there and its reciprocal; aspheric row: q and 1/q of the conic there
        float s2t = 0.0f;                             // PEN, spherical row: sin^2 on the refraction side = 1 - cos_t^2, formed
                                                      // as (dx^2 + dy^2) + c tmp: no cancellation towards normal incidence
        {
            int kl = NS - 1;
            asm("" : "+v"(kl) : "s"(r));              // pins the load inside the ray loop
            rk_next = s_row[kl];
            float db;
            if (ASPH && ((kbits >> (NS - 1)) & 1u)) {                 // wave-uniform
                float px, py;
                TL_LOAD_HIT(__popc(kbits) - 1, px, py);
                const float4 po = s_poly[ASPH ? NS - 1 : 0];
                const Asph A = {rk_next.x, s_kappa[ASPH ? NS - 1 : 0], po.x, po.y, po.z, po.w};
                const float pz = sag_at(A, px * px + py * py, r_t, cos_t);
                db = ((px - xi) * dx + (py - yi) * dy) + (pz - rk_next.y) * dz;
                hx = px; hy = py; hz = pz;
            } else {
                TL_HIT(TL_HIT_S2T, rk_next.x, xi, yi, rk_next.y, dx, dy, dz, hx, hy, hz, cos_t, r_t, db);
            }
            // image-plane adjoint: x_img = x_S + dist*cx', dist = -z_S/cz' = -db
            const float dist = -db, inv_cz = tl_rcp(dz);
            const float b_dist = sx * dx + sy * dy;
            a.x = sx; a.y = sy;
            a.cx = scx + sx * dist;
            a.cy = scy + sy * dist;
            a.z = -b_dist * inv_cz;
            a.cz = -b_dist * dist * inv_cz;
        }
        // One row.  GEN = false: the all-spherical code, one straight-line block per row.  GEN = true: row k or row k-1 may
        // be aspheric (wave-uniform branches).  An aspheric lens runs GEN only on the rows that need it: kept apart, the
        // spherical rows keep their single basic block -- with the branches in every row they ran 23 % slower
        // (profiles/r03_ab_asph_walkback.txt).
        auto row_impl = [&](auto kc, auto gen) {
            constexpr int k = row_index<decltype(kc)>::value;
            constexpr int kp = k > 0 ? k - 1 : 0;
            constexpr bool GEN = ASPH && decltype(gen)::value;
            const float c = rk_next.x, t_k = rk_next.y, mu = rk_next.z, inv_mu = rk_next.w;
            float c_p = 0.0f, t_p = 0.0f;
            if (k > 0) {                              // request row k-1 now: it is this row's "previous surface" too
                int kr = k - 1;
                asm("" : "+v"(kr) : "v"(hz));         // ... and not before row k+1 is done
                rk_next = s_row[kr];
                c_p = rk_next.x; t_p = rk_next.y;
            }
            const bool asph_k = GEN && ((kbits >> k) & 1u);                  // wave-uniform
            const bool asph_p = GEN && k > 0 && ((kbits >> kp) & 1u);
            // (GEN) the stored hit on row k-1: requested now, used once the refraction at row k is undone
            float px_s = 0.0f, py_s = 0.0f;
            if (GEN && k > 0) {
                if (asph_p) TL_LOAD_HIT(__popc(kbits & ((1u << kp) - 1u)), px_s, py_s);
            }
            const bool zpos = PEN && (hz - t_k) > 0.0f;                      // zRELU of this row is active
            PenSeed sk = pen_seed(gq_l);                                     // this row's seeds of zRELU, theta, theta'
            if (STK) {                                                       // (kPenRay) + the stacks' seeds of this ray
                const float *sq_ = gstk + ((size_t)k * nra + (size_t)ob);
                float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
                if (valid) { s0 = LD(sq_); s1 = LD(sq_ + (size_t)NS * nra); s2 = LD(sq_ + (size_t)(2 * NS) * nra); }
                sk.z += alive ? s0 : 0.0f; sk.th += alive ? s1 : 0.0f; sk.thp += alive ? s2 : 0.0f;
            }
            StepVals v;
            AsphVals av;
            Asph A;
            float ix, iy, iz;
            if (asph_k) {
                // ---- aspheric normal at the hit, refraction undone with the vector form of Snell's law
                const float4 po = s_poly[ASPH ? k : 0];
                A.c = c; A.kappa = s_kappa[ASPH ? k : 0]; A.a0 = po.x; A.a1 = po.y; A.a2 = po.z; A.a3 = po.w;
                av.X = hx; av.Y = hy;
                av.rho = hx * hx + hy * hy;
                av.rq = r_t; av.q = cos_t;                                   // from the hit computation (sag_at)
                av.dsag = 0.5f * c * av.rq + av.rho * (2.0f * A.a0 + av.rho * (3.0f * A.a1 + av.rho * (4.0f * A.a2 + av.rho * (5.0f * A.a3))));
                av.m = 2.0f * av.dsag;
                av.inv_n = tl_rsq(1.0f + (av.m * av.m) * av.rho);
                av.nx = -(av.m * hx) * av.inv_n; av.ny = -(av.m * hy) * av.inv_n;
                av.cos_t = (dx * av.nx + dy * av.ny) + dz * av.inv_n;        // refraction-side cosine
                av.r_t = tl_rcp_adj(av.cos_t);
                float s2t_a = 1.0f - av.cos_t * av.cos_t;
                if (PEN) {                                                   // |d x n|^2: see s2t
                    const float kx = dy * av.inv_n - dz * av.ny, ky = dz * av.nx - dx * av.inv_n, kz = dx * av.ny - dy * av.nx;
                    s2t_a = (kx * kx + ky * ky) + kz * kz;
                }
                av.s2 = (inv_mu * inv_mu) * s2t_a;
                const float ci2 = 1.0f - av.s2;
                float r_i;
                tl_rsq_sqrt(ci2, r_i, av.cos_i);
                av.g = av.cos_t - mu * av.cos_i;                             // cx3 = mu cx + g nx
                ix = (dx - av.g * av.nx) * inv_mu; iy = (dy - av.g * av.ny) * inv_mu; iz = (dz - av.g * av.inv_n) * inv_mu;
                av.cx3 = dx; av.cy3 = dy; av.r_z = tl_rcp_adj(dz);
            } else {
                v.x1 = hx; v.y1 = hy;
                v.cos_t = cos_t; v.r_t = r_t;
                v.cx3 = dx; v.cy3 = dy; v.r_z = tl_rcp_adj(dz);   // the direction leaving surface k
                // ---- undo the refraction at the hit point: the normal there is n = (-c X, -c Y, 1 - c Z), and
                //      d_in = (d_out - g n) / mu with the forward's g = cos_t - mu cos_i  (g n = (-gc X, -gc Y, g - gc Z))
                v.s2 = (inv_mu * inv_mu) * (PEN ? s2t : 1.0f - cos_t * cos_t);   // sin^2 of incidence (Snell)
                v.cos2 = 1.0f - v.s2;
                tl_rsq_sqrt(v.cos2, v.r_i, v.cos_i);
                v.g = cos_t - mu * v.cos_i;
                v.gc = v.g * c;
                ix = (dx + v.gc * hx) * inv_mu; iy = (dy + v.gc * hy) * inv_mu;
                iz = ((dz - v.g) + v.gc * hz) * inv_mu;
            }
            // ---- state that entered surface k (frame k), and the hit on surface k-1 for the next round
            Ray in;
            in.cx = ix; in.cy = iy; in.cz = iz;
            if (k == 0) {                                      // exactly the launch conditions
                in.x = valid ? (p.x_in + (xoff + chunk * p.xs_p))[(int64_t)ut * p.xs_p] : 0.0f;
                in.y = valid ? (p.y_in + (yoff + chunk * p.ys_p))[(int64_t)ut * p.ys_p] : 0.0f;
                in.z = z0; in.cx = cx0; in.cy = cy0; in.cz = cz0;
                const float d0 = (hz - z0) * tl_rcp(cz0);      // z1 = z + d cz
                if (asph_k) {
                    av.s = d0;
                } else {
                    v.d = d0;
                    // the few intersection quantities the adjoint needs besides what the walk already knows
                    v.e = -((in.x * in.cx + in.y * in.cy) + in.z * in.cz);
                    const float mz = in.z + v.e * in.cz;
                    v.m2 = ((in.x * in.x + in.y * in.y) + in.z * in.z) - v.e * v.e;
                    v.tmp = c * v.m2 - 2.0f * mz;
                    v.q = v.d - v.e;
                }
            } else {
                // The incoming line through the hit h (frame k) with direction i.  ehi = -(h . i) is the parameter of
                // its point nearest to vertex k: the forward step's e = ehi + d, m2 = |h|^2 - ehi^2, mz = h_z + ehi i_z
                // and q = d - e = -ehi come from it, and so do the same quantities about vertex k-1 (q = h + (0,0,t)),
                // which the closed-form intersection with surface k-1 needs -- one dot product and one |h|^2 for both.
                const float ehi = -((hx * ix + hy * iy) + hz * iz);
                const float hh = (hx * hx + hy * hy) + hz * hz;
                const float hzs = hz + t_p;
                float db, px, py, pz;
                if (asph_p) {
                    // row k-1 is aspheric: its hit was stored by the forward; z from the sag, distance along the line
                    const float4 po = s_poly[ASPH ? kp : 0];
                    const Asph Ap = {c_p, s_kappa[ASPH ? kp : 0], po.x, po.y, po.z, po.w};
                    px = px_s; py = py_s;
                    pz = sag_at(Ap, px * px + py * py, r_t, cos_t);
                    db = ((px - hx) * ix + (py - hy) * iy) + (pz - hzs) * iz;
                } else {
                    const float e_ = ehi - t_p * iz;
                    const float m2_ = (hh + t_p * (hz + hzs)) - e_ * e_;
                    const float mz_ = hzs + e_ * iz;
                    const float tmp_ = c_p * m2_ - 2.0f * mz_;
                    const float cos2_ = iz * iz - c_p * tmp_;
                    tl_rsq_sqrt(cos2_, r_t, cos_t);            // refraction side of surface k-1, for the next row
                    if (PEN) s2t = (ix * ix + iy * iy) + c_p * tmp_;
                    db = e_ + tmp_ * tl_rcp(iz + cos_t);
                    px = hx + db * ix; py = hy + db * iy; pz = hzs + db * iz;
                }
                if (asph_k) {
                    av.s = -db;
                } else {
                    v.d = -db;
                    v.e = ehi - db;
                    v.q = -ehi;
                    v.m2 = hh - ehi * ehi;
                    v.tmp = c * v.m2 - 2.0f * (hz + ehi * iz);
                }
                in.x = px; in.y = py; in.z = pz - t_p;
                hx = px; hy = py; hz = pz;                     // hit on surface k-1, frame k-1
            }
            // ---- adjoint of the forward step k at that state
            float g_c, g_t, g_mu;
            if (asph_k) {
                float ga[5];
                asph_adjoint<PENB, true>(in, A, mu, av, a, g_c, g_t, g_mu, ga, sk, zpos);
                // lane q of every quad keeps the quad's sum of term q (kappa, a4, a6 | a8, a10) in two private slots
                const int jk = __popc(kbits & ((1u << k) - 1u));
                sasph_dyn[(2 * jk) * kBlock + tid] += quad_term_sums(ga[0], ga[1], ga[2], q_odd, q_hi);
                sasph_dyn[(2 * jk + 1) * kBlock + tid] += quad_term_sums(ga[3], ga[4], 0.0f, q_odd, q_hi);
            } else {
                v.inv_den = tl_rcp_adj(in.cz + v.cos_i);
                step_adjoint<PENB, true>(in, c, mu, v, a, g_c, g_t, g_mu, sk, zpos);
            }
            dx = ix; dy = iy; dz = iz;                         // the ray between surfaces k-1 and k
            r_c[k] += g_c;
            if (PAIR) {                                        // pair sums: both lanes add and store the same value
                g_t += quad_perm<0xB1>(g_t);
                g_mu += quad_perm<0xB1>(g_mu);
            }
            sacc_dyn[k * SLOTS + slot] += g_t;
            sacc_dyn[(NS + k) * SLOTS + slot] += g_mu;
            asm volatile("" : "+v"(hz) : "v"(r_c[k]), "v"(a.x), "v"(a.z));      // row fence, see the header
        };
        auto row = [&](auto kc) {
            if constexpr (ASPH) {
                constexpr int k = row_index<decltype(kc)>::value;
                constexpr int kp = k > 0 ? k - 1 : 0;
                const bool any_asph = ((kbits >> k) & 1u) || (k > 0 && ((kbits >> kp) & 1u));       // wave-uniform
                if (any_asph) row_impl(kc, std::true_type{});
                else row_impl(kc, std::false_type{});
            } else {
                row_impl(kc, std::false_type{});
            }
        };
        static_for_down<NS>(row);
#undef TL_LOAD_HIT
        TL_WALK_ENTRANCE_ADD(a);
        if (valid) {
            if (gxin) (gxin + ob)[ut] = a.x;
            if (gyin) (gyin + ob)[ut] = a.y;
        }
    }
    // ---- block reduction: this lane's sums -> the quad-transposed rows the rolled kernel keeps, then the common tail
    const int lane = tid & 63, wv = tid >> 6;
    if (!PAIR) {
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            const float vt = sacc_dyn[k * kBlock + tid], vm = sacc_dyn[(NS + k) * kBlock + tid];
            sacc_dyn[k * kBlock + tid] = quad_term_sums(r_c[k], vt, vm, q_odd, q_hi);   // own slot of the g_t block only
        }
    } else {
        // the pair slots [2 NS][128] and the [NS][256] rows written next overlap: read everything first; the pair
        // sum sits in both lanes of a pair, the even one contributes it
        float vt[NS], vm[NS];
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            vt[k] = q_odd ? 0.0f : sacc_dyn[k * SLOTS + slot];
            vm[k] = q_odd ? 0.0f : sacc_dyn[(NS + k) * SLOTS + slot];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < NS; ++k) sacc_dyn[k * kBlock + tid] = quad_term_sums(r_c[k], vt[k], vm[k], q_odd, q_hi);
    }
    TL_WALK_STORE_PARTIALS(NS);
    if (ASPH) {
        // g_kappa[k] -> column 3NS+3+k ; g_poly[k][j] -> column 4NS+3+4k+j.  Slot j holds this lens' j-th aspheric row:
        // lanes = 0, 1, 2 (mod 4) of the even slot row hold kappa, a4, a6, lanes = 0, 1 of the odd one a8, a10.
        if (tid < NS && !((kbits_all >> tid) & 1u)) {                  // spherical rows: zeros
            row[(size_t)(3 * NS + 3 + tid) * nrows_] = 0.0;
            for (int j = 0; j < 4; ++j) row[(size_t)(4 * NS + 3 + 4 * tid + j) * nrows_] = 0.0;
        }
        int j = 0;
        for (int k = 0; k < NS; ++k) {
            if (!((kbits_all >> k) & 1u)) continue;                    // wave-uniform
            if ((j & (kWaves - 1)) == wv) {
                const float *qa = sasph_dyn + (size_t)(2 * j) * kBlock, *qb = qa + kBlock;
                double va = (double)qa[lane] + (double)qa[lane + 64];
                va += (double)qa[lane + 128];
                va += (double)qa[lane + 192];
                double vb = (double)qb[lane] + (double)qb[lane + 64];
                vb += (double)qb[lane + 128];
                vb += (double)qb[lane + 192];
#pragma unroll
                for (int o = 32; o >= 4; o >>= 1) { va += __shfl_xor(va, o, 64); vb += __shfl_xor(vb, o, 64); }
                if (lane == 0) row[(size_t)(3 * NS + 3 + k) * nrows_] = va;
                if (lane == 1 || lane == 2) row[(size_t)(4 * NS + 3 + 4 * k + (lane - 1)) * nrows_] = va;
                if (lane < 2) row[(size_t)(4 * NS + 3 + 4 * k + 2 + lane) * nrows_] = vb;
            }
            ++j;
        }
    }
}

#undef TL_WALK_STORE_PARTIALS
#undef TL_WALK_ENTRANCE_ADD
#undef TL_WALK_ENTRANCE_SUMS
#undef TL_HIT
#undef TL_HIT_S2T
#undef TL_HIT_PLAIN

// ------------------------------------------------------------------ arithmetic self-test (tl_selftest_arith)
__global__ void selftest_arith_kernel(const float *__restrict__ a, const float *__restrict__ b, const int64_t n,
                                      float *__restrict__ quot, float *__restrict__ root)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    quot[i] = tl_div(a[i], b[i]);
    root[i] = tl_sqrt(b[i]);
}

static int launch_selftest_arith(const float *a, const float *b, int64_t n, float *quot, float *root, hipStream_t st)
{
    hipLaunchKernelGGL(selftest_arith_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, b, n, quot, root);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------ host launchers
// (the C entry's blocks -- tl_rays, tl_seeds, tl_grads -- come down as they are: a kernel's pointer list is written out
// once, at its hipLaunchKernelGGL)
static int launch_fwd(const tl_problem &p, const tl_rays &o, const tl_part &w, hipStream_t st)
{
    dim3 grid(w.nbx, tl_lenses(p) * p.F * p.W), block(kBlock);
#define TL_FWD(PEN_, ASPH_, OPD_) \
    hipLaunchKernelGGL((trace_fwd_kernel<PEN_, ASPH_, OPD_>), grid, block, 0, st, p, o.x, o.y, o.cx, o.cy, o.ok, o.back, o.opd, o.stacks, w.part)
    const bool asph = p.surf_kind != nullptr, wopd = p.n_index != nullptr && o.opd != nullptr;
    if (p.aggregate && asph) TL_FWD(true, true, false);
    else if (p.aggregate) TL_FWD(true, false, false);
    else if (asph && wopd) TL_FWD(false, true, true);
    else if (asph) TL_FWD(false, true, false);
#if TL_FAST
    else if (wopd) {
        // All-spherical lens, fast mode: the ray outputs, flags and moments come from the kernel that a trace without OPD
        // runs, so that asking for the OPD changes no bit of them (contraction fuses the two kernel bodies into different
        // multiply-adds: up to 3e-6 mm in x, y otherwise); trace_fwd_kernel then writes the OPD alone, and gives none to a ray
        // that the first kernel's `ok` calls dead (kOkIn).  (An optional path, not tuned: one more forward launch.)
        hipLaunchKernelGGL((trace_fwd_plain_kernel<2>), grid, block, 0, st, p, o.x, o.y, o.cx, o.cy, o.ok, o.back, w.part);
        tl_problem q = p;
        q.cond_flags = nullptr;
        hipLaunchKernelGGL((trace_fwd_kernel<false, false, true>), grid, block, 0, st, q, (float *)nullptr, (float *)nullptr,
                           (float *)nullptr, (float *)nullptr, o.ok /* read, not written */, (uint8_t *)nullptr, o.opd,
                           (float *)nullptr, (double *)nullptr);
    }
#else
    else if (wopd) TL_FWD(false, false, true);
#endif
#if TL_FAST
    // two rays per lane: -10 % in fast mode (latency-bound chains), +4 % in strict mode (issue-bound, fewer waves)
    else hipLaunchKernelGGL((trace_fwd_plain_kernel<2>), grid, block, 0, st, p, o.x, o.y, o.cx, o.cy, o.ok, o.back, w.part);
#else
    else TL_FWD(false, false, false);
#endif
#undef TL_FWD
    return (int)hipGetLastError();
}

template <int NS>
static int launch_bwd_ns(const tl_problem &p, const tl_seeds &g, const tl_grads &o, const tl_part &w, hipStream_t st,
                         const tl_fallback &fb)
{
    dim3 grid(w.nbx, tl_lenses(p) * p.F * p.W), block(kBlock);
    // (gstk: the per-ray stack seeds, kPenRay; the caller has checked p.aggregate)
    const float *gstk = g.g_stacks;
#define TL_BWD(ASPH_, PEN_) \
    hipLaunchKernelGGL((trace_bwd_kernel<NS, ASPH_, PEN_>), grid, block, 0, st, p, g.gx, g.gy, g.gcx, g.gcy, g.g_moments, \
                       o.g_x_in, o.g_y_in, w.part, fb.mom, fb.poison, fb.token, g.g_opd, fb.dead_ok, gstk)
    if (p.surf_kind && p.aggregate && gstk) TL_BWD(true, kPenRay);
    else if (p.surf_kind && p.aggregate) TL_BWD(true, kPenUniform);
    else if (p.surf_kind) TL_BWD(true, kPenNone);
    else if (p.aggregate && gstk) TL_BWD(false, kPenRay);
    else if (p.aggregate) TL_BWD(false, kPenUniform);
    else TL_BWD(false, kPenNone);
#undef TL_BWD
    return (int)hipGetLastError();
}

// the checkpoint kernel of the row bucket tl_bwd_bucket(p.S) (its partial rows: tl_bwd_row doubles); fb: see tl_fallback
static int launch_bwd(const tl_problem &p, const tl_seeds &g, const tl_grads &o, const tl_part &w, hipStream_t st,
                      const tl_fallback &fb = {})
{
    const int ns = tl_bwd_bucket(p.S);
    switch (ns) {
    case 4:  return launch_bwd_ns<4>(p, g, o, w, st, fb);
    case 8:  return launch_bwd_ns<8>(p, g, o, w, st, fb);
    case 12: return launch_bwd_ns<12>(p, g, o, w, st, fb);
    case 16: return launch_bwd_ns<16>(p, g, o, w, st, fb);
    case 20: return launch_bwd_ns<20>(p, g, o, w, st, fb);
    case 24: return launch_bwd_ns<24>(p, g, o, w, st, fb);
    case 32: return launch_bwd_ns<32>(p, g, o, w, st, fb);
    default: return -1;
    }
}

// w.inv / w.ck: partial rows of the walk-back kernel (3S+3 columns) and of its checkpoint fallback
// (3NS+3 columns); exactly one of the two launches does the work, decided on the device (fallback_needed) -- except
// with the penalty term, where the checkpoint kernel also takes the rays that died on the way (see trace_bwd_kernel).
// (f.ok: the forward's ok bytes, or p.cond_flags in their place when the forward wrote those)
static int launch_bwd_inv(const tl_problem &p, const tl_seeds &g, const tl_rays &f, const tl_grads &o, const tl_walkback &w,
                          hipStream_t st)
{
    dim3 grid(w.inv.nbx, tl_lenses(p) * p.F * p.W), block(kBlock);
    // TL_INV_LDS_PAD (bytes, development only): extra dynamic LDS per block = fewer resident blocks per CU, to measure how
    // the kernel's throughput depends on its occupancy without touching its code.  TL_INV_ROLLED=1 (development only):
    // the rolled kernel for every lens, for A/B timing against the unrolled one.
    static const size_t lds_pad = [] { const char *v = getenv("TL_INV_LDS_PAD"); return (v && *v) ? (size_t)atol(v) : (size_t)0; }();
    static const bool rolled_only = [] { const char *v = getenv("TL_INV_ROLLED"); return v && *v == '1'; }();
    const size_t lds = (size_t)p.S * kBlock * sizeof(float);
    const bool asph = p.surf_kind != nullptr, pen = p.aggregate != 0;
    const bool hits = asph && p.asph_hits != nullptr && p.asph_hit_slots > 0;
    const size_t lds_asph = hits ? (size_t)2 * p.asph_hit_slots * kBlock * sizeof(float) : 0;
    const float *gstk = g.g_stacks;
#define TL_INV_ARGS p, g.gx, g.gy, g.gcx, g.gcy, g.g_moments, f.x, f.y, f.cx, f.cy, f.ok, f.moments, o.g_x_in, o.g_y_in, \
                    w.inv.part
#define TL_INVU_V(NS_, ASPH_, PEN_) \
    hipLaunchKernelGGL((trace_bwd_inv_unrolled_kernel<NS_, ASPH_, PEN_>), grid, block, \
                       (NS_ < kInvUnrollPairMin ? 2 : 1) * lds + lds_asph + lds_pad, st, TL_INV_ARGS, w.poison, w.token, gstk)
#define TL_INVU(NS_) \
    case NS_: if (asph && pen && gstk) TL_INVU_V(NS_, true, kPenRay); else if (asph && pen) TL_INVU_V(NS_, true, kPenUniform); \
              else if (asph) TL_INVU_V(NS_, true, kPenNone); else if (pen && gstk) TL_INVU_V(NS_, false, kPenRay); \
              else if (pen) TL_INVU_V(NS_, false, kPenUniform); else TL_INVU_V(NS_, false, kPenNone); break
    if (tl_route(p) == TL_ROUTE_WALK_UNROLLED && !rolled_only) {              // (no skip there for waves past the end of a small pupil)
        switch (p.S) {
#ifdef TL_INVU_DEV      // development builds: the row counts of the bench workloads only (compile time)
            TL_INVU(7); TL_INVU(11); TL_INVU(20);
#else
            TL_INVU(3); TL_INVU(4); TL_INVU(5); TL_INVU(6); TL_INVU(7); TL_INVU(8); TL_INVU(9); TL_INVU(10); TL_INVU(11); TL_INVU(12);
            TL_INVU(13); TL_INVU(14); TL_INVU(15); TL_INVU(16); TL_INVU(17); TL_INVU(18); TL_INVU(19); TL_INVU(20);
#endif
        default: return -1;
        }
    } else if (pen) {
        return -1;                // (the C entry point sends the penalty term of such lenses to tl_trace_bwd)
    } else if (asph) {
        hipLaunchKernelGGL(trace_bwd_inv_kernel<true>, grid, block, lds + lds_pad, st, TL_INV_ARGS, 0 /*unused*/, w.poison, w.token);
    } else {
        hipLaunchKernelGGL(trace_bwd_inv_kernel<false>, grid, block, lds + lds_pad, st, TL_INV_ARGS, 0 /*unused*/, w.poison, w.token);
    }
#undef TL_INVU
#undef TL_INVU_V
#undef TL_INV_ARGS
    const int herr = (int)hipGetLastError();
    if (herr) return herr;
    return launch_bwd(p, g, o, w.ck, st, {f.moments, w.poison, w.token, (pen || p.cond_flags) ? f.ok : nullptr});
}

}  // namespace TL_NS

// the per-mode entry points tl_common.h declares (TL_DECLARE_MODE), for the mode this translation unit is built in
namespace TL_API_NS {
int api_fwd(const tl_problem &p, const tl_rays &out, const tl_part &w, hipStream_t st) { return TL_NS::launch_fwd(p, out, w, st); }
int api_bwd(const tl_problem &p, const tl_seeds &g, const tl_grads &out, const tl_part &w, hipStream_t st)
{ return TL_NS::launch_bwd(p, g, out, w, st); }
int api_bwd_inv(const tl_problem &p, const tl_seeds &g, const tl_rays &fwd, const tl_grads &out, const tl_walkback &w, hipStream_t st)
{ return TL_NS::launch_bwd_inv(p, g, fwd, out, w, st); }
int api_selftest_arith(const float *a, const float *b, int64_t n, float *quot, float *root, hipStream_t st)
{ return TL_NS::launch_selftest_arith(a, b, n, quot, root, st); }
}
