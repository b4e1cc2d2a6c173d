// tl_common.h -- shared by the per-mode kernel TUs and the C-ABI TU.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <type_traits>
#include "../../include/tl_trace.h"

// compile-time surface-row buckets of the backward kernel
static inline int tl_bwd_bucket(int S)
{
    static const int b[] = {4, 8, 12, 16, 20, 24, 32};
    for (int v : b) if (S <= v) return v;
    return -1;
}

// doubles per block-partial row of the backward kernel (see trace_bwd_kernel)
// g_c | g_t | g_mu [NS each] | g_z g_cx g_cy | [g_kappa[NS] | g_poly[NS][4]] | g_n[NS+1]
__host__ __device__ static inline int tl_bwd_row(int ns, bool asph) { return (asph ? 8 : 3) * ns + 3 + ns + 1; }

// Row counts the walk-back kernel is instantiated for with its row loop unrolled (trace_bwd_inv_unrolled_kernel), and
// the smallest pupil it takes (no skip there for waves past the end of a small pupil).
#define TL_INVU_MIN 3
#define TL_INVU_MAX 20
// bytes of the penalty walk-back's scan map (tl_kernels.inc: tl_scanmap): one per (row of the grid, 256-ray chunk, wave of
// the 256-thread block), rounded up to 256
__host__ __device__ static inline size_t tl_scanmap_bytes(int rows, int64_t nchunks)
{
    return (((size_t)rows * (size_t)nchunks * 4u) + 255u) & ~(size_t)255u;
}

static inline bool tl_walk_unrolled(int S, int P) { return S >= TL_INVU_MIN && S <= TL_INVU_MAX && P >= 256; }

// The host's routing of tl_trace_bwd_from_outputs (tl_trace.h: tl_bwd_route), written once: the C entry point, launch_bwd_inv
// and tl_bwd_route all read it.  Aspheric rows are walked back by the unrolled kernels only from their stored hit points.
static inline int tl_route(const tl_problem &p)
{
    if (p.P == 0) return TL_ROUTE_EMPTY;
    const bool hits_ok = p.surf_kind == nullptr || (p.asph_hits != nullptr && p.asph_hit_slots > 0);
    if (tl_walk_unrolled(p.S, p.P) && hits_ok) return TL_ROUTE_WALK_UNROLLED;
    return p.aggregate ? TL_ROUTE_CHECKPOINT : TL_ROUTE_WALK_ROLLED;
}

// What makes a checkpoint launch (trace_bwd_kernel) the fallback of a walk-back launch in front of it: the forward's moments
// and the walk-back's poison word / token decide on the device whether it runs; dead_ok = the forward's ok bytes when it also
// takes single rays (the penalty term's dead rays, flagged ill-conditioned rays).  All zero: an ordinary backward.
struct tl_fallback {
    const double *mom;
    const unsigned *poison;
    unsigned token;
    const uint8_t *dead_ok;
};

// One array of block partials in the workspace and the grid of the launch that fills it: nbx blocks per grid row (rays
// per thread follow from the grid: TL_BLOCK_CHUNKS).  What tl_walkback carries down to a walk-back launch: its own partials,
// those of the checkpoint launch queued behind it, and the poison word / token that tell the two apart (see tl_fallback).
struct tl_part { double *part; int nbx; };
struct tl_walkback {
    tl_part inv, ck;
    unsigned *poison;
    unsigned token;
};

// per-mode launchers (defined once, at the end of tl_kernels.inc, for the mode of the including unit); return hipError_t
// as int.  The blocks are the C entry's, forwarded as they are; tl_part / tl_walkback are filled from the entry point's
// workspace layout (tl_api.hip: Layout).
#define TL_DECLARE_MODE(NS)                                                                                        \
    namespace NS {                                                                                                 \
    int api_fwd(const tl_problem &p, const tl_rays &out, const tl_part &w, hipStream_t st);                        \
    int api_bwd(const tl_problem &p, const tl_seeds &g, const tl_grads &out, const tl_part &w, hipStream_t st);    \
    int api_bwd_inv(const tl_problem &p, const tl_seeds &g, const tl_rays &fwd, const tl_grads &out,               \
                    const tl_walkback &w, hipStream_t st);                                                         \
    int api_selftest_arith(const float *a, const float *b, int64_t n, float *quot, float *root, hipStream_t st);   \
    }
TL_DECLARE_MODE(tl_strict)
TL_DECLARE_MODE(tl_fast)

// double-precision twin (tl_f64.hip): generic, untuned kernels behind tl_trace_fwd_f64 / tl_trace_bwd_f64
namespace tl_f64 {
int launch_fwd(const tl_problem &p, const tl_rays &out, double *part, int nbx, hipStream_t st);
int launch_reduce_moments(const tl_problem &p, const double *part, double *mom, int nbx, hipStream_t st);
int launch_bwd(const tl_problem &p, const tl_seeds &g, const tl_grads &out, double *part, int nbx, hipStream_t st);
}

// The calling thread's error message (tl_last_error) and the frame around every launch of a C entry point; defined in
// tl_api.hip, used by every translation unit that holds entry points.
namespace tl_host {
int fail(int code, const char *msg);            // sets the message, returns code
int hip_fail(int herr, const char *where);      // "<where>: <HIP's error string>", returns TL_ELAUNCH
int use_device(int device);                     // hipSetDevice: TL_OK, or hip_fail(.., "hipSetDevice")
int launched(const char *what);                 // hipGetLastError() behind a launch: TL_OK, or hip_fail(.., what)
}
