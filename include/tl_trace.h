/*
 * tl_trace.h -- C ABI of the MI355X (gfx950) sequential ray-trace library, libtltrace.so
 *
 * The reference (OceanT-shirt/TorchOptics) has no FFI: its hot path is a chain of
 * in-process Python calls.  Each entry point below states which reference function it
 * stands in for (file:line under torchlens/); the Python host in torchoptics_amd/
 * mirrors the reference signatures on top of these.  The image side (image_ops.py) is here
 * too: tl_svola_* blurs an image with the lens's PSFs, tl_warp_* resamples it through the
 * distortion map and multiplies the relative illumination in.  tl_focus_* sums the through-focus
 * moments of a traced fan (best focus, tangential / sagittal foci, axial colour), tl_enclosed_* its
 * encircled / ensquared energy under a smooth edge, tl_zfit_* fits Zernike wavefront coefficients
 * to its transverse ray errors, tl_mtf_* sums its geometric OTF at given spatial frequencies, tl_tfmtf_* the
 * same at equally spaced focal planes from one pass over the rays.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless marked "host";
 *   - nothing is allocated here: the caller owns all buffers (stream-ordered borrow);
 *   - functions are re-entrant and thread-safe (autograd calls backward from its own
 *     thread; ray aiming re-enters the tracer inside a forward);
 *   - return 0 on success, a negative TL_E* code otherwise; tl_last_error() gives the
 *     message for the calling thread;
 *   - the ray batch is [B lenses][F fields][W wavelengths][P pupil points] with P contiguous
 *     ("FWP" layout): one wavefront = 64 consecutive pupil points of one (b, f, w).  B = 1 is the
 *     reference's callers' case; every "[F,...]" / "[S]" shape below gains a leading B when B > 1.
 */
#ifndef TL_TRACE_H
#define TL_TRACE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TL_ABI_VERSION 15
#define TL_MAX_SURFACES 32       /* rows per lens the backward kernels are built for */
#define TL_NMOM 10               /* per-field sums, see tl_trace_fwd */
#define TL_MAX_POLY 4            /* even aspheric terms a4,a6,a8,a10 */
#define TL_MAX_HIT_SLOTS 8       /* aspheric rows per lens whose hit points tl_trace_fwd can hand to the walk-back */
#define TL_MAX_AIM_ITER 16       /* Newton steps of tl_ray_aim_iter (RayTracer n_ray_aiming_iter) */

enum {
    TL_OK = 0,
    TL_EINVAL = -1,      /* bad argument (null pointer, bad size, S > TL_MAX_SURFACES ...) */
    TL_ELAUNCH = -2,     /* HIP launch / runtime failure; message has hipGetErrorString */
    TL_EWORKSPACE = -3   /* workspace too small, see tl_workspace_bytes */
};

enum { TL_MODE_STRICT = 0,   /* op-order-faithful fp32, no FMA contraction, IEEE sqrt and divide:
                                forward bit-exact with the reference's eager fp32 ops        */
       TL_MODE_FAST = 1 };   /* FMA contraction + hardware rcp/rsq; a few ulp from strict   */

/*
 * One trace problem.  Mirrors the argument list of
 *   trace_skew(x, y, z, cx, cy, c, t, mu, mask, aggregate, allow_backward_rays)
 *   (ray_tracing_lite.py:594), whose tensors broadcast over a leading lens axis [B, ...]: a batch of B padded
 *   lenses (Structure / Lens of lens_modeling.py:151-386 hold B rows) is ONE launch here, blockIdx.y = (b F + f) W + w.
 *   Padded rows (c = 0, t = 0, mu = 1, mask 0) are traced as the identity rows they are in the reference.
 */
typedef struct tl_problem {
    int32_t F, P, W, S;          /* fields, pupil points in this shard, wavelengths, surface rows (per lens) */
    int32_t device;              /* HIP device ordinal the pointers live on */
    int32_t mode;                /* TL_MODE_* */
    int32_t allow_backward;      /* allow_backward_rays (ray_tracing_lite.py:629) */
    int32_t aggregate;           /* aggregate=True of trace_skew (:641-657): evaluate the penalty-term quantities
                                    (aspheric rows included: theta from the cosine at the aspheric normal) */
    /* entrance-pupil ray coordinates; element strides (floats) over (b, f, p, w), 0 = broadcast.
       Reference shapes [1|B, 1|F, P, 1|W] (ray_tracing_lite.py:112-113). */
    const float *x_in, *y_in;
    int64_t xs_f, xs_p, xs_w;
    int64_t ys_f, ys_p, ys_w;
    const float *z;              /* [B]   pupil position (ray_tracing_lite.py:91)            */
    const float *cx, *cy;        /* initial direction cosines (:116-118), element (b, f) at
                                    cx[b * cx_stride_b + f * cx_stride]                      */
    int32_t cx_stride, cy_stride;/* 1 or 0 (broadcast over fields)                           */
    const float *c, *t;          /* [B,S]   curvature, thickness (:121-122)                  */
    const float *mu;             /* [B,W,S] n_before/n_after per wavelength (:123)           */
    const uint8_t *mask;         /* [B,S]   non-padding rows (:124)                          */
    /* ---- aspheric extension (not in the reference; all three NULL = all-spherical) ----
       sag(rho) = c rho/(1+sqrt(1-(1+kappa) c^2 rho)) + a4 rho^2 + a6 rho^3 + a8 rho^4 + a10 rho^5,
       rho = x^2+y^2; rows with surf_kind 1 are intersected by Newton iteration from the closed-form
       sphere hit and refracted at the aspheric normal; rows with surf_kind 0 take the reference's
       closed form and ignore kappa / poly. */
    const float *kappa;          /* [B,S]   conic constant                                   */
    const float *poly;           /* [B,S,TL_MAX_POLY] a4,a6,a8,a10                           */
    const uint8_t *surf_kind;    /* [B,S]   0 = closed-form sphere, 1 = Newton asphere       */
    const float *n_index;        /* [B,W,S+1] refractive indices (entry 0 = object space); only
                                    read when tl_trace_fwd is asked for `opd`                 */
    /* ---- lens batch (ABI 12) ---- */
    int32_t B;                   /* lenses in this launch; 0 is read as 1.  B * F * W <= 65535 */
    int32_t cx_stride_b, cy_stride_b;   /* element stride of cx / cy over the lens index (0 = shared) */
    int64_t xs_b, ys_b;          /* element stride of x_in / y_in over the lens index (0 = shared) */
    /* ---- ABI 13 ---- */
    float *asph_hits;            /* [asph_hit_slots][2][B,F,W,P] float, nullable: the hit point (X, Y) of every ray on the
                                    j-th aspheric row of its lens, j < asph_hit_slots -- WRITTEN by tl_trace_fwd, READ by
                                    tl_trace_bwd_from_outputs, which then needs no Newton iteration on the reversed ray (and
                                    re-anchors the reconstruction at every aspheric row).  8 bytes per ray and aspheric row.
                                    A lens with more aspheric rows than slots is still traced correctly: its backward falls
                                    back, on the device, to the checkpoint kernel.  NULL: Newton on the reversed ray. */
    int32_t asph_hit_slots;      /* 0..TL_MAX_HIT_SLOTS */
    int32_t moments_x;           /* 1: tl_trace_fwd also accumulates the x-moments 4..6 (compute_rms2d reads y only:
                                    ray_tracing_lite.py:684-701); 0: they are returned as 0 */
    uint8_t *cond_flags;         /* [B,F,W,P] bytes, nullable: the `ok` output with the conditioning flag -- 0 dead, 1 live, 2 live
                                    and ill-conditioned (smallest cos^2 of incidence or refraction below 0.01: the rays moment 9
                                    counts) -- WRITTEN by tl_trace_fwd (next to `ok`, which stays 0/1), READ by
                                    tl_trace_bwd_from_outputs in place of fwd->ok.  With it, a launch that holds such rays is
                                    no longer handed to the checkpoint kernel as a whole: the walk-back differentiates the
                                    rays marked 1 and the checkpoint kernel exactly those marked 2 (waves without one skip
                                    their chunk); the two partial sums are added.  NULL: one ill-conditioned ray sends the
                                    whole launch to the checkpoint kernel. */
} tl_problem;

int         tl_version(void);            /* == TL_ABI_VERSION */
const char *tl_last_error(void);         /* host string, thread-local, never NULL */
size_t      tl_problem_size(void);       /* sizeof(tl_problem): lets a foreign-language binding check its layout */

/* Bytes of scratch (device) the calls below need for this problem. */
size_t tl_workspace_bytes(const tl_problem *p);

/*
 * The buffers of a trace call, as three blocks of named device pointers (ABI 15).  A caller zero-initialises a block and
 * assigns the members it has; the library reads a block during the call only.  Shapes for B = 1; with a lens batch
 * every per-ray array gains a leading B: [B,F,W,P], moments [B,F,TL_NMOM], stacks [3][S][B,F,W,P].
 *
 * tl_rays -- what tl_trace_fwd writes (every member nullable = not wanted), and what tl_trace_bwd_from_outputs reads again:
 *   x,y,cx,cy : [F,W,P] float
 *   ok,back   : [F,W,P] uint8
 *   opd       : [F,W,P] float  optical path length sum_k n_k d_k + n_S d_image from the pupil plane
 *               to the image plane, 0 for failed rays; needs p->n_index (extension; its gradient: tl_seeds.g_opd)
 *   stacks    : [3][S][F,W,P] float (p->aggregate only): the per-surface stacks
 *               z_RELU | theta_norm | theta_prime_norm that trace_skew(aggregate=True) returns
 *               (their gradient: tl_seeds.g_stacks)
 *   moments   : [F,TL_NMOM] double, per field over (w,p):
 *               0 sum y | 1 sum ok*y | 2 sum ok*y^2 | 3 sum ok | 4 sum x | 5 sum ok*x |
 *               6 sum ok*x^2 | 7 sum back | 8 sum q (p->aggregate only) |
 *               9 number of ILL-CONDITIONED live rays: smallest cos^2 of incidence / refraction along the
 *                 path below 0.01 (fp32 rounding is amplified ~1/cos^2 there)
 *               -- 0..3 are the sufficient statistics of compute_rms2d (ray_tracing_lite.py:678-702);
 *               q = per-ray sum over the surfaces of theta_norm + theta_prime_norm + z_RELU
 *               (ray_tracing_lite.py:641-657), NaN -> 0, i.e. sumQ * n_sequence of
 *               optics_simulator_lite.py:441-448.  All reduced in a fixed order (bitwise reproducible).
 */
typedef struct tl_rays {
    float *x, *y, *cx, *cy;
    uint8_t *ok, *back;
    float *opd;
    float *stacks;
    double *moments;
} tl_rays;

/*
 * tl_seeds -- the upstream gradients of a backward call, each nullable:
 *   gx,gy,gcx,gcy : [F,W,P] upstream gradients of the per-ray outputs
 *   g_moments     : [F,TL_NMOM] double upstream gradient of `moments`; the per-ray
 *                   seed  gM0 + ok*(gM1 + 2*y*gM2)  (and the x analogue) is formed in-kernel;
 *                   entry 8 seeds the penalty term when p->aggregate
 *   g_opd         : [F,W,P] upstream gradient of the optical path length output (needs p->n_index and
 *                   tl_grads.g_n_index).  OPD = sum_k n_k d_k + n_S d_image: it enters the adjoint of every marching distance
 *                   and so reaches c, t, mu, z, cx, cy, kappa, poly, x_in, y_in; g_n_index [W,S+1] = d/d n_index
 *   g_stacks      : [3][S][F,W,P] float, dense, in the layout of tl_rays.stacks: the upstream gradient of
 *                   z_RELU | theta_norm | theta_prime_norm of every row and ray.
 *                   Needs p->aggregate (TL_EINVAL, before any HIP call, otherwise).  Per ray r and row k:
 *                     - ray ok after row k: theta and theta' are differentiated through cos^2 with the clamp conventions of
 *                       the fused seed (entry 8 of g_moments), z_RELU passes the gradient where z > 0;
 *                     - ray not ok after row k (parked): theta = theta' = 1 carry no gradient, z_RELU = max(-t_k, 0) gives
 *                       d/dt_k only.
 *                   It adds to entry 8 of g_moments: a loss may read both the fused sum and the stacks.  The routing is that of
 *                   the penalty term (tl_trace_bwd_from_outputs: the walk-back for 3..20 rows, P >= 256, aspheric hits stored;
 *                   the checkpoint kernel otherwise).  No host synchronisation: the calls can be recorded into a HIP graph.
 */
typedef struct tl_seeds {
    const float *gx, *gy, *gcx, *gcy;
    const double *g_moments;
    const float *g_opd;
    const float *g_stacks;
} tl_seeds;

/*
 * tl_grads -- the gradient outputs of a backward call:
 *   g_c,g_t [S], g_mu [W,S], g_z [1], g_cx,g_cy [F] : float, required, OVERWRITTEN (not accumulated); summed over the
 *                   rays in fp64 in a fixed order and rounded once.  Lens batch: per lens, [B,S], [B,W,S], [B],
 *                   [B,F] (and g_kappa [B,S], g_poly [B,S,4], g_n_index [B,W,S+1]); a lens never sees another's rays
 *   g_kappa [S], g_poly [S,TL_MAX_POLY] : float (aspheric extension: required iff p->surf_kind)
 *   g_n_index [W,S+1] : float, given together with tl_seeds.g_opd
 *   g_x_in,g_y_in : [F,W,P] float per-ray input gradients (nullable; used by ray aiming,
 *                   ray_tracing_lite.py:169-181)
 */
typedef struct tl_grads {
    float *g_c, *g_t, *g_mu, *g_z, *g_cx, *g_cy;
    float *g_kappa, *g_poly, *g_n_index;
    float *g_x_in, *g_y_in;
} tl_grads;

/*
 * Forward trace: replaces the whole Python loop trace_skew (ray_tracing_lite.py:594-675 =
 * find_marching_distance_spherical :525-545, update_ray_coordinates :514-522,
 * reset_bad_rays :574-591, apply_snell_spherical :548-571, image-plane transfer :659-663).
 * Writes the members of `out` that are not NULL.  A NULL block pointer (here and below) is TL_EINVAL.
 */
int tl_trace_fwd(const tl_problem *p, const tl_rays *out, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Backward trace: replaces PyTorch autograd's replay of the recorded graph of trace_skew
 * (SURVEY 3.4).  Recomputes the forward per ray in registers, then sweeps the surfaces in
 * reverse.
 */
int tl_trace_bwd(const tl_problem *p, const tl_seeds *g, const tl_grads *out,
                 void *workspace, size_t workspace_bytes, void *stream);

/*
 * Backward trace WITHOUT re-tracing forwards: same gradients as tl_trace_bwd, computed by walking each ray
 * back from the forward kernel's own output (`fwd`: x, y, cx, cy, ok, moments as tl_trace_fwd wrote them for this problem;
 * back, opd, stacks are not read) -- undo the refraction at surface k, intersect the incoming line with surface k-1, apply
 * the adjoint step.
 * No per-surface state is kept, so the kernel runs at twice the occupancy and needs no bit-exact
 * re-derivation of the forward; the reconstructed states differ from the forward's by rounding only,
 * which perturbs the gradients at the 1e-6 level (tested) -- except for ill-conditioned rays (moment 9 of
 * tl_trace_fwd), where it would reach 1e-4.  The call therefore always enqueues the checkpoint kernel of
 * tl_trace_bwd behind the walk-back kernel; both decide ON THE DEVICE which of them does the work (no host
 * synchronisation; the idle launch retires in microseconds).  The checkpoint kernel takes over when
 *   - `fwd->moments` (nullable) counts an ill-conditioned live ray -- for exactly those rays when
 *     the forward left their flags in p->cond_flags (read in place of fwd->ok, which may then be NULL; the ok bytes given
 *     otherwise must be 0 / 1 as tl_trace_fwd writes them), for the whole launch when it did not -- or
 *   - the walk-back met a non-finite adjoint (it then flags a word at the end of the workspace): the whole launch.
 * Pass `fwd->moments` whenever it is available.  It may be NULL only when p->cond_flags is NULL too: an ill-conditioned fan is
 * then walked back anyway (nothing tells the call that it holds such rays).  With p->cond_flags and no `fwd->moments` the
 * call is refused (TL_EINVAL, before any HIP call; the message names cond_flags and moments): the walk-back leaves the rays
 * flagged 2 to the checkpoint kernel, which takes them only when the moments count them -- their gradient would be dropped.
 * allow_backward = 1 only, no OPD gradient (TL_EINVAL for g->g_opd or out->g_n_index: use tl_trace_bwd).  Aspheric rows
 * are walked back too (g_kappa, g_poly as in tl_trace_bwd, required iff p->surf_kind).
 * Workspace: tl_workspace_bytes(p); its contents need not be initialised.
 * Recorded into a HIP graph, the call is replayed with the same internal token: give the tl_trace_fwd of the same
 * step the SAME workspace with its full tl_workspace_bytes(p) (with or without `moments`) -- it clears the flag word, so
 * that one replay that had to fall back does not pin every later replay to the (exact, slower) checkpoint kernel.
 * Penalty term (p->aggregate, ABI 13): walked back too for lenses of 3..20 rows -- the rays alive at the image plane by
 * the walk-back kernel, the rays that died on the way (they keep the gradient of the rows they passed alive) by the
 * checkpoint kernel in the same call; other lenses, pupils of fewer than 256 points and aspheric lenses whose hits were not
 * stored are handed to tl_trace_bwd as a whole (the bits of tl_trace_bwd; tl_bwd_route below names the decision).  Aspheric
 * rows (ABI 13): with p->asph_hits filled by tl_trace_fwd the hit on an aspheric row is read instead of searched.
 */
int tl_trace_bwd_from_outputs(const tl_problem *p, const tl_seeds *g, const tl_rays *fwd, const tl_grads *out,
                              void *workspace, size_t workspace_bytes, void *stream);

/*
 * Which kernels tl_trace_bwd_from_outputs enqueues for `p` -- the decision it takes on the host, from S, P, aggregate,
 * surf_kind, asph_hits and asph_hit_slots alone (nothing else of `p` is read, no pointer is followed, no HIP call is made:
 * callable without a device; additive entry point, ABI unchanged):
 *   TL_ROUTE_CHECKPOINT      the whole call is handed to tl_trace_bwd: the penalty term (p->aggregate) of a lens outside
 *                            3..20 rows, of a pupil below 256 points, or with aspheric rows whose hits are not stored
 *                            (p->asph_hits NULL or p->asph_hit_slots 0).  The gradients have the bits of tl_trace_bwd.
 *   TL_ROUTE_WALK_ROLLED     trace_bwd_inv_kernel, rows in a loop: no penalty term, and 1, 2 or 21..32 rows, or P < 256, or
 *                            aspheric rows without stored hits (Newton iteration on the reversed ray).
 *   TL_ROUTE_WALK_UNROLLED   trace_bwd_inv_unrolled_kernel<S>: 3..20 rows, P >= 256, aspheric rows (if any) with stored hits;
 *                            with or without the penalty term.
 *   TL_ROUTE_EMPTY           P = 0: an empty shard, the gradients are zeroed by memsets.
 * Behind either walk-back the checkpoint kernel is still enqueued and takes, on the device, what the walk-back leaves (see
 * above): the route names the launch, not every ray's path.  TL_EINVAL for p NULL, S outside 1..TL_MAX_SURFACES or P < 0.
 */
enum { TL_ROUTE_CHECKPOINT = 0, TL_ROUTE_WALK_ROLLED = 1, TL_ROUTE_WALK_UNROLLED = 2, TL_ROUTE_EMPTY = 3 };
int tl_bwd_route(const tl_problem *p);

/*
 * Spot moments of arbitrary per-ray tensors (same TL_NMOM layout): the reduction inside
 * compute_rms2d(x, y, ray_ok) (ray_tracing_lite.py:678-702) when its inputs did not come
 * from tl_trace_fwd.  Element strides over (f, p, w); x may be NULL.
 */
int tl_spot_moments(int32_t device, int32_t F, int32_t P, int32_t W,
                    const float *x, const float *y, const uint8_t *ok,
                    int64_t s_f, int64_t s_p, int64_t s_w,
                    double *moments, void *workspace, size_t workspace_bytes, void *stream);

/*
 * The closed form of compute_rms2d (ray_tracing_lite.py:684-701) on the moments, and its derivative:
 *   rms = mean_f sqrt((M2 - 2 m M1 + m^2 M3) / n),  m = M0 / n,  n = P*W rays per field (of the WHOLE
 *   pupil when it is sharded over GPUs: pass the all-reduced moments).
 *   rms [B] float (one value per lens: moments [B,F,TL_NMOM]; compute_rms2d itself reads lens 0 only);
 *   d_moments [B,F,TL_NMOM] double = d rms[b] / d moments[b] (zero where the variance is 0).
 */
int tl_spot_rms(int32_t device, int32_t B, int32_t F, double n_per_field, const double *moments, float *rms,
                double *d_moments, void *stream);

/*
 * loss_dict of RaytracedOptics.compute_loss_out (optics_simulator_lite.py:430-450) per lens, on the moments of an
 * aggregate trace:  rms[b] as tl_spot_rms,  penalty[b] = (sum_f moments[b,f,8]) / n_sequence  (sumQ :441-448, the
 * per-ray sums fused into the trace kernel; rounded to float),  loss[b] = rms[b] + penalty_rate * penalty[b]  (:449).
 * One launch instead of ~10 elementwise ones; same rounding points as that op sequence.
 *   n_sequence: [B] doubles on the device (padded batches: rows of each lens' sequence), or NULL: n_sequence_all for all;
 *   d_rms [B,F,TL_NMOM] double = d rms[b] / d moments[b], for tl_unsup_loss_bwd.
 * tl_unsup_loss_bwd: g_moments [B,F,TL_NMOM] = d(sum_b g_loss[b] loss[b] + g_rms[b] rms[b] + g_penalty[b] penalty[b]) /
 *   d moments; each upstream gradient nullable (not all three), element b at g[b * g_stride] (g_stride 0: one value for all).
 */
int tl_unsup_loss(int32_t device, int32_t B, int32_t F, double n_per_field, const double *moments, const double *n_sequence,
                  double n_sequence_all, float penalty_rate, float *loss, float *rms, float *penalty, double *d_rms,
                  void *stream);
int tl_unsup_loss_bwd(int32_t device, int32_t B, int32_t F, const double *d_rms, const float *g_loss, const float *g_rms,
                      const float *g_penalty, int32_t g_stride, const double *n_sequence, double n_sequence_all,
                      float penalty_rate, double *g_moments, void *stream);

/* d(loss)/dy, d(loss)/dx per ray from d(loss)/d(moments); outputs [F,P,W]-strided like y. */
int tl_spot_seed(int32_t device, int32_t F, int32_t P, int32_t W,
                 const float *x, const float *y, const uint8_t *ok,
                 int64_t s_f, int64_t s_p, int64_t s_w,
                 const double *g_moments, float *gx, float *gy, void *stream);

/*
 * Paraxial entrance-pupil position w.r.t. the first vertex -- the `z` argument of the trace
 * (compute_pupil_position, ray_tracing_lite.py:301-350): z = B/A of the ABCD product of the K rows in
 * front of the stop, row k = refraction at curvature c[k] from index n[k] to n[k+1], then a gap t[k].
 *   c, t [B,K], n [B,K+1] (n[.,0] = object space), z [B] (nullable): float; B lenses, one thread each (rows behind a
 *   lens' own stop padded with c = 0, t = 0, n = 1: identity).
 *   g_z [B] (nullable): upstream gradient; then g_c, g_t [B,K] and g_n [B,K+1] are OVERWRITTEN with
 *   d(loss)/d(c, t, n).  One tiny launch instead of the ~25 (+ ~60 in autograd) of the elementwise / 2x2-matmul chain.
 *   mode (ABI 13): TL_MODE_STRICT -- z is the reference's fp32 value bit for bit (its pairwise product tree of fp32 2x2
 *   matrices, reduce_abcd :301-318, every operation rounded separately); TL_MODE_FAST -- the product in fp64, rounded
 *   once.  The gradient is the fp64 adjoint in both modes.
 */
int tl_pupil_position(int32_t device, int32_t B, int32_t K, const float *c, const float *t, const float *n, float *z,
                      const float *g_z, float *g_c, float *g_t, float *g_n, int32_t mode, void *stream);

/*
 * Ray aiming, one iteration (RayTracer.ray_aiming, ray_tracing_lite.py:129-208, with compute_pupil_radius :834-844,
 * ray_aiming_mode 'real'): per (lens, field, wavelength) the three 'tee' rays -- bottom and top meridional, +x sagittal --
 * are traced to the stop through the K rows in front of it, one Newton step each brings them to where an ideal pupil
 * would put them (stop radius = height of the on-axis d-line marginal ray), and the affine pupil map through the
 * corrected rays is returned:   x_pupil' = x_pupil * x_scale,   y_pupil' = y_pupil * y_scale + y_offset.
 * One thread per (lens, field, wavelength), fp64 in registers, Jacobian by central differences (the reference:
 * two eager traces + an autograd pass, ~60 tensor ops per call).  No gradient: the reference aims a detached lens (:108).
 *   c, t [B,K]; n [B,K,W] refractive index behind each row at the tracer's wavelengths, n_d [B,K] at the d line (rows
 *   behind a lens' own stop padded: c = 0, t = 0, n = 1); mask [B,K] (backward-ray test, :626-632); kappa [B,K],
 *   poly [B,K,TL_MAX_POLY], surf_kind [B,K] nullable (aspheric rows); z [B] pupil position; hfov [B] half field of view
 *   (rad), fields [F] relative field heights (cy = sin(hfov * field), :116-118); epd [B];
 *   x_scale, y_scale, y_offset [B,F,W] float outputs.
 */
int tl_ray_aim(int32_t device, int32_t B, int32_t F, int32_t W, int32_t K, const float *c, const float *t, const float *n,
               const float *n_d, const uint8_t *mask, const float *kappa, const float *poly, const uint8_t *surf_kind,
               const float *z, const float *hfov, const float *fields, const float *epd, int32_t allow_backward,
               float *x_scale, float *y_scale, float *y_offset, void *stream);

/*
 * Ray aiming, N iterations (RayTracer(n_ray_aiming_iter=N), any mode, with or without a vignetting function): tl_ray_aim's
 * arguments with n_iter, tee_ref and rs before the outputs, in one launch for any N.  Per (lens, field, wavelength):
 *   p0    the reference tee points (bottom y, top y, sagittal x) = tee_ref[b,f,0..2], default (-1, 1, 1); the meridional
 *         rays sit at pupil x = 0, the sagittal ray at y = (p0.bottom + p0.top) / 2 (apply_vignetting of the tee rays)
 *   rs    stop radius: rs[b] when given ('paraxial': magnification * epd / 2), else the on-axis d-line marginal ray
 *   step k = 1..N: trace the tee rays at p0 + s_{k-1} to the stop, error e = stop / rs - p0, s_k = s_{k-1} - e / J;
 *         J = d(xs_rel + ys_rel)/dp at k = 1 (the reference's; N = 1 is tl_ray_aim's result bit for bit), the stop
 *         coordinate's own partial (d xs/d xp sagittal, d ys/d yp meridional) at k >= 2.  A dead ray or a non-finite
 *         step: no step in that iteration.
 *   map   affine through (p0 -> p0 + s_N):  x_scale = (p0.x + s.x) / p0.x,
 *         y_scale = ((p0.u + s.u) - (p0.l + s.l)) / (p0.u - p0.l),  y_offset = (p0.l s.u - p0.u s.l) / (p0.l - p0.u)
 *   n_iter in 1..TL_MAX_AIM_ITER; tee_ref [B,F,3] float nullable; rs [B] float nullable.  TL_EINVAL (before any HIP call)
 *   for a bad argument.  One 16-lane group per (lens, field, wavelength): an iteration costs one trace of latency.
 */
int tl_ray_aim_iter(int32_t device, int32_t B, int32_t F, int32_t W, int32_t K, const float *c, const float *t, const float *n,
                    const float *n_d, const uint8_t *mask, const float *kappa, const float *poly, const uint8_t *surf_kind,
                    const float *z, const float *hfov, const float *fields, const float *epd, int32_t allow_backward,
                    int32_t n_iter, const float *tee_ref, const float *rs, float *x_scale, float *y_scale, float *y_offset,
                    void *stream);

/*
 * The aimed fan, [B,F,W,P] floats (consecutive pupil points contiguous), from one shared relative pupil grid xp, yp [P] and
 * tl_ray_aim's map:  x = clamp(xp x_scale, -2, 2) epd / 2,  y = clamp(yp y_scale + y_offset, -2, 2) epd / 2
 * (RayTracer.trace_rays, ray_tracing_lite.py:104-113: remap, torch.clamp(-2, 2), scale_to_epd) -- one launch for seven,
 * same rounding points.  x_scale, y_scale, y_offset [B,F,W]; epd [B].
 */
int tl_aim_fan(int32_t device, int32_t B, int32_t F, int32_t W, int32_t P, const float *xp, const float *yp,
               const float *x_scale, const float *y_scale, const float *y_offset, const float *epd, float *x_out, float *y_out,
               void *stream);

/*
 * Double precision -- RayTracer(double_precision=True) (ray_tracing_lite.py:82-84; the reference crashes there: Specs and
 * Lens have no .double()).  The same trace, forward and checkpoint backward, entirely in fp64: generic,
 * untuned kernels (one ray per lane, rolled loops) for reference-quality numbers on the GPU, not for speed.
 * `p` is a tl_problem whose float-typed pointers (x_in, y_in, z, cx, cy, c, t, mu, kappa, poly) POINT AT DOUBLES, same
 * shapes and strides (in elements); mask / surf_kind stay uint8; aggregate must be 0, n_index / asph_hits are ignored.
 * The blocks are read the same way: their float-typed members point at doubles (moments [B,F,TL_NMOM] as in tl_trace_fwd,
 * entry 8 = 0).  Members with no meaning here -- opd, stacks, g_opd, g_stacks, g_n_index -- must be NULL (TL_EINVAL): no
 * penalty term and no path length in double precision.  Workspace: tl_workspace_bytes_f64(p).
 */
size_t tl_workspace_bytes_f64(const tl_problem *p);
int tl_trace_fwd_f64(const tl_problem *p, const tl_rays *out, void *workspace, size_t workspace_bytes, void *stream);
int tl_trace_bwd_f64(const tl_problem *p, const tl_seeds *g, const tl_grads *out,
                     void *workspace, size_t workspace_bytes, void *stream);

/*
 * PSF soft histogram of a ray fan and its adjoint (the contraction inside compute_psf, ray_tracing.py:206-270; additive
 * entry points, ABI unchanged).  G grids (lens x field), W channels, R rays; ray r of (g, w) is element
 * g s_g + w s_w + r of x, y (and of weight / ok, gx / gy): rays contiguous, s_g and s_w element strides -- the tracer's
 * [B,F,W,P] outputs are taken as they are (s_g = W P, s_w = P).  Per grid, in pitch units
 *     u = x / x_pitch[g],   v = (y - y_centre[g]) / y_pitch[g],
 *     Gx_j = exp(-2 (u - (x_first + j))^2), j < nxh,    Gy_i = exp(-2 (v - (y_first + i))^2), i < ny
 * (a Gaussian of sigma = half a pixel at every pixel centre), and
 *     hist[g,w,i,j] = sum_r wt_r Gy_i(r) Gx_j(r)      the un-mirrored, un-normalised half kernel, float [G,W,ny,nxh].
 * wt_r = weight[r] (float, nullable), or ok[r] != 0 (the tracer's ray_ok bytes, nullable), or 1; not both (TL_EINVAL).  A ray
 * of weight 0 adds exactly 0, whatever its coordinates.
 * Forward: fp32 MFMA tiles in k-ordered FMA chains of <= 1024 rays, one fp32 partial per block in the workspace, summed in a
 * fixed order in fp64 and rounded once: the same bits on every run, no atomics.
 * Backward: g_hist [G,W,ny,nxh] -> gx, gy (strided like x, y; OVERWRITTEN; 0 for a ray of weight 0) = d/dx_r, d/dy_r, and,
 * each nullable, [G] floats reduced in a fixed order in fp64:
 *     g_x_pitch[g] = -sum_r gx_r x_r / x_pitch,  g_y_pitch[g] = -sum_r gy_r (y_r - y_centre) / y_pitch,  g_y_centre[g] = -sum_r gy_r,
 * so a grid sized from the data (pitch from the fan's extent, centre from its mean) differentiates through.  The weights carry
 * no gradient.
 * TL_EINVAL before any HIP call, with the function's name in the message: a required pointer NULL, nxh or ny outside 1..32,
 * G W > 65535, R < 1, weight and ok both given.  TL_EWORKSPACE: fewer bytes than tl_psf_workspace_bytes asks for (one size
 * serves both calls; 0 for arguments out of range).  No host synchronisation; caller-owned buffers; re-entrant.
 */
size_t tl_psf_workspace_bytes(int32_t G, int32_t W, int64_t R, int32_t nxh, int32_t ny);
int tl_psf_accumulate(int32_t device, int32_t G, int32_t W, int64_t R, const float *x, const float *y, const float *weight,
                      const uint8_t *ok, int64_t s_g, int64_t s_w, const float *x_pitch, const float *y_pitch,
                      const float *y_centre, int32_t nxh, int32_t ny, float x_first, float y_first, float *hist,
                      void *workspace, size_t workspace_bytes, void *stream);
int tl_psf_accumulate_bwd(int32_t device, int32_t G, int32_t W, int64_t R, const float *x, const float *y, const float *weight,
                          const uint8_t *ok, int64_t s_g, int64_t s_w, const float *x_pitch, const float *y_pitch,
                          const float *y_centre, int32_t nxh, int32_t ny, float x_first, float y_first, const float *g_hist,
                          float *gx, float *gy, float *g_x_pitch, float *g_y_pitch, float *g_y_centre, void *workspace,
                          size_t workspace_bytes, void *stream);

/*
 * The PSF soft histogram of K traced fans on G grids, each grid reading ONE fan rotated about the grid's centre: the PSF
 * grid over an image of a rotationally symmetric lens, where the PSF at azimuth phi is the histogram of the +y-meridian spot
 * rotated by phi (imaging.psf_grid_from_trace(fused=True); additive entry points, ABI unchanged).  x, y, weight, ok, gx, gy
 * are addressed as above with the SOURCE index: ray r of fan k, channel w is element k s_g + w s_w + r, k < K.  Per grid
 * g < G, with k = src[g] (device int32 [G], 0 <= src[g] < K) and c[g], s[g] (device floats [G], cos and sin of the angle):
 *     xi = x[k,w,r],   eta = y[k,w,r] - y_centre[k]                       y_centre is per SOURCE, [K]
 *     x' = fma(c, xi, s * eta),   y' = fma(c, eta, -(s * xi))             float32: one product, one fma each, as written
 *     u = x' / x_pitch[g],   v = y' / y_pitch[g]                          the pitches are per GRID, [G]
 *     hist[g,w,i,j] = sum_r wt_r Gy_i(v) Gx_j(u),   j < nx, i < ny        float [G,W,ny,nx], Gx, Gy as above
 * on the FULL grid: nothing is mirrored, x_first = 0.5 - nx/2 centres it as y_first = 0.5 - ny/2 does.  A ray of weight 0
 * (or ok 0) is dropped BEFORE the rotation: it adds exactly 0 whatever its coordinates, NaN included.  With c = 1, s = 0 and
 * src[g] = g the results have the bits of tl_psf_accumulate / _bwd on the same arguments (nxh = nx; the sign of a gradient
 * that underflowed to an exact zero aside: turning it back adds 0 gy' to it).
 * Forward: the scheme of tl_psf_accumulate (fp32 MFMA chains of 64 rays, fp64 totals, fixed-order partials): the same bits
 * on every run, no atomics.
 * Backward: g_hist [G,W,ny,nx] -> gx, gy [K,W,R] (strided like x, y; OVERWRITTEN) in SOURCE coordinates, the sum over the
 * grids that read the fan.  field_start [K+1], field_grids [G] (device int32) are the CSR inverse of src: the grids of fan k
 * are field_grids[field_start[k] .. field_start[k+1]), ascending.  One lane per source ray walks that list, rotates each
 * grid's (gx', gy') back, t_xi = fma(c, gx', -(s * gy')), t_eta = fma(c, gy', s * gx'), and adds the terms in list order (the
 * first is taken as it is): no atomics, the same bits on every run; a fan that no grid reads gets exactly +0.0.
 * g_y_centre [K] (nullable) = -sum_{w,r} gy, reduced in fp64 in a fixed order.  The pitches and the weights carry no gradient.
 * TL_EINVAL before any HIP call, with the function's name in the message: a required pointer NULL, nx or ny outside 1..32,
 * G, K or W < 1, G W or K W > 2^20 = 1048576 (the rows are folded over two grid axes inside: the 65535 of tl_psf_accumulate
 * does not bind), R < 1, G W R or K W R > 2^36, weight and ok both given.  NOT checked (it would need a host sync): the
 * entries of src, field_start and field_grids -- an entry out of range reads or writes out of bounds; the caller guarantees
 * 0 <= src[g] < K and that the CSR lists are the inverse of src.  TL_EWORKSPACE: fewer bytes than
 * tl_psf_rot_workspace_bytes asks for (one size serves both calls; 0 for arguments out of range).  No host synchronisation;
 * caller-owned buffers; re-entrant.
 */
size_t tl_psf_rot_workspace_bytes(int32_t G, int32_t K, int32_t W, int64_t R, int32_t nx, int32_t ny);
int tl_psf_rot_accumulate(int32_t device, int32_t G, int32_t K, int32_t W, int64_t R, const float *x, const float *y,
                          const float *weight, const uint8_t *ok, int64_t s_g, int64_t s_w, const int32_t *src, const float *c,
                          const float *s, const float *x_pitch, const float *y_pitch, const float *y_centre, int32_t nx,
                          int32_t ny, float x_first, float y_first, float *hist, void *workspace, size_t workspace_bytes,
                          void *stream);
int tl_psf_rot_accumulate_bwd(int32_t device, int32_t G, int32_t K, int32_t W, int64_t R, const float *x, const float *y,
                              const float *weight, const uint8_t *ok, int64_t s_g, int64_t s_w, const int32_t *src,
                              const float *c, const float *s, const float *x_pitch, const float *y_pitch,
                              const float *y_centre, int32_t nx, int32_t ny, float x_first, float y_first,
                              const int32_t *field_start, const int32_t *field_grids, const float *g_hist, float *gx, float *gy,
                              float *g_y_centre, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Spatially varying overlap-add PSF convolution of an image and its adjoints (imaging.svola_convolution(fused=True);
 * additive entry points, ABI unchanged).  The image [B,H,W,C] is cut into a gh x gw grid of overlapping patches of
 * ph = H/gh + 2 oh rows and pw = W/gw + 2 ow columns in the frame of Ih = H + 2 oh rows and Iw = W + 2 ow columns (the image
 * plus the overlap margin); patch n = i gw + j owns frame rows [r0[i], r1[i]) and columns [c0[j], c1[j]).  With P the image
 * extended by symmetric reflection (-1-i -> i, H+i -> H-1-i) and a = kh/2, b = kw/2,
 *     out[b,y,x,c] = sum_n w_n(y + oh, x + ow) sum_{i<kh, j<kw} psfs[b,n,i,j,c] P[b, y + a - i, x + b - j, c],
 *     w_n(r, q)    = wr[i][r] wc[j][q]
 * where wr [gh][Ih] and wc [gw][Iw] are DEVICE tables of doubles: the window of patch row i (column j) at frame row r
 * (column q), 0 outside the patch, already divided by the sum over the patches of that axis (the window is separable, so
 * the 2-D normalisation is the product of the two).  r0, r1, c0, c1 are HOST arrays of gh / gw ints, non-decreasing; every
 * row and column of the central H x W must lie inside a patch.  Element strides address image (b, y, x, c), psfs and g_psfs
 * (b, n, i, j, c); psf_batch is B or 1 (PSFs shared by the batch: g_psfs is then the sum over b).  out, g_out and g_image
 * are contiguous [B,H,W,C] floats.
 *   tl_svola_fwd        out.  One block per tile of <= 32 x 32 pixels that no patch edge crosses, so the covering patches
 *                       are block-uniform: the tile plus halo is staged in LDS with the reflection resolved in the index,
 *                       the taps come through the scalar cache.  No workspace.
 *   tl_svola_bwd_psf    g_psfs = d/d psfs of sum(g_out out).  Per-tile partials in the workspace, summed in a fixed order
 *                       in fp64 and rounded once: the same bits on every run, no atomics.
 *   tl_svola_bwd_image  g_image = d/d image: the correlation of w_n g_out with the PSFs on the extended frame (workspace),
 *                       then each pixel gathers its own value and those of its mirror images.  No atomics.
 * TL_EINVAL before any HIP call, with the function's name and the argument in the message: a required pointer NULL, kh or
 * kw even or > 31, oh + kh/2 > H or ow + kw/2 > W, gh or gw outside 1..128, psf_batch not 1 or B, patch bounds that are not
 * ph (pw) long, decreasing or outside the frame, an uncovered row or column.  TL_EWORKSPACE: fewer bytes than
 * tl_svola_workspace_bytes asks for (one size serves both backward calls; 0 for arguments out of range).  No host
 * synchronisation; caller-owned buffers; the launches go on `stream`.
 */
typedef struct tl_svola_geom {
    int32_t device;
    int32_t B, H, W, C;               /* image [B,H,W,C] */
    int32_t psf_batch;                /* B, or 1: PSFs shared by the batch */
    int32_t gh, gw, kh, kw, oh, ow;
    int64_t image_stride[4];          /* elements: b, y, x, c */
    int64_t psfs_stride[5];           /* elements: b, n, i, j, c */
    int64_t g_psfs_stride[5];         /* elements: b, n, i, j, c (tl_svola_bwd_psf) */
} tl_svola_geom;

size_t tl_svola_workspace_bytes(const tl_svola_geom *g, const int32_t *r0, const int32_t *r1, const int32_t *c0,
                                const int32_t *c1);
int tl_svola_fwd(const tl_svola_geom *g, const int32_t *r0, const int32_t *r1, const int32_t *c0, const int32_t *c1,
                 const double *wr, const double *wc, const float *image, const float *psfs, float *out, void *stream);
int tl_svola_bwd_psf(const tl_svola_geom *g, const int32_t *r0, const int32_t *r1, const int32_t *c0, const int32_t *c1,
                     const double *wr, const double *wc, const float *image, const float *g_out, float *g_psfs,
                     void *workspace, size_t workspace_bytes, void *stream);
int tl_svola_bwd_image(const tl_svola_geom *g, const int32_t *r0, const int32_t *r1, const int32_t *c0, const int32_t *c1,
                       const double *wr, const double *wc, const float *psfs, const float *g_out, float *g_image,
                       void *workspace, size_t workspace_bytes, void *stream);

/*
 * Bicubic resampling of an image at per-pixel source coordinates, with gradients to the coordinates and to a gain
 * (imaging.warp_bicubic(fused=True); additive entry points, ABI unchanged): distortion and relative illumination of a rendered
 * image.  image [B,H,W,C]; x, y [coord_batch,Ho,Wo], normalised source coordinates, -1 at the centre of the first column (row)
 * and +1 at the centre of the last; gain [gain_batch,Ho,Wo,gain_channels] or NULL (then gain_batch and gain_channels are not
 * read).  Per output pixel
 *     xc = clamp(x, -1, 1),  u = (xc + 1) / 2 (W - 1),  j0 = floor(u),  t = u - j0,
 *     columns j0 - 1, j0, j0 + 1, j0 + 2, each clipped into [0, W - 1] (replicate padding); rows likewise from y and H;
 *     w(-1) = a(t^3 - 2t^2 + t), w(0) = (a+2)t^3 - (a+3)t^2 + 1, w(1) = -(a+2)t^3 + (2a+3)t^2 - at, w(2) = a(t^2 - t^3), a = -0.75;
 *     out[b,yo,xo,c] = gain sum_i sum_j wy_i wx_j image[b, row_i, col_j, c].
 * Element strides address image and gain (b, y, x, c), x, y (b, y, x) and the gradient outputs, which have the shapes of x, y
 * and gain.  out and g_out are contiguous [B,Ho,Wo,C] floats.
 *   tl_warp_fwd   out.  One lane per output pixel, the channels looped in the lane; no LDS, no workspace.
 *   tl_warp_bwd   g_x, g_y = d/dx, d/dy of sum(g_out out) (both or neither: NULL for none) and g_gain (NULL for none; needs
 *                 gain), in one launch that recomputes the taps; the forward output is not needed.  d/dx is the derivative
 *                 weights times (W - 1)/2 where -1 <= x <= 1 and 0 outside; at an integer u it is taken in the cell with
 *                 t = 0 (the interpolant is C1, so both cells agree).  Whatever is shared (coord_batch or gain_batch 1 with
 *                 B > 1, gain_channels 1 with C > 1) receives the sum over what shares it, taken inside one lane in a fixed
 *                 order (b outer, c inner): no atomics, no workspace, the same bits on every run.
 * Only clipped integer indices form addresses, so no coordinate value can read outside the image; a NaN coordinate gives NaN
 * in that pixel's output and gradients and nowhere else.  The gradient to the image is tl_warp_bwd_image below.
 * TL_EINVAL before any HIP call, with the function's name and the argument in the message: a required pointer NULL, a size
 * below 1 (or H, W, Ho, Wo above 2^20), coord_batch or gain_batch neither 1 nor B, gain_channels neither 1 nor C.  C is not a
 * grid dimension and has no upper limit; B is cut into launches of 65535 lenses.  No host synchronisation, no allocation;
 * the launches go on `stream`.
 */
typedef struct tl_warp_geom {
    int32_t device;
    int32_t B, H, W, C;               /* image [B,H,W,C] */
    int32_t Ho, Wo;                   /* output [B,Ho,Wo,C] */
    int32_t coord_batch;              /* B, or 1: coordinates shared by the batch */
    int32_t gain_batch;               /* B, or 1: gain shared by the batch */
    int32_t gain_channels;            /* C, or 1: gain shared by the channels */
    int64_t image_stride[4];          /* elements: b, y, x, c */
    int64_t x_stride[3];              /* elements: b, y, x */
    int64_t y_stride[3];
    int64_t gain_stride[4];           /* elements: b, y, x, c */
    int64_t g_x_stride[3];            /* tl_warp_bwd */
    int64_t g_y_stride[3];
    int64_t g_gain_stride[4];
} tl_warp_geom;

int tl_warp_fwd(const tl_warp_geom *g, const float *image, const float *x, const float *y, const float *gain, float *out,
                void *stream);
int tl_warp_bwd(const tl_warp_geom *g, const float *image, const float *x, const float *y, const float *gain, const float *g_out,
                float *g_x, float *g_y, float *g_gain, void *stream);

/*
 * The gradient of sum(g_out out) to the image of tl_warp_fwd: a scatter,
 *     g_image[b,r,q,c] = sum over output pixels and taps (i,j) with (row_i, col_j) = (r,q) of wy_i wx_j a,
 *     a = g_out[b,yo,xo,c] gain[..] (gain 1 when NULL), taken as the fp32 product,
 * accumulated in 64-bit FIXED POINT with integer atomics, so the result has the same bits in any order or grouping of the
 * output pixels, under any launch plan and in every run.  The image is not read (the gradient is linear in it); only B, H, W,
 * C of it are used, image_stride and the g_*_stride members are not.  g_out and g_image are contiguous [B,Ho,Wo,C] and
 * [B,H,W,C] floats.  The contract:
 *   scale         m = the largest finite |a| of the whole call; E with 2^(E-1) <= m < 2^E; Hb = ceil(log2(16 Ho Wo)), in
 *                 integers; the quantum is Q = 2^(E + Hb - 62).  Ho Wo <= 2^26, so Hb <= 30 and Q <= 2^(E-32).
 *   contribution  the fp32 product (wy_i wx_j) a, times 1/Q in fp64 (exact), rounded to the nearest int64, added with an
 *                 integer atomic.  |wy wx| <= 1 and at most 16 Ho Wo <= 2^Hb contributions reach one address, so
 *                 |sum| <= 2^62: overflow is impossible by construction.
 *   result        fp32(sum Q), rounded once.  A source pixel that no tap reaches is +0.0; m = 0, or no finite a, gives zeros.
 *   non-finite    a non-finite a, or a NaN coordinate (whose taps are the clipped indices around j0 = 0, as in the forward),
 *                 is left out of m and of the sums and marks its destination elements instead: a marked element is NaN,
 *                 every other element keeps the bits of the clean run.
 *   error         per contribution at most Q/2, plus the fp32 roundings of weights and products and the one of the result:
 *                 ABSOLUTE on the scale of the largest seed (at least 2^-32 of m), not relative per pixel.
 *   consequences  scaling g_out by a power of two scales the result exactly (barring fp32 under- or overflow of the
 *                 products); the result does not depend on the launch plan or on `flags`.
 * A pre-pass finds m on the device (integer atomicMax on the bit pattern), the scatter kernel privatises a box of the source
 * image in LDS per tile of output pixels and flushes it with one atomic per touched entry, a last kernel converts.
 * `flags` bit 0: direct global atomics only, no LDS box (the A/B switch; the same bits).  `work`: the accumulators, the marks
 * and the m word, tl_warp_bwd_image_work_bytes(g) bytes (0 for a geometry that is refused), aligned to 8; it is cleared
 * inside the call and holds nothing afterwards.  No host synchronisation, no allocation; the launches go on `stream`.
 * TL_EINVAL before any HIP call as for tl_warp_bwd, and for Ho Wo > 2^26, B H W C > 2^40, unknown flag bits, and a
 * workspace that is NULL, misaligned or too small.
 */
size_t tl_warp_bwd_image_work_bytes(const tl_warp_geom *g);
int tl_warp_bwd_image(const tl_warp_geom *g, const float *x, const float *y, const float *gain, const float *g_out,
                      float *g_image, void *work, size_t work_bytes, int flags, void *stream);

/*
 * Structural similarity of two images per lens under a separable Gaussian window, and its gradients to both images
 * (imaging.ssim(fused=True); additive entry points, ABI unchanged).  a, b [B,H,W,C] floats, addressed through element strides
 * (b, y, x, c).  With w the K window weights (odd K, 3..11; the caller normalises them), the VALID window w (x) w, Hm = H - K + 1,
 * Wm = W - K + 1 and, per map pixel and channel,
 *     mu_a = w*a,  mu_b = w*b,  va = w*a^2 - mu_a^2,  vb = w*b^2 - mu_b^2,  cab = w*ab - mu_a mu_b,
 *     S = (2 mu_a mu_b + C1)(2 cab + C2) / ((mu_a^2 + mu_b^2 + C1)(va + vb + C2)),
 *     value[b] = the mean of S over Hm x Wm x C                                              value [B] floats, contiguous.
 * The gradient of sum_b g_value[b] value[b] to an image p (a or b; q is the other one) is
 *     g_p[b,y,x,c] = g_value[b] / (Hm Wm C) sum_{i,j} w_i w_j (dm + 2 p[b,y,x,c] ds + q[b,y,x,c] dc)[b, y - i, x - j, c]
 * over the map pixels that exist, with the partial maps  ds = dS/d va (= dS/d vb),  dc = dS/d cab,
 * dm_p = dS/d mu_p - 2 mu_p ds - mu_q dc (the derivative to the window mean with the raw second moments held fixed).
 * The maps are dense channels-last [B,Hm,Wm,C] floats of tl_ssim_maps_elems(g) elements each, stored unscaled: the
 * forward does not depend on g_value.
 *   tl_ssim_fwd   value, and the maps that `flags` asks for: bit 0 dm_a and ds_a, bit 1 dm_b and ds_b, dc with either bit; a
 *                 map that is not asked for may be NULL and is not written.  One workgroup per tile of 32 x 16 map pixels and
 *                 lens stages the tile plus halo of both images in LDS (whole row spans across the channels, in chunks of four
 *                 channels: C has no upper limit), runs the window along the rows and then down the columns over the five
 *                 products and writes ONE fp64 partial sum per (lens, tile) into `work`; a second kernel adds the tiles of a
 *                 lens in fp64 in a fixed order.  Before squaring, each tile subtracts its own first pixel (per image and
 *                 channel) and adds it back to the means: the variances are shift invariant, and the fp32 cancellation of
 *                 w*a^2 - mu_a^2 against C2 shrinks with the tile's contrast instead of its brightness.
 *   tl_ssim_bwd   g_p for ONE image, called once per image that needs a gradient with the roles set by the caller: p and q
 *                 are read through a_stride and b_stride, g_p is written through g_stride, (dm, ds) are the maps of p.  One
 *                 workgroup per tile of 32 x 16 image pixels gathers the three maps over the tile plus halo (zero outside the
 *                 map).  No workspace.
 * No atomics anywhere: both calls give the same bits on every run.  `work`: tl_ssim_work_bytes(g) bytes (0 for a geometry
 * that is refused), aligned to 8; it holds nothing afterwards.  C is not a grid dimension; B is cut into launches of 65535
 * lenses.  No host synchronisation, no allocation; the launches go on `stream`.
 * TL_EINVAL before any HIP call, with the function's name and the argument in the message: a required pointer NULL, a size
 * below 1, K even, below 3 or above 11, H or W below K or above 2^20 (or more than 2^22 tiles of 16 x 32 pixels in the
 * image), unknown flag bits, a map that the flags ask for but that is NULL, and a workspace that is NULL, misaligned or
 * too small.
 */
typedef struct tl_ssim_geom {
    int32_t device;
    int32_t B, H, W, C;               /* a, b [B,H,W,C] */
    int32_t K;                        /* window taps per axis: odd, 3..11 */
    float window[11];                 /* the first K are read */
    float C1, C2;                     /* (k1 L)^2, (k2 L)^2 */
    int32_t flags;                    /* tl_ssim_fwd: bit 0 the maps of a, bit 1 the maps of b are wanted */
    int64_t a_stride[4];              /* elements: b, y, x, c; of p in tl_ssim_bwd */
    int64_t b_stride[4];              /* of q in tl_ssim_bwd */
    int64_t g_stride[4];              /* of g_p (tl_ssim_bwd) */
} tl_ssim_geom;

size_t tl_ssim_work_bytes(const tl_ssim_geom *g);
size_t tl_ssim_maps_elems(const tl_ssim_geom *g);
int tl_ssim_fwd(const tl_ssim_geom *g, const float *a, const float *b, float *value, float *dm_a, float *ds_a, float *dm_b,
                float *ds_b, float *dc, void *work, size_t work_bytes, void *stream);
int tl_ssim_bwd(const tl_ssim_geom *g, const float *p, const float *q, const float *dm, const float *ds, const float *dc,
                const float *g_value, float *g_p, void *stream);

/*
 * Multi-scale structural similarity (what tf.image.ssim_multiscale computes) and its gradients to both images
 * (imaging.ms_ssim(fused=True); additive entry points, ABI unchanged).  a, b [B,H,W,C] floats through element strides, window,
 * K, C1, C2 as in tl_ssim_geom.  With M = levels (1..8) and p = power:
 *     level 0 is the images; level k + 1 is the 2 x 2 mean of level k with stride 2, ceil(H_k / 2) x ceil(W_k / 2), the last row
 *     or column of an odd side counted twice:  pooled[y', x'] = 1/4 sum_{dy,dx in {0,1}} img[min(2y' + dy, H_k - 1), min(2x' + dx, W_k - 1)]
 *     cs_k[b,c]   = mean over level k's valid map of (2 cab + C2) / (va + vb + C2),   ssim_k[b,c] = mean over the map of S
 *     v_k = cs_k for k < M - 1,  v_{M-1} = ssim_{M-1}                                  terms [B,C,M] floats, contiguous
 *     ms[b,c] = prod_k max(v_k, 0)^p_k,   value[b] = mean_c ms[b,c]                     value [B] floats, contiguous
 *     d ms / d v_k = p_k ms / v_k where every term of (b, c) is > 0, and exactly 0 for all k otherwise.
 *   tl_ms_ssim_fwd   one call for the whole pyramid: per level a pooling launch (both images at once; level 0 is read through the
 *                    caller's strides, the pooled levels are dense channels-last in `keep`) and the term forward -- tl_ssim_fwd's
 *                    kernel summing CS or S into one fp64 partial per (lens, tile, channel) -- and ONE finish launch that adds
 *                    the partials in a fixed order and forms terms, value and the factors d ms / d v_k in fp64.  `flags` bit 0 /
 *                    bit 1: keep the partial maps for the gradient to a / to b.
 *   tl_ms_ssim_bwd   g_p for ONE image (which = 0: p is a, 1: p is b; the caller swaps p, q and their strides as for tl_ssim_bwd;
 *                    `flags` as in the forward).  Per level from the coarsest to the finest tl_ssim_bwd's kernel with the seed
 *                    g_value[b] / C  d ms / d v_k / (Hm_k Wm_k) per channel, adding in its store the adjoint of the pooling of
 *                    the level above: 1/4 g_{k+1}[y / 2, x / 2], times 2 per axis on which the pixel is the doubled last one.
 * `keep`: tl_ms_ssim_keep_elems(g) floats, aligned to 8 bytes, written by the forward and read by the backward: B C M doubles
 * (the factors), the pooled levels of both images, and per level dm_a (bit 0), dm_b (bit 1), ds, dc (either bit) -- 4 bytes per
 * map element each.  `work`: tl_ms_ssim_work_bytes(g) bytes, aligned to 8; it holds nothing between the calls (the forward's tile
 * partials; the backward's gradients to the pooled levels).  Both planners give 0 for a geometry that is refused.
 * No atomics: the same bits on every run.  B is cut into launches of 65535 lenses inside the call; every launch goes on `stream`
 * back to back, no host synchronisation, no allocation.
 * TL_EINVAL before any HIP call, with the function's name and the argument in the message: a required pointer NULL, a size below
 * 1, K even, below 3 or above 11, levels outside 1..8, a level with a side below K (the message names the level and its size),
 * H or W above 2^20 (or H W C >= 2^31), unknown flag bits, `which` not 0 or 1 or naming an image whose maps the flags do not
 * keep, and keep or work NULL, misaligned or too small.
 */
typedef struct tl_ms_ssim_geom {
    int32_t device;
    int32_t B, H, W, C;               /* a, b [B,H,W,C] */
    int32_t K;                        /* window taps per axis: odd, 3..11 */
    float window[11];                 /* the first K are read */
    float C1, C2;                     /* (k1 L)^2, (k2 L)^2 */
    int32_t levels;                   /* M: 1..8 */
    float power[8];                   /* the first M are read */
    int32_t flags;                    /* bit 0 the maps of a, bit 1 the maps of b are kept */
    int64_t a_stride[4];              /* elements: b, y, x, c; of p in tl_ms_ssim_bwd */
    int64_t b_stride[4];              /* of q in tl_ms_ssim_bwd */
    int64_t g_stride[4];              /* of g_p (tl_ms_ssim_bwd) */
} tl_ms_ssim_geom;

size_t tl_ms_ssim_work_bytes(const tl_ms_ssim_geom *g);
size_t tl_ms_ssim_keep_elems(const tl_ms_ssim_geom *g);
int tl_ms_ssim_fwd(const tl_ms_ssim_geom *g, const float *a, const float *b, float *value, float *terms, float *keep,
                   size_t keep_elems, void *work, size_t work_bytes, void *stream);
int tl_ms_ssim_bwd(const tl_ms_ssim_geom *g, const float *p, const float *q, const float *keep, size_t keep_elems,
                   const float *g_value, float *g_p, int which, void *work, size_t work_bytes, void *stream);

/*
 * Through-focus spot moments (extension; metrics.focus_moments / metrics.through_focus stand on them).  Behind the last surface a
 * ray is a straight line: at a plane shifted by d along +z it lands at (x + d u, y + d v), u = cx / cz, v = cy / cz, so the mean
 * square radius of a spot is a parabola in d whose coefficients are second moments of (x, y, u, v).
 *
 * x, y, cx, cy (float) and ok (bytes) are [F, P, W] tensors that share ONE stride triple s_f, s_p, s_w (elements); a row is one
 * (f, w).  A ray is LIVE iff ok != 0 and s = 1 - cx^2 - cy^2 > 0; then cz = sqrt(s).  Per row
 *   moments[f, w, 0..10] = sum over live rays of (1, x, y, u, v, x^2, y^2, u^2, v^2, x u, y v)
 * with every product, quotient, root and sum in fp64 from the fp32 inputs.  A dead ray adds exactly 0 whatever its coordinates hold
 * (NaN, inf, cx^2 + cy^2 >= 1).  One partial per block goes to the workspace, a second kernel adds the partials of a row in a
 * fixed order: no atomics, the same bits on every run.  F W < 2^31 rows are taken (the grid's y dimension is cut into launches of
 * 65535 rows inside the call, all on `stream`, back to back), P < 2^31.  Where s_p = 1 and a row's five base addresses are aligned
 * (16 bytes the floats, 4 the flags) a lane takes four consecutive rays with 16-byte loads, otherwise one ray at a time.
 *
 * tl_focus_seed: d(sum g_moments . moments) / d(x, y, cx, cy), per ray in fp64, rounded once to float, written with the inputs'
 * strides into those of gx, gy, gcx, gcy that are not NULL (at least one):
 *   gx = g1 + 2 x g5 + u g9,   gy = g2 + 2 y g6 + v g10,   gu = g3 + 2 u g7 + x g9,   gv = g4 + 2 v g8 + y g10,
 *   gcx = (gu (1 - cy^2) + gv cx cy) / cz^3,   gcy = (gu cx cy + gv (1 - cx^2)) / cz^3;          a dead ray gets zeros.
 *
 * TL_EINVAL before any HIP call, with the function's name in the message: a required pointer NULL, F, P or W below 1, F W or P at
 * or above 2^31, every output of the seed NULL.  TL_EWORKSPACE: workspace NULL or below tl_focus_workspace_bytes(F, P, W) (0 for
 * sizes that are refused).
 */
size_t tl_focus_workspace_bytes(int64_t F, int64_t P, int64_t W);
int tl_focus_moments(int32_t device, int64_t F, int64_t P, int64_t W, const float *x, const float *y, const float *cx,
                     const float *cy, const uint8_t *ok, int64_t s_f, int64_t s_p, int64_t s_w, double *moments /* [F,W,11] */,
                     void *workspace, size_t workspace_bytes, void *stream);
int tl_focus_seed(int32_t device, int64_t F, int64_t P, int64_t W, const float *x, const float *y, const float *cx,
                  const float *cy, const uint8_t *ok, int64_t s_f, int64_t s_p, int64_t s_w, const double *g_moments /* [F,W,11] */,
                  float *gx, float *gy, float *gcx, float *gcy, void *stream);

/*
 * Encircled / ensquared energy of a traced fan (extension; metrics.enclosed_energy / metrics.spot_centroid stand on them): how
 * much of the light falls inside a circle of radius R, or inside a pixel of half side R, about a centre.
 *
 * x, y (float) and ok (bytes) are [F, P, W] tensors that share ONE stride triple s_f, s_p, s_w (elements); a row is one (f, w).
 * A ray is LIVE iff ok != 0; a dead ray adds exactly 0 to every sum and gets exactly 0 gradient whatever its coordinates hold
 * (NaN, inf, 1e30); live rays must be finite.  Per row, over the live rays,
 *   tl_enclosed_centroid   S[f, w] = (n, sum x, sum y)
 *   tl_enclosed_sums       sums[f, w, k] = sum e_k, with dx = x - centre[f, w, 0], dy = y - centre[f, w, 1],
 *       shape 0 (circle)   e_k = sigma((R_k - rho) inv_k),  rho = sqrt(dx^2 + dy^2)
 *       shape 1 (square)   e_k = sigma((R_k - |dx|) inv_k) sigma((R_k - |dy|) inv_k)                    (R_k is the half side)
 *   sigma(u) = 0 for u <= -1, 1 for u >= 1, else t^2 (3 - 2 t) with t = (u + 1) / 2; sigma'(u) = 3 t (1 - t) inside the band.
 * radii R_1 < ... < R_K (> 0) and inv_soft = 1 / softness (> 0) are HOST arrays of K <= 32 doubles: they travel to the kernels
 * as a by-value argument, nothing is uploaded and no call synchronises.  Every difference, product, root and sum is in fp64 from
 * the fp32 inputs, uncontracted; one partial per block goes to the workspace and a second kernel adds a row's partials in a fixed
 * order: no atomics, the same bits on every run.  Layout handling, launch plan and limits are tl_focus_moments' (16-byte loads
 * where s_p = 1 and the row's bases are aligned, one ray at a time elsewhere; F W < 2^31 rows in launches of 65535; P < 2^31).
 *
 * tl_enclosed_seed: d(sum g_sums . sums) / d(x, y) per ray in fp64, plus g_lin[f, w, 0..1] (the seeds of sum x, sum y; NULL = 0) on
 * live rays, rounded once to float and written with the inputs' strides into gx, gy (either may be NULL); dead rays get zeros.
 *   circle   d e_k / dx = -sigma'(u) inv_k dx / rho   (0 at rho = 0)
 *   square   d e_k / dx = -sigma'(u_x) sigma(u_y) inv_k sgn(dx)   (sgn(0) = 0),       y likewise.
 * g_centre[f, w, 0..1] (NULL = not wanted) = minus the row's sum of those edge terms (without g_lin), through partials and the
 * fixed-order reduce.
 *
 * TL_EINVAL before any HIP call, with the function's name in the message: a required pointer NULL, F, P or W below 1, F W or P at
 * or above 2^31, K outside 1..32, an unknown shape, a radius or softness not finite and positive, radii not strictly increasing,
 * every output of the seed NULL.  TL_EWORKSPACE: workspace NULL or below tl_enclosed_workspace_bytes(F, P, W, K) (0 for sizes
 * that are refused; tl_enclosed_centroid needs that of K = 1).
 */
size_t tl_enclosed_workspace_bytes(int64_t F, int64_t P, int64_t W, int K);
int tl_enclosed_centroid(int32_t device, int64_t F, int64_t P, int64_t W, const float *x, const float *y, const uint8_t *ok,
                         int64_t s_f, int64_t s_p, int64_t s_w, double *S /* [F,W,3] */, void *workspace, size_t workspace_bytes,
                         void *stream);
int tl_enclosed_sums(int32_t device, int64_t F, int64_t P, int64_t W, const float *x, const float *y, const uint8_t *ok,
                     int64_t s_f, int64_t s_p, int64_t s_w, const double *centre /* [F,W,2] */, const double *radii /* host, K */,
                     const double *inv_soft /* host, K */, int K, int shape, double *sums /* [F,W,K] */, void *workspace,
                     size_t workspace_bytes, void *stream);
int tl_enclosed_seed(int32_t device, int64_t F, int64_t P, int64_t W, const float *x, const float *y, const uint8_t *ok,
                     int64_t s_f, int64_t s_p, int64_t s_w, const double *centre /* [F,W,2] */, const double *radii /* host, K */,
                     const double *inv_soft /* host, K */, int K, int shape, const double *g_sums /* [F,W,K] */,
                     const double *g_lin /* [F,W,2] or NULL */, float *gx, float *gy, double *g_centre /* [F,W,2] or NULL */,
                     void *workspace, size_t workspace_bytes, void *stream);

/*
 * Zernike wavefront fit of a traced fan from its transverse ray errors (extension; metrics.zernike_moments / metrics.zernike_fit
 * stand on them).  The ray error (x, y) is the gradient of the wavefront over the pupil, so the coefficients a of the Noll-indexed
 * Zernike polynomials Z_2 .. Z_{J+1} (orthonormal over the unit disc, radial order <= `order` = N in 2 .. 6, J = (N+1)(N+2)/2 - 1;
 * p along x, q along y) solve, per row and over its live rays, the least-squares problem
 *   min_a  sum (x - sum_j a_j dZ_j/dp)^2 + (y - sum_j a_j dZ_j/dq)^2,     G a = b,  G_jk = sum grad Z_j . grad Z_k,
 *   b_j = sum x dZ_j/dp + y dZ_j/dq.
 *
 * x, y (float) and ok (bytes) are [F, P, W] tensors that share ONE stride triple s_f, s_p, s_w (elements); px, py (float), the
 * rays' pupil coordinates, share a triple of their own, ps_f, ps_p, ps_w (0, 1, 0 for one pupil shared by every row).  A row is one
 * (f, w); a ray is LIVE iff ok != 0; a dead ray adds exactly 0 to every sum and gets exactly 0 gradient whatever x, y, px, py hold.
 *
 * tl_zfit_moments: per row the K = 3 N^2 + 2 monomial sums, with tri(a, b) = (a + b)(a + b + 1) / 2 + b,
 *   moments[f, w, tri(a, b)]                        = sum p^a q^b          a + b <= 2N - 2          (N (2N - 1) of them; the first is n)
 *   moments[f, w, N(2N-1) + tri(a, b)]              = sum x p^a q^b        a + b <= N - 1
 *   moments[f, w, N(2N-1) + N(N+1)/2 + tri(a, b)]   = sum y p^a q^b        a + b <= N - 1
 *   moments[f, w, K - 2], moments[f, w, K - 1]      = sum x^2, sum y^2
 * in fp64 from the fp32 inputs, uncontracted: p^0 = 1, p^k = p^(k-1) p, a term is (p^a q^b) and then times x.  Layout handling,
 * launch plan, reduction and limits are tl_focus_moments' (16-byte loads where both ray strides are 1 and the row's bases are
 * aligned; one partial per block, a fixed-order reduce, no atomics; F W < 2^31 rows in launches of 65535; P < 2^31).
 *
 * tl_zfit_solve, the fit (moments not NULL): per row [rows = F W] the normal equations in the Zernike basis from the moments, scaled
 * by their diagonal D, G^ = D^-1/2 G D^-1/2, factorised by Cholesky in natural order.  A row is VALID iff 2n >= J (fewer equations than unknowns leave G singular), every D_jj > 0 and
 * every pivot (the value whose root is the factor's diagonal) exceeds 2^-30.  Writes a[row, J] (zeros for an invalid row),
 * q[row] = sum (x^2 + y^2) - b . a (0 for an invalid row), valid[row] and factor[row, J J + J] (the scaled factor and D^-1/2) for the adjoint.
 * tl_zfit_solve, the adjoint (moments NULL): from factor, a, valid and the adjoints g_a[row, J] of a and g_q[row] of
 * q = sum (x^2 + y^2) - b . a, b_bar = G^-1 g_a - 2 g_q a, written as coef[row, J + 1]: the coefficients of sum_j b_bar_j Z_j over
 * the monomials p^a q^b of degree 1 .. N at index tri(a, b) - 1, then 2 g_q; zeros for an invalid row.
 * tl_zfit_seed: gx = coef_J x + d/dp sum_m coef_m p^a q^b, gy likewise with y and d/dq, per ray in fp64 (Horner), rounded once to
 * float, written with the rays' strides into those of gx, gy that are not NULL; dead rays get zeros.
 * No call synchronises or uploads anything.
 *
 * TL_EINVAL before any HIP call, with the function's name in the message: a required pointer NULL, F, P, W or rows below 1, F W,
 * rows or P at or above 2^31, an order outside 2 .. 6, both outputs of the seed NULL.  TL_EWORKSPACE: workspace NULL or below
 * tl_zfit_workspace_bytes(F, P, W, order) (0 for arguments that are refused).
 */
size_t tl_zfit_workspace_bytes(int64_t F, int64_t P, int64_t W, int order);
int tl_zfit_moments(int32_t device, int64_t F, int64_t P, int64_t W, int order, const float *x, const float *y, const uint8_t *ok,
                    int64_t s_f, int64_t s_p, int64_t s_w, const float *px, const float *py, int64_t ps_f, int64_t ps_p,
                    int64_t ps_w, double *moments /* [F,W,K] */, void *workspace, size_t workspace_bytes, void *stream);
int tl_zfit_solve(int32_t device, int64_t rows, int order, const double *moments /* [rows,K] or NULL */,
                  const double *g_a /* [rows,J] */, const double *g_q /* [rows] */, double *a /* [rows,J] */, double *q /* [rows] */,
                  uint8_t *valid /* [rows] */, double *factor /* [rows,J J + J] */, double *coef /* [rows,J + 1] */, void *stream);
int tl_zfit_seed(int32_t device, int64_t F, int64_t P, int64_t W, int order, const float *x, const float *y, const uint8_t *ok,
                 int64_t s_f, int64_t s_p, int64_t s_w, const float *px, const float *py, int64_t ps_f, int64_t ps_p, int64_t ps_w,
                 const double *coef /* [F,W,J + 1] */, float *gx, float *gy, void *stream);

/*
 * Geometric OTF of a traced fan as Fourier sums over the spot (extension; metrics.otf_sums / metrics.geometric_mtf stand on them):
 * the characteristic function of the spot at J spatial-frequency vectors, exact for the traced rays at any frequency -- no
 * histogram, no bin width in the result.
 *
 * x, y (float) and ok (bytes) are [F, P, W] tensors that share ONE stride triple s_f, s_p, s_w (elements); a row is one (f, w).
 * A ray is LIVE iff ok != 0; a dead ray adds exactly 0 to every sum and gets exactly 0 gradient whatever its coordinates hold
 * (NaN, inf, 1e30): it is excluded by a select, not by a product with 0; live rays must be finite.  origin[f, w, 0..1] (device
 * doubles, contiguous) is a constant of the calculation: the modulus of the OTF does not depend on it, only the phase does, so it
 * gets no gradient; it exists for conditioning.  nu_x, nu_y are HOST arrays of J <= 16 doubles, cycles per length unit of x,
 * finite, of any sign, zero allowed: they travel to the kernels as a by-value argument, nothing is uploaded and no call
 * synchronises.  Per row, over the live rays, every operation in fp64 from the fp32 inputs, uncontracted:
 *   dx = (double)x - o_x,  dy = (double)y - o_y,  u = nu_x dx + nu_y dy  (two products, one sum: cycles),  r = u - rint(u)  (exact)
 *   sums[f, w, j, 0] = C_j = sum cos(2 pi r),   sums[f, w, j, 1] = S_j = sum sin(2 pi r)
 * through the device library's double-precision sincospi on 2 r (the factor 2 is exact, pi never multiplies in).  OTF_j = (C_j -
 * i S_j) / n, MTF_j = sqrt(C_j^2 + S_j^2) / n.  nu = 0 gives the term (1, 0) exactly: C = n, S = 0 without a rounding.  One partial
 * per block goes to the workspace and a second kernel adds a row's partials in a fixed order: no atomics, the same bits on every
 * run, and a column has the bits it has when it is computed alone.  Layout handling, launch plan and limits are
 * tl_enclosed_sums' (16-byte loads where s_p = 1 and the row's bases are aligned, one ray at a time elsewhere; F W < 2^31 rows in
 * launches of 65535; P < 2^31).
 *
 * tl_mtf_seed: for the seeds g_sums[f, w, j, 0..1] = (gC_j, gS_j), with phi = 2 pi r,  dC_j / dx = -2 pi nu_xj sin phi,  dS_j / dx =
 * 2 pi nu_xj cos phi:   q_j = gS_j cos phi_j - gC_j sin phi_j,   gx = 2 pi sum_j nu_xj q_j,   gy = 2 pi sum_j nu_yj q_j,
 * the sums over j in order in fp64, times 2 pi, rounded once to float and written with the inputs' strides into gx, gy (either
 * may be NULL, not both); dead rays get zeros.  It reduces nothing and leaves the workspace untouched; the workspace is checked
 * as for tl_mtf_sums so that one allocation serves both calls.
 *
 * TL_EINVAL before any HIP call, with the function's name in the message: a required pointer NULL, F, P or W below 1, F W or P at
 * or above 2^31, J outside 1..16, a frequency not finite, both outputs of the seed NULL.  TL_EWORKSPACE: workspace NULL or below
 * tl_mtf_workspace_bytes(F, P, W, J) (0 for arguments that are refused).
 */
size_t tl_mtf_workspace_bytes(int64_t F, int64_t P, int64_t W, int J);
int tl_mtf_sums(int32_t device, int64_t F, int64_t P, int64_t W, const float *x, const float *y, const uint8_t *ok, int64_t s_f,
                int64_t s_p, int64_t s_w, const double *origin /* [F,W,2] */, const double *nu_x /* host, J */,
                const double *nu_y /* host, J */, int J, double *sums /* [F,W,J,2] */, void *workspace, size_t workspace_bytes,
                void *stream);
int tl_mtf_seed(int32_t device, int64_t F, int64_t P, int64_t W, const float *x, const float *y, const uint8_t *ok, int64_t s_f,
                int64_t s_p, int64_t s_w, const double *origin /* [F,W,2] */, const double *nu_x /* host, J */,
                const double *nu_y /* host, J */, int J, const double *g_sums /* [F,W,J,2] */, float *gx, float *gy,
                void *workspace, size_t workspace_bytes, void *stream);

/*
 * Through-focus geometric OTF (extension; metrics.otf_sums_through_focus / metrics.through_focus_mtf stand on them): the Fourier
 * sums of tl_mtf_sums at Z equally spaced focal planes from ONE pass over the traced rays.  Behind the last surface a ray is a
 * line, so its phase at the plane shifted by d is a + d b, and over equally spaced planes exp(2 pi i (a + d_z b)) is a geometric
 * sequence: one term and one rotor per ray and frequency vector, then one complex multiplication per further plane.
 *
 * x, y, cx, cy (float) and ok (bytes) are [F, P, W] tensors that share ONE stride triple s_f, s_p, s_w (elements).  A ray is LIVE
 * iff ok != 0 and s = 1 - cx^2 - cy^2 > 0 (tl_focus_moments' rule, in fp64); a dead ray is excluded by a select: it adds +0.0 to
 * every sum and gets exactly 0 gradient whatever it holds.  origin[f, w, 0..1] (device doubles, contiguous) is a constant, as for
 * tl_mtf_sums.  nu_x, nu_y are HOST arrays of J <= 16 doubles; shift_first = d0 and shift_step = dd are host doubles and Z <= 16
 * the number of planes, plane z at d0 + z dd (Z = 1 ignores the step).  All of them travel by value in the kernel argument:
 * nothing is uploaded, no call synchronises.  Per row over the live rays, every operation in fp64 from the fp32 inputs, uncontracted:
 *   cz = sqrt(s),  u = cx / cz,  v = cy / cz,  dx = (double)x - o_x,  dy = (double)y - o_y
 *   a  = nu_x dx + nu_y dy  (cycles),   b = nu_x u + nu_y v  (cycles per unit of shift)
 *   p0 = a + d0 b,  r0 = p0 - rint(p0),  (c_0, s_0) = sincospi(2 r0)         plane 0
 *   q  = dd b,      rq = q - rint(q),    (cr, sr)   = sincospi(2 rq)         the rotor
 *   (c_z, s_z) = (c_{z-1} cr - s_{z-1} sr,  s_{z-1} cr + c_{z-1} sr),  z = 1 .. Z - 1
 *   sums[f, w, j, z, 0] = C_jz = sum c_z,   sums[f, w, j, z, 1] = S_jz = sum s_z;   OTF = (C - i S) / n,  MTF = sqrt(C^2 + S^2) / n.
 * nu = 0 gives a = b = 0 and the term (1, 0) at every plane exactly: C = n, S = 0 without a rounding.
 * BITS.  (i) A (vector, plane) column's bits depend only on the row's rays, its origin, nu_j, shift_first, shift_step and z: not
 * on J, Z, the register bucket of the launch or the other columns of the call.  (ii) With shift_first = 0 plane 0 has the bits of
 * tl_mtf_sums on the same x, y, ok and origin wherever the two live rules agree.  (iii) No atomics: the same bytes on every run,
 * whatever the buffers held before.  Layout handling, launch plan and limits are tl_mtf_sums'; a launch holds JB x ZB columns
 * in registers, the powers of two that hold J and Z with JB ZB <= 32; a call of more vectors goes in several launches back to
 * back, each reading the rays again.
 *
 * tl_tfmtf_seed: for the seeds g_sums[f, w, j, z, 0..1] = (gC, gS)_jz, with Q_jz = gS_jz c_z - gC_jz s_z:
 *   gx = 2 pi sum_j nu_xj sum_z Q_jz,   gu = 2 pi sum_j nu_xj sum_z (d0 + z dd) Q_jz,   gy, gv likewise with nu_y,
 *   gcx = (gu (1 - cy^2) + gv cx cy) / cz^3,   gcy = (gu cx cy + gv (1 - cx^2)) / cz^3,
 * the sums in fp64 in the order j, then z, rounded once to float and written with the inputs' strides into gx, gy, gcx, gcy (any
 * may be NULL, not all); dead rays get zeros.  It reduces nothing and leaves the workspace untouched; the workspace is checked as
 * for tl_tfmtf_sums so that one allocation serves both calls.
 *
 * TL_EINVAL before any HIP call, with the function's name in the message: a required pointer NULL, F, P or W below 1, F W or P at
 * or above 2^31, J or Z outside 1..16, a frequency or a shift not finite, all outputs of the seed NULL.  TL_EWORKSPACE: workspace
 * NULL or below tl_tfmtf_workspace_bytes(F, P, W, J, Z) (0 for arguments that are refused).
 */
size_t tl_tfmtf_workspace_bytes(int64_t F, int64_t P, int64_t W, int J, int Z);
int tl_tfmtf_sums(int32_t device, int64_t F, int64_t P, int64_t W, const float *x, const float *y, const float *cx, const float *cy,
                  const uint8_t *ok, int64_t s_f, int64_t s_p, int64_t s_w, const double *origin /* [F,W,2] */,
                  const double *nu_x /* host, J */, const double *nu_y /* host, J */, int J, double shift_first, double shift_step,
                  int Z, double *sums /* [F,W,J,Z,2] */, void *workspace, size_t workspace_bytes, void *stream);
int tl_tfmtf_seed(int32_t device, int64_t F, int64_t P, int64_t W, const float *x, const float *y, const float *cx, const float *cy,
                  const uint8_t *ok, int64_t s_f, int64_t s_p, int64_t s_w, const double *origin /* [F,W,2] */,
                  const double *nu_x /* host, J */, const double *nu_y /* host, J */, int J, double shift_first, double shift_step,
                  int Z, const double *g_sums /* [F,W,J,Z,2] */, float *gx, float *gy, float *gcx, float *gcy, void *workspace,
                  size_t workspace_bytes, void *stream);

/*
 * Diagnostic: quot[i] = a[i] / b[i] and root[i] = sqrt(b[i]) evaluated by the division and square root the trace kernels of
 * `mode` use.  Strict mode promises the correctly rounded (IEEE) results on the operand ranges of the trace, from shorter
 * instruction sequences than the compiler's general ones: tests/test_gpu_arith.py holds it to that, bit for bit.
 */
int tl_selftest_arith(int32_t device, int32_t mode, const float *a, const float *b, int64_t n, float *quot, float *root,
                      void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TL_TRACE_H */
