// Strict arithmetic mode: build this TU with -ffp-contract=off (no FMA contraction) and the
// HIP default correctly-rounded fp32 sqrt/divide, so the forward is operation-for-operation
// the reference's eager fp32 graph (ray_tracing_lite.py:525-571, 594-675).
#include "tl_common.h"
#define TL_NS tl_strict_impl
#define TL_API_NS tl_strict
#define TL_FAST 0
#include "tl_kernels.inc"
