// Fast arithmetic mode: build this TU with -ffp-contract=fast; sqrt / divide use the
// hardware v_sqrt_f32 / v_rcp_f32 (1 ulp).  Same algorithm, a few ulp from strict.
#include "tl_common.h"
#define TL_NS tl_fast_impl
#define TL_API_NS tl_fast
#define TL_FAST 1
#include "tl_kernels.inc"
