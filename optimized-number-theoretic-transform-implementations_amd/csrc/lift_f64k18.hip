/* lift_f64k18.hip -- instantiates the fused lift kernels (lift_fwd_kernel, N = 2^6..2^14) for (ArithF64, headroom class 18). */
#include "ntt_kernels_lift.h"

namespace ntt {
NTT_DEFINE_LAUNCH_LIFT_FWD(ArithF64, 18)
} /* namespace ntt */
