/* lift_f64w.hip -- instantiates the fused lift kernels (lift_fwd_kernel, N = 2^6..2^14) for (ArithF64W). */
#include "ntt_kernels_lift.h"

namespace ntt {
NTT_DEFINE_LAUNCH_LIFT_FWD(ArithF64W, 0)
} /* namespace ntt */
