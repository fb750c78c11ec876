/* sample_f64k1.hip -- instantiates the fused sampling kernels (sample_fwd_kernel, N = 2^6..2^14) for (ArithF64, headroom class 1). */
#include "ntt_kernels_sample.h"

namespace ntt {
NTT_DEFINE_LAUNCH_SAMPLE_FWD(ArithF64, 1)
} /* namespace ntt */
