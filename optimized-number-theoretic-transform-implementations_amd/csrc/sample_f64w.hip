/* sample_f64w.hip -- instantiates the fused sampling kernels (sample_fwd_kernel, N = 2^6..2^14) for (ArithF64W: q up to 2^52). */
#include "ntt_kernels_sample.h"

namespace ntt {
NTT_DEFINE_LAUNCH_SAMPLE_FWD(ArithF64W, 0)
} /* namespace ntt */
