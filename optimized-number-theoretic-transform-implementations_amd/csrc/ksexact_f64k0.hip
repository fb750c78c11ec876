/* ksexact_f64k0.hip -- instantiates the NTT-domain exact scaled ModDown kernels (moddown_exact_fwd_kernel, N = 2^6..2^14) for (ArithF64, headroom class 0). */
#include "ntt_kernels_exact.h"

namespace ntt {
NTT_DEFINE_LAUNCH_MODDOWN_EXACT_FWD(ArithF64, 0)
} /* namespace ntt */
