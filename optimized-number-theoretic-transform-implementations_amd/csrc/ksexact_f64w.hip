/* ksexact_f64w.hip -- instantiates the NTT-domain exact scaled ModDown kernels (moddown_exact_fwd_kernel, N = 2^6..2^14) for the 52-bit policy (ArithF64W). */
#include "ntt_kernels_exact.h"

namespace ntt {
NTT_DEFINE_LAUNCH_MODDOWN_EXACT_FWD(ArithF64W, 0)
} /* namespace ntt */
