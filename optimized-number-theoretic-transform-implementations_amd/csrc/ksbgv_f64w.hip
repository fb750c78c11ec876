/* ksbgv_f64w.hip -- instantiates the BGV ModDown kernels (moddown_bgv_fwd_kernel, N = 2^6..2^14) for (ArithF64W, 52-bit moduli). */
#include "ntt_kernels_bgv.h"

namespace ntt {
NTT_DEFINE_LAUNCH_MODDOWN_BGV_FWD(ArithF64W, 0)
} /* namespace ntt */
