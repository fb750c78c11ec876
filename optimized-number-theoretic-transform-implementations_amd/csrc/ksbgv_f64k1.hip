/* ksbgv_f64k1.hip -- instantiates the BGV ModDown kernels (moddown_bgv_fwd_kernel, N = 2^6..2^14) for (ArithF64, headroom class 1). */
#include "ntt_kernels_bgv.h"

namespace ntt {
NTT_DEFINE_LAUNCH_MODDOWN_BGV_FWD(ArithF64, 1)
} /* namespace ntt */
