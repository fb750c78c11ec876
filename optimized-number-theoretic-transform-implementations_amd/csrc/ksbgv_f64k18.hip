/* ksbgv_f64k18.hip -- instantiates the BGV ModDown kernels (moddown_bgv_fwd_kernel, N = 2^6..2^14) for (ArithF64, headroom class 18). */
#include "ntt_kernels_bgv.h"

namespace ntt {
NTT_DEFINE_LAUNCH_MODDOWN_BGV_FWD(ArithF64, 18)
} /* namespace ntt */
