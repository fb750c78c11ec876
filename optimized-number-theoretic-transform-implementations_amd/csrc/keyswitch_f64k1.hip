/* keyswitch_f64k1.hip -- instantiates the NTT-domain ModDown kernels (moddown_fwd_kernel, N = 2^6..2^14) for (ArithF64, headroom class 1). */
#include "ntt_kernels_keyswitch.h"

namespace ntt {
NTT_DEFINE_LAUNCH_MODDOWN_FWD(ArithF64, 1)
} /* namespace ntt */
