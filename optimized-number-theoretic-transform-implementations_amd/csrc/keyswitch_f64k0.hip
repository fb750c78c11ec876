/* keyswitch_f64k0.hip -- instantiates the NTT-domain ModDown kernels (moddown_fwd_kernel, N = 2^6..2^14) for (ArithF64, headroom class 0). */
#include "ntt_kernels_keyswitch.h"

namespace ntt {
NTT_DEFINE_LAUNCH_MODDOWN_FWD(ArithF64, 0)
} /* namespace ntt */
