/* keyswitch_f64w.hip -- instantiates the NTT-domain ModDown kernels (moddown_fwd_kernel, N = 2^6..2^14) for (ArithF64W, the wide policy for 2^51 < q < 2^52). */
#include "ntt_kernels_keyswitch.h"

namespace ntt {
NTT_DEFINE_LAUNCH_MODDOWN_FWD(ArithF64W, 0)
} /* namespace ntt */
