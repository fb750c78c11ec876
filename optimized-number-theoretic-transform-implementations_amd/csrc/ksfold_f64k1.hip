/* ksfold_f64k1.hip -- instantiates the ModDown-into-a-ciphertext kernels (ksfold_fwd_kernel, N = 2^6..2^14) for (ArithF64, headroom class 1). */
#include "ntt_kernels_ksfold.h"

namespace ntt {
NTT_DEFINE_LAUNCH_KSFOLD_FWD(ArithF64, 1)
} /* namespace ntt */
