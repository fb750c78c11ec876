/* ksfold_f64k18.hip -- instantiates the ModDown-into-a-ciphertext kernels (ksfold_fwd_kernel, N = 2^6..2^14) for (ArithF64, headroom class 18). */
#include "ntt_kernels_ksfold.h"

namespace ntt {
NTT_DEFINE_LAUNCH_KSFOLD_FWD(ArithF64, 18)
} /* namespace ntt */
