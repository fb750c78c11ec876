/* ksfold_f64w.hip -- instantiates the ModDown-into-a-ciphertext kernels (ksfold_fwd_kernel, N = 2^6..2^14) for (ArithF64W: moduli up to 2^52). */
#include "ntt_kernels_ksfold.h"

namespace ntt {
NTT_DEFINE_LAUNCH_KSFOLD_FWD(ArithF64W, 0)
} /* namespace ntt */
