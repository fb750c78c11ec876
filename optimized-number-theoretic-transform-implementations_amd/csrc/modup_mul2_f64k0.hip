/* modup_mul2_f64k0.hip -- instantiates the pair form of the ModUp-times-key kernels (modup_mul2_kernel: ntt_kernels_modup_mul.h's body with two components, N = 2^6..2^14) for (ArithF64, headroom class 0). */
#include "ntt_kernels_modup_mul.h"

namespace ntt {
NTT_DEFINE_LAUNCH_MODUP_MUL(ArithF64, 0, 2)
} /* namespace ntt */
