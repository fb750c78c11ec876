/* modup_mul_f64k18.hip -- instantiates the ModUp-times-key kernels (modup_mul_kernel, N = 2^6..2^14) for (ArithF64, headroom class 18). */
#include "ntt_kernels_modup_mul.h"

namespace ntt {
NTT_DEFINE_LAUNCH_MODUP_MUL(ArithF64, 18, 1)
} /* namespace ntt */
