/* modup_mul_f64w.hip -- instantiates the ModUp-times-key kernels (modup_mul_kernel, N = 2^6..2^14) for (ArithF64W, headroom class 0). */
#include "ntt_kernels_modup_mul.h"

namespace ntt {
NTT_DEFINE_LAUNCH_MODUP_MUL(ArithF64W, 0, 1)
} /* namespace ntt */
