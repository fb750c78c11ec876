/* slots_f64k1.hip -- instantiates the fused slot kernels (slots_inv_kernel, slots_fwd_kernel, N = 2^6..2^14) for (ArithF64, headroom class 1). */
#include "ntt_kernels_slots.h"

namespace ntt {
NTT_DEFINE_LAUNCH_SLOTS(ArithF64, 1)
} /* namespace ntt */
