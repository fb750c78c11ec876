/* slots_f64w.hip -- instantiates the fused slot kernels (slots_inv_kernel, slots_fwd_kernel, N = 2^6..2^14) for ArithF64W (moduli up to 2^52). */
#include "ntt_kernels_slots.h"

namespace ntt {
NTT_DEFINE_LAUNCH_SLOTS(ArithF64W, 0)
} /* namespace ntt */
