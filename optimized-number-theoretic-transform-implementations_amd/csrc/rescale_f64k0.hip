/* rescale_f64k0.hip -- instantiates the NTT-domain rescale kernels (rescale_fwd_kernel, N = 2^6..2^14) for (ArithF64, headroom class 0). */
#include "ntt_kernels_rescale.h"

namespace ntt {
NTT_DEFINE_LAUNCH_RESCALE_FWD(ArithF64, 0)
} /* namespace ntt */
