/* rescale_f64k1.hip -- instantiates the NTT-domain rescale kernels (rescale_fwd_kernel, N = 2^6..2^14) for (ArithF64, headroom class 1). */
#include "ntt_kernels_rescale.h"

namespace ntt {
NTT_DEFINE_LAUNCH_RESCALE_FWD(ArithF64, 1)
} /* namespace ntt */
