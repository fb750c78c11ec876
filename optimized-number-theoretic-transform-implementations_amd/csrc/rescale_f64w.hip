/* rescale_f64w.hip -- instantiates the NTT-domain rescale kernels (rescale_fwd_kernel, N = 2^6..2^14) for ArithF64W (moduli up to 2^52). */
#include "ntt_kernels_rescale.h"

namespace ntt {
NTT_DEFINE_LAUNCH_RESCALE_FWD(ArithF64W, 0)
} /* namespace ntt */
