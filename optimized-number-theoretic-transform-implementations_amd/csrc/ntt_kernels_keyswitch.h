/*
 * ntt_kernels_keyswitch.h -- moddown_fwd_kernel: the NTT-domain RNS ModDown (divide by the product P of the special primes, drop
 * the P limbs) for a run of Q limbs in ONE launch.  Included by the keyswitch_f64*.hip units only (the host layer sees the
 * launchers of ntt_keyswitch.h).
 *
 * The in-place variant of moddown_fwd_body (ntt_kernels_moddown.h).  Per block of Q limb l:
 *   prologue  u_l = FastBConv_{P->q_l}([t + h]_P) - [h]_{q_l} (ntt_keyswitch.h); with np = 1 the rescale's (moddown_digit1);
 *   epilogue  (c^ - x) * P^-1, stored over c^.
 * 8N np bytes of t and 16N of c^ per limb-polynomial.
 */
#pragma once
#include "ntt_kernels_moddown.h"

namespace ntt {

template <class A> struct KModDown {
  KArgs<A>        k;  /* k.a = the run's first Q limb (c^), limb_stride / poly_stride of the operand, the run's limb records */
  const uint64_t *t;  /* the first P limb's coefficients; P limb j at t + j * k.limb_stride */
  int             np;
  BconvSrc        pl[kBconvLimbs];
  BconvDst        ql[kBconvLimbs];
};

template <class A, int LOGN, int KSH>
__global__ void __launch_bounds__((Geom<LOGN, false, flavor_of<A>()>::WG), (Geom<LOGN, false, flavor_of<A>()>::WPS))
  moddown_fwd_kernel(const KModDown<A> kr)
{
  moddown_fwd_body<A, LOGN, KSH, kModDownInPlace>(kr);
}

template <class A, int LOGN, int KSH> hipError_t launch_moddown_fwd_n(const ModDownFwdArgs &ma)
{
  return launch_moddown_variant_n<A, LOGN, KModDown<A>, moddown_fwd_kernel<A, LOGN, KSH>>(ma, [](KModDown<A> &) {});
}

#define NTT_DEFINE_LAUNCH_MODDOWN_FWD(A, KSH)                                                                                                   \
  template <> hipError_t launch_moddown_fwd<A, KSH>(const ModDownFwdArgs &ma)                                                                   \
  {                                                                                                                                             \
    return with_int<6, 14>((int)ma.logn, hipErrorNotSupported, [&](auto ln) { return launch_moddown_fwd_n<A, decltype(ln)::value, KSH>(ma); }); \
  }

} // namespace ntt
