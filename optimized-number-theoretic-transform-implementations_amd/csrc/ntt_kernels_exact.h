/*
 * ntt_kernels_exact.h -- moddown_exact_fwd_kernel: the NTT-domain EXACT scaled ModDown (ntt_rns_mod_down_exact_batch) for a run of Q
 * limbs in ONE launch.  Included by the ksexact_f64*.hip units only (the host layer sees the launchers of ntt_exact.h).
 *
 * The exact variant of moddown_fwd_body (ntt_kernels_moddown.h): moddown_fwd_kernel with two changes.  Per block of Q limb l:
 *   prologue  u_l = ExactBConv_{P->q_l}([m t]_P): bconv_tile with the FP64 sum of fl(z_j) rho_j beside the 128-bit sum of every word
 *             (bconv_tile_exact), v = rint of it into the sum before the one Barrett reduction (ntt_exact.h);
 *   epilogue  (c^ [m]_q - x) * P^-1 with the limb's FP64 constants -- c^ [m P^-1] - x [P^-1] with the common factor taken out, one
 *             product more than moddown_fwd_kernel.
 * 8N np bytes of t and 16N of c^ per limb-polynomial.  One P prime takes the general path ([p^_0]_q = 1).  v depends on the P words
 * alone and is formed by ntt_exact.h's operations in ntt_exact.h's order: every workgroup, whichever limb it serves, and the
 * coefficient kernel of the sandwich route arrive at the same v.
 */
#pragma once
#include "ntt_kernels_moddown.h"

namespace ntt {

template <class A> struct KModDownExactFwd {
  KArgs<A>        k;  /* k.a = the run's first Q limb (c^), limb_stride / poly_stride of the operand, the run's limb records */
  const uint64_t *t;  /* the first P limb's coefficients; P limb j at t + j * k.limb_stride */
  int             np;
  BconvSrc        pl[kBconvLimbs];  /* inv = [m p^_j^-1]_{p_j}, h = 0 */
  BconvDst        ql[kBconvLimbs];  /* s = [P^-1]_q, h = q - [P]_q   */
  double          rho[kBconvLimbs]; /* 1.0 / (double)p_j              */
  uint64_t        mq[kBconvLimbs];  /* [m]_{q_l}                      */
};

template <class A, int LOGN, int KSH>
__global__ void __launch_bounds__((Geom<LOGN, false, flavor_of<A>()>::WG), (Geom<LOGN, false, flavor_of<A>()>::WPS))
  moddown_exact_fwd_kernel(const KModDownExactFwd<A> kr)
{
  moddown_fwd_body<A, LOGN, KSH, kModDownExact>(kr);
}

template <class A, int LOGN, int KSH> hipError_t launch_moddown_exact_fwd_n(const ModDownExactFwdArgs &xa)
{
  return launch_moddown_variant_n<A, LOGN, KModDownExactFwd<A>, moddown_exact_fwd_kernel<A, LOGN, KSH>>(xa.ma, [&](KModDownExactFwd<A> &kr) {
    for(int l = 0; l < xa.ma.nlimbs; l++) kr.mq[l] = xa.mq[l];
    for(int j = 0; j < xa.ma.np; j++) kr.rho[j] = xa.rho[j];
  });
}

#define NTT_DEFINE_LAUNCH_MODDOWN_EXACT_FWD(A, KSH)                                                                                                   \
  template <> hipError_t launch_moddown_exact_fwd<A, KSH>(const ModDownExactFwdArgs &xa)                                                              \
  {                                                                                                                                                   \
    return with_int<6, 14>((int)xa.ma.logn, hipErrorNotSupported, [&](auto ln) { return launch_moddown_exact_fwd_n<A, decltype(ln)::value, KSH>(xa); }); \
  }

} // namespace ntt
