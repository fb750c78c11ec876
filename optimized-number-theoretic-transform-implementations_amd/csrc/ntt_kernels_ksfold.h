/*
 * ntt_kernels_ksfold.h -- ksfold_fwd_kernel: the NTT-domain RNS ModDown of an accumulator over Q u P WRITTEN INTO (or added to) a
 * ciphertext over Q, for a run of Q limbs in ONE launch: the last step of a relinearisation ((d0, d1) += ModDown(acc0, acc1)) and of a
 * rotation (c1' = ModDown(acc1)).  Included by the ksfold_f64*.hip units only (the host layer sees the launchers of ntt_ct_mul.h).
 *
 * The fold variant of moddown_fwd_body (ntt_kernels_moddown.h): moddown_fwd_kernel's prologue and stages, another epilogue.  Per block
 * of Q limb l:
 *   epilogue  a quarter-tile at a time: c^ read from the ACCUMULATOR in the last group's layout, r = (c^ - x) * P^-1 with the limb's
 *             FP64 constants, canonical after mul_store; when accumulating, the ciphertext's word e is read beside it and r + e gets one
 *             conditional subtraction in integer arithmetic (both canonical: r + e < 2q < 2^53, exact); the result is stored to the
 *             CIPHERTEXT, whose limb and polynomial strides are its own.  The accumulator's Q limbs are not written.
 * 8N np bytes of t, 8N of c^, 8N stored and, when accumulating, 8N of the addend per limb-polynomial.
 */
#pragma once
#include "ntt_kernels_moddown.h"

namespace ntt {

template <class A> struct KKsFold {
  KArgs<A>        k;  /* k.a = the run's first Q limb of the accumulator (c^, read only), its strides, the run's limb records */
  const uint64_t *t;  /* the first P limb's coefficients; P limb j at t + j * k.limb_stride */
  uint64_t *      out; /* the run's first limb of the ciphertext */
  uint64_t        out_limb_stride, out_poly_stride;
  int             np, accumulate;
  BconvSrc        pl[kBconvLimbs];
  BconvDst        ql[kBconvLimbs];
};

template <class A, int LOGN, int KSH>
__global__ void __launch_bounds__((Geom<LOGN, false, flavor_of<A>()>::WG), (Geom<LOGN, false, flavor_of<A>()>::WPS))
  ksfold_fwd_kernel(const KKsFold<A> kr)
{
  moddown_fwd_body<A, LOGN, KSH, kModDownFold>(kr);
}

template <class A, int LOGN, int KSH> hipError_t launch_ksfold_fwd_n(const KsFoldArgs &ka)
{
  return launch_moddown_variant_n<A, LOGN, KKsFold<A>, ksfold_fwd_kernel<A, LOGN, KSH>>(ka.m, [&](KKsFold<A> &kr) { moddown_fold_out(kr, ka); });
}

#define NTT_DEFINE_LAUNCH_KSFOLD_FWD(A, KSH)                                                                                                  \
  template <> hipError_t launch_ksfold_fwd<A, KSH>(const KsFoldArgs &ka)                                                                      \
  {                                                                                                                                           \
    return with_int<6, 14>((int)ka.m.logn, hipErrorNotSupported, [&](auto ln) { return launch_ksfold_fwd_n<A, decltype(ln)::value, KSH>(ka); }); \
  }

} // namespace ntt
