/*
 * ntt_kernels_bgv.h -- moddown_bgv_fwd_kernel: the NTT-domain BGV ModDown (ntt_rns_mod_down_bgv_batch in place,
 * ntt_rns_mod_down_bgv_add_batch into a ciphertext) for a run of Q limbs in ONE launch.  Included by the ksbgv_f64*.hip units only (the
 * host layer sees the launchers of ntt_bgv.h, which states the arithmetic).
 *
 * The BGV variant of moddown_fwd_body (ntt_kernels_moddown.h): ksfold_fwd_kernel with the prologue's constants changed.  Per block of
 * Q limb l:
 *   tables    np > 1: bconv_ghat's [p^_j]_{q_l}, each entry multiplied by [T]_{q_l} by the thread that formed it (one Shoup product per
 *             P prime and workgroup); the offset arrives as [T h]_{q_l} from the host;
 *   prologue  u_l = [T]_{q_l} (F_l - [h]_{q_l}) = [T F_l]_{q_l} - [T h]_{q_l}: bconv_tile over the scaled table and moddown_digit -- word for
 *             word ksfold_fwd_kernel's work; np = 1: bgv_digit1 (no table, no 128-bit sum; the source product stays, one more Shoup
 *             product per word for [T]_{q_l});
 *   epilogue  ksfold_fwd_kernel's: c^ read from the accumulator, (c^ - x) P^-1 with the limb's FP64 constants, the optional addend, the
 *             store to `out`.  The in-place form passes out = the accumulator's own Q limbs (the body's note on the quarter-tile's
 *             read-before-store order).
 */
#pragma once
#include "ntt_kernels_moddown.h"

namespace ntt {

template <class A> struct KModDownBgv {
  KArgs<A>        k;   /* k.a = the run's first Q limb of the accumulator (c^), its strides, the run's limb records */
  const uint64_t *t;   /* the first P limb's coefficients; P limb j at t + j * k.limb_stride */
  uint64_t *      out; /* the run's first limb of the destination (the ciphertext, or the accumulator itself) */
  uint64_t        out_limb_stride, out_poly_stride;
  int             np, accumulate;
  BconvSrc        pl[kBconvLimbs]; /* h = [h T]_{p_j}, inv = [T^-1 p^_j^-1]_{p_j} */
  BconvDst        ql[kBconvLimbs]; /* s = [P^-1]_q, h = [T h]_q                  */
  BgvScale        ts[kBconvLimbs]; /* [T]_q                                       */
};

template <class A, int LOGN, int KSH>
__global__ void __launch_bounds__((Geom<LOGN, false, flavor_of<A>()>::WG), (Geom<LOGN, false, flavor_of<A>()>::WPS))
  moddown_bgv_fwd_kernel(const KModDownBgv<A> kr)
{
  moddown_fwd_body<A, LOGN, KSH, kModDownBgv>(kr);
}

template <class A, int LOGN, int KSH> hipError_t launch_moddown_bgv_fwd_n(const ModDownBgvArgs &ba)
{
  return launch_moddown_variant_n<A, LOGN, KModDownBgv<A>, moddown_bgv_fwd_kernel<A, LOGN, KSH>>(ba.k.m, [&](KModDownBgv<A> &kr) {
    for(int l = 0; l < ba.k.m.nlimbs; l++) kr.ts[l] = ba.ts[l];
    moddown_fold_out(kr, ba.k);
  });
}

#define NTT_DEFINE_LAUNCH_MODDOWN_BGV_FWD(A, KSH)                                                                                                  \
  template <> hipError_t launch_moddown_bgv_fwd<A, KSH>(const ModDownBgvArgs &ba)                                                                  \
  {                                                                                                                                                \
    return with_int<6, 14>((int)ba.k.m.logn, hipErrorNotSupported, [&](auto ln) { return launch_moddown_bgv_fwd_n<A, decltype(ln)::value, KSH>(ba); }); \
  }

} // namespace ntt
