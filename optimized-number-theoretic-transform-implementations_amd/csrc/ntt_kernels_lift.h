/*
 * ntt_kernels_lift.h -- lift_fwd_kernel: the lift of a plaintext into the RNS fused with the forward transform (NTT_LIFT_TRANSFORMED)
 * for a run of limbs in ONE launch.  Included by the lift_f64*.hip units only (the host layer sees the launchers of ntt_lift.h).
 *
 * produce_fwd_body (ntt_kernels_produce.h) with the lift's digit: the plaintext's block as raw words -- a word mod t up to 2^61, or the
 * bit pattern of a double -- is turned into the limb's canonical word in integer arithmetic (lift_word, lift_digit).  8N bytes of
 * plaintext, shared by the run's limbs, beside the frame's.  The mode is a wave-uniform run-time field of the argument record.
 */
#pragma once
#include "ntt_kernels_produce.h"
#include "ntt_lift.h"

namespace ntt {

template <class A> struct KLift {
  KArgs<A>        k; /* k.a = limb 0 of the run (c^), limb_stride / poly_stride of the output, the run's limb records */
  const uint64_t *m; /* the plaintext, [batch][N] with its own polynomial stride */
  uint64_t        m_poly_stride;
  uint32_t        accumulate;
  LiftCall        call[1]; /* (an array: read through an opaque index, see produce_fwd_body) */
  LiftLimb        ll[kLiftLimbs];
};

template <class A, int LOGN, int KSH>
__global__ void __launch_bounds__((Geom<LOGN, false, flavor_of<A>()>::WG), (Geom<LOGN, false, flavor_of<A>()>::WPS))
  lift_fwd_kernel(const KLift<A> kl)
{
  produce_fwd_body<A, LOGN, KSH>(kl, [&](uint64_t(&raw)[kE], uint64_t b, uint32_t tg, uint32_t, const LiftLimb &ll, const LiftCall &call) {
    const uint64_t *mblk = kl.m + b * kl.m_poly_stride;
    static_for<0, kE>([&](auto ee) {
      constexpr int   E   = decltype(ee)::value;
      const uint64_t *row = mblk + ((uint32_t)E << Plan<LOGN>::LT);
      raw[E]              = lift_digit(lift_word(stream_load(coef_at(row, tg)), call), call.mode, ll);
    });
  });
}

#define NTT_DEFINE_LAUNCH_LIFT_FWD(A, KSH)                                                                                                \
  template <> hipError_t launch_lift_fwd<A, KSH>(const LiftFwdArgs &la)                                                                   \
  {                                                                                                                                       \
    return NTT_LAUNCH_PRODUCE_FWD(A, KSH, KLift, lift_fwd_kernel, la, ([&](KLift<A> &kl) {                                                \
      kl.m             = la.m;                                                                                                            \
      kl.m_poly_stride = la.m_poly_stride ? la.m_poly_stride : (1ull << la.logn);                                                         \
    }));                                                                                                                                  \
  }

} // namespace ntt
