/*
 * ntt_kernels_sample.h -- sample_fwd_kernel: a random polynomial drawn in the RNS fused with the forward transform
 * (NTT_SAMPLE_TRANSFORMED) for a run of limbs in ONE launch.  Included by the sample_f64*.hip units only (the host layer sees the
 * launchers of ntt_sample.h).
 *
 * produce_fwd_body (ntt_kernels_produce.h) with the sampler's digit: for each of the thread's kE coefficients the Philox block of (P, s)
 * and the limb's canonical word in integer arithmetic (sample_block, sample_small / sample_small_digit, sample_uniform_digit).  Nothing
 * is read.  The small kinds' block is the same in every limb's workgroup and is computed again in each: ten rounds of two 32 x 32 ->
 * 64-bit products per coefficient and limb, where the composition's element-wise launch computes it once per coefficient.  The kind and
 * the multiplier are wave-uniform run-time fields of the argument record.
 */
#pragma once
#include "ntt_kernels_produce.h"
#include "ntt_sample.h"

namespace ntt {

template <class A> struct KSample {
  KArgs<A>   k; /* k.a = limb 0 of the run (c^), limb_stride / poly_stride of the output, the run's limb records */
  uint32_t   accumulate;
  SampleCall call[1]; /* (an array: read through an opaque index, see produce_fwd_body) */
  SampleLimb ll[kSampleLimbs];
};

template <class A, int LOGN, int KSH>
__global__ void __launch_bounds__((Geom<LOGN, false, flavor_of<A>()>::WG), (Geom<LOGN, false, flavor_of<A>()>::WPS))
  sample_fwd_kernel(const KSample<A> ks)
{
  produce_fwd_body<A, LOGN, KSH>(ks, [&](uint64_t(&raw)[kE], uint64_t b, uint32_t tg, uint32_t lz, const SampleLimb &ll, const SampleCall &call) {
    const uint64_t Pn      = call.first_poly + b;
    const bool     uniform = call.kind == kSampleUniform;
    const uint32_t tag     = sample_tag(call.kind, call.limb0 + lz);
    static_for<0, kE>([&](auto ee) {
      constexpr int     E   = decltype(ee)::value;
      const SampleBlock blk = sample_block(call, Pn, ((uint32_t)E << Plan<LOGN>::LT) + tg, tag);
      raw[E]                = uniform ? sample_uniform_digit(blk, ll) : sample_small_digit(sample_small(call.kind, blk), ll);
    });
  });
}

#define NTT_DEFINE_LAUNCH_SAMPLE_FWD(A, KSH)                                                                                              \
  template <> hipError_t launch_sample_fwd<A, KSH>(const SampleFwdArgs &sa)                                                               \
  {                                                                                                                                       \
    return NTT_LAUNCH_PRODUCE_FWD(A, KSH, KSample, sample_fwd_kernel, sa, [](KSample<A> &) {});                                           \
  }

} // namespace ntt
