/*
 * ntt_produce.h -- what the producers into the RNS share on the host side: the lifts (ntt_lift.h), the device-side sampler
 * (ntt_sample.h) and whatever comes next.  The launch record the host layer fills (host/host_produce.inc) and the kernels' launchers
 * read (ntt_kernels_produce.h, lift.hip, sample.hip), and the limbs of one launch.
 */
#pragma once
#include "ntt_keyswitch.h"

namespace ntt {

constexpr int kProduceLimbs = 16; /* limbs of one launch (= kMaxLimbs) */

/* What the host layer hands a producer's launcher, with the family's Call: one record for the coefficient kernel (a chunk of up to
 * kProduceLimbs limbs) and the fused kernel (a run of limbs; FP64 policies, N = 2^6..2^14).  host_produce.inc fills it. */
template <class Call> struct ProduceArgs {
  uint64_t *  c;      /* limb 0 of the chunk / the run (canonical words)               */
  const void *limbs;  /* fused: HOST array of the run's LimbRec<A>                     */
  int         nlimbs; /* 1 .. kProduceLimbs                                            */
  uint64_t    limb_stride, poly_stride, batch;
  uint32_t    logn;
  Call        call;
  BconvDst    ll[kProduceLimbs]; /* the limbs' constants (LiftLimb, SampleLimb)        */
  int         max_grid, num_cus; /* (num_cus: fused)                                   */
  hipStream_t stream;
};

/* the fields the coefficient kernels' records (KLiftCoef, KSampleCoef) share, from the host's record; false: an argument out of range */
template <class K, class Call> bool produce_coef_record(K &k, const ProduceArgs<Call> &pa)
{
  if(pa.nlimbs < 1 || pa.nlimbs > kProduceLimbs || pa.logn < 1 || pa.logn > 30) return false;
  k.c           = pa.c;
  k.limb_stride = pa.limb_stride;
  k.poly_stride = pa.poly_stride ? pa.poly_stride : (1ull << pa.logn);
  k.batch       = pa.batch;
  k.logn        = pa.logn;
  k.nlimbs      = pa.nlimbs;
  k.call[0]     = pa.call;
  k.accumulate  = pa.call.accumulate;
  for(int l = 0; l < pa.nlimbs; l++) k.limbs[l] = pa.ll[l];
  return true;
}

} // namespace ntt
