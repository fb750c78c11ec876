/* sample.hip -- the coefficient form of the device-side sampler (ntt_rns_sample_batch without NTT_SAMPLE_TRANSFORMED, and the middle of the
 * composed NTT-domain route): c_l (+)= the limb's word of a random polynomial for up to 16 limbs in ONE launch.  Nothing is read: 8NL
 * bytes for L limbs, 16NL accumulating.  Integer arithmetic of its own (ntt_sample.h) for every policy and every N >= 2. */
#include "ntt_sample.h"

namespace ntt {

struct KSampleCoef {
  uint64_t * c;
  uint64_t   limb_stride, poly_stride, batch;
  uint32_t   logn;
  int        nlimbs;
  uint32_t   accumulate;
  SampleCall call[1]; /* (an array: read through an opaque index, see the kernel) */
  SampleLimb limbs[kSampleLimbs];
};

/* One coefficient position per thread and iteration (lift_coef_kernel's shape): for the small kinds the Philox block and the centred
 * value once, then per limb the digit and the store, four limbs at a time; the uniform kind draws one block per limb (the tag carries
 * the limb).  The limbs' constants (112 words) are staged in LDS and re-read per limb and iteration, as in that kernel. */
__global__ void __launch_bounds__(256) sample_coef_kernel(const KSampleCoef k)
{
  __shared__ SampleLimb lim[kSampleLimbs];
#pragma unroll
  for(int l = 0; l < kSampleLimbs; l++) {
    if(threadIdx.x == (unsigned)l && l < k.nlimbs) lim[l] = k.limbs[l];
  }
  __syncthreads();
  const uint64_t n    = k.batch << k.logn;
  const uint64_t mask = (1ull << k.logn) - 1ull;
  for(uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    asm volatile("" ::: "memory"); /* (the constants' LDS reads stay inside the loop) */
    const uint64_t p = i >> k.logn;
    const uint32_t s = (uint32_t)(i & mask);
    const uint64_t j = p * k.poly_stride + s;
    /* the call's constants are read per iteration through an index the compiler cannot see through, as in lift_coef_kernel */
    uint32_t cz = 0;
    asm volatile("" : "+s"(cz));
    const SampleCall call    = k.call[cz];
    const uint64_t   P       = call.first_poly + p;
    const bool       uniform = call.kind == kSampleUniform;
    int              v       = 0;
    if(!uniform) v = sample_small(call.kind, sample_block(call, P, s, call.kind));
    /* four limbs at a time (lift_coef_kernel's shape): accumulating, their words are requested together, ahead of the arithmetic */
#pragma unroll 1
    for(int l0 = 0; l0 < k.nlimbs; l0 += 4) {
      uint64_t *cl = k.c + j + (uint64_t)l0 * k.limb_stride;
      uint64_t  c[4];
#pragma unroll
      for(int e = 0; e < 4; e++) c[e] = k.accumulate && l0 + e < k.nlimbs ? cl[(uint64_t)e * k.limb_stride] : 0;
#pragma unroll
      for(int e = 0; e < 4; e++) {
        if(l0 + e < k.nlimbs) {
          const SampleLimb r = lim[l0 + e];
          const uint64_t   d = uniform ? sample_uniform_digit(sample_block(call, P, s, sample_tag(kSampleUniform, call.limb0 + (uint32_t)(l0 + e))), r)
                                       : sample_small_digit(v, r);
          const uint64_t   u = d + c[e]; /* c = 0 unless accumulating: below 2q */
          cl[(uint64_t)e * k.limb_stride] = u >= r.q ? u - r.q : u;
        }
      }
    }
  }
}

hipError_t launch_sample_coef(const SampleCoefArgs &sa)
{
  KSampleCoef k{};
  if(!produce_coef_record(k, sa)) return hipErrorInvalidValue;
  const uint64_t n = sa.batch << sa.logn;
  if(n == 0) return hipSuccess;
  hipLaunchKernelGGL(sample_coef_kernel, dim3(coef_grid(n, sa.max_grid)), dim3(256), 0, sa.stream, k);
  return hipGetLastError();
}

} /* namespace ntt */
