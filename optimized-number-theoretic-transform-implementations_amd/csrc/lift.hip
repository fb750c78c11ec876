/* lift.hip -- the coefficient form of the lift into the RNS (ntt_rns_from_plain_batch, ntt_rns_from_double_batch without
 * NTT_LIFT_TRANSFORMED, and the middle of the composed NTT-domain route): c_l (+)= the limb's word of the lifted plaintext for up to 16
 * limbs in ONE launch, the plaintext word read once per coefficient (8N(L + 1) bytes for L limbs, 8N(2L + 1) accumulating).  Integer
 * arithmetic of its own (ntt_lift.h) for every policy and every N >= 2. */
#include "ntt_lift.h"

namespace ntt {

struct KLiftCoef {
  uint64_t *      c;
  const uint64_t *m;
  uint64_t        limb_stride, poly_stride, m_poly_stride, batch;
  uint32_t        logn;
  int             nlimbs;
  uint32_t        accumulate;
  LiftCall        call[1]; /* (an array: read through an opaque index, see the kernel) */
  LiftLimb        limbs[kLiftLimbs];
};

/* One coefficient position per thread and iteration (rescale_coef_kernel's shape): the plaintext word and its limb-independent part
 * (lift_word: the scaled mode's quotient, the double mode's magnitude) once, then per limb the digit and the store, four limbs at a time.  The limbs' constants (112 words) are staged in LDS and re-read per limb and
 * iteration, as in that kernel. */
__global__ void __launch_bounds__(256) lift_coef_kernel(const KLiftCoef k)
{
  __shared__ LiftLimb lim[kLiftLimbs];
#pragma unroll
  for(int l = 0; l < kLiftLimbs; l++) {
    if(threadIdx.x == (unsigned)l && l < k.nlimbs) lim[l] = k.limbs[l];
  }
  __syncthreads();
  const uint64_t n    = k.batch << k.logn;
  const uint64_t mask = (1ull << k.logn) - 1ull;
  for(uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    asm volatile("" ::: "memory"); /* (the constants' LDS reads stay inside the loop) */
    const uint64_t p = i >> k.logn, s = i & mask;
    const uint64_t j = p * k.poly_stride + s;
    /* the call's constants are read per iteration through an index the compiler cannot see through: held across the loop beside
     * the addresses they spilled 20 scalar registers */
    uint32_t cz = 0;
    asm volatile("" : "+s"(cz));
    const uint32_t mode = k.call[cz].mode;
    LiftWord       w;
    {
      const LiftCall call = k.call[cz];
      w                   = lift_word(k.m[p * k.m_poly_stride + s], call);
    }
    /* four limbs at a time (plain_kernel's shape): accumulating, their words are requested together, ahead of the arithmetic */
#pragma unroll 1
    for(int l0 = 0; l0 < k.nlimbs; l0 += 4) {
      uint64_t *cl = k.c + j + (uint64_t)l0 * k.limb_stride;
      uint64_t  c[4];
#pragma unroll
      for(int e = 0; e < 4; e++) c[e] = k.accumulate && l0 + e < k.nlimbs ? cl[(uint64_t)e * k.limb_stride] : 0;
#pragma unroll
      for(int e = 0; e < 4; e++) {
        if(l0 + e < k.nlimbs) {
          const LiftLimb r = lim[l0 + e];
          uint64_t       v = lift_digit(w, mode, r) + c[e]; /* c = 0 unless accumulating: below 2q */
          cl[(uint64_t)e * k.limb_stride] = v >= r.q ? v - r.q : v;
        }
      }
    }
  }
}

hipError_t launch_lift_coef(const LiftCoefArgs &la)
{
  KLiftCoef k{};
  if(!produce_coef_record(k, la)) return hipErrorInvalidValue;
  k.m              = la.m;
  k.m_poly_stride  = la.m_poly_stride ? la.m_poly_stride : (1ull << la.logn);
  const uint64_t n = la.batch << la.logn;
  if(n == 0) return hipSuccess;
  hipLaunchKernelGGL(lift_coef_kernel, dim3(coef_grid(n, la.max_grid)), dim3(256), 0, la.stream, k);
  return hipGetLastError();
}

} /* namespace ntt */
