/* rescale_coef.hip -- the coefficient form of the RNS rescale (ntt_rns_rescale_batch without NTT_RESCALE_TRANSFORMED, and the
 * middle of the NTT-domain sandwich): c_l <- (c_l - u_l) * s_l mod q_l for up to 16 kept limbs in ONE launch, t read once per
 * coefficient (8N(2L+1) bytes for L kept limbs).  Integer arithmetic for every modulus below 2^62: u_l by Barrett (rescale_digit), the product
 * by Shoup's method. */
#include "ntt_rescale.h"

namespace ntt {

struct KRescaleCoef {
  uint64_t *      c;
  const uint64_t *t;
  uint64_t        limb_stride, poly_stride, batch;
  uint32_t        logn;
  int             nlimbs;
  uint64_t        qL, hL;
  RescaleLimb     limbs[kRescaleLimbs];
};

/* One coefficient position per thread and iteration: t's word, then the words of every kept limb requested together (up to 16
 * loads in flight per lane -- one at a time would leave the memory system idle), then the products and the stores.  The limbs'
 * constants (80 words) are staged in LDS and re-read per limb and iteration: held in scalar registers across the loop they
 * spilled (211 SGPRs). */
__global__ void __launch_bounds__(256) rescale_coef_kernel(const KRescaleCoef k)
{
  __shared__ RescaleLimb lim[kRescaleLimbs];
#pragma unroll
  for(int l = 0; l < kRescaleLimbs; l++) {
    if(threadIdx.x == (unsigned)l && l < k.nlimbs) lim[l] = k.limbs[l];
  }
  __syncthreads();
  const uint64_t n    = k.batch << k.logn;
  const uint64_t mask = (1ull << k.logn) - 1ull;
  for(uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    asm volatile("" ::: "memory"); /* (the constants' LDS reads stay inside the loop) */
    const uint64_t j  = (i >> k.logn) * k.poly_stride + (i & mask);
    const uint64_t tv = k.t[j];
    uint64_t       c[kRescaleLimbs];
    /* (the limbs' addresses as one chain of per-lane pointers: sixteen scalar limb offsets held across the loop would not fit) */
    const uint64_t *cl = k.c + j;
#pragma unroll
    for(int l = 0; l < kRescaleLimbs; l++) {
      c[l] = l < k.nlimbs ? *cl : 0;
      cl += k.limb_stride;
      asm volatile("" : "+v"(cl));
    }
    uint64_t *co = k.c + j;
#pragma unroll
    for(int l = 0; l < kRescaleLimbs; l++) {
      if(l < k.nlimbs) {
        const RescaleLimb r = lim[l];
        const uint64_t    u = rescale_digit(tv, k.qL, k.hL, r);
        const uint64_t    d = c[l] >= u ? c[l] - u : c[l] + (r.q - u);
        uint64_t          v = d * r.s - mulhi64(d, r.s_shoup) * r.q; /* [0, 2q) */
        v                   = v >= r.q ? v - r.q : v;
        *co                 = v;
      }
      co += k.limb_stride;
      asm volatile("" : "+v"(co));
    }
  }
}

hipError_t launch_rescale_coef(const RescaleCoefArgs &ra)
{
  if(ra.nlimbs < 1 || ra.nlimbs > kRescaleLimbs) return hipErrorInvalidValue;
  KRescaleCoef k{};
  k.c           = ra.c;
  k.t           = ra.t;
  k.limb_stride = ra.limb_stride;
  k.poly_stride = ra.poly_stride ? ra.poly_stride : (1ull << ra.logn);
  k.batch       = ra.batch;
  k.logn        = ra.logn;
  k.nlimbs      = ra.nlimbs;
  k.qL          = ra.qL;
  k.hL          = ra.hL;
  for(int l = 0; l < ra.nlimbs; l++) k.limbs[l] = ra.limbs[l];
  const uint64_t n = ra.batch << ra.logn;
  if(n == 0) return hipSuccess;
  /* the pointwise kernels' grid rule (host_products.inc grid_pw): about four iterations per workgroup */
  const uint64_t total = (n + 255) / 256;
  uint64_t       g     = (total + 3) / 4;
  if(g < 2048) g = total < 2048 ? total : 2048;
  if(g > (1u << 22)) g = 1u << 22;
  if(ra.max_grid > 0) g = total < (uint64_t)ra.max_grid ? total : (uint64_t)ra.max_grid;
  hipLaunchKernelGGL(rescale_coef_kernel, dim3((unsigned)(g ? g : 1)), dim3(256), 0, ra.stream, k);
  return hipGetLastError();
}

} /* namespace ntt */
