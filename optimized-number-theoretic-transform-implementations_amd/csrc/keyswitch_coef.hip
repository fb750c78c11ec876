/* keyswitch_coef.hip -- the coefficient-domain base conversions of hybrid key switching (ntt_keyswitch.h):
 *   bconv_kernel         ModUp: up to 16 destination limbs <- FastBConv of the digit's count <= 16 limbs, the digit read once per
 *                        launch (8N(count + ndst) bytes per polynomial);
 *   moddown_coef_kernel  ModDown without NTT_MODDOWN_TRANSFORMED, and the middle of the NTT-domain sandwich: up to 16 Q limbs
 *                        <- (c_l - u_l) * P^-1, the np P limbs read once per launch (8N(2 nq + np) bytes per polynomial).
 * Integer arithmetic for every modulus the plans accept (below 2^61): Shoup products for z_i, 128-bit sums of z_i [b^_i]_q reduced
 * once by Barrett (the bounds are proved in ntt_keyswitch.h).  The constants -- up to 16 x 16 words of [b^_i]_q -- are staged in
 * LDS and re-read per coefficient, as rescale_coef_kernel does with its limbs' constants. */
#include "ntt_keyswitch.h"

namespace ntt {

struct KBconv {
  uint64_t *a;
  uint64_t  limb_stride, poly_stride, batch;
  uint32_t  logn;
  int       first, count, k0, ndst;
  BconvSrc  sl[kBconvLimbs];
  BconvDst  dl[kBconvLimbs];
  uint64_t  g[kBconvLimbs][kBconvLimbs];
};

struct KModDownCoef {
  uint64_t *      c;
  const uint64_t *t;
  uint64_t        limb_stride, poly_stride, batch;
  uint32_t        logn;
  int             nlimbs, np;
  BconvSrc        pl[kBconvLimbs];
  BconvDst        ql[kBconvLimbs];
  uint64_t        g[kBconvLimbs][kBconvLimbs];
};

/* One coefficient position per thread and iteration: the source words requested together, the digits z_i, then per destination
 * limb the 128-bit sum over the sources, its reduction and the store. */
__global__ void __launch_bounds__(256) bconv_kernel(const KBconv k)
{
  __shared__ BconvSrc src[kBconvLimbs];
  __shared__ BconvDst dst[kBconvLimbs];
  __shared__ uint64_t gs[kBconvLimbs][kBconvLimbs];
  for(unsigned i = threadIdx.x; i < (unsigned)(kBconvLimbs * kBconvLimbs); i += blockDim.x) gs[i / kBconvLimbs][i % kBconvLimbs] = k.g[i / kBconvLimbs][i % kBconvLimbs];
  if(threadIdx.x < (unsigned)kBconvLimbs) {
    src[threadIdx.x] = k.sl[threadIdx.x];
    dst[threadIdx.x] = k.dl[threadIdx.x];
  }
  __syncthreads();
  const uint64_t n     = k.batch << k.logn;
  const uint64_t mask  = (1ull << k.logn) - 1ull;
  const int      slot0 = k.k0 < k.first ? k.k0 : k.k0 + k.count;
  for(uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    asm volatile("" ::: "memory"); /* (the constants' LDS reads stay inside the loop) */
    const uint64_t j = (i >> k.logn) * k.poly_stride + (i & mask);
    uint64_t       z[kBconvLimbs];
    const uint64_t *xs = k.a + (uint64_t)k.first * k.limb_stride + j;
#pragma unroll
    for(int s = 0; s < kBconvLimbs; s++) {
      z[s] = s < k.count ? *xs : 0;
      xs += k.limb_stride;
      asm volatile("" : "+v"(xs));
    }
#pragma unroll
    for(int s = 0; s < kBconvLimbs; s++) {
      if(s < k.count) z[s] = bconv_digit(z[s], src[s]);
    }
    uint64_t *co = k.a + (uint64_t)slot0 * k.limb_stride + j;
#pragma unroll
    for(int d = 0; d < kBconvLimbs; d++) {
      if(d < k.ndst) {
        uint64_t hi = 0, lo = 0;
#pragma unroll
        for(int s = 0; s < kBconvLimbs; s++) {
          if(s < k.count) bconv_mac(hi, lo, z[s], gs[s][d]);
        }
        const BconvDst dd = dst[d];
        const uint64_t v  = bconv_reduce(hi, lo, dd);
        *co               = v >= dd.q ? v - dd.q : v;
      }
      /* the next destination limb: the next slot, or past the digit */
      co += k.k0 + d + 1 == k.first ? (uint64_t)(k.count + 1) * k.limb_stride : k.limb_stride;
      asm volatile("" : "+v"(co));
    }
  }
}

hipError_t launch_bconv(const BconvArgs &ba)
{
  if(ba.count < 1 || ba.count > kBconvLimbs || ba.ndst < 1 || ba.ndst > kBconvLimbs) return hipErrorInvalidValue;
  KBconv k{};
  k.a           = ba.a;
  k.limb_stride = ba.limb_stride;
  k.poly_stride = ba.poly_stride ? ba.poly_stride : (1ull << ba.logn);
  k.batch       = ba.batch;
  k.logn        = ba.logn;
  k.first       = ba.first;
  k.count       = ba.count;
  k.k0          = ba.k0;
  k.ndst        = ba.ndst;
  for(int s = 0; s < ba.count; s++) k.sl[s] = ba.sl[s];
  for(int d = 0; d < ba.ndst; d++) k.dl[d] = ba.dl[d];
  for(int s = 0; s < ba.count; s++)
    for(int d = 0; d < ba.ndst; d++) k.g[s][d] = ba.g[s][d];
  const uint64_t n = ba.batch << ba.logn;
  if(n == 0) return hipSuccess;
  hipLaunchKernelGGL(bconv_kernel, dim3(coef_grid(n, ba.max_grid)), dim3(256), 0, ba.stream, k);
  return hipGetLastError();
}

/* One coefficient position per thread and iteration: the P words and the Q words requested together (up to 32 loads in flight
 * per lane), the digits z_j, then per Q limb the sum, (c - u) * P^-1 by Shoup's method and the store. */
__global__ void __launch_bounds__(256) moddown_coef_kernel(const KModDownCoef k)
{
  __shared__ BconvSrc src[kBconvLimbs];
  __shared__ BconvDst dst[kBconvLimbs];
  __shared__ uint64_t gs[kBconvLimbs][kBconvLimbs];
  for(unsigned i = threadIdx.x; i < (unsigned)(kBconvLimbs * kBconvLimbs); i += blockDim.x) gs[i / kBconvLimbs][i % kBconvLimbs] = k.g[i / kBconvLimbs][i % kBconvLimbs];
  if(threadIdx.x < (unsigned)kBconvLimbs) {
    src[threadIdx.x] = k.pl[threadIdx.x];
    dst[threadIdx.x] = k.ql[threadIdx.x];
  }
  __syncthreads();
  const uint64_t n    = k.batch << k.logn;
  const uint64_t mask = (1ull << k.logn) - 1ull;
  for(uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    asm volatile("" ::: "memory"); /* (the constants' LDS reads stay inside the loop) */
    const uint64_t  j  = (i >> k.logn) * k.poly_stride + (i & mask);
    uint64_t        z[kBconvLimbs], c[kBconvLimbs];
    const uint64_t *ts = k.t + j;
#pragma unroll
    for(int s = 0; s < kBconvLimbs; s++) {
      z[s] = s < k.np ? *ts : 0;
      ts += k.limb_stride;
      asm volatile("" : "+v"(ts));
    }
    const uint64_t *cl = k.c + j;
#pragma unroll
    for(int l = 0; l < kBconvLimbs; l++) {
      c[l] = l < k.nlimbs ? *cl : 0;
      cl += k.limb_stride;
      asm volatile("" : "+v"(cl));
    }
#pragma unroll
    for(int s = 0; s < kBconvLimbs; s++) {
      if(s < k.np) z[s] = bconv_digit(z[s], src[s]);
    }
    uint64_t *co = k.c + j;
#pragma unroll
    for(int l = 0; l < kBconvLimbs; l++) {
      if(l < k.nlimbs) {
        uint64_t hi = 0, lo = 0;
#pragma unroll
        for(int s = 0; s < kBconvLimbs; s++) {
          if(s < k.np) bconv_mac(hi, lo, z[s], gs[s][l]);
        }
        const BconvDst r = dst[l];
        const uint64_t u = moddown_digit(hi, lo, r);
        const uint64_t d = c[l] >= u ? c[l] - u : c[l] + (r.q - u);
        uint64_t       v = d * r.s - mulhi64(d, r.s_shoup) * r.q; /* [0, 2q) */
        *co              = v >= r.q ? v - r.q : v;
      }
      co += k.limb_stride;
      asm volatile("" : "+v"(co));
    }
  }
}

hipError_t launch_moddown_coef(const ModDownCoefArgs &ma)
{
  if(ma.nlimbs < 1 || ma.nlimbs > kBconvLimbs || ma.np < 1 || ma.np > kBconvLimbs) return hipErrorInvalidValue;
  KModDownCoef k{};
  k.c           = ma.c;
  k.t           = ma.t;
  k.limb_stride = ma.limb_stride;
  k.poly_stride = ma.poly_stride ? ma.poly_stride : (1ull << ma.logn);
  k.batch       = ma.batch;
  k.logn        = ma.logn;
  k.nlimbs      = ma.nlimbs;
  k.np          = ma.np;
  for(int s = 0; s < ma.np; s++) k.pl[s] = ma.pl[s];
  for(int l = 0; l < ma.nlimbs; l++) k.ql[l] = ma.ql[l];
  for(int s = 0; s < ma.np; s++)
    for(int l = 0; l < ma.nlimbs; l++) k.g[s][l] = ma.g[s][l];
  const uint64_t n = ma.batch << ma.logn;
  if(n == 0) return hipSuccess;
  hipLaunchKernelGGL(moddown_coef_kernel, dim3(coef_grid(n, ma.max_grid)), dim3(256), 0, ma.stream, k);
  return hipGetLastError();
}

} /* namespace ntt */
