/* exact_coef.hip -- the coefficient-domain EXACT base conversions of BFV multiplication (ntt_exact.h):
 *   exact_up_coef_kernel    exact ModUp: up to 16 destination limbs <- ExactBConv of the digit's count <= 16 limbs, the digit read once
 *                           per launch (8N(count + ndst) bytes per polynomial, as bconv_kernel);
 *   exact_down_coef_kernel  exact scaled ModDown without NTT_MODDOWN_TRANSFORMED, and the middle of the NTT-domain sandwich: up to 16 Q
 *                           limbs <- c_l [m P^-1] - ExactBConv_{P->q_l}([m t]_P) [P^-1], the np P limbs read once per launch
 *                           (8N(2 nq + np) bytes per polynomial, as moddown_coef_kernel).
 * keyswitch_coef.hip's kernels with ONE FP64 sum per coefficient position beside the digits: v = rint(sum_i fl(z_i) rho_i) is formed
 * once and shared by the launch's destination limbs, where it enters each 128-bit sum as one more product before the Barrett
 * reduction.  The sum depends on the source words only, so the launches of one call agree on it. */
#include "ntt_exact.h"

namespace ntt {

/* (3.6 KB and 3.9 KB: the kernel arguments hold 4 KB) */
struct KBconvExact {
  uint64_t *a;
  uint64_t  limb_stride, poly_stride, batch;
  uint32_t  logn;
  int       first, count, k0, ndst;
  BconvSrc  sl[kBconvLimbs];
  BconvDst  dl[kBconvLimbs];
  uint64_t  g[kBconvLimbs][kBconvLimbs];
  double    rho[kBconvLimbs];
};

struct KModDownExact {
  uint64_t *      c;
  const uint64_t *t;
  uint64_t        limb_stride, poly_stride, batch;
  uint32_t        logn;
  int             nlimbs, np;
  BconvSrc        pl[kBconvLimbs];
  BconvDst        ql[kBconvLimbs];
  uint64_t        g[kBconvLimbs][kBconvLimbs];
  double          rho[kBconvLimbs];
  ExactScale      es[kBconvLimbs];
};
static_assert(sizeof(KBconvExact) <= 3840 && sizeof(KModDownExact) <= 3968, "the exact kernels' argument records must stay below 4 KB");

/* v of one coefficient position from its digits, in ntt_exact.h's operation order */
__device__ __forceinline__ uint64_t exact_v(const uint64_t (&z)[kBconvLimbs], const double *rho, int n)
{
  double s = exact_term(z[0], rho[0]);
#pragma unroll
  for(int i = 1; i < kBconvLimbs; i++) {
    if(i < n) s = s + exact_term(z[i], rho[i]);
  }
  return exact_round(s);
}

/* bconv_kernel's loop; v beside the digits */
__global__ void __launch_bounds__(256) exact_up_coef_kernel(const KBconvExact k)
{
  __shared__ BconvSrc src[kBconvLimbs];
  __shared__ BconvDst dst[kBconvLimbs];
  __shared__ double   rho[kBconvLimbs];
  __shared__ uint64_t gs[kBconvLimbs][kBconvLimbs];
  for(unsigned i = threadIdx.x; i < (unsigned)(kBconvLimbs * kBconvLimbs); i += blockDim.x) gs[i / kBconvLimbs][i % kBconvLimbs] = k.g[i / kBconvLimbs][i % kBconvLimbs];
  if(threadIdx.x < (unsigned)kBconvLimbs) {
    src[threadIdx.x] = k.sl[threadIdx.x];
    dst[threadIdx.x] = k.dl[threadIdx.x];
    rho[threadIdx.x] = k.rho[threadIdx.x];
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
    const uint64_t v  = exact_v(z, rho, k.count);
    uint64_t *     co = k.a + (uint64_t)slot0 * k.limb_stride + j;
#pragma unroll
    for(int d = 0; d < kBconvLimbs; d++) {
      if(d < k.ndst) {
        uint64_t hi = 0, lo = 0;
#pragma unroll
        for(int s = 0; s < kBconvLimbs; s++) {
          if(s < k.count) bconv_mac(hi, lo, z[s], gs[s][d]);
        }
        *co = exact_bconv_finish(hi, lo, v, dst[d]);
      }
      /* the next destination limb: the next slot, or past the digit */
      co += k.k0 + d + 1 == k.first ? (uint64_t)(k.count + 1) * k.limb_stride : k.limb_stride;
      asm volatile("" : "+v"(co));
    }
  }
}

hipError_t launch_bconv_exact(const BconvExactArgs &xa)
{
  const BconvArgs &ba = xa.ba;
  if(ba.count < 1 || ba.count > kBconvLimbs || ba.ndst < 1 || ba.ndst > kBconvLimbs) return hipErrorInvalidValue;
  KBconvExact k{};
  k.a           = ba.a;
  k.limb_stride = ba.limb_stride;
  k.poly_stride = ba.poly_stride ? ba.poly_stride : (1ull << ba.logn);
  k.batch       = ba.batch;
  k.logn        = ba.logn;
  k.first       = ba.first;
  k.count       = ba.count;
  k.k0          = ba.k0;
  k.ndst        = ba.ndst;
  for(int s = 0; s < ba.count; s++) {
    k.sl[s]  = ba.sl[s];
    k.rho[s] = xa.rho[s];
  }
  for(int d = 0; d < ba.ndst; d++) k.dl[d] = ba.dl[d];
  for(int s = 0; s < ba.count; s++)
    for(int d = 0; d < ba.ndst; d++) k.g[s][d] = ba.g[s][d];
  const uint64_t n = ba.batch << ba.logn;
  if(n == 0) return hipSuccess;
  hipLaunchKernelGGL(exact_up_coef_kernel, dim3(coef_grid(n, ba.max_grid)), dim3(256), 0, ba.stream, k);
  return hipGetLastError();
}

/* moddown_coef_kernel's loop; v beside the digits, the two-constant epilogue */
__global__ void __launch_bounds__(256) exact_down_coef_kernel(const KModDownExact k)
{
  __shared__ BconvSrc   src[kBconvLimbs];
  __shared__ BconvDst   dst[kBconvLimbs];
  __shared__ double     rho[kBconvLimbs];
  __shared__ ExactScale es[kBconvLimbs];
  __shared__ uint64_t   gs[kBconvLimbs][kBconvLimbs];
  for(unsigned i = threadIdx.x; i < (unsigned)(kBconvLimbs * kBconvLimbs); i += blockDim.x) gs[i / kBconvLimbs][i % kBconvLimbs] = k.g[i / kBconvLimbs][i % kBconvLimbs];
  if(threadIdx.x < (unsigned)kBconvLimbs) {
    src[threadIdx.x] = k.pl[threadIdx.x];
    dst[threadIdx.x] = k.ql[threadIdx.x];
    rho[threadIdx.x] = k.rho[threadIdx.x];
    es[threadIdx.x]  = k.es[threadIdx.x];
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
    const uint64_t v  = exact_v(z, rho, k.np);
    uint64_t *     co = k.c + j;
#pragma unroll
    for(int l = 0; l < kBconvLimbs; l++) {
      if(l < k.nlimbs) {
        uint64_t hi = 0, lo = 0;
#pragma unroll
        for(int s = 0; s < kBconvLimbs; s++) {
          if(s < k.np) bconv_mac(hi, lo, z[s], gs[s][l]);
        }
        const BconvDst r = dst[l];
        *co              = moddown_exact_word(c[l], exact_bconv_finish(hi, lo, v, r), r, es[l]);
      }
      co += k.limb_stride;
      asm volatile("" : "+v"(co));
    }
  }
}

hipError_t launch_moddown_exact_coef(const ModDownExactArgs &xa)
{
  const ModDownCoefArgs &ma = xa.ma;
  if(ma.nlimbs < 1 || ma.nlimbs > kBconvLimbs || ma.np < 1 || ma.np > kBconvLimbs) return hipErrorInvalidValue;
  KModDownExact k{};
  k.c           = ma.c;
  k.t           = ma.t;
  k.limb_stride = ma.limb_stride;
  k.poly_stride = ma.poly_stride ? ma.poly_stride : (1ull << ma.logn);
  k.batch       = ma.batch;
  k.logn        = ma.logn;
  k.nlimbs      = ma.nlimbs;
  k.np          = ma.np;
  for(int s = 0; s < ma.np; s++) {
    k.pl[s]  = ma.pl[s];
    k.rho[s] = xa.rho[s];
  }
  for(int l = 0; l < ma.nlimbs; l++) {
    k.ql[l] = ma.ql[l];
    k.es[l] = xa.es[l];
  }
  for(int s = 0; s < ma.np; s++)
    for(int l = 0; l < ma.nlimbs; l++) k.g[s][l] = ma.g[s][l];
  const uint64_t n = ma.batch << ma.logn;
  if(n == 0) return hipSuccess;
  hipLaunchKernelGGL(exact_down_coef_kernel, dim3(coef_grid(n, ma.max_grid)), dim3(256), 0, ma.stream, k);
  return hipGetLastError();
}

} /* namespace ntt */
