/* galois_coef.hip -- the Galois automorphisms sigma_g: a(X) -> a(X^g) and the rotation key product (ntt_galois.h), element-wise
 * kernels over a run of up to 16 limbs (blockIdx.y) and the whole batch:
 *   galois_ntt_kernel    NTT domain: out[s] = in[src(s)], src from __brev, one multiply-add and a mask (galois_ntt_src): no index
 *                        table, no LDS.  Consecutive lanes write consecutive slots and read inside one aligned tile of the input
 *                        (64 slots: one 512-byte block, every byte used): 16N bytes per limb and polynomial.  <true>: one aligned
 *                        pair of slots per lane, 16-byte accesses (the source pair is aligned too, swapped when src is odd);
 *                        <false>: one slot per lane, for operands that are not 16-byte aligned throughout.
 *   galois_dot_kernel    c[s] (+)= sum_{i<k} a_i[src(s)] * key_i[s] mod q_l with the same addressing: the exact 128-bit sum of up
 *                        to 32 products below (2^61)^2, plus c < 2^61 when accumulating -- 32 (2^61)^2 + 2^61 < 2^128 -- reduced
 *                        once (bconv_mac, bconv_reduce: proved in ntt_keyswitch.h for any 128-bit input and odd q < 2^63), then
 *                        one conditional subtraction.  8N(2k + 1) bytes per limb and polynomial (8N(k + 1) with a key shared by
 *                        the batch; 8N more when accumulating).
 *   galois_coef_kernel   coefficients: out[t] = a[u] or q - a[u - N] with u = g^-1 t mod 2N (galois_coef_src): a signed stride
 *                        gather.  Consecutive workgroups cover consecutive 256-word pieces of one polynomial, so the workgroups
 *                        that re-read a polynomial's lines (each 64-byte line serves 8 outputs, spread over the polynomial) run
 *                        together and the re-reads are served on chip. */
#include "ntt_galois.h"

namespace ntt {

struct KGalois {
  uint64_t *      out;
  const uint64_t *in;
  uint64_t        limb_stride, poly_stride, batch;
  uint32_t        logn, g; /* galois_coef_kernel: g holds g^-1 mod 2N */
  uint64_t        q[kGaloisLimbs];
};

struct KGaloisDot {
  uint64_t *      c;
  const uint64_t *a[kGaloisDot];
  const uint64_t *key[kGaloisDot];
  int             k, accumulate;
  uint64_t        limb_stride, poly_stride, key_limb_stride, key_poly_stride, batch;
  uint32_t        logn, g;
  BconvDst        ql[kGaloisLimbs];
};

template <bool PAIR> __global__ void __launch_bounds__(256) galois_ntt_kernel(const KGalois k)
{
  const uint64_t  lo  = (uint64_t)blockIdx.y * k.limb_stride;
  uint64_t *      out = k.out + lo;
  const uint64_t *in  = k.in + lo;
  if constexpr(PAIR) {
    /* pair t of a polynomial: slots 2t, 2t + 1 <- the aligned pair that holds src(2t), swapped when src(2t) is its odd word */
    const uint32_t lp   = k.logn - 1u;
    const uint64_t n    = k.batch << lp;
    const uint32_t mask = (1u << lp) - 1u;
    for(uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
      const uint32_t   s    = ((uint32_t)i & mask) << 1;
      const uint64_t   base = (i >> lp) * k.poly_stride;
      const uint32_t   src  = galois_ntt_src(s, k.g, k.logn);
      const ulonglong2 v    = *reinterpret_cast<const ulonglong2 *>(in + base + (src & ~1u));
      *reinterpret_cast<ulonglong2 *>(out + base + s) = (src & 1u) ? make_ulonglong2(v.y, v.x) : v;
    }
  } else {
    const uint64_t n    = k.batch << k.logn;
    const uint32_t mask = (1u << k.logn) - 1u;
    for(uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
      const uint32_t s    = (uint32_t)i & mask;
      const uint64_t base = (i >> k.logn) * k.poly_stride;
      out[base + s]       = in[base + galois_ntt_src(s, k.g, k.logn)];
    }
  }
}

__global__ void __launch_bounds__(256) galois_coef_kernel(const KGalois k)
{
  const uint64_t  lo   = (uint64_t)blockIdx.y * k.limb_stride;
  uint64_t *      out  = k.out + lo;
  const uint64_t *in   = k.in + lo;
  const uint64_t  q    = k.q[blockIdx.y];
  const uint64_t  n    = k.batch << k.logn;
  const uint32_t  mask = (1u << k.logn) - 1u;
  for(uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t t    = (uint32_t)i & mask;
    const uint64_t base = (i >> k.logn) * k.poly_stride;
    const uint32_t u    = galois_coef_src(t, k.g, k.logn);
    const uint64_t v    = in[base + (u & mask)];
    out[base + t]       = (u > mask && v != 0) ? q - v : v;
  }
}

/* One output word per thread and iteration: the k source words and the k key words requested four pairs at a time, the products
 * summed in 128 bits. */
__global__ void __launch_bounds__(256) galois_dot_kernel(const KGaloisDot k)
{
  const BconvDst d    = k.ql[blockIdx.y];
  const uint64_t lo   = (uint64_t)blockIdx.y * k.limb_stride;
  const uint64_t klo  = (uint64_t)blockIdx.y * k.key_limb_stride;
  const uint64_t n    = k.batch << k.logn;
  const uint32_t mask = (1u << k.logn) - 1u;
  for(uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t s    = (uint32_t)i & mask;
    const uint64_t p    = i >> k.logn;
    const uint64_t dst  = lo + p * k.poly_stride + s;
    const uint64_t src  = lo + p * k.poly_stride + galois_ntt_src(s, k.g, k.logn);
    const uint64_t kix  = klo + p * k.key_poly_stride + s;
    uint64_t       hi   = 0, sum = k.accumulate ? k.c[dst] : 0;
    int            j    = 0;
    for(; j + 4 <= k.k; j += 4) {
      uint64_t x[4], y[4];
#pragma unroll
      for(int e = 0; e < 4; e++) {
        x[e] = k.a[j + e][src];
        y[e] = k.key[j + e][kix];
      }
#pragma unroll
      for(int e = 0; e < 4; e++) bconv_mac(hi, sum, x[e], y[e]);
    }
    for(; j < k.k; j++) bconv_mac(hi, sum, k.a[j][src], k.key[j][kix]);
    const uint64_t v = bconv_reduce(hi, sum, d);
    k.c[dst]         = v >= d.q ? v - d.q : v;
  }
}

hipError_t launch_galois(const GaloisArgs &ga)
{
  if(ga.nlimbs < 1 || ga.nlimbs > kGaloisLimbs || ga.logn < 1 || ga.logn > 30) return hipErrorInvalidValue;
  KGalois k{};
  k.out         = ga.out;
  k.in          = ga.in;
  k.limb_stride = ga.limb_stride;
  k.poly_stride = ga.poly_stride ? ga.poly_stride : (1ull << ga.logn);
  k.batch       = ga.batch;
  k.logn        = ga.logn;
  const uint64_t n = ga.batch << ga.logn;
  if(n == 0) return hipSuccess;
  if(ga.ntt_domain) {
    k.g = ga.g;
    /* 16-byte accesses where every word pair of both operands is 16-byte aligned */
    const bool pair = (((uintptr_t)ga.out | (uintptr_t)ga.in) & 15) == 0 && ((k.limb_stride | k.poly_stride) & 1) == 0;
    if(pair) hipLaunchKernelGGL(galois_ntt_kernel<true>, dim3(coef_grid(n / 2, ga.max_grid), ga.nlimbs), dim3(256), 0, ga.stream, k);
    else hipLaunchKernelGGL(galois_ntt_kernel<false>, dim3(coef_grid(n, ga.max_grid), ga.nlimbs), dim3(256), 0, ga.stream, k);
  } else {
    k.g = galois_inverse(ga.g) & ((2u << ga.logn) - 1u);
    for(int l = 0; l < ga.nlimbs; l++) k.q[l] = ga.q[l];
    hipLaunchKernelGGL(galois_coef_kernel, dim3(coef_grid(n, ga.max_grid), ga.nlimbs), dim3(256), 0, ga.stream, k);
  }
  return hipGetLastError();
}

hipError_t launch_galois_dot(const GaloisDotArgs &da)
{
  if(da.nlimbs < 1 || da.nlimbs > kGaloisLimbs || da.k < 1 || da.k > kGaloisDot || da.logn < 1 || da.logn > 30) return hipErrorInvalidValue;
  KGaloisDot k{};
  k.c = da.c;
  for(int i = 0; i < da.k; i++) {
    k.a[i]   = da.a[i];
    k.key[i] = da.key[i];
  }
  k.k               = da.k;
  k.accumulate      = da.accumulate ? 1 : 0;
  k.limb_stride     = da.limb_stride;
  k.poly_stride     = da.poly_stride ? da.poly_stride : (1ull << da.logn);
  k.key_limb_stride = da.key_limb_stride;
  k.key_poly_stride = da.key_poly_stride;
  k.batch           = da.batch;
  k.logn            = da.logn;
  k.g               = da.g;
  for(int l = 0; l < da.nlimbs; l++) k.ql[l] = da.ql[l];
  const uint64_t n = da.batch << da.logn;
  if(n == 0) return hipSuccess;
  hipLaunchKernelGGL(galois_dot_kernel, dim3(coef_grid(n, da.max_grid), da.nlimbs), dim3(256), 0, da.stream, k);
  return hipGetLastError();
}

} /* namespace ntt */
