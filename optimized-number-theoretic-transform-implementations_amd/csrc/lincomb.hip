/* lincomb.hip -- the evaluator's linear layer on RNS operands (ntt_lincomb.h), an element-wise kernel over a run of up to 16 limbs
 * (blockIdx.y) and the whole batch, in a translation unit of its own:
 *   lincomb_kernel  c[s] (+)= bias_l + sum_{i<k} a_i[src_{g_i}(s)] * mu_i mod q_l, mu_i the word m_i[s] of term i's polynomial
 *                   multiplier or its scalar s_{i,l}.  galois_dot_kernel's shape and addressing with a Galois element per term: one
 *                   word per lane, the source slot from __brev, one multiply-add and a mask (galois_ntt_src; the identity for
 *                   g = 1), so consecutive lanes read inside one aligned tile of a_i and every byte fetched is used.  The term
 *                   records, the scalars, the Barrett constants and the bias sit in the kernel arguments (3.5 KB): uniform reads.
 *                   The exact 128-bit sum (bconv_mac), one Barrett reduction (bconv_reduce: proved in ntt_keyswitch.h for any
 *                   128-bit input and odd q < 2^63), one conditional subtraction; the bounds on k are in ntt_lincomb.h.
 *                   8N(k + n_m + 1) bytes per limb and polynomial for n_m polynomial multipliers (8N(k + 1) with multipliers shared
 *                   by the batch; 8N more when accumulating). */
#include "ntt_lincomb.h"

namespace ntt {

struct KLincomb {
  uint64_t *  c;
  LincombTerm t[kLincombTerms];
  int         k, accumulate;
  uint64_t    limb_stride, poly_stride, m_limb_stride, m_poly_stride, batch;
  uint32_t    logn;
  uint64_t    scalars[kLincombTerms][kLincombLimbs];
  BconvDst    ql[kLincombLimbs];
  uint64_t    bias[kLincombLimbs];
};
static_assert(sizeof(KLincomb) < 4096, "the kernel-argument record must stay under 4 KB");

/* term j's words for one position: the source word of a_j through sigma_{g_j} and the multiplier -- the scalar, a uniform read of
 * the kernel arguments, replaced by the word of m_j where the term has a polynomial multiplier (a uniform branch) */
__device__ __forceinline__ void lincomb_load(const KLincomb &k, int j, uint64_t base, uint32_t s, uint64_t mix, uint64_t &x, uint64_t &y)
{
  const LincombTerm &t = k.t[j];
  x                    = t.a[base + galois_ntt_src(s, t.g, k.logn)];
  y                    = k.scalars[j][blockIdx.y];
  if(t.m) y = t.m[mix];
}

/* One output word per thread and iteration: the source and multiplier words requested four terms at a time, ahead of their products,
 * and the last one to three terms as a group of their own (lincomb_word's order: c + bias first, the terms in order).  Every thread
 * reads all its words before it stores its own position: c may BE an a_i with g_i = 1, or an m_i in c's layout. */
__global__ void __launch_bounds__(256) lincomb_kernel(const KLincomb k)
{
  const BconvDst d    = k.ql[blockIdx.y];
  const uint64_t bias = k.bias[blockIdx.y];
  const uint64_t lo   = (uint64_t)blockIdx.y * k.limb_stride;
  const uint64_t mlo  = (uint64_t)blockIdx.y * k.m_limb_stride;
  const uint64_t n    = k.batch << k.logn;
  const uint32_t mask = (1u << k.logn) - 1u;
  for(uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t s    = (uint32_t)i & mask;
    const uint64_t p    = i >> k.logn;
    const uint64_t base = lo + p * k.poly_stride;
    const uint64_t mix  = mlo + p * k.m_poly_stride + s;
    uint64_t       hi   = 0, sum = (k.accumulate ? k.c[base + s] : 0) + bias;
    uint64_t       x[4], y[4];
    int            j = 0;
    for(; j + 4 <= k.k; j += 4) {
#pragma unroll
      for(int e = 0; e < 4; e++) lincomb_load(k, j + e, base, s, mix, x[e], y[e]);
#pragma unroll
      for(int e = 0; e < 4; e++) bconv_mac(hi, sum, x[e], y[e]);
    }
    const int r = k.k - j; /* 0 .. 3 */
#pragma unroll
    for(int e = 0; e < 3; e++)
      if(e < r) lincomb_load(k, j + e, base, s, mix, x[e], y[e]);
#pragma unroll
    for(int e = 0; e < 3; e++)
      if(e < r) bconv_mac(hi, sum, x[e], y[e]);
    const uint64_t v = bconv_reduce(hi, sum, d);
    k.c[base + s]    = v >= d.q ? v - d.q : v;
  }
}

hipError_t launch_lincomb(const LincombArgs &la)
{
  if(la.nlimbs < 1 || la.nlimbs > kLincombLimbs || la.k < 1 || la.k > kLincombTerms || la.logn < 1 || la.logn > 30) return hipErrorInvalidValue;
  KLincomb k{};
  k.c = la.c;
  for(int i = 0; i < la.k; i++) {
    k.t[i] = la.t[i];
    for(int l = 0; l < la.nlimbs; l++) k.scalars[i][l] = la.scalars[i][l];
  }
  k.k             = la.k;
  k.accumulate    = la.accumulate ? 1 : 0;
  k.limb_stride   = la.limb_stride;
  k.poly_stride   = la.poly_stride ? la.poly_stride : (1ull << la.logn);
  k.m_limb_stride = la.m_limb_stride;
  k.m_poly_stride = la.m_poly_stride;
  k.batch         = la.batch;
  k.logn          = la.logn;
  for(int l = 0; l < la.nlimbs; l++) {
    k.ql[l]   = la.ql[l];
    k.bias[l] = la.bias[l];
  }
  const uint64_t n = la.batch << la.logn;
  if(n == 0) return hipSuccess;
  hipLaunchKernelGGL(lincomb_kernel, dim3(coef_grid(n, la.max_grid), la.nlimbs), dim3(256), 0, la.stream, k);
  return hipGetLastError();
}

} /* namespace ntt */
