/* plain.hip -- out of the RNS (ntt_plain.h): two element-wise kernels that read the L words of one coefficient and write one word, in a
 * translation unit of their own:
 *   plain_kernel         m[p,s] = [x_c]_t, or round(t x / Q) mod t with the other constants: one output word per lane, grid-stride over
 *                        batch x N.  The L source words are requested four limbs at a time, ahead of their arithmetic, and the last one
 *                        to three as a group of their own (lincomb_kernel's shape; plain_word's order); consecutive lanes read
 *                        consecutive words of every limb.  Per limb one Shoup product, one conversion, one FP64 product and sum, one
 *                        128-bit multiply-add; then rint, one Barrett reduction (bconv_reduce) and one conditional subtraction.  The
 *                        constants sit in the kernel arguments (0.75 KB): uniform reads.  8N(L + 1) bytes per polynomial.
 *   plain_double_kernel  y[p,s] = fl(x_c) * scale for L = 1 or 2 (plain_double): 8N(L + 1) bytes per polynomial.
 * Integer and FP64 arithmetic that no policy owns: they serve every plan and every N >= 2.  Every lane reads all its words before its
 * one store: the output may BE limb 0 of the source (same polynomial stride). */
#include "ntt_plain.h"

namespace ntt {

struct KPlain {
  uint64_t *      m;
  const uint64_t *a;
  uint64_t        a_limb_stride, a_poly_stride, m_poly_stride, batch;
  uint32_t        logn;
  int             nlimbs;
  PlainConsts     k;
};
static_assert(sizeof(KPlain) < 4096, "the kernel-argument record must stay under 4 KB");

struct KPlainDouble {
  double *        y;
  const uint64_t *a;
  uint64_t        a_limb_stride, a_poly_stride, y_poly_stride, batch;
  uint32_t        logn;
  int             nlimbs;
  DoubleConsts    k;
};

__global__ void __launch_bounds__(256) plain_kernel(const KPlain k)
{
  const uint64_t n    = k.batch << k.logn;
  const uint64_t mask = (1ull << k.logn) - 1ull;
  for(uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t  p = i >> k.logn, s = i & mask;
    const uint64_t *src = k.a + p * k.a_poly_stride + s;
    uint64_t        hi = 0, lo = 0;
    double          f = 0.0;
    uint64_t        x[4];
    int             j = 0;
#pragma unroll 1
    for(; j + 4 <= k.nlimbs; j += 4) {
#pragma unroll
      for(int e = 0; e < 4; e++) x[e] = src[(uint64_t)(j + e) * k.a_limb_stride];
#pragma unroll
      for(int e = 0; e < 4; e++) plain_step(x[e], j + e, k.k, f, hi, lo);
    }
    const int r = k.nlimbs - j; /* 0 .. 3 */
#pragma unroll
    for(int e = 0; e < 3; e++)
      if(e < r) x[e] = src[(uint64_t)(j + e) * k.a_limb_stride];
#pragma unroll
    for(int e = 0; e < 3; e++)
      if(e < r) plain_step(x[e], j + e, k.k, f, hi, lo);
    k.m[p * k.m_poly_stride + s] = plain_finish(f, hi, lo, k.k);
  }
}

__global__ void __launch_bounds__(256) plain_double_kernel(const KPlainDouble k)
{
  const uint64_t n    = k.batch << k.logn;
  const uint64_t mask = (1ull << k.logn) - 1ull;
  for(uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t  p = i >> k.logn, s = i & mask;
    const uint64_t *src = k.a + p * k.a_poly_stride + s;
    const uint64_t  x0  = src[0];
    const uint64_t  x1  = k.nlimbs == 2 ? src[k.a_limb_stride] : 0;
    k.y[p * k.y_poly_stride + s] = plain_double(x0, x1, k.nlimbs, k.k);
  }
}

hipError_t launch_plain(const PlainArgs &pa)
{
  if(pa.nlimbs < 1 || pa.nlimbs > kPlainLimbs || pa.logn < 1 || pa.logn > 30) return hipErrorInvalidValue;
  KPlain k{};
  k.m             = pa.m;
  k.a             = pa.a;
  k.a_limb_stride = pa.a_limb_stride;
  k.a_poly_stride = pa.a_poly_stride;
  k.m_poly_stride = pa.m_poly_stride;
  k.batch         = pa.batch;
  k.logn          = pa.logn;
  k.nlimbs        = pa.nlimbs;
  k.k             = pa.k;
  const uint64_t n = pa.batch << pa.logn;
  if(n == 0) return hipSuccess;
  hipLaunchKernelGGL(plain_kernel, dim3(coef_grid(n, pa.max_grid)), dim3(256), 0, pa.stream, k);
  return hipGetLastError();
}

hipError_t launch_plain_double(const PlainDoubleArgs &pa)
{
  if(pa.nlimbs < 1 || pa.nlimbs > 2 || pa.logn < 1 || pa.logn > 30) return hipErrorInvalidValue;
  KPlainDouble k{};
  k.y             = pa.y;
  k.a             = pa.a;
  k.a_limb_stride = pa.a_limb_stride;
  k.a_poly_stride = pa.a_poly_stride;
  k.y_poly_stride = pa.y_poly_stride;
  k.batch         = pa.batch;
  k.logn          = pa.logn;
  k.nlimbs        = pa.nlimbs;
  k.k             = pa.k;
  const uint64_t n = pa.batch << pa.logn;
  if(n == 0) return hipSuccess;
  hipLaunchKernelGGL(plain_double_kernel, dim3(coef_grid(n, pa.max_grid)), dim3(256), 0, pa.stream, k);
  return hipGetLastError();
}

} /* namespace ntt */
