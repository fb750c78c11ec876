/* ct_elem.hip -- the element-wise kernels of a homomorphic multiplication on NTT-domain ciphertexts (ntt_ct_mul.h), over a run of up to
 * 16 limbs (blockIdx.y) and the whole batch, in a translation unit of its own:
 *   tensor_kernel   (c0, c1, c2)[s] = (a0 b0, a0 b1 + a1 b0, a1 b1)[s] mod q_l: the four input words of a position are loaded once, the
 *                   products are exact 128-bit integers (bconv_mac), one Barrett reduction per output word (bconv_reduce: proved in
 *                   ntt_keyswitch.h for any 128-bit input and odd q < 2^63), then one conditional subtraction.  With lazy input words,
 *                   anywhere in [0, 4q) for q < 2^61, a product is below (4q)^2 < 2^126 and the middle sum below 2 (4q)^2 < 2^127:
 *                   nothing overflows.  56N bytes per limb and polynomial; squaring (b_j is a_j): 16N read, 24N written.
 *   ct_fold_kernel  c[s] (+)= a[s] mod q_l, the two operands in layouts of their own: the addition (or the copy) that ends
 *                   ntt_rns_mod_down_add_batch's composition route.  Canonical words: c + a < 2q, one conditional subtraction. */
#include "ntt_ct_mul.h"

namespace ntt {

struct KTensor {
  uint64_t *      c[3];
  const uint64_t *a[2];
  const uint64_t *b[2];
  int             square;
  uint64_t        limb_stride, poly_stride, batch;
  uint32_t        logn;
  BconvDst        ql[kCtLimbs];
};

/* keypair_dot2_kernel's shape: one word per lane, the limb is the grid's y index.  Every thread reads its four words before it stores
 * its three, and no other thread touches that position: an output may BE an input. */
__global__ void __launch_bounds__(256) tensor_kernel(const KTensor k)
{
  const BconvDst d    = k.ql[blockIdx.y];
  const uint64_t lo   = (uint64_t)blockIdx.y * k.limb_stride;
  const uint64_t n    = k.batch << k.logn;
  const uint32_t mask = (1u << k.logn) - 1u;
  for(uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t s  = (uint32_t)i & mask;
    const uint64_t p  = i >> k.logn;
    const uint64_t at = lo + p * k.poly_stride + s;
    const uint64_t x0 = k.a[0][at], x1 = k.a[1][at];
    const uint64_t y0 = k.square ? x0 : k.b[0][at];
    const uint64_t y1 = k.square ? x1 : k.b[1][at];
    uint64_t       h1 = 0, l1 = 0;
    bconv_mac(h1, l1, x0, y1);
    bconv_mac(h1, l1, x1, y0);
    const uint64_t v0 = bconv_reduce(mulhi64(x0, y0), x0 * y0, d);
    const uint64_t v1 = bconv_reduce(h1, l1, d);
    const uint64_t v2 = bconv_reduce(mulhi64(x1, y1), x1 * y1, d);
    k.c[0][at]        = v0 >= d.q ? v0 - d.q : v0;
    k.c[1][at]        = v1 >= d.q ? v1 - d.q : v1;
    k.c[2][at]        = v2 >= d.q ? v2 - d.q : v2;
  }
}

hipError_t launch_tensor(const TensorArgs &ta)
{
  if(ta.nlimbs < 1 || ta.nlimbs > kCtLimbs || ta.logn < 1 || ta.logn > 30) return hipErrorInvalidValue;
  KTensor k{};
  for(int j = 0; j < 3; j++) k.c[j] = ta.c[j];
  for(int j = 0; j < 2; j++) {
    k.a[j] = ta.a[j];
    k.b[j] = ta.b[j];
  }
  k.square      = ta.square ? 1 : 0;
  k.limb_stride = ta.limb_stride;
  k.poly_stride = ta.poly_stride ? ta.poly_stride : (1ull << ta.logn);
  k.batch       = ta.batch;
  k.logn        = ta.logn;
  for(int l = 0; l < ta.nlimbs; l++) k.ql[l] = ta.ql[l];
  const uint64_t n = ta.batch << ta.logn;
  if(n == 0) return hipSuccess;
  hipLaunchKernelGGL(tensor_kernel, dim3(coef_grid(n, ta.max_grid), ta.nlimbs), dim3(256), 0, ta.stream, k);
  return hipGetLastError();
}

struct KCtFold {
  uint64_t *      c;
  const uint64_t *a;
  uint64_t        c_limb_stride, c_poly_stride, a_limb_stride, a_poly_stride, batch;
  uint32_t        logn;
  int             accumulate;
  uint64_t        q[kCtLimbs];
};

__global__ void __launch_bounds__(256) ct_fold_kernel(const KCtFold k)
{
  const uint64_t q    = k.q[blockIdx.y];
  const uint64_t clo  = (uint64_t)blockIdx.y * k.c_limb_stride;
  const uint64_t alo  = (uint64_t)blockIdx.y * k.a_limb_stride;
  const uint64_t n    = k.batch << k.logn;
  const uint32_t mask = (1u << k.logn) - 1u;
  for(uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t s   = (uint32_t)i & mask;
    const uint64_t p   = i >> k.logn;
    const uint64_t dst = clo + p * k.c_poly_stride + s;
    uint64_t       v   = k.a[alo + p * k.a_poly_stride + s];
    if(k.accumulate) {
      v += k.c[dst];
      v = v >= q ? v - q : v;
    }
    k.c[dst] = v;
  }
}

hipError_t launch_ct_fold(const CtFoldArgs &fa)
{
  if(fa.nlimbs < 1 || fa.nlimbs > kCtLimbs || fa.logn < 1 || fa.logn > 30) return hipErrorInvalidValue;
  KCtFold k{};
  k.c             = fa.c;
  k.a             = fa.a;
  k.c_limb_stride = fa.c_limb_stride;
  k.c_poly_stride = fa.c_poly_stride ? fa.c_poly_stride : (1ull << fa.logn);
  k.a_limb_stride = fa.a_limb_stride;
  k.a_poly_stride = fa.a_poly_stride ? fa.a_poly_stride : (1ull << fa.logn);
  k.batch         = fa.batch;
  k.logn          = fa.logn;
  k.accumulate    = fa.accumulate ? 1 : 0;
  for(int l = 0; l < fa.nlimbs; l++) k.q[l] = fa.q[l];
  const uint64_t n = fa.batch << fa.logn;
  if(n == 0) return hipSuccess;
  hipLaunchKernelGGL(ct_fold_kernel, dim3(coef_grid(n, fa.max_grid), fa.nlimbs), dim3(256), 0, fa.stream, k);
  return hipGetLastError();
}

} /* namespace ntt */
