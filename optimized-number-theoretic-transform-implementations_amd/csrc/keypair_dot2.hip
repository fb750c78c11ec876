/* keypair_dot2.hip -- the rotation key product for BOTH components of a key (ntt_galois.h), an element-wise kernel over a run of up to
 * 16 limbs (blockIdx.y) and the whole batch, in a translation unit of its own:
 *   keypair_dot2_kernel  c_j[s] (+)= sum_{i<k} a_i[src(s)] * key_j,i[s] mod q_l, j = 0, 1, with galois_dot_kernel's addressing
 *                        (galois_coef.hip): every permuted word is loaded once and multiplied into two exact 128-bit sums (up to 32
 *                        products below 2^124 plus c < 2^64 each), one Barrett reduction per sum (bconv_mac, bconv_reduce: proved in
 *                        ntt_keyswitch.h for any 128-bit input and odd q < 2^63), then one conditional subtraction.  8N(3k + 2)
 *                        bytes per limb and polynomial (8N(k + 2) with broadcast keys; 16N more when accumulating).  With g = 1 and
 *                        k = 1 it is the two-output element-wise product of the pair key products' composition route
 *                        (host/host_key_pair.inc): c_j[s] (+)= x[s] * key_j[s], canonical for lazy key words too. */
#include "ntt_galois.h"

namespace ntt {

struct KKeyPairDot2 {
  uint64_t *      c[2];
  const uint64_t *a[kGaloisDot];
  const uint64_t *key[2][kGaloisDot];
  int             k, accumulate;
  uint64_t        limb_stride, poly_stride, key_limb_stride, key_poly_stride, batch;
  uint32_t        logn, g;
  BconvDst        ql[kGaloisLimbs];
};

/* galois_dot_kernel with two sums per output word: x[e] is requested once and enters both. */
__global__ void __launch_bounds__(256) keypair_dot2_kernel(const KKeyPairDot2 k)
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
    uint64_t       hi0  = 0, sum0 = k.accumulate ? k.c[0][dst] : 0;
    uint64_t       hi1  = 0, sum1 = k.accumulate ? k.c[1][dst] : 0;
    int            j    = 0;
    for(; j + 4 <= k.k; j += 4) {
      uint64_t x[4], y0[4], y1[4];
#pragma unroll
      for(int e = 0; e < 4; e++) {
        x[e]  = k.a[j + e][src];
        y0[e] = k.key[0][j + e][kix];
        y1[e] = k.key[1][j + e][kix];
      }
#pragma unroll
      for(int e = 0; e < 4; e++) {
        bconv_mac(hi0, sum0, x[e], y0[e]);
        bconv_mac(hi1, sum1, x[e], y1[e]);
      }
    }
    for(; j < k.k; j++) {
      const uint64_t x = k.a[j][src];
      bconv_mac(hi0, sum0, x, k.key[0][j][kix]);
      bconv_mac(hi1, sum1, x, k.key[1][j][kix]);
    }
    const uint64_t v0 = bconv_reduce(hi0, sum0, d);
    const uint64_t v1 = bconv_reduce(hi1, sum1, d);
    k.c[0][dst]       = v0 >= d.q ? v0 - d.q : v0;
    k.c[1][dst]       = v1 >= d.q ? v1 - d.q : v1;
  }
}

hipError_t launch_galois_dot2(const GaloisDot2Args &da)
{
  if(da.nlimbs < 1 || da.nlimbs > kGaloisLimbs || da.k < 1 || da.k > kGaloisDot || da.logn < 1 || da.logn > 30) return hipErrorInvalidValue;
  KKeyPairDot2 k{};
  for(int j = 0; j < 2; j++) {
    k.c[j] = da.c[j];
    for(int i = 0; i < da.k; i++) k.key[j][i] = da.key[j][i];
  }
  for(int i = 0; i < da.k; i++) k.a[i] = da.a[i];
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
  hipLaunchKernelGGL(keypair_dot2_kernel, dim3(coef_grid(n, da.max_grid), da.nlimbs), dim3(256), 0, da.stream, k);
  return hipGetLastError();
}

} /* namespace ntt */
