/*
 * ntt_lincomb.h -- the RNS linear combination with a Galois map and a multiplier per term (ntt_rns_lincomb_batch): the argument
 * record and the launcher of lincomb_kernel (lincomb.hip), the host layer's view of it, and one output word stated for host and
 * device (lincomb_word).
 *
 * Per limb l (prime q = q_l < 2^61), polynomial p and storage slot s:
 *   c[l,p,s] = ( [accumulate: c[l,p,s]] + bias_l + sum_{i<k} a_i[l,p,src_{g_i}(s)] * mu_i(l,p,s) ) mod q,   canonical,
 *   mu_i     = m_i[l,p,s] (m_i[l,s] when the multipliers are shared by the batch) where term i has a polynomial multiplier,
 *              the scalar s_{i,l} otherwise,
 *   src_g    = galois_ntt_src (ntt_galois.h; the identity for g = 1).
 * The sum is the exact integer in 128 bits (bconv_mac), reduced once (bconv_reduce: any 128-bit input, odd q < 2^63, result in
 * [0, 2q)), then one conditional subtraction: every output word is the one canonical residue.
 *   canonical inputs   k <= 16: 16 (2^61)^2 + 2^61 + 2^61 < 2^127
 *   lazy a_i (< 4q)    k <= 8:  a_i < 2^63, the multipliers, scalars, bias and c canonical: 8 2^63 2^61 + 2^62 <= 2^127 + 2^62 < 2^128
 */
#pragma once
#include "ntt_galois.h"

namespace ntt {

constexpr int kLincombLimbs = 16; /* limbs of one launch (blockIdx.y) */
constexpr int kLincombTerms = 16; /* terms of one call */

/* one output word in the kernel's operation order: the accumulator starts as c + bias (both canonical: below 2^62), the k products
 * enter it in term order, one Barrett reduction, one conditional subtraction.  x[i] is the (permuted) word of a_i, mu[i] its
 * multiplier; c_in is 0 where the call does not accumulate. */
NTT_HD uint64_t lincomb_word(uint64_t c_in, uint64_t bias, const uint64_t *x, const uint64_t *mu, int k, const BconvDst &d)
{
  uint64_t hi = 0, lo = c_in + bias;
  for(int i = 0; i < k; i++) bconv_mac(hi, lo, x[i], mu[i]);
  const uint64_t v = bconv_reduce(hi, lo, d);
  return v >= d.q ? v - d.q : v;
}

/* term i of the call: the run's first limb of a_i, of its polynomial multiplier (nullptr: the scalars[i][] are the multiplier),
 * and the Galois element */
struct LincombTerm {
  const uint64_t *a;
  const uint64_t *m;
  uint32_t        g, pad;
};

/* c (+)= bias + sum_i sigma_{g_i}(a_i) * mu_i over a run of up to 16 limbs and the whole batch (lincomb_kernel; lincomb.hip).  The
 * multipliers have strides of their own (shared by the batch: limb stride N, polynomial stride 0). */
struct LincombArgs {
  uint64_t *  c; /* the run's first limb */
  LincombTerm t[kLincombTerms];
  int         k;
  uint64_t    limb_stride, poly_stride, m_limb_stride, m_poly_stride, batch;
  uint32_t    logn;
  int         nlimbs;
  bool        accumulate;
  uint64_t    scalars[kLincombTerms][kLincombLimbs]; /* [term][limb of the run], canonical */
  BconvDst    ql[kLincombLimbs];                     /* q, floor(2^64 / q), floor(2^128 / q) */
  uint64_t    bias[kLincombLimbs];                   /* canonical */
  int         max_grid;
  hipStream_t stream;
};
hipError_t launch_lincomb(const LincombArgs &la);

} // namespace ntt
