/*
 * ntt_slots.h -- BFV / BGV slot encode and decode: the slot order, stated once for the host, the kernels and the tests, and the
 * launchers the host layer sees (host/host_slots.inc).  The kernels are in slots.hip and the slots_f64*.hip units.
 *
 * A plan for (N, t, psi), m = log2 N, h = N / 2.  The forward transform stores a(psi^(2 bitrev_m(s) + 1)) at word s.
 *   slot index   i = r h + j, row r in {0, 1}, column 0 <= j < h
 *   exponent     e(i) = 5^j mod 2N (r = 0),  2N - (5^j mod 2N) (r = 1)
 *   position     pos(i) = bitrev_m((e(i) - 1) / 2): a permutation of 0..N-1 (the identity for N = 2); ipos is its inverse
 *   decode       v[i] = fwd(a)[pos(i)] = a(psi^e(i))
 *   encode       a = inv(a^),  a^[pos(i)] = v[i],  i.e.  a^[s] = v[ipos(s)]
 * So sigma_g with g = 5^r rotates both rows left by r (new (row, j) holds the old (row, (j + r) mod h)), g = 2N - 1 swaps the rows,
 * and products of polynomials are slot-wise products.
 */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ntt_keyswitch.h" /* (the policies; coef_grid) */

namespace ntt {

/* 5^j mod 2N by square-and-multiply in wrapping arithmetic masked to 2N (2N a power of two: the mask is the reduction) */
NTT_HD uint64_t slot_pow5(uint64_t j, uint64_t two_n)
{
  const uint64_t mask = two_n - 1;
  uint64_t       b = 5 & mask, x = 1 & mask;
  for(; j; j >>= 1) {
    if(j & 1) x = (x * b) & mask;
    b = (b * b) & mask;
  }
  return x;
}

/* pos(i) for N = 2^m, i < N */
NTT_HD uint64_t slot_position(unsigned m, uint64_t i)
{
  const uint64_t N = 1ull << m, h = N >> 1;
  const uint64_t r = i >= h ? 1 : 0, j = i - r * h;
  uint64_t       e = slot_pow5(j, 2 * N);
  if(r) e = 2 * N - e;
  uint64_t x = (e - 1) >> 1, y = 0;
  for(unsigned b = 0; b < m; b++) {
    y = (y << 1) | (x & 1);
    x >>= 1;
  }
  return y;
}

/* pos[i] = slot_position(m, i) and ipos[pos[i]] = i for i < 2^logn, one thread per slot (slots_table_kernel) */
hipError_t launch_slots_tables(uint32_t *pos, uint32_t *ipos, uint32_t logn, hipStream_t stream);

/* the composition's half: out[p][s] = in[p][tab[s]], p < batch, s < 2^logn (slots_perm_kernel), every policy and every N >= 2 */
struct SlotsPermArgs {
  uint64_t *      out;
  const uint64_t *in;
  const uint32_t *tab; /* N entries below N */
  uint64_t        out_stride, in_stride, batch;
  uint32_t        logn;
  int             max_grid;
  hipStream_t     stream;
};
hipError_t launch_slots_perm(const SlotsPermArgs &sa);

/* the fused route, FP64 policies, N = 2^6..2^14, ONE launch: encode -- a = inv(a^), a^[s] = v[ipos[s]] (slots_inv_kernel);
 * decode -- v[ipos[s]] = fwd(a)[s] (slots_fwd_kernel; a is read only) */
struct SlotsArgs {
  uint64_t *      a;     /* coefficients: written by encode, read by decode */
  uint64_t *      v;     /* slots: read by encode, written by decode        */
  const uint32_t *ipos;
  const void *    limb;  /* HOST copy of the plan's LimbRec<A>              */
  uint64_t        a_stride, v_stride, batch;
  uint32_t        logn;
  bool            encode;
  int             max_grid, num_cus;
  hipStream_t     stream;
};
template <class A, int KSH> hipError_t launch_slots(const SlotsArgs &sa);
template <> hipError_t launch_slots<ArithF64, 0>(const SlotsArgs &);
template <> hipError_t launch_slots<ArithF64, 1>(const SlotsArgs &);
template <> hipError_t launch_slots<ArithF64, 18>(const SlotsArgs &);
template <> hipError_t launch_slots<ArithF64W, 0>(const SlotsArgs &);

} // namespace ntt
