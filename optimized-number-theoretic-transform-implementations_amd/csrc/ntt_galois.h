/*
 * ntt_galois.h -- launchers of the Galois automorphism kernels (ntt_galois_batch, ntt_rns_galois_batch, ntt_rns_galois_dot_batch):
 * the host layer's view of them, and the index functions the kernels, the host checks and the CPU tests share.
 *
 * The kernels live in galois_coef.hip (galois_ntt_kernel, galois_dot_kernel, galois_coef_kernel) and in keypair_dot2.hip (keypair_dot2_kernel); this header declares the argument
 * records and the launchers, nothing that the host translation unit would instantiate.
 *
 * sigma_g(a)(X) = a(X^g) in Z_q[X] / (X^N + 1), g odd, 0 < g < 2N, N = 2^m.
 *   coefficients   a[i] goes to position g i mod N, negated when (g i mod 2N) >= N.  Read from the output's side, with
 *                  u = g^-1 t mod 2N: out[t] = a[u] for u < N, q - a[u - N] (0 stays 0) otherwise -- galois_coef_src.
 *   NTT domain     storage slot s holds the evaluation at psi^(2i+1), i = bitrev_m(s) (as ntt_fwd_batch leaves it).  sigma_g(a) at
 *                  psi^(2i+1) is a at psi^(g(2i+1)) = psi^(2j+1) with j = (g i + (g - 1) / 2) mod N: out[s] = in[bitrev_m(j)], a
 *                  permutation of words -- galois_ntt_src.
 * The map i -> j is affine mod 2^m: the low k bits of j depend on the low k bits of i alone, which are the HIGH k bits of the
 * slots.  So the 2^b outputs of one aligned storage tile come from exactly one aligned storage tile of the input, for every b: a
 * wavefront that writes 64 consecutive slots reads one aligned 512-byte block, every byte of it; an aligned pair of slots (b = 1)
 * comes from an aligned pair, possibly swapped: slot s ^ 1 flips the top bit of i, which adds g N / 2 = N / 2 (mod N) to j and
 * flips the low bit of the source slot.
 */
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ntt_keyswitch.h"

namespace ntt {

constexpr int kGaloisLimbs = kBconvLimbs; /* limbs of one launch */
constexpr int kGaloisDot   = 32;          /* operand pairs of the rotation key product (= kMaxDot) */

/* the low m bits of x reversed, 1 <= m <= 32 */
NTT_HD uint32_t galois_bitrev(uint32_t x, uint32_t m)
{
#if defined(__HIP_DEVICE_COMPILE__)
  return __brev(x) >> (32u - m);
#else
  x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
  x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);
  x = ((x >> 4) & 0x0F0F0F0Fu) | ((x & 0x0F0F0F0Fu) << 4);
  x = ((x >> 8) & 0x00FF00FFu) | ((x & 0x00FF00FFu) << 8);
  x = (x >> 16) | (x << 16);
  return x >> (32u - m);
#endif
}

/* NTT domain: the storage slot whose word output slot s receives; s < N = 2^m, 1 <= m <= 31, g odd (arithmetic mod 2^32: exact
 * mod 2^m) */
NTT_HD uint32_t galois_ntt_src(uint32_t s, uint32_t g, uint32_t m)
{
  const uint32_t i = galois_bitrev(s, m);
  const uint32_t j = (g * i + (g >> 1)) & ((1u << m) - 1u);
  return galois_bitrev(j, m);
}

/* coefficients: u = g^-1 t mod 2N for output position t < N = 2^m, m <= 30: the source position is u & (N - 1), the word is
 * negated when u >= N (bit m of the result) */
NTT_HD uint32_t galois_coef_src(uint32_t t, uint32_t ginv, uint32_t m) { return (ginv * t) & ((2u << m) - 1u); }

/* g^-1 mod 2^32 for odd g (Newton: g g = 1 mod 8, so g is its own inverse to 3 bits, and every step doubles them); the caller
 * reduces mod 2N */
NTT_HD uint32_t galois_inverse(uint32_t g)
{
  uint32_t x = g;
  for(int it = 0; it < 4; it++) x *= 2u - g * x; /* 6, 12, 24, 48 bits */
  return x;
}

/* sigma_g over a run of up to 16 limbs and the whole batch.  NTT domain (galois_ntt_kernel): words copied bit for bit;
 * coefficients (galois_coef_kernel): canonical words in, canonical words out, q[l] the limbs' primes. */
struct GaloisArgs {
  uint64_t *      out; /* the run's first limb */
  const uint64_t *in;
  uint64_t        limb_stride, poly_stride, batch;
  uint32_t        logn, g;
  int             nlimbs;
  bool            ntt_domain;
  uint64_t        q[kGaloisLimbs]; /* coefficients only */
  int             max_grid;
  hipStream_t     stream;
};
hipError_t launch_galois(const GaloisArgs &ga);

/* the rotation key product over a run of up to 16 limbs (galois_dot_kernel):
 *   c[s] (+)= sum_{i<k} a_i[galois_ntt_src(s)] * key_i[s] mod q_l,
 * the keys with strides of their own (a broadcast key: limb stride N, polynomial stride 0) */
struct GaloisDotArgs {
  uint64_t *      c; /* the run's first limb, as every a[i] and key[i] */
  const uint64_t *a[kGaloisDot];
  const uint64_t *key[kGaloisDot];
  int             k;
  uint64_t        limb_stride, poly_stride, key_limb_stride, key_poly_stride, batch;
  uint32_t        logn, g;
  int             nlimbs;
  bool            accumulate;
  BconvDst        ql[kGaloisLimbs]; /* q, floor(2^64 / q), floor(2^128 / q) */
  int             max_grid;
  hipStream_t     stream;
};
hipError_t launch_galois_dot(const GaloisDotArgs &da);

/* the rotation key product for both components of the key (keypair_dot2_kernel):
 *   c_j[s] (+)= sum_{i<k} a_i[galois_ntt_src(s)] * key_j,i[s] mod q_l,  j = 0, 1,
 * every permuted digit word loaded once */
struct GaloisDot2Args {
  uint64_t *      c[2]; /* the run's first limb, as every a[i] and key[j][i] */
  const uint64_t *a[kGaloisDot];
  const uint64_t *key[2][kGaloisDot];
  int             k;
  uint64_t        limb_stride, poly_stride, key_limb_stride, key_poly_stride, batch;
  uint32_t        logn, g;
  int             nlimbs;
  bool            accumulate;
  BconvDst        ql[kGaloisLimbs];
  int             max_grid;
  hipStream_t     stream;
};
hipError_t launch_galois_dot2(const GaloisDot2Args &da);

} // namespace ntt
