/*
 * rns_key_switch_pair.c -- a hybrid key switch that produces the actual PAIR (c0, c1): examples/rns_key_switch.c's parameters (N = 2^13,
 * Q = one 60-bit and seven 50-bit primes, P = two 60-bit primes, four digits of two Q limbs), ONE input polynomial, and a
 * key-switching key of two polynomials per digit.  The accumulator is a [2][limb][N] buffer, c1 = c0 + LIMBS N.  Per digit k the
 * digit's limbs (coefficients) are placed in a 10-limb buffer, whose other slots are scratch, and
 *         ntt_rns_mod_up_mul_pair_batch_strided(10, plans, c0, c1, ext, 2k, 2, key0_k, key1_k, N, 10 N, 1,
 *                                               NTT_MUL_ACCUMULATE | NTT_MUL_B_BROADCAST, stream)
 * extends it to every other prime of Q u P once, transforms it once and multiplies it into both NTT-domain accumulators.  Then ONE
 *         ntt_rns_mod_down_batch_strided(8, 2, plans, c0, N, 10 N, 2, NTT_MODDOWN_TRANSFORMED, stream)
 * over both components (batch 2).  Prints ntt_poly_checksum of each remaining limb of c0 and c1 (tests/test_gpu_key_pair.py compares
 * them with the model).
 *
 *   gcc -O2 -std=gnu11 -Iinclude examples/rns_key_switch_pair.c \
 *       -Loptimized-number-theoretic-transform-implementations_amd -lntt_mi355x -o build/rns_key_switch_pair
 */
#include <stdint.h>
#include <stdio.h>

#include "ntt_mi355x.h"

#define CHECK(call)                                                              \
  do {                                                                           \
    int rc_ = (call);                                                            \
    if(rc_ != NTT_OK) {                                                          \
      fprintf(stderr, "%s failed (%d): %s\n", #call, rc_, ntt_last_error());    \
      return 1;                                                                  \
    }                                                                            \
  } while(0)

enum { NQ = 8, NP = 2, LIMBS = NQ + NP, DIGITS = 4, ALPHA = 2 };

int main(void)
{
  const uint64_t N = 1u << 13, limb_stride = N, poly_stride = (uint64_t)LIMBS * N;
  uint64_t       q[LIMBS];
  ntt_plan *     plans[LIMBS];
  for(int l = 0; l < LIMBS; l++) {
    /* Q: 60, 50 x 7; P: the next two 60-bit primes */
    q[l] = l == 0 ? ntt_find_prime(60, N, 0) : l < NQ ? ntt_find_prime(50, N, (unsigned)(l - 1)) : ntt_find_prime(60, N, (unsigned)(l - NQ + 1));
    const uint64_t root = ntt_min_root(q[l], N);
    if(!q[l] || !root) return 3;
    CHECK(ntt_plan_create(&plans[l], 0, N, q[l], root, NTT_ARITH_AUTO));
  }
  uint64_t *ext = NULL, *acc = NULL, *key = NULL, *d_sum = NULL;
  CHECK(ntt_dev_malloc(0, (void **)&ext, (size_t)poly_stride * 8));
  CHECK(ntt_dev_malloc(0, (void **)&acc, (size_t)2 * poly_stride * 8)); /* [2][limb][N]: c0, c1 */
  CHECK(ntt_dev_malloc(0, (void **)&key, (size_t)2 * LIMBS * N * 8));   /* [2][limb][N]: key0_k, key1_k */
  CHECK(ntt_dev_malloc(0, (void **)&d_sum, 8));
  uint64_t *const c0 = acc, *const c1 = acc + poly_stride;
  uint64_t *const key0 = key, *const key1 = key + (uint64_t)LIMBS * N;
  for(int k = 0; k < DIGITS; k++) {
    /* the digit's limbs, in coefficients */
    for(int l = ALPHA * k; l < ALPHA * (k + 1); l++) CHECK(ntt_fill_uniform(0, ext + l * limb_stride, N, q[l], 100 + l, 0, NULL));
    /* key k: two NTT-domain polynomials per limb, each [limb][N] */
    for(int l = 0; l < LIMBS; l++) {
      CHECK(ntt_fill_uniform(0, key0 + l * N, N, q[l], 1000 + 16 * k + l, 0, NULL));
      CHECK(ntt_fill_uniform(0, key1 + l * N, N, q[l], 2000 + 16 * k + l, 0, NULL));
    }
    const unsigned flags = NTT_MUL_B_BROADCAST | (k ? NTT_MUL_ACCUMULATE : 0);
    CHECK(ntt_rns_mod_up_mul_pair_batch_strided(LIMBS, plans, c0, c1, ext, ALPHA * k, ALPHA, key0, key1, limb_stride, poly_stride, 1, flags, NULL));
  }
  /* both components at once: c1 is the second polynomial of the [2][limb][N] buffer */
  CHECK(ntt_rns_mod_down_batch_strided(NQ, NP, plans, acc, limb_stride, poly_stride, 2, NTT_MODDOWN_TRANSFORMED, NULL));
  for(int p = 0; p < 2; p++) {
    for(int l = 0; l < NQ; l++) {
      uint64_t sum = 0;
      CHECK(ntt_poly_checksum(0, d_sum, acc + p * poly_stride + l * limb_stride, N, 1, NULL));
      CHECK(ntt_stream_sync(0, NULL));
      CHECK(ntt_d2h(0, &sum, d_sum, 8));
      printf("comp %d limb %d q %llu checksum %016llx\n", p, l, (unsigned long long)q[l], (unsigned long long)sum);
    }
  }
  CHECK(ntt_dev_free(0, ext));
  CHECK(ntt_dev_free(0, acc));
  CHECK(ntt_dev_free(0, key));
  CHECK(ntt_dev_free(0, d_sum));
  for(int l = 0; l < LIMBS; l++) ntt_plan_destroy(plans[l]);
  return 0;
}
