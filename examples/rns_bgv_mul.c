/*
 * rns_bgv_mul.c -- one complete BGV multiplication (tensor, relinearisation, modulus switch) on ciphertexts held in the NTT domain,
 * through public calls only: examples/rns_ciphertext_mul.c with the two divisions replaced by the ones that keep the plaintext mod T.
 * N = 2^13, Q = one 60-bit and seven 50-bit primes, P = two 60-bit primes, four digits of two Q limbs, T = 65537.  The ciphertexts
 * (a0, a1) and (b0, b1) are [limb][N] over Q; d is a [3][8][N] buffer (d0, d1, d2), the accumulator a [2][10][N] buffer (acc0, acc1).
 * The tensor, the approximate ModUp and the key products are scheme-agnostic (BGV keys carry noise T e; the ModUp overshoot cancels
 * mod QP).
 *   1  ntt_rns_tensor_batch_strided(8, plans, d0, d1, d2, a0, a1, b0, b1, N, 8 N, 1, 0, stream)       (d0, d1, d2) = (a0, a1) (x) (b0, b1)
 *   2  ntt_rns_inv_batch_strided(8, plans, d2, N, 8 N, 1, stream)                                     d2 to coefficients
 *   3  per digit k: its two limbs of d2 into a 10-limb buffer whose other slots are scratch, then
 *      ntt_rns_mod_up_mul_pair_batch_strided(10, plans, acc0, acc1, ext, 2k, 2, key0_k, key1_k, N, 10 N, 1, flags, stream)
 *   4  ntt_rns_mod_down_bgv_add_batch_strided(8, 2, plans, d, acc, T, N, 8 N, N, 10 N, 2,
 *                                             NTT_MODDOWN_TRANSFORMED | NTT_MODDOWN_ACCUMULATE, stream)  (d0, d1) += ModDown_T(acc0, acc1)
 *   5  ntt_rns_mod_down_bgv_batch_strided(7, 1, plans, d, T, N, 8 N, 2, NTT_MODDOWN_TRANSFORMED, stream)  switch by the last Q prime
 * Step 4 leaves the plaintext as it is (the key's P s^2 term divides exactly); step 5 multiplies it by q_7^-1 mod T, which the caller
 * tracks.  Prints ntt_poly_checksum of each remaining limb of d0 and d1 (tests/test_gpu_bgv.py compares them with the model).
 *
 *   gcc -O2 -std=gnu11 -Iinclude examples/rns_bgv_mul.c \
 *       -Loptimized-number-theoretic-transform-implementations_amd -lntt_mi355x -o build/rns_bgv_mul
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
  const uint64_t N = 1u << 13, T = 65537, ct_poly = (uint64_t)NQ * N, acc_poly = (uint64_t)LIMBS * N;
  uint64_t       q[LIMBS];
  ntt_plan *     plans[LIMBS];
  for(int l = 0; l < LIMBS; l++) {
    /* Q: 60, 50 x 7; P: the next two 60-bit primes */
    q[l] = l == 0 ? ntt_find_prime(60, N, 0) : l < NQ ? ntt_find_prime(50, N, (unsigned)(l - 1)) : ntt_find_prime(60, N, (unsigned)(l - NQ + 1));
    const uint64_t root = ntt_min_root(q[l], N);
    if(!q[l] || !root) return 3;
    CHECK(ntt_plan_create(&plans[l], 0, N, q[l], root, NTT_ARITH_AUTO));
  }
  uint64_t *in = NULL, *d = NULL, *ext = NULL, *acc = NULL, *key = NULL, *d_sum = NULL;
  CHECK(ntt_dev_malloc(0, (void **)&in, (size_t)4 * ct_poly * 8));   /* [4][limb][N]: a0, a1, b0, b1 */
  CHECK(ntt_dev_malloc(0, (void **)&d, (size_t)3 * ct_poly * 8));    /* [3][limb][N]: d0, d1, d2 */
  CHECK(ntt_dev_malloc(0, (void **)&ext, (size_t)acc_poly * 8));
  CHECK(ntt_dev_malloc(0, (void **)&acc, (size_t)2 * acc_poly * 8)); /* [2][limb][N] over Q u P: acc0, acc1 */
  CHECK(ntt_dev_malloc(0, (void **)&key, (size_t)2 * acc_poly * 8)); /* [2][limb][N]: key0_k, key1_k */
  CHECK(ntt_dev_malloc(0, (void **)&d_sum, 8));
  uint64_t *const d2 = d + 2 * ct_poly, *const key0 = key, *const key1 = key + acc_poly;
  /* the operands, NTT domain: any canonical words are the transform of some polynomial */
  for(int j = 0; j < 4; j++)
    for(int l = 0; l < NQ; l++) CHECK(ntt_fill_uniform(0, in + j * ct_poly + l * N, N, q[l], (uint64_t)(100 + 16 * j + l), 0, NULL));
  CHECK(ntt_rns_tensor_batch_strided(NQ, plans, d, d + ct_poly, d2, in, in + ct_poly, in + 2 * ct_poly, in + 3 * ct_poly, N, ct_poly, 1, 0, NULL));
  CHECK(ntt_rns_inv_batch_strided(NQ, plans, d2, N, ct_poly, 1, NULL));
  for(int k = 0; k < DIGITS; k++) {
    /* the digit's two limbs of d2 (adjacent: limb stride N) into the extended operand */
    CHECK(ntt_copy_probe(0, ext + (uint64_t)ALPHA * k * N, d2 + (uint64_t)ALPHA * k * N, ALPHA * N, NULL));
    for(int l = 0; l < LIMBS; l++) {
      CHECK(ntt_fill_uniform(0, key0 + l * N, N, q[l], (uint64_t)(1000 + 16 * k + l), 0, NULL));
      CHECK(ntt_fill_uniform(0, key1 + l * N, N, q[l], (uint64_t)(1500 + 16 * k + l), 0, NULL));
    }
    const unsigned flags = NTT_MUL_B_BROADCAST | (k ? NTT_MUL_ACCUMULATE : 0);
    CHECK(ntt_rns_mod_up_mul_pair_batch_strided(LIMBS, plans, acc, acc + acc_poly, ext, ALPHA * k, ALPHA, key0, key1, N, acc_poly, 1, flags, NULL));
  }
  /* both components at once: (d0, d1) are the first two polynomials of d, (acc0, acc1) those of acc */
  CHECK(ntt_rns_mod_down_bgv_add_batch_strided(NQ, NP, plans, d, acc, T, N, ct_poly, N, acc_poly, 2, NTT_MODDOWN_TRANSFORMED | NTT_MODDOWN_ACCUMULATE, NULL));
  /* the modulus switch: the first NQ plans with the last of them as the one divided-out prime */
  CHECK(ntt_rns_mod_down_bgv_batch_strided(NQ - 1, 1, plans, d, T, N, ct_poly, 2, NTT_MODDOWN_TRANSFORMED, NULL));
  for(int p = 0; p < 2; p++) {
    for(int l = 0; l < NQ - 1; l++) {
      uint64_t sum = 0;
      CHECK(ntt_poly_checksum(0, d_sum, d + p * ct_poly + l * N, N, 1, NULL));
      CHECK(ntt_stream_sync(0, NULL));
      CHECK(ntt_d2h(0, &sum, d_sum, 8));
      printf("comp %d limb %d q %llu checksum %016llx\n", p, l, (unsigned long long)q[l], (unsigned long long)sum);
    }
  }
  CHECK(ntt_dev_free(0, in));
  CHECK(ntt_dev_free(0, d));
  CHECK(ntt_dev_free(0, ext));
  CHECK(ntt_dev_free(0, acc));
  CHECK(ntt_dev_free(0, key));
  CHECK(ntt_dev_free(0, d_sum));
  for(int l = 0; l < LIMBS; l++) ntt_plan_destroy(plans[l]);
  return 0;
}
