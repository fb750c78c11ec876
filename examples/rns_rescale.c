/*
 * rns_rescale.c -- plain-C caller of the RNS rescale on the operand a CKKS library rescales after every multiplication: a ciphertext
 * pair (c0, c1) kept in the NTT domain, each polynomial's limbs side by side ([batch][limb][N], N = 2^13), over a modulus chain of
 * one 60-bit prime followed by five 50-bit primes.  The pair is rescaled twice -- q_5, then q_4 dropped -- with
 *     ntt_rns_rescale_batch_strided(nlimbs, plans, d, N, LIMBS * N, 2, NTT_RESCALE_TRANSFORMED, stream)
 * which runs the inverse transform of the dropped limb once and then, per run of compatible kept limbs, one forward-transform
 * launch that folds the dropped limb in (the 60-bit limb, an integer-policy plan, takes the inverse / element-wise / forward
 * sandwich).  The layout stays as it is: after a rescale the caller simply passes one limb fewer with the same strides.
 * Prints ntt_poly_checksum of every remaining limb of both polynomials (tests/test_gpu_rescale.py checks them against the model).
 *
 *   gcc -O2 -std=gnu11 -Iinclude examples/rns_rescale.c \
 *       -Loptimized-number-theoretic-transform-implementations_amd -lntt_mi355x -o build/rns_rescale
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

enum { LIMBS = 6, POLYS = 2 };

int main(void)
{
  const uint64_t N = 1u << 13, limb_stride = N, poly_stride = (uint64_t)LIMBS * N;
  uint64_t       q[LIMBS];
  ntt_plan *     plans[LIMBS];
  for(int l = 0; l < LIMBS; l++) {
    q[l] = l == 0 ? ntt_find_prime(60, N, 0) : ntt_find_prime(50, N, (unsigned)(l - 1));
    const uint64_t root = ntt_min_root(q[l], N);
    if(!q[l] || !root) return 3;
    CHECK(ntt_plan_create(&plans[l], 0, N, q[l], root, NTT_ARITH_AUTO));
  }
  uint64_t *d = NULL, *d_sum = NULL;
  CHECK(ntt_dev_malloc(0, (void **)&d, (size_t)POLYS * poly_stride * 8));
  CHECK(ntt_dev_malloc(0, (void **)&d_sum, 8));
  /* coefficients: uniform residues, polynomial p's limb l from seed 100 + p */
  for(int p = 0; p < POLYS; p++)
    for(int l = 0; l < LIMBS; l++) CHECK(ntt_fill_uniform(0, d + p * poly_stride + l * limb_stride, N, q[l], 100 + p, 0, NULL));
  CHECK(ntt_rns_fwd_batch_strided(LIMBS, plans, d, limb_stride, poly_stride, POLYS, NULL));
  /* two rescales in the NTT domain: q_5, then q_4 */
  CHECK(ntt_rns_rescale_batch_strided(LIMBS, plans, d, limb_stride, poly_stride, POLYS, NTT_RESCALE_TRANSFORMED, NULL));
  CHECK(ntt_rns_rescale_batch_strided(LIMBS - 1, plans, d, limb_stride, poly_stride, POLYS, NTT_RESCALE_TRANSFORMED, NULL));
  for(int p = 0; p < POLYS; p++) {
    for(int l = 0; l < LIMBS - 2; l++) {
      uint64_t sum = 0;
      CHECK(ntt_poly_checksum(0, d_sum, d + p * poly_stride + l * limb_stride, N, 1, NULL));
      CHECK(ntt_stream_sync(0, NULL));
      CHECK(ntt_d2h(0, &sum, d_sum, 8));
      printf("poly %d limb %d q %llu checksum %016llx\n", p, l, (unsigned long long)q[l], (unsigned long long)sum);
    }
  }
  CHECK(ntt_dev_free(0, d));
  CHECK(ntt_dev_free(0, d_sum));
  for(int l = 0; l < LIMBS; l++) ntt_plan_destroy(plans[l]);
  return 0;
}
