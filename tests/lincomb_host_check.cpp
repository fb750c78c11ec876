/* lincomb_host_check.cpp -- the host side of the RNS linear combination (csrc/ntt_lincomb.h: lincomb_word and what it calls, bconv_mac and
 * bconv_reduce) on vectors written by tests/test_lincomb_cpu.py, against unsigned __int128 arithmetic.  Host only, with the sanitizers:
 * hipcc --cuda-host-only -Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined -ffp-contract=off -I csrc (host code only:
 * nothing is built for the GPU).
 *
 *   lincomb_host_check FILE      FILE: nl  k  K, the nl primes,
 *                                      K rows of nl groups: c  bias  x_0 .. x_{k-1}  mu_0 .. mu_{k-1}
 *   prints K rows of nl words: ( c + bias + sum_i x_i mu_i ) mod q_l.
 * Every word is formed twice -- lincomb_word, in the kernel's operation order, and the definition with % on the 128-bit integer (the
 * caller keeps the sum below 2^128: the bounds of ntt_lincomb.h) -- and the program fails (exit 1) where they differ.  The Barrett
 * constants are formed here with 128-bit integers, by the formulas of ntt_keyswitch.h. */
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ntt_lincomb.h"

using namespace ntt;
typedef unsigned __int128 u128;

static uint64_t rd(FILE *f)
{
  uint64_t v = 0;
  if(fscanf(f, "%" SCNu64, &v) != 1) {
    fprintf(stderr, "short input\n");
    exit(2);
  }
  return v;
}

int main(int argc, char **argv)
{
  if(argc != 2) return 2;
  FILE *f = fopen(argv[1], "r");
  if(!f) return 2;
  const int      nl = (int)rd(f), k = (int)rd(f);
  const uint64_t K  = rd(f);
  if(nl < 1 || k < 1 || k > kLincombTerms) return 2;
  std::vector<BconvDst> dst(nl);
  for(auto &d : dst) {
    d          = BconvDst{};
    d.q        = rd(f);
    d.bar      = ~0ull / d.q;
    const u128 mu = ~(u128)0 / d.q;
    d.mu_lo    = (uint64_t)mu;
    d.mu_hi    = (uint64_t)(mu >> 64);
  }
  std::vector<uint64_t> x(k), mu(k);
  for(uint64_t r = 0; r < K; r++) {
    for(int l = 0; l < nl; l++) {
      const uint64_t c = rd(f), bias = rd(f);
      for(auto &v : x) v = rd(f);
      for(auto &v : mu) v = rd(f);
      const uint64_t got = lincomb_word(c, bias, x.data(), mu.data(), k, dst[l]);
      u128           sum = (u128)c + bias;
      for(int i = 0; i < k; i++) sum += (u128)x[i] * mu[i];
      const uint64_t want = (uint64_t)(sum % dst[l].q);
      if(got != want) {
        fprintf(stderr, "row %" PRIu64 " limb %d: lincomb_word %" PRIu64 " reference %" PRIu64 "\n", r, l, got, want);
        return 1;
      }
      printf("%" PRIu64 "%c", got, l + 1 == nl ? '\n' : ' ');
    }
  }
  fclose(f);
  return 0;
}
