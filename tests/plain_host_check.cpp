/* plain_host_check.cpp -- the host side of the conversions out of the RNS (csrc/ntt_plain.h: plain_word, plain_double and what they
 * call) on vectors written by tests/test_plain_cpu.py.  Host only, with the sanitizers: hipcc --cuda-host-only -Xarch_host
 * -fsanitize=address -Xarch_host -fsanitize=undefined -ffp-contract=off -I csrc (host code only: nothing is built for the GPU).
 *
 *   plain_host_check FILE
 *     FILE: "P" nl t h K, nl rows  q_i c_i g_i,  K rows of nl words          prints K words: plain_word
 *           "D" nl scale_bits K, nl rows  q_i c_i (c_i = [q_{1-i}^-1]_{q_i}; 0 for one limb),  K rows of nl words
 *                                                                            prints K bit patterns: plain_double
 * The Shoup words, rho_i = 1.0 / (double)q_i and floor(2^128 / t) are formed here with 128-bit integers, by the formulas of
 * host/host_plain.inc.  For "P" the 128-bit sum is formed a second time with unsigned __int128 and % t, from the same digits and the
 * same v, and the program fails (exit 1) where bconv_reduce's word differs; the test compares the output with the model. */
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ntt_plain.h"

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

static uint64_t shoup(uint64_t w, uint64_t q) { return (uint64_t)(((u128)w << 64) / q); }

int main(int argc, char **argv)
{
  if(argc != 2) return 2;
  FILE *f = fopen(argv[1], "r");
  if(!f) return 2;
  char mode[4] = {0};
  if(fscanf(f, "%1s", mode) != 1) return 2;
  const int nl = (int)rd(f);
  if(mode[0] == 'P') {
    if(nl < 1 || nl > kPlainLimbs) return 2;
    const uint64_t t = rd(f), h = rd(f), K = rd(f);
    PlainConsts    k{};
    const u128     all = ~(u128)0, mu = all / t + (all % t == t - 1 ? 1u : 0u);
    k.d.q     = t;
    k.d.mu_lo = (uint64_t)mu;
    k.d.mu_hi = (uint64_t)(mu >> 64);
    k.d.h     = h;
    for(int i = 0; i < nl; i++) {
      const uint64_t q = rd(f), c = rd(f), g = rd(f);
      k.l[i] = PlainLimb{q, c, shoup(c, q), g, 1.0 / (double)q};
    }
    std::vector<uint64_t> x(nl);
    for(uint64_t r = 0; r < K; r++) {
      for(auto &v : x) v = rd(f);
      const uint64_t got = plain_word(x.data(), nl, k);
      /* the same digits and v, summed and reduced by the compiler's 128-bit arithmetic */
      u128   sum = 0;
      double s   = 0.0;
      for(int i = 0; i < nl; i++) {
        const uint64_t z  = (uint64_t)((u128)x[i] * k.l[i].inv % k.l[i].p);
        const double   fz = (double)z * k.l[i].rho;
        s                 = i ? s + fz : fz;
        sum += (u128)z * k.l[i].g;
      }
      sum += (u128)(uint64_t)__builtin_rint(s) * h;
      const uint64_t want = (uint64_t)(sum % t);
      if(got != want) {
        fprintf(stderr, "row %" PRIu64 ": plain_word %" PRIu64 " reference %" PRIu64 "\n", r, got, want);
        return 1;
      }
      printf("%" PRIu64 "\n", got);
    }
  } else if(mode[0] == 'D') {
    if(nl < 1 || nl > 2) return 2;
    const uint64_t sb = rd(f), K = rd(f);
    DoubleConsts   k{};
    memcpy(&k.scale, &sb, 8);
    uint64_t q[2] = {0, 0};
    for(int i = 0; i < nl; i++) {
      q[i]           = rd(f);
      const uint64_t c = rd(f);
      k.sl[i]        = BconvSrc{q[i], 0, c, shoup(c, q[i])};
    }
    const u128 Q = nl == 2 ? (u128)q[0] * q[1] : (u128)q[0];
    k.q_lo       = (uint64_t)Q;
    k.q_hi       = (uint64_t)(Q >> 64);
    for(uint64_t r = 0; r < K; r++) {
      const uint64_t x0 = rd(f), x1 = nl == 2 ? rd(f) : 0;
      const double   y  = plain_double(x0, x1, nl, k);
      uint64_t       b;
      memcpy(&b, &y, 8);
      printf("%" PRIu64 "\n", b);
    }
  } else return 2;
  fclose(f);
  return 0;
}
