/* exact_host_check.cpp -- the host side of the exact base conversion (csrc/ntt_exact.h: exact_bconv, moddown_exact_word and what they
 * call) on vectors written by tests/test_exact_bconv_cpu.py.  Host only: hipcc --cuda-host-only -ffp-contract=off -I csrc.
 *
 *   exact_host_check FILE      FILE: mode (0 conversion, 1 scaled ModDown)  n  nd  mult  K
 *                                    n source primes, nd destination primes,
 *                                    K rows of n source words (mode 1: followed by nd destination words c_l)
 *   prints K rows of nd words: ExactBConv_{B->q_d}([mult x]_B), or c_l [mult B^-1] - that [B^-1] mod q_d.
 * The per-call constants are formed here with 128-bit integers, by the formulas of ntt_keyswitch.h / ntt_exact.h. */
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ntt_exact.h"

using namespace ntt;
typedef unsigned __int128 u128;

static uint64_t mulmod(uint64_t a, uint64_t b, uint64_t q) { return (uint64_t)((u128)a * b % q); }
static uint64_t powmod(uint64_t a, uint64_t e, uint64_t q)
{
  uint64_t r = 1;
  for(a %= q; e; e >>= 1, a = mulmod(a, a, q))
    if(e & 1) r = mulmod(r, a, q);
  return r;
}
static uint64_t shoup(uint64_t w, uint64_t q) { return (uint64_t)(((u128)w << 64) / q); }
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
  const int      mode = (int)rd(f), n = (int)rd(f), nd = (int)rd(f);
  const uint64_t mult = rd(f), K = rd(f);
  if(n < 1 || n > kBconvLimbs || nd < 1) return 2;
  std::vector<uint64_t> b(n), q(nd);
  for(auto &v : b) v = rd(f);
  for(auto &v : q) v = rd(f);
  BconvSrc src[kBconvLimbs];
  double   rho[kBconvLimbs];
  for(int i = 0; i < n; i++) {
    uint64_t hat = 1;
    for(int k = 0; k < n; k++)
      if(k != i) hat = mulmod(hat, b[k] % b[i], b[i]);
    const uint64_t inv = mulmod(n == 1 ? 1 : powmod(hat, b[i] - 2, b[i]), mult % b[i], b[i]);
    src[i]             = BconvSrc{b[i], 0, inv, shoup(inv, b[i])};
    rho[i]             = 1.0 / (double)b[i];
  }
  std::vector<BconvDst>   dst(nd);
  std::vector<ExactScale> es(nd);
  std::vector<uint64_t>   g((size_t)nd * kBconvLimbs);
  for(int d = 0; d < nd; d++) {
    uint64_t bq = 1;
    for(int i = 0; i < n; i++) {
      uint64_t hat = 1;
      for(int k = 0; k < n; k++)
        if(k != i) hat = mulmod(hat, b[k] % q[d], q[d]);
      g[(size_t)d * kBconvLimbs + i] = hat;
      bq                             = mulmod(bq, b[i] % q[d], q[d]);
    }
    BconvDst r{};
    r.q        = q[d];
    r.bar      = ~0ull / q[d];
    const u128 mu = ~(u128)0 / q[d];
    r.mu_lo    = (uint64_t)mu;
    r.mu_hi    = (uint64_t)(mu >> 64);
    r.s        = powmod(bq, q[d] - 2, q[d]);
    r.s_shoup  = shoup(r.s, q[d]);
    r.h        = q[d] - bq;
    dst[d]     = r;
    es[d].ms   = mulmod(r.s, mult % q[d], q[d]);
    es[d].ms_shoup = shoup(es[d].ms, q[d]);
  }
  std::vector<uint64_t> x(n), c(nd);
  for(uint64_t k = 0; k < K; k++) {
    for(auto &v : x) v = rd(f);
    if(mode)
      for(auto &v : c) v = rd(f);
    for(int d = 0; d < nd; d++) {
      const uint64_t u = exact_bconv(x.data(), src, rho, &g[(size_t)d * kBconvLimbs], n, dst[d]);
      printf("%" PRIu64 "%c", mode ? moddown_exact_word(c[d], u, dst[d], es[d]) : u, d + 1 == nd ? '\n' : ' ');
    }
  }
  fclose(f);
  return 0;
}
