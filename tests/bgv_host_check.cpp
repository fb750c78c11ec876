/* bgv_host_check.cpp -- the host side of the BGV ModDown (csrc/ntt_bgv.h: bgv_scale, bgv_digit1, bgv_sub_plain, bgv_sub_folded, bgv_word
 * and what they call) on vectors written by tests/test_bgv_cpu.py, against unsigned __int128 arithmetic.  Host only, with the
 * sanitizers: hipcc --cuda-host-only -Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined -ffp-contract=off -I csrc (host code only: nothing is built for the GPU).
 *
 *   bgv_host_check FILE      FILE: np  nd  T  K, the np P primes, the nd kept primes,
 *                                  K rows of np source words t_j followed by nd words c_l
 *   prints K rows of nd words: ( c_l - [T]_q (F_l - [h]_q) ) [P^-1]_q mod q_l.
 * Every word is formed four ways -- the definition's order (bgv_sub_plain), the kernels' folded order (bgv_sub_folded), for one prime
 * bgv_digit1, and the definition with % on 128-bit integers -- and the program fails (exit 1) where two of them differ.  The per-call
 * constants are formed here with 128-bit integers, by the formulas of ntt_keyswitch.h / ntt_bgv.h. */
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ntt_bgv.h"

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
  const int      n = (int)rd(f), nd = (int)rd(f);
  const uint64_t T = rd(f), K = rd(f);
  if(n < 1 || n > kBconvLimbs || nd < 1) return 2;
  std::vector<uint64_t> p(n), q(nd);
  for(auto &v : p) v = rd(f);
  for(auto &v : q) v = rd(f);
  /* plain: h = [h]_p, inv = [p^^-1]_p, and [T^-1]_p beside them; folded: h = [h T]_p, inv = [T^-1 p^^-1]_p */
  BconvSrc              plain[kBconvLimbs], fold[kBconvLimbs];
  std::vector<uint64_t> tinv(n), hatinv(n);
  for(int i = 0; i < n; i++) {
    uint64_t hat = 1;
    for(int k = 0; k < n; k++)
      if(k != i) hat = mulmod(hat, p[k] % p[i], p[i]);
    hatinv[i]         = powmod(hat, p[i] - 2, p[i]);
    tinv[i]           = powmod(T % p[i], p[i] - 2, p[i]);
    const uint64_t hp = (p[i] - 1) / 2, inv = mulmod(tinv[i], hatinv[i], p[i]);
    plain[i]          = BconvSrc{p[i], hp, hatinv[i], shoup(hatinv[i], p[i])};
    fold[i]           = BconvSrc{p[i], mulmod(hp, T % p[i], p[i]), inv, shoup(inv, p[i])};
  }
  std::vector<BconvDst> dst(nd), dstT(nd);
  std::vector<BgvScale> ts(nd);
  std::vector<uint64_t> g((size_t)nd * kBconvLimbs), gt((size_t)nd * kBconvLimbs);
  for(int d = 0; d < nd; d++) {
    uint64_t pq = 1;
    for(int i = 0; i < n; i++) pq = mulmod(pq, p[i] % q[d], q[d]);
    BconvDst r{};
    r.q           = q[d];
    r.bar         = ~0ull / q[d];
    const u128 mu = ~(u128)0 / q[d];
    r.mu_lo       = (uint64_t)mu;
    r.mu_hi       = (uint64_t)(mu >> 64);
    r.s           = powmod(pq, q[d] - 2, q[d]);
    r.s_shoup     = shoup(r.s, q[d]);
    r.h           = mulmod((pq + q[d] - 1) % q[d], (q[d] + 1) / 2, q[d]); /* (P - 1) / 2 mod q */
    ts[d]         = BgvScale{T % q[d], shoup(T % q[d], q[d])};
    dst[d]        = r;
    dstT[d]       = r;
    dstT[d].h     = bgv_scale(r.h, ts[d], q[d]);
    if(dstT[d].h != mulmod(r.h, T % q[d], q[d])) return 1;
    for(int i = 0; i < n; i++) {
      uint64_t hat = 1;
      for(int k = 0; k < n; k++)
        if(k != i) hat = mulmod(hat, p[k] % q[d], q[d]);
      g[(size_t)d * kBconvLimbs + i]  = hat;
      gt[(size_t)d * kBconvLimbs + i] = bgv_scale(hat, ts[d], q[d]);
      if(gt[(size_t)d * kBconvLimbs + i] != mulmod(hat, T % q[d], q[d])) return 1;
    }
  }
  std::vector<uint64_t> t(n), tt(n), c(nd);
  for(uint64_t k = 0; k < K; k++) {
    for(auto &v : t) v = rd(f);
    for(auto &v : c) v = rd(f);
    /* the definition's first product as a word of its own: t_j [T^-1]_p, then the plain constants add [h]_p and multiply by [p^^-1]_p */
    for(int i = 0; i < n; i++) tt[i] = mulmod(t[i], tinv[i], p[i]);
    for(int d = 0; d < nd; d++) {
      const uint64_t *gd = &g[(size_t)d * kBconvLimbs], *gtd = &gt[(size_t)d * kBconvLimbs];
      const uint64_t  u0 = bgv_sub_plain(tt.data(), plain, gd, n, dst[d], ts[d]);
      const uint64_t  u1 = bgv_sub_folded(t.data(), fold, gtd, n, dstT[d]);
      /* 128-bit reference: F = sum z_j [p^_j]_q mod q with z_j by %, then the last line of the definition */
      u128 F = 0;
      for(int i = 0; i < n; i++) {
        const uint64_t z = mulmod((tt[i] + (p[i] - 1) / 2) % p[i], hatinv[i], p[i]);
        F                = (F + (u128)z * gd[i]) % q[d];
      }
      const uint64_t u2 = mulmod((uint64_t)((F + q[d] - dst[d].h) % q[d]), T % q[d], q[d]);
      if(u0 != u1 || u0 != u2) {
        fprintf(stderr, "row %" PRIu64 " limb %d: plain %" PRIu64 " folded %" PRIu64 " reference %" PRIu64 "\n", k, d, u0, u1, u2);
        return 1;
      }
      if(n == 1 && bgv_digit1(t[0], fold[0], dstT[d], ts[d]) != u0) {
        fprintf(stderr, "row %" PRIu64 " limb %d: bgv_digit1 differs\n", k, d);
        return 1;
      }
      const uint64_t w = bgv_word(c[d], u0, dst[d]);
      if(w != mulmod((c[d] + q[d] - u0) % q[d], dst[d].s, q[d])) {
        fprintf(stderr, "row %" PRIu64 " limb %d: bgv_word differs\n", k, d);
        return 1;
      }
      printf("%" PRIu64 "%c", w, d + 1 == nd ? '\n' : ' ');
    }
  }
  fclose(f);
  return 0;
}
