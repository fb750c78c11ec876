/* lift_host_check.cpp -- the host side of the lifts into the RNS (csrc/ntt_lift.h: lift_word, lift_digit and what they call) on
 * vectors written by tests/test_lift_cpu.py.  Host only, with the sanitizers: hipcc --cuda-host-only -Xarch_host -fsanitize=address
 * -Xarch_host -fsanitize=undefined -ffp-contract=off -I csrc (host code only: nothing is built for the GPU).
 *
 *   lift_host_check FILE
 *     FILE: mode (0 centred, 1 scaled, 2 double)  nl  t  scale_bits  K,  nl primes,  K words (plaintext words, or bit patterns of doubles)
 *     prints K rows of nl words: lift_digit(lift_word(.))
 * The constants are formed here with 128-bit integers by the formulas of host/host_lift.inc: floor(2^64 / q), floor(2^128 / q),
 * floor(2^128 / t), r = Q mod t, [t]_q, [D]_q = -r t^-1 mod q and its Shoup word.  For the scaled mode the quotient w is formed a
 * second time with unsigned __int128 division, and the program fails (exit 1) where lift_scaled_w differs; the test compares the
 * output with the big-integer definitions. */
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ntt_lift.h"

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

static uint64_t powmod(uint64_t a, uint64_t e, uint64_t q)
{
  uint64_t r = 1 % q;
  for(a %= q; e; e >>= 1, a = (uint64_t)((u128)a * a % q))
    if(e & 1) r = (uint64_t)((u128)r * a % q);
  return r;
}

int main(int argc, char **argv)
{
  if(argc != 2) return 2;
  FILE *f = fopen(argv[1], "r");
  if(!f) return 2;
  const uint32_t mode = (uint32_t)rd(f);
  const int      nl   = (int)rd(f);
  const uint64_t t = rd(f), sb = rd(f), K = rd(f);
  if(mode > 2 || nl < 1 || nl > 64 || (mode != kLiftDouble && t < 2)) return 2;
  std::vector<uint64_t> q((size_t)nl);
  for(auto &v : q) v = rd(f);
  LiftCall   c{};
  const u128 all = ~(u128)0;
  c.mode         = mode;
  memcpy(&c.scale, &sb, 8);
  {
    const uint64_t td = mode == kLiftDouble ? 2 : t;
    const u128     mu = all / td + (all % td == td - 1 ? 1u : 0u);
    c.td.q            = td;
    c.td.mu_lo        = (uint64_t)mu;
    c.td.mu_hi        = (uint64_t)(mu >> 64);
  }
  if(mode != kLiftDouble) {
    c.half_dn = t / 2;
    c.half_up = t - t / 2;
    c.r       = 1 % t;
    for(int l = 0; l < nl; l++) c.r = (uint64_t)((u128)c.r * (q[(size_t)l] % t) % t);
  }
  std::vector<LiftLimb> ll((size_t)nl);
  for(int l = 0; l < nl; l++) {
    LiftLimb &     d  = ll[(size_t)l];
    const uint64_t ql = q[(size_t)l];
    const u128     mu = all / ql;
    d                 = LiftLimb{};
    d.q               = ql;
    d.bar             = ~0ull / ql;
    d.mu_lo           = (uint64_t)mu;
    d.mu_hi           = (uint64_t)(mu >> 64);
    if(mode == kLiftCentred) d.s = t % ql;
    if(mode == kLiftScaled) {
      const uint64_t x = (uint64_t)((u128)(c.r % ql) * powmod(t % ql, ql - 2, ql) % ql);
      d.s              = x ? ql - x : 0;
    }
    d.s_shoup = (uint64_t)(((u128)d.s << 64) / ql);
  }
  for(uint64_t k = 0; k < K; k++) {
    const uint64_t raw = rd(f);
    const LiftWord w   = lift_word(raw, c);
    if(mode == kLiftScaled) {
      const uint64_t want = (uint64_t)(((u128)c.r * raw + t / 2) / t);
      if(w.b != want) {
        fprintf(stderr, "word %" PRIu64 ": lift_scaled_w %" PRIu64 " reference %" PRIu64 "\n", k, w.b, want);
        return 1;
      }
    }
    for(int l = 0; l < nl; l++) printf("%" PRIu64 "%c", lift_digit(w, mode, ll[(size_t)l]), l + 1 < nl ? ' ' : '\n');
  }
  fclose(f);
  return 0;
}
