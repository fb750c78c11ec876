/* sample_host_check.cpp -- the host side of the device-side sampler (csrc/ntt_sample.h: philox4x32_10, sample_block, sample_small,
 * sample_small_digit, sample_uniform_digit) on vectors written by tests/test_sample_cpu.py.  Host only, with the sanitizers: hipcc
 * --cuda-host-only -Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined -I csrc (nothing is built for the GPU).
 *
 *   sample_host_check FILE
 *     FILE: kind (0 ternary, 1 cbd21, 2 uniform)  nl  mult  seed  K,  nl primes,  K pairs (P, s)
 *     prints K rows: the block's four words (tag of limb 0), the centred value (0 for the uniform kind), then nl words sample_digit(.)
 * The limb constants are formed here with 128-bit integers by the formulas of host/host_sample.inc: floor(2^64 / q), floor(2^128 / q),
 * [mult]_q and its Shoup word.  The uniform word is formed a second time with unsigned __int128 division, and the program fails (exit
 * 1) where sample_uniform_digit differs; the test compares the output with the Python model. */
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ntt_sample.h"

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
  const uint32_t kind = (uint32_t)rd(f);
  const int      nl   = (int)rd(f);
  const uint64_t mult = rd(f), seed = rd(f), K = rd(f);
  if(kind > 2 || nl < 1 || nl > 64 || mult < 1) return 2;
  std::vector<SampleLimb> ll((size_t)nl);
  const u128              all = ~(u128)0;
  for(int l = 0; l < nl; l++) {
    SampleLimb &   d  = ll[(size_t)l];
    const uint64_t ql = rd(f);
    const u128     mu = all / ql;
    d                 = SampleLimb{};
    d.q               = ql;
    d.bar             = ~0ull / ql;
    d.mu_lo           = (uint64_t)mu;
    d.mu_hi           = (uint64_t)(mu >> 64);
    d.s               = mult % ql;
    d.s_shoup         = (uint64_t)(((u128)d.s << 64) / ql);
  }
  SampleCall c{};
  c.kind = kind;
  c.key0 = (uint32_t)seed;
  c.key1 = (uint32_t)(seed >> 32);
  for(uint64_t k = 0; k < K; k++) {
    const uint64_t    P = rd(f);
    const uint32_t    s = (uint32_t)rd(f);
    const SampleBlock b = sample_block(c, P, s, sample_tag(kind, 0));
    printf("%" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 " %d", b.w[0], b.w[1], b.w[2], b.w[3], kind == kSampleUniform ? 0 : sample_small(kind, b));
    for(int l = 0; l < nl; l++) {
      const uint64_t got = sample_digit(c, P, s, (uint32_t)l, ll[(size_t)l]);
      if(kind == kSampleUniform) {
        const SampleBlock bl   = sample_block(c, P, s, sample_tag(kind, (uint32_t)l));
        const u128        x    = (u128)bl.w[0] | ((u128)bl.w[1] << 32) | ((u128)bl.w[2] << 64) | ((u128)bl.w[3] << 96);
        const uint64_t    want = (uint64_t)(x % ll[(size_t)l].q);
        if(got != want) {
          fprintf(stderr, "row %" PRIu64 " limb %d: sample_uniform_digit %" PRIu64 " reference %" PRIu64 "\n", k, l, got, want);
          return 1;
        }
      }
      printf(" %" PRIu64, got);
    }
    printf("\n");
  }
  fclose(f);
  return 0;
}
