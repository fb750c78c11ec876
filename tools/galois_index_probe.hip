/* tools/galois_index_probe.hip -- the index functions of the Galois kernels (csrc/ntt_galois.h: galois_ntt_src, galois_coef_src,
 * galois_inverse) compiled for the CPU and printed, so that a test can compare them with its model word for word without a GPU
 * (tests/test_galois_cpu.py).  Host only, no device code is built or run:
 *   hipcc --cuda-host-only -O1 -std=c++17 -Iinclude -Iinclude/internal -I<csrc> -o build/galois_index_probe tools/galois_index_probe.hip
 *   build/galois_index_probe N g [N g ...]   per pair a line "# N g", then per slot s < N a line "<ntt source slot> <coefficient
 *                                            source position> <1 if the coefficient is negated>"
 *   build/galois_index_probe --reduce q k c  bconv_mac / bconv_reduce on k products (q - 1)(q - 1) plus c: the canonical result */
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "ntt_galois.h"

using namespace ntt;

int main(int argc, char **argv)
{
  if(argc == 5 && !strcmp(argv[1], "--reduce")) {
    const uint64_t q = strtoull(argv[2], nullptr, 0), c = strtoull(argv[4], nullptr, 0);
    const int      k = atoi(argv[3]);
    BconvDst       d{};
    d.q                        = q;
    d.bar                      = ~0ull / q;
    const unsigned __int128 mu = ~(unsigned __int128)0 / q;
    d.mu_lo                    = (uint64_t)mu;
    d.mu_hi                    = (uint64_t)(mu >> 64);
    uint64_t hi = 0, lo = c;
    for(int i = 0; i < k; i++) bconv_mac(hi, lo, q - 1, q - 1);
    const uint64_t v = bconv_reduce(hi, lo, d);
    printf("%" PRIu64 " %" PRIu64 " %" PRIu64 "\n", hi, lo, v >= q ? v - q : v);
    return 0;
  }
  if(argc < 3 || (argc - 1) % 2) {
    fprintf(stderr, "usage: %s N g [N g ...] | --reduce q k c\n", argv[0]);
    return 2;
  }
  for(int a = 1; a + 1 < argc; a += 2) {
    const uint64_t n = strtoull(argv[a], nullptr, 0), g = strtoull(argv[a + 1], nullptr, 0);
    uint32_t       m = 0;
    while((1ull << m) < n) m++;
    if(n < 2 || (1ull << m) != n || m > 30 || !(g & 1) || g >= 2 * n) return 2;
    const uint32_t ginv = galois_inverse((uint32_t)g) & (uint32_t)(2 * n - 1);
    printf("# %" PRIu64 " %" PRIu64 "\n", n, g);
    for(uint32_t s = 0; s < n; s++) {
      const uint32_t u = galois_coef_src(s, ginv, m);
      printf("%u %u %u\n", galois_ntt_src(s, (uint32_t)g, m), u & (uint32_t)(n - 1), u >= n ? 1u : 0u);
    }
  }
  return 0;
}
