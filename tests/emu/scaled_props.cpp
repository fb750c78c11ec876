/*
 * scaled_props.cpp -- scalar property check of ArithF64S (csrc/ntt_arith.h) against 128-bit integer arithmetic
 * (TEST INFRASTRUCTURE, built and run by tests/test_scaled_cpu.py with the flags of tests/emu/Makefile).
 *   scaled_props Q CASES SEED
 * Random and edge operands |Y| <= min(2^53 - 1, 2^16 q), |W| <= q/2, |X| < 2q: the full-record product, the compact product, the
 * two-instruction reduce, the canonical word, the lazy word and the butterfly's adds must equal the integer reference, and the
 * quotient estimates must obey rho = 1/2 + B theta2 / 2 (full record) and 1/2 + B theta2 (compact).  Prints the number of
 * violated claims per kind; exit status 1 if any.
 */
#include <cstdio>
#include <cstdlib>

#include "ntt_arith.h"

using namespace ntt;
typedef __int128 i128;

static uint64_t rng_state;
static uint64_t rnd()
{
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ULL);
  z          = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
  z          = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
  return z ^ (z >> 31);
}
static int64_t rnd_sym(int64_t bound) { return (int64_t)(rnd() % (uint64_t)(2 * bound + 1)) - bound; } /* [-bound, bound] */

static double  scaled(int64_t v) { return __builtin_ldexp((double)v, -1074); }   /* |v| < 2^53: exact */
static int64_t units(double v) { return (int64_t)__builtin_ldexp(v, 1074); }
static i128    mod(i128 v, i128 q) { return ((v % q) + q) % q; }

int main(int argc, char **argv)
{
  if(argc < 4) return 2;
  const uint64_t q     = strtoull(argv[1], 0, 0);
  const long     cases = atol(argv[2]);
  rng_state            = strtoull(argv[3], 0, 0);
  F64Consts c{};
  c.q      = (double)q;
  c.qinv   = 1.0 / c.q;
  c.qi     = q;
  c.q2_sub = ArithF64S::word_to_val(2 * q);
  const double  th2  = c.q / 9007199254740992.0;
  const int64_t ymax = q < (1ull << 37) ? (int64_t)(q << 16) : (int64_t)((1ull << 53) - 1); /* 2^16 q in the small-modulus class */
  const int64_t wmax = (int64_t)(q / 2), xmax = (int64_t)(2 * q - 1);
  const int64_t yedge[] = {0, 1, -1, ymax, -ymax, ymax - 1, (int64_t)q, -(int64_t)q, (int64_t)(q / 2), (int64_t)(q / 2) + 1, -(int64_t)(q / 2) - 1,
                           (int64_t)(2 * q), (int64_t)(1ull << 52), -(int64_t)(1ull << 52), (int64_t)(1ull << 52) - 1};
  const int64_t wedge[] = {0, 1, -1, wmax, -wmax, wmax - 1, 2, (int64_t)(1ull << 25)};
  const int     ny = sizeof(yedge) / sizeof(yedge[0]), nw = sizeof(wedge) / sizeof(wedge[0]);
  long bad_full = 0, bad_rho = 0, bad_c = 0, bad_rhoc = 0, bad_red = 0, bad_canon = 0, bad_lazy = 0, bad_add = 0;
  for(long i = 0; i < cases; i++) {
    int64_t Y = i < ny * nw ? yedge[i % ny] : rnd_sym(ymax);
    int64_t W = i < ny * nw ? wedge[i / ny] : rnd_sym(wmax);
    if(Y > ymax || Y < -ymax) Y = ymax;
    if(W > wmax || W < -wmax) W = wmax;
    const int64_t X  = rnd_sym(xmax);
    const double  y  = scaled(Y), x = scaled(X);
    const TwF64   t  = {(double)W, (double)W / c.q};
    const double  by = (Y < 0 ? -(double)Y : (double)Y) / c.q;
    /* full record */
    const double r = ArithF64S::mulmod(t, y, c);
    const i128   R = units(r);
    if(scaled((int64_t)R) != r || mod((i128)Y * W - R, q) != 0) bad_full++;
    if(__builtin_fabs((double)R) > (0.5 + 0.5 * by * th2) * c.q * (1 + 1e-12) + 1.0) bad_rho++;
    /* compact twiddle */
    const double rc = ArithF64S::mulmod_c(t.w, y, c);
    const i128   RC = units(rc);
    if(scaled((int64_t)RC) != rc || mod((i128)Y * W - RC, q) != 0) bad_c++;
    if(__builtin_fabs((double)RC) > (0.5 + by * th2) * c.q * (1 + 1e-12) + 1.0) bad_rhoc++;
    /* reduce */
    const double v = ArithF64S::reduce(y, c);
    const i128   V = units(v);
    if(scaled((int64_t)V) != v || mod((i128)Y - V, q) != 0 || __builtin_fabs((double)V) > 0.5 * c.q + 2.0) bad_red++;
    /* canonical and lazy words */
    if((i128)ArithF64S::to_canonical(y, c) != mod(Y, q)) bad_canon++;
    if((i128)ArithF64S::store_fwd_lazy(x, c) != (i128)X + 2 * (i128)q) bad_lazy++;
    /* the butterfly's adds: |X| < 2q, |m| <= q */
    if(by <= 2.0) {
      double xx = x, yy = y;
      ArithF64S::fwd_bfly<false>(xx, yy, t, c);
      if((i128)units(xx) != (i128)X + R || (i128)units(yy) != (i128)X - R) bad_add++;
    }
  }
  printf("cases %ld q %llu: full %ld rho %ld compact %ld rho_c %ld reduce %ld canonical %ld lazy %ld adds %ld\n", cases, (unsigned long long)q, bad_full,
         bad_rho, bad_c, bad_rhoc, bad_red, bad_canon, bad_lazy, bad_add);
  return (bad_full | bad_rho | bad_c | bad_rhoc | bad_red | bad_canon | bad_lazy | bad_add) ? 1 : 0;
}
