/*
 * ntt_plain.h -- out of the RNS: the last step of a decryption (ntt_rns_to_plain_batch, ntt_rns_to_double_batch): the argument records
 * and the launchers of the kernels (plain.hip), the host layer's view of them, and one output word stated for host and device
 * (plain_word, plain_double).
 *
 * x in [0, Q) is the integer behind the L canonical words x_i of one coefficient, Q = prod q_i, q^_i = Q / q_i, q_i < 2^61, L <= 16;
 * t is the plaintext modulus, 2 <= t < 2^61, ANY integer.  Both modes of to_plain are ONE statement with other constants:
 *   z_i = [x_i c_i]_{q_i}  (Shoup),   s = ((fl(z_0) rho_0 + fl(z_1) rho_1) + ...) left to right,  rho_i = 1.0 / (double)q_i,
 *   v   = rint(s),   m = ( sum_i z_i g_i + v h ) mod t,   canonical.
 *
 *   default (BGV)    m = [x_c]_t, x_c the centred representative of x mod Q.  ExactBConv_{Q->t} of ntt_exact.h with t for the
 *                    destination prime: c_i = [q^_i^-1]_{q_i}, g_i = [q^_i]_t, h = [-Q]_t.  sum z_i q^_i = x + u Q and v = u, or u + 1
 *                    from Q / 2 on.  Nothing has to be coprime to anything.  Exact for |2x - Q| > 2^-43 Q (ntt_exact.h's bound);
 *                    inside that band [x]_t or [x - Q]_t.
 *   NTT_PLAIN_SCALE (BFV)   m = round(t x / Q) mod t, gcd(t, q_i) = 1.  c_i = [t q^_i^-1]_{q_i}, g_i = [-q_i^-1]_t, h = 1: with
 *                    z_i' = [x_i q^_i^-1]_{q_i} write t z_i' = a_i q_i + r_i, r_i = z_i = [t z_i']_{q_i}.  sum_i t z_i' / q_i = t x / Q + t u,
 *                    so sum_i a_i + sum_i r_i / q_i = t x / Q (mod t), frac(sum r_i / q_i) = frac(t x / Q) and a_i = -r_i q_i^-1 (mod t):
 *                    round(t x / Q) = sum_i a_i + rint(sum_i r_i / q_i) = v + sum_i r_i g_i (mod t).  Q is odd: no ties.  The terms
 *                    r_i / q_i lie below 1 as ntt_exact.h's do, so its 2^-44 bound on the FP64 sum holds unchanged: with
 *                    rho = t x mod Q the result is exact for |2 rho - Q| > 2^-43 Q, and one of the two neighbours inside that band.
 * The sequence of FP64 operations is part of the contract (exact_term, exact_round: no fused multiply-add) -- device, host and the
 * tests' model agree bit for bit.  0 <= v <= 16; the 128-bit sum stays below 16 (2^61)^2 + 16 2^61 = 2^126 + 2^65 and is reduced
 * once by bconv_reduce (plain_dst, host_plain.inc, says why any t >= 2 is served by it), then one conditional subtraction.
 *
 * to_double (CKKS), L in {1, 2}:  y = fl(x_c) * scale, fl the round-to-nearest-even conversion of the exact signed integer, then one
 * IEEE product.  Two limbs: z_0 = [x_0 q_1^-1]_{q_0}, z_1 = [x_1 q_0^-1]_{q_1}, x = z_0 q_1 + z_1 q_0 - u Q with u in {0, 1}: below
 * 2 Q < 2^123, exact in 128 bits -- no floating-point estimate, no band.  The 128-bit magnitude |x_c| is normalised to 64 bits with
 * a sticky bit and converted once (double(hi) 2^64 + double(lo) would round twice); x_c = 0 gives +0.0 * scale.
 */
#pragma once
#include "ntt_exact.h"

namespace ntt {

constexpr int kPlainLimbs = 16;

/* limb i of a to_plain call: q_i, c_i with its Shoup word, g_i and rho_i side by side (one run of kernel-argument words per limb) */
struct PlainLimb {
  uint64_t p;
  uint64_t inv;       /* c_i                                */
  uint64_t inv_shoup; /* floor(c_i * 2^64 / q_i)            */
  uint64_t g;         /* g_i, in [0, t)                     */
  double   rho;       /* 1.0 / (double)q_i                  */
};

/* the constants of one to_plain call: the limbs, and d = {t, floor(2^128 / t), .h = h} */
struct PlainConsts {
  PlainLimb l[kPlainLimbs];
  BconvDst  d;
};

/* one limb's share of a coefficient: its digit z = [x c]_q (bconv_digit without an offset: Shoup, x c - floor(x c' / 2^64) q in [0, 2q)
 * for any x < 2^64) into the FP64 sum (term 0 is the first: no 0.0 + ...) and into the 128-bit sum */
NTT_HD void plain_step(uint64_t x, int i, const PlainConsts &k, double &s, uint64_t &hi, uint64_t &lo)
{
  const PlainLimb &l = k.l[i];
  uint64_t         z = x * l.inv - mulhi64(x, l.inv_shoup) * l.p;
  z                  = z >= l.p ? z - l.p : z;
  const double f     = exact_term(z, l.rho);
  s                  = i ? s + f : f;
  bconv_mac(hi, lo, z, l.g);
}

/* the output word from the two sums: exact_bconv_finish with t for the prime */
NTT_HD uint64_t plain_finish(double s, uint64_t hi, uint64_t lo, const PlainConsts &k) { return exact_bconv_finish(hi, lo, exact_round(s), k.d); }

/* one output word of to_plain from the n words of its coefficient, in the kernel's operation order (the host-side statement of it) */
NTT_HD uint64_t plain_word(const uint64_t *x, int n, const PlainConsts &k)
{
  uint64_t hi = 0, lo = 0;
  double   s  = 0.0;
  for(int i = 0; i < n; i++) plain_step(x[i], i, k, s, hi, lo);
  return plain_finish(s, hi, lo, k);
}

/* the constants of one to_double call: n = 1 -- q[0] only; n = 2 -- sl[0] = {q_0, 0, [q_1^-1]_{q_0}, Shoup}, sl[1] likewise with the
 * primes swapped, Q = q_0 q_1 as two words */
struct DoubleConsts {
  BconvSrc sl[2];
  uint64_t q_hi, q_lo; /* Q */
  double   scale;
};

/* fl(hi 2^64 + lo), round to nearest even, ONE rounding: the leading bit is moved to bit 63 of one word, every bit shifted out is
 * kept as a sticky bit 0 (the conversion drops 11 bits of that word: bit 0 can only break a tie, as the lost bits would), the one
 * hardware conversion rounds, and the power of two it is scaled by is exact.  hi < 2^58 (Q < 2^122). */
NTT_HD double plain_u128_to_double(uint64_t hi, uint64_t lo)
{
  if(hi == 0) return (double)lo;
  const int      lz = __builtin_clzll(hi); /* 6 .. 63 */
  const uint64_t w  = (hi << lz) | (lo >> (64 - lz)) | ((lo << lz) ? 1u : 0u);
  return __builtin_ldexp((double)w, 64 - lz);
}

/* one output of to_double from the n words of its coefficient (n = 1 or 2), in the kernel's operation order */
NTT_HD double plain_double(uint64_t x0, uint64_t x1, int n, const DoubleConsts &k)
{
  uint64_t hi = 0, lo = x0;
  if(n == 2) {
    const uint64_t z0 = bconv_digit(x0, k.sl[0]), z1 = bconv_digit(x1, k.sl[1]);
    lo                = 0;
    bconv_mac(hi, lo, z0, k.sl[1].p);
    bconv_mac(hi, lo, z1, k.sl[0].p);
    if(hi > k.q_hi || (hi == k.q_hi && lo >= k.q_lo)) { /* below 2Q: one subtraction */
      hi = hi - k.q_hi - (lo < k.q_lo ? 1u : 0u);
      lo = lo - k.q_lo;
    }
  }
  /* centred: x > (Q - 1) / 2, that is 2x > Q (Q odd, 2x < 2^123), is x - Q: the magnitude Q - x, negative */
  const uint64_t dh  = (hi << 1) | (lo >> 63), dl = lo << 1;
  const bool     neg = dh > k.q_hi || (dh == k.q_hi && dl > k.q_lo);
  if(neg) {
    hi = k.q_hi - hi - (k.q_lo < lo ? 1u : 0u);
    lo = k.q_lo - lo;
  }
  const double f = plain_u128_to_double(hi, lo);
  return (neg ? -f : f) * k.scale;
}

/* m <- the plaintext word of every coefficient: `a` is limb 0 of the source, its limbs a_limb_stride words apart (plain_kernel;
 * plain.hip) */
struct PlainArgs {
  uint64_t *      m;
  const uint64_t *a;
  uint64_t        a_limb_stride, a_poly_stride, m_poly_stride, batch;
  uint32_t        logn;
  int             nlimbs;
  PlainConsts     k;
  int             max_grid;
  hipStream_t     stream;
};
hipError_t launch_plain(const PlainArgs &pa);

/* y <- fl(x_c) * scale for one or two limbs (plain_double_kernel; plain.hip) */
struct PlainDoubleArgs {
  double *        y;
  const uint64_t *a;
  uint64_t        a_limb_stride, a_poly_stride, y_poly_stride, batch;
  uint32_t        logn;
  int             nlimbs;
  DoubleConsts    k;
  int             max_grid;
  hipStream_t     stream;
};
hipError_t launch_plain_double(const PlainDoubleArgs &pa);

} // namespace ntt
