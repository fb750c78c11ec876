/*
 * ntt_lift.h -- into the RNS: the first step of an encryption, and every plaintext operand (ntt_rns_from_plain_batch,
 * ntt_rns_from_double_batch): the argument records and the launchers of the kernels (lift.hip, lift_f64*.hip), the host layer's view of
 * them, and one output word stated for host and device (lift_centred, lift_scaled, lift_double).
 *
 * One plaintext word per coefficient becomes one canonical word per limb q_l < 2^61.  Integer arithmetic only; every definition fixes
 * every output word, so the coefficient kernel, the fused kernel, the host statement and the tests' big integers agree bit for bit.
 *
 *   centred (BGV; plaintext operands)   c_l = [m_c]_{q_l},  m_c = m for 2m < t, else m - t:  [m]_{q_l} - (m >= ceil(t/2) ? [t]_{q_l} : 0)
 *                    (mod q_l): one 64-bit Barrett reduction, one correction (rescale_digit's shape).  2 <= t < 2^61, any integer.
 *   scaled (BFV, NTT_LIFT_SCALE)        c_l = [floor((Q m + floor(t/2)) / t)]_{q_l},  Q = prod q_l,  gcd(t, q_l) = 1.  With r = Q mod t and
 *                    D = floor(Q / t):  Q m + floor(t/2) = t D m + (r m + floor(t/2)), so the value is D m + w with
 *                    w = floor((r m + floor(t/2)) / t) <= t -- ONE 128-by-64-bit quotient per word (lift_scaled_w: Barrett with
 *                    floor(2^128 / t), r m + t/2 < 2^122), the same for every limb.  [D]_{q_l} = -r t^-1 mod q_l (t D = Q - r and Q = 0
 *                    mod q_l): the host needs no multi-precision arithmetic.  Per limb [D]_{q_l} [m]_{q_l} (Shoup) + [w]_{q_l}.
 *   double (CKKS)    p = fl(y * scale), ONE IEEE product; v = rint(p), ties to even; c_l = [v]_{q_l}.  v = 0 for NaN, +-inf and
 *                    |p| >= 2^127 (defined behaviour).  |v| < 2^127 is an exact 128-bit magnitude -- the 53-bit significand shifted by
 *                    the exponent (lift_double_mag) --, reduced per limb by bconv_reduce and negated where p < 0.  No floating-point
 *                    arithmetic beyond the product and rint.
 * A word m >= t is the caller's error: the result is then unspecified, but every operation above is defined for any 64-bit m and ends
 * in a conditional subtraction, so the word lies in [0, q_l).
 */
#pragma once
#include "ntt_produce.h"

namespace ntt {

constexpr int kLiftLimbs = kProduceLimbs; /* limbs of one launch */

enum LiftMode : uint32_t { kLiftCentred = 0, kLiftScaled = 1, kLiftDouble = 2 };

/* limb l of a lift: BconvDst with q, bar, mu as bconv_dst forms them and the mode's multiplier in s (s_shoup its Shoup word):
 * centred [t]_q, scaled [D]_q; h is not used */
using LiftLimb = BconvDst;

/* what the limbs share: the mode, the plaintext modulus as a 128-bit Barrett divisor (td: t, floor(2^128 / t); plain_dst), r = Q mod t,
 * floor(t/2), ceil(t/2), and the scale of the double mode */
struct LiftCall {
  uint32_t mode, accumulate;
  BconvDst td;
  uint64_t r, half_dn, half_up;
  double   scale;
};

/* the word-level part, the same for every limb: {a, b, neg} = centred {m, 0, m >= ceil(t/2)}; scaled {m, w, -}; double {lo, hi, p < 0}
 * of the magnitude */
struct LiftWord {
  uint64_t a, b;
  bool     neg;
};

/* floor(x / t) for x = hi 2^64 + lo < 2^127, t >= 2: bconv_reduce's estimate e = floor(x mu / 2^128) is the quotient or one less, the
 * remainder lo - e t (exact in wrapping arithmetic, below 2t < 2^62) decides.  (mod 2^64 -- the true quotient fits a word wherever
 * m < t.) */
NTT_HD uint64_t lift_quot128(uint64_t hi, uint64_t lo, const BconvDst &d)
{
  const uint64_t c0  = mulhi64(lo, d.mu_lo);
  const uint64_t m1l = lo * d.mu_hi, m1h = mulhi64(lo, d.mu_hi);
  const uint64_t m2l = hi * d.mu_lo, m2h = mulhi64(hi, d.mu_lo);
  const uint64_t s1  = m1l + c0;
  const uint64_t s2  = s1 + m2l;
  const uint64_t cy  = (s1 < m1l ? 1u : 0u) + (s2 < s1 ? 1u : 0u);
  const uint64_t e   = hi * d.mu_hi + m1h + m2h + cy;
  return lo - e * d.q >= d.q ? e + 1 : e;
}

/* w = floor((r m + floor(t/2)) / t) */
NTT_HD uint64_t lift_scaled_w(uint64_t m, const LiftCall &c)
{
  uint64_t hi = 0, lo = c.half_dn;
  bconv_mac(hi, lo, m, c.r);
  return lift_quot128(hi, lo, c.td);
}

/* |v| of v = rint(fl(y scale)) as 128 bits, 0 where the product is not finite or reaches 2^127; neg = the product's sign */
NTT_HD LiftWord lift_double_mag(uint64_t ybits, const LiftCall &c)
{
  union {
    double   d;
    uint64_t u;
  } y, v;
  y.u            = ybits;
  const double p = y.d * c.scale;
  v.d            = __builtin_rint(p);
  const uint64_t mag = v.u & ~(1ull << 63);
  const int      ex  = (int)(mag >> 52); /* biased; an integer-valued double is 0 (ex = 0) or at least 1 (ex >= 1023) */
  LiftWord       w{0, 0, (v.u >> 63) != 0};
  if(ex < 1023 || ex >= 1023 + 127) return w; /* 0; NaN and inf (ex = 2047); |v| >= 2^127 */
  const uint64_t sig = (mag & ((1ull << 52) - 1)) | (1ull << 52);
  const int      sh  = ex - 1075; /* v = sig 2^sh, -52 <= sh <= 74 */
  if(sh <= 0) w.a = sig >> -sh;
  else if(sh < 64) {
    w.a = sig << sh;
    w.b = sig >> (64 - sh);
  } else w.b = sig << (sh - 64);
  return w;
}

NTT_HD LiftWord lift_word(uint64_t raw, const LiftCall &c)
{
  if(c.mode == kLiftDouble) return lift_double_mag(raw, c);
  if(c.mode == kLiftScaled) return LiftWord{raw, lift_scaled_w(raw, c), false};
  return LiftWord{raw, 0, raw >= c.half_up};
}

/* [m_c]_q from m and whether it is the upper half */
NTT_HD uint64_t lift_centred(uint64_t m, bool upper, const LiftLimb &l)
{
  const uint64_t v = bconv_reduce64(m, l);
  const uint64_t s = upper ? l.s : 0;
  return v >= s ? v - s : v + (l.q - s);
}

/* [D m + w]_q */
NTT_HD uint64_t lift_scaled(uint64_t m, uint64_t w, const LiftLimb &l)
{
  const uint64_t a = bconv_reduce64(m, l);
  uint64_t       z = a * l.s - mulhi64(a, l.s_shoup) * l.q; /* [0, 2q) */
  z                = z >= l.q ? z - l.q : z;
  z += bconv_reduce64(w, l);
  return z >= l.q ? z - l.q : z;
}

/* [+-(hi 2^64 + lo)]_q */
NTT_HD uint64_t lift_double(uint64_t hi, uint64_t lo, bool neg, const LiftLimb &l)
{
  uint64_t v = bconv_reduce(hi, lo, l);
  v          = v >= l.q ? v - l.q : v;
  return neg && v ? l.q - v : v;
}

/* one output word: the limb's part of a lifted word */
NTT_HD uint64_t lift_digit(const LiftWord &w, uint32_t mode, const LiftLimb &l)
{
  if(mode == kLiftDouble) return lift_double(w.b, w.a, w.neg, l);
  if(mode == kLiftScaled) return lift_scaled(w.a, w.b, l);
  return lift_centred(w.a, w.neg, l);
}

struct LiftArgs : ProduceArgs<LiftCall> {
  const uint64_t *m; /* the plaintext: words mod t, or the bit patterns of doubles ([batch][N]) */
  uint64_t        m_poly_stride;
};

/* coefficients: c_l (+)= the lift for up to kLiftLimbs limbs, the plaintext word read once (lift_coef_kernel; lift.hip) */
using LiftCoefArgs = LiftArgs;
hipError_t launch_lift_coef(const LiftCoefArgs &la);

/* NTT domain, FP64 policies, N = 2^6..2^14: c_l^ (+)= fwd(the lift) in ONE launch over a run of limbs (lift_fwd_kernel;
 * lift_f64*.hip) */
using LiftFwdArgs = LiftArgs;
template <class A, int KSH> hipError_t launch_lift_fwd(const LiftFwdArgs &la);
template <> hipError_t launch_lift_fwd<ArithF64, 0>(const LiftFwdArgs &);
template <> hipError_t launch_lift_fwd<ArithF64, 1>(const LiftFwdArgs &);
template <> hipError_t launch_lift_fwd<ArithF64, 18>(const LiftFwdArgs &);
template <> hipError_t launch_lift_fwd<ArithF64W, 0>(const LiftFwdArgs &);

} // namespace ntt
