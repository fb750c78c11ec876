/*
 * ntt_keyswitch.h -- launchers of the RNS base-conversion kernels of hybrid key switching (ntt_rns_mod_up_batch,
 * ntt_rns_mod_down_batch): the host layer's view of them, and the integer arithmetic they share.
 *
 * The kernel templates live in ntt_kernels_keyswitch.h (moddown_fwd_kernel, instantiated in keyswitch_f64*.hip; its body,
 * moddown_fwd_body of ntt_kernels_moddown.h, is also that of the ksfold, BGV and exact ModDown kernels), in
 * ntt_kernels_modup_mul.h (modup_mul_kernel, modup_mul2_kernel; modup_mul_f64*.hip, modup_mul2_f64*.hip) and in keyswitch_coef.hip
 * (bconv_kernel, moddown_coef_kernel); this header declares the argument records and the launchers, nothing
 * that the host translation unit would instantiate.
 *
 * Fast base conversion from a basis B = {b_i} (product B, b^_i = B / b_i) to a prime q:
 *   FastBConv_{B->q}(x) = ( sum_i [x_i * b^_i^-1]_{b_i} * b^_i ) mod q,
 * an integer sum: z_i = [x_i * b^_i^-1]_{b_i} by Shoup's method (bconv_digit), then sum_i z_i * [b^_i]_q accumulated in 128 bits
 * (bconv_mac) and reduced once (bconv_reduce).
 *   ModUp     the digit's limbs are the basis; every other limb l of the operand gets FastBConv_{B->q_l} of the digit.
 *   ModDown   the P limbs are the basis; Q limb l becomes (c_l - u_l) * P^-1 mod q_l with
 *             u_l = FastBConv_{P->q_l}([t + h]_P) - [h]_{q_l},  h = (P - 1) / 2 (0: floor).  [h]_{p_j} = (p_j - 1) / 2, since
 *             2h = P - 1 = -1 mod p_j.  With one P prime this is the rescale's u_l (rescale_digit) word for word.
 */
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ntt_arith.h"

namespace ntt {

constexpr int kBconvLimbs = 16; /* source limbs (a ModUp digit, the P primes) and destination limbs of one launch (= kMaxLimbs) */

/* a source prime b_i: the Shoup constants of b^_i^-1 mod b_i and the offset added first (ModDown: [h]_{p_i}; ModUp: 0) */
struct BconvSrc {
  uint64_t p;
  uint64_t h;         /* in [0, p)                          */
  uint64_t inv;       /* [b^_i^-1]_{b_i} (1 for one prime)  */
  uint64_t inv_shoup; /* floor(inv * 2^64 / p)              */
};

/* a destination prime q: Barrett constants for 64- and 128-bit words, and (ModDown) the scale and the offset */
struct BconvDst {
  uint64_t q;
  uint64_t bar;          /* floor(2^64 / q)                  */
  uint64_t mu_lo, mu_hi; /* floor(2^128 / q) as two words    */
  uint64_t s;            /* ModDown: [P^-1]_q                 */
  uint64_t s_shoup;      /* floor(s * 2^64 / q)              */
  uint64_t h;            /* ModDown: [h]_q (0: floor)         */
};

/* x mod q in [0, 2q) for ANY 128-bit x = hi 2^64 + lo and odd q < 2^63: Barrett with mu = floor(2^128 / q).  The estimate
 * e = floor(x mu / 2^128) satisfies x/q - 2 < x (2^128/q - 1) / 2^128 - 1 < e <= x/q, so e is floor(x/q) or one less and
 * x - e q lies in [0, 2q) -- below 2^64, so the difference is exact in wrapping 64-bit arithmetic.  Bits 128..191 of x mu are
 * formed exactly: bits 0..63 hold lo(lo mu_lo) alone (no carry out), the two carries out of bits 64..127 are counted. */
NTT_HD uint64_t bconv_reduce(uint64_t hi, uint64_t lo, const BconvDst &d)
{
  const uint64_t c0  = mulhi64(lo, d.mu_lo);
  const uint64_t m1l = lo * d.mu_hi, m1h = mulhi64(lo, d.mu_hi);
  const uint64_t m2l = hi * d.mu_lo, m2h = mulhi64(hi, d.mu_lo);
  const uint64_t s1  = m1l + c0;
  const uint64_t s2  = s1 + m2l;
  const uint64_t cy  = (s1 < m1l ? 1u : 0u) + (s2 < s1 ? 1u : 0u);
  const uint64_t e   = hi * d.mu_hi + m1h + m2h + cy; /* floor(x mu / 2^128) mod 2^64 */
  return lo - e * d.q;
}

/* a mod q in [0, q) for any a < 2^64: Barrett with floor(2^64 / q) (the same bound: a - floor(a bar / 2^64) q in [0, 2q)) */
NTT_HD uint64_t bconv_reduce64(uint64_t a, const BconvDst &d)
{
  const uint64_t v = a - mulhi64(a, d.bar) * d.q;
  return v >= d.q ? v - d.q : v;
}

/* z_i = [(x_i + h_i) * b^_i^-1]_{b_i} in [0, b_i) for canonical x_i < b_i < 2^61 (x + h < 2b: one subtraction; Shoup:
 * w inv - floor(w inv_shoup / 2^64) b lies in [0, 2b) for any w < 2^64) */
NTT_HD uint64_t bconv_digit(uint64_t x, const BconvSrc &s)
{
  uint64_t w = x + s.h;
  w          = w >= s.p ? w - s.p : w;
  uint64_t z = w * s.inv - mulhi64(w, s.inv_shoup) * s.p;
  return z >= s.p ? z - s.p : z;
}

/* the 128-bit sum of z * g over the basis, z < 2^61 and g < q < 2^61: every product is below 2^122, a sum of up to 16 of them
 * below 2^126 -- nothing overflows and bconv_reduce receives the exact integer */
NTT_HD void bconv_mac(uint64_t &hi, uint64_t &lo, uint64_t z, uint64_t g)
{
  const uint64_t pl = z * g;
  lo += pl;
  hi += mulhi64(z, g) + (lo < pl ? 1u : 0u);
}

/* ModDown's subtrahend from the accumulated sum: FastBConv - [h]_q (mod q), canonical */
NTT_HD uint64_t moddown_digit(uint64_t hi, uint64_t lo, const BconvDst &d)
{
  uint64_t v = bconv_reduce(hi, lo, d);
  v          = v >= d.q ? v - d.q : v;
  return v >= d.h ? v - d.h : v + (d.q - d.h);
}

/* the same for ONE P prime p (b^ = 1, z = [t + h]_p < 2^61): Barrett of the word itself -- rescale_digit's arithmetic */
NTT_HD uint64_t moddown_digit1(uint64_t t, const BconvSrc &s, const BconvDst &d)
{
  uint64_t w       = t + s.h;
  w                = w >= s.p ? w - s.p : w;
  const uint64_t v = bconv_reduce64(w, d);
  return v >= d.h ? v - d.h : v + (d.q - d.h);
}

/* the grid of the element-wise kernels over n coefficient positions (bconv_kernel, moddown_coef_kernel, the galois kernels): that of
 * rescale_coef_kernel (host_products.inc grid_pw), about four iterations per workgroup */
inline unsigned coef_grid(uint64_t n, int max_grid)
{
  const uint64_t total = (n + 255) / 256;
  uint64_t       g     = (total + 3) / 4;
  if(g < 2048) g = total < 2048 ? total : 2048;
  if(g > (1u << 22)) g = 1u << 22;
  if(max_grid > 0) g = total < (uint64_t)max_grid ? total : (uint64_t)max_grid;
  return (unsigned)(g ? g : 1);
}

/* ModUp, coefficients: destination limb k of the launch (k0 + k of the operand's other limbs: slot k0 + k, or k0 + k + count
 * from the digit on) <- FastBConv of the count source limbs (bconv_kernel; keyswitch_coef.hip).  g[i][k] = [b^_i]_{q_k}. */
struct BconvArgs {
  uint64_t *  a; /* the operand's limb 0 */
  uint64_t    limb_stride, poly_stride, batch;
  uint32_t    logn;
  int         first, count; /* the digit: slots [first, first + count) */
  int         k0, ndst;     /* destination limbs k0 .. k0 + ndst - 1    */
  BconvSrc    sl[kBconvLimbs];
  BconvDst    dl[kBconvLimbs];
  uint64_t    g[kBconvLimbs][kBconvLimbs];
  int         max_grid;
  hipStream_t stream;
};
hipError_t launch_bconv(const BconvArgs &ba);

/* ModDown, coefficients: c_l <- (c_l - u_l) * P^-1 for up to 16 Q limbs, the np P limbs read once (moddown_coef_kernel).
 * g[j][l] = [p^_j]_{q_l}. */
struct ModDownCoefArgs {
  uint64_t *      c; /* the launch's first Q limb */
  const uint64_t *t; /* the first P limb          */
  uint64_t        limb_stride, poly_stride, batch;
  uint32_t        logn;
  int             nlimbs, np;
  BconvSrc        pl[kBconvLimbs];
  BconvDst        ql[kBconvLimbs];
  uint64_t        g[kBconvLimbs][kBconvLimbs];
  int             max_grid;
  hipStream_t     stream;
};
hipError_t launch_moddown_coef(const ModDownCoefArgs &ma);

/* ModDown, NTT domain, FP64 policies, N = 2^6..2^14: c_l^ <- (c_l^ - fwd(u_l)) * P^-1 in ONE launch over a run of Q limbs
 * (moddown_fwd_kernel; keyswitch_f64*.hip).  The P limbs arrive inverse-transformed.  [p^_j]_{q_l} is formed by each
 * workgroup (one limb) in its prologue: a 16 x 16 table beside the run's limb records would not fit the kernel arguments. */
struct ModDownFwdArgs {
  uint64_t *      c;      /* the run's first Q limb (NTT domain, canonical) */
  const uint64_t *t;      /* the first P limb, coefficients                 */
  const void *    limbs;  /* HOST array of the run's LimbRec<A>             */
  int             nlimbs; /* 1 .. kBconvLimbs                               */
  int             np;     /* 1 .. kBconvLimbs                               */
  uint64_t        limb_stride, poly_stride, batch;
  uint32_t        logn;
  BconvSrc        pl[kBconvLimbs];
  BconvDst        ql[kBconvLimbs];
  int             max_grid, num_cus;
  hipStream_t     stream;
};
template <class A, int KSH> hipError_t launch_moddown_fwd(const ModDownFwdArgs &ma);
template <> hipError_t launch_moddown_fwd<ArithF64, 0>(const ModDownFwdArgs &);
template <> hipError_t launch_moddown_fwd<ArithF64, 1>(const ModDownFwdArgs &);
template <> hipError_t launch_moddown_fwd<ArithF64, 18>(const ModDownFwdArgs &);
template <> hipError_t launch_moddown_fwd<ArithF64W, 0>(const ModDownFwdArgs &);

/* ModUp fused into the key product, FP64 policies, N = 2^6..2^14: c_l^ (+)= fwd(FastBConv_{digit->q_l}) (.) key_l^ in ONE launch over a
 * run of limbs of the extended basis; a digit limb inside the run is transformed as it stands.  The extended digit is never written.
 * [b^_i]_{q_l} is formed by each workgroup, as in moddown_fwd_kernel.
 *   ncomp = 1   one component (modup_mul_kernel; modup_mul_f64*.hip);
 *   ncomp = 2   the pair form: c0_l^ (+)= fwd(.) (.) key0_l^ and c1_l^ (+)= fwd(.) (.) key1_l^ from ONE conversion and ONE set of forward
 *               stages (modup_mul2_kernel; modup_mul2_f64*.hip).  own = all ones (count = 1, dig = a): every limb is transformed as it
 *               stands, the pair form of the forward-multiply. */
struct ModUpMulArgs {
  uint64_t *      a;      /* the run's first limb of the extended operand (read only: the digit's own limbs)  */
  const uint64_t *dig;    /* the digit's first limb, coefficients                                             */
  const uint64_t *b[2];   /* key_j^, the run's first limb (j < ncomp)                                         */
  uint64_t *      out[2]; /* c_j^, the run's first limb                                                       */
  int             ncomp;  /* 1 or 2: the launcher's NC                                                        */
  const void *    limbs;  /* HOST array of the run's LimbRec<A>                                               */
  int             nlimbs; /* 1 .. kBconvLimbs                                                                 */
  int             count;  /* 1 .. kBconvLimbs                                                                 */
  uint32_t        own;    /* bit l: limb l of the run belongs to the digit                                    */
  uint64_t        limb_stride, poly_stride, b_limb_stride, batch;
  uint32_t        logn;
  bool            lazy_in, b_bcast, accumulate;
  BconvSrc        sl[kBconvLimbs];
  BconvDst        dl[kBconvLimbs];
  int             max_grid, num_cus;
  hipStream_t     stream;
};
template <class A, int KSH, int NC> hipError_t launch_modup_mul(const ModUpMulArgs &ma);
template <> hipError_t launch_modup_mul<ArithF64, 0, 1>(const ModUpMulArgs &);
template <> hipError_t launch_modup_mul<ArithF64, 1, 1>(const ModUpMulArgs &);
template <> hipError_t launch_modup_mul<ArithF64, 18, 1>(const ModUpMulArgs &);
template <> hipError_t launch_modup_mul<ArithF64W, 0, 1>(const ModUpMulArgs &);
template <> hipError_t launch_modup_mul<ArithF64, 0, 2>(const ModUpMulArgs &);
template <> hipError_t launch_modup_mul<ArithF64, 1, 2>(const ModUpMulArgs &);
template <> hipError_t launch_modup_mul<ArithF64, 18, 2>(const ModUpMulArgs &);
template <> hipError_t launch_modup_mul<ArithF64W, 0, 2>(const ModUpMulArgs &);

} // namespace ntt
