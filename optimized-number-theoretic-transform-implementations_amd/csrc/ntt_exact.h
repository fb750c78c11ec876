/*
 * ntt_exact.h -- the EXACT RNS base conversion of BFV multiplication (ntt_rns_mod_up_exact_batch, ntt_rns_mod_down_exact_batch): the
 * arithmetic it adds to the fast conversion of ntt_keyswitch.h, the argument records and the launchers of its kernels (exact_coef.hip; ntt_kernels_exact.h, instantiated in ksexact_f64*.hip).
 *
 * The integer sum of the fast conversion is x + u B, 0 <= u < n.  Halevi, Polyakov and Shoup's floating-point correction finds u from
 * the same digits z_i = [x_i * b^_i^-1]_{b_i}:  sum_i z_i / b_i = (x + u B) / B = u + x / B, so
 *   v = rint(s),  s = ((fl(z_0) rho_0 + fl(z_1) rho_1) + ...)   left to right,   rho_i = 1.0 / (double)b_i  (formed on the host)
 * is u for x < B / 2 and u + 1 for x > B / 2, and
 *   ExactBConv_{B->q}(x) = ( sum_i z_i [b^_i]_q  -  v [B]_q ) mod q
 * is the CENTRED representative of x (x, or x - B from B / 2 on), reduced mod q.  The sequence of FP64 operations is part of the
 * contract -- device, host and the tests' model agree bit for bit: fl is the round-to-nearest conversion of the 64-bit word, every
 * product and every sum one IEEE round-to-nearest operation (no fused multiply-add: the library is built with -ffp-contract=off), rint
 * rounds ties to even (v_rndne_f64).
 *
 * Error: z_i < b_i < 2^61, so every term is below 1 + 2^-52 and every partial sum below 16 + 2^-48 for n <= 16.  fl(z_i), rho_i and
 * their product carry a relative error of at most 2^-53 each: below 2^-51 per term in all (first order: 3 x 2^-53, terms about 1).
 * Every sum of a partial sum below 16 + 2^-48 is rounded to a multiple of at most 2^-48 (an error of at most 2^-49).  n terms and
 * n - 1 sums, n <= 16:  16 x 2^-51 + 15 x 2^-49 < 2^-47 + 2^-45.1 < 2^-44.  Hence for x in [0, B) with |2x - B| > 2^-43 B (x / B at
 * least 2^-44 away from 1/2) v is the rounding of the exact sum and the result is the centred representative of x; inside that band
 * it is x or x - B.  v is a function of the source words alone: every destination limb of a call, whichever launch serves it, forms
 * the same v from the same operations and so takes the same choice.
 *
 * 0 <= v <= n <= 16 (u + x / B < n, rounded): v (q - [B]_q) < 2^65 enters the 128-bit sum as one more bconv_mac before the one Barrett
 * reduction (below 2^126 + 2^65: nothing overflows).  BconvDst::h, which the exact forms have no other use for (there is no
 * half-offset: the centred remainder does the rounding), carries q - [B]_q.
 *
 * Exact scaled ModDown, multiplier m:  the source constants carry [m b^_j^-1]_{p_j}, so the digits are those of [m t]_P at no cost;
 *   c_l <- c_l [m P^-1]_{q_l} - ExactBConv_{P->q_l}([m t]_P) [P^-1]_{q_l}   (mod q_l)
 * which is round(m x / P) mod q_l for the x in [0, QP) behind the operand (P is odd: no ties), floor or ceiling inside the band.
 */
#pragma once
#include "ntt_keyswitch.h"

namespace ntt {

/* one term of s: fl(z) * rho, two roundings */
NTT_HD double exact_term(uint64_t z, double rho) { return (double)z * rho; }

/* v = rint(s), ties to even; 0 <= s < 16 + 2^-44 */
NTT_HD uint64_t exact_round(double s) { return (uint64_t)__builtin_rint(s); }

/* ( (hi, lo) - v [B]_q ) mod q, canonical: (hi, lo) the 128-bit sum of z_i [b^_i]_q, d.h = q - [B]_q */
NTT_HD uint64_t exact_bconv_finish(uint64_t hi, uint64_t lo, uint64_t v, const BconvDst &d)
{
  bconv_mac(hi, lo, v, d.h);
  const uint64_t r = bconv_reduce(hi, lo, d);
  return r >= d.q ? r - d.q : r;
}

/* ExactBConv of n words x[i], canonical mod src[i].p, to d: the whole conversion of one coefficient in the kernels' operation order
 * (the host-side statement of it: the tests' harness calls this) */
NTT_HD uint64_t exact_bconv(const uint64_t *x, const BconvSrc *src, const double *rho, const uint64_t *g, int n, const BconvDst &d)
{
  uint64_t hi = 0, lo = 0;
  double   s  = 0.0;
  for(int i = 0; i < n; i++) {
    const uint64_t z = bconv_digit(x[i], src[i]);
    const double   t = exact_term(z, rho[i]);
    s                = i ? s + t : t;
    bconv_mac(hi, lo, z, g[i]);
  }
  return exact_bconv_finish(hi, lo, exact_round(s), d);
}

/* the second constant of the exact ModDown's epilogue: [m P^-1]_q with its Shoup word (BconvDst::s is [P^-1]_q) */
struct ExactScale {
  uint64_t ms;
  uint64_t ms_shoup; /* floor(ms * 2^64 / q) */
};

/* c [m P^-1]_q - u [P^-1]_q mod q, canonical, for c, u < 2^64 (Shoup: each product in [0, 2q)) */
NTT_HD uint64_t moddown_exact_word(uint64_t c, uint64_t u, const BconvDst &d, const ExactScale &e)
{
  uint64_t a = c * e.ms - mulhi64(c, e.ms_shoup) * d.q;
  uint64_t b = u * d.s - mulhi64(u, d.s_shoup) * d.q;
  a          = a >= d.q ? a - d.q : a;
  b          = b >= d.q ? b - d.q : b;
  return a >= b ? a - b : a + (d.q - b);
}

/* Exact ModUp, coefficients: BconvArgs with rho[i] = 1.0 / (double)b_i and dl[k].h = q_k - [B]_{q_k} (exact_up_coef_kernel) */
struct BconvExactArgs {
  BconvArgs ba;
  double    rho[kBconvLimbs];
};
hipError_t launch_bconv_exact(const BconvExactArgs &xa);

/* Exact scaled ModDown, coefficients: ModDownCoefArgs with pl[j].inv = [m p^_j^-1]_{p_j}, pl[j].h = 0, ql[l].h = q_l - [P]_{q_l},
 * rho[j] = 1.0 / (double)p_j and es[l] = [m P^-1]_{q_l} (exact_down_coef_kernel) */
struct ModDownExactArgs {
  ModDownCoefArgs ma;
  double          rho[kBconvLimbs];
  ExactScale      es[kBconvLimbs];
};
hipError_t launch_moddown_exact_coef(const ModDownExactArgs &xa);

/* Exact scaled ModDown, NTT domain, FP64 policies, N = 2^6..2^14: ONE launch over a run of Q limbs (moddown_exact_fwd_kernel;
 * ksexact_f64*.hip).  ModDownFwdArgs with the exact constants (pl[j].inv = [m p^_j^-1]_{p_j}, pl[j].h = 0, ql[l].h = q_l - [P]_{q_l}),
 * rho[j] = 1.0 / (double)p_j and mq[l] = [m]_{q_l}. */
struct ModDownExactFwdArgs {
  ModDownFwdArgs ma;
  double         rho[kBconvLimbs];
  uint64_t       mq[kBconvLimbs];
};
template <class A, int KSH> hipError_t launch_moddown_exact_fwd(const ModDownExactFwdArgs &xa);
template <> hipError_t launch_moddown_exact_fwd<ArithF64, 0>(const ModDownExactFwdArgs &);
template <> hipError_t launch_moddown_exact_fwd<ArithF64, 1>(const ModDownExactFwdArgs &);
template <> hipError_t launch_moddown_exact_fwd<ArithF64, 18>(const ModDownExactFwdArgs &);
template <> hipError_t launch_moddown_exact_fwd<ArithF64W, 0>(const ModDownExactFwdArgs &);

} // namespace ntt
