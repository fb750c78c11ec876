/*
 * ntt_bgv.h -- BGV modulus switching: the RNS ModDown that keeps the plaintext mod T (ntt_rns_mod_down_bgv_batch,
 * ntt_rns_mod_down_bgv_add_batch): the arithmetic it adds to ntt_keyswitch.h, the argument record and the launchers of its kernel
 * (ntt_kernels_bgv.h, instantiated in ksbgv_f64*.hip).
 *
 * Dividing by P = prod p_j must subtract a correction that is = x mod P and = 0 mod T.  With t_j the coefficients of P limb j,
 * p^_j = P / p_j and h = (P - 1) / 2 ([h]_{p_j} = (p_j - 1) / 2):
 *   z_j = [ ( t_j [T^-1]_{p_j} + [h]_{p_j} ) [p^_j^-1]_{p_j} ]_{p_j}          canonical
 *   F_l = ( sum_j z_j [p^_j]_{q_l} ) mod q_l                                  the exact integer sum, reduced once
 *   c_l <- ( c_l - [T]_{q_l} (F_l - [h]_{q_l}) ) [P^-1]_{q_l}  mod q_l        canonical
 * The sum is w + h + v P with w the centred residue of x T^-1 mod P and 0 <= v < np, so the Q limbs hold (x - T w) / P - v T: a multiple
 * of T away from y = (x - T w) / P, and y = x P^-1 (mod T).  The caller owns the factor P^-1 mod T.
 *
 * Every intermediate is a canonical residue, so every order of folding the constants gives the same words:
 *   source    z_j = [ (t_j + [h T]_{p_j}) [T^-1 p^_j^-1]_{p_j} ]_{p_j}: bconv_digit with BconvSrc::h = [h T]_{p_j} and
 *             BconvSrc::inv = [T^-1 p^_j^-1]_{p_j} (bgv_sources, host) -- ONE Shoup product per source word, as the approximate ModDown;
 *   sum       [T]_{q_l} (F_l - [h]_{q_l}) = ( sum_j z_j [T p^_j]_{q_l} ) - [T h]_{q_l}: moddown_digit with the table entries and
 *             BconvDst::h multiplied by [T]_{q_l} once per launch (coefficients: on the host) or once per workgroup (the block kernel:
 *             bconv_ghat cannot carry T, bgv_scale on its np entries can; the offset comes from the host) -- NO product per word;
 *   one prime there is no table (p^_0 = 1): [T]_{q_l} [z_0]_{q_l} - [T h]_{q_l} with one Shoup product per word (bgv_digit1).
 * Hence the coefficient route is moddown_coef_kernel itself with these constants (it has no one-prime shortcut: np = 1 takes its general
 * path with g[0][l] = [T]_{q_l}), and only the block kernel is new.  T may share a factor with a kept prime: [T]_{q_l} = 0 gives
 * c_l [P^-1]_{q_l}.
 */
#pragma once
#include "ntt_ct_mul.h"

namespace ntt {

/* [T]_q of a destination prime with its Shoup word */
struct BgvScale {
  uint64_t tq;
  uint64_t tq_shoup; /* floor(tq * 2^64 / q) */
};

/* v [T]_q mod q, canonical, for any v < 2^64 (Shoup: the product in [0, 2q)) */
NTT_HD uint64_t bgv_scale(uint64_t v, const BgvScale &s, uint64_t q)
{
  const uint64_t r = v * s.tq - mulhi64(v, s.tq_shoup) * q;
  return r >= q ? r - q : r;
}

/* the subtrahend for ONE P prime: [T]_q [z]_q - [T h]_q, z = bconv_digit(t, s) (s.inv = [T^-1]_p, not 1: the product is not skipped),
 * dt.h = [T h]_q as in the folded order below */
NTT_HD uint64_t bgv_digit1(uint64_t t, const BconvSrc &s, const BconvDst &dt, const BgvScale &ts)
{
  const uint64_t v = bgv_scale(bconv_reduce64(bconv_digit(t, s), dt), ts, dt.q);
  return v >= dt.h ? v - dt.h : v + (dt.q - dt.h);
}

/* the subtrahend by the definition's order, n >= 1 primes: [T]_q (F - [h]_q) with g[j] = [p^_j]_q and d.h = [h]_q (the host-side
 * statement: the tests' harness compares it with the folded order below and with 128-bit integers) */
NTT_HD uint64_t bgv_sub_plain(const uint64_t *t, const BconvSrc *src, const uint64_t *g, int n, const BconvDst &d, const BgvScale &ts)
{
  uint64_t hi = 0, lo = 0;
  for(int j = 0; j < n; j++) bconv_mac(hi, lo, bconv_digit(t[j], src[j]), g[j]);
  return bgv_scale(moddown_digit(hi, lo, d), ts, d.q);
}

/* the same words in the kernels' order: gt[j] = bgv_scale(g[j]) = [T p^_j]_q and dt.h = bgv_scale(d.h) = [T h]_q, no product per word */
NTT_HD uint64_t bgv_sub_folded(const uint64_t *t, const BconvSrc *src, const uint64_t *gt, int n, const BconvDst &dt)
{
  uint64_t hi = 0, lo = 0;
  for(int j = 0; j < n; j++) bconv_mac(hi, lo, bconv_digit(t[j], src[j]), gt[j]);
  return moddown_digit(hi, lo, dt);
}

/* (c - u) [P^-1]_q mod q, canonical, for canonical c and u (moddown_coef_kernel's last step) */
NTT_HD uint64_t bgv_word(uint64_t c, uint64_t u, const BconvDst &d)
{
  const uint64_t x = c >= u ? c - u : c + (d.q - u);
  const uint64_t v = x * d.s - mulhi64(x, d.s_shoup) * d.q;
  return v >= d.q ? v - d.q : v;
}

/* BGV ModDown, NTT domain, FP64 policies, N = 2^6..2^14: out_l^ (+)= (c_l^ - fwd(u_l)) P^-1 in ONE launch over a run of Q limbs
 * (moddown_bgv_fwd_kernel; ksbgv_f64*.hip).  k is ksfold_fwd_kernel's record with k.m.pl from bgv_sources and k.m.ql[l].h = [T h]_{q_l};
 * the in-place form passes out = k.m.c with the accumulator's strides and accumulate = false.  ts[l] = [T]_{q_l}. */
struct ModDownBgvArgs {
  KsFoldArgs k;
  BgvScale   ts[kBconvLimbs];
};
template <class A, int KSH> hipError_t launch_moddown_bgv_fwd(const ModDownBgvArgs &ba);
template <> hipError_t launch_moddown_bgv_fwd<ArithF64, 0>(const ModDownBgvArgs &);
template <> hipError_t launch_moddown_bgv_fwd<ArithF64, 1>(const ModDownBgvArgs &);
template <> hipError_t launch_moddown_bgv_fwd<ArithF64, 18>(const ModDownBgvArgs &);
template <> hipError_t launch_moddown_bgv_fwd<ArithF64W, 0>(const ModDownBgvArgs &);

} // namespace ntt
