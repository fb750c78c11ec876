/*
 * ntt_rescale.h -- launchers of the RNS rescale kernels (ntt_rns_rescale_batch): the host layer's view of them.
 *
 * The kernel templates live in ntt_kernels_rescale.h and are instantiated in rescale_*.hip only; this header declares the
 * argument records and the launchers, nothing that the host translation unit would instantiate.
 *
 * A rescale drops the last prime q_L of an RNS polynomial: limb l < L becomes (c_l - u_l) * s_l mod q_l with
 *   t   = the dropped limb's coefficients (canonical words mod q_L, up to 2^61),
 *   u_l = ((t + h) mod q_L) mod q_l - h_l  (mod q_l),  h = (q_L - 1) / 2, h_l = h mod q_l  (round; h = h_l = 0: floor),
 *   s_l = q_L^-1 mod q_l.
 * In the NTT domain the subtrahend is fwd_{q_l}(u_l): rescale_fwd_kernel forms u_l in its prologue and runs the forward block
 * stages on it; rescale_coef_kernel is the coefficient form.
 */
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ntt_arith.h"

namespace ntt {

/* the per-limb constants of a rescale (integer words; the FP64 kernels take s_l as a word too) */
struct RescaleLimb {
  uint64_t q;       /* q_l                                      */
  uint64_t bar;     /* floor(2^64 / q_l): Barrett quotient      */
  uint64_t s;       /* q_L^-1 mod q_l                           */
  uint64_t s_shoup; /* floor(s * 2^64 / q_l): Shoup constant    */
  uint64_t h;       /* h mod q_l (0: floor)                     */
};
constexpr int kRescaleLimbs = 16; /* kept limbs of one launch (= kMaxLimbs) */

/* (t + h) mod q_L mod q_l - h_l (mod q_l), exactly, for canonical t < q_L < 2^62 and q_l < 2^62: Barrett with one correction */
NTT_HD uint64_t rescale_digit(uint64_t t, uint64_t qL, uint64_t hL, const RescaleLimb &r)
{
  uint64_t w = t + hL;
  w          = w >= qL ? w - qL : w;
  uint64_t v = w - mulhi64(w, r.bar) * r.q; /* [0, 2q) */
  v          = v >= r.q ? v - r.q : v;
  return v >= r.h ? v - r.h : v + (r.q - r.h);
}

/* coefficients: c_l <- (c_l - u_l) * s_l for up to kRescaleLimbs kept limbs, t read once (rescale_coef.hip) */
struct RescaleCoefArgs {
  uint64_t *      c;           /* limb 0 of the chunk                                      */
  const uint64_t *t;           /* the dropped limb (coefficients)                          */
  uint64_t        limb_stride; /* words between consecutive limbs                          */
  uint64_t        poly_stride; /* words between consecutive polynomials of a limb          */
  uint64_t        batch;
  uint32_t        logn;
  int             nlimbs;
  uint64_t        qL, hL;
  RescaleLimb     limbs[kRescaleLimbs];
  int             max_grid;
  hipStream_t     stream;
};
hipError_t launch_rescale_coef(const RescaleCoefArgs &ra);

/* NTT domain, FP64 policies, N = 2^6..2^14: c_l^ <- (c_l^ - fwd(u_l)) * s_l in ONE launch over a run of limbs
 * (rescale_fwd_kernel; rescale_f64*.hip) */
struct RescaleFwdArgs {
  uint64_t *      c;      /* limb 0 of the run (NTT domain, canonical)       */
  const uint64_t *t;      /* the dropped limb after its inverse transform   */
  const void *    limbs;  /* HOST array of the run's LimbRec<A>             */
  int             nlimbs; /* 1 .. kRescaleLimbs                             */
  uint64_t        limb_stride, poly_stride, batch;
  uint32_t        logn;
  uint64_t        qL, hL;
  RescaleLimb     rl[kRescaleLimbs];
  int             max_grid, num_cus;
  hipStream_t     stream;
};
template <class A, int KSH> hipError_t launch_rescale_fwd(const RescaleFwdArgs &ra);
template <> hipError_t launch_rescale_fwd<ArithF64, 0>(const RescaleFwdArgs &);
template <> hipError_t launch_rescale_fwd<ArithF64, 1>(const RescaleFwdArgs &);
template <> hipError_t launch_rescale_fwd<ArithF64, 18>(const RescaleFwdArgs &);
template <> hipError_t launch_rescale_fwd<ArithF64W, 0>(const RescaleFwdArgs &);

} // namespace ntt
