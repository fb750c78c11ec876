/*
 * ntt_kernels_rescale.h -- rescale_fwd_kernel: the NTT-domain RNS rescale (drop the last prime q_L) for a run of kept limbs in
 * ONE launch.  Included by the rescale_f64*.hip units only (the host layer sees the launchers of ntt_rescale.h).
 *
 * Per block of kept limb l (FP64 policies, N = 2^6..2^14, one block = one polynomial):
 *   prologue  t's block (the dropped limb, already inverse-transformed) as raw words -- up to 2^61, not exact in a double -- is
 *             reduced in integer arithmetic: u_l = ((t + h) mod q_L) mod q_l - h_l (mod q_l) (rescale_digit), then converted;
 *   stages    the forward block stages, unchanged (fwd_mul_kernel's plain loop);
 *   epilogue  a quarter-tile at a time: c^ read in the last group's layout, (c^ - x) * s_l with the limb's FP64 constants
 *             (x and the difference reduced to |.| <= q/2 first: the bounds of ArithF64::mul_out), canonical words stored.
 * 8N bytes of t and 16N of c^ per limb-polynomial, where an inverse + element-wise kernel + forward sandwich moves 48N.
 * The limb is the grid's y index (limb_params MULTI); the x extent is a multiple of 8 so that the limb-blocks reading one t
 * block share blockIdx % 8 -- under the observed round-robin placement one XCD, t read from HBM once per run (speed only).
 */
#pragma once
#include <hip/hip_runtime.h>

/* the block kernels' pieces (Geom, KArgs, limb_params, the stage groups and exchanges) -- not all of ntt_kernels.h, whose launch
 * section defines a kernel of its own (team_ctl_clear_kernel) in every unit that includes it */
#include "ntt_core.h"
#include "ntt_passplan.h"
#include "ntt_kernels_block.h"
#include "ntt_rescale.h"
#include "ntt_kernels_bconv.h"

namespace ntt {

template <class A> struct KRescale {
  KArgs<A>        k;  /* k.a = limb 0 of the run (c^), limb_stride / poly_stride of the operand, the run's limb records */
  const uint64_t *t;  /* the dropped limb's coefficients, laid out like every limb (poly_stride) */
  uint64_t        qL, hL;
  RescaleLimb     rl[kRescaleLimbs];
};

template <class A, int LOGN, int KSH>
__global__ void __launch_bounds__((Geom<LOGN, false, flavor_of<A>()>::WG), (Geom<LOGN, false, flavor_of<A>()>::WPS))
  rescale_fwd_kernel(const KRescale<A> kr)
{
  static_assert(A::kCompact, "built for the FP64 policies");
  uint32_t        bid, gdim, limb;
  const Params<A> p = limb_params<A, false, true>(kr.k, bid, gdim, limb);
  using P = Plan<LOGN>;
  using G = Geom<LOGN, false, flavor_of<A>()>;
  constexpr uint32_t MASK   = fused_mask<A, LOGN, false, KSH>();
  constexpr int      LDS_TW = G::LDS_TW;
  __shared__ typename A::val lds_all[G::BPW * P::LDS_ELEMS + LDS_TW];
  const uint32_t       tid = threadIdx.x;
  const uint32_t       sub = tid >> P::LT;
  const uint32_t       t   = tid & (P::T - 1);
  typename A::val *    lds = lds_all + sub * P::LDS_ELEMS;
  const RescaleLimb    rl  = kr.rl[limb];
  const lds_ctw_ptr<A> gtw = (lds_ctw_ptr<A>)reinterpret_cast<typename A::ctw *>(lds_all + G::BPW * P::LDS_ELEMS);
  if constexpr(LDS_TW > 0) {
    fill_lds_tables<A, LOGN, false>(reinterpret_cast<typename A::ctw *>(lds_all + G::BPW * P::LDS_ELEMS), p, 0u, tid);
    __syncthreads();
  }
  /* s_l as a balanced double, |.| <= q/2 (the multiplier of every product of this workgroup) */
  const double sb = A::reduce(A::u64_to_f64_lt52(rl.s), p.c);
  for(uint64_t b0 = (uint64_t)bid * G::BPW; b0 < p.nblocks; b0 += (uint64_t)gdim * G::BPW) {
    uint64_t   b    = b0 + sub;
    const bool live = b < p.nblocks;
    if(!live) b = p.nblocks - 1;
    const uint64_t  off  = blk_off<LOGN>(p, b); /* (whole polynomials: s0 = 0) */
    const uint64_t *tblk = kr.t + off;
    uint64_t *      cblk = p.a + off;
    uint32_t        tg   = t; /* (an opaque copy per block, as fwd_mul_kernel's plain loop) */
    asm volatile("" : "+v"(tg));
    typename A::val x[kE];
    {
      uint64_t raw[kE];
      static_for<0, kE>([&](auto ee) {
        constexpr int   E   = decltype(ee)::value;
        const uint64_t *row = tblk + ((uint32_t)E << P::LT);
        raw[E]              = rescale_digit(stream_load(coef_at(row, tg)), kr.qL, kr.hL, rl);
      });
      convert_inputs<A, false>(x, raw, false, p.c);
    }
    fwd_block_stages<A, LOGN, MASK>(x, tg, p, lds, gtw);
    static_for<0, 4>([&](auto qq) {
      constexpr int Q = decltype(qq)::value;
      uint64_t      rc[kE], u[kE];
      sched_fence();
      load_last_raw<LOGN, 4 * Q, 4 * Q + 4>(rc, tg, cblk);
      static_for<4 * Q, 4 * Q + 4>([&](auto ee) {
        constexpr int E = decltype(ee)::value;
        const double  d = A::reduce(A::u64_to_f64_lt52(rc[E]) - A::reduce(x[E], p.c), p.c); /* |c^ - x| < 1.5 q before */
        u[E]            = A::mul_store(A::mulmod_c(sb, d, p.c), p.c);
      });
      if(live) store_last_raw<LOGN, 4 * Q, 4 * Q + 4>(u, tg, cblk);
      sched_fence();
    });
  }
}

template <class A, int LOGN, int KSH> hipError_t launch_rescale_fwd_n(const RescaleFwdArgs &ra)
{
  using G = Geom<LOGN, false, flavor_of<A>()>;
  if(ra.nlimbs < 1 || ra.nlimbs > kRescaleLimbs || ra.nlimbs > kMaxLimbs) return hipErrorInvalidValue;
  KRescale<A>    kr{};
  const uint64_t nl = (uint64_t)ra.nlimbs;
  fill_kargs(kr.k, ra.c, ra.limbs, nl, ra.limb_stride, ra.poly_stride, ra.logn, 0, ra.batch);
  for(int l = 0; l < ra.nlimbs; l++) kr.rl[l] = ra.rl[l];
  kr.t  = ra.t;
  kr.qL = ra.qL;
  kr.hL = ra.hL;
  /* the x extent a multiple of 8 (the header's note on the XCDs) */
  return launch_plain_loop<G, KRescale<A>, rescale_fwd_kernel<A, LOGN, KSH>>(kr, nl, ra.batch, ra.num_cus, ra.max_grid, true, ra.stream);
}

#define NTT_DEFINE_LAUNCH_RESCALE_FWD(A, KSH)                                                                                                   \
  template <> hipError_t launch_rescale_fwd<A, KSH>(const RescaleFwdArgs &ra)                                                                   \
  {                                                                                                                                             \
    return with_int<6, 14>((int)ra.logn, hipErrorNotSupported, [&](auto ln) { return launch_rescale_fwd_n<A, decltype(ln)::value, KSH>(ra); }); \
  }

} // namespace ntt
