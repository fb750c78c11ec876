/*
 * ntt_kernels_lift.h -- lift_fwd_kernel: the lift of a plaintext into the RNS fused with the forward transform (NTT_LIFT_TRANSFORMED)
 * for a run of limbs in ONE launch.  Included by the lift_f64*.hip units only (the host layer sees the launchers of ntt_lift.h).
 *
 * rescale_fwd_kernel with another digit function and an additive epilogue.  Per block of limb l (FP64 policies, N = 2^6..2^14, one
 * block = one polynomial):
 *   prologue  the plaintext's block as raw words -- a word mod t up to 2^61, or the bit pattern of a double -- is turned into the
 *             limb's canonical word in integer arithmetic (lift_word, lift_digit), then converted;
 *   stages    the forward block stages, unchanged;
 *   epilogue  canonical words stored in the last group's layout; accumulating, a quarter-tile at a time: c^ read in that layout and
 *             added (the value reduced to |.| <= q/2 first: the sum stays below 1.5 q).
 * 8N bytes of plaintext, shared by the run's limbs, and 8N (16N accumulating) per limb-polynomial.  The mode and the accumulation are
 * wave-uniform run-time fields of the argument record.  The limb is the grid's y index (limb_params MULTI); the x extent is a multiple
 * of 8, as in rescale_fwd_kernel: the limb-blocks reading one plaintext block share blockIdx % 8 (speed only).
 */
#pragma once
#include <hip/hip_runtime.h>

#include "ntt_core.h"
#include "ntt_passplan.h"
#include "ntt_kernels_block.h"
#include "ntt_lift.h"
#include "ntt_kernels_bconv.h"

namespace ntt {

template <class A> struct KLift {
  KArgs<A>        k; /* k.a = limb 0 of the run (c^), limb_stride / poly_stride of the output, the run's limb records */
  const uint64_t *m; /* the plaintext, [batch][N] with its own polynomial stride */
  uint64_t        m_poly_stride;
  uint32_t        accumulate;
  LiftCall        call[1]; /* (an array: read through an opaque index, see the kernel) */
  LiftLimb        ll[kLiftLimbs];
};
static_assert(sizeof(KLift<ArithF64>) < 4096 && sizeof(KLift<ArithF64W>) < 4096, "the kernel-argument record must stay under 4 KB");

template <class A, int LOGN, int KSH>
__global__ void __launch_bounds__((Geom<LOGN, false, flavor_of<A>()>::WG), (Geom<LOGN, false, flavor_of<A>()>::WPS))
  lift_fwd_kernel(const KLift<A> kl)
{
  static_assert(A::kCompact, "built for the FP64 policies");
  uint32_t        bid, gdim, limb;
  const Params<A> p = limb_params<A, false, true>(kl.k, bid, gdim, limb);
  using P = Plan<LOGN>;
  using G = Geom<LOGN, false, flavor_of<A>()>;
  constexpr uint32_t MASK   = fused_mask<A, LOGN, false, KSH>();
  constexpr int      LDS_TW = G::LDS_TW;
  __shared__ typename A::val lds_all[G::BPW * P::LDS_ELEMS + LDS_TW];
  const uint32_t       tid = threadIdx.x;
  const uint32_t       sub = tid >> P::LT;
  const uint32_t       t   = tid & (P::T - 1);
  typename A::val *    lds = lds_all + sub * P::LDS_ELEMS;
  const lds_ctw_ptr<A> gtw = (lds_ctw_ptr<A>)reinterpret_cast<typename A::ctw *>(lds_all + G::BPW * P::LDS_ELEMS);
  if constexpr(LDS_TW > 0) {
    fill_lds_tables<A, LOGN, false>(reinterpret_cast<typename A::ctw *>(lds_all + G::BPW * P::LDS_ELEMS), p, 0u, tid);
    __syncthreads();
  }
  for(uint64_t b0 = (uint64_t)bid * G::BPW; b0 < p.nblocks; b0 += (uint64_t)gdim * G::BPW) {
    uint64_t   b    = b0 + sub;
    const bool live = b < p.nblocks;
    if(!live) b = p.nblocks - 1;
    const uint64_t *mblk = kl.m + b * kl.m_poly_stride; /* (whole polynomials: block b is polynomial b) */
    uint64_t *      cblk = p.a + blk_off<LOGN>(p, b);
    uint32_t        tg   = t; /* (an opaque copy per block, as fwd_mul_kernel's plain loop) */
    asm volatile("" : "+v"(tg));
    typename A::val x[kE];
    {
      /* The lift's constants (36 scalar registers) are read from the kernel arguments per block, through indices the compiler cannot
       * see through: loop invariants, they would otherwise be held across the stages, which at 2^12..2^14 have no scalar register to
       * spare (rescale_fwd_kernel's 14 words of constants fit; these spilled 4-14 registers). */
      uint32_t lz = limb, cz = 0;
      asm volatile("" : "+s"(lz), "+s"(cz));
      const LiftLimb ll   = kl.ll[lz];
      const LiftCall call = kl.call[cz];
      uint64_t       raw[kE];
      static_for<0, kE>([&](auto ee) {
        constexpr int   E   = decltype(ee)::value;
        const uint64_t *row = mblk + ((uint32_t)E << P::LT);
        raw[E]              = lift_digit(lift_word(stream_load(coef_at(row, tg)), call), call.mode, ll);
      });
      convert_inputs<A, false>(x, raw, false, p.c);
    }
    fwd_block_stages<A, LOGN, MASK>(x, tg, p, lds, gtw);
    if(kl.accumulate) {
      static_for<0, 4>([&](auto qq) {
        constexpr int Q = decltype(qq)::value;
        uint64_t      rc[kE], u[kE];
        sched_fence();
        load_last_raw<LOGN, 4 * Q, 4 * Q + 4>(rc, tg, cblk);
        static_for<4 * Q, 4 * Q + 4>([&](auto ee) {
          constexpr int E = decltype(ee)::value;
          u[E]            = A::mul_store_acc(A::reduce(x[E], p.c), rc[E], p.c);
        });
        if(live) store_last_raw<LOGN, 4 * Q, 4 * Q + 4>(u, tg, cblk);
        sched_fence();
      });
    } else {
      static_for<0, 4>([&](auto qq) {
        constexpr int Q = decltype(qq)::value;
        uint64_t      u[kE];
        static_for<4 * Q, 4 * Q + 4>([&](auto ee) {
          constexpr int E = decltype(ee)::value;
          u[E]            = A::mul_store(x[E], p.c);
        });
        if(live) store_last_raw<LOGN, 4 * Q, 4 * Q + 4>(u, tg, cblk);
      });
    }
  }
}

template <class A, int LOGN, int KSH> hipError_t launch_lift_fwd_n(const LiftFwdArgs &la)
{
  using G = Geom<LOGN, false, flavor_of<A>()>;
  if(la.nlimbs < 1 || la.nlimbs > kLiftLimbs || la.nlimbs > kMaxLimbs) return hipErrorInvalidValue;
  KLift<A>       kl{};
  const uint64_t nl = (uint64_t)la.nlimbs;
  fill_kargs(kl.k, la.c, la.limbs, nl, la.limb_stride, la.poly_stride, la.logn, 0, la.batch);
  for(int l = 0; l < la.nlimbs; l++) kl.ll[l] = la.ll[l];
  kl.m             = la.m;
  kl.m_poly_stride = la.m_poly_stride ? la.m_poly_stride : (1ull << la.logn);
  kl.call[0]       = la.call;
  kl.accumulate    = la.call.accumulate;
  /* rescale_fwd_kernel's grid: the plain loop of the forward block kernel, the x extent a multiple of 8 */
  return launch_plain_loop<G, KLift<A>, lift_fwd_kernel<A, LOGN, KSH>>(kl, nl, la.batch, la.num_cus, la.max_grid, true, la.stream);
}

#define NTT_DEFINE_LAUNCH_LIFT_FWD(A, KSH)                                                                                                \
  template <> hipError_t launch_lift_fwd<A, KSH>(const LiftFwdArgs &la)                                                                   \
  {                                                                                                                                       \
    return with_int<6, 14>((int)la.logn, hipErrorNotSupported, [&](auto ln) { return launch_lift_fwd_n<A, decltype(ln)::value, KSH>(la); }); \
  }

} // namespace ntt
