/*
 * ntt_kernels_slots.h -- slots_inv_kernel and slots_fwd_kernel: the BFV / BGV slot encode and decode fused with the transform mod t,
 * ONE launch per call.  Included by the slots_f64*.hip units only (the host layer sees the launcher of ntt_slots.h, which states the
 * slot order).
 *
 * FP64 policies, N = 2^6..2^14, one block = one polynomial = one workgroup's work:
 *   slots_inv_kernel  (encode) the inverse block stages behind another load: the lane reads the table words ipos[s] for the positions
 *                     s of the last group's layout (what global_load_last reads: runs of 2^RL consecutive s, so the table words come as
 *                     8-byte pairs) and gathers v[ipos[s]]; the coefficients leave in natural order, as ever;
 *   slots_fwd_kernel  (decode) the forward block stages (rescale_fwd_kernel's plain loop), then word s is scattered to v[ipos[s]].
 * Every gathered or scattered word belongs to the workgroup's own polynomial (the table words are masked to N: at most 128 KiB); the
 * 4N-byte table is shared by the batch.  16N algorithmic bytes per polynomial.  The coefficient side of decode is only read.
 */
#pragma once
#include <hip/hip_runtime.h>

#include "ntt_core.h"
#include "ntt_passplan.h"
#include "ntt_kernels_block.h"
#include "ntt_slots.h"
#include "ntt_kernels_bconv.h"

namespace ntt {

template <class A> struct KSlots {
  KArgs<A>        k;    /* k.a = the coefficient side, poly_stride its stride, limbs[0] the plan's record */
  uint64_t *      v;    /* the slot side */
  uint64_t        v_stride;
  const uint32_t *ipos;
};

/* the table words of slots E, E + 1 of the last group's layout (consecutive positions, the first one even) */
template <int LOGN, int E> __device__ __forceinline__ void slots_index_pair(uint32_t &i0, uint32_t &i1, const uint32_t *ipos, uint32_t ib)
{
  using P          = Plan<LOGN>;
  constexpr int G  = P::NG - 1;
  static_assert((P::IOFF(G, E) & 1u) == 0 && P::IOFF(G, E + 1) == P::IOFF(G, E) + 1, "slots E, E + 1 are neighbours");
  const uint2 w = *reinterpret_cast<const uint2 *>(reinterpret_cast<const char *>(ipos + P::IOFF(G, E)) + (uint32_t)(ib * 4u));
  i0            = w.x & ((1u << LOGN) - 1u);
  i1            = w.y & ((1u << LOGN) - 1u);
}

template <class A, int LOGN, int KSH>
__global__ void __launch_bounds__((Geom<LOGN, true, flavor_of<A>()>::WG), (Geom<LOGN, true, flavor_of<A>()>::WPS))
  slots_inv_kernel(const KSlots<A> ks)
{
  static_assert(A::kCompact, "built for the FP64 policies");
  uint32_t        bid, gdim, limb;
  const Params<A> p = limb_params<A, true, false>(ks.k, bid, gdim, limb);
  using P = Plan<LOGN>;
  using G = Geom<LOGN, true, flavor_of<A>()>;
  /* whole polynomials: the pass ends the transform (N^-1 folded in); the slot words are canonical (fused_kernel's mask) */
  constexpr uint32_t MASK   = fused_mask<A, LOGN, true, KSH>() | kLastInvFlag | (A::kWide52 ? kCanonInFlag : 0u);
  constexpr int      GL     = P::NG - 1;
  constexpr int      LDS_TW = G::LDS_TW;
  __shared__ typename A::val lds_all[G::BPW * P::LDS_ELEMS + LDS_TW];
  const uint32_t       tid = threadIdx.x;
  const uint32_t       sub = tid >> P::LT;
  const uint32_t       t   = tid & (P::T - 1);
  typename A::val *    lds = lds_all + sub * P::LDS_ELEMS;
  const lds_ctw_ptr<A> gtw = (lds_ctw_ptr<A>)reinterpret_cast<typename A::ctw *>(lds_all + G::BPW * P::LDS_ELEMS);
  if constexpr(LDS_TW > 0) {
    fill_lds_tables<A, LOGN, true>(reinterpret_cast<typename A::ctw *>(lds_all + G::BPW * P::LDS_ELEMS), p, 0u, tid);
    __syncthreads();
  }
  for(uint64_t b0 = (uint64_t)bid * G::BPW; b0 < p.nblocks; b0 += (uint64_t)gdim * G::BPW) {
    uint64_t   b    = b0 + sub;
    const bool live = b < p.nblocks;
    if(!live) b = p.nblocks - 1; /* idle sub-blocks shadow a real block (barriers are workgroup-wide), never store */
    const uint64_t *vblk = ks.v + b * ks.v_stride;
    uint64_t *      ablk = p.a + blk_off<LOGN>(p, b);
    uint32_t        tg   = t; /* (an opaque copy per block, as rescale_fwd_kernel's loop) */
    asm volatile("" : "+v"(tg));
    typename A::val x[kE];
    {
      uint64_t       raw[kE];
      const uint32_t ib = P::IBASE(GL, tg);
      static_for<0, kE / 2>([&](auto hh) {
        constexpr int E = 2 * decltype(hh)::value;
        uint32_t      i0, i1;
        slots_index_pair<LOGN, E>(i0, i1, ks.ipos, ib);
        raw[E]     = stream_load(coef_at(vblk, i0));
        raw[E + 1] = stream_load(coef_at(vblk, i1));
      });
      convert_inputs<A, true>(x, raw, false, p.c);
    }
    run_group<A, LOGN, GL, true, MASK, (G::TBL(GL) > 0)>(x, tg, 0u, p, gtw + G::TBL_OFF(GL));
    static_for<0, P::NG - 1>([&](auto gg) {
      constexpr int GI = P::NG - 1 - decltype(gg)::value;
      exchange<A, LOGN, GI, GI - 1>(x, tg, lds);
      run_group<A, LOGN, GI - 1, true, MASK, (G::TBL(GI - 1) > 0)>(x, tg, 0u, p, gtw + G::TBL_OFF(GI - 1));
    });
    if(live) global_store_first<A, LOGN, true>(x, tg, ablk, p.c, false);
  }
}

template <class A, int LOGN, int KSH>
__global__ void __launch_bounds__((Geom<LOGN, false, flavor_of<A>()>::WG), (Geom<LOGN, false, flavor_of<A>()>::WPS))
  slots_fwd_kernel(const KSlots<A> ks)
{
  static_assert(A::kCompact, "built for the FP64 policies");
  uint32_t        bid, gdim, limb;
  const Params<A> p = limb_params<A, false, false>(ks.k, bid, gdim, limb);
  using P = Plan<LOGN>;
  using G = Geom<LOGN, false, flavor_of<A>()>;
  constexpr uint32_t MASK   = fused_mask<A, LOGN, false, KSH>();
  constexpr int      GL     = P::NG - 1;
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
    const uint64_t *ablk = p.a + blk_off<LOGN>(p, b);
    uint64_t *      vblk = ks.v + b * ks.v_stride;
    uint32_t        tg   = t; /* (an opaque copy per block, as rescale_fwd_kernel's loop) */
    asm volatile("" : "+v"(tg));
    typename A::val x[kE];
    global_load_first<A, LOGN, false>(x, tg, ablk, false, p.c);
    fwd_block_stages<A, LOGN, MASK>(x, tg, p, lds, gtw);
    const uint32_t ib = P::IBASE(GL, tg);
    static_for<0, kE / 2>([&](auto hh) {
      constexpr int E = 2 * decltype(hh)::value;
      uint32_t      i0, i1;
      slots_index_pair<LOGN, E>(i0, i1, ks.ipos, ib);
      const uint64_t u0 = out_word<A, false, false>(x[E], false, p.c), u1 = out_word<A, false, false>(x[E + 1], false, p.c);
      if(live) {
        stream_store(coef_at(vblk, i0), u0);
        stream_store(coef_at(vblk, i1), u1);
      }
    });
  }
}

template <class A, int LOGN, int KSH> hipError_t launch_slots_n(const SlotsArgs &sa)
{
  KSlots<A> ks{};
  fill_kargs(ks.k, sa.a, sa.limb, 1, 0, sa.a_stride, sa.logn, 0, sa.batch);
  ks.k.lastinv = sa.encode ? 1u : 0u;
  ks.v         = sa.v;
  ks.v_stride  = sa.v_stride ? sa.v_stride : (1ull << sa.logn);
  ks.ipos      = sa.ipos;
  /* the grids of the kernels this loop is shared with (launch_plain_loop); one limb: no rounding to eights */
  if(sa.encode) {
    using G = Geom<LOGN, true, flavor_of<A>()>;
    return launch_plain_loop<G, KSlots<A>, slots_inv_kernel<A, LOGN, KSH>>(ks, 1, sa.batch, sa.num_cus, sa.max_grid, false, sa.stream);
  }
  using G = Geom<LOGN, false, flavor_of<A>()>;
  return launch_plain_loop<G, KSlots<A>, slots_fwd_kernel<A, LOGN, KSH>>(ks, 1, sa.batch, sa.num_cus, sa.max_grid, false, sa.stream);
}

#define NTT_DEFINE_LAUNCH_SLOTS(A, KSH)                                                                                            \
  template <> hipError_t launch_slots<A, KSH>(const SlotsArgs &sa)                                                                 \
  {                                                                                                                                \
    if(!sa.a || !sa.v || !sa.ipos || !sa.limb) return hipErrorInvalidValue;                                                        \
    return with_int<6, 14>((int)sa.logn, hipErrorNotSupported, [&](auto ln) { return launch_slots_n<A, decltype(ln)::value, KSH>(sa); }); \
  }

} // namespace ntt
