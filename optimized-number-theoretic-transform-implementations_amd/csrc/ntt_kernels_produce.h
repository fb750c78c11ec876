/*
 * ntt_kernels_produce.h -- produce_fwd_body: the ONE body of the kernels that produce a polynomial into the RNS fused with the forward
 * transform, and the one launcher of them: the lifts of a plaintext (ntt_kernels_lift.h) and the device-side sampler
 * (ntt_kernels_sample.h).  A producer writes one canonical word per coefficient and limb from a source of its own -- a loaded plaintext
 * word, a block of a counter-based generator -- and differs from the others in that source alone.  Each kernel keeps its name, launch
 * bounds and argument record and states its digit as the body's `fill`.
 *
 * rescale_fwd_kernel (ntt_kernels_rescale.h) with another digit function and an additive epilogue.  Per block of limb l (FP64 policies,
 * N = 2^6..2^14, one block = one polynomial):
 *   prologue  the producer's `fill`: the thread's kE canonical words, in integer arithmetic; then converted;
 *   stages    the forward block stages, unchanged;
 *   epilogue  canonical words stored in the last group's layout; accumulating, a quarter-tile at a time: c^ read in that layout and
 *             added (the value reduced to |.| <= q/2 first: the sum stays below 1.5 q).
 * 8N (16N accumulating) bytes per limb-polynomial beside what `fill` reads.  The accumulation is a wave-uniform run-time field of the
 * argument record.  The limb is the grid's y index (limb_params MULTI); the x extent is a multiple of 8, as in rescale_fwd_kernel: the
 * limb-blocks of one polynomial share blockIdx % 8 (speed only).
 *
 * A new producer: a call record and its digit functions (as ntt_lift.h's), ProduceArgs (ntt_produce.h) with that call, a kernel that passes its
 * `fill` to the body, and an entry point in front of produce_route (host/host_produce.inc).  The coefficient kernels (lift.hip,
 * sample.hip) are not folded: the same loop behind a function boundary costs each two vector registers (profiles/r24/refactor_codegen.txt).
 */
#pragma once
#include <hip/hip_runtime.h>

#include "ntt_core.h"
#include "ntt_passplan.h"
#include "ntt_kernels_block.h"
#include "ntt_produce.h"
#include "ntt_kernels_bconv.h"

namespace ntt {

/* K: k (k.a = limb 0 of the run (c^), limb_stride / poly_stride of the output, the run's limb records), accumulate, call[1],
 * ll[kProduceLimbs].  fill(raw, b, tg, lz, ll, call) writes the kE canonical words of lane tg in block b (= polynomial b) of limb lz of the
 * launch: word E is coefficient (E << Plan<LOGN>::LT) + tg. */
template <class A, int LOGN, int KSH, class K, class Fill> __device__ __forceinline__ void produce_fwd_body(const K &kr, Fill &&fill)
{
  static_assert(A::kCompact, "built for the FP64 policies");
  static_assert(sizeof(K) < 4096, "the kernel-argument record must stay under 4 KB");
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
  const lds_ctw_ptr<A> gtw = (lds_ctw_ptr<A>)reinterpret_cast<typename A::ctw *>(lds_all + G::BPW * P::LDS_ELEMS);
  if constexpr(LDS_TW > 0) {
    fill_lds_tables<A, LOGN, false>(reinterpret_cast<typename A::ctw *>(lds_all + G::BPW * P::LDS_ELEMS), p, 0u, tid);
    __syncthreads();
  }
  for(uint64_t b0 = (uint64_t)bid * G::BPW; b0 < p.nblocks; b0 += (uint64_t)gdim * G::BPW) {
    uint64_t   b    = b0 + sub;
    const bool live = b < p.nblocks;
    if(!live) b = p.nblocks - 1;
    uint64_t *cblk = p.a + blk_off<LOGN>(p, b); /* (whole polynomials: block b is polynomial b) */
    uint32_t  tg   = t;                         /* (an opaque copy per block, as fwd_mul_kernel's plain loop) */
    asm volatile("" : "+v"(tg));
    typename A::val x[kE];
    {
      /* The producer's constants (the lift's: 36 scalar registers, the sampler's: 22) are read from the kernel arguments per block,
       * through indices the compiler cannot see through: loop invariants, they would otherwise be held across the stages, which at
       * 2^12..2^14 have no scalar register to spare (rescale_fwd_kernel's 14 words of constants fit; the lift's spilled 4-14
       * registers). */
      uint32_t lz = limb, cz = 0;
      asm volatile("" : "+s"(lz), "+s"(cz));
      const auto ll   = kr.ll[lz];
      const auto call = kr.call[cz];
      uint64_t   raw[kE];
      fill(raw, b, tg, lz, ll, call);
      convert_inputs<A, false>(x, raw, false, p.c);
    }
    fwd_block_stages<A, LOGN, MASK>(x, tg, p, lds, gtw);
    if(kr.accumulate) {
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

/* The launcher of the fused kernels: the argument check, the common fields of the record K, `extra(kr)` for the producer's own, the
 * launch of Kernel over rescale_fwd_kernel's grid (the plain loop of the forward block kernel, the x extent a multiple of 8). */
template <class A, int LOGN, class K, void (&Kernel)(const K), class Args, class F> hipError_t launch_produce_fwd_n(const Args &pa, F &&extra)
{
  using G = Geom<LOGN, false, flavor_of<A>()>;
  if(pa.nlimbs < 1 || pa.nlimbs > kProduceLimbs || pa.nlimbs > kMaxLimbs) return hipErrorInvalidValue;
  K              kr{};
  const uint64_t nl = (uint64_t)pa.nlimbs;
  fill_kargs(kr.k, pa.c, pa.limbs, nl, pa.limb_stride, pa.poly_stride, pa.logn, 0, pa.batch);
  for(int l = 0; l < pa.nlimbs; l++) kr.ll[l] = pa.ll[l];
  kr.call[0]    = pa.call;
  kr.accumulate = pa.call.accumulate;
  extra(kr);
  return launch_plain_loop<G, K, Kernel>(kr, nl, pa.batch, pa.num_cus, pa.max_grid, true, pa.stream);
}

/* the body of a producer's launch_*_fwd<A, KSH>: N = 2^6..2^14 to its instance */
#define NTT_LAUNCH_PRODUCE_FWD(A, KSH, K, kernel, pa, extra)                                                                               \
  with_int<6, 14>((int)(pa).logn, hipErrorNotSupported, [&](auto ln) {                                                                     \
    return launch_produce_fwd_n<A, decltype(ln)::value, K<A>, kernel<A, decltype(ln)::value, KSH>>(pa, extra);                              \
  })

} // namespace ntt
