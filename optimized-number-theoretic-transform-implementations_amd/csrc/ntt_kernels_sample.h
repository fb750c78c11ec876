/*
 * ntt_kernels_sample.h -- sample_fwd_kernel: a random polynomial drawn in the RNS fused with the forward transform
 * (NTT_SAMPLE_TRANSFORMED) for a run of limbs in ONE launch.  Included by the sample_f64*.hip units only (the host layer sees the
 * launchers of ntt_sample.h).
 *
 * lift_fwd_kernel's frame with the plaintext load replaced by a counter-based generator.  Per block of limb l (FP64 policies,
 * N = 2^6..2^14, one block = one polynomial):
 *   prologue  for each of the thread's kE coefficients the Philox block of (P, s) and the limb's canonical word in integer arithmetic
 *             (sample_block, sample_small / sample_small_digit, sample_uniform_digit), then converted.  Nothing is read.  The small
 *             kinds' block is the same in every limb's workgroup and is computed again in each: ten rounds of two 32 x 32 -> 64-bit
 *             products per coefficient and limb, where the composition's element-wise launch computes it once per coefficient;
 *   stages    the forward block stages, unchanged;
 *   epilogue  canonical words stored in the last group's layout; accumulating, a quarter-tile at a time: c^ read in that layout and
 *             added (lift_fwd_kernel's epilogue).
 * 8N bytes (16N accumulating) per limb-polynomial.  The kind, the multiplier and the accumulation are wave-uniform run-time fields of the
 * argument record.  The limb is the grid's y index (limb_params MULTI); the grid is lift_fwd_kernel's.
 */
#pragma once
#include <hip/hip_runtime.h>

#include "ntt_core.h"
#include "ntt_passplan.h"
#include "ntt_kernels_block.h"
#include "ntt_sample.h"
#include "ntt_kernels_bconv.h"

namespace ntt {

template <class A> struct KSample {
  KArgs<A>   k; /* k.a = limb 0 of the run (c^), limb_stride / poly_stride of the output, the run's limb records */
  uint32_t   accumulate;
  SampleCall call[1]; /* (an array: read through an opaque index, see the kernel) */
  SampleLimb ll[kSampleLimbs];
};
static_assert(sizeof(KSample<ArithF64>) < 4096 && sizeof(KSample<ArithF64W>) < 4096, "the kernel-argument record must stay under 4 KB");

template <class A, int LOGN, int KSH>
__global__ void __launch_bounds__((Geom<LOGN, false, flavor_of<A>()>::WG), (Geom<LOGN, false, flavor_of<A>()>::WPS))
  sample_fwd_kernel(const KSample<A> ks)
{
  static_assert(A::kCompact, "built for the FP64 policies");
  uint32_t        bid, gdim, limb;
  const Params<A> p = limb_params<A, false, true>(ks.k, bid, gdim, limb);
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
      /* The call's constants (22 scalar registers) are read from the kernel arguments per block, through indices the compiler cannot
       * see through, as in lift_fwd_kernel: loop invariants, they would otherwise be held across the stages, which at 2^12..2^14 have
       * no scalar register to spare. */
      uint32_t lz = limb, cz = 0;
      asm volatile("" : "+s"(lz), "+s"(cz));
      const SampleLimb ll      = ks.ll[lz];
      const SampleCall call    = ks.call[cz];
      const uint64_t   Pn      = call.first_poly + b;
      const bool       uniform = call.kind == kSampleUniform;
      const uint32_t   tag     = sample_tag(call.kind, call.limb0 + lz);
      uint64_t         raw[kE];
      static_for<0, kE>([&](auto ee) {
        constexpr int     E   = decltype(ee)::value;
        const SampleBlock blk = sample_block(call, Pn, ((uint32_t)E << P::LT) + tg, tag);
        raw[E]                = uniform ? sample_uniform_digit(blk, ll) : sample_small_digit(sample_small(call.kind, blk), ll);
      });
      convert_inputs<A, false>(x, raw, false, p.c);
    }
    fwd_block_stages<A, LOGN, MASK>(x, tg, p, lds, gtw);
    if(ks.accumulate) {
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

template <class A, int LOGN, int KSH> hipError_t launch_sample_fwd_n(const SampleFwdArgs &sa)
{
  using G = Geom<LOGN, false, flavor_of<A>()>;
  if(sa.nlimbs < 1 || sa.nlimbs > kSampleLimbs || sa.nlimbs > kMaxLimbs) return hipErrorInvalidValue;
  KSample<A>     ks{};
  const uint64_t nl = (uint64_t)sa.nlimbs;
  fill_kargs(ks.k, sa.c, sa.limbs, nl, sa.limb_stride, sa.poly_stride, sa.logn, 0, sa.batch);
  for(int l = 0; l < sa.nlimbs; l++) ks.ll[l] = sa.ll[l];
  ks.call[0]    = sa.call;
  ks.accumulate = sa.call.accumulate;
  /* lift_fwd_kernel's grid: the plain loop of the forward block kernel, the x extent a multiple of 8 */
  return launch_plain_loop<G, KSample<A>, sample_fwd_kernel<A, LOGN, KSH>>(ks, nl, sa.batch, sa.num_cus, sa.max_grid, true, sa.stream);
}

#define NTT_DEFINE_LAUNCH_SAMPLE_FWD(A, KSH)                                                                                                  \
  template <> hipError_t launch_sample_fwd<A, KSH>(const SampleFwdArgs &sa)                                                                   \
  {                                                                                                                                           \
    return with_int<6, 14>((int)sa.logn, hipErrorNotSupported, [&](auto ln) { return launch_sample_fwd_n<A, decltype(ln)::value, KSH>(sa); }); \
  }

} // namespace ntt
