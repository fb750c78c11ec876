/*
 * ntt_kernels_modup_mul.h -- modup_mul_kernel and modup_mul2_kernel: one digit's term of the key-switching inner product for ONE
 * component or for BOTH components of the key,
 *   c^ (+)= fwd(ModUp(digit)) (.) key^        or        c0^ (+)= fwd(ModUp(digit)) (.) key0^,   c1^ (+)= fwd(ModUp(digit)) (.) key1^,
 * for a run of limbs of the extended basis in ONE launch.  One body, templated on the number of components NC; the two kernels are
 * its instances under their own names.  Included by the modup_mul_f64*.hip (NC = 1) and modup_mul2_f64*.hip (NC = 2) units only
 * (the host layer sees the launchers of ntt_keyswitch.h).
 *
 * moddown_fwd_kernel's skeleton (ntt_kernels_keyswitch.h) with fwd_mul_kernel's plain-loop epilogue (ntt_kernels_products.h).  Per
 * block of limb l (FP64 policies, N = 2^6..2^14, one block = one polynomial):
 *   prologue  l is one of the digit's own limbs (a bit of the kernel arguments, workgroup-uniform): its block as it stands.
 *             Otherwise the digit's count blocks as raw words -- up to 2^61, not exact in a double -- are converted in integer
 *             arithmetic: FastBConv_{B->q_l} (ntt_keyswitch.h), canonical, word for word what bconv_kernel would have written into
 *             the operand's slot l; with count = 1 Barrett of the word itself.  Then converted;
 *   stages    the forward block stages, unchanged;
 *   epilogue  once per component, a quarter-tile at a time: key_j^ (and c_j^ when accumulating) read in the last group's layout, the
 *             product, c_j^ stored.  x[] is the only state live across the passes -- the register set of one quarter-tile product,
 *             not of two (fwd_mul_kernel's note: two products at a time do not fit).
 * Per limb-polynomial 8N count bytes of the digit, 8N NC of the keys (from the L2 when they are broadcast) and 8N NC (16N NC
 * accumulating) of c^; the extended digit never exists in memory, and one conversion and one set of forward stages serve both
 * products.  [b^_i]_{q_l} = prod_{k != i} b_k mod q_l is formed once per workgroup (its limb is the grid's y index) into LDS, as
 * moddown_fwd_kernel forms its [p^_j]_{q_l}: a 16 x 16 table has no room in the kernel arguments.
 * With every limb of the run marked as the digit's own (own = all ones) the prologue is the plain load of the operand and the kernel
 * is the forward-multiply, c_j^ (+)= fwd(a) (.) b_j^ (the host layer uses its pair form).
 * Component 0 is stored before component 1's key is read: c_j^ may coincide with key_j^ as in fwd_mul_kernel, and the host layer
 * refuses c0^ against key1^ (and c1^ against key0^).
 */
#pragma once
#include <hip/hip_runtime.h>

/* the block kernels' pieces (see ntt_kernels_moddown.h on why not all of ntt_kernels.h) */
#include "ntt_core.h"
#include "ntt_passplan.h"
#include "ntt_kernels_block.h"
#include "ntt_kernels_bconv.h"

namespace ntt {

template <class A, int NC> struct KModUpMul {
  KArgs<A>        k;             /* k.a = the run's first limb of the extended operand (a digit limb of the run is read there) */
  const uint64_t *dig;           /* the digit's first limb, coefficients; digit limb i at dig + i * k.limb_stride */
  const uint64_t *b[NC];         /* key_j^, the run's first limb */
  uint64_t *      out[NC];       /* c_j^, the run's first limb (k.limb_stride / k.poly_stride, as the extended operand) */
  uint64_t        b_limb_stride; /* words between consecutive limbs of a key^ */
  uint32_t        lazy_in, b_bcast, accumulate; /* as KMul's */
  uint32_t        own;           /* bit l: limb l of the run is one of the digit's own limbs */
  int             count;
  BconvSrc        sl[kBconvLimbs];
  BconvDst        dl[kBconvLimbs];
};

template <class A, int LOGN, int KSH, int NC> __device__ __forceinline__ void modup_mul_body(const KModUpMul<A, NC> &kr)
{
  static_assert(A::kCompact, "built for the FP64 policies");
  uint32_t        bid, gdim, limb;
  const Params<A> p = limb_params<A, false, true>(kr.k, bid, gdim, limb);
  using P = Plan<LOGN>;
  using G = Geom<LOGN, false, flavor_of<A>()>;
  constexpr uint32_t MASK   = fused_mask<A, LOGN, false, KSH>();
  constexpr int      LDS_TW = G::LDS_TW;
  __shared__ typename A::val lds_all[G::BPW * P::LDS_ELEMS + LDS_TW];
  __shared__ uint64_t        ghat[kBconvLimbs]; /* [b^_i]_{q_l} */
  const uint32_t       tid   = threadIdx.x;
  const uint32_t       sub   = tid >> P::LT;
  const uint32_t       t     = tid & (P::T - 1);
  typename A::val *    lds   = lds_all + sub * P::LDS_ELEMS;
  const BconvDst       dl    = kr.dl[limb];
  const int            count = kr.count;
  const bool           own   = ((kr.own >> limb) & 1u) != 0;
  const bool           lazy  = kr.lazy_in != 0;
  const bool           bc    = kr.b_bcast != 0;
  const bool           acc   = kr.accumulate != 0;
  const uint64_t       boff  = (uint64_t)limb * kr.b_limb_stride;
  const uint64_t       coff  = (uint64_t)limb * kr.k.limb_stride;
  const lds_ctw_ptr<A> gtw   = (lds_ctw_ptr<A>)reinterpret_cast<typename A::ctw *>(lds_all + G::BPW * P::LDS_ELEMS);
  if constexpr(LDS_TW > 0) fill_lds_tables<A, LOGN, false>(reinterpret_cast<typename A::ctw *>(lds_all + G::BPW * P::LDS_ELEMS), p, 0u, tid);
  if(!own && count > 1) bconv_ghat(ghat, kr.sl, count, dl, tid);
  __syncthreads(); /* (the tables and ghat; every condition above is workgroup-uniform) */
  for(uint64_t b0 = (uint64_t)bid * G::BPW; b0 < p.nblocks; b0 += (uint64_t)gdim * G::BPW) {
    uint64_t   b    = b0 + sub;
    const bool live = b < p.nblocks;
    if(!live) b = p.nblocks - 1;
    const uint64_t  off  = blk_off<LOGN>(p, b); /* (whole polynomials: s0 = 0) */
    const uint64_t *dblk = kr.dig + off;
    const uint64_t  bo   = bc ? boff : boff + off; /* a broadcast key^ is one dense polynomial per limb */
    const uint64_t  co   = coff + off;
    uint32_t        tg   = t; /* (an opaque copy per block, as fwd_mul_kernel's plain loop) */
    asm volatile("" : "+v"(tg));
    typename A::val x[kE];
    {
      uint64_t raw[kE];
      if(own) {
        const uint64_t *ablk = p.a + off;
        static_for<0, kE>([&](auto ee) {
          constexpr int   E   = decltype(ee)::value;
          const uint64_t *row = ablk + ((uint32_t)E << P::LT);
          raw[E]              = stream_load(coef_at(row, tg));
        });
      } else if(count == 1) {
        /* b^ = 1, z = x: Barrett of the word itself */
        static_for<0, kE>([&](auto ee) {
          constexpr int   E   = decltype(ee)::value;
          const uint64_t *row = dblk + ((uint32_t)E << P::LT);
          raw[E]              = bconv_reduce64(stream_load(coef_at(row, tg)), dl);
        });
      } else {
        bconv_tile<P::LT>(raw, dblk, kr.k.limb_stride, kr.sl, ghat, count, tg, [&](uint64_t hi, uint64_t lo) {
          const uint64_t v = bconv_reduce(hi, lo, dl);
          return v >= dl.q ? v - dl.q : v;
        });
      }
      convert_inputs<A, false>(x, raw, false, p.c);
    }
    fwd_block_stages<A, LOGN, MASK>(x, tg, p, lds, gtw);
    /* one component at a time, a quarter-tile at a time: x[] is the only state carried from one pass to the next */
    static_for<0, NC>([&](auto jj) {
      constexpr int   J    = decltype(jj)::value;
      const uint64_t *bblk = kr.b[J] + bo;
      uint64_t *      cblk = kr.out[J] + co;
      static_for<0, 4>([&](auto qq) {
        constexpr int Q = decltype(qq)::value;
        uint64_t      rb[kE], rc[kE], u[kE];
        sched_fence();
        load_last_raw<LOGN, 4 * Q, 4 * Q + 4>(rb, tg, bblk);
        /* (the accumulator words: c_j^ itself, or zeros when the call does not accumulate) */
        if(acc) load_last_raw<LOGN, 4 * Q, 4 * Q + 4>(rc, tg, cblk);
        else static_for<4 * Q, 4 * Q + 4>([&](auto ee) { rc[decltype(ee)::value] = 0; });
        mul_out_tile<A, 4 * Q, 4 * Q + 4, 1>(u, x, rb, rc, lazy, p.c);
        if(live) store_last_raw<LOGN, 4 * Q, 4 * Q + 4>(u, tg, cblk);
        sched_fence();
      });
    });
  }
}

/* the body's two instances under the names that tests, traces and profiles key on */
template <class A, int LOGN, int KSH>
__global__ void __launch_bounds__((Geom<LOGN, false, flavor_of<A>()>::WG), (Geom<LOGN, false, flavor_of<A>()>::WPS))
  modup_mul_kernel(const KModUpMul<A, 1> kr)
{
  modup_mul_body<A, LOGN, KSH, 1>(kr);
}

template <class A, int LOGN, int KSH>
__global__ void __launch_bounds__((Geom<LOGN, false, flavor_of<A>()>::WG), (Geom<LOGN, false, flavor_of<A>()>::WPS))
  modup_mul2_kernel(const KModUpMul<A, 2> kr)
{
  modup_mul_body<A, LOGN, KSH, 2>(kr);
}

template <class A, int LOGN, int KSH, int NC> hipError_t launch_modup_mul_n(const ModUpMulArgs &ma)
{
  using G = Geom<LOGN, false, flavor_of<A>()>;
  if(ma.ncomp != NC || ma.nlimbs < 1 || ma.nlimbs > kBconvLimbs || ma.nlimbs > kMaxLimbs || ma.count < 1 || ma.count > kBconvLimbs)
    return hipErrorInvalidValue;
  KModUpMul<A, NC> kr{};
  const uint64_t   nl = (uint64_t)ma.nlimbs;
  fill_kargs(kr.k, ma.a, ma.limbs, nl, ma.limb_stride, ma.poly_stride, ma.logn, 0, ma.batch);
  for(int l = 0; l < ma.nlimbs; l++) kr.dl[l] = ma.dl[l];
  for(int j = 0; j < ma.count; j++) kr.sl[j] = ma.sl[j];
  kr.dig = ma.dig;
  for(int j = 0; j < NC; j++) {
    kr.b[j]   = ma.b[j];
    kr.out[j] = ma.out[j];
  }
  kr.b_limb_stride = ma.b_limb_stride;
  kr.lazy_in       = ma.lazy_in ? 1u : 0u;
  kr.b_bcast       = ma.b_bcast ? 1u : 0u;
  kr.accumulate    = ma.accumulate ? 1u : 0u;
  kr.own           = ma.own;
  kr.count         = ma.count;
  /* moddown_fwd_kernel's grid: the plain loop of the forward block kernel, the x extent a multiple of 8 so that the limb-blocks
   * reading one block of the digit share blockIdx % 8 (speed only).  NTT_OPT_MAX_GRID is taken as it stands (per limb at least 1). */
  const bool eights = ma.max_grid <= 0;
  if constexpr(NC == 1) return launch_plain_loop<G, KModUpMul<A, 1>, modup_mul_kernel<A, LOGN, KSH>>(kr, nl, ma.batch, ma.num_cus, ma.max_grid, eights, ma.stream);
  else return launch_plain_loop<G, KModUpMul<A, 2>, modup_mul2_kernel<A, LOGN, KSH>>(kr, nl, ma.batch, ma.num_cus, ma.max_grid, eights, ma.stream);
}

#define NTT_DEFINE_LAUNCH_MODUP_MUL(A, KSH, NC)                                       \
  template <> hipError_t launch_modup_mul<A, KSH, NC>(const ModUpMulArgs &ma)         \
  {                                                                                   \
    return with_int<6, 14>((int)ma.logn, hipErrorNotSupported, [&](auto ln) { return launch_modup_mul_n<A, decltype(ln)::value, KSH, NC>(ma); }); \
  }

} // namespace ntt
