/*
 * ntt_kernels_modup_mul2.h -- modup_mul2_kernel: one digit's term of BOTH components of a key switch,
 *   c0^ (+)= fwd(ModUp(digit)) (.) key0^,   c1^ (+)= fwd(ModUp(digit)) (.) key1^,
 * for a run of limbs of the extended basis in ONE launch.  Included by the modup_mul2_f64*.hip units only (the host layer sees the
 * launchers of ntt_keyswitch.h).
 *
 * modup_mul_kernel's skeleton (ntt_kernels_modup_mul.h): the prologue (a digit limb of the run as it stands, Barrett of the word for
 * count = 1, the half-tile 128-bit conversion with [b^_i]_{q_l} in LDS otherwise) and the forward block stages are those, unchanged.
 * The quarter-tile epilogue runs once per component with x[] live across the two passes: key_j^ (and c_j^ when accumulating) read in
 * the last group's layout, the product, c_j^ stored -- the register set of one quarter-tile product, not of two (fwd_mul_kernel's
 * note: two products at a time do not fit).  Per limb-polynomial 8N count bytes of the digit, 16N of the keys (from the L2 when
 * they are broadcast) and 16N (32N accumulating) of c0^, c1^; one conversion and one set of forward stages serve both products.
 * With every limb of the run marked as the digit's own (own = all ones) the prologue is the plain load of the operand and the kernel
 * is the pair form of the forward-multiply, c_j^ (+)= fwd(a) (.) b_j^.
 * Component 0 is stored before component 1's key is read: c0^ may coincide with key0^ as in fwd_mul_kernel, and the host layer
 * refuses c0^ against key1^ (and c1^ against key0^).
 */
#pragma once
#include <hip/hip_runtime.h>

/* the block kernels' pieces (see ntt_kernels_keyswitch.h on why not all of ntt_kernels.h) */
#include "ntt_core.h"
#include "ntt_passplan.h"
#include "ntt_kernels_block.h"
#include "ntt_keyswitch.h"

namespace ntt {

template <class A> struct KModUpMul2 {
  KArgs<A>        k;             /* k.a = the run's first limb of the extended operand (a digit limb of the run is read there) */
  const uint64_t *dig;           /* the digit's first limb, coefficients; digit limb i at dig + i * k.limb_stride */
  const uint64_t *b[2];          /* key0^, key1^, the run's first limb */
  uint64_t *      out[2];        /* c0^, c1^, the run's first limb (k.limb_stride / k.poly_stride, as the extended operand) */
  uint64_t        b_limb_stride; /* words between consecutive limbs of either key^ */
  uint32_t        lazy_in, b_bcast, accumulate; /* as KMul's */
  uint32_t        own;           /* bit l: limb l of the run is one of the digit's own limbs */
  int             count;
  BconvSrc        sl[kBconvLimbs];
  BconvDst        dl[kBconvLimbs];
};

template <class A, int LOGN, int KSH>
__global__ void __launch_bounds__((Geom<LOGN, false, flavor_of<A>()>::WG), (Geom<LOGN, false, flavor_of<A>()>::WPS))
  modup_mul2_kernel(const KModUpMul2<A> kr)
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
  if(!own && count > 1) {
    if(tid < (uint32_t)count) {
      /* prod_{k != i} b_k mod q_l: g < q_l and b_k < 2^61, each product below 2^122 (bconv_reduce takes any 128-bit word) */
      uint64_t g = 1;
      for(int k = 0; k < count; k++) {
        if(k == (int)tid) continue;
        const uint64_t bk = kr.sl[k].p;
        g                 = bconv_reduce(mulhi64(g, bk), g * bk, dl);
        g                 = g >= dl.q ? g - dl.q : g;
      }
      ghat[tid] = g;
    }
  }
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
        /* half a tile at a time: the 128-bit sums of 8 words stay in registers beside nothing else (x is not live yet) */
        static_for<0, 2>([&](auto hh) {
          constexpr int H = decltype(hh)::value;
          uint64_t      hi[kE / 2], lo[kE / 2];
          static_for<0, kE / 2>([&](auto ee) {
            hi[decltype(ee)::value] = 0;
            lo[decltype(ee)::value] = 0;
          });
          const uint64_t *dj = dblk;
          for(int j = 0; j < count; j++) {
            const BconvSrc s = kr.sl[j];
            const uint64_t g = ghat[j];
            static_for<0, kE / 2>([&](auto ee) {
              constexpr int   E   = decltype(ee)::value;
              const uint64_t *row = dj + ((uint32_t)(H * kE / 2 + E) << P::LT);
              bconv_mac(hi[E], lo[E], bconv_digit(stream_load(coef_at(row, tg)), s), g);
            });
            dj += kr.k.limb_stride;
          }
          static_for<0, kE / 2>([&](auto ee) {
            constexpr int  E    = decltype(ee)::value;
            const uint64_t v    = bconv_reduce(hi[E], lo[E], dl);
            raw[H * kE / 2 + E] = v >= dl.q ? v - dl.q : v;
          });
        });
      }
      convert_inputs<A, false>(x, raw, false, p.c);
    }
    run_group<A, LOGN, 0, false, MASK, (G::TBL(0) > 0)>(x, tg, 0u, p, gtw);
    static_for<0, P::NG - 1>([&](auto gg) {
      constexpr int GI = decltype(gg)::value;
      exchange<A, LOGN, GI, GI + 1>(x, tg, lds);
      run_group<A, LOGN, GI + 1, false, MASK, (G::TBL(GI + 1) > 0)>(x, tg, 0u, p, gtw + G::TBL_OFF(GI + 1));
    });
    /* one component at a time, a quarter-tile at a time: x[] is the only state carried from one pass to the next */
    static_for<0, 2>([&](auto jj) {
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

template <class A, int LOGN, int KSH> hipError_t launch_modup_mul2_n(const ModUpMul2Args &ma)
{
  using G = Geom<LOGN, false, flavor_of<A>()>;
  if(ma.nlimbs < 1 || ma.nlimbs > kBconvLimbs || ma.nlimbs > kMaxLimbs || ma.count < 1 || ma.count > kBconvLimbs) return hipErrorInvalidValue;
  KModUpMul2<A>  kr{};
  const uint64_t nl = (uint64_t)ma.nlimbs;
  fill_kargs(kr.k, ma.a, ma.limbs, nl, ma.limb_stride, ma.poly_stride, ma.logn, 0, ma.batch);
  for(int l = 0; l < ma.nlimbs; l++) kr.dl[l] = ma.dl[l];
  for(int j = 0; j < ma.count; j++) kr.sl[j] = ma.sl[j];
  kr.dig           = ma.dig;
  kr.b[0]          = ma.b[0];
  kr.b[1]          = ma.b[1];
  kr.out[0]        = ma.out[0];
  kr.out[1]        = ma.out[1];
  kr.b_limb_stride = ma.b_limb_stride;
  kr.lazy_in       = ma.lazy_in ? 1u : 0u;
  kr.b_bcast       = ma.b_bcast ? 1u : 0u;
  kr.accumulate    = ma.accumulate ? 1u : 0u;
  kr.own           = ma.own;
  kr.count         = ma.count;
  /* modup_mul_kernel's grid */
  const uint64_t wgs = block_grid<G>(ma.batch, 0, nl, ma.num_cus, ma.max_grid, G::PERSISTENT ? 1 : 4, ma.max_grid <= 0);
  if(ma.batch == 0) return hipSuccess;
  kr.k.wgs_per_limb = (uint32_t)wgs;
  hipLaunchKernelGGL((modup_mul2_kernel<A, LOGN, KSH>), dim3((unsigned)wgs, (unsigned)nl), dim3(G::WG), 0, ma.stream, kr);
  return hipGetLastError();
}

template <class A, int KSH> hipError_t launch_modup_mul2_impl(const ModUpMul2Args &ma)
{
  switch(ma.logn) {
#define NTT_MODUP_MUL2_CASE(LN) \
  case LN: return launch_modup_mul2_n<A, LN, KSH>(ma);
    NTT_MODUP_MUL2_CASE(6) NTT_MODUP_MUL2_CASE(7) NTT_MODUP_MUL2_CASE(8) NTT_MODUP_MUL2_CASE(9) NTT_MODUP_MUL2_CASE(10) NTT_MODUP_MUL2_CASE(11)
    NTT_MODUP_MUL2_CASE(12) NTT_MODUP_MUL2_CASE(13) NTT_MODUP_MUL2_CASE(14)
#undef NTT_MODUP_MUL2_CASE
    default: return hipErrorNotSupported;
  }
}

#define NTT_DEFINE_LAUNCH_MODUP_MUL2(A, KSH) \
  template <> hipError_t launch_modup_mul2<A, KSH>(const ModUpMul2Args &ma) { return launch_modup_mul2_impl<A, KSH>(ma); }

} // namespace ntt
