/*
 * ntt_kernels_modup_mul.h -- modup_mul_kernel: one digit's term of the key-switching inner product, c^ (+)= fwd(ModUp(digit)) (.) key^,
 * for a run of limbs of the extended basis in ONE launch.  Included by the modup_mul_f64*.hip units only (the host layer sees the
 * launchers of ntt_keyswitch.h).
 *
 * moddown_fwd_kernel's skeleton (ntt_kernels_keyswitch.h) with fwd_mul_kernel's plain-loop epilogue (ntt_kernels_products.h).  Per
 * block of limb l (FP64 policies, N = 2^6..2^14, one block = one polynomial):
 *   prologue  l is one of the digit's own limbs (a bit of the kernel arguments, workgroup-uniform): its block as it stands.
 *             Otherwise the digit's count blocks as raw words -- up to 2^61, not exact in a double -- are converted in integer
 *             arithmetic: FastBConv_{B->q_l} (ntt_keyswitch.h), canonical, word for word what bconv_kernel would have written into
 *             the operand's slot l; with count = 1 Barrett of the word itself.  Then converted;
 *   stages    the forward block stages, unchanged;
 *   epilogue  a quarter-tile at a time: key^ (and c^ when accumulating) read in the last group's layout, the product, c^ stored.
 * 8N count bytes of the digit, 8N of the key (from the L2 when it is broadcast) and 8N (16N accumulating) of c^ per limb-polynomial;
 * the extended digit never exists in memory.  [b^_i]_{q_l} = prod_{k != i} b_k mod q_l is formed once per workgroup (its limb is the
 * grid's y index) into LDS, as moddown_fwd_kernel forms its [p^_j]_{q_l}: a 16 x 16 table has no room in the kernel arguments.
 */
#pragma once
#include <hip/hip_runtime.h>

/* the block kernels' pieces (see ntt_kernels_keyswitch.h on why not all of ntt_kernels.h) */
#include "ntt_core.h"
#include "ntt_passplan.h"
#include "ntt_kernels_block.h"
#include "ntt_keyswitch.h"

namespace ntt {

template <class A> struct KModUpMul {
  KArgs<A>        k;             /* k.a = the run's first limb of the extended operand (a digit limb of the run is read there) */
  const uint64_t *dig;           /* the digit's first limb, coefficients; digit limb i at dig + i * k.limb_stride */
  const uint64_t *b;             /* key^, the run's first limb */
  uint64_t *      out;           /* c^, the run's first limb (k.limb_stride / k.poly_stride, as the extended operand) */
  uint64_t        b_limb_stride; /* words between consecutive limbs of key^ */
  uint32_t        lazy_in, b_bcast, accumulate; /* as KMul's */
  uint32_t        own;           /* bit l: limb l of the run is one of the digit's own limbs */
  int             count;
  BconvSrc        sl[kBconvLimbs];
  BconvDst        dl[kBconvLimbs];
};

template <class A, int LOGN, int KSH>
__global__ void __launch_bounds__((Geom<LOGN, false, flavor_of<A>()>::WG), (Geom<LOGN, false, flavor_of<A>()>::WPS))
  modup_mul_kernel(const KModUpMul<A> kr)
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
  const uint64_t *     bptr  = kr.b + (uint64_t)limb * kr.b_limb_stride;
  uint64_t *           cptr  = kr.out + (uint64_t)limb * kr.k.limb_stride;
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
    const uint64_t *bblk = bc ? bptr : bptr + off; /* a broadcast key^ is one dense polynomial per limb */
    uint64_t *      cblk = cptr + off;
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
    static_for<0, 4>([&](auto qq) {
      constexpr int Q = decltype(qq)::value;
      uint64_t      rb[kE], rc[kE], u[kE];
      sched_fence();
      load_last_raw<LOGN, 4 * Q, 4 * Q + 4>(rb, tg, bblk);
      /* (the accumulator words: c^ itself, or zeros when the call does not accumulate) */
      if(acc) load_last_raw<LOGN, 4 * Q, 4 * Q + 4>(rc, tg, cblk);
      else static_for<4 * Q, 4 * Q + 4>([&](auto ee) { rc[decltype(ee)::value] = 0; });
      mul_out_tile<A, 4 * Q, 4 * Q + 4, 1>(u, x, rb, rc, lazy, p.c);
      if(live) store_last_raw<LOGN, 4 * Q, 4 * Q + 4>(u, tg, cblk);
      sched_fence();
    });
  }
}

template <class A, int LOGN, int KSH> hipError_t launch_modup_mul_n(const ModUpMulArgs &ma)
{
  using G = Geom<LOGN, false, flavor_of<A>()>;
  if(ma.nlimbs < 1 || ma.nlimbs > kBconvLimbs || ma.nlimbs > kMaxLimbs || ma.count < 1 || ma.count > kBconvLimbs) return hipErrorInvalidValue;
  KModUpMul<A>   kr{};
  const uint64_t nl = (uint64_t)ma.nlimbs;
  fill_kargs(kr.k, ma.a, ma.limbs, nl, ma.limb_stride, ma.poly_stride, ma.logn, 0, ma.batch);
  for(int l = 0; l < ma.nlimbs; l++) kr.dl[l] = ma.dl[l];
  for(int j = 0; j < ma.count; j++) kr.sl[j] = ma.sl[j];
  kr.dig           = ma.dig;
  kr.b             = ma.b;
  kr.out           = ma.out;
  kr.b_limb_stride = ma.b_limb_stride;
  kr.lazy_in       = ma.lazy_in ? 1u : 0u;
  kr.b_bcast       = ma.b_bcast ? 1u : 0u;
  kr.accumulate    = ma.accumulate ? 1u : 0u;
  kr.own           = ma.own;
  kr.count         = ma.count;
  /* moddown_fwd_kernel's grid: the plain loop of the forward block kernel, the x extent a multiple of 8 so that the limb-blocks
   * reading one block of the digit share blockIdx % 8 (speed only).  NTT_OPT_MAX_GRID is taken as it stands (per limb at least 1). */
  const uint64_t wgs = block_grid<G>(ma.batch, 0, nl, ma.num_cus, ma.max_grid, G::PERSISTENT ? 1 : 4, ma.max_grid <= 0);
  if(ma.batch == 0) return hipSuccess;
  kr.k.wgs_per_limb = (uint32_t)wgs;
  hipLaunchKernelGGL((modup_mul_kernel<A, LOGN, KSH>), dim3((unsigned)wgs, (unsigned)nl), dim3(G::WG), 0, ma.stream, kr);
  return hipGetLastError();
}

template <class A, int KSH> hipError_t launch_modup_mul_impl(const ModUpMulArgs &ma)
{
  switch(ma.logn) {
#define NTT_MODUP_MUL_CASE(LN) \
  case LN: return launch_modup_mul_n<A, LN, KSH>(ma);
    NTT_MODUP_MUL_CASE(6) NTT_MODUP_MUL_CASE(7) NTT_MODUP_MUL_CASE(8) NTT_MODUP_MUL_CASE(9) NTT_MODUP_MUL_CASE(10) NTT_MODUP_MUL_CASE(11)
    NTT_MODUP_MUL_CASE(12) NTT_MODUP_MUL_CASE(13) NTT_MODUP_MUL_CASE(14)
#undef NTT_MODUP_MUL_CASE
    default: return hipErrorNotSupported;
  }
}

#define NTT_DEFINE_LAUNCH_MODUP_MUL(A, KSH) \
  template <> hipError_t launch_modup_mul<A, KSH>(const ModUpMulArgs &ma) { return launch_modup_mul_impl<A, KSH>(ma); }

} // namespace ntt
