/*
 * ntt_kernels_bconv.h -- what the block kernels that reduce raw words in front of the forward block stages have in common
 * (modup_mul_kernel / modup_mul2_kernel, the four kernels of moddown_fwd_body, rescale_fwd_kernel): the [b^_i]_q table, the half-tile 128-bit
 * base conversion and the forward stage chain.  Included by ntt_kernels_modup_mul.h, ntt_kernels_moddown.h and
 * ntt_kernels_rescale.h, after the block kernels' pieces.
 *
 * Every piece is inlined into its caller and adds NO workgroup barrier (the stage chain has the exchanges' own, nothing else): where
 * the tables are published and what else that barrier covers differs from kernel to kernel and stays with the kernel.
 */
#pragma once
#include "ntt_keyswitch.h"

namespace ntt {

/* ghat[tid] = [b^_tid]_q = prod_{k != tid} src[k].p mod d.q for tid < n, formed once per workgroup (its limb is the grid's y index):
 * a 16 x 16 table has no room in the kernel arguments.  g < q and p_k < 2^61, each product below 2^122 (bconv_reduce takes any
 * 128-bit word).  The caller publishes ghat with a barrier of its own. */
__device__ __forceinline__ void bconv_ghat(uint64_t *ghat, const BconvSrc *src, int n, const BconvDst &d, uint32_t tid)
{
  if(tid < (uint32_t)n) {
    uint64_t g = 1;
    for(int k = 0; k < n; k++) {
      if(k == (int)tid) continue;
      const uint64_t pk = src[k].p;
      g                 = bconv_reduce(mulhi64(g, pk), g * pk, d);
      g                 = g >= d.q ? g - d.q : g;
    }
    ghat[tid] = g;
  }
}

/* raw[e] = fin(hi, lo) of the 128-bit sum over the n source limbs of bconv_digit(word, src[j]) * ghat[j], for the thread's 16 words
 * of a block in the first group's layout (slot e <-> index (e << LT) + tg); source limb j's block at blk + j * limb_stride.  Half a
 * tile at a time: the 128-bit sums of 8 words stay in registers beside nothing else (x is not live yet). */
template <int LT, class F>
__device__ __forceinline__ void bconv_tile(uint64_t (&raw)[kE], const uint64_t *blk, uint64_t limb_stride, const BconvSrc *src, const uint64_t *ghat,
                                           int n, uint32_t tg, F &&fin)
{
  static_for<0, 2>([&](auto hh) {
    constexpr int H = decltype(hh)::value;
    uint64_t      hi[kE / 2], lo[kE / 2];
    static_for<0, kE / 2>([&](auto ee) {
      hi[decltype(ee)::value] = 0;
      lo[decltype(ee)::value] = 0;
    });
    const uint64_t *bj = blk;
    for(int j = 0; j < n; j++) {
      const BconvSrc s = src[j];
      const uint64_t g = ghat[j];
      static_for<0, kE / 2>([&](auto ee) {
        constexpr int   E   = decltype(ee)::value;
        const uint64_t *row = bj + ((uint32_t)(H * kE / 2 + E) << LT);
        bconv_mac(hi[E], lo[E], bconv_digit(stream_load(coef_at(row, tg)), s), g);
      });
      bj += limb_stride;
    }
    static_for<0, kE / 2>([&](auto ee) {
      constexpr int E     = decltype(ee)::value;
      raw[H * kE / 2 + E] = fin(hi[E], lo[E]);
    });
  });
}

/* the forward block stages of a whole polynomial (block 0 of its transform), x in the first group's layout on entry and in the
 * last group's on return: fwd_mul_kernel's plain loop, the LDS twiddle tables behind gtw */
template <class A, int LOGN, uint32_t MASK>
__device__ __forceinline__ void fwd_block_stages(typename A::val (&x)[kE], uint32_t tg, const Params<A> &p, typename A::val *lds, lds_ctw_ptr<A> gtw)
{
  using P = Plan<LOGN>;
  using G = Geom<LOGN, false, flavor_of<A>()>;
  run_group<A, LOGN, 0, false, MASK, (G::TBL(0) > 0)>(x, tg, 0u, p, gtw);
  static_for<0, P::NG - 1>([&](auto gg) {
    constexpr int GI = decltype(gg)::value;
    exchange<A, LOGN, GI, GI + 1>(x, tg, lds);
    run_group<A, LOGN, GI + 1, false, MASK, (G::TBL(GI + 1) > 0)>(x, tg, 0u, p, gtw + G::TBL_OFF(GI + 1));
  });
}

} // namespace ntt
