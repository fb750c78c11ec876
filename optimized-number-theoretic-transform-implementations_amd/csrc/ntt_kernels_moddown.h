/*
 * ntt_kernels_moddown.h -- moddown_fwd_body: the ONE body of the four kernels that fuse an NTT-domain RNS ModDown with the forward
 * transform, and the one launcher of the four.  Included by ntt_kernels_keyswitch.h, ntt_kernels_ksfold.h, ntt_kernels_bgv.h and
 * ntt_kernels_exact.h, each of which keeps its kernel's name, launch bounds and argument record and states its variant's arithmetic.
 *
 * rescale_fwd_kernel's structure (ntt_kernels_rescale.h) with the prologue changed.  Per block of Q limb l (FP64 policies,
 * N = 2^6..2^14, one block = one polynomial):
 *   tables    [p^_j]_{q_l} = prod_{k != j} p_k mod q_l, formed once per workgroup (its limb is the grid's y index) into LDS: no table
 *             of np x nq words has room beside the run's limb records in the kernel arguments;
 *   prologue  the np P limbs' blocks (already inverse-transformed) as raw words -- up to 2^61, not exact in a double -- are reduced
 *             in integer arithmetic to the subtrahend u_l, then converted;
 *   stages    the forward block stages, unchanged;
 *   epilogue  a quarter-tile at a time: c^ read in the last group's layout, (c^ - x) * P^-1 with the limb's FP64 constants, stored.
 * The variants differ at four points, all decided at compile time (no kernel has a run-time flag the others lack):
 *                     tables                      prologue                                   result               extra factor
 *   kModDownInPlace   np > 1                      np = 1: moddown_digit1; bconv_tile         in place             --
 *   kModDownFold      np > 1                      the same                                   `out`, (+)= addend   --
 *   kModDownBgv       np > 1, times [T]_{q_l}     np = 1: bgv_digit1; bconv_tile             `out`, (+)= addend   --
 *   kModDownExact     always                      bconv_tile_exact                           in place             c^ [m]_{q_l}
 */
#pragma once
#include <hip/hip_runtime.h>

/* the block kernels' pieces (Geom, KArgs, limb_params, the stage groups and exchanges) -- not all of ntt_kernels.h, whose launch
 * section defines a kernel of its own (team_ctl_clear_kernel) in every unit that includes it */
#include "ntt_core.h"
#include "ntt_passplan.h"
#include "ntt_kernels_block.h"
#include "ntt_kernels_bconv.h"
#include "ntt_ct_mul.h"
#include "ntt_bgv.h"
#include "ntt_exact.h"

namespace ntt {

enum ModDownVariant { kModDownInPlace, kModDownFold, kModDownBgv, kModDownExact };

/* bconv_tile with s = sum_j fl(z_j) rho[j] (left to right from 0.0, which adds exactly) beside every 128-bit sum: raw[e] = fin(hi, lo, s).
 * A QUARTER of the tile at a time, not bconv_tile's half: the four FP64 sums and the conversions' temporaries beside eight 128-bit sums
 * do not fit the 128 registers of the instances that run four waves per SIMD (they spilled 5-15 registers at N = 2^7..2^9, 2^12, 2^13). */
template <int LT, class F>
__device__ __forceinline__ void bconv_tile_exact(uint64_t (&raw)[kE], const uint64_t *blk, uint64_t limb_stride, const BconvSrc *src, const double *rho,
                                                 const uint64_t *ghat, int n, uint32_t tg, F &&fin)
{
  constexpr int W = kE / 4;
  static_for<0, 4>([&](auto hh) {
    constexpr int H = decltype(hh)::value;
    uint64_t      hi[W], lo[W];
    double        s[W];
    sched_fence(); /* (one quarter's reductions are not interleaved with the next quarter's loads) */
    static_for<0, W>([&](auto ee) {
      hi[decltype(ee)::value] = 0;
      lo[decltype(ee)::value] = 0;
      s[decltype(ee)::value]  = 0.0;
    });
    const uint64_t *bj = blk;
    for(int j = 0; j < n; j++) {
      const BconvSrc sj = src[j];
      const double   rj = rho[j];
      const uint64_t g  = ghat[j];
      static_for<0, W>([&](auto ee) {
        constexpr int   E   = decltype(ee)::value;
        const uint64_t *row = bj + ((uint32_t)(H * W + E) << LT);
        const uint64_t  z   = bconv_digit(stream_load(coef_at(row, tg)), sj);
        s[E]                = s[E] + exact_term(z, rj);
        bconv_mac(hi[E], lo[E], z, g);
      });
      bj += limb_stride;
    }
    static_for<0, W>([&](auto ee) {
      constexpr int E = decltype(ee)::value;
      raw[H * W + E]  = fin(hi[E], lo[E], s[E]);
    });
  });
}

/* K is the variant's argument record: KModDown, KKsFold, KModDownBgv or KModDownExactFwd.  All have k, t, np, pl and ql; the fold
 * variants add out, its strides and accumulate, BGV ts, the exact variant rho and mq. */
template <class A, int LOGN, int KSH, ModDownVariant V, class K> __device__ __forceinline__ void moddown_fwd_body(const K &kr)
{
  static_assert(A::kCompact, "built for the FP64 policies");
  static_assert(sizeof(K) <= 3840, "the argument record must stay below 4 KB");
  constexpr bool FOLD  = V == kModDownFold || V == kModDownBgv;
  constexpr bool BGV   = V == kModDownBgv;
  constexpr bool EXACT = V == kModDownExact;
  uint32_t        bid, gdim, limb;
  const Params<A> p = limb_params<A, false, true>(kr.k, bid, gdim, limb);
  using P = Plan<LOGN>;
  using G = Geom<LOGN, false, flavor_of<A>()>;
  constexpr uint32_t MASK   = fused_mask<A, LOGN, false, KSH>();
  constexpr int      LDS_TW = G::LDS_TW;
  __shared__ typename A::val lds_all[G::BPW * P::LDS_ELEMS + LDS_TW];
  __shared__ uint64_t        ghat[kBconvLimbs]; /* [p^_j]_{q_l}; BGV: [T p^_j]_{q_l} */
  const uint32_t    tid = threadIdx.x;
  const uint32_t    sub = tid >> P::LT;
  const uint32_t    t   = tid & (P::T - 1);
  typename A::val * lds = lds_all + sub * P::LDS_ELEMS;
  BgvScale          ts{};
  if constexpr(BGV) ts = kr.ts[limb];
  const int np  = kr.np;
  bool      acc = false;
  if constexpr(FOLD) acc = kr.accumulate != 0;
  const BconvDst ql  = kr.ql[limb];
  uint64_t *     out = nullptr;
  if constexpr(FOLD) out = kr.out + (uint64_t)limb * kr.out_limb_stride;
  const lds_ctw_ptr<A> gtw = (lds_ctw_ptr<A>)reinterpret_cast<typename A::ctw *>(lds_all + G::BPW * P::LDS_ELEMS);
  if constexpr(LDS_TW > 0) fill_lds_tables<A, LOGN, false>(reinterpret_cast<typename A::ctw *>(lds_all + G::BPW * P::LDS_ELEMS), p, 0u, tid);
  /* (every condition of a barrier is uniform over the workgroup: np is a kernel argument) */
  if constexpr(EXACT) {
    bconv_ghat(ghat, kr.pl, np, ql, tid); /* one P prime takes the general path too ([p^_0]_q = 1) */
    __syncthreads();
  } else {
    if(np > 1) {
      bconv_ghat(ghat, kr.pl, np, ql, tid);
      /* [T]_{q_l} sits in the table and not in a per-word product in front of convert_inputs, nor in a second FP64 constant of the
       * epilogue: the words are the same (canonical residues throughout), the table costs np products per workgroup instead of N, and
       * the kernel keeps ksfold_fwd_kernel's registers */
      if constexpr(BGV) {
        if(tid < (uint32_t)np) ghat[tid] = bgv_scale(ghat[tid], ts, ql.q); /* (the entry this thread has just written) */
      }
    }
    if constexpr(LDS_TW > 0) __syncthreads();
    else if(np > 1) __syncthreads();
  }
  /* P^-1 mod q_l as a balanced double, |.| <= q/2 (a multiplier of every product of this workgroup) */
  const double sb = A::reduce(A::u64_to_f64_lt52(ql.s), p.c);
  for(uint64_t b0 = (uint64_t)bid * G::BPW; b0 < p.nblocks; b0 += (uint64_t)gdim * G::BPW) {
    uint64_t   b    = b0 + sub;
    const bool live = b < p.nblocks;
    if(!live) b = p.nblocks - 1;
    const uint64_t  off  = blk_off<LOGN>(p, b); /* (whole polynomials: s0 = 0) */
    const uint64_t *tblk = kr.t + off;
    uint64_t *      ablk = p.a + off; /* c^: the accumulator's Q limb */
    uint64_t *      cblk = ablk;      /* the destination: c^ itself, or the ciphertext with its own strides */
    if constexpr(FOLD) cblk = out + block_offset<LOGN>(b, 0u, kr.out_poly_stride);
    uint32_t tg = t; /* (an opaque copy per block, as fwd_mul_kernel's plain loop) */
    asm volatile("" : "+v"(tg));
    typename A::val x[kE];
    {
      uint64_t raw[kE];
      if constexpr(EXACT) {
        bconv_tile_exact<P::LT>(raw, tblk, kr.k.limb_stride, kr.pl, kr.rho, ghat, np, tg,
                                [&](uint64_t hi, uint64_t lo, double s) { return exact_bconv_finish(hi, lo, exact_round(s), ql); });
      } else {
        if(np == 1) { /* the rescale's prologue: no table, no 128-bit sum */
          const BconvSrc s0 = kr.pl[0];
          static_for<0, kE>([&](auto ee) {
            constexpr int   E   = decltype(ee)::value;
            const uint64_t *row = tblk + ((uint32_t)E << P::LT);
            const uint64_t  w   = stream_load(coef_at(row, tg));
            if constexpr(BGV) raw[E] = bgv_digit1(w, s0, ql, ts);
            else raw[E] = moddown_digit1(w, s0, ql);
          });
        } else {
          bconv_tile<P::LT>(raw, tblk, kr.k.limb_stride, kr.pl, ghat, np, tg, [&](uint64_t hi, uint64_t lo) { return moddown_digit(hi, lo, ql); });
        }
      }
      convert_inputs<A, false>(x, raw, false, p.c);
    }
    fwd_block_stages<A, LOGN, MASK>(x, tg, p, lds, gtw);
    /* m mod q_l as sb, but formed here from the scalar word: held across the stages it is the register that spills at N = 2^9 and 2^13 */
    double mb = 0.0;
    if constexpr(EXACT) {
      uint64_t mq = kr.mq[limb];
      asm volatile("" : "+s"(mq));
      mb = A::reduce(A::u64_to_f64_lt52(mq), p.c);
    }
    /* every thread reads the four words of a quarter-tile before it stores those same four, and no other thread touches them: the
     * destination may be the accumulator's own Q limbs (the in-place variants, and BGV's in-place form through `out`) */
    static_for<0, 4>([&](auto qq) {
      constexpr int Q = decltype(qq)::value;
      uint64_t      rc[kE], re[kE], u[kE];
      sched_fence();
      load_last_raw<LOGN, 4 * Q, 4 * Q + 4>(rc, tg, ablk);
      if constexpr(FOLD) {
        if(acc) load_last_raw<LOGN, 4 * Q, 4 * Q + 4>(re, tg, cblk);
      }
      static_for<4 * Q, 4 * Q + 4>([&](auto ee) {
        constexpr int E = decltype(ee)::value;
        double        d;
        if constexpr(EXACT) {
          const double cm = A::mulmod_c(mb, A::reduce(A::u64_to_f64_lt52(rc[E]), p.c), p.c); /* |c^ m mod q| <= q */
          d               = A::reduce(cm - A::reduce(x[E], p.c), p.c);                      /* |.| <= 1.5 q before */
        } else {
          d = A::reduce(A::u64_to_f64_lt52(rc[E]) - A::reduce(x[E], p.c), p.c); /* |c^ - x| < 1.5 q before */
        }
        const uint64_t r = A::mul_store(A::mulmod_c(sb, d, p.c), p.c);
        if constexpr(FOLD) {
          const uint64_t v = r + (acc ? re[E] : 0); /* canonical + canonical: below 2q */
          u[E]             = v >= ql.q ? v - ql.q : v;
        } else {
          u[E] = r;
        }
      });
      if(live) store_last_raw<LOGN, 4 * Q, 4 * Q + 4>(u, tg, cblk);
      sched_fence();
    });
  }
}

/* The launcher of the four: the argument check, the common fields of the record K, `extra(kr)` for the variant's own, the launch of
 * Kernel over the plain loop's grid. */
template <class A, int LOGN, class K, void (&Kernel)(const K), class F> hipError_t launch_moddown_variant_n(const ModDownFwdArgs &ma, F &&extra)
{
  using G = Geom<LOGN, false, flavor_of<A>()>;
  if(ma.nlimbs < 1 || ma.nlimbs > kBconvLimbs || ma.nlimbs > kMaxLimbs || ma.np < 1 || ma.np > kBconvLimbs) return hipErrorInvalidValue;
  K              kr{};
  const uint64_t nl = (uint64_t)ma.nlimbs;
  fill_kargs(kr.k, ma.c, ma.limbs, nl, ma.limb_stride, ma.poly_stride, ma.logn, 0, ma.batch);
  for(int l = 0; l < ma.nlimbs; l++) kr.ql[l] = ma.ql[l];
  for(int j = 0; j < ma.np; j++) kr.pl[j] = ma.pl[j];
  kr.t  = ma.t;
  kr.np = ma.np;
  extra(kr);
  return launch_plain_loop<G, K, Kernel>(kr, nl, ma.batch, ma.num_cus, ma.max_grid, true, ma.stream);
}

/* the fold variants' destination (poly_stride 0 = dense: N) */
template <class K> inline void moddown_fold_out(K &kr, const KsFoldArgs &ka)
{
  kr.out             = ka.out;
  kr.out_limb_stride = ka.out_limb_stride;
  kr.out_poly_stride = ka.out_poly_stride ? ka.out_poly_stride : (1ull << ka.m.logn);
  kr.accumulate      = ka.accumulate ? 1 : 0;
}

} // namespace ntt
