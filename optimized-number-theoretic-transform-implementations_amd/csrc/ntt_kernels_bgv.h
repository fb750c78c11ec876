/*
 * ntt_kernels_bgv.h -- moddown_bgv_fwd_kernel: the NTT-domain BGV ModDown (ntt_rns_mod_down_bgv_batch in place,
 * ntt_rns_mod_down_bgv_add_batch into a ciphertext) for a run of Q limbs in ONE launch.  Included by the ksbgv_f64*.hip units only (the
 * host layer sees the launchers of ntt_bgv.h, which states the arithmetic).
 *
 * ksfold_fwd_kernel's structure (ntt_kernels_ksfold.h) with the prologue's constants changed.  Per block of Q limb l (FP64 policies,
 * N = 2^6..2^14, one block = one polynomial):
 *   tables    np > 1: bconv_ghat's [p^_j]_{q_l}, each entry multiplied by [T]_{q_l} by the thread that formed it (one Shoup product per
 *             P prime and workgroup); the offset arrives as [T h]_{q_l} from the host;
 *   prologue  the np P limbs' blocks (already inverse-transformed) as raw words are reduced in integer arithmetic to
 *             u_l = [T]_{q_l} (F_l - [h]_{q_l}) = [T F_l]_{q_l} - [T h]_{q_l}: bconv_tile over the scaled table and moddown_digit -- word for
 *             word ksfold_fwd_kernel's work; np = 1: bgv_digit1 (no table, no 128-bit sum; the source product stays, one more Shoup
 *             product per word for [T]_{q_l}); then converted;
 *   stages    the forward block stages, unchanged;
 *   epilogue  ksfold_fwd_kernel's: c^ read from the accumulator, (c^ - x) P^-1 with the limb's FP64 constants, the optional addend, the
 *             store to `out`.  The in-place form passes out = the accumulator's own Q limbs: every thread reads the four words of a
 *             quarter-tile before it stores those same four, and no other thread touches them.
 * [T]_{q_l} sits in the table and not in a per-word product in front of convert_inputs, nor in a second FP64 constant of the epilogue:
 * the words are the same (canonical residues throughout), the table costs np products per workgroup instead of N, and the kernel keeps
 * ksfold_fwd_kernel's registers.
 */
#pragma once
#include <hip/hip_runtime.h>

#include "ntt_core.h"
#include "ntt_passplan.h"
#include "ntt_kernels_block.h"
#include "ntt_kernels_bconv.h"
#include "ntt_bgv.h"

namespace ntt {

template <class A> struct KModDownBgv {
  KArgs<A>        k;   /* k.a = the run's first Q limb of the accumulator (c^), its strides, the run's limb records */
  const uint64_t *t;   /* the first P limb's coefficients; P limb j at t + j * k.limb_stride */
  uint64_t *      out; /* the run's first limb of the destination (the ciphertext, or the accumulator itself) */
  uint64_t        out_limb_stride, out_poly_stride;
  int             np, accumulate;
  BconvSrc        pl[kBconvLimbs]; /* h = [h T]_{p_j}, inv = [T^-1 p^_j^-1]_{p_j} */
  BconvDst        ql[kBconvLimbs]; /* s = [P^-1]_q, h = [T h]_q                  */
  BgvScale        ts[kBconvLimbs]; /* [T]_q                                       */
};

template <class A, int LOGN, int KSH>
__global__ void __launch_bounds__((Geom<LOGN, false, flavor_of<A>()>::WG), (Geom<LOGN, false, flavor_of<A>()>::WPS))
  moddown_bgv_fwd_kernel(const KModDownBgv<A> kr)
{
  static_assert(A::kCompact, "built for the FP64 policies");
  static_assert(sizeof(KModDownBgv<A>) <= 3840, "the argument record must stay below 4 KB");
  uint32_t        bid, gdim, limb;
  const Params<A> p = limb_params<A, false, true>(kr.k, bid, gdim, limb);
  using P = Plan<LOGN>;
  using G = Geom<LOGN, false, flavor_of<A>()>;
  constexpr uint32_t MASK   = fused_mask<A, LOGN, false, KSH>();
  constexpr int      LDS_TW = G::LDS_TW;
  __shared__ typename A::val lds_all[G::BPW * P::LDS_ELEMS + LDS_TW];
  __shared__ uint64_t        ghat[kBconvLimbs]; /* [T p^_j]_{q_l} */
  const uint32_t       tid = threadIdx.x;
  const uint32_t       sub = tid >> P::LT;
  const uint32_t       t   = tid & (P::T - 1);
  typename A::val *    lds = lds_all + sub * P::LDS_ELEMS;
  const BgvScale       ts  = kr.ts[limb];
  const int            np  = kr.np;
  const bool           acc = kr.accumulate != 0;
  const BconvDst       ql  = kr.ql[limb];
  uint64_t *const      out = kr.out + (uint64_t)limb * kr.out_limb_stride;
  const lds_ctw_ptr<A> gtw = (lds_ctw_ptr<A>)reinterpret_cast<typename A::ctw *>(lds_all + G::BPW * P::LDS_ELEMS);
  if constexpr(LDS_TW > 0) fill_lds_tables<A, LOGN, false>(reinterpret_cast<typename A::ctw *>(lds_all + G::BPW * P::LDS_ELEMS), p, 0u, tid);
  if(np > 1) {
    bconv_ghat(ghat, kr.pl, np, ql, tid);
    if(tid < (uint32_t)np) ghat[tid] = bgv_scale(ghat[tid], ts, ql.q); /* (the entry this thread has just written) */
  }
  if constexpr(LDS_TW > 0) __syncthreads();
  else if(np > 1) __syncthreads();
  /* P^-1 mod q_l as a balanced double, |.| <= q/2 (the multiplier of every product of this workgroup) */
  const double sb = A::reduce(A::u64_to_f64_lt52(ql.s), p.c);
  for(uint64_t b0 = (uint64_t)bid * G::BPW; b0 < p.nblocks; b0 += (uint64_t)gdim * G::BPW) {
    uint64_t   b    = b0 + sub;
    const bool live = b < p.nblocks;
    if(!live) b = p.nblocks - 1;
    const uint64_t  off  = blk_off<LOGN>(p, b); /* (whole polynomials: s0 = 0) */
    const uint64_t *tblk = kr.t + off;
    const uint64_t *ablk = p.a + off;
    uint64_t *      cblk = out + block_offset<LOGN>(b, 0u, kr.out_poly_stride);
    uint32_t        tg   = t; /* (an opaque copy per block, as fwd_mul_kernel's plain loop) */
    asm volatile("" : "+v"(tg));
    typename A::val x[kE];
    {
      uint64_t raw[kE];
      if(np == 1) {
        const BconvSrc s0 = kr.pl[0];
        static_for<0, kE>([&](auto ee) {
          constexpr int   E   = decltype(ee)::value;
          const uint64_t *row = tblk + ((uint32_t)E << P::LT);
          raw[E]              = bgv_digit1(stream_load(coef_at(row, tg)), s0, ql, ts);
        });
      } else {
        bconv_tile<P::LT>(raw, tblk, kr.k.limb_stride, kr.pl, ghat, np, tg, [&](uint64_t hi, uint64_t lo) { return moddown_digit(hi, lo, ql); });
      }
      convert_inputs<A, false>(x, raw, false, p.c);
    }
    fwd_block_stages<A, LOGN, MASK>(x, tg, p, lds, gtw);
    static_for<0, 4>([&](auto qq) {
      constexpr int Q = decltype(qq)::value;
      uint64_t      rc[kE], re[kE], u[kE];
      sched_fence();
      load_last_raw<LOGN, 4 * Q, 4 * Q + 4>(rc, tg, ablk);
      if(acc) load_last_raw<LOGN, 4 * Q, 4 * Q + 4>(re, tg, cblk);
      static_for<4 * Q, 4 * Q + 4>([&](auto ee) {
        constexpr int  E = decltype(ee)::value;
        const double   d = A::reduce(A::u64_to_f64_lt52(rc[E]) - A::reduce(x[E], p.c), p.c); /* |c^ - x| < 1.5 q before */
        const uint64_t r = A::mul_store(A::mulmod_c(sb, d, p.c), p.c);
        const uint64_t v = r + (acc ? re[E] : 0); /* canonical + canonical: below 2q */
        u[E]             = v >= ql.q ? v - ql.q : v;
      });
      if(live) store_last_raw<LOGN, 4 * Q, 4 * Q + 4>(u, tg, cblk);
      sched_fence();
    });
  }
}

template <class A, int LOGN, int KSH> hipError_t launch_moddown_bgv_fwd_n(const ModDownBgvArgs &ba)
{
  using G                  = Geom<LOGN, false, flavor_of<A>()>;
  const KsFoldArgs &    ka = ba.k;
  const ModDownFwdArgs &ma = ka.m;
  if(ma.nlimbs < 1 || ma.nlimbs > kBconvLimbs || ma.nlimbs > kMaxLimbs || ma.np < 1 || ma.np > kBconvLimbs) return hipErrorInvalidValue;
  KModDownBgv<A> kr{};
  const uint64_t nl = (uint64_t)ma.nlimbs;
  fill_kargs(kr.k, ma.c, ma.limbs, nl, ma.limb_stride, ma.poly_stride, ma.logn, 0, ma.batch);
  for(int l = 0; l < ma.nlimbs; l++) {
    kr.ql[l] = ma.ql[l];
    kr.ts[l] = ba.ts[l];
  }
  for(int j = 0; j < ma.np; j++) kr.pl[j] = ma.pl[j];
  kr.t               = ma.t;
  kr.np              = ma.np;
  kr.out             = ka.out;
  kr.out_limb_stride = ka.out_limb_stride;
  kr.out_poly_stride = ka.out_poly_stride ? ka.out_poly_stride : (1ull << ma.logn);
  kr.accumulate      = ka.accumulate ? 1 : 0;
  /* ksfold_fwd_kernel's grid: the plain loop of the forward block kernel, the x extent a multiple of 8 */
  const uint64_t wgs = block_grid<G>(ma.batch, 0, nl, ma.num_cus, ma.max_grid, G::PERSISTENT ? 1 : 4, true);
  if(ma.batch == 0) return hipSuccess;
  kr.k.wgs_per_limb = (uint32_t)wgs;
  hipLaunchKernelGGL((moddown_bgv_fwd_kernel<A, LOGN, KSH>), dim3((unsigned)wgs, (unsigned)nl), dim3(G::WG), 0, ma.stream, kr);
  return hipGetLastError();
}

#define NTT_DEFINE_LAUNCH_MODDOWN_BGV_FWD(A, KSH)                                                                                                  \
  template <> hipError_t launch_moddown_bgv_fwd<A, KSH>(const ModDownBgvArgs &ba)                                                                  \
  {                                                                                                                                                \
    return with_int<6, 14>((int)ba.k.m.logn, hipErrorNotSupported, [&](auto ln) { return launch_moddown_bgv_fwd_n<A, decltype(ln)::value, KSH>(ba); }); \
  }

} // namespace ntt
