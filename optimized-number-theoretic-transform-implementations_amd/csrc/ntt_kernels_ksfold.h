/*
 * ntt_kernels_ksfold.h -- ksfold_fwd_kernel: the NTT-domain RNS ModDown of an accumulator over Q u P WRITTEN INTO (or added to) a
 * ciphertext over Q, for a run of Q limbs in ONE launch: the last step of a relinearisation ((d0, d1) += ModDown(acc0, acc1)) and of a
 * rotation (c1' = ModDown(acc1)).  Included by the ksfold_f64*.hip units only (the host layer sees the launchers of ntt_ct_mul.h).
 *
 * The prologue and the stages are those of the in-place ModDown kernel (ntt_kernels_keyswitch.h); the epilogue differs.  Per block of
 * Q limb l (FP64 policies, N = 2^6..2^14, one block = one polynomial):
 *   prologue  the np P limbs' blocks (already inverse-transformed) as raw words are reduced in integer arithmetic to
 *             u_l = FastBConv_{P->q_l}([t + h]_P) - [h]_{q_l} (ntt_keyswitch.h), then converted;
 *   stages    the forward block stages, unchanged;
 *   epilogue  a quarter-tile at a time: c^ read from the ACCUMULATOR in the last group's layout, r = (c^ - x) * P^-1 with the limb's
 *             FP64 constants, canonical after mul_store; when accumulating, the ciphertext's word e is read beside it and r + e gets one
 *             conditional subtraction in integer arithmetic (both canonical: r + e < 2q < 2^53, exact); the result is stored to the
 *             CIPHERTEXT, whose limb and polynomial strides are its own.  The accumulator's Q limbs are not written.
 * 8N np bytes of t, 8N of c^, 8N stored and, when accumulating, 8N of the addend per limb-polynomial.
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

namespace ntt {

template <class A> struct KKsFold {
  KArgs<A>        k;  /* k.a = the run's first Q limb of the accumulator (c^, read only), its strides, the run's limb records */
  const uint64_t *t;  /* the first P limb's coefficients; P limb j at t + j * k.limb_stride */
  uint64_t *      out; /* the run's first limb of the ciphertext */
  uint64_t        out_limb_stride, out_poly_stride;
  int             np, accumulate;
  BconvSrc        pl[kBconvLimbs];
  BconvDst        ql[kBconvLimbs];
};

template <class A, int LOGN, int KSH>
__global__ void __launch_bounds__((Geom<LOGN, false, flavor_of<A>()>::WG), (Geom<LOGN, false, flavor_of<A>()>::WPS))
  ksfold_fwd_kernel(const KKsFold<A> kr)
{
  static_assert(A::kCompact, "built for the FP64 policies");
  uint32_t        bid, gdim, limb;
  const Params<A> p = limb_params<A, false, true>(kr.k, bid, gdim, limb);
  using P = Plan<LOGN>;
  using G = Geom<LOGN, false, flavor_of<A>()>;
  constexpr uint32_t MASK   = fused_mask<A, LOGN, false, KSH>();
  constexpr int      LDS_TW = G::LDS_TW;
  __shared__ typename A::val lds_all[G::BPW * P::LDS_ELEMS + LDS_TW];
  __shared__ uint64_t        ghat[kBconvLimbs]; /* [p^_j]_{q_l} */
  const uint32_t       tid = threadIdx.x;
  const uint32_t       sub = tid >> P::LT;
  const uint32_t       t   = tid & (P::T - 1);
  typename A::val *    lds = lds_all + sub * P::LDS_ELEMS;
  const BconvDst       ql  = kr.ql[limb];
  const int            np  = kr.np;
  const bool           acc = kr.accumulate != 0;
  uint64_t *const      out = kr.out + (uint64_t)limb * kr.out_limb_stride;
  const lds_ctw_ptr<A> gtw = (lds_ctw_ptr<A>)reinterpret_cast<typename A::ctw *>(lds_all + G::BPW * P::LDS_ELEMS);
  if constexpr(LDS_TW > 0) fill_lds_tables<A, LOGN, false>(reinterpret_cast<typename A::ctw *>(lds_all + G::BPW * P::LDS_ELEMS), p, 0u, tid);
  if(np > 1) bconv_ghat(ghat, kr.pl, np, ql, tid);
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
          raw[E]              = moddown_digit1(stream_load(coef_at(row, tg)), s0, ql);
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

template <class A, int LOGN, int KSH> hipError_t launch_ksfold_fwd_n(const KsFoldArgs &ka)
{
  using G                  = Geom<LOGN, false, flavor_of<A>()>;
  const ModDownFwdArgs &ma = ka.m;
  if(ma.nlimbs < 1 || ma.nlimbs > kBconvLimbs || ma.nlimbs > kMaxLimbs || ma.np < 1 || ma.np > kBconvLimbs) return hipErrorInvalidValue;
  KKsFold<A>     kr{};
  const uint64_t nl = (uint64_t)ma.nlimbs;
  fill_kargs(kr.k, ma.c, ma.limbs, nl, ma.limb_stride, ma.poly_stride, ma.logn, 0, ma.batch);
  for(int l = 0; l < ma.nlimbs; l++) kr.ql[l] = ma.ql[l];
  for(int j = 0; j < ma.np; j++) kr.pl[j] = ma.pl[j];
  kr.t               = ma.t;
  kr.np              = ma.np;
  kr.out             = ka.out;
  kr.out_limb_stride = ka.out_limb_stride;
  kr.out_poly_stride = ka.out_poly_stride ? ka.out_poly_stride : (1ull << ma.logn);
  kr.accumulate      = ka.accumulate ? 1 : 0;
  /* the in-place ModDown kernel's grid: the plain loop of the forward block kernel, the x extent a multiple of 8 */
  const uint64_t wgs = block_grid<G>(ma.batch, 0, nl, ma.num_cus, ma.max_grid, G::PERSISTENT ? 1 : 4, true);
  if(ma.batch == 0) return hipSuccess;
  kr.k.wgs_per_limb = (uint32_t)wgs;
  hipLaunchKernelGGL((ksfold_fwd_kernel<A, LOGN, KSH>), dim3((unsigned)wgs, (unsigned)nl), dim3(G::WG), 0, ma.stream, kr);
  return hipGetLastError();
}

#define NTT_DEFINE_LAUNCH_KSFOLD_FWD(A, KSH)                                                                                                  \
  template <> hipError_t launch_ksfold_fwd<A, KSH>(const KsFoldArgs &ka)                                                                      \
  {                                                                                                                                           \
    return with_int<6, 14>((int)ka.m.logn, hipErrorNotSupported, [&](auto ln) { return launch_ksfold_fwd_n<A, decltype(ln)::value, KSH>(ka); }); \
  }

} // namespace ntt
