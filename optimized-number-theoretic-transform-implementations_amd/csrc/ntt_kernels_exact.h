/*
 * ntt_kernels_exact.h -- moddown_exact_fwd_kernel: the NTT-domain EXACT scaled ModDown (ntt_rns_mod_down_exact_batch) for a run of Q
 * limbs in ONE launch.  Included by the ksexact_f64*.hip units only (the host layer sees the launchers of ntt_exact.h).
 *
 * moddown_fwd_kernel's structure (ntt_kernels_keyswitch.h) with two changes.  Per block of Q limb l (FP64 policies, N = 2^6..2^14, one
 * block = one polynomial):
 *   prologue  the np P limbs' blocks (already inverse-transformed) as raw words are reduced in integer arithmetic to
 *             u_l = ExactBConv_{P->q_l}([m t]_P): bconv_tile with the FP64 sum of fl(z_j) rho_j beside the 128-bit sum of every word
 *             (bconv_tile_exact), v = rint of it into the sum before the one Barrett reduction (ntt_exact.h), then converted;
 *   stages    the forward block stages, unchanged;
 *   epilogue  a quarter-tile at a time: c^ read in the last group's layout, (c^ [m]_q - x) * P^-1 with the limb's FP64 constants --
 *             c^ [m P^-1] - x [P^-1] with the common factor taken out, one product more than moddown_fwd_kernel.
 * 8N np bytes of t and 16N of c^ per limb-polynomial.  One P prime takes the general path ([p^_0]_q = 1).  v depends on the P words
 * alone and is formed by ntt_exact.h's operations in ntt_exact.h's order: every workgroup, whichever limb it serves, and the
 * coefficient kernel of the sandwich route arrive at the same v.
 */
#pragma once
#include <hip/hip_runtime.h>

#include "ntt_core.h"
#include "ntt_passplan.h"
#include "ntt_kernels_block.h"
#include "ntt_kernels_bconv.h"
#include "ntt_exact.h"

namespace ntt {

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

template <class A> struct KModDownExactFwd {
  KArgs<A>        k;  /* k.a = the run's first Q limb (c^), limb_stride / poly_stride of the operand, the run's limb records */
  const uint64_t *t;  /* the first P limb's coefficients; P limb j at t + j * k.limb_stride */
  int             np;
  BconvSrc        pl[kBconvLimbs];  /* inv = [m p^_j^-1]_{p_j}, h = 0 */
  BconvDst        ql[kBconvLimbs];  /* s = [P^-1]_q, h = q - [P]_q   */
  double          rho[kBconvLimbs]; /* 1.0 / (double)p_j              */
  uint64_t        mq[kBconvLimbs];  /* [m]_{q_l}                      */
};

template <class A, int LOGN, int KSH>
__global__ void __launch_bounds__((Geom<LOGN, false, flavor_of<A>()>::WG), (Geom<LOGN, false, flavor_of<A>()>::WPS))
  moddown_exact_fwd_kernel(const KModDownExactFwd<A> kr)
{
  static_assert(A::kCompact, "built for the FP64 policies");
  static_assert(sizeof(KModDownExactFwd<A>) <= 3840, "the argument record must stay below 4 KB");
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
  const lds_ctw_ptr<A> gtw = (lds_ctw_ptr<A>)reinterpret_cast<typename A::ctw *>(lds_all + G::BPW * P::LDS_ELEMS);
  if constexpr(LDS_TW > 0) fill_lds_tables<A, LOGN, false>(reinterpret_cast<typename A::ctw *>(lds_all + G::BPW * P::LDS_ELEMS), p, 0u, tid);
  bconv_ghat(ghat, kr.pl, np, ql, tid);
  __syncthreads();
  /* P^-1 mod q_l as a balanced double, |.| <= q/2 (a multiplier of every product of this workgroup) */
  const double sb = A::reduce(A::u64_to_f64_lt52(ql.s), p.c);
  for(uint64_t b0 = (uint64_t)bid * G::BPW; b0 < p.nblocks; b0 += (uint64_t)gdim * G::BPW) {
    uint64_t   b    = b0 + sub;
    const bool live = b < p.nblocks;
    if(!live) b = p.nblocks - 1;
    const uint64_t  off  = blk_off<LOGN>(p, b); /* (whole polynomials: s0 = 0) */
    const uint64_t *tblk = kr.t + off;
    uint64_t *      cblk = p.a + off;
    uint32_t        tg   = t; /* (an opaque copy per block, as fwd_mul_kernel's plain loop) */
    asm volatile("" : "+v"(tg));
    typename A::val x[kE];
    {
      uint64_t raw[kE];
      bconv_tile_exact<P::LT>(raw, tblk, kr.k.limb_stride, kr.pl, kr.rho, ghat, np, tg,
                              [&](uint64_t hi, uint64_t lo, double s) { return exact_bconv_finish(hi, lo, exact_round(s), ql); });
      convert_inputs<A, false>(x, raw, false, p.c);
    }
    fwd_block_stages<A, LOGN, MASK>(x, tg, p, lds, gtw);
    /* m mod q_l likewise, formed here from the scalar word: held across the stages it is the register that spills at N = 2^9 and 2^13 */
    uint64_t mq = kr.mq[limb];
    asm volatile("" : "+s"(mq));
    const double mb = A::reduce(A::u64_to_f64_lt52(mq), p.c);
    static_for<0, 4>([&](auto qq) {
      constexpr int Q = decltype(qq)::value;
      uint64_t      rc[kE], u[kE];
      sched_fence();
      load_last_raw<LOGN, 4 * Q, 4 * Q + 4>(rc, tg, cblk);
      static_for<4 * Q, 4 * Q + 4>([&](auto ee) {
        constexpr int E  = decltype(ee)::value;
        const double  cm = A::mulmod_c(mb, A::reduce(A::u64_to_f64_lt52(rc[E]), p.c), p.c); /* |c^ m mod q| <= q */
        const double  d  = A::reduce(cm - A::reduce(x[E], p.c), p.c);                      /* |.| <= 1.5 q before */
        u[E]             = A::mul_store(A::mulmod_c(sb, d, p.c), p.c);
      });
      if(live) store_last_raw<LOGN, 4 * Q, 4 * Q + 4>(u, tg, cblk);
      sched_fence();
    });
  }
}

template <class A, int LOGN, int KSH> hipError_t launch_moddown_exact_fwd_n(const ModDownExactFwdArgs &xa)
{
  using G                  = Geom<LOGN, false, flavor_of<A>()>;
  const ModDownFwdArgs &ma = xa.ma;
  if(ma.nlimbs < 1 || ma.nlimbs > kBconvLimbs || ma.nlimbs > kMaxLimbs || ma.np < 1 || ma.np > kBconvLimbs) return hipErrorInvalidValue;
  KModDownExactFwd<A> kr{};
  const uint64_t      nl = (uint64_t)ma.nlimbs;
  fill_kargs(kr.k, ma.c, ma.limbs, nl, ma.limb_stride, ma.poly_stride, ma.logn, 0, ma.batch);
  for(int l = 0; l < ma.nlimbs; l++) {
    kr.ql[l] = ma.ql[l];
    kr.mq[l] = xa.mq[l];
  }
  for(int j = 0; j < ma.np; j++) {
    kr.pl[j]  = ma.pl[j];
    kr.rho[j] = xa.rho[j];
  }
  kr.t  = ma.t;
  kr.np = ma.np;
  /* moddown_fwd_kernel's grid: the plain loop of the forward block kernel */
  const uint64_t wgs = block_grid<G>(ma.batch, 0, nl, ma.num_cus, ma.max_grid, G::PERSISTENT ? 1 : 4, true);
  if(ma.batch == 0) return hipSuccess;
  kr.k.wgs_per_limb = (uint32_t)wgs;
  hipLaunchKernelGGL((moddown_exact_fwd_kernel<A, LOGN, KSH>), dim3((unsigned)wgs, (unsigned)nl), dim3(G::WG), 0, ma.stream, kr);
  return hipGetLastError();
}

#define NTT_DEFINE_LAUNCH_MODDOWN_EXACT_FWD(A, KSH)                                                                                                   \
  template <> hipError_t launch_moddown_exact_fwd<A, KSH>(const ModDownExactFwdArgs &xa)                                                              \
  {                                                                                                                                                   \
    return with_int<6, 14>((int)xa.ma.logn, hipErrorNotSupported, [&](auto ln) { return launch_moddown_exact_fwd_n<A, decltype(ln)::value, KSH>(xa); }); \
  }

} // namespace ntt
