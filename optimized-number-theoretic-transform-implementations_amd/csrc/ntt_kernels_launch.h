/*
 * ntt_kernels_launch.h -- column_kernel (strided passes) and the type-erased launch interface: PassArgs / ProdArgs / DotArgs / MulArgs, the launchers that choose
 * grids and kernel variants, and the NTT_DEFINE_LAUNCH_* macros the inst_*.hip translation units expand.
 * Part of ntt_kernels.h (included from there, in this order: block, team, products, launch); not a header of its own.
 */
#pragma once

namespace ntt {

template <class A, int R, bool INV, int KSH, bool MULTI = false>
__global__ void __launch_bounds__(256) column_kernel(const KArgs<A> k)
{
  /* k.nblocks = polynomials per limb, k.s0 = first global stage of the pass */
  uint32_t           bid, gdim, limb_;
  const Params<A>    p     = limb_params<A, INV, MULTI>(k, bid, gdim, limb_);
  constexpr uint32_t MASK  = column_mask<A, R, INV, KSH>();
  const uint32_t     lcols = p.logn - R;
  const uint64_t     total = p.nblocks << lcols;
  for(uint64_t g = (uint64_t)bid * blockDim.x + threadIdx.x; g < total; g += (uint64_t)gdim * blockDim.x) {
    const uint64_t poly = g >> lcols;
    const uint32_t col  = (uint32_t)(g & ((1ull << lcols) - 1));
    if constexpr(A::kRadix4) {
      /* (even stage count: launch_pass refuses anything else for this policy) */
      if constexpr(R % 2 == 0) column_pass_thread_r4<A, R, INV>(p.a + poly_offset<false>(poly, p.pstride, p.ptab), col, p.logn, p.s0, p.tw, p.c, p.lazy != 0);
    } else {
      column_pass_thread<A, R, INV, MASK>(p.a + poly_offset<false>(poly, p.pstride, p.ptab), col, p.logn, p.s0, p.wide != 0, p.lastinv != 0, p.tw, p.c, p.lazy != 0);
    }
  }
}

/* ------------------------------------------------------------------ */
/* type-erased launch interface (one translation unit per policy/class) */
/* ------------------------------------------------------------------ */
struct PassArgs {
  uint64_t *  a;
  const void *limbs;       /* HOST array of LimbRec<A>, one per limb (copied into the kernel arguments) */
  int         nlimbs;      /* >= 1 */
  uint64_t    limb_stride; /* words between consecutive limbs' slabs   */
  uint64_t    poly_stride; /* words between consecutive polynomials of a limb (0 = dense: N) */
  const uint64_t *ptab;    /* pointer batch: DEVICE table of per-polynomial word offsets (a = null: entries are addresses / 8), `batch` entries;
                            * null = the progression above */
  uint64_t    batch;       /* polynomials per limb                     */
  uint32_t    logn;   /* whole transform                   */
  int         fused;  /* Pass::fused; 2 = both passes of a 2^16 / 2^17 transform in one workgroup (r = m - 14); 3 = both passes as
                       * items of one launch with the intermediate kept in the XCD's L2 (team_kernel, r = m - 12); 4 = a 2^15-point
                       * transform in one pass, the polynomial in the registers of one workgroup (onepass_kernel) */
  int         r;      /* Pass::r                           */
  int         s;      /* Pass::s                           */
  int         inverse;
  int         wide;
  int         lastinv;
  int         lazy;     /* the caller asked for lazy outputs of the whole transform */
  int         ends;     /* this pass is the last one of the transform */
  int         max_grid; /* cap on workgroups (0 = default) */
  int         num_cus;  /* compute units of the device     */
  int         oversub;  /* persistent block kernels: workgroups per resident slot (0 = block_oversub's default) */
  void *      team_ctl; /* fused == 3: device memory for the queues and counters (TeamCtl + batch counters) */
  int         team_lag, team_wpc;
  hipStream_t stream;
};

template <class A, int KSH> hipError_t launch_pass(const PassArgs &pa);

/* fused product (fused_product_kernel): c = inv(fwd(b) * ahat), whole polynomials of 2^14 points */
struct ProdArgs {
  uint64_t *      b;
  const uint64_t *ahat;
  uint64_t *      out;
  const void *    limbs;       /* HOST array of LimbRec<A> */
  int             nlimbs;
  uint64_t        limb_stride;
  uint64_t        poly_stride; /* words between consecutive polynomials of a limb, the same for all three operands (0 = dense: N) */
  uint64_t        batch;       /* per limb */
  uint32_t        logn;
  uint32_t        block_log; /* N > 2^14: log2 of the blocks (12, 13 or 14); the column passes around the launch cover logn - block_log stages */
  int             a_lazy;
  int             max_grid, num_cus;
  int             oversub;  /* as PassArgs::oversub */
  void *          team_ctl; /* launch_team_product: device memory for the queues and 2 * batch counters */
  int             team_lag, team_wpc;
  int             four; /* launch_team_product: ahat holds a's COEFFICIENTS; the launch transforms both operands */
  int             both; /* launch_product, N <= 2^14: the same for the fused product kernels */
  int             ptrs; /* launch_product, N <= 2^14, both: b, ahat and out are DEVICE TABLES of polynomial addresses (the PTRS kernels); nlimbs > 1: every
                             * polynomial's limbs limb_stride words apart behind its entry (launch_team_product: one limb) */
  uint64_t        ptr_limb_off; /* ptrs: words from every table entry to the (first) limb of this launch */
  hipStream_t     stream;
};
template <class A, int KSH> hipError_t launch_product(const ProdArgs &pa);
template <class A, int KSH> hipError_t launch_team_product(const ProdArgs &pa);

/* c = inverse block pass of sum_i a_i^ (.) b_i^ (dot_inv_kernel) */
struct DotArgs {
  uint64_t *             out;
  const uint64_t *const *a; /* HOST arrays of npairs device pointers (limb 0's slabs) */
  const uint64_t *const *b;
  int                    npairs;
  int                    lazy_in, b_bcast;
  const void *           limbs; /* HOST array of LimbRec<A> */
  int                    nlimbs;
  uint64_t               limb_stride, b_limb_stride;
  uint64_t               poly_stride; /* words between consecutive polynomials of a limb: every a_i^, c, and every b_i^ that is not broadcast (0 = dense: N) */
  uint64_t               batch;     /* per limb */
  uint32_t               logn;
  uint32_t               block_log; /* N > 2^14: log2 of the blocks (12 or 14); the inverse column passes follow as launches of their own */
  int                    max_grid, num_cus;
  int                    oversub; /* as PassArgs::oversub */
  void *                 team_ctl; /* N = 2^15..2^17: non-null = both passes as items of ONE launch (team_dot_kernel); TeamCtl + nlimbs * batch counters */
  int                    team_lag, team_wpc;
  int                    ptrs; /* out, every a[i] and every b[i] that is not broadcast are DEVICE TABLES of polynomial addresses; N <= 2^14 with nlimbs > 1: every
                                    * polynomial's limbs limb_stride words apart behind its entry (team_dot_kernel: one limb) */
  uint64_t               ptr_limb_off; /* ptrs: words from every table entry to the (first) limb of this launch */
  hipStream_t            stream;
};
template <class A, int KSH> hipError_t launch_dot(const DotArgs &da);

/* c^ = forward block pass of a, times b^ (+ c^) (fwd_mul_kernel) */
struct MulArgs {
  uint64_t *      a;   /* coefficients (N > 2^14: after the forward column passes) */
  const uint64_t *b;   /* b^ */
  uint64_t *      out; /* c^ */
  int             lazy_in, b_bcast, accumulate;
  const void *    limbs; /* HOST array of LimbRec<A> */
  int             nlimbs;
  uint64_t        limb_stride, b_limb_stride;
  uint64_t        poly_stride; /* words between consecutive polynomials of a limb: a, c^, and b^ unless broadcast (0 = dense: N) */
  uint64_t        batch;
  uint32_t        logn;
  uint32_t        block_log; /* N > 2^14: log2 of the blocks (12 or 14) */
  int             max_grid, num_cus;
  int             oversub; /* as PassArgs::oversub */
  void *          team_ctl; /* N = 2^15..2^17: non-null = column items and row items with the product as ONE launch (team_mul_kernel); a = the caller's coefficients */
  int             team_lag, team_wpc;
  int             one_pass; /* N = 2^15, FP64 policies: the transform in one pass with the product at its output (onepass_mul_kernel) */
  int             ptrs; /* a, out and b (unless broadcast) are DEVICE TABLES of polynomial addresses; N <= 2^14 with nlimbs > 1: every polynomial's limbs
                             * limb_stride words apart behind its entry (onepass_mul_kernel, team_mul_kernel: one limb) */
  uint64_t        ptr_limb_off; /* ptrs: words from every table entry to the (first) limb of this launch */
  hipStream_t     stream;
};
template <class A, int KSH> hipError_t launch_fwd_mul(const MulArgs &ma);

/* What a pass stores: the last pass of a transform honours the caller's lazy flag; every earlier pass of an
 * integer policy keeps the reference's lazy ranges in HBM (no reduction between stages, as in
 * src/ntt_reference.c:17-30 -- which also makes the final lazy values the reference's bit for bit).  The FP64
 * policy ignores the run-time flag (its passes exchange canonical words). */
inline int pass_lazy(const PassArgs &pa) { return pa.ends ? pa.lazy : 1; }

/* the MULTI kernel variants exist for the scheduled FP64 policy, its 52-bit form and the wide integer policy (RNS bases of
 * 54..60-bit primes: a ciphertext is a few polynomials x tens of such limbs -- one launch instead of one chain per prime) */
template <class A> constexpr bool multi_limb_built() { return A::kCompact || A::kIntWide; }

inline uint64_t limb_count(int nlimbs) { return (uint64_t)(nlimbs > 0 ? nlimbs : 1); }

/* Run-time flags as template arguments: with_bools(f, b0, b1, ..) calls f(std::bool_constant<b0>{}, std::bool_constant<b1>{}, ..).
 * f is instantiated for EVERY combination: it guards the kernel variants that are not built with `if constexpr`. */
template <class F> inline hipError_t with_bools(F &&f) { return f(); }
template <class F, class... B> inline hipError_t with_bools(F &&f, bool b, B... rest)
{
  return b ? with_bools([&](auto... c) { return f(std::true_type{}, c...); }, rest...)
           : with_bools([&](auto... c) { return f(std::false_type{}, c...); }, rest...);
}
/* (with_int, a run-time value as a template argument: ntt_kernels_block.h) */

/* The pointer-table form of a launch (separately held polynomials): the kernel's PTRS variant reads every operand pointer as a
 * DEVICE table of polynomial addresses; k.ptab is the table behind k.a's operand and k.a what is left of the address -- the words
 * from every entry to the (first) limb of the launch, as a byte offset. */
template <class A> inline void use_ptr_table(KArgs<A> &k, const uint64_t *table, uint64_t limb_off)
{
  k.ptab = table;
  k.a    = reinterpret_cast<uint64_t *>((uintptr_t)limb_off * 8u);
}

/* Workgroups launched per resident slot of a persistent block kernel.  One workgroup per slot (the r01..r04 grids) lets the four
 * 256-thread workgroups that share a CU at 2^12 run IN PHASE for the whole launch: they start together, do identical work and
 * meet at the memory system, the LDS pipe and their barriers at the same time.  With several times as many workgroups as
 * slots a slot is refilled whenever its workgroup runs out of blocks, at a time of its own, and the phases of a CU's workgroups
 * decorrelate: measured (profiles/r05/grid_sweep.txt, three alternating repetitions on one box) 2^12 forward 0.592 -> 0.622 of
 * the roofline at 8 workgroups per slot, inverse 0.617 -> 0.641, flat from 8 to 16, 0.61 with one block per workgroup (no
 * prefetch across blocks left); the 1024-thread kernels (2^13, 2^14: one workgroup per CU, 16 waves in step by construction)
 * measured no gain (0.591 at 1, 2, 4 per slot, 0.586 at 8) and keep one.  requested > 0 (NTT_OPT_BLOCK_OVERSUB) overrides. */
template <int LOGN, int WG> constexpr int block_oversub_default(bool whole_polynomials)
{
  return (LOGN == 12 && WG == 256 && whole_polynomials) ? 8 : 1;
}
template <int LOGN, int WG> inline uint64_t block_oversub(int requested, bool whole_polynomials)
{
  return (uint64_t)(requested > 0 ? requested : block_oversub_default<LOGN, WG>(whole_polynomials));
}
/* block_grid's per_slot for the product launchers around a block kernel (dot, forward-multiply): the transforms' oversubscription
 * of the persistent sizes, four looping workgroups per slot where the tables are filled once per workgroup */
template <class G, int LOGN> inline uint64_t product_per_slot(int requested, bool whole_polynomials)
{
  return G::PERSISTENT ? block_oversub<LOGN, G::WG>(requested, whole_polynomials) : 4;
}
/* kernels that fill LDS tables once per workgroup and loop: whole polynomials only (the table depends on the block position) */
template <class G> constexpr bool fills_tables() { return !G::PERSISTENT && G::LDS_TW > 0; }

template <class A> KArgs<A> make_kargs(const PassArgs &pa)
{
  KArgs<A> k{};
  fill_kargs(k, pa.a, pa.limbs, limb_count(pa.nlimbs), pa.limb_stride, pa.poly_stride, pa.logn, 0, pa.batch);
  k.wide    = (uint32_t)pa.wide;
  k.lastinv = (uint32_t)pa.lastinv;
  k.lazy    = (uint32_t)pa.lazy;
  k.ptab    = pa.ptab;
  return k;
}

template <class A, int LOGN, bool INV, int KSH> hipError_t launch_fused(const PassArgs &pa)
{
  using G = Geom<LOGN, INV, flavor_of<A>()>;
  if(fills_tables<G>() && pa.s != 0) return hipErrorInvalidValue;
  KArgs<A> p  = make_kargs<A>(pa);
  p.s0        = (uint32_t)pa.s;
  p.lazy      = (uint32_t)pass_lazy(pa);
  p.nblocks   = pa.batch << pa.s;
  const uint64_t nl = limb_count(pa.nlimbs);
  /* Workgroups that loop over the slab in step produce their loads and stores in bursts; how well the memory system takes
   * them depends on the allocation (the "two modes" of 2^8..2^10: 0.63 or 0.72 of the roofline from one hipMalloc block to
   * the next, profiles/r05/small_size_modes.txt).  At 2^8 and 2^9, where a table fill is cheap, sixteen times as many
   * workgroups (one or two iterations each on a 6 GiB slab) lift the slow mode by 5-7 % (0.633 -> 0.678, 0.636 -> 0.667;
   * inverse +4.5 %) and leave the fast one where it was; 2^10 and 2^11 lose what the larger tables cost, 2^6 and 2^7 are mixed:
   * unchanged (profiles/r05/small_size_grid.txt). */
  const uint64_t per_slot = G::PERSISTENT ? block_oversub<LOGN, G::WG>(pa.oversub, pa.s == 0)
                                          : (uint64_t)(pa.oversub > 0 ? pa.oversub : ((LOGN == 8 || LOGN == 9) ? 64 : 4)); /* (NTT_OPT_BLOCK_OVERSUB: sweeps) */
  /* 2^10: about six iterations per workgroup on large batches (32768 workgroups on a 6 GiB slab: slow mode 0.633 -> 0.653; the
   * 8192 of smaller batches stay, where more workgroups lost 2 %) */
  const uint64_t min_cap = (fills_tables<G>() && LOGN == 10 && pa.oversub <= 0) ? ((p.nblocks + G::BPW - 1) / G::BPW) / 6 : 0;
  const uint64_t wgs     = block_grid<G>(p.nblocks, p.s0, nl, pa.num_cus, pa.max_grid, per_slot, false, min_cap);
  if(wgs == 0) return hipSuccess;
  p.wgs_per_limb = (uint32_t)wgs;
  const dim3 grid((unsigned)wgs, (unsigned)nl), wg(G::WG); /* (MULTI variants: blockIdx.y is the limb) */
  /* several limbs in one launch: the MULTI variants, built for the policies RNS bases use */
  return with_bools([&](auto multi) -> hipError_t {
    constexpr bool MULTI = decltype(multi)::value;
    if constexpr(MULTI && !multi_limb_built<A>()) {
      return hipErrorNotSupported;
    } else if constexpr(INV) {
      /* the inverse kernel exists in two variants: ending a whole transform (N^-1 folded into
       * its last group) -- every block size -- and, for the block size used below column
       * passes, not ending it */
      static_assert(!(A::kRadix4 && multi_limb_built<A>()), "radix-4: single-limb launches only (its blocks always take the LASTINV kernel)");
      if(pa.lastinv || A::kRadix4) {
        /* (radix-4 formulation: N^-1 is a pass of its own, fused into the LAST pass's store -- the blocks of a larger
         * transform run the same kernel with the multiplier record of 1: host/host_plan.inc, limbrec_mid) */
        hipLaunchKernelGGL((fused_kernel<A, LOGN, true, KSH, true, false, MULTI>), grid, wg, 0, pa.stream, p);
      } else if constexpr(LOGN == kFusedLarge || LOGN == kFusedSmallBlock) {
        hipLaunchKernelGGL((fused_kernel<A, LOGN, true, KSH, false, false, MULTI>), grid, wg, 0, pa.stream, p);
      } else {
        return hipErrorInvalidValue;
      }
    } else {
      if constexpr(A::kTracksBounds) { /* (lazy outputs: a kernel variant for the FP64 policies, a run-time flag for the integer ones) */
        if(pa.ends && pa.lazy) {
          hipLaunchKernelGGL((fused_kernel<A, LOGN, false, KSH, false, true, MULTI>), grid, wg, 0, pa.stream, p);
          return hipGetLastError();
        }
      }
      hipLaunchKernelGGL((fused_kernel<A, LOGN, false, KSH, false, false, MULTI>), grid, wg, 0, pa.stream, p);
    }
    return hipGetLastError();
  }, nl > 1);
}

/* pa.r = LEAD (1..3): the whole transform of 2^(14+LEAD) points in one launch; pa.batch polynomials */
/* Built for the FP64 policy at N = 2^16 and 2^17 (BASELINE configs 3 and 5).  The integer policy's larger
 * temporaries and the N = 2^15 inverse do not fit the 128-register budget of a 1024-thread workgroup without
 * scratch: those cases stay on the one-launch-per-pass path (host/host_transforms.inc: the two_phase condition). */
template <class A, int LEAD> constexpr bool two_phase_built() { return A::kTracksBounds && LEAD >= 2; }

template <class A, int LEAD, bool INV, int KSH> hipError_t launch_twophase(const PassArgs &pa)
{
  if constexpr(!two_phase_built<A, LEAD>()) {
    return hipErrorNotSupported;
  } else {
  if(pa.nlimbs > 1) return hipErrorNotSupported; /* (RNS sets take the per-pass launches) */
  KArgs<A> p = make_kargs<A>(pa);
  p.s0       = (uint32_t)LEAD;
  p.lastinv  = (uint32_t)pa.inverse;
  uint64_t wgs = pa.batch;
  uint64_t cap = (uint64_t)(pa.num_cus > 0 ? pa.num_cus : 256);
  if(pa.max_grid > 0) cap = (uint64_t)pa.max_grid;
  if(wgs > cap) wgs = cap;
  if(wgs == 0) return hipSuccess;
  p.wgs_per_limb = (uint32_t)wgs;
  hipLaunchKernelGGL((twophase_kernel<A, LEAD, INV, KSH>), dim3((unsigned)wgs), dim3(1024), 0, pa.stream, p);
  return hipGetLastError();
  }
}

/* grid of the one-pass 2^15 kernels: one persistent 1024-thread workgroup per CU, the limbs of a launch sharing them */
inline uint64_t onepass_grid(uint64_t batch, uint64_t nl, int num_cus, int max_grid)
{
  uint64_t cap = (uint64_t)(num_cus > 0 ? num_cus : 256);
  if(max_grid > 0) cap = (uint64_t)max_grid;
  cap = cap / nl > 0 ? cap / nl : 1;
  return batch < cap ? batch : cap;
}

/* N = 2^15 in one pass (onepass_kernel), pa.batch polynomials per limb */
template <class A> constexpr bool onepass_built() { return A::kCompact && A::kTracksBounds; }
template <class A, bool INV, int KSH> hipError_t launch_onepass(const PassArgs &pa)
{
  if constexpr(!onepass_built<A>()) {
    return hipErrorNotSupported;
  } else {
    if(pa.logn != (uint32_t)kFusedLarge + 1) return hipErrorNotSupported; /* (a lazy call gets canonical words: inside the lazy ranges) */
    const uint64_t nl = limb_count(pa.nlimbs);
    if(nl > (uint64_t)kMaxLimbs) return hipErrorNotSupported;
    KArgs<A> p = make_kargs<A>(pa);
    p.s0       = 1;
    p.lastinv  = (uint32_t)pa.inverse;
    p.lazy     = 0;
    const uint64_t wgs = onepass_grid(pa.batch, nl, pa.num_cus, pa.max_grid);
    if(wgs == 0) return hipSuccess;
    p.wgs_per_limb = (uint32_t)wgs;
    const dim3 grid((unsigned)wgs, (unsigned)nl);
    return with_bools([&](auto multi) {
      hipLaunchKernelGGL((onepass_kernel<A, INV, KSH, decltype(multi)::value>), grid, dim3(1024), 0, pa.stream, p);
      return hipGetLastError();
    }, nl > 1);
  }
}

/* Zeroes a control block (queue heads, owners, per-polynomial counters) in front of an XCD-local launch -- as a KERNEL, not as an
 * asynchronous memset: captured into a HIP graph, a memset node in front of the kernel node did not always take effect before the
 * kernel's first workgroups read the counters (stale counters of the previous replay: second-pass items that do not wait, or
 * queues that look exhausted -- found by replaying a captured NTT-domain product between other work, round 5:
 * tests/test_gpu_parity.py::test_one_launch_ntt_domain_products_captured_in_a_hip_graph).  A kernel in front of a kernel on the
 * same stream is ordered in a graph exactly as outside one. */
static __global__ void __launch_bounds__(256) team_ctl_clear_kernel(unsigned *w, size_t n)
{
  for(size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) w[i] = 0u;
}
static inline hipError_t team_ctl_clear(void *ctl, size_t bytes, hipStream_t stream)
{
  const size_t n = (bytes + 3) / 4;
  size_t       g = (n + 255) / 256;
  if(g > 64) g = 64;
  hipLaunchKernelGGL(team_ctl_clear_kernel, dim3((unsigned)g), dim3(256), 0, stream, static_cast<unsigned *>(ctl), n);
  return hipGetLastError();
}

/* What the XCD-local ("team") launchers share, in front of their kernel arguments: refuses (before anything is enqueued) more limbs
 * than records, a missing control block and 2^limit_log or more polynomials; fills kt's queue fields (ar.team_lag, else
 * default_lag; the numbering of the queues' polynomials); zeroes the control block -- Ctl and `counters` counters per polynomial;
 * and sets the grid: ar.team_wpc (default four: 40.6 KB of LDS each, at most 128 VGPRs) 256-thread workgroups per CU, or ar.max_grid. */
template <class Ctl, class KT, class Args>
inline hipError_t team_prologue(KT &kt, const Args &ar, int limit_log, int counters, int default_lag, dim3 &grid)
{
  const uint64_t nl = limb_count(ar.nlimbs);
  if(nl > (uint64_t)kMaxLimbs || !ar.team_ctl || nl * ar.batch >= (1ull << limit_log)) return hipErrorNotSupported;
  kt.ctl        = static_cast<Ctl *>(ar.team_ctl);
  kt.lag        = (uint32_t)(ar.team_lag > 0 ? ar.team_lag : default_lag);
  kt.nlimbs     = (uint32_t)nl;
  kt.poly_major = nl > 1 && (ar.poly_stride ? ar.poly_stride : (1ull << ar.logn)) > ar.limb_stride;
  kt.split_rcp  = team_split_rcp(kt.poly_major ? nl : ar.batch);
  uint64_t wgs  = (uint64_t)(ar.num_cus > 0 ? ar.num_cus : 256) * (ar.team_wpc > 0 ? ar.team_wpc : 4);
  if(ar.max_grid > 0) wgs = (uint64_t)ar.max_grid;
  grid = dim3((unsigned)wgs);
  return team_ctl_clear(ar.team_ctl, sizeof(Ctl) + (size_t)counters * (size_t)(nl * ar.batch) * sizeof(unsigned), ar.stream);
}

/* pa.r = LEAD (3..5), pa.batch polynomials of 2^(12 + LEAD) points per limb; pa.team_ctl: TeamCtl with nlimbs * batch counters,
 * zeroed here.  Several limbs (an RNS set, [limb][batch][N]): the MULTI variant, the queues run over all limbs' polynomials. */
template <class A, int LEAD, bool INV, int KSH> hipError_t launch_team(const PassArgs &pa)
{
  if constexpr(!(A::kCompact || A::kIntWide)) {
    return hipErrorNotSupported;
  } else {
    if(pa.wide || pa.lazy) return hipErrorNotSupported;
    KTeam<A>         kt{};
    dim3             grid;
    const hipError_t e = team_prologue<TeamCtl>(kt, pa, 31, 1, 6, grid);
    if(e != hipSuccess) return e;
    kt.k              = make_kargs<A>(pa);
    kt.k.lazy         = 0; /* canonical out (the integer policies read this flag at run time) */
    kt.k.lastinv      = (uint32_t)pa.inverse;
    kt.k.wgs_per_limb = grid.x;
    return with_bools([&](auto multi) {
      hipLaunchKernelGGL((team_kernel<A, LEAD, INV, KSH, decltype(multi)::value>), grid, dim3(256), 0, pa.stream, kt);
      return hipGetLastError();
    }, kt.nlimbs > 1);
  }
}

template <class A, int R, bool INV, int KSH> hipError_t launch_column(const PassArgs &pa)
{
  KArgs<A> p = make_kargs<A>(pa);
  p.s0       = (uint32_t)pa.s;
  p.lazy     = (uint32_t)pass_lazy(pa);
  const uint64_t nl    = limb_count(pa.nlimbs);
  const uint64_t total = pa.batch << (pa.logn - R);
  uint64_t       wgs   = (total + 255) / 256;
  uint64_t       cap   = pa.max_grid > 0 ? (uint64_t)pa.max_grid : (1ull << 22);
  cap                  = cap / nl > 0 ? cap / nl : 1;
  if(wgs > cap) wgs = cap;
  if(wgs == 0) return hipSuccess;
  p.wgs_per_limb = (uint32_t)wgs;
  return with_bools([&](auto multi) -> hipError_t {
    constexpr bool MULTI = decltype(multi)::value;
    if constexpr(MULTI && !multi_limb_built<A>()) {
      return hipErrorNotSupported;
    } else {
      hipLaunchKernelGGL((column_kernel<A, R, INV, KSH, MULTI>), dim3((unsigned)wgs, (unsigned)nl), dim3(256), 0, pa.stream, p);
      return hipGetLastError();
    }
  }, nl > 1);
}

/* fused product on blocks of 2^BL points: whole polynomials (BL = logn; 8..11: fused_product_small_kernel) or the blocks of a
 * larger one between column passes (BL = 12 or 14); pp is filled but for the grid */
template <class A, int KSH, int BL> hipError_t launch_product_blocks(const ProdArgs &pa, KProd<A> &pp)
{
  using G = Geom<BL, false, 3>;
  const uint32_t s0 = pp.f.s0;
  const uint64_t nl = limb_count(pa.nlimbs);
  /* 2^8..2^11: tables filled once per workgroup, four looping workgroups per slot.  2^12: 256-thread workgroups, one wave per SIMD
   * each; whole polynomials: several workgroups per resident slot, as for the transforms -- block_oversub; measured 0.369 -> 0.401
   * of the 24N roofline at 8 per slot, profiles/r05/oversub_sweep.txt.  2^13: one 512-thread workgroup per CU by LDS (64 KB exchange
   * buffer + 30 KB table; a second one does not fit); 2^14: one of 1024 threads.
   * From 2^12 up a workgroup keeps the tables of ONE block position: its stride is a multiple of the blocks per polynomial. */
  static_assert(BL < 12 ? fills_tables<G>() : (G::PERSISTENT && G::BPW == 1), "the grid rule block_grid applies to this geometry");
  static_assert(BL != 12 || (G::WG == 256 && G::WG_PER_CU0 >= 1), "2^12: one wave per SIMD each, min(WG_PER_CU0, WPS) resident");
  static_assert(BL < 13 || (G::WG_PER_CU0 == 1 && G::WPS * 256 >= G::WG), "2^13, 2^14: one workgroup per CU");
  const uint64_t per_slot = BL < 12 ? 4 : (BL == 12 ? block_oversub<12, G::WG>(pa.oversub, s0 == 0) : 1);
  pp.f.wgs_per_limb = (uint32_t)block_grid<G>(pp.f.nblocks, s0, nl, pa.num_cus, pa.max_grid, per_slot);
  const dim3 grid(pp.f.wgs_per_limb, (unsigned)nl), wg(G::WG);
  return with_bools([&](auto multi, auto both, auto whole, auto ptrs) -> hipError_t {
    constexpr bool MULTI = decltype(multi)::value, BOTH = decltype(both)::value, WHOLE = decltype(whole)::value, PTRS = decltype(ptrs)::value;
    /* (the PTRS kernels: both operands' coefficients, whole polynomials -- refused by the caller otherwise) */
    /* (2^13-point blocks of a larger product: measured no faster than 2^14, not built) */
    if constexpr((PTRS && !(BOTH && WHOLE)) || (BL == 13 && !WHOLE)) {
      return hipErrorNotSupported;
    } else if constexpr(BL < 12) {
      hipLaunchKernelGGL((fused_product_small_kernel<A, BL, KSH, MULTI, BOTH, PTRS>), grid, wg, 0, pa.stream, pp);
      return hipGetLastError();
    } else {
      hipLaunchKernelGGL((fused_product_kernel<A, BL, KSH, true, WHOLE, MULTI, BOTH, PTRS>), grid, wg, 0, pa.stream, pp);
      return hipGetLastError();
    }
  }, nl > 1, pa.both, s0 == 0, pa.ptrs);
}

template <class A, int KSH> hipError_t launch_product_impl(const ProdArgs &pa)
{
  if constexpr(!A::kCompact) {
    return hipErrorNotSupported;
  } else {
    if(pa.logn < 8 || pa.logn > 17) return hipErrorNotSupported;
    const uint32_t blog = pa.logn <= 14 ? pa.logn : (pa.block_log ? pa.block_log : 14u);
    if(blog < 12 && pa.logn > 14) return hipErrorInvalidValue;
    const uint32_t s0 = pa.logn - blog; /* leading stages done by column passes around this launch */
    KProd<A> pp{};
    fill_kargs(pp.f, pa.b, pa.limbs, limb_count(pa.nlimbs), pa.limb_stride, pa.poly_stride, pa.logn, s0, pa.batch << s0);
    pp.ahat   = pa.ahat;
    pp.out    = pa.out;
    pp.a_lazy = (uint32_t)pa.a_lazy;
    if(pp.f.nblocks == 0) return hipSuccess;
    /* a^ always arrives as the lazy words ntt_fwd_batch_lazy leaves (the canonical-operand variant is not built) -- or not
     * at all: pa.both, whole polynomials, a's coefficients in pa.ahat */
    if(!pa.a_lazy && !pa.both) return hipErrorNotSupported;
    if(pa.both && s0 != 0 && blog != 12 && blog != 14) return hipErrorInvalidValue;
    if(pa.ptrs) {
      /* separately held polynomials: the three operand pointers are tables (several limbs: the limbs of every polynomial
       * pa.limb_stride words apart behind its table entry -- the MULTI instances, whose limb_params add limb * limb_stride) */
      if(!pa.both || s0 != 0) return hipErrorNotSupported;
      use_ptr_table(pp.f, pa.b, pa.ptr_limb_off);
    }
    /* (a block_log above 14 runs the 2^14 kernel) */
    return with_int<8, 14>(blog < 14 ? (int)blog : 14, hipErrorNotSupported, [&](auto bl) { return launch_product_blocks<A, KSH, decltype(bl)::value>(pa, pp); });
  }
}

/* a product at N = 2^15..2^17 as one launch (team_product_kernel); pa.team_ctl: TeamProdCtl + 2 * nlimbs * batch counters.
 * Several limbs ([limb][batch][N] slabs, limb_stride apart): the MULTI variants -- ONE launch for a whole RNS product. */
template <class A, int KSH> hipError_t launch_team_product_impl(const ProdArgs &pa)
{
  if constexpr(!A::kCompact) {
    return hipErrorNotSupported;
  } else {
    if((!pa.a_lazy && !pa.four) || pa.logn < kTeamBlock + 3 || pa.logn > kTeamBlock + 5) return hipErrorNotSupported;
    KTeamProd<A>     kt{};
    dim3             grid;
    const hipError_t e = team_prologue<TeamProdCtl>(kt, pa, 30, 2, 8, grid);
    if(e != hipSuccess) return e;
    fill_kargs(kt.k.f, pa.b, pa.limbs, kt.nlimbs, kt.nlimbs > 1 ? pa.limb_stride : 0, pa.poly_stride, pa.logn, pa.logn - kTeamBlock, pa.batch);
    kt.k.f.wgs_per_limb = grid.x;
    kt.k.ahat           = pa.ahat;
    kt.k.out            = pa.out;
    kt.k.a_lazy         = 1;
    /* pa.ptrs: b, ahat (a's coefficients) and out are device tables (several limbs: every polynomial's limbs pa.limb_stride words
     * apart behind its table entry -- the MULTI instances) */
    if(pa.ptrs) use_ptr_table(kt.k.f, pa.b, pa.ptr_limb_off);
    return with_int<3, 5>((int)(pa.logn - kTeamBlock), hipErrorNotSupported, [&](auto lead) {
      /* four: ahat = a itself (coefficients), both forward transforms happen inside the launch */
      return with_bools([&](auto four, auto multi, auto ptrs) -> hipError_t {
        constexpr bool FOUR = decltype(four)::value, MULTI = decltype(multi)::value, PTRS = decltype(ptrs)::value;
        if constexpr(PTRS && !FOUR) {
          return hipErrorNotSupported;
        } else {
          hipLaunchKernelGGL((team_product_kernel<A, decltype(lead)::value, KSH, FOUR, MULTI, PTRS>), grid, dim3(256), 0, pa.stream, kt);
          return hipGetLastError();
        }
      }, pa.four, kt.nlimbs > 1, pa.ptrs);
    });
  }
}

/* the operand fields of dot_inv_kernel and team_dot_kernel */
template <class A> inline void fill_dot(KDot<A> &kd, const DotArgs &da, uint64_t b_limb_stride)
{
  kd.npairs        = (uint32_t)da.npairs;
  kd.lazy_in       = (uint32_t)da.lazy_in;
  kd.b_bcast       = (uint32_t)da.b_bcast;
  kd.b_limb_stride = b_limb_stride;
  for(int i = 0; i < da.npairs && i < kMaxDot; i++) {
    kd.a[i] = da.a[i];
    kd.b[i] = da.b[i];
  }
}

/* the inverse block kernel's grid: resident workgroups striding over the blocks */
template <class A, int LOGN, int KSH, bool LASTINV> hipError_t launch_dot_blocks(const DotArgs &da)
{
  using G = Geom<LOGN, true, flavor_of<A>()>;
  const uint32_t s0 = da.logn - (uint32_t)LOGN;
  if(fills_tables<G>() && s0 != 0) return hipErrorInvalidValue;
  KDot<A>        kd{};
  const uint64_t nl = limb_count(da.nlimbs);
  fill_kargs(kd.k, da.out, da.limbs, nl, da.limb_stride, da.poly_stride, da.logn, s0, da.batch << s0);
  kd.k.lastinv = LASTINV ? 1u : 0u;
  kd.k.lazy    = LASTINV ? 0u : 1u;
  fill_dot(kd, da, da.b_limb_stride);
  const uint64_t wgs = block_grid<G>(kd.k.nblocks, s0, nl, da.num_cus, da.max_grid, product_per_slot<G, LOGN>(da.oversub, s0 == 0));
  if(wgs == 0) return hipSuccess;
  kd.k.wgs_per_limb = (uint32_t)wgs;
  if(da.ptrs) use_ptr_table(kd.k, da.out, da.ptr_limb_off);
  /* (several limbs with tables: the limbs of an RNS set behind every table entry, da.limb_stride words apart) */
  return with_bools([&](auto multi, auto ptrs) -> hipError_t {
    constexpr bool MULTI = decltype(multi)::value, PTRS = decltype(ptrs)::value;
    if constexpr((PTRS && !LASTINV) || (MULTI && !multi_limb_built<A>())) {
      return hipErrorNotSupported;
    } else {
      hipLaunchKernelGGL((dot_inv_kernel<A, LOGN, KSH, LASTINV, MULTI, PTRS>), dim3((unsigned)wgs, (unsigned)nl), dim3(G::WG), 0, da.stream, kd);
      return hipGetLastError();
    }
  }, nl > 1, da.ptrs);
}

/* the NTT-domain product at N = 2^15..2^17 as ONE launch (team_dot_kernel); da.team_ctl: TeamCtl + nlimbs * batch counters, zeroed here */
template <class A, int KSH> hipError_t launch_team_dot(const DotArgs &da)
{
  if constexpr(!(A::kCompact || A::kIntWide)) {
    return hipErrorNotSupported;
  } else {
    if(da.logn < (uint32_t)kTeamBlock + 3 || da.logn > (uint32_t)kTeamBlock + 5 || da.npairs < 1 || da.npairs > kMaxDot) return hipErrorNotSupported;
    KTeamDot<A>      kt{};
    dim3             grid;
    const hipError_t e = team_prologue<TeamCtl>(kt, da, 31, 1, 8, grid);
    if(e != hipSuccess) return e;
    const bool multi = kt.nlimbs > 1;
    fill_kargs(kt.d.k, da.out, da.limbs, kt.nlimbs, multi ? da.limb_stride : 0, da.poly_stride, da.logn, da.logn - (uint32_t)kTeamBlock, da.batch);
    kt.d.k.wgs_per_limb = grid.x;
    kt.d.k.lastinv      = 1;
    kt.d.k.lazy         = 0;
    fill_dot(kt.d, da, multi ? da.b_limb_stride : 0);
    if(da.ptrs) use_ptr_table(kt.d.k, da.out, da.ptr_limb_off);
    return with_int<3, 5>((int)(da.logn - kTeamBlock), hipErrorNotSupported, [&](auto lead) {
      return with_bools([&](auto multi_c, auto ptrs) {
        hipLaunchKernelGGL((team_dot_kernel<A, decltype(lead)::value, KSH, decltype(multi_c)::value, decltype(ptrs)::value>), grid, dim3(256), 0, da.stream, kt);
        return hipGetLastError();
      }, multi, da.ptrs);
    });
  }
}

template <class A, int KSH> hipError_t launch_dot_impl(const DotArgs &da)
{
  if(da.npairs < 1 || da.npairs > kMaxDot || da.nlimbs > kMaxLimbs) return hipErrorInvalidValue;
  if(da.team_ctl) return launch_team_dot<A, KSH>(da);
  if(da.logn > (uint32_t)kFusedMax) {
    if(da.ptrs) return hipErrorNotSupported;
    if(da.block_log == (uint32_t)kFusedSmallBlock) return launch_dot_blocks<A, kFusedSmallBlock, KSH, false>(da);
    if(da.block_log == (uint32_t)kFusedLarge) return launch_dot_blocks<A, kFusedLarge, KSH, false>(da);
    return hipErrorInvalidValue;
  }
  return with_int<6, 14>((int)da.logn, hipErrorNotSupported, [&](auto ln) { return launch_dot_blocks<A, decltype(ln)::value, KSH, true>(da); });
}

/* the operand fields of fwd_mul_kernel, team_mul_kernel and onepass_mul_kernel */
template <class A> inline void fill_mul(KMul<A> &km, const MulArgs &ma, uint64_t b_limb_stride)
{
  km.b             = ma.b;
  km.out           = ma.out;
  km.b_limb_stride = b_limb_stride;
  km.lazy_in       = (uint32_t)ma.lazy_in;
  km.b_bcast       = (uint32_t)ma.b_bcast;
  km.accumulate    = (uint32_t)ma.accumulate;
}

/* the forward block kernel's grid */
template <class A, int LOGN, int KSH> hipError_t launch_fwd_mul_blocks(const MulArgs &ma)
{
  using G = Geom<LOGN, false, flavor_of<A>()>;
  const uint32_t s0 = ma.logn - (uint32_t)LOGN;
  if((fills_tables<G>() || G::BPW > 1) && s0 != 0) return hipErrorInvalidValue; /* (two blocks per workgroup: whole polynomials only) */
  KMul<A>        km{};
  const uint64_t nl = limb_count(ma.nlimbs);
  fill_kargs(km.k, ma.a, ma.limbs, nl, ma.limb_stride, ma.poly_stride, ma.logn, s0, ma.batch << s0);
  fill_mul(km, ma, ma.b_limb_stride);
  const uint64_t wgs = block_grid<G>(km.k.nblocks, s0, nl, ma.num_cus, ma.max_grid, product_per_slot<G, LOGN>(ma.oversub, s0 == 0));
  if(wgs == 0) return hipSuccess;
  km.k.wgs_per_limb = (uint32_t)wgs;
  if(ma.ptrs) {
    if(s0 != 0) return hipErrorNotSupported;
    use_ptr_table(km.k, ma.a, ma.ptr_limb_off);
  }
  /* (several limbs with tables: the limbs of an RNS set behind every table entry, ma.limb_stride words apart) */
  return with_bools([&](auto multi, auto ptrs) -> hipError_t {
    constexpr bool MULTI = decltype(multi)::value, PTRS = decltype(ptrs)::value;
    if constexpr(MULTI && !multi_limb_built<A>()) {
      return hipErrorNotSupported;
    } else {
      hipLaunchKernelGGL((fwd_mul_kernel<A, LOGN, KSH, MULTI, PTRS>), dim3((unsigned)wgs, (unsigned)nl), dim3(G::WG), 0, ma.stream, km);
      return hipGetLastError();
    }
  }, nl > 1, ma.ptrs);
}

template <class A, int KSH> hipError_t launch_team_mul(const MulArgs &ma)
{
  if constexpr(!(A::kCompact || A::kIntWide)) {
    return hipErrorNotSupported;
  } else {
    if(ma.logn < (uint32_t)kTeamBlock + 3 || ma.logn > (uint32_t)kTeamBlock + 5) return hipErrorNotSupported;
    KTeamMul<A>      kt{};
    dim3             grid;
    const hipError_t e = team_prologue<TeamCtl>(kt, ma, 31, 1, 8, grid);
    if(e != hipSuccess) return e;
    const bool multi = kt.nlimbs > 1;
    fill_kargs(kt.m.k, ma.a, ma.limbs, kt.nlimbs, multi ? ma.limb_stride : 0, ma.poly_stride, ma.logn, ma.logn - (uint32_t)kTeamBlock, ma.batch);
    kt.m.k.wgs_per_limb = grid.x;
    kt.m.k.lazy         = 0;
    fill_mul(kt.m, ma, multi ? ma.b_limb_stride : 0);
    if(ma.ptrs) use_ptr_table(kt.m.k, ma.a, ma.ptr_limb_off);
    return with_int<3, 5>((int)(ma.logn - kTeamBlock), hipErrorNotSupported, [&](auto lead) {
      return with_bools([&](auto multi_c, auto ptrs) {
        hipLaunchKernelGGL((team_mul_kernel<A, decltype(lead)::value, KSH, decltype(multi_c)::value, decltype(ptrs)::value>), grid, dim3(256), 0, ma.stream, kt);
        return hipGetLastError();
      }, multi, ma.ptrs);
    });
  }
}

/* N = 2^15 in one pass with the product at the output (onepass_mul_kernel) */
template <class A, int KSH> hipError_t launch_onepass_mul(const MulArgs &ma)
{
  if constexpr(!onepass_built<A>()) {
    return hipErrorNotSupported;
  } else {
    if(ma.logn != (uint32_t)kFusedLarge + 1) return hipErrorNotSupported;
    const uint64_t nl = limb_count(ma.nlimbs);
    KMul<A>        km{};
    fill_kargs(km.k, ma.a, ma.limbs, nl, ma.limb_stride, ma.poly_stride, ma.logn, 1, ma.batch);
    fill_mul(km, ma, ma.b_limb_stride);
    const uint64_t wgs = onepass_grid(ma.batch, nl, ma.num_cus, ma.max_grid);
    if(wgs == 0) return hipSuccess;
    km.k.wgs_per_limb = (uint32_t)wgs;
    if(ma.ptrs) use_ptr_table(km.k, ma.a, ma.ptr_limb_off);
    return with_bools([&](auto multi, auto ptrs) -> hipError_t {
      constexpr bool MULTI = decltype(multi)::value, PTRS = decltype(ptrs)::value;
      if constexpr(MULTI && PTRS) { /* (tables: one limb per launch) */
        return hipErrorNotSupported;
      } else {
        hipLaunchKernelGGL((onepass_mul_kernel<A, KSH, MULTI, PTRS>), dim3((unsigned)wgs, (unsigned)nl), dim3(1024), 0, ma.stream, km);
        return hipGetLastError();
      }
    }, nl > 1, ma.ptrs);
  }
}

template <class A, int KSH> hipError_t launch_fwd_mul_impl(const MulArgs &ma)
{
  if(ma.nlimbs > kMaxLimbs) return hipErrorInvalidValue;
  if(ma.ptrs && !ma.one_pass && !ma.team_ctl && ma.logn > (uint32_t)kFusedMax) return hipErrorNotSupported;
  if(ma.one_pass) return launch_onepass_mul<A, KSH>(ma);
  if(ma.team_ctl) return launch_team_mul<A, KSH>(ma);
  if(ma.logn > (uint32_t)kFusedMax) {
    if(ma.block_log == (uint32_t)kFusedSmallBlock) return launch_fwd_mul_blocks<A, kFusedSmallBlock, KSH>(ma);
    if(ma.block_log == (uint32_t)kFusedLarge) return launch_fwd_mul_blocks<A, kFusedLarge, KSH>(ma);
    return hipErrorInvalidValue;
  }
  return with_int<6, 14>((int)ma.logn, hipErrorNotSupported, [&](auto ln) { return launch_fwd_mul_blocks<A, decltype(ln)::value, KSH>(ma); });
}

/* launch_pass<A, KSH>: pa.fused and pa.r pick the launcher */
template <class A, int KSH> hipError_t launch_pass_impl(const PassArgs &pa)
{
  return with_bools([&](auto inverse) -> hipError_t {
    constexpr bool INV = decltype(inverse)::value;
    if(pa.fused == 4) return launch_onepass<A, INV, KSH>(pa);
    if(pa.fused == 3) return with_int<3, 5>(pa.r, hipErrorInvalidValue, [&](auto lead) { return launch_team<A, decltype(lead)::value, INV, KSH>(pa); });
    if(pa.fused == 2) return with_int<1, 3>(pa.r, hipErrorInvalidValue, [&](auto lead) { return launch_twophase<A, decltype(lead)::value, INV, KSH>(pa); });
    if(pa.fused) return with_int<6, 14>(pa.r, hipErrorInvalidValue, [&](auto ln) { return launch_fused<A, decltype(ln)::value, INV, KSH>(pa); });
    return with_int<1, 4>(pa.r, hipErrorInvalidValue, [&](auto r) { return launch_column<A, decltype(r)::value, INV, KSH>(pa); });
  }, pa.inverse);
}

/* the radix-4 formulation (ArithU64R4): block passes, and column passes of one or two radix-4 levels before (forward) or
 * after (inverse) them (ntt_passplan.h: make_passes_r4) */
template <class A, int KSH> hipError_t launch_pass_radix4_impl(const PassArgs &pa)
{
  return with_bools([&](auto inverse) -> hipError_t {
    constexpr bool INV = decltype(inverse)::value;
    if(pa.fused == 1) return with_int<6, 14>(pa.r, hipErrorInvalidValue, [&](auto ln) { return launch_fused<A, decltype(ln)::value, INV, KSH>(pa); });
    if(pa.fused || pa.s != 0) return hipErrorInvalidValue;
    if(pa.r == 2) return launch_column<A, 2, INV, KSH>(pa);
    if(pa.r == 4) return launch_column<A, 4, INV, KSH>(pa);
    return hipErrorInvalidValue;
  }, pa.inverse);
}

/* each instantiating .hip file expands the macros of its policy and class once */
#define NTT_DEFINE_LAUNCH_PASS(A, KSH) \
  template <> hipError_t launch_pass<A, KSH>(const PassArgs &pa) { return launch_pass_impl<A, KSH>(pa); }
#define NTT_DEFINE_LAUNCH_PASS_RADIX4(A, KSH) \
  template <> hipError_t launch_pass<A, KSH>(const PassArgs &pa) { return launch_pass_radix4_impl<A, KSH>(pa); }

#define NTT_DEFINE_LAUNCH_FWD_MUL(A, KSH) \
  template <> hipError_t launch_fwd_mul<A, KSH>(const MulArgs &ma) { return launch_fwd_mul_impl<A, KSH>(ma); }

#define NTT_DEFINE_LAUNCH_DOT(A, KSH) \
  template <> hipError_t launch_dot<A, KSH>(const DotArgs &da) { return launch_dot_impl<A, KSH>(da); }

#define NTT_DEFINE_LAUNCH_PRODUCT(A, KSH) \
  template <> hipError_t launch_product<A, KSH>(const ProdArgs &pa) { return launch_product_impl<A, KSH>(pa); }
/* (a translation unit of its own per policy: inst_team_*.hip) */
#define NTT_DEFINE_LAUNCH_TEAM_PRODUCT(A, KSH) \
  template <> hipError_t launch_team_product<A, KSH>(const ProdArgs &pa) { return launch_team_product_impl<A, KSH>(pa); }

} /* namespace ntt */
