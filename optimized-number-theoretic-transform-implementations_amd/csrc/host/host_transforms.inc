/* host/host_transforms.inc -- batched transforms: dispatch over policies and classes, what every route shares (launch records, the XCD-local decision, the chunk walk), the launch choice (one pass / XCD-local / two-phase / per-pass chunks), the ntt_*_batch entry points.
 * A section of ntt_host.hip (one translation unit, included from there in order); not compiled by itself. */

/* ------------------------------------------------------------------ */
/* transforms                                                          */
/* ------------------------------------------------------------------ */
/* A launch over several limbs runs ONE kernel instantiation: the coarsest headroom class among the limbs of the run (a coarser
 * class is valid for every modulus a finer one serves: it only reduces / folds more often).  rns_for_runs sets the override
 * around the run's call; every class dispatch below goes through these two. */
static thread_local int t_run_kcls = INT_MIN, t_run_int_cls = INT_MIN;
static int eff_kcls(const ntt_plan *p) { return (t_run_kcls != INT_MIN && p->kcls != kWideClass) ? t_run_kcls : p->kcls; }
static int eff_int_cls(const ntt_plan *p) { return (t_run_int_cls != INT_MIN && p->int_cls >= 0) ? t_run_int_cls : p->int_cls; }

/* The plan's radix-2 policy and (effective) headroom class as the template arguments of a launcher: f(KernelClass<A, KSH>{}) for the eight
 * pairs every launcher of a plain transform or an NTT-domain product is built for (with_f64_class: the FP64 half by itself).  The
 * radix-4 policy is not among them: only launch_pass has it (dispatch_pass). */
template <class F> static hipError_t with_class(const ntt_plan *p, F &&f)
{
  if(p->arith != NTT_ARITH_U64) return with_f64_class(eff_kcls(p), f);
  switch(eff_int_cls(p)) { /* (same tables; the wide policy's stages around its Barrett products) */
    case 3: return f(KernelClass<ArithU64X<3>, 3>{});
    case 1: return f(KernelClass<ArithU64X<1>, 1>{});
    case 0: return f(KernelClass<ArithU64X<0>, 0>{});
    default: return f(KernelClass<ArithU64, 0>{});
  }
}

static hipError_t dispatch_pass(const ntt_plan *p, const PassArgs &pa)
{
  /* (generic = the column-pass cross-check path: the reference's butterflies) */
  if(p->arith == NTT_ARITH_U64 && p->generic) return launch_pass<ArithU64, 0>(pa);
  if(p->arith == NTT_ARITH_U64_R4) return launch_pass<ArithU64R4, 0>(pa);
  return with_class(p, [&](auto k) { return launch_pass<typename decltype(k)::A, decltype(k)::KSH>(pa); });
}

/* Where the XCD-local one-launch kernels (team_kernel and its product forms) are built: the FP64 policies and the wide integer policy,
 * N = 2^15..2^17, from 64 polynomials of the launch on (the eight queues) */
static bool team_window(const ntt_plan *p, uint64_t polys)
{
  const bool int_wide = p->arith == NTT_ARITH_U64 && p->int_cls >= 0;
  return (p->arith == NTT_ARITH_F64 || int_wide) && p->m >= kTeamBlock + 3 && p->m <= kTeamBlock + 5 && polys >= 64 && polys < (1ull << 29);
}

/* The one-launch form or the per-chunk launches, for the NTT-domain products: inside the window NTT_OPT_XCD_LOCAL 1 / 0 forces either,
 * the automatic choice (-1) is the route's own measured rule `pays` */
template <class Pays> static bool team_pays(const ntt_plan *p, uint64_t polys, int nlimbs, Pays pays)
{
  if(!team_window(p, polys) || p->block_log || nlimbs > kMaxLimbs) return false;
  return p->xcd_local >= 0 ? p->xcd_local == 1 : pays();
}

/* XCD-local two-pass launches: FP64 policies and the wide integer policy, N = 2^15..2^17, plain calls (canonical in,
 * canonical out).  Automatic choice (-1), as measured (profiles/r03/sweep_xcd_local.txt, profiles/r04/ab_xcd_*.txt): the
 * FORWARD transform of a batch that keeps all eight queues busy for several lags (+8..14 % over one launch per pass; wide
 * integer policy +18..23 %); the inverse only at 2^17 (+3..5 %, integer +15 %) -- at 2^15 and 2^16 its first pass is the
 * heavy one and the column items wait longer than the L2 can hold their polynomials: per-pass launches there.
 * NTT_OPT_XCD_LOCAL 1 forces the path wherever it is built (batch >= 64), 0 disables it. */
/* nlimbs > 1: the limbs of an RNS set in ONE launch (the queues run over all limbs' polynomials): `batch` is per limb */
static bool team_applies(const ntt_plan *p, uint64_t batch, bool inverse, bool wide, bool lazy, int nlimbs, bool product = false)
{
  if(nlimbs < 1 || nlimbs > kMaxLimbs) return false;
  batch *= (uint64_t)nlimbs; /* polynomials of the launch */
  /* the FP64 policies; transforms (not the product launch) also for the wide integer policy */
  const bool int_wide = p->arith == NTT_ARITH_U64 && p->int_cls >= 0 && !product;
  if(!team_window(p, batch) || (p->arith != NTT_ARITH_F64 && !int_wide) || p->generic || wide || lazy) return false;
  const int on = p->xcd_local;
  if(on >= 0) return on == 1;
  /* the wide integer policy (profiles/r04/ab_xcd_int.txt): forward +18..23 % at all three sizes; inverse +15 % at 2^17, none at
   * 2^16, -14 % at 2^15 */
  if(int_wide) return batch >= 512 && (!inverse || p->m == kTeamBlock + 5);
  /* FP64 inverse (profiles/r04/ab_xcd_f64_inv.txt): slower at 2^15 and 2^16 (-21 %, -12 %), +2.6..5.5 % at 2^17 */
  if(inverse) return p->m == kTeamBlock + 5 && batch >= 512;
  /* the product launch (all transforms of a product as items of one launch) pays from 2^23 coefficients per operand on:
   * 64 / 128 / 256 polynomials at 2^17 / 2^16 / 2^15 (measured against the per-chunk launches, single limb, batches
   * 64..384: profiles/r03/ablations.txt (h)) */
  if(product) return batch >= 64 && (batch << p->m) >= (1ull << 23);
  return !inverse && batch >= 512;
}

/* The stream's control block, at least sizeof(TeamCtl) + batch counters.
 * A (plan, stream) pair owns TWO blocks, both allocated by the first direct (uncaptured) call: one for direct launches
 * and one for launches captured into HIP graphs.  A captured launch bakes the block's address into its clearing-kernel and kernel
 * nodes, so the graph block is never freed or regrown while the plan lives, and direct launches never touch it: a graph
 * replayed on another stream cannot collide with direct calls on the capture stream.  (Two graphs captured on the same
 * plan and stream share the graph block: replay them one after the other, not concurrently -- INTEGRATION.md.)
 * Nothing here synchronises the device: an outgrown direct block is retired, not freed (launches still queued may be
 * using it), and released with the plan.  While capturing nothing is allocated (not capturable): without a graph block of
 * sufficient size *out stays null and the caller takes the per-pass launches. */
static int team_buffer(const ntt_plan *p, void *stream, uint64_t batch, void **out)
{
  std::lock_guard<std::mutex> lock(p->team_mu);
  /* (batch_hint is written by ntt_plan_set_option under the same mutex) */
  const size_t need = sizeof(TeamCtl) + (size_t)(batch > 2 * p->batch_hint ? batch : 2 * p->batch_hint) * sizeof(unsigned);
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  /* a query that fails (the legacy stream asked during a global-mode capture) counts as capturing: allocating would invalidate it */
  const bool capturing = hipStreamIsCapturing((hipStream_t)stream, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone;
  *out = nullptr;
  ntt_plan::TeamBuf *tb = nullptr;
  for(ntt_plan::TeamBuf &t : p->team_bufs) {
    if(t.stream == stream) tb = &t;
  }
  if(capturing) {
    if(tb && tb->g && tb->gbytes >= need) *out = tb->g;
    return NTT_OK;
  }
  if(!tb) {
    p->team_bufs.push_back(ntt_plan::TeamBuf{stream, nullptr, 0, nullptr, 0});
    tb = &p->team_bufs.back();
  }
  if(tb->bytes < need) {
    /* a reserved size is taken as given, an outgrown one doubled */
    const size_t grow = p->batch_hint && !tb->d ? need : need * 2;
    void *d = nullptr;
    HIP_TRY(hipMalloc(&d, grow));
    p->ctl_allocs++;
    if(tb->d) p->team_retired.push_back(tb->d);
    tb->d     = d;
    tb->bytes = grow;
  }
  if(tb->gbytes < tb->bytes) {
    /* the graph block follows the direct block's size (first direct call, a larger direct call, ntt_plan_reserve): graphs
     * captured so far keep the address baked into their nodes -- the old block is retired, not freed -- and captures from now on
     * get the larger one.  (Rounds 3-5 sized it once: a larger ntt_plan_reserve before a capture silently left the captured call on
     * the per-pass launches.) */
    void *g = nullptr;
    HIP_TRY(hipMalloc(&g, tb->bytes));
    p->ctl_allocs++;
    if(tb->g) p->team_retired.push_back(tb->g);
    tb->g      = g;
    tb->gbytes = tb->bytes;
  }
  *out = tb->d;
  return NTT_OK;
}

/* Sizes the (plan, stream) control blocks for calls of up to `polys` polynomials x limbs (products count their operands:
 * twice that many entries) -- the allocation an XCD-local launch would otherwise make on its first call, an implicit device
 * synchronisation inside a call documented as asynchronous.  Not while the stream is being captured. */
extern "C" int ntt_plan_reserve(const ntt_plan *p, void *stream, uint64_t polys)
{
  if(!p) return fail(NTT_ERR_ARG, "null plan");
  if(polys == 0) return NTT_OK;
  USE_DEVICE(p->device);
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if(hipStreamIsCapturing((hipStream_t)stream, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone)
    return fail(NTT_ERR_ARG, "reserve before the capture begins");
  void *ctl = nullptr;
  return team_buffer(p, stream, 2 * polys, &ctl);
}

/* The limbs one launch serves: the plan's own record (every ordinary call), or an RNS set's records (host array, copied
 * into the kernel arguments) with the word distance between the limbs' slabs ([limb][batch][N]). */
struct LimbSet {
  const void *d;
  int         n;
  uint64_t    stride;  /* words between consecutive limbs of one polynomial */
  uint64_t    pstride; /* words between consecutive polynomials of one limb; 0 = dense (N) */
  const uint64_t *ptab = nullptr; /* pointer batch: DEVICE table, entry i = address of polynomial i's limb 0 (the data pointer of the call is
                                   * then the limb offset alone: null + limb * stride words); pstride is then only a hint of the typical
                                   * spacing (queue numbering of the XCD-local launches) */
};
/* (pointer + words) that is also defined for the null base of a pointer batch */
static uint64_t *advance(uint64_t *base, uint64_t words) { return reinterpret_cast<uint64_t *>(reinterpret_cast<uintptr_t>(base) + 8u * (uintptr_t)words); }
/* the words between consecutive polynomials of a limb */
static uint64_t poly_words(const ntt_plan *p, const LimbSet &ls) { return ls.pstride ? ls.pstride : p->N; }

/* ---- launch records (PassArgs, ProdArgs, DotArgs, MulArgs: ntt_kernels_launch.h) ----
 * What every route sets goes by the same member names in all four: launch_common fills it.  Each kind has ONE builder (launch_one_pass
 * here, prod_args, dot_args, mul_args beside their routes) that starts from a zeroed record, calls it and adds the kind's operands; a
 * route then sets only what distinguishes it -- with set_team / set_ptrs, or a plain assignment (block_log, oversub). */
template <class Args> static void launch_common(Args &x, const ntt_plan *p, const LimbSet &ls, uint64_t batch, void *stream)
{
  x.limbs       = ls.d;
  x.nlimbs      = ls.n;
  x.limb_stride = ls.stride;
  x.poly_stride = ls.pstride;
  x.batch       = batch;
  x.logn        = (uint32_t)p->m;
  x.max_grid    = p->max_grid;
  x.num_cus     = p->num_cus;
  x.stream      = (hipStream_t)stream;
}
/* the XCD-local one-launch form: the stream's control block, `lag` polynomials between the passes of a queue unless NTT_OPT_XCD_LOCAL_LAG
 * says otherwise, and -- the records that name a block size -- the team kernels' 2^12-point blocks */
template <class Args> static void set_team(Args &x, const ntt_plan *p, void *ctl, int lag)
{
  x.team_ctl = ctl;
  x.team_lag = p->team_lag ? p->team_lag : lag;
  x.team_wpc = p->team_wpc;
  if constexpr(std::is_same_v<Args, DotArgs> || std::is_same_v<Args, MulArgs>) x.block_log = (uint32_t)kTeamBlock;
}
/* a pointer batch: the record's operand pointers are DEVICE tables of polynomial addresses, this launch's (first) limb limb_off words
 * behind every entry */
template <class Args> static void set_ptrs(Args &x, uint64_t limb_off)
{
  x.ptrs         = 1;
  x.ptr_limb_off = limb_off;
}
/* a table where a record has an operand pointer */
static uint64_t *as_words(const void *table) { return const_cast<uint64_t *>(static_cast<const uint64_t *>(table)); }

/* One pass of a transform -- or a whole transform as one launch (ps.fused 2, 3, 4: PassArgs) -- on nb polynomials starting at d.
 * team_ctl: the XCD-local launch's control block, with its lag. */
static int launch_one_pass(const ntt_plan *p, const Pass &ps, uint64_t *d, uint64_t nb, bool inverse, bool wide, bool lazy,
                           bool ends, void *stream, const LimbSet &ls, bool oversub = true, void *team_ctl = nullptr, int team_lag = 0)
{
  PassArgs pa{};
  launch_common(pa, p, ls, nb, stream);
  pa.a       = d;
  pa.ptab    = ls.ptab; /* (a set with a table only ever reaches run_transform: null on the products' column passes, as ever) */
  pa.fused   = ps.fused;
  pa.r       = ps.r;
  pa.s       = ps.s;
  pa.inverse = inverse;
  pa.wide    = wide;
  pa.lastinv = inverse && ps.s == 0;
  pa.lazy    = lazy;
  pa.ends    = ends;
  if(oversub) pa.oversub = p->block_oversub;
  if(team_ctl) set_team(pa, p, team_ctl, team_lag);
  return launched(dispatch_pass(p, pa));
}

/* Multi-pass routes (N > 2^14) run chunk by chunk so that what one pass writes is still in the 256 MiB Infinity Cache when
 * the next pass reads it: only the first read and the last write of a chunk have to reach HBM.  A chunk of `mib` MiB holds
 * that many polynomials of EVERY limb; fn(first, nb, off): nb polynomials from the first-th on, off words into every operand. */
template <class Fn> static int for_chunks(const ntt_plan *p, const LimbSet &ls, uint64_t batch, uint64_t mib, int npasses, Fn fn)
{
  uint64_t chunk = batch;
  if(npasses > 1) {
    chunk = (mib << 20) / (p->N * sizeof(uint64_t) * (uint64_t)ls.n);
    if(chunk < 1) chunk = 1;
    if(chunk > batch) chunk = batch;
  }
  for(uint64_t first = 0; first < batch; first += chunk) {
    const int rc = fn(first, batch - first < chunk ? batch - first : chunk, first * poly_words(p, ls));
    if(rc) return rc;
  }
  return NTT_OK;
}

static int run_transform(const ntt_plan *p, uint64_t *d_a, uint64_t batch, bool inverse, bool wide, void *stream,
                         bool lazy = false, const LimbSet *set = nullptr)
{
  if(!p || (!d_a && batch && !(set && set->ptab))) return fail(NTT_ERR_ARG, "null argument");
  if(batch == 0) return NTT_OK;
  if(inverse ? !p->has_inv : !p->has_fwd) return fail(NTT_ERR_ARG, "plan lacks the table for this direction");
  USE_DEVICE(p->device);
  const LimbSet ls = set ? *set : LimbSet{p->limbrec.data(), 1, 0, 0};
  const PassList L = p->arith == NTT_ARITH_U64_R4
                         ? make_passes_r4(p->m)
                         : make_passes(p->m, p->generic, p->block_log ? p->block_log : multi_pass_block(p->m, inverse, p->arith == NTT_ARITH_F64));
  /* N = 2^15, FP64 policies: ONE pass -- a workgroup holds the whole polynomial in its registers, every coefficient crosses HBM
   * twice (ntt_kernels_block.h: onepass_kernel; measured against the two-pass forms in profiles/r06/onepass_2p15.txt).  One workgroup
   * per CU and polynomial: the automatic choice wants a polynomial for every second CU -- measured crossover (profiles/r06/
   * onepass_small_batches.txt): 64..96 polynomials even, 128 +11 % forward, 192 +11 / +7 %, 255 +25 / +20 %; 32 polynomials -40 % --;
   * smaller batches spread over the chip as 2^12-point blocks through the per-pass launches.  A call that asks for lazy outputs gets this
   * kernel's canonical words: they satisfy the lazy contract ([0,4q) forward, [0,2q) inverse), and one pass with the final reduction
   * beats two passes without it (the record's lazy stays 0; so does its oversub). */
  if(p->m == kFusedMax + 1 && p->arith == NTT_ARITH_F64 && !p->generic && ls.n <= kMaxLimbs &&
     one_pass_pays(p, batch * (uint64_t)ls.n)) {
    return launch_one_pass(p, Pass{4, 1, 0}, d_a, batch, inverse, wide, /* lazy */ false, /* ends */ true, stream, ls, /* oversub */ false);
  }
  /* both passes as items of ONE launch with the intermediate kept in each XCD's L2 (ntt_kernels_team.h: team_kernel) */
  void *ctl = nullptr;
  if(team_applies(p, batch, inverse, wide, lazy, ls.n)) {
    /* the queue heads and counters live in a buffer the plan keeps per stream; it is allocated on first use -- except
     * while the stream is being captured into a HIP graph (allocation is not capturable): the call then takes the
     * per-pass launches, which need no memory of their own */
    int rc = team_buffer(p, stream, batch * (uint64_t)ls.n, &ctl);
    if(rc) return rc;
  }
  if(ctl) {
    /* polynomials between the two passes of a queue.  The L2 keeps the intermediate while lag x polynomial size stays
     * below about 2.5 MiB (measured, FETCH_SIZE 1.0x the data: 2^15 up to lag 10, 2^16 up to 5, 2^17 not even at 2;
     * profiles/r03/team_kernel_l2_retention.txt), but with four workgroups per CU a lag below 8 makes second-pass items
     * wait: 2^15 gets both (lag 10: 0.43 of the roofline against 0.40-0.41 beyond), 2^16 and 2^17 run fastest at 8-10
     * with the second pass served by the Infinity Cache (profiles/r03/sweep_xcd_local_lag.txt) */
    const int lag = p->m == kTeamBlock + 4 ? 8 : 10;
    /* (team_applies: canonical in, canonical out) */
    return launch_one_pass(p, Pass{3, p->m - kTeamBlock, 0}, d_a, batch, inverse, /* wide */ false, /* lazy */ false, /* ends */ true, stream, ls,
                           /* oversub */ true, ctl, lag);
  }
  /* the one-launch two-phase kernel owns a CU per polynomial: it only pays when the batch fills the chip (measured +3 % at
   * batch ~30k; a batch below the CU count would leave CUs idle where the per-pass launches spread one polynomial
   * over 16 workgroups) -- the automatic choice is gated on that, an explicit NTT_OPT_TWO_PHASE 1 is honoured as given */
  const bool tp_auto = p->two_phase < 0 && !inverse && p->m == kFusedMax + 2 && p->kcls != kWideClass &&
                       batch >= 2ull * (uint64_t)p->num_cus;
  if((p->two_phase == 1 || tp_auto) && ls.n == 1 && !p->generic && p->arith == NTT_ARITH_F64 && p->m >= kFusedMax + 2 &&
     p->m <= kFusedMax + 3) {
    /* one launch, one workgroup per polynomial, both passes back to back (ntt_kernels_block.h: twophase_kernel) */
    return launch_one_pass(p, Pass{2, p->m - kFusedMax, 0}, d_a, batch, inverse, wide, lazy, /* ends */ true, stream, ls);
  }
  return for_chunks(p, ls, batch, (uint64_t)p->chunk_mib, L.n, [&](uint64_t first, uint64_t nb, uint64_t off) -> int {
    /* a chunk starts `first` polynomials in: that many strides -- or table entries, the data pointer unmoved -- further */
    LimbSet cs = ls;
    if(ls.ptab) cs.ptab = ls.ptab + first;
    uint64_t *const d = ls.ptab ? d_a : d_a + off;
    for(int k = 0; k < L.n; k++) {
      const Pass &ps = L.p[inverse ? L.n - 1 - k : k];
      /* (radix-4 inverse: a pass that does not end the transform multiplies by 1, not by N^-1) */
      cs.d = p->arith == NTT_ARITH_U64_R4 && inverse && ps.s != 0 ? (const void *)p->limbrec_mid.data() : ls.d;
      const int rc = launch_one_pass(p, ps, d, nb, inverse, wide && k == 0, lazy, k == L.n - 1, stream, cs);
      if(rc) return rc;
    }
    return NTT_OK;
  });
}

extern "C" int ntt_fwd_batch(const ntt_plan *p, uint64_t *d_a, uint64_t batch, void *stream)
{
  return run_transform(p, d_a, batch, false, false, stream);
}
extern "C" int ntt_inv_batch(const ntt_plan *p, uint64_t *d_a, uint64_t batch, void *stream)
{
  return run_transform(p, d_a, batch, true, false, stream);
}
extern "C" int ntt_transform_batch(const ntt_plan *p, uint64_t *d_a, uint64_t batch, unsigned flags, void *stream)
{
  if(flags & ~(unsigned)(NTT_FLAG_INVERSE | NTT_FLAG_WIDE_IN | NTT_FLAG_LAZY_OUT)) return fail(NTT_ERR_ARG, "unknown flag");
  return run_transform(p, d_a, batch, (flags & NTT_FLAG_INVERSE) != 0, (flags & NTT_FLAG_WIDE_IN) != 0, stream,
                       (flags & NTT_FLAG_LAZY_OUT) != 0);
}
extern "C" int ntt_fwd_batch_lazy(const ntt_plan *p, uint64_t *d_a, uint64_t batch, void *stream)
{
  return run_transform(p, d_a, batch, false, false, stream, true);
}
extern "C" int ntt_inv_batch_lazy(const ntt_plan *p, uint64_t *d_a, uint64_t batch, void *stream)
{
  return run_transform(p, d_a, batch, true, false, stream, true);
}
extern "C" int ntt_fwd_batch_wide(const ntt_plan *p, uint64_t *d_a, uint64_t batch, void *stream)
{
  return run_transform(p, d_a, batch, false, true, stream);
}
extern "C" int ntt_inv_batch_wide(const ntt_plan *p, uint64_t *d_a, uint64_t batch, void *stream)
{
  return run_transform(p, d_a, batch, true, true, stream);
}
