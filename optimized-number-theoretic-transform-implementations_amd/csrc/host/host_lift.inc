/* host/host_lift.inc -- into the RNS, the first step of an encryption and every plaintext operand: ntt_rns_from_plain_batch,
 * ntt_rns_from_double_batch and their strided forms.  A section of ntt_host.hip (one translation unit, included from there in order); not
 * compiled by itself.  The kernels are in lift.hip and the lift_f64*.hip units; this section sees their launchers and argument records
 * only (ntt_lift.h, which states the arithmetic).
 *
 *   coefficients   lift_coef_kernel, one launch per 16 limbs (the plaintext word read once per launch): 8N(L + 1) bytes, 8N(2L + 1)
 *                  accumulating; integer arithmetic of its own for every policy and every N >= 2.
 *   NTT domain     per run of compatible limbs (rns_runs):
 *                  fused        FP64 policies at N = 2^6..2^14, where NTT_OPT_LIFT_FUSED on plans[0] allows it: ONE lift_fwd_kernel
 *                               launch, 8N + 8NL bytes (16NL accumulating);
 *                  composition  anything else (integer or radix-4 plans, N < 2^6, N >= 2^15, NTT_OPT_LIFT_FUSED 0): lift_coef_kernel and
 *                               the forward transform over the run in place; accumulating, the inverse transform over the run first
 *                               (c is canonical on both sides of every step, so the words are those of the fused kernel).
 * Everything is checked before the first launch.  Nothing is allocated, the host is not synchronised and no memset is issued: the calls
 * can be captured into a graph. */

/* where the fused kernel is built */
static bool lift_fused_built(const ntt_plan *p) { return p->arith == NTT_ARITH_F64 && !p->generic && p->m >= kFusedMin && p->m <= kFusedMax; }

/* The automatic choice (NTT_OPT_LIFT_FUSED -1), from profiles/r19/lift_bench.txt (a): 50-bit primes, t = 65537, 2^13 and 2^14, L = 1, 4, 16,
 * 64 and 1024 polynomials, composition time / fused time as ranges over five rounds of alternating processes; a figure's own spread over
 * the rounds is 1.00-1.07.  The fused kernel is the default where it is not slower by more than that spread at both batch sizes:
 *   accumulating    every mode, every shape: 1.13-2.27 (centred 1.52-2.27, scaled 1.13-1.70, double 1.36-1.97) -- the composition pays an
 *                   inverse and a forward transform.  Fused.
 *   storing, centred  2^13: 1.06-1.37 at every L and both batch sizes.  Fused through 2^13 (smaller sizes follow 2^13: not measured).
 *                   2^14: 1.10-1.40 at 64 polynomials, but 0.91-0.92 (L = 4) and 0.99-1.00 (L = 16) at 1024.  Composition.
 *   storing, scaled   0.73-0.97 in 9 of the 12 shapes (the 128-by-64-bit quotient is redone in every limb's workgroup, the
 *                   composition's element-wise launch forms it once per word).  Composition.
 *   storing, double   0.88-0.94 at (2^13, L = 1, 64), (2^14, L = 4, 1024) and (2^14, L = 16, 1024), 1.00-1.33 elsewhere: the 128-bit
 *                   reduction per limb loses at the large shapes.  Composition.
 * The fused kernel runs at 0.24-0.46 of ntt_copy_probe's rate at its algorithmic bytes at 1024 polynomials (the coefficient kernel: 0.47-0.93): its
 * prologue's integer work is not hidden behind the stages.  That is what the storing rows lose on, and it is untuned. */
static bool lift_fused_applies(const ntt_plan *p0, const ntt_plan *p, uint32_t mode, bool acc)
{
  if(!lift_fused_built(p)) return false;
  if(p0->lift_fused >= 0) return p0->lift_fused == 1;
  return acc || (mode == kLiftCentred && p->m <= 13);
}

/* limb q's constants: Barrett words and the mode's multiplier -- centred [t]_q; scaled [D]_q = -r t^-1 mod q (t D = Q - r, Q = 0 mod q) */
static LiftLimb lift_limb(uint64_t q, uint32_t mode, uint64_t t, uint64_t r)
{
  LiftLimb l = bconv_dst(q);
  if(mode == kLiftCentred) l.s = t % q;
  if(mode == kLiftScaled) {
    const uint64_t x = h_mulmod(r % q, h_powmod(t % q, q - 2, q), q);
    l.s              = x ? q - x : 0;
  }
  l.s_shoup = shoup_of(l.s, q);
  return l;
}

static int lift_coef_launch(ntt_plan *const *plans, int first, int n, uint64_t *d_c, const uint64_t *d_m, const LiftCall &call,
                            const LiftLimb *ll, uint64_t batch, void *stream, const Layout &lay, uint64_t m_poly_stride)
{
  LiftCoefArgs la{};
  la.c             = d_c + (uint64_t)first * lay.limb;
  la.m             = d_m;
  la.limb_stride   = lay.limb;
  la.poly_stride   = lay.poly;
  la.m_poly_stride = m_poly_stride;
  la.batch         = batch;
  la.logn          = (uint32_t)plans[0]->m;
  la.nlimbs        = n;
  la.call          = call;
  for(int i = 0; i < n; i++) la.limbs[i] = ll[first + i];
  la.max_grid = plans[0]->max_grid;
  la.stream   = (hipStream_t)stream;
  const hipError_t e = launch_lift_coef(la);
  if(e != hipSuccess) return fail(NTT_ERR_HIP, std::string("lift_coef_kernel: ") + hipGetErrorString(e));
  return NTT_OK;
}

static int lift_fwd_launch(ntt_plan *const *plans, int first, int n, uint64_t *d_c, const uint64_t *d_m, const LiftCall &call,
                           const LiftLimb *ll, uint64_t batch, void *stream, const Layout &lay, uint64_t m_poly_stride)
{
  const std::vector<unsigned char> recs = rns_records(plans, first, n);
  LiftFwdArgs                      la{};
  la.c             = d_c + (uint64_t)first * lay.limb;
  la.m             = d_m;
  la.limbs         = recs.data();
  la.nlimbs        = n;
  la.limb_stride   = lay.limb;
  la.poly_stride   = lay.poly;
  la.m_poly_stride = m_poly_stride;
  la.batch         = batch;
  la.logn          = (uint32_t)plans[first]->m;
  la.call          = call;
  for(int i = 0; i < n; i++) la.ll[i] = ll[first + i];
  la.max_grid = plans[first]->max_grid;
  la.num_cus  = plans[first]->num_cus;
  la.stream   = (hipStream_t)stream;
  const hipError_t e = with_f64_class(run_class(plans, first, n), [&](auto k) { return launch_lift_fwd<typename decltype(k)::A, decltype(k)::KSH>(la); });
  if(e != hipSuccess) return fail(NTT_ERR_HIP, std::string("lift_fwd_kernel: ") + hipGetErrorString(e));
  return NTT_OK;
}

/* both calls: d_m is the plaintext as words (the double mode's are bit patterns) */
static int rns_lift(int nlimbs, ntt_plan *const *plans, uint64_t *d_c, const uint64_t *d_m, uint32_t mode, uint64_t t, double scale,
                    uint64_t batch, unsigned flags, void *stream, const Layout &lay, uint64_t m_poly_stride)
{
  const unsigned known = NTT_LIFT_TRANSFORMED | NTT_LIFT_ACCUMULATE | (mode == kLiftDouble ? 0u : (unsigned)NTT_LIFT_SCALE);
  if(flags & ~known) return fail(NTT_ERR_ARG, mode == kLiftDouble && (flags & NTT_LIFT_SCALE) ? "from_double: NTT_LIFT_SCALE is from_plain's" : "unknown flag");
  if(mode != kLiftDouble && (t < 2 || t >= (1ull << 61))) return fail(NTT_ERR_ARG, "from_plain: the plaintext modulus must satisfy 2 <= t < 2^61");
  int rc = rns_check(nlimbs, plans);
  if(rc) return rc;
  if(plans[0]->m < 1 || plans[0]->m > 30) return fail(NTT_ERR_ARG, "lift: N out of range");
  if(flags & NTT_LIFT_SCALE) mode = kLiftScaled;
  for(int l = 0; l < nlimbs; l++) {
    if(plans[l]->q >= (1ull << 61)) return fail(NTT_ERR_ARG, "lift: every prime must be below 2^61");
    if(mode == kLiftScaled && t % plans[l]->q == 0) return fail(NTT_ERR_ARG, "from_plain: NTT_LIFT_SCALE needs every prime coprime to t");
  }
  if(batch > 0 && (!d_c || !d_m)) return fail(NTT_ERR_ARG, "null argument");
  const uint64_t N = plans[0]->N;
  rc               = layout_check(N, nlimbs, batch, lay);
  if(rc) return rc;
  if(m_poly_stride < N || m_poly_stride > (1ull << 40)) return fail(NTT_ERR_ARG, "layout: the plaintext's polynomial stride must be N .. 2^40 words");
  const bool ntt_dom = (flags & NTT_LIFT_TRANSFORMED) != 0;
  const bool acc     = (flags & NTT_LIFT_ACCUMULATE) != 0;
  const std::vector<std::pair<int, int>> runs = rns_runs(nlimbs, plans);
  if(ntt_dom) {
    /* every table the call will need, before anything is written */
    for(const std::pair<int, int> &run : runs) {
      const bool fused = lift_fused_applies(plans[0], plans[run.first], mode, acc);
      for(int l = run.first; l < run.first + run.second; l++) {
        if(!plans[l]->has_fwd) return fail(NTT_ERR_ARG, "lift: a limb's plan lacks the forward table");
        if(!fused && acc && !plans[l]->has_inv) return fail(NTT_ERR_ARG, "lift: a limb's plan lacks the inverse table (composed accumulation)");
      }
    }
  }
  if(batch == 0) return NTT_OK;
  /* in the fused route another limb's workgroup may still be reading the plaintext: no overlap at all */
  if(galois_overlap(galois_span(d_m, N, 1, batch, 0, m_poly_stride), galois_span(d_c, N, nlimbs, batch, lay.limb, lay.poly)))
    return fail(NTT_ERR_ARG, "lift: the plaintext overlaps the output");
  LiftCall call{};
  call.mode       = mode;
  call.accumulate = acc ? 1u : 0u;
  call.scale      = scale;
  call.td         = plain_dst(mode == kLiftDouble ? 2 : t, 0);
  if(mode != kLiftDouble) {
    call.half_dn = t / 2;
    call.half_up = t - t / 2;
    uint64_t r   = 1 % t;
    for(int l = 0; l < nlimbs; l++) r = (uint64_t)((unsigned __int128)r * (plans[l]->q % t) % t);
    call.r = r; /* Q mod t */
  }
  std::vector<LiftLimb> ll((size_t)nlimbs);
  for(int l = 0; l < nlimbs; l++) ll[(size_t)l] = lift_limb(plans[l]->q, mode, t, call.r);
  USE_DEVICE(plans[0]->device);
  if(!ntt_dom) {
    for(int first = 0; !rc && first < nlimbs; first += kLiftLimbs) {
      rc = lift_coef_launch(plans, first, nlimbs - first < kLiftLimbs ? nlimbs - first : kLiftLimbs, d_c, d_m, call, ll.data(), batch, stream, lay,
                            m_poly_stride);
    }
    return rc;
  }
  const Layout one{lay.limb, lay.poly};
  for(const std::pair<int, int> &run : runs) {
    if(rc) break;
    const int first = run.first, n = run.second;
    if(lift_fused_applies(plans[0], plans[first], mode, acc)) {
      rc = lift_fwd_launch(plans, first, n, d_c, d_m, call, ll.data(), batch, stream, lay, m_poly_stride);
      continue;
    }
    uint64_t *c = d_c + (uint64_t)first * lay.limb;
    if(acc) rc = rns_transform(n, plans + first, c, batch, true, stream, one);
    if(!rc) rc = lift_coef_launch(plans, first, n, d_c, d_m, call, ll.data(), batch, stream, lay, m_poly_stride);
    if(!rc) rc = rns_transform(n, plans + first, c, batch, false, stream, one);
  }
  return rc;
}

static uint64_t lift_n(int nlimbs, ntt_plan *const *plans) { return (nlimbs > 0 && plans && plans[0]) ? plans[0]->N : 0; }

extern "C" int ntt_rns_from_plain_batch(int nlimbs, ntt_plan *const *plans, uint64_t *d_c, const uint64_t *d_m, uint64_t t, uint64_t batch,
                                        unsigned flags, void *stream)
{
  return rns_lift(nlimbs, plans, d_c, d_m, kLiftCentred, t, 0.0, batch, flags, stream, limb_major(plans, nlimbs, batch), lift_n(nlimbs, plans));
}

extern "C" int ntt_rns_from_plain_batch_strided(int nlimbs, ntt_plan *const *plans, uint64_t *d_c, const uint64_t *d_m, uint64_t t,
                                                uint64_t c_limb_stride, uint64_t c_poly_stride, uint64_t m_poly_stride, uint64_t batch,
                                                unsigned flags, void *stream)
{
  return rns_lift(nlimbs, plans, d_c, d_m, kLiftCentred, t, 0.0, batch, flags, stream, Layout{c_limb_stride, c_poly_stride}, m_poly_stride);
}

extern "C" int ntt_rns_from_double_batch(int nlimbs, ntt_plan *const *plans, uint64_t *d_c, const double *d_y, double scale, uint64_t batch,
                                         unsigned flags, void *stream)
{
  return rns_lift(nlimbs, plans, d_c, reinterpret_cast<const uint64_t *>(d_y), kLiftDouble, 0, scale, batch, flags, stream,
                  limb_major(plans, nlimbs, batch), lift_n(nlimbs, plans));
}

extern "C" int ntt_rns_from_double_batch_strided(int nlimbs, ntt_plan *const *plans, uint64_t *d_c, const double *d_y, double scale,
                                                 uint64_t c_limb_stride, uint64_t c_poly_stride, uint64_t y_poly_stride, uint64_t batch,
                                                 unsigned flags, void *stream)
{
  return rns_lift(nlimbs, plans, d_c, reinterpret_cast<const uint64_t *>(d_y), kLiftDouble, 0, scale, batch, flags, stream,
                  Layout{c_limb_stride, c_poly_stride}, y_poly_stride);
}
