/* host/host_sample.inc -- random polynomials in the RNS drawn on the device: ntt_rns_sample_batch and its strided form.  A section of
 * ntt_host.hip (one translation unit, included from there in order); not compiled by itself.  The kernels are in sample.hip and the
 * sample_f64*.hip units; this section sees their launchers and argument records only (ntt_sample.h, which states the generator and the
 * three kinds -- a statistical generator, not a cryptographic one).
 *
 *   coefficients   sample_coef_kernel, one launch per 16 limbs: 8NL bytes, 16NL accumulating; integer arithmetic of its own for every
 *                  policy and every N >= 2.  The uniform kind always takes it (uniform is uniform in either domain).
 *   NTT domain     (small kinds) per run of compatible limbs (rns_runs):
 *                  fused        FP64 policies at N = 2^6..2^14, where NTT_OPT_SAMPLE_FUSED on plans[0] allows it: ONE sample_fwd_kernel
 *                               launch, 8NL bytes (16NL accumulating);
 *                  composition  anything else (integer or radix-4 plans, N < 2^6, N >= 2^15, NTT_OPT_SAMPLE_FUSED 0): sample_coef_kernel
 *                               and the forward transform over the run in place; accumulating, the inverse transform over the run
 *                               first (c is canonical on both sides of every step, so the words are those of the fused kernel).
 * Everything is checked before the first launch.  Nothing is allocated, the host is not synchronised and no memset is issued: the calls
 * can be captured into a graph. */

/* where the fused kernel is built */
static bool sample_fused_built(const ntt_plan *p) { return p->arith == NTT_ARITH_F64 && !p->generic && p->m >= kFusedMin && p->m <= kFusedMax; }

/* The automatic choice (NTT_OPT_SAMPLE_FUSED -1), from profiles/r23/sample_bench.txt (a): the first L of 24 50-bit primes, 2^13 and 2^14,
 * L = 1, 4, 16, 64 and 1024 polynomials, both small kinds, composition time / fused time as ranges over five rounds of fresh processes; a
 * figure's own spread over the rounds is 1.00-1.08.  The fused kernel is the default where it is not slower at both batch sizes:
 *   accumulating    every kind, every shape: 1.46-2.34 (the composition pays an inverse and a forward transform).  Fused.
 *   storing         L = 4 and 16: 1.05-1.38 in 14 of the 16 rows, 0.98-1.02 (not different) in the two at (2^14, L = 16, 64 polynomials).  Fused.
 *                   L = 1: 1.41-1.53 at 1024 polynomials and 1.09-1.14 at (2^14, 64), but 0.94-0.97 at (2^13, 64): 64 workgroups on
 *                   256 CUs, where the fused kernel's long prologue (ten Philox rounds for each of a thread's 16 coefficients, ahead of
 *                   the stages) is not hidden by other workgroups and the composition's two short launches take 21.1 against 21.8-22.4
 *                   us.  Composition for a single-limb run through 2^13 (smaller sizes follow 2^13: not measured).
 * Recomputing the Philox block in every limb's workgroup does not cost the fused kernel its lead: the saved 16N bytes per limb-polynomial
 * pay for it in 20 of the 24 storing rows, two are not different and two lose 3-6 %.  It runs at 0.14-0.28 of ntt_copy_probe's rate at its algorithmic bytes storing and 0.27-0.49
 * accumulating (the coefficient kernel: 0.28-0.93 for the small kinds, 0.23-0.74 uniform -- one block per word written when L = 1, one
 * per limb for the uniform kind): its prologue's integer work is not hidden behind the stages, as in lift_fwd_kernel, and it is untuned.
 * Against the detour the parent commit can express ((b): the small values drawn with torch on the device, then ntt_rns_from_plain_batch
 * with the same flags) the fused kernel takes 1/1.11-1/2.43 of the time for ternary values and 1/2.27-1/20.4 for the centred binomial. */
static bool sample_fused_applies(const ntt_plan *p0, const ntt_plan *p, int run_limbs, bool acc)
{
  if(!sample_fused_built(p)) return false;
  if(p0->sample_fused >= 0) return p0->sample_fused == 1;
  return acc || run_limbs > 1 || p->m > 13;
}

/* limb q's constants: Barrett words and [mult]_q with its Shoup word */
static SampleLimb sample_limb(uint64_t q, uint64_t mult)
{
  SampleLimb l = bconv_dst(q);
  l.s          = mult % q;
  l.s_shoup    = shoup_of(l.s, q);
  return l;
}

static SampleCall sample_call_at(const SampleCall &call, int first)
{
  SampleCall c = call;
  c.limb0      = (uint32_t)first;
  return c;
}

static int sample_coef_launch(ntt_plan *const *plans, int first, int n, uint64_t *d_c, const SampleCall &call, const SampleLimb *ll,
                              uint64_t batch, void *stream, const Layout &lay)
{
  SampleCoefArgs sa{};
  sa.c           = d_c + (uint64_t)first * lay.limb;
  sa.limb_stride = lay.limb;
  sa.poly_stride = lay.poly;
  sa.batch       = batch;
  sa.logn        = (uint32_t)plans[0]->m;
  sa.nlimbs      = n;
  sa.call        = sample_call_at(call, first);
  for(int i = 0; i < n; i++) sa.limbs[i] = ll[first + i];
  sa.max_grid = plans[0]->max_grid;
  sa.stream   = (hipStream_t)stream;
  const hipError_t e = launch_sample_coef(sa);
  if(e != hipSuccess) return fail(NTT_ERR_HIP, std::string("sample_coef_kernel: ") + hipGetErrorString(e));
  return NTT_OK;
}

static int sample_fwd_launch(ntt_plan *const *plans, int first, int n, uint64_t *d_c, const SampleCall &call, const SampleLimb *ll,
                             uint64_t batch, void *stream, const Layout &lay)
{
  const std::vector<unsigned char> recs = rns_records(plans, first, n);
  SampleFwdArgs                    sa{};
  sa.c           = d_c + (uint64_t)first * lay.limb;
  sa.limbs       = recs.data();
  sa.nlimbs      = n;
  sa.limb_stride = lay.limb;
  sa.poly_stride = lay.poly;
  sa.batch       = batch;
  sa.logn        = (uint32_t)plans[first]->m;
  sa.call        = sample_call_at(call, first);
  for(int i = 0; i < n; i++) sa.ll[i] = ll[first + i];
  sa.max_grid = plans[first]->max_grid;
  sa.num_cus  = plans[first]->num_cus;
  sa.stream   = (hipStream_t)stream;
  const hipError_t e = with_f64_class(run_class(plans, first, n), [&](auto k) { return launch_sample_fwd<typename decltype(k)::A, decltype(k)::KSH>(sa); });
  if(e != hipSuccess) return fail(NTT_ERR_HIP, std::string("sample_fwd_kernel: ") + hipGetErrorString(e));
  return NTT_OK;
}

static int rns_sample(int nlimbs, ntt_plan *const *plans, uint64_t *d_c, int kind, uint64_t mult, uint64_t seed, uint64_t first_poly,
                      uint64_t batch, unsigned flags, void *stream, const Layout &lay)
{
  if(flags & ~(unsigned)(NTT_SAMPLE_TRANSFORMED | NTT_SAMPLE_ACCUMULATE)) return fail(NTT_ERR_ARG, "unknown flag");
  if(kind != NTT_SAMPLE_TERNARY && kind != NTT_SAMPLE_CBD21 && kind != NTT_SAMPLE_UNIFORM) return fail(NTT_ERR_ARG, "sample: unknown kind");
  if(mult < 1 || mult >= (1ull << 61)) return fail(NTT_ERR_ARG, "sample: the multiplier must satisfy 1 <= mult < 2^61");
  if(kind == NTT_SAMPLE_UNIFORM && mult != 1) return fail(NTT_ERR_ARG, "sample: the uniform kind takes mult = 1");
  int rc = rns_check(nlimbs, plans);
  if(rc) return rc;
  if(plans[0]->m < 1 || plans[0]->m > 30) return fail(NTT_ERR_ARG, "sample: N out of range");
  for(int l = 0; l < nlimbs; l++) {
    if(plans[l]->q >= (1ull << 61)) return fail(NTT_ERR_ARG, "sample: every prime must be below 2^61");
  }
  if(batch > 0 && !d_c) return fail(NTT_ERR_ARG, "null argument");
  const uint64_t N = plans[0]->N;
  rc               = layout_check(N, nlimbs, batch, lay);
  if(rc) return rc;
  const bool ntt_dom = (flags & NTT_SAMPLE_TRANSFORMED) != 0 && kind != NTT_SAMPLE_UNIFORM;
  const bool acc     = (flags & NTT_SAMPLE_ACCUMULATE) != 0;
  const std::vector<std::pair<int, int>> runs = rns_runs(nlimbs, plans);
  if(ntt_dom) {
    /* every table the call will need, before anything is written */
    for(const std::pair<int, int> &run : runs) {
      const bool fused = sample_fused_applies(plans[0], plans[run.first], run.second, acc);
      for(int l = run.first; l < run.first + run.second; l++) {
        if(!plans[l]->has_fwd) return fail(NTT_ERR_ARG, "sample: a limb's plan lacks the forward table");
        if(!fused && acc && !plans[l]->has_inv) return fail(NTT_ERR_ARG, "sample: a limb's plan lacks the inverse table (composed accumulation)");
      }
    }
  }
  if(batch == 0) return NTT_OK;
  SampleCall call{};
  call.kind       = (uint32_t)kind;
  call.accumulate = acc ? 1u : 0u;
  call.key0       = (uint32_t)seed;
  call.key1       = (uint32_t)(seed >> 32);
  call.first_poly = first_poly;
  std::vector<SampleLimb> ll((size_t)nlimbs);
  for(int l = 0; l < nlimbs; l++) ll[(size_t)l] = sample_limb(plans[l]->q, mult);
  USE_DEVICE(plans[0]->device);
  if(!ntt_dom) {
    for(int first = 0; !rc && first < nlimbs; first += kSampleLimbs) {
      rc = sample_coef_launch(plans, first, nlimbs - first < kSampleLimbs ? nlimbs - first : kSampleLimbs, d_c, call, ll.data(), batch, stream, lay);
    }
    return rc;
  }
  const Layout one{lay.limb, lay.poly};
  for(const std::pair<int, int> &run : runs) {
    if(rc) break;
    const int first = run.first, n = run.second;
    if(sample_fused_applies(plans[0], plans[first], n, acc)) {
      rc = sample_fwd_launch(plans, first, n, d_c, call, ll.data(), batch, stream, lay);
      continue;
    }
    uint64_t *c = d_c + (uint64_t)first * lay.limb;
    if(acc) rc = rns_transform(n, plans + first, c, batch, true, stream, one);
    if(!rc) rc = sample_coef_launch(plans, first, n, d_c, call, ll.data(), batch, stream, lay);
    if(!rc) rc = rns_transform(n, plans + first, c, batch, false, stream, one);
  }
  return rc;
}

extern "C" int ntt_rns_sample_batch(int nlimbs, ntt_plan *const *plans, uint64_t *d_c, int kind, uint64_t mult, uint64_t seed,
                                    uint64_t first_poly, uint64_t batch, unsigned flags, void *stream)
{
  return rns_sample(nlimbs, plans, d_c, kind, mult, seed, first_poly, batch, flags, stream, limb_major(plans, nlimbs, batch));
}

extern "C" int ntt_rns_sample_batch_strided(int nlimbs, ntt_plan *const *plans, uint64_t *d_c, int kind, uint64_t mult, uint64_t seed,
                                            uint64_t first_poly, uint64_t c_limb_stride, uint64_t c_poly_stride, uint64_t batch,
                                            unsigned flags, void *stream)
{
  return rns_sample(nlimbs, plans, d_c, kind, mult, seed, first_poly, batch, flags, stream, Layout{c_limb_stride, c_poly_stride});
}
