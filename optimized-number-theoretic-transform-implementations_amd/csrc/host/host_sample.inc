/* host/host_sample.inc -- random polynomials in the RNS drawn on the device: ntt_rns_sample_batch and its strided form.  A section of
 * ntt_host.hip (one translation unit, included from there in order); not compiled by itself.  The kernels are in sample.hip and the
 * sample_f64*.hip units; this section sees their launchers and argument records only (ntt_sample.h, which states the generator and the
 * three kinds -- a statistical generator, not a cryptographic one).
 *
 * The route is produce_route (host_produce.inc) with sample_coef_kernel -- 8NL bytes, 16NL accumulating; the uniform kind always takes
 * it (uniform is uniform in either domain) -- and, for the small kinds, sample_fwd_kernel, 8NL bytes (16NL accumulating), where
 * NTT_OPT_SAMPLE_FUSED on plans[0] allows it.  This section keeps the sampler's own checks, the rule of that option and the constants. */

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
  if(!produce_fused_built(p)) return false;
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

static int rns_sample(int nlimbs, ntt_plan *const *plans, uint64_t *d_c, int kind, uint64_t mult, uint64_t seed, uint64_t first_poly,
                      uint64_t batch, unsigned flags, void *stream, const Layout &lay)
{
  if(flags & ~(unsigned)(NTT_SAMPLE_TRANSFORMED | NTT_SAMPLE_ACCUMULATE)) return fail(NTT_ERR_ARG, "unknown flag");
  if(kind != NTT_SAMPLE_TERNARY && kind != NTT_SAMPLE_CBD21 && kind != NTT_SAMPLE_UNIFORM) return fail(NTT_ERR_ARG, "sample: unknown kind");
  if(mult < 1 || mult >= (1ull << 61)) return fail(NTT_ERR_ARG, "sample: the multiplier must satisfy 1 <= mult < 2^61");
  if(kind == NTT_SAMPLE_UNIFORM && mult != 1) return fail(NTT_ERR_ARG, "sample: the uniform kind takes mult = 1");
  const int rc = produce_check("sample", nlimbs, plans, d_c != nullptr, batch, lay, produce_any_limb);
  if(rc) return rc;
  const bool acc = (flags & NTT_SAMPLE_ACCUMULATE) != 0;
  SampleFwdArgs sa{};
  sa.call.kind       = (uint32_t)kind;
  sa.call.accumulate = acc ? 1u : 0u;
  sa.call.key0       = (uint32_t)seed;
  sa.call.key1       = (uint32_t)(seed >> 32);
  sa.call.first_poly = first_poly;
  std::vector<SampleLimb> ll((size_t)nlimbs);
  for(int l = 0; l < nlimbs; l++) ll[(size_t)l] = sample_limb(plans[l]->q, mult);
  /* (the uniform kind is uniform in either domain: always the coefficient kernel) */
  return produce_route(
    "sample", nlimbs, plans, d_c, batch, (flags & NTT_SAMPLE_TRANSFORMED) != 0 && kind != NTT_SAMPLE_UNIFORM, acc, stream, lay, nullptr,
    [&](const std::pair<int, int> &run) { return sample_fused_applies(plans[0], plans[run.first], run.second, acc); },
    [&](int first, int n) {
      SampleCoefArgs a = sa;
      produce_args(a, plans[0], first, n, d_c, ll.data(), batch, stream, lay);
      a.call.limb0 = (uint32_t)first;
      return produce_launched("sample_coef_kernel", launch_sample_coef(a));
    },
    [&](int first, int n) {
      const std::vector<unsigned char> recs = rns_records(plans, first, n);
      SampleFwdArgs                    a    = sa;
      produce_args(a, plans[first], first, n, d_c, ll.data(), batch, stream, lay);
      a.limbs      = recs.data();
      a.call.limb0 = (uint32_t)first;
      return produce_launched("sample_fwd_kernel", with_f64_class(run_class(plans, first, n), [&](auto k) {
                                return launch_sample_fwd<typename decltype(k)::A, decltype(k)::KSH>(a);
                              }));
    });
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
