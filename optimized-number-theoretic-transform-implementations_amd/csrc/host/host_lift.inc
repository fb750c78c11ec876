/* host/host_lift.inc -- into the RNS, the first step of an encryption and every plaintext operand: ntt_rns_from_plain_batch,
 * ntt_rns_from_double_batch and their strided forms.  A section of ntt_host.hip (one translation unit, included from there in order); not
 * compiled by itself.  The kernels are in lift.hip and the lift_f64*.hip units; this section sees their launchers and argument records
 * only (ntt_lift.h, which states the arithmetic).
 *
 * The route is produce_route (host_produce.inc) with lift_coef_kernel -- the plaintext word read once per launch: 8N(L + 1) bytes,
 * 8N(2L + 1) accumulating -- and lift_fwd_kernel, 8N + 8NL bytes (16NL accumulating), where NTT_OPT_LIFT_FUSED on plans[0] allows it.
 * This section keeps the lifts' own checks, the rule of that option and the constants. */

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
  if(!produce_fused_built(p)) return false;
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

/* both calls: d_m is the plaintext as words (the double mode's are bit patterns) */
static int rns_lift(int nlimbs, ntt_plan *const *plans, uint64_t *d_c, const uint64_t *d_m, uint32_t mode, uint64_t t, double scale,
                    uint64_t batch, unsigned flags, void *stream, const Layout &lay, uint64_t m_poly_stride)
{
  const unsigned known = NTT_LIFT_TRANSFORMED | NTT_LIFT_ACCUMULATE | (mode == kLiftDouble ? 0u : (unsigned)NTT_LIFT_SCALE);
  if(flags & ~known) return fail(NTT_ERR_ARG, mode == kLiftDouble && (flags & NTT_LIFT_SCALE) ? "from_double: NTT_LIFT_SCALE is from_plain's" : "unknown flag");
  if(mode != kLiftDouble && (t < 2 || t >= (1ull << 61))) return fail(NTT_ERR_ARG, "from_plain: the plaintext modulus must satisfy 2 <= t < 2^61");
  if(flags & NTT_LIFT_SCALE) mode = kLiftScaled;
  const int rc = produce_check("lift", nlimbs, plans, d_c && d_m, batch, lay, [&](int l) {
    return mode == kLiftScaled && t % plans[l]->q == 0 ? "from_plain: NTT_LIFT_SCALE needs every prime coprime to t" : nullptr;
  });
  if(rc) return rc;
  const uint64_t N = plans[0]->N;
  if(m_poly_stride < N || m_poly_stride > (1ull << 40)) return fail(NTT_ERR_ARG, "layout: the plaintext's polynomial stride must be N .. 2^40 words");
  const bool acc = (flags & NTT_LIFT_ACCUMULATE) != 0;
  /* in the fused route another limb's workgroup may still be reading the plaintext: no overlap at all */
  const bool overlap = batch > 0 && galois_overlap(galois_span(d_m, N, 1, batch, 0, m_poly_stride), galois_span(d_c, N, nlimbs, batch, lay.limb, lay.poly));
  LiftArgs la{};
  la.m               = d_m;
  la.m_poly_stride   = m_poly_stride;
  la.call.mode       = mode;
  la.call.accumulate = acc ? 1u : 0u;
  la.call.scale      = scale;
  la.call.td         = plain_dst(mode == kLiftDouble ? 2 : t, 0);
  if(mode != kLiftDouble) {
    la.call.half_dn = t / 2;
    la.call.half_up = t - t / 2;
    uint64_t r      = 1 % t;
    for(int l = 0; l < nlimbs; l++) r = (uint64_t)((unsigned __int128)r * (plans[l]->q % t) % t);
    la.call.r = r; /* Q mod t */
  }
  std::vector<LiftLimb> ll((size_t)nlimbs);
  for(int l = 0; l < nlimbs; l++) ll[(size_t)l] = lift_limb(plans[l]->q, mode, t, la.call.r);
  return produce_route(
    "lift", nlimbs, plans, d_c, batch, (flags & NTT_LIFT_TRANSFORMED) != 0, acc, stream, lay, overlap ? "lift: the plaintext overlaps the output" : nullptr,
    [&](const std::pair<int, int> &run) { return lift_fused_applies(plans[0], plans[run.first], mode, acc); },
    [&](int first, int n) {
      LiftArgs a = la;
      produce_args(a, plans[0], first, n, d_c, ll.data(), batch, stream, lay);
      return produce_launched("lift_coef_kernel", launch_lift_coef(a));
    },
    [&](int first, int n) {
      const std::vector<unsigned char> recs = rns_records(plans, first, n);
      LiftArgs                         a    = la;
      produce_args(a, plans[first], first, n, d_c, ll.data(), batch, stream, lay);
      a.limbs = recs.data();
      return produce_launched("lift_fwd_kernel", with_f64_class(run_class(plans, first, n), [&](auto k) {
                                return launch_lift_fwd<typename decltype(k)::A, decltype(k)::KSH>(a);
                              }));
    });
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
