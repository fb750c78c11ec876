/* host/host_bgv.inc -- BGV modulus switching: ntt_rns_mod_down_bgv_batch, ntt_rns_mod_down_bgv_add_batch and their strided forms: the
 * ModDown whose correction is = x mod P and = 0 mod T, so that the plaintext mod T survives the division (ntt_bgv.h states the
 * arithmetic).  A section of ntt_host.hip (one translation unit, included from there in order); not compiled by itself.
 *
 *   coefficients   moddown_coef_kernel ITSELF, one launch per 16 Q limbs (the P limbs read once per launch), with the constants folded on
 *                  the host: BconvSrc::h = [h T]_{p_j}, BconvSrc::inv = [T^-1 p^_j^-1]_{p_j}, g[j][l] = [T p^_j]_{q_l}, BconvDst::h =
 *                  [T h]_{q_l}.  The kernel has no one-prime shortcut, so np = 1 takes the same path (g[0][l] = [T]_{q_l}).  The add form
 *                  then runs ct_fold_kernel, one launch per 16 limbs, as ntt_rns_mod_down_add_batch's composition does.
 *   NTT domain     the inverse transform of the P limbs once, then per run of compatible Q limbs (rns_runs):
 *                  fused     FP64 policies, N = 2^6..2^14, where NTT_OPT_BGV_FUSED on plans[0] allows it: ONE moddown_bgv_fwd_kernel
 *                            launch for either form (the in-place form stores into the accumulator's own Q limbs);
 *                  sandwich  anything else: the inverse over the run, the coefficient launch, the forward over the run (the add form:
 *                            in place on d_a, then ct_fold_kernel).
 * Nothing is allocated, the host is not synchronised and no memset is issued: the calls can be captured into a graph. */

/* The automatic choice (NTT_OPT_BGV_FUSED -1).  The fused kernel redoes the conversion in every Q limb's workgroup, the sandwich's
 * coefficient kernel once per 16 Q limbs, so the fused route loses ground as np grows.  From profiles/r16/bgv_bench.txt (24 Q limbs of
 * 50-bit primes, np 60-bit P primes, T = 65537; the call rate of the fused route over the sandwich of the same library at 64 / 1024
 * polynomials, ranges over five rounds of alternating processes, 2^13 then 2^14):
 *     in place   np 1: 1.99-2.08 / 2.19-2.21, 1.86-1.93 / 1.87-1.88;   np 2: 1.56-1.57 / 1.42-1.43, 1.40-1.42 / 1.26;
 *                np 4: 1.26-1.27 / 1.11, 1.13-1.14 / 0.98;             np 8: 0.97 / 0.82-0.83, 0.88 / 0.73-0.74
 *     add form   np 1: 2.25-2.32 / 2.54-2.56, 1.86-1.93 / 2.26-2.27;   np 2: 1.78-1.81 / 1.65-1.68, 1.48-1.50 / 1.54-1.55;
 *                np 4: 1.46-1.48 / 1.30-1.32, 1.23-1.24 / 1.21-1.22;   np 8: 1.11-1.12 / 0.97, 0.95 / 0.89
 * (the parent's own spread 1.00-1.06).  The fused kernel is taken for exactly those np at which it is not slower at both 64 and 1024
 * polynomials: in place up to np 4 at 2^13 and up to np 2 at 2^14 (np 4 is 0.98 there at 1024 polynomials, in every round); the add
 * form, whose sandwich pays an element-wise launch more, up to np 4 at both sizes; np 8 is slower at 1024 polynomials everywhere.
 * Unmeasured np go with the next measured np above (3 with 4, 5..7 with 8), sizes below 2^13 with 2^13.  At 2 polynomials, launch-bound,
 * the fused kernel reads 1.27-1.47 at np 1, 1.00-1.16 at np 2 and 0.82-0.94 at np 4: the default loses there at np 3 and 4. */
static int bgv_fused_max_np(bool add_form, int logn) { return !add_form && logn >= 14 ? 2 : 4; }

static bool bgv_fused_applies(const ntt_plan *p0, const ntt_plan *p, int np, bool add_form)
{
  if(!ksfold_built(p)) return false; /* (the same instances: FP64 policies, N = 2^6..2^14) */
  if(p0->bgv_fused >= 0) return p0->bgv_fused == 1;
  return np <= bgv_fused_max_np(add_form, p->m);
}

/* the P primes' constants with T folded in: h = [h T]_{p_j}, inv = [T^-1 p^_j^-1]_{p_j} (T mod p_j != 0: checked by the caller) */
static void bgv_sources(const uint64_t *pr, int np, uint64_t t, BconvSrc *out)
{
  bconv_sources(pr, np, true, out);
  for(int j = 0; j < np; j++) {
    const uint64_t tp = t % pr[j];
    out[j].h          = h_mulmod(out[j].h, tp, pr[j]);
    out[j].inv        = h_mulmod(out[j].inv, h_powmod(tp, pr[j] - 2, pr[j]), pr[j]);
    out[j].inv_shoup  = shoup_of(out[j].inv, pr[j]);
  }
}

static BgvScale bgv_scale_of(uint64_t t, uint64_t q)
{
  const uint64_t tq = t % q;
  return BgvScale{tq, shoup_of(tq, q)};
}

/* moddown_coef_kernel over Q limbs [first, first + n) of d_a with the BGV constants */
static int bgv_coef_launch(ntt_plan *const *plans, int first, int n, int nq, int np, uint64_t *d_a, uint64_t t, uint64_t batch, void *stream,
                           const Layout &lay, const uint64_t *pr)
{
  ModDownCoefArgs ma{};
  ma.c           = d_a + (uint64_t)first * lay.limb;
  ma.t           = d_a + (uint64_t)nq * lay.limb;
  ma.limb_stride = lay.limb;
  ma.poly_stride = lay.poly;
  ma.batch       = batch;
  ma.logn        = (uint32_t)plans[0]->m;
  ma.nlimbs      = n;
  ma.np          = np;
  bgv_sources(pr, np, t, ma.pl);
  for(int l = 0; l < n; l++) {
    const uint64_t q  = plans[first + l]->q;
    const uint64_t tq = t % q;
    uint64_t       g[kBconvLimbs];
    ma.ql[l]   = moddown_dst(q, pr, np, false, g);
    ma.ql[l].h = h_mulmod(ma.ql[l].h, tq, q);
    for(int j = 0; j < np; j++) ma.g[j][l] = h_mulmod(g[j], tq, q);
  }
  ma.max_grid = plans[0]->max_grid;
  ma.stream   = (hipStream_t)stream;
  const hipError_t e = launch_moddown_coef(ma);
  if(e != hipSuccess) return fail(NTT_ERR_HIP, std::string("moddown_coef_kernel (BGV constants): ") + hipGetErrorString(e));
  return NTT_OK;
}

/* moddown_bgv_fwd_kernel over the run [first, first + n): out = d_c's limbs of the run (the in-place form: d_a's own) */
static int bgv_fwd_launch(ntt_plan *const *plans, int first, int n, int nq, int np, uint64_t *d_c, uint64_t *d_a, uint64_t t, uint64_t batch,
                          bool accumulate, void *stream, const Layout &clay, const Layout &alay, const uint64_t *pr)
{
  const std::vector<unsigned char> recs = rns_records(plans, first, n);
  ModDownBgvArgs                   ba{};
  KsFoldArgs &                     ka = ba.k;
  ModDownFwdArgs &                 ma = ka.m;
  const int                        kc = moddown_fwd_args(ma, recs, plans, first, n, nq, np, d_a, batch, stream, alay);
  bgv_sources(pr, np, t, ma.pl);
  for(int l = 0; l < n; l++) {
    const uint64_t q = plans[first + l]->q;
    uint64_t       g[kBconvLimbs]; /* (formed again by the kernel's workgroups: no room for the table in its arguments) */
    ma.ql[l]   = moddown_dst(q, pr, np, false, g);
    ma.ql[l].h = h_mulmod(ma.ql[l].h, t % q, q);
    ba.ts[l]   = bgv_scale_of(t, q);
  }
  ka.out             = d_c + (uint64_t)first * clay.limb;
  ka.out_limb_stride = clay.limb;
  ka.out_poly_stride = clay.poly;
  ka.accumulate      = accumulate;
  const hipError_t e = with_f64_class(kc, [&](auto k) { return launch_moddown_bgv_fwd<typename decltype(k)::A, decltype(k)::KSH>(ba); });
  if(e != hipSuccess) return fail(NTT_ERR_HIP, std::string("moddown_bgv_fwd_kernel: ") + hipGetErrorString(e));
  return NTT_OK;
}

/* both public forms: d_c == nullptr is the in-place form (clay is then alay) */
static int rns_mod_down_bgv(int nq, int np, ntt_plan *const *plans, uint64_t *d_c, uint64_t *d_a, uint64_t t, uint64_t batch, unsigned flags,
                            void *stream, const Layout &clay, const Layout &alay, bool add_form)
{
  if(nq < 1 || np < 1 || np > kBconvLimbs) return fail(NTT_ERR_ARG, "ModDown needs 1 <= nq and 1 <= np <= 16");
  const int nlimbs = nq + np;
  int       rc     = rns_check(nlimbs, plans);
  if(rc) return rc;
  if(flags & (unsigned)NTT_MODDOWN_FLOOR) return fail(NTT_ERR_ARG, "the BGV ModDown's correction is centred: FLOOR does not apply");
  if(!add_form && (flags & (unsigned)NTT_MODDOWN_ACCUMULATE)) return fail(NTT_ERR_ARG, "ACCUMULATE belongs to the add form");
  if(flags & ~(unsigned)(NTT_MODDOWN_TRANSFORMED | NTT_MODDOWN_ACCUMULATE)) return fail(NTT_ERR_ARG, "unknown flag");
  if(t == 0 || t >= (1ull << 61)) return fail(NTT_ERR_ARG, "the plaintext modulus must satisfy 1 <= t < 2^61");
  if(!d_a || (add_form && !d_c)) return fail(NTT_ERR_ARG, "null argument");
  if(plans[0]->m < 1 || plans[0]->m > 30) return fail(NTT_ERR_ARG, "mod_down_bgv: N out of range");
  rc = layout_check(plans[0]->N, nlimbs, batch, alay);
  if(!rc && add_form) rc = layout_check(plans[0]->N, nq, batch, clay);
  if(!rc) rc = distinct_primes(nlimbs, plans);
  if(rc) return rc;
  for(int j = nq; j < nlimbs; j++) {
    if(t % plans[j]->q == 0) return fail(NTT_ERR_ARG, "a P prime divides the plaintext modulus");
  }
  const bool accumulate = (flags & NTT_MODDOWN_ACCUMULATE) != 0;
  const bool overlap    = add_form && galois_overlap(galois_span(d_c, plans[0]->N, nq, batch, clay.limb, clay.poly),
                                                     galois_span(d_a, plans[0]->N, nlimbs, batch, alay.limb, alay.poly));
  return moddown_route(
    nq, np, plans, d_a, batch, (flags & NTT_MODDOWN_TRANSFORMED) != 0, stream, alay, overlap ? "mod_down_bgv_add: d_c overlaps d_a" : nullptr,
    [&](const ntt_plan *p) { return bgv_fused_applies(plans[0], p, np, add_form) ? kModDownFusedInto : kModDownSandwich; },
    [&](int first, int n, const uint64_t *pr) { return bgv_coef_launch(plans, first, n, nq, np, d_a, t, batch, stream, alay, pr); },
    [&](ModDownRun, int first, int n, const uint64_t *pr) { /* (the in-place form: into d_a's own Q limbs) */
      return bgv_fwd_launch(plans, first, n, nq, np, add_form ? d_c : d_a, d_a, t, batch, accumulate, stream, add_form ? clay : alay, alay, pr);
    },
    [&](int first, int n) { return add_form ? ct_fold_launches(plans, first, n, d_c, d_a, batch, accumulate, stream, clay, alay) : NTT_OK; });
}

extern "C" int ntt_rns_mod_down_bgv_batch(int nq, int np, ntt_plan *const *plans, uint64_t *d_a, uint64_t t, uint64_t batch, unsigned flags,
                                          void *stream)
{
  const Layout lay = limb_major(plans, nq + np, batch);
  return rns_mod_down_bgv(nq, np, plans, nullptr, d_a, t, batch, flags, stream, lay, lay, false);
}

extern "C" int ntt_rns_mod_down_bgv_batch_strided(int nq, int np, ntt_plan *const *plans, uint64_t *d_a, uint64_t t, uint64_t limb_stride,
                                                  uint64_t poly_stride, uint64_t batch, unsigned flags, void *stream)
{
  const Layout lay{limb_stride, poly_stride};
  return rns_mod_down_bgv(nq, np, plans, nullptr, d_a, t, batch, flags, stream, lay, lay, false);
}

extern "C" int ntt_rns_mod_down_bgv_add_batch(int nq, int np, ntt_plan *const *plans, uint64_t *d_c, uint64_t *d_a, uint64_t t, uint64_t batch,
                                              unsigned flags, void *stream)
{
  return rns_mod_down_bgv(nq, np, plans, d_c, d_a, t, batch, flags, stream, limb_major(plans, nq, batch), limb_major(plans, nq + np, batch), true);
}

extern "C" int ntt_rns_mod_down_bgv_add_batch_strided(int nq, int np, ntt_plan *const *plans, uint64_t *d_c, uint64_t *d_a, uint64_t t,
                                                      uint64_t c_limb_stride, uint64_t c_poly_stride, uint64_t a_limb_stride,
                                                      uint64_t a_poly_stride, uint64_t batch, unsigned flags, void *stream)
{
  return rns_mod_down_bgv(nq, np, plans, d_c, d_a, t, batch, flags, stream, Layout{c_limb_stride, c_poly_stride},
                          Layout{a_limb_stride, a_poly_stride}, true);
}
