/* host/host_exact.inc -- the exact base conversions of BFV multiplication: ntt_rns_mod_up_exact_batch, ntt_rns_mod_down_exact_batch and
 * their strided forms.  A section of ntt_host.hip (one translation unit, included from there in order); not compiled by itself.  The
 * kernels are in exact_coef.hip; this section sees their launchers only (ntt_exact.h, which states the arithmetic and its error bound).
 *
 *   exact ModUp     ntt_rns_mod_up_batch with ExactBConv for FastBConv: every limb outside the digit gets the CENTRED digit value.
 *                   coefficients   exact_up_coef_kernel, one launch per 16 destination limbs (the digit read once per launch);
 *                   NTT domain     the inverse of the digit's limbs, those launches, the forward transform of every limb.
 *   exact ModDown   limbs 0 .. nq-1 are Q, limbs nq .. nq+np-1 are P; the Q limbs become round(mult * x / P) exactly:
 *                   coefficients   exact_down_coef_kernel, one launch per 16 Q limbs: 8N(2nq + np) bytes;
 *                   NTT domain     the inverse transform of the P limbs, then per run of compatible Q limbs (rns_runs): FP64 policies at
 *                                  N = 2^6..2^14 -- moddown_exact_fwd_kernel, ONE launch per run: 8N(2nq + 3np) bytes in all; anything
 *                                  else -- the sandwich: the inverse over the run, exact_down_coef_kernel, the forward over the run.
 *                                  The route switch is NTT_OPT_RESCALE_FUSED on plans[0] (rescale_fused_applies), as for ModDown,
 *                                  and the measured rule: the fused kernel up to kExactFusedMaxNp P primes (exact_fused_applies).
 * v (ntt_exact.h) is formed by every launch from the source words with the same operations: one v per coefficient for the whole call.
 * Nothing is allocated, the host is not synchronised and no memset is issued: the calls can be captured into a graph. */

/* The fused kernel redoes the conversion in every Q limb's workgroup, the sandwich's coefficient kernel once per 16 Q limbs: the fused
 * route loses as np grows.  profiles/r15/exact_bench.txt, 24 Q limbs, call rate of the fused route over the sandwich at 64 / 1024
 * polynomials: np 1: 1.78-1.80 / 1.85-1.86 (2^13), 1.64-1.65 / 1.51-1.52 (2^14); np 2: 1.55-1.57 / 1.57-1.58, 1.41-1.42 / 1.26; np 4:
 * 1.26-1.29 / 1.23, 1.12-1.13 / 0.97-0.98; np 8: 0.95-0.97 / 0.89-0.90, 0.84 / 0.72-0.73 -- slower at both batch sizes at np 8 only (5..7
 * were not measured and go with 8). */
constexpr int kExactFusedMaxNp = 4;
static bool exact_fused_applies(const ntt_plan *p0, const ntt_plan *p, int np) { return np <= kExactFusedMaxNp && rescale_fused_applies(p0, p); }

/* rho_i = 1.0 / (double)b_i: one IEEE division per source prime */
static void exact_rhos(const uint64_t *b, int n, double *rho)
{
  for(int i = 0; i < n; i++) rho[i] = 1.0 / (double)b[i];
}

/* exact_up_coef_kernel over ModUp's whole destination range, one launch per 16 destination limbs (modup_launches with the exact record:
 * dl[d].h = q - [B]_q) */
static int modup_exact_launches(ntt_plan *const *plans, const uint64_t *b, BconvExactArgs &xa, int ndest)
{
  BconvArgs &ba    = xa.ba;
  const int  first = ba.first, count = ba.count;
  for(int k0 = 0; k0 < ndest; k0 += kBconvLimbs) {
    ba.k0   = k0;
    ba.ndst = ndest - k0 < kBconvLimbs ? ndest - k0 : kBconvLimbs;
    for(int d = 0; d < ba.ndst; d++) {
      const int      k = k0 + d;
      const uint64_t q = plans[k < first ? k : k + count]->q;
      uint64_t       g[kBconvLimbs];
      ba.dl[d]   = bconv_dst(q);
      ba.dl[d].h = q - bconv_hats(b, count, q, g); /* [B]_q is not 0: the primes are distinct */
      for(int i = 0; i < count; i++) ba.g[i][d] = g[i];
    }
    const hipError_t e = launch_bconv_exact(xa);
    if(e != hipSuccess) return fail(NTT_ERR_HIP, std::string("exact_up_coef_kernel: ") + hipGetErrorString(e));
  }
  return NTT_OK;
}

/* ------------------------------------------------------------------ */
/* exact ModUp                                                         */
/* ------------------------------------------------------------------ */
static int rns_mod_up_exact(int nlimbs, ntt_plan *const *plans, uint64_t *d_a, int first, int count, uint64_t batch, unsigned flags,
                            void *stream, const Layout &lay)
{
  int rc = rns_check(nlimbs, plans);
  if(rc) return rc;
  if(count < 1 || count > kBconvLimbs || first < 0 || first > nlimbs - count) return fail(NTT_ERR_ARG, "the digit's limbs are out of range");
  if(flags & ~(unsigned)NTT_MODUP_TRANSFORMED) return fail(NTT_ERR_ARG, "unknown flag");
  if(!d_a) return fail(NTT_ERR_ARG, "null argument");
  rc = layout_check(plans[0]->N, nlimbs, batch, lay);
  if(!rc) rc = distinct_primes(nlimbs, plans);
  if(rc) return rc;
  const bool ntt_dom = (flags & NTT_MODUP_TRANSFORMED) != 0;
  if(ntt_dom) {
    for(int l = 0; l < nlimbs; l++) {
      if(!plans[l]->has_fwd) return fail(NTT_ERR_ARG, "a limb's plan lacks the forward table");
      if(l >= first && l < first + count && !plans[l]->has_inv) return fail(NTT_ERR_ARG, "a digit limb's plan lacks the inverse table");
    }
  }
  if(batch == 0) return NTT_OK;
  USE_DEVICE(plans[0]->device);
  const Layout   one{lay.limb, lay.poly};
  uint64_t       b[kBconvLimbs];
  BconvExactArgs xa{};
  modup_args(plans, d_a, first, count, batch, stream, lay, b, xa.ba);
  exact_rhos(b, count, xa.rho);
  if(ntt_dom) rc = rns_transform(count, plans + first, d_a + (uint64_t)first * lay.limb, batch, true, stream, one);
  if(!rc) rc = modup_exact_launches(plans, b, xa, nlimbs - count);
  if(!rc && ntt_dom) rc = rns_transform(nlimbs, plans, d_a, batch, false, stream, one);
  return rc;
}

extern "C" int ntt_rns_mod_up_exact_batch(int nlimbs, ntt_plan *const *plans, uint64_t *d_a, int first, int count, uint64_t batch,
                                          unsigned flags, void *stream)
{
  return rns_mod_up_exact(nlimbs, plans, d_a, first, count, batch, flags, stream, limb_major(plans, nlimbs, batch));
}

extern "C" int ntt_rns_mod_up_exact_batch_strided(int nlimbs, ntt_plan *const *plans, uint64_t *d_a, int first, int count,
                                                  uint64_t limb_stride, uint64_t poly_stride, uint64_t batch, unsigned flags, void *stream)
{
  return rns_mod_up_exact(nlimbs, plans, d_a, first, count, batch, flags, stream, Layout{limb_stride, poly_stride});
}

/* ------------------------------------------------------------------ */
/* exact scaled ModDown                                                */
/* ------------------------------------------------------------------ */
/* the P primes' constants with the multiplier folded in: inv = [m p^_j^-1]_{p_j}, no offset */
static void exact_sources(const uint64_t *pr, int np, uint64_t mult, BconvSrc *out, double *rho)
{
  bconv_sources(pr, np, false, out);
  for(int j = 0; j < np; j++) {
    out[j].inv       = h_mulmod(out[j].inv, mult % pr[j], pr[j]);
    out[j].inv_shoup = shoup_of(out[j].inv, pr[j]);
  }
  exact_rhos(pr, np, rho);
}

/* Q limb q's constants for the P primes pr[0 .. np-1]: Barrett, [P^-1]_q, h = q - [P]_q (not 0: the primes are distinct); g[j] = [p^_j]_q */
static BconvDst moddown_exact_dst(uint64_t q, const uint64_t *pr, int np, uint64_t *g)
{
  BconvDst       d  = bconv_dst(q);
  const uint64_t pm = bconv_hats(pr, np, q, g);
  d.s               = h_powmod(pm, q - 2, q);
  d.s_shoup         = shoup_of(d.s, q);
  d.h               = q - pm;
  return d;
}

static int moddown_exact_fwd_launch(ntt_plan *const *plans, int first, int n, int nq, int np, uint64_t *d_a, uint64_t mult, uint64_t batch,
                                    void *stream, const Layout &lay, const uint64_t *pr)
{
  const std::vector<unsigned char> recs = rns_records(plans, first, n);
  ModDownExactFwdArgs              xa{};
  ModDownFwdArgs &                 ma = xa.ma;
  const int                        kc = moddown_fwd_args(ma, recs, plans, first, n, nq, np, d_a, batch, stream, lay);
  exact_sources(pr, np, mult, ma.pl, xa.rho);
  for(int l = 0; l < n; l++) {
    const uint64_t q = plans[first + l]->q;
    uint64_t       g[kBconvLimbs]; /* (formed again by the kernel's workgroups: no room for the table in its arguments) */
    ma.ql[l] = moddown_exact_dst(q, pr, np, g);
    xa.mq[l] = mult % q;
  }
  const hipError_t e = with_f64_class(kc, [&](auto k) { return launch_moddown_exact_fwd<typename decltype(k)::A, decltype(k)::KSH>(xa); });
  if(e != hipSuccess) return fail(NTT_ERR_HIP, std::string("moddown_exact_fwd_kernel: ") + hipGetErrorString(e));
  return NTT_OK;
}

static int moddown_exact_launch(ntt_plan *const *plans, int first, int n, int nq, int np, uint64_t *d_a, uint64_t mult, uint64_t batch,
                                void *stream, const Layout &lay, const uint64_t *pr)
{
  ModDownExactArgs xa{};
  ModDownCoefArgs &ma = xa.ma;
  ma.c           = d_a + (uint64_t)first * lay.limb;
  ma.t           = d_a + (uint64_t)nq * lay.limb;
  ma.limb_stride = lay.limb;
  ma.poly_stride = lay.poly;
  ma.batch       = batch;
  ma.logn        = (uint32_t)plans[0]->m;
  ma.nlimbs      = n;
  ma.np          = np;
  exact_sources(pr, np, mult, ma.pl, xa.rho);
  for(int l = 0; l < n; l++) {
    const uint64_t q = plans[first + l]->q;
    uint64_t       g[kBconvLimbs];
    ma.ql[l]          = moddown_exact_dst(q, pr, np, g);
    xa.es[l].ms       = h_mulmod(ma.ql[l].s, mult % q, q);
    xa.es[l].ms_shoup = shoup_of(xa.es[l].ms, q);
    for(int j = 0; j < np; j++) ma.g[j][l] = g[j];
  }
  ma.max_grid = plans[0]->max_grid;
  ma.stream   = (hipStream_t)stream;
  const hipError_t e = launch_moddown_exact_coef(xa);
  if(e != hipSuccess) return fail(NTT_ERR_HIP, std::string("exact_down_coef_kernel: ") + hipGetErrorString(e));
  return NTT_OK;
}

static int rns_mod_down_exact(int nq, int np, ntt_plan *const *plans, uint64_t *d_a, uint64_t mult, uint64_t batch, unsigned flags,
                              void *stream, const Layout &lay)
{
  if(nq < 1 || np < 1 || np > kBconvLimbs) return fail(NTT_ERR_ARG, "ModDown needs 1 <= nq and 1 <= np <= 16");
  const int nlimbs = nq + np;
  int       rc     = rns_check(nlimbs, plans);
  if(rc) return rc;
  if(flags & (unsigned)(NTT_MODDOWN_FLOOR | NTT_MODDOWN_ACCUMULATE)) return fail(NTT_ERR_ARG, "the exact ModDown rounds and overwrites: FLOOR and ACCUMULATE do not apply");
  if(flags & ~(unsigned)NTT_MODDOWN_TRANSFORMED) return fail(NTT_ERR_ARG, "unknown flag");
  if(mult == 0 || mult >= (1ull << 61)) return fail(NTT_ERR_ARG, "the multiplier must satisfy 1 <= mult < 2^61");
  if(!d_a) return fail(NTT_ERR_ARG, "null argument");
  rc = layout_check(plans[0]->N, nlimbs, batch, lay);
  if(!rc) rc = distinct_primes(nlimbs, plans);
  if(rc) return rc;
  return moddown_route(
    nq, np, plans, d_a, batch, (flags & NTT_MODDOWN_TRANSFORMED) != 0, stream, lay, nullptr,
    [&](const ntt_plan *p) { return exact_fused_applies(plans[0], p, np) ? kModDownFusedHere : kModDownSandwich; },
    [&](int first, int n, const uint64_t *pr) { return moddown_exact_launch(plans, first, n, nq, np, d_a, mult, batch, stream, lay, pr); },
    [&](ModDownRun, int first, int n, const uint64_t *pr) { return moddown_exact_fwd_launch(plans, first, n, nq, np, d_a, mult, batch, stream, lay, pr); },
    moddown_no_fold);
}

extern "C" int ntt_rns_mod_down_exact_batch(int nq, int np, ntt_plan *const *plans, uint64_t *d_a, uint64_t mult, uint64_t batch,
                                            unsigned flags, void *stream)
{
  return rns_mod_down_exact(nq, np, plans, d_a, mult, batch, flags, stream, limb_major(plans, nq + np, batch));
}

extern "C" int ntt_rns_mod_down_exact_batch_strided(int nq, int np, ntt_plan *const *plans, uint64_t *d_a, uint64_t mult,
                                                    uint64_t limb_stride, uint64_t poly_stride, uint64_t batch, unsigned flags, void *stream)
{
  return rns_mod_down_exact(nq, np, plans, d_a, mult, batch, flags, stream, Layout{limb_stride, poly_stride});
}
