/* host/host_ct_mul.inc -- the first and the last step of a homomorphic multiplication on NTT-domain ciphertexts: ntt_rns_tensor_batch,
 * ntt_rns_mod_down_add_batch and their strided forms.  A section of ntt_host.hip (one translation unit, included from there in
 * order); not compiled by itself.  The kernels are in ct_elem.hip and the ksfold_f64*.hip units; this section sees their launchers
 * only (ntt_ct_mul.h).
 *
 *   tensor        (c0, c1, c2) = (a0 b0, a0 b1 + a1 b0, a1 b1) per limb and word: tensor_kernel, one launch per 16 limbs, integer
 *                 arithmetic for every policy and every N >= 2.
 *   mod_down_add  c_l (+)= r_l, r_l what ntt_rns_mod_down_batch leaves in Q limb l of the accumulator d_a.  Per run of compatible Q
 *                 limbs (rns_runs):
 *                 fused        TRANSFORMED, FP64 policies, N = 2^6..2^14, where NTT_OPT_MODDOWN_ADD_FUSED on plans[0] allows it: ONE
 *                              ksfold_fwd_kernel launch.  d_a's Q limbs of the run are only read.
 *                 composition  anything else: ntt_rns_mod_down_batch's route of that run in place on d_a (NTT_OPT_RESCALE_FUSED keeps
 *                              selecting it), then ct_fold_kernel, one launch per 16 limbs.
 *                 The inverse transform of the P limbs is issued once, in front of every run.
 * Nothing is allocated, the host is not synchronised and no memset is issued: the calls can be captured into a graph. */

/* ------------------------------------------------------------------ */
/* tensor                                                              */
/* ------------------------------------------------------------------ */
static int rns_tensor(int nlimbs, ntt_plan *const *plans, uint64_t *const (&c)[3], const uint64_t *const (&a)[2], const uint64_t *const (&b)[2],
                      uint64_t batch, unsigned flags, void *stream, const Layout &lay)
{
  int rc = rns_check(nlimbs, plans);
  if(rc) return rc;
  if(flags & ~(unsigned)NTT_MUL_LAZY_IN) return fail(NTT_ERR_ARG, "unknown flag");
  if(!c[0] || !c[1] || !c[2] || !a[0] || !a[1] || !b[0] || !b[1]) return fail(NTT_ERR_ARG, "null argument");
  if(plans[0]->m < 1 || plans[0]->m > 30) return fail(NTT_ERR_ARG, "tensor: N out of range");
  rc = layout_check(plans[0]->N, nlimbs, batch, lay);
  if(rc || batch == 0) return rc;
  const uint64_t N     = plans[0]->N;
  const auto     words = [&](const uint64_t *p) { return galois_span(p, N, nlimbs, batch, lay.limb, lay.poly); };
  for(int i = 0; i < 3; i++) {
    for(int j = i + 1; j < 3; j++)
      if(galois_overlap(words(c[i]), words(c[j]))) return fail(NTT_ERR_ARG, "tensor: two outputs overlap");
    /* an output may BE an input (every thread reads its four words before it stores its three); a shifted overlap is refused */
    const uint64_t *in[4] = {a[0], a[1], b[0], b[1]};
    for(const uint64_t *x : in)
      if(x != c[i] && galois_overlap(words(c[i]), words(x))) return fail(NTT_ERR_ARG, "tensor: an output overlaps an input it is not identical to");
  }
  USE_DEVICE(plans[0]->device);
  TensorArgs ta{};
  ta.square      = b[0] == a[0] && b[1] == a[1];
  ta.limb_stride = lay.limb;
  ta.poly_stride = lay.poly;
  ta.batch       = batch;
  ta.logn        = (uint32_t)plans[0]->m;
  ta.max_grid    = plans[0]->max_grid;
  ta.stream      = (hipStream_t)stream;
  for(int f = 0; f < nlimbs; f += kCtLimbs) {
    ta.nlimbs = nlimbs - f < kCtLimbs ? nlimbs - f : kCtLimbs;
    for(int j = 0; j < 3; j++) ta.c[j] = c[j] + (uint64_t)f * lay.limb;
    for(int j = 0; j < 2; j++) {
      ta.a[j] = a[j] + (uint64_t)f * lay.limb;
      ta.b[j] = b[j] + (uint64_t)f * lay.limb;
    }
    for(int l = 0; l < ta.nlimbs; l++) ta.ql[l] = bconv_dst(plans[f + l]->q);
    const hipError_t e = launch_tensor(ta);
    if(e != hipSuccess) return fail(NTT_ERR_HIP, std::string("tensor_kernel: ") + hipGetErrorString(e));
  }
  return NTT_OK;
}

extern "C" int ntt_rns_tensor_batch(int nlimbs, ntt_plan *const *plans, uint64_t *d_c0, uint64_t *d_c1, uint64_t *d_c2, const uint64_t *d_a0,
                                    const uint64_t *d_a1, const uint64_t *d_b0, const uint64_t *d_b1, uint64_t batch, unsigned flags, void *stream)
{
  return rns_tensor(nlimbs, plans, {d_c0, d_c1, d_c2}, {d_a0, d_a1}, {d_b0, d_b1}, batch, flags, stream, limb_major(plans, nlimbs, batch));
}

extern "C" int ntt_rns_tensor_batch_strided(int nlimbs, ntt_plan *const *plans, uint64_t *d_c0, uint64_t *d_c1, uint64_t *d_c2,
                                            const uint64_t *d_a0, const uint64_t *d_a1, const uint64_t *d_b0, const uint64_t *d_b1,
                                            uint64_t limb_stride, uint64_t poly_stride, uint64_t batch, unsigned flags, void *stream)
{
  return rns_tensor(nlimbs, plans, {d_c0, d_c1, d_c2}, {d_a0, d_a1}, {d_b0, d_b1}, batch, flags, stream, Layout{limb_stride, poly_stride});
}

/* ------------------------------------------------------------------ */
/* ModDown into a ciphertext                                           */
/* ------------------------------------------------------------------ */
static bool ksfold_built(const ntt_plan *p) { return p->arith == NTT_ARITH_F64 && !p->generic && p->m >= kFusedMin && p->m <= kFusedMax; }

/* The automatic choice (NTT_OPT_MODDOWN_ADD_FUSED -1).  From profiles/r14/ct_mul_bench.txt (24 Q limbs of 50-bit primes, np 60-bit P
 * primes, TRANSFORMED | ACCUMULATE; the call rate of the fused route over that of the composition route of the same library, ranges
 * over five rounds of alternating processes; the parent's own spread 1.01-1.02):
 *     np   2^13 x 2     2^13 x 64    2^13 x 1024   2^14 x 2     2^14 x 64    2^14 x 1024
 *      1   1.05-1.06    1.35-1.38    1.49-1.50     1.08-1.08    1.27-1.32    1.51-1.52
 *      2   1.01-1.03    1.22-1.26    1.28-1.29     1.05-1.06    1.17-1.19    1.29-1.30
 *      4   0.99-1.01    1.18-1.19    1.20-1.21     1.04-1.04    1.15-1.16    1.21-1.22
 * The fused kernel is not slower than the composition at both 64 and 1024 polynomials for every np measured, and the gain shrinks
 * with np as the conversion's share of the call grows (it is the same in both routes); the launch-bound 2-polynomial rows are inside
 * the spread or ahead.  So: fused wherever it is built.  (Against the parent commit's ntt_rns_mod_down_batch plus the addition with
 * torch integer ops the fused route reads 1.66-2.86 at 64 and 1024 polynomials and 1.10-1.31 at 2; the fused call takes 6-16 % longer
 * than the parent's ModDown alone, the floor, at 1024 polynomials and 7-37 % longer at 64.) */
static bool ksfold_pays(int np)
{
  (void)np; /* (no np measured at which the composition is ahead) */
  return true;
}

static bool ksfold_applies(const ntt_plan *p0, const ntt_plan *p, int np)
{
  if(!ksfold_built(p)) return false;
  if(p0->moddown_add_fused >= 0) return p0->moddown_add_fused == 1;
  return ksfold_pays(np);
}

static int ksfold_launch(ntt_plan *const *plans, int first, int n, int nq, int np, uint64_t *d_c, uint64_t *d_a, uint64_t batch, bool floor_div,
                         bool accumulate, void *stream, const Layout &clay, const Layout &alay, const uint64_t *pr)
{
  const std::vector<unsigned char> recs = rns_records(plans, first, n);
  KsFoldArgs                       ka{};
  ModDownFwdArgs &                 ma = ka.m;
  const int                        kc = moddown_fwd_args(ma, recs, plans, first, n, nq, np, d_a, batch, stream, alay);
  bconv_sources(pr, np, !floor_div, ma.pl);
  for(int l = 0; l < n; l++) {
    uint64_t g[kBconvLimbs]; /* (formed again by the kernel's workgroups: no room for the table in its arguments) */
    ma.ql[l] = moddown_dst(plans[first + l]->q, pr, np, floor_div, g);
  }
  ka.out             = d_c + (uint64_t)first * clay.limb;
  ka.out_limb_stride = clay.limb;
  ka.out_poly_stride = clay.poly;
  ka.accumulate      = accumulate;
  const hipError_t e = with_f64_class(kc, [&](auto k) { return launch_ksfold_fwd<typename decltype(k)::A, decltype(k)::KSH>(ka); });
  if(e != hipSuccess) return fail(NTT_ERR_HIP, std::string("ksfold_fwd_kernel: ") + hipGetErrorString(e));
  return NTT_OK;
}

/* c_l (+)= a_l over Q limbs [first, first + n): ct_fold_kernel, one launch per 16 limbs */
static int ct_fold_launches(ntt_plan *const *plans, int first, int n, uint64_t *d_c, const uint64_t *d_a, uint64_t batch, bool accumulate,
                            void *stream, const Layout &clay, const Layout &alay)
{
  CtFoldArgs fa{};
  fa.c_limb_stride = clay.limb;
  fa.c_poly_stride = clay.poly;
  fa.a_limb_stride = alay.limb;
  fa.a_poly_stride = alay.poly;
  fa.batch         = batch;
  fa.logn          = (uint32_t)plans[0]->m;
  fa.accumulate    = accumulate;
  fa.max_grid      = plans[0]->max_grid;
  fa.stream        = (hipStream_t)stream;
  for(int f = first; f < first + n; f += kCtLimbs) {
    fa.nlimbs = first + n - f < kCtLimbs ? first + n - f : kCtLimbs;
    fa.c      = d_c + (uint64_t)f * clay.limb;
    fa.a      = d_a + (uint64_t)f * alay.limb;
    for(int l = 0; l < fa.nlimbs; l++) fa.q[l] = plans[f + l]->q;
    const hipError_t e = launch_ct_fold(fa);
    if(e != hipSuccess) return fail(NTT_ERR_HIP, std::string("ct_fold_kernel: ") + hipGetErrorString(e));
  }
  return NTT_OK;
}

static int rns_mod_down_add(int nq, int np, ntt_plan *const *plans, uint64_t *d_c, uint64_t *d_a, uint64_t batch, unsigned flags, void *stream,
                            const Layout &clay, const Layout &alay)
{
  if(nq < 1 || np < 1 || np > kBconvLimbs) return fail(NTT_ERR_ARG, "ModDown needs 1 <= nq and 1 <= np <= 16");
  const int nlimbs = nq + np;
  int       rc     = rns_check(nlimbs, plans);
  if(rc) return rc;
  if(flags & ~(unsigned)(NTT_MODDOWN_TRANSFORMED | NTT_MODDOWN_FLOOR | NTT_MODDOWN_ACCUMULATE)) return fail(NTT_ERR_ARG, "unknown flag");
  if(!d_a || !d_c) return fail(NTT_ERR_ARG, "null argument");
  if(plans[0]->m < 1 || plans[0]->m > 30) return fail(NTT_ERR_ARG, "mod_down_add: N out of range");
  rc = layout_check(plans[0]->N, nlimbs, batch, alay);
  if(!rc) rc = layout_check(plans[0]->N, nq, batch, clay);
  if(!rc) rc = distinct_primes(nlimbs, plans);
  if(rc) return rc;
  const bool floor_div  = (flags & NTT_MODDOWN_FLOOR) != 0;
  const bool accumulate = (flags & NTT_MODDOWN_ACCUMULATE) != 0;
  const bool overlap    = galois_overlap(galois_span(d_c, plans[0]->N, nq, batch, clay.limb, clay.poly),
                                         galois_span(d_a, plans[0]->N, nlimbs, batch, alay.limb, alay.poly));
  return moddown_route(
    nq, np, plans, d_a, batch, (flags & NTT_MODDOWN_TRANSFORMED) != 0, stream, alay, overlap ? "mod_down_add: d_c overlaps d_a" : nullptr,
    [&](const ntt_plan *p) {
      return ksfold_applies(plans[0], p, np) ? kModDownFusedInto : rescale_fused_applies(plans[0], p) ? kModDownFusedHere : kModDownSandwich;
    },
    [&](int first, int n, const uint64_t *pr) { return moddown_coef_launch(plans, first, n, nq, np, d_a, batch, floor_div, stream, alay, pr); },
    [&](ModDownRun k, int first, int n, const uint64_t *pr) {
      return k == kModDownFusedInto ? ksfold_launch(plans, first, n, nq, np, d_c, d_a, batch, floor_div, accumulate, stream, clay, alay, pr)
                                    : moddown_fwd_launch(plans, first, n, nq, np, d_a, batch, floor_div, stream, alay, pr);
    },
    [&](int first, int n) { return ct_fold_launches(plans, first, n, d_c, d_a, batch, accumulate, stream, clay, alay); });
}

extern "C" int ntt_rns_mod_down_add_batch(int nq, int np, ntt_plan *const *plans, uint64_t *d_c, uint64_t *d_a, uint64_t batch, unsigned flags,
                                          void *stream)
{
  return rns_mod_down_add(nq, np, plans, d_c, d_a, batch, flags, stream, limb_major(plans, nq, batch), limb_major(plans, nq + np, batch));
}

extern "C" int ntt_rns_mod_down_add_batch_strided(int nq, int np, ntt_plan *const *plans, uint64_t *d_c, uint64_t *d_a, uint64_t c_limb_stride,
                                                  uint64_t c_poly_stride, uint64_t a_limb_stride, uint64_t a_poly_stride, uint64_t batch,
                                                  unsigned flags, void *stream)
{
  return rns_mod_down_add(nq, np, plans, d_c, d_a, batch, flags, stream, Layout{c_limb_stride, c_poly_stride}, Layout{a_limb_stride, a_poly_stride});
}
