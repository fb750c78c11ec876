/* host/host_keyswitch.inc -- the base conversions of hybrid key switching: ntt_rns_mod_up_batch, ntt_rns_mod_down_batch and their
 * strided forms.  A section of ntt_host.hip (one translation unit, included from there in order); not compiled by itself.  The
 * kernels are in the keyswitch_*.hip units; this section sees their launchers only (ntt_keyswitch.h).
 *
 *   ModUp     limbs [first, first + count) of the operand are the digit; every other limb gets FastBConv of it:
 *             coefficients   bconv_kernel, one launch per 16 destination limbs (the digit read once per launch);
 *             NTT domain     the inverse of the digit's limbs, those launches, the forward transform of every limb.
 *   ModDown   limbs 0 .. nq-1 are Q, limbs nq .. nq+np-1 are P; the Q limbs become round(x / P) - v (floor: floor(x / P) - v),
 *             0 <= v < np: the rescale (host_rescale.inc) with the dropped prime generalised to a set:
 *             coefficients   moddown_coef_kernel, one launch per 16 Q limbs (the P limbs read once per launch): 8N(2nq + np) bytes;
 *             NTT domain     the inverse transform of the P limbs, then per run of compatible Q limbs (rns_runs): FP64 policies at
 *                            N = 2^6..2^14 -- moddown_fwd_kernel, ONE launch per run: 8N(2nq + 3np) bytes in all; anything else --
 *                            the sandwich: the inverse over the run, moddown_coef_kernel, the forward over the run.  The route
 *                            switch is NTT_OPT_RESCALE_FUSED on plans[0] (rescale_fused_applies).
 *             The route itself is moddown_route, shared with ntt_rns_mod_down_add_batch (host_ct_mul.inc), the exact ModDown
 *             (host_exact.inc) and the BGV ModDown (host_bgv.inc); moddown_fwd_args fills what their fused launches have in common.
 * The per-call constants take O(n^2) modular products for n source primes plus O(n) per destination prime (prefix and suffix
 * products; one inverse per source prime and per destination prime, none per pair).  Nothing is allocated, the host is not
 * synchronised and no memset is issued: the calls can be captured into a graph. */

/* a destination prime's Barrett constants (ModDown adds the scale and the offset) */
static BconvDst bconv_dst(uint64_t q)
{
  BconvDst d{};
  d.q                        = q;
  d.bar                      = ~0ull / q; /* = floor(2^64 / q): q is odd */
  const unsigned __int128 mu = ~(unsigned __int128)0 / q; /* = floor(2^128 / q) likewise */
  d.mu_lo                    = (uint64_t)mu;
  d.mu_hi                    = (uint64_t)(mu >> 64);
  return d;
}

static uint64_t shoup_of(uint64_t w, uint64_t q) { return (uint64_t)(((unsigned __int128)w << 64) / q); }

/* the source primes b_0 .. b_{n-1}: [b^_i^-1]_{b_i} (b^_i mod b_i as a product of n - 1 words, then one inverse) and the offset
 * [h]_{b_i} = (b_i - 1) / 2 of h = (B - 1) / 2 (2h = -1 mod b_i), or 0 */
static void bconv_sources(const uint64_t *b, int n, bool half, BconvSrc *out)
{
  for(int i = 0; i < n; i++) {
    uint64_t hat = 1;
    for(int k = 0; k < n; k++) {
      if(k != i) hat = h_mulmod(hat, b[k] % b[i], b[i]);
    }
    const uint64_t inv = n == 1 ? 1 : h_powmod(hat, b[i] - 2, b[i]);
    out[i]             = BconvSrc{b[i], half ? (b[i] - 1) / 2 : 0, inv, shoup_of(inv, b[i])};
  }
}

/* g[i] = [b^_i]_q for every source prime (prefix and suffix products mod q); returns [B]_q */
static uint64_t bconv_hats(const uint64_t *b, int n, uint64_t q, uint64_t *g)
{
  uint64_t pre[kBconvLimbs + 1], suf[kBconvLimbs + 1];
  pre[0] = 1;
  suf[n] = 1;
  for(int i = 0; i < n; i++) pre[i + 1] = h_mulmod(pre[i], b[i] % q, q);
  for(int i = n - 1; i >= 0; i--) suf[i] = h_mulmod(suf[i + 1], b[i] % q, q);
  for(int i = 0; i < n; i++) g[i] = h_mulmod(pre[i], suf[i + 1], q);
  return pre[n];
}

/* the operand's primes are pairwise distinct (a repeated prime has no inverse of its co-factor) */
static int distinct_primes(int nlimbs, ntt_plan *const *plans)
{
  for(int a = 0; a < nlimbs; a++)
    for(int b = a + 1; b < nlimbs; b++)
      if(plans[a]->q == plans[b]->q) return fail(NTT_ERR_ARG, "a prime appears twice among the operand's limbs");
  return NTT_OK;
}

/* ModUp's constants and launch loop, shared by ntt_rns_mod_up_batch and the key products that convert on their composition route
 * (host_modup_mul.inc, host_key_pair.inc).  modup_args: the digit's primes into b[] and everything of the launch record that does not
 * depend on the destination limbs. */
static void modup_args(ntt_plan *const *plans, uint64_t *d_a, int first, int count, uint64_t batch, void *stream, const Layout &lay, uint64_t *b,
                       BconvArgs &ba)
{
  for(int i = 0; i < count; i++) b[i] = plans[first + i]->q;
  bconv_sources(b, count, false, ba.sl);
  ba.a           = d_a;
  ba.limb_stride = lay.limb;
  ba.poly_stride = lay.poly;
  ba.batch       = batch;
  ba.logn        = (uint32_t)plans[0]->m;
  ba.first       = first;
  ba.count       = count;
  ba.max_grid    = plans[0]->max_grid;
  ba.stream      = (hipStream_t)stream;
}

/* bconv_kernel over ranges (k0, ndst) of ModUp's destination index -- the operand's limbs without the digit: destination k is slot k
 * in front of the digit, slot k + count behind it --, one launch per 16 destination limbs of a range */
static int modup_launches(ntt_plan *const *plans, const uint64_t *b, BconvArgs &ba, const std::pair<int, int> *ranges, size_t nranges)
{
  const int first = ba.first, count = ba.count;
  for(size_t r = 0; r < nranges; r++) {
    const int end = ranges[r].first + ranges[r].second;
    for(int k0 = ranges[r].first; k0 < end; k0 += kBconvLimbs) {
      ba.k0   = k0;
      ba.ndst = end - k0 < kBconvLimbs ? end - k0 : kBconvLimbs;
      for(int d = 0; d < ba.ndst; d++) {
        const int      k = k0 + d;
        const uint64_t q = plans[k < first ? k : k + count]->q;
        uint64_t       g[kBconvLimbs];
        ba.dl[d] = bconv_dst(q);
        bconv_hats(b, count, q, g);
        for(int i = 0; i < count; i++) ba.g[i][d] = g[i];
      }
      const hipError_t e = launch_bconv(ba);
      if(e != hipSuccess) return fail(NTT_ERR_HIP, std::string("bconv_kernel: ") + hipGetErrorString(e));
    }
  }
  return NTT_OK;
}

/* the destination ranges of the runs that convert through memory (fused[r] == 0), adjacent ranges joined: every run gives
 * [0, nlimbs - count), ntt_rns_mod_up_batch's launches */
static std::vector<std::pair<int, int>> modup_dst_ranges(const std::vector<std::pair<int, int>> &runs, const std::vector<char> &fused, int first,
                                                         int count)
{
  std::vector<std::pair<int, int>> dst;
  for(size_t r = 0; r < runs.size(); r++) {
    if(fused[r]) continue;
    for(int l = runs[r].first; l < runs[r].first + runs[r].second; l++) {
      if(l >= first && l < first + count) continue;
      const int k = l < first ? l : l - count;
      if(!dst.empty() && dst.back().first + dst.back().second == k) dst.back().second++;
      else dst.emplace_back(k, 1);
    }
  }
  return dst;
}

/* ------------------------------------------------------------------ */
/* ModUp                                                               */
/* ------------------------------------------------------------------ */
static int rns_mod_up(int nlimbs, ntt_plan *const *plans, uint64_t *d_a, int first, int count, uint64_t batch, unsigned flags,
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
  const Layout one{lay.limb, lay.poly};
  uint64_t     b[kBconvLimbs];
  BconvArgs    ba{};
  modup_args(plans, d_a, first, count, batch, stream, lay, b, ba);
  if(ntt_dom) rc = rns_transform(count, plans + first, d_a + (uint64_t)first * lay.limb, batch, true, stream, one);
  const std::pair<int, int> all(0, nlimbs - count);
  if(!rc) rc = modup_launches(plans, b, ba, &all, 1);
  if(!rc && ntt_dom) rc = rns_transform(nlimbs, plans, d_a, batch, false, stream, one);
  return rc;
}

extern "C" int ntt_rns_mod_up_batch(int nlimbs, ntt_plan *const *plans, uint64_t *d_a, int first, int count, uint64_t batch,
                                    unsigned flags, void *stream)
{
  return rns_mod_up(nlimbs, plans, d_a, first, count, batch, flags, stream, limb_major(plans, nlimbs, batch));
}

extern "C" int ntt_rns_mod_up_batch_strided(int nlimbs, ntt_plan *const *plans, uint64_t *d_a, int first, int count,
                                            uint64_t limb_stride, uint64_t poly_stride, uint64_t batch, unsigned flags, void *stream)
{
  return rns_mod_up(nlimbs, plans, d_a, first, count, batch, flags, stream, Layout{limb_stride, poly_stride});
}

/* ------------------------------------------------------------------ */
/* ModDown                                                             */
/* ------------------------------------------------------------------ */
/* Q limb q's constants for the P primes pr[0 .. np-1]: Barrett, [P^-1]_q, [h]_q = (P - 1) / 2 mod q = ([P]_q - 1) 2^-1; g[j] = [p^_j]_q */
static BconvDst moddown_dst(uint64_t q, const uint64_t *pr, int np, bool floor_div, uint64_t *g)
{
  BconvDst       d  = bconv_dst(q);
  const uint64_t pm = bconv_hats(pr, np, q, g);
  d.s               = h_powmod(pm, q - 2, q);
  d.s_shoup         = shoup_of(d.s, q);
  d.h               = floor_div ? 0 : h_mulmod((pm + q - 1) % q, (q + 1) / 2, q);
  return d;
}

static int moddown_coef_launch(ntt_plan *const *plans, int first, int n, int nq, int np, uint64_t *d_a, uint64_t batch, bool floor_div,
                               void *stream, const Layout &lay, const uint64_t *pr)
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
  bconv_sources(pr, np, !floor_div, ma.pl);
  for(int l = 0; l < n; l++) {
    uint64_t g[kBconvLimbs];
    ma.ql[l] = moddown_dst(plans[first + l]->q, pr, np, floor_div, g);
    for(int j = 0; j < np; j++) ma.g[j][l] = g[j];
  }
  ma.max_grid = plans[0]->max_grid;
  ma.stream   = (hipStream_t)stream;
  const hipError_t e = launch_moddown_coef(ma);
  if(e != hipSuccess) return fail(NTT_ERR_HIP, std::string("moddown_coef_kernel: ") + hipGetErrorString(e));
  return NTT_OK;
}

/* The fields of a fused ModDown launch (moddown_fwd_body's four kernels) that every variant fills alike: the run [first, first + n) of
 * d_a's Q limbs, its P limbs behind the nq Q limbs, the run's limb records (recs: the caller's, alive until the launch returns), sizes
 * and launch limits of the run's first plan.  The sources, ql[] and the variant's own constants are the caller's.  Returns the run's
 * headroom class. */
static int moddown_fwd_args(ModDownFwdArgs &ma, const std::vector<unsigned char> &recs, ntt_plan *const *plans, int first, int n, int nq, int np,
                            uint64_t *d_a, uint64_t batch, void *stream, const Layout &lay)
{
  ma.c           = d_a + (uint64_t)first * lay.limb;
  ma.t           = d_a + (uint64_t)nq * lay.limb;
  ma.limbs       = recs.data();
  ma.nlimbs      = n;
  ma.np          = np;
  ma.limb_stride = lay.limb;
  ma.poly_stride = lay.poly;
  ma.batch       = batch;
  ma.logn        = (uint32_t)plans[first]->m;
  ma.max_grid    = plans[first]->max_grid;
  ma.num_cus     = plans[first]->num_cus;
  ma.stream      = (hipStream_t)stream;
  return run_class(plans, first, n);
}

static int moddown_fwd_launch(ntt_plan *const *plans, int first, int n, int nq, int np, uint64_t *d_a, uint64_t batch, bool floor_div,
                              void *stream, const Layout &lay, const uint64_t *pr)
{
  const std::vector<unsigned char> recs = rns_records(plans, first, n);
  ModDownFwdArgs                   ma{};
  const int                        kc = moddown_fwd_args(ma, recs, plans, first, n, nq, np, d_a, batch, stream, lay);
  bconv_sources(pr, np, !floor_div, ma.pl);
  for(int l = 0; l < n; l++) {
    uint64_t g[kBconvLimbs]; /* (formed again by the kernel's workgroups: no room for the table in its arguments) */
    ma.ql[l] = moddown_dst(plans[first + l]->q, pr, np, floor_div, g);
  }
  const hipError_t e = with_f64_class(kc, [&](auto k) { return launch_moddown_fwd<typename decltype(k)::A, decltype(k)::KSH>(ma); });
  if(e != hipSuccess) return fail(NTT_ERR_HIP, std::string("moddown_fwd_kernel: ") + hipGetErrorString(e));
  return NTT_OK;
}

/* The route of every ModDown call (ntt_rns_mod_down_batch, _add_, _bgv_, _bgv_add_, _exact_) behind its own argument checks.  What
 * differs comes in as
 *   kind(p)              how the run whose first plan is p is served (ModDownRun);
 *   coef(first, n, pr)   the coefficient kernel over Q limbs [first, first + n) of d_a, in place;
 *   fused(k, first, n, pr)   the fused kernel of kind k over the run;
 *   fold(first, n)       d_c's limbs (+)= d_a's where the result was left in d_a (moddown_no_fold: the in-place calls);
 *   overlap              the error text if d_c overlaps d_a, else null -- formed by the caller, reported here in its place.
 * pr: the P primes. */
enum ModDownRun {
  kModDownSandwich,  /* the inverse over the run, coef, the forward over the run; then fold */
  kModDownFusedHere, /* fused, the result in d_a's Q limbs; then fold                     */
  kModDownFusedInto  /* fused, the result where the call wants it: no fold                */
};
static int moddown_no_fold(int, int) { return NTT_OK; }

template <class Kind, class Coef, class Fused, class Fold>
static int moddown_route(int nq, int np, ntt_plan *const *plans, uint64_t *d_a, uint64_t batch, bool ntt_dom, void *stream, const Layout &alay,
                         const char *overlap, Kind kind, Coef coef, Fused fused, Fold fold)
{
  const int                              nlimbs = nq + np;
  const std::vector<std::pair<int, int>> runs   = rns_runs(nq, plans);
  std::vector<ModDownRun>                kinds(runs.size(), kModDownSandwich);
  if(ntt_dom) {
    /* every table the call will need, before anything is written */
    for(int j = nq; j < nlimbs; j++) {
      if(!plans[j]->has_inv) return fail(NTT_ERR_ARG, "a P limb's plan lacks the inverse table");
    }
    for(size_t r = 0; r < runs.size(); r++) {
      kinds[r] = kind(plans[runs[r].first]);
      for(int l = runs[r].first; l < runs[r].first + runs[r].second; l++) {
        if(!plans[l]->has_fwd) return fail(NTT_ERR_ARG, "a Q limb's plan lacks the forward table");
        if(kinds[r] == kModDownSandwich && !plans[l]->has_inv) return fail(NTT_ERR_ARG, "a Q limb's plan lacks the inverse table (sandwich route)");
      }
    }
  }
  if(batch == 0) return NTT_OK;
  if(overlap) return fail(NTT_ERR_ARG, overlap);
  USE_DEVICE(plans[0]->device);
  uint64_t pr[kBconvLimbs];
  for(int j = 0; j < np; j++) pr[j] = plans[nq + j]->q;
  const Layout one{alay.limb, alay.poly};
  int          rc = NTT_OK;
  if(!ntt_dom) {
    for(int first = 0; !rc && first < nq; first += kBconvLimbs) rc = coef(first, nq - first < kBconvLimbs ? nq - first : kBconvLimbs, pr);
    if(!rc) rc = fold(0, nq);
    return rc;
  }
  rc = rns_transform(np, plans + nq, d_a + (uint64_t)nq * alay.limb, batch, true, stream, one);
  for(size_t r = 0; !rc && r < runs.size(); r++) {
    const int first = runs[r].first, n = runs[r].second;
    if(kinds[r] != kModDownSandwich) {
      rc = fused(kinds[r], first, n, pr);
      if(kinds[r] == kModDownFusedInto) continue;
    } else {
      uint64_t *c = d_a + (uint64_t)first * alay.limb;
      rc          = rns_transform(n, plans + first, c, batch, true, stream, one);
      if(!rc) rc = coef(first, n, pr);
      if(!rc) rc = rns_transform(n, plans + first, c, batch, false, stream, one);
    }
    if(!rc) rc = fold(first, n);
  }
  return rc;
}

static int rns_mod_down(int nq, int np, ntt_plan *const *plans, uint64_t *d_a, uint64_t batch, unsigned flags, void *stream,
                        const Layout &lay)
{
  if(nq < 1 || np < 1 || np > kBconvLimbs) return fail(NTT_ERR_ARG, "ModDown needs 1 <= nq and 1 <= np <= 16");
  const int nlimbs = nq + np;
  int       rc     = rns_check(nlimbs, plans);
  if(rc) return rc;
  if(flags & ~(unsigned)(NTT_MODDOWN_TRANSFORMED | NTT_MODDOWN_FLOOR)) return fail(NTT_ERR_ARG, "unknown flag");
  if(!d_a) return fail(NTT_ERR_ARG, "null argument");
  rc = layout_check(plans[0]->N, nlimbs, batch, lay);
  if(!rc) rc = distinct_primes(nlimbs, plans);
  if(rc) return rc;
  const bool floor_div = (flags & NTT_MODDOWN_FLOOR) != 0;
  return moddown_route(
    nq, np, plans, d_a, batch, (flags & NTT_MODDOWN_TRANSFORMED) != 0, stream, lay, nullptr,
    [&](const ntt_plan *p) { return rescale_fused_applies(plans[0], p) ? kModDownFusedHere : kModDownSandwich; },
    [&](int first, int n, const uint64_t *pr) { return moddown_coef_launch(plans, first, n, nq, np, d_a, batch, floor_div, stream, lay, pr); },
    [&](ModDownRun, int first, int n, const uint64_t *pr) { return moddown_fwd_launch(plans, first, n, nq, np, d_a, batch, floor_div, stream, lay, pr); },
    moddown_no_fold);
}

extern "C" int ntt_rns_mod_down_batch(int nq, int np, ntt_plan *const *plans, uint64_t *d_a, uint64_t batch, unsigned flags, void *stream)
{
  return rns_mod_down(nq, np, plans, d_a, batch, flags, stream, limb_major(plans, nq + np, batch));
}

extern "C" int ntt_rns_mod_down_batch_strided(int nq, int np, ntt_plan *const *plans, uint64_t *d_a, uint64_t limb_stride,
                                              uint64_t poly_stride, uint64_t batch, unsigned flags, void *stream)
{
  return rns_mod_down(nq, np, plans, d_a, batch, flags, stream, Layout{limb_stride, poly_stride});
}
