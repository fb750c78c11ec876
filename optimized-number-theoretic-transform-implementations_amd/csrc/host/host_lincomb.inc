/* host/host_lincomb.inc -- the evaluator's linear layer: ntt_rns_lincomb_batch and its strided form.  A section of ntt_host.hip (one
 * translation unit, included from there in order); not compiled by itself.  The kernel is in lincomb.hip; this section sees its
 * launcher and argument record only (ntt_lincomb.h).
 *
 *   lincomb   c (+)= bias + sum_{i<k} sigma_{g_i}(a_i) * mu_i per limb and word, mu_i a polynomial multiplier or a per-limb scalar:
 *             lincomb_kernel, one launch per 16 limbs, integer arithmetic for every policy and every N >= 2.
 * Everything is checked before the first launch.  Nothing is allocated, the host is not synchronised and no memset is issued: the
 * call can be captured into a graph. */

static int rns_lincomb(int nlimbs, ntt_plan *const *plans, uint64_t *d_c, int k, const uint64_t *const *d_a, const uint64_t *const *d_m,
                       const uint64_t *h_s, const uint64_t *h_g, const uint64_t *h_bias, uint64_t batch, unsigned flags, void *stream,
                       const Layout &lay)
{
  int rc = rns_check(nlimbs, plans);
  if(rc) return rc;
  if(flags & ~(unsigned)(NTT_LINCOMB_ACCUMULATE | NTT_LINCOMB_M_BROADCAST | NTT_LINCOMB_LAZY_IN)) return fail(NTT_ERR_ARG, "unknown flag");
  const bool lazy = (flags & NTT_LINCOMB_LAZY_IN) != 0, bcast = (flags & NTT_LINCOMB_M_BROADCAST) != 0;
  if(k < 1 || k > (lazy ? kLincombTerms / 2 : kLincombTerms))
    return fail(NTT_ERR_ARG, lazy ? "lincomb: number of terms must be 1 .. 8 with NTT_LINCOMB_LAZY_IN" : "lincomb: number of terms must be 1 .. 16");
  if(!d_c || !d_a) return fail(NTT_ERR_ARG, "null argument");
  int nm = 0;
  for(int i = 0; i < k; i++) {
    if(!d_a[i]) return fail(NTT_ERR_ARG, "null operand"); /* (before any limb offset is added) */
    if(d_m && d_m[i]) nm++;
  }
  if(bcast && !nm) return fail(NTT_ERR_ARG, "lincomb: NTT_LINCOMB_M_BROADCAST without a polynomial multiplier");
  if(plans[0]->m < 1 || plans[0]->m > 30) return fail(NTT_ERR_ARG, "lincomb: N out of range");
  const uint64_t N = plans[0]->N;
  for(int i = 0; i < k; i++) {
    const uint64_t g = h_g ? h_g[i] : 1;
    if(!(g & 1) || g >= 2 * N) return fail(NTT_ERR_ARG, "lincomb: g must be odd and below 2N");
    if(h_s && !(d_m && d_m[i])) {
      for(int l = 0; l < nlimbs; l++)
        if(h_s[(size_t)i * nlimbs + l] >= plans[l]->q) return fail(NTT_ERR_ARG, "lincomb: a scalar is not below its prime");
    }
  }
  for(int l = 0; h_bias && l < nlimbs; l++)
    if(h_bias[l] >= plans[l]->q) return fail(NTT_ERR_ARG, "lincomb: a bias is not below its prime");
  rc = layout_check(N, nlimbs, batch, lay);
  if(rc || batch == 0) return rc;
  /* a multiplier shared by the batch is [limb][N] */
  const uint64_t   mls = bcast ? N : lay.limb, mps = bcast ? 0 : lay.poly;
  const GaloisSpan out = galois_span(d_c, N, nlimbs, batch, lay.limb, lay.poly);
  for(int i = 0; i < k; i++) {
    /* c may BE a_i where g_i = 1, or m_i in c's layout (every thread reads all its words before it stores its own position); a
     * permuted read of c, a multiplier shared by the batch and any shifted overlap are refused */
    const bool same_a = d_a[i] == d_c && (h_g ? h_g[i] : 1) == 1;
    if(!same_a && galois_overlap(out, galois_span(d_a[i], N, nlimbs, batch, lay.limb, lay.poly)))
      return fail(NTT_ERR_ARG, d_a[i] == d_c ? "lincomb: d_c is an a_i whose g is not 1" : "lincomb: d_c overlaps an a_i it is not identical to");
    if(!(d_m && d_m[i])) continue;
    const bool same_m = d_m[i] == d_c && !bcast;
    if(!same_m && galois_overlap(out, galois_span(d_m[i], N, nlimbs, bcast ? 1 : batch, mls, mps)))
      return fail(NTT_ERR_ARG, "lincomb: d_c overlaps a multiplier it is not identical to");
  }
  USE_DEVICE(plans[0]->device);
  LincombArgs la{};
  la.k             = k;
  la.limb_stride   = lay.limb;
  la.poly_stride   = lay.poly;
  la.m_limb_stride = mls;
  la.m_poly_stride = mps;
  la.batch         = batch;
  la.logn          = (uint32_t)plans[0]->m;
  la.accumulate    = (flags & NTT_LINCOMB_ACCUMULATE) != 0;
  la.max_grid      = plans[0]->max_grid;
  la.stream        = (hipStream_t)stream;
  for(int first = 0; first < nlimbs; first += kLincombLimbs) {
    la.nlimbs = nlimbs - first < kLincombLimbs ? nlimbs - first : kLincombLimbs;
    la.c      = d_c + (uint64_t)first * lay.limb;
    for(int i = 0; i < k; i++) {
      la.t[i].a = d_a[i] + (uint64_t)first * lay.limb;
      la.t[i].m = (d_m && d_m[i]) ? d_m[i] + (uint64_t)first * mls : nullptr;
      la.t[i].g = (uint32_t)(h_g ? h_g[i] : 1);
      for(int l = 0; l < la.nlimbs; l++) la.scalars[i][l] = h_s ? h_s[(size_t)i * nlimbs + first + l] : 1;
    }
    for(int l = 0; l < la.nlimbs; l++) {
      la.ql[l]   = bconv_dst(plans[first + l]->q);
      la.bias[l] = h_bias ? h_bias[first + l] : 0;
    }
    const hipError_t e = launch_lincomb(la);
    if(e != hipSuccess) return fail(NTT_ERR_HIP, std::string("lincomb_kernel: ") + hipGetErrorString(e));
  }
  return NTT_OK;
}

extern "C" int ntt_rns_lincomb_batch(int nlimbs, ntt_plan *const *plans, uint64_t *d_c, int k, const uint64_t *const *d_a,
                                     const uint64_t *const *d_m, const uint64_t *h_s, const uint64_t *h_g, const uint64_t *h_bias, uint64_t batch,
                                     unsigned flags, void *stream)
{
  return rns_lincomb(nlimbs, plans, d_c, k, d_a, d_m, h_s, h_g, h_bias, batch, flags, stream, limb_major(plans, nlimbs, batch));
}

extern "C" int ntt_rns_lincomb_batch_strided(int nlimbs, ntt_plan *const *plans, uint64_t *d_c, int k, const uint64_t *const *d_a,
                                             const uint64_t *const *d_m, const uint64_t *h_s, const uint64_t *h_g, const uint64_t *h_bias,
                                             uint64_t limb_stride, uint64_t poly_stride, uint64_t batch, unsigned flags, void *stream)
{
  return rns_lincomb(nlimbs, plans, d_c, k, d_a, d_m, h_s, h_g, h_bias, batch, flags, stream, Layout{limb_stride, poly_stride});
}
