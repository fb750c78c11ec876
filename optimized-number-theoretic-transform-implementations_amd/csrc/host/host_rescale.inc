/* host/host_rescale.inc -- the RNS rescale (modulus drop): ntt_rns_rescale_batch and its strided form.
 * A section of ntt_host.hip (one translation unit, included from there in order); not compiled by itself.  The kernels are in the
 * rescale_*.hip units; this section sees their launchers only (ntt_rescale.h).
 *
 * Limbs 0 .. L-1 of an RNS polynomial with primes q_0 .. q_L become round(x / q_L) (floor with NTT_RESCALE_FLOOR) mod Q / q_L:
 *   coefficients   rescale_coef_kernel, one launch per 16 kept limbs (t read once per launch): 8N(2L+1) bytes;
 *   NTT domain     the inverse transform of limb L (t stays in its slot), then per run of compatible kept limbs (rns_runs):
 *                  FP64 policies at N = 2^6..2^14 -- rescale_fwd_kernel, ONE launch per run: 8N(2L+3) bytes in all;
 *                  anything else (integer or radix-4 plans, N < 2^6, N >= 2^15, NTT_OPT_RESCALE_FUSED 0) -- the sandwich: the
 *                  inverse over the run, rescale_coef_kernel, the forward over the run.
 * Nothing is allocated, the host is not synchronised and no memset is issued: the call can be captured into a graph. */

/* kept limb l's constants for the dropped prime qL */
static RescaleLimb rescale_limb(uint64_t q, uint64_t qL, bool floor_div)
{
  RescaleLimb r{};
  r.q       = q;
  r.bar     = ~0ull / q; /* = floor(2^64 / q): q is odd */
  r.s       = h_powmod(qL % q, q - 2, q);
  r.s_shoup = (uint64_t)(((unsigned __int128)r.s << 64) / q);
  r.h       = floor_div ? 0 : ((qL - 1) / 2) % q;
  return r;
}

/* the fused NTT-domain route for a run whose first plan is p: the FP64 policies on whole-polynomial blocks, the option on
 * (NTT_OPT_RESCALE_FUSED, read from plans[0]) */
static bool rescale_fused_applies(const ntt_plan *p0, const ntt_plan *p)
{
  return p0->rescale_fused != 0 && p->arith == NTT_ARITH_F64 && !p->generic && p->m >= kFusedMin && p->m <= kFusedMax;
}

static int rescale_coef_launch(ntt_plan *const *plans, int first, int n, uint64_t *d_a, uint64_t batch, uint64_t qL, bool floor_div,
                               void *stream, const Layout &lay, int last)
{
  RescaleCoefArgs ra{};
  ra.c           = d_a + (uint64_t)first * lay.limb;
  ra.t           = d_a + (uint64_t)last * lay.limb;
  ra.limb_stride = lay.limb;
  ra.poly_stride = lay.poly;
  ra.batch       = batch;
  ra.logn        = (uint32_t)plans[0]->m;
  ra.nlimbs      = n;
  ra.qL          = qL;
  ra.hL          = floor_div ? 0 : (qL - 1) / 2;
  for(int i = 0; i < n; i++) ra.limbs[i] = rescale_limb(plans[first + i]->q, qL, floor_div);
  ra.max_grid = plans[0]->max_grid;
  ra.stream   = (hipStream_t)stream;
  HIP_TRY(launch_rescale_coef(ra));
  return NTT_OK;
}

static int rescale_fwd_launch(ntt_plan *const *plans, int first, int n, uint64_t *d_a, uint64_t batch, uint64_t qL, bool floor_div,
                              void *stream, const Layout &lay, int last)
{
  const std::vector<unsigned char> recs = rns_records(plans, first, n);
  RescaleFwdArgs                   ra{};
  ra.c           = d_a + (uint64_t)first * lay.limb;
  ra.t           = d_a + (uint64_t)last * lay.limb;
  ra.limbs       = recs.data();
  ra.nlimbs      = n;
  ra.limb_stride = lay.limb;
  ra.poly_stride = lay.poly;
  ra.batch       = batch;
  ra.logn        = (uint32_t)plans[first]->m;
  ra.qL          = qL;
  ra.hL          = floor_div ? 0 : (qL - 1) / 2;
  for(int i = 0; i < n; i++) ra.rl[i] = rescale_limb(plans[first + i]->q, qL, floor_div);
  ra.max_grid = plans[first]->max_grid;
  ra.num_cus  = plans[first]->num_cus;
  ra.stream   = (hipStream_t)stream;
  const hipError_t e = with_f64_class(run_class(plans, first, n), [&](auto k) { return launch_rescale_fwd<typename decltype(k)::A, decltype(k)::KSH>(ra); });
  if(e != hipSuccess) return fail(NTT_ERR_HIP, std::string("rescale_fwd_kernel: ") + hipGetErrorString(e));
  return NTT_OK;
}

static int rns_rescale(int nlimbs, ntt_plan *const *plans, uint64_t *d_a, uint64_t batch, unsigned flags, void *stream, const Layout &lay)
{
  if(nlimbs < 2) return fail(NTT_ERR_ARG, "a rescale needs at least two limbs");
  int rc = rns_check(nlimbs, plans);
  if(rc) return rc;
  if(flags & ~(unsigned)(NTT_RESCALE_TRANSFORMED | NTT_RESCALE_FLOOR)) return fail(NTT_ERR_ARG, "unknown flag");
  if(!d_a) return fail(NTT_ERR_ARG, "null argument");
  rc = layout_check(plans[0]->N, nlimbs, batch, lay);
  if(rc) return rc;
  const int       L         = nlimbs - 1;
  const ntt_plan *pL        = plans[L];
  const bool      ntt_dom   = (flags & NTT_RESCALE_TRANSFORMED) != 0;
  const bool      floor_div = (flags & NTT_RESCALE_FLOOR) != 0;
  for(int l = 0; l < L; l++) {
    if(plans[l]->q == pL->q) return fail(NTT_ERR_ARG, "the dropped prime equals a kept prime");
  }
  const std::vector<std::pair<int, int>> runs = rns_runs(L, plans);
  if(ntt_dom) {
    /* every table the call will need, before anything is written */
    if(!pL->has_inv) return fail(NTT_ERR_ARG, "the dropped limb's plan lacks the inverse table");
    for(const std::pair<int, int> &run : runs) {
      const bool fused = rescale_fused_applies(plans[0], plans[run.first]);
      for(int l = run.first; l < run.first + run.second; l++) {
        if(!plans[l]->has_fwd) return fail(NTT_ERR_ARG, "a kept limb's plan lacks the forward table");
        if(!fused && !plans[l]->has_inv) return fail(NTT_ERR_ARG, "a kept limb's plan lacks the inverse table (sandwich route)");
      }
    }
  }
  if(batch == 0) return NTT_OK;
  USE_DEVICE(plans[0]->device);
  const uint64_t qL  = pL->q;
  const Layout   one{lay.limb, lay.poly};
  if(!ntt_dom) {
    for(int first = 0; !rc && first < L; first += kRescaleLimbs) {
      rc = rescale_coef_launch(plans, first, L - first < kRescaleLimbs ? L - first : kRescaleLimbs, d_a, batch, qL, floor_div, stream, lay, L);
    }
    return rc;
  }
  rc = rns_transform(1, plans + L, d_a + (uint64_t)L * lay.limb, batch, true, stream, one);
  for(const std::pair<int, int> &run : runs) {
    if(rc) break;
    const int first = run.first, n = run.second;
    if(rescale_fused_applies(plans[0], plans[first])) {
      rc = rescale_fwd_launch(plans, first, n, d_a, batch, qL, floor_div, stream, lay, L);
      continue;
    }
    uint64_t *c = d_a + (uint64_t)first * lay.limb;
    rc          = rns_transform(n, plans + first, c, batch, true, stream, one);
    if(!rc) rc = rescale_coef_launch(plans, first, n, d_a, batch, qL, floor_div, stream, lay, L);
    if(!rc) rc = rns_transform(n, plans + first, c, batch, false, stream, one);
  }
  return rc;
}

extern "C" int ntt_rns_rescale_batch(int nlimbs, ntt_plan *const *plans, uint64_t *d_a, uint64_t batch, unsigned flags, void *stream)
{
  return rns_rescale(nlimbs, plans, d_a, batch, flags, stream, limb_major(plans, nlimbs, batch));
}

extern "C" int ntt_rns_rescale_batch_strided(int nlimbs, ntt_plan *const *plans, uint64_t *d_a, uint64_t limb_stride, uint64_t poly_stride,
                                             uint64_t batch, unsigned flags, void *stream)
{
  return rns_rescale(nlimbs, plans, d_a, batch, flags, stream, Layout{limb_stride, poly_stride});
}
