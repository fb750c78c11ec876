/* host/host_produce.inc -- the one host route of the calls that produce a polynomial into the RNS: the lifts (host_lift.inc) and the
 * device-side sampler (host_sample.inc).  A section of ntt_host.hip (one translation unit, included from there in order); not compiled by
 * itself.  The kernels share one frame too (ntt_kernels_produce.h).
 *
 *   coefficients   the family's coefficient kernel, one launch per 16 limbs; integer arithmetic of its own for every policy and every
 *                  N >= 2.
 *   NTT domain     per run of compatible limbs (rns_runs):
 *                  fused        where the family's rule allows it (FP64 policies at N = 2^6..2^14: produce_fused_built): ONE launch of
 *                               its fused kernel;
 *                  composition  anything else (integer or radix-4 plans, N < 2^6, N >= 2^15, the family's option 0): the coefficient
 *                               kernel and the forward transform over the run in place; accumulating, the inverse transform over the run
 *                               first (c is canonical on both sides of every step, so the words are those of the fused kernel).
 * Everything is checked before the first launch.  Nothing is allocated, the host is not synchronised and no memset is issued: the calls
 * can be captured into a graph.
 *
 * An entry keeps its own checks in front of produce_check, and between produce_check and produce_route what has its place there; the
 * first failing check decides the text a caller reads, so the order is part of the interface. */

/* where the fused kernels are built */
static bool produce_fused_built(const ntt_plan *p) { return p->arith == NTT_ARITH_F64 && !p->generic && p->m >= kFusedMin && p->m <= kFusedMax; }

/* The checks every producer makes, in their order: the limb list, N, per limb q < 2^61 and then limb_check(l) -- the family's own
 * condition on limb l as an error text, or null --, the operands, the output's layout.  `name` leads the family's texts. */
template <class LimbCheck>
static int produce_check(const std::string &name, int nlimbs, ntt_plan *const *plans, bool operands, uint64_t batch, const Layout &lay,
                         LimbCheck limb_check)
{
  const int rc = rns_check(nlimbs, plans);
  if(rc) return rc;
  if(plans[0]->m < 1 || plans[0]->m > 30) return fail(NTT_ERR_ARG, name + ": N out of range");
  for(int l = 0; l < nlimbs; l++) {
    if(plans[l]->q >= (1ull << 61)) return fail(NTT_ERR_ARG, name + ": every prime must be below 2^61");
    if(const char *own = limb_check(l)) return fail(NTT_ERR_ARG, own);
  }
  if(batch > 0 && !operands) return fail(NTT_ERR_ARG, "null argument");
  return layout_check(plans[0]->N, nlimbs, batch, lay);
}
static const char *produce_any_limb(int) { return nullptr; }

/* the fields every producer's launch carries (ProduceArgs): limbs [first, first + n) of d_c with their constants, and the geometry of
 * plan p -- plans[0] for the coefficient kernel, the run's first plan for the fused one */
template <class Args>
static void produce_args(Args &pa, const ntt_plan *p, int first, int n, uint64_t *d_c, const BconvDst *ll, uint64_t batch, void *stream,
                         const Layout &lay)
{
  pa.c           = d_c + (uint64_t)first * lay.limb;
  pa.nlimbs      = n;
  pa.limb_stride = lay.limb;
  pa.poly_stride = lay.poly;
  pa.batch       = batch;
  pa.logn        = (uint32_t)p->m;
  for(int i = 0; i < n; i++) pa.ll[i] = ll[first + i];
  pa.max_grid = p->max_grid;
  pa.num_cus  = p->num_cus;
  pa.stream   = (hipStream_t)stream;
}

/* what a producer's launcher returned, as the status of the call */
static int produce_launched(const char *kernel, hipError_t e)
{
  if(e != hipSuccess) return fail(NTT_ERR_HIP, std::string(kernel) + ": " + hipGetErrorString(e));
  return NTT_OK;
}

/* The route behind the checks.  What differs comes in as
 *   fused_applies(run)     whether the run {first, count} is served by the fused kernel;
 *   coef_launch(first, n)  the coefficient kernel over limbs [first, first + n) of d_c;
 *   fwd_launch(first, n)   the fused kernel over the run;
 *   overlap                the error text if an operand overlaps d_c, else null -- formed by the caller, reported here in its place. */
template <class Fused, class Coef, class Fwd>
static int produce_route(const std::string &name, int nlimbs, ntt_plan *const *plans, uint64_t *d_c, uint64_t batch, bool ntt_dom, bool acc,
                         void *stream, const Layout &lay, const char *overlap, Fused fused_applies, Coef coef_launch, Fwd fwd_launch)
{
  const std::vector<std::pair<int, int>> runs = rns_runs(nlimbs, plans);
  if(ntt_dom) {
    /* every table the call will need, before anything is written */
    for(const std::pair<int, int> &run : runs) {
      const bool fused = fused_applies(run);
      for(int l = run.first; l < run.first + run.second; l++) {
        if(!plans[l]->has_fwd) return fail(NTT_ERR_ARG, name + ": a limb's plan lacks the forward table");
        if(!fused && acc && !plans[l]->has_inv) return fail(NTT_ERR_ARG, name + ": a limb's plan lacks the inverse table (composed accumulation)");
      }
    }
  }
  if(batch == 0) return NTT_OK;
  if(overlap) return fail(NTT_ERR_ARG, overlap);
  USE_DEVICE(plans[0]->device);
  int rc = NTT_OK;
  if(!ntt_dom) {
    for(int first = 0; !rc && first < nlimbs; first += kProduceLimbs) rc = coef_launch(first, nlimbs - first < kProduceLimbs ? nlimbs - first : kProduceLimbs);
    return rc;
  }
  const Layout one{lay.limb, lay.poly};
  for(const std::pair<int, int> &run : runs) {
    if(rc) break;
    const int first = run.first, n = run.second;
    if(fused_applies(run)) {
      rc = fwd_launch(first, n);
      continue;
    }
    uint64_t *c = d_c + (uint64_t)first * lay.limb;
    if(acc) rc = rns_transform(n, plans + first, c, batch, true, stream, one);
    if(!rc) rc = coef_launch(first, n);
    if(!rc) rc = rns_transform(n, plans + first, c, batch, false, stream, one);
  }
  return rc;
}
