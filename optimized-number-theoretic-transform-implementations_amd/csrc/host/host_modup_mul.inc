/* host/host_modup_mul.inc -- one digit's term of the key-switching inner product in one call: ntt_rns_mod_up_mul_batch and its strided
 * form, c^ (+)= fwd(ModUp(digit)) (.) key^ over every limb of the extended basis.  A section of ntt_host.hip (one translation unit,
 * included from there in order); not compiled by itself.  The kernel is in the modup_mul_f64*.hip units; this section sees its
 * launchers only (ntt_keyswitch.h).  modup_mul_launch also serves the pair form of host_key_pair.inc.
 *
 * Per run of compatible limbs (rns_runs):
 *   fused        FP64 policies, N = 2^6..2^14, where NTT_OPT_MODUP_FUSED on plans[0] allows it: ONE modup_mul_kernel launch -- the base
 *                conversion in the prologue of the forward block stages, the key product in their epilogue.  The extended digit is
 *                never written: 8N count + 8N (key) + 8N or 16N (c^) bytes per limb-polynomial.
 *   composition  anything else: bconv_kernel into the operand's other slots of the run (ntt_rns_mod_up_batch's launches, restricted
 *                to the limbs that need them), then the ntt_rns_fwd_mul_batch route over the run.
 * Every read of the digit by a base conversion -- the bconv launches, then the fused launches -- is issued in front of the first
 * forward-multiply of a composition run, which may use its limbs of the operand as scratch.  With every run on the composition the
 * launches are exactly those of the two calls.  Nothing is allocated, the host is not synchronised and no memset is issued. */

static bool modup_mul_built(const ntt_plan *p)
{
  return p->arith == NTT_ARITH_F64 && !p->generic && p->m >= kFusedMin && p->m <= kFusedMax;
}

/* The automatic choice (NTT_OPT_MODUP_FUSED -1), from profiles/r10/modup_mul_bench.txt (24 limbs of 50-bit primes, broadcast key,
 * accumulating; the call rate of the fused route over that of the parent commit's ntt_rns_mod_up_batch + ntt_rns_fwd_mul_batch,
 * ranges over eight rounds of alternating processes):
 *     count   2^14 x 2     2^14 x 64    2^14 x 1024   2^13 x 2     2^13 x 64    2^13 x 1024
 *       1     1.22-1.33    1.86-1.96    1.47-1.49     1.22-1.29    1.67-1.78    1.65-1.70
 *       2     0.70-0.74    1.10-1.13    0.85-0.86     0.69-0.72    1.05-1.09    0.93-0.95
 *       3     0.59-0.64    0.96-0.99    0.73-0.74     0.61-0.63    0.93-0.98    0.79-0.81
 *       4     0.54-0.59    0.84-0.85    0.65-0.65     0.55-0.57    0.83-0.85    0.70-0.71
 *       8     0.35-0.37    0.52-0.54    0.41-0.42     0.37-0.38    0.52-0.53    0.45-0.45
 * The fused call's time grows by about 1.0 ms per source limb at 2^14 x 1024 (2.23 ms at count 1, 9.17 ms at count 8), the two calls'
 * by 0.07 ms: per destination limb the fused kernel re-reads the digit (3.2 GB per source limb there if no cache holds it) and repeats
 * its conversion (a Shoup product and a 128-bit multiply-add per source limb and coefficient), where bconv_kernel does both once per
 * 16 destination limbs; which of the two bounds it has not been measured.  C, the largest count at which the fused call was not
 * slower than the two calls at both 64 and 1024 polynomials at 2^14, is 1.  The 2-polynomial rows show no gain beyond it (0.70-0.74 at
 * count 2), so there is no launch-bound extension of the rule: fused for count == 1, the composition otherwise. */
static bool modup_fused_pays(int count) { return count <= 1; }

static bool modup_fused_applies(const ntt_plan *p0, const ntt_plan *p, int count)
{
  if(!modup_mul_built(p)) return false;
  if(p0->modup_fused >= 0) return p0->modup_fused == 1;
  return modup_fused_pays(count);
}

/* ONE launch of the fused kernel over the run [rf, rf + rn): ncomp = 1 modup_mul_kernel (c[0] (+)= .. key[0]), ncomp = 2 modup_mul2_kernel
 * (both components; host_key_pair.inc).  x is the extended operand, the digit its limbs [first, first + count).  count = 0 is
 * host_key_pair.inc's fwd_mul_pair: no conversion, every limb of the run is its own digit limb and the kernel's count is 1. */
static int modup_mul_launch(ntt_plan *const *plans, int rf, int rn, int first, int count, int ncomp, uint64_t *const *c, uint64_t *x,
                            const uint64_t *const *key, uint64_t bslab, uint64_t batch, unsigned flags, void *stream, const Layout &lay,
                            const BconvSrc *sl)
{
  const std::vector<unsigned char> recs = rns_records(plans, rf, rn);
  ModUpMulArgs                     ma{};
  ma.a     = x + (uint64_t)rf * lay.limb;
  ma.dig   = x + (uint64_t)first * lay.limb;
  ma.ncomp = ncomp;
  for(int j = 0; j < ncomp; j++) {
    ma.b[j]   = key[j] + (uint64_t)rf * bslab;
    ma.out[j] = c[j] + (uint64_t)rf * lay.limb;
  }
  ma.limbs         = recs.data();
  ma.nlimbs        = rn;
  ma.count         = count ? count : 1;
  ma.limb_stride   = lay.limb;
  ma.poly_stride   = lay.poly;
  ma.b_limb_stride = bslab;
  ma.batch         = batch;
  ma.logn          = (uint32_t)plans[rf]->m;
  ma.lazy_in       = (flags & NTT_MUL_LAZY_IN) != 0;
  ma.b_bcast       = (flags & NTT_MUL_B_BROADCAST) != 0;
  ma.accumulate    = (flags & NTT_MUL_ACCUMULATE) != 0;
  for(int i = 0; i < count; i++) ma.sl[i] = sl[i];
  for(int l = 0; l < rn; l++) {
    ma.dl[l] = bconv_dst(plans[rf + l]->q);
    if(!count || (rf + l >= first && rf + l < first + count)) ma.own |= 1u << l;
  }
  ma.max_grid = plans[rf]->max_grid;
  ma.num_cus  = plans[rf]->num_cus;
  ma.stream   = (hipStream_t)stream;
  const hipError_t e = with_int<1, 2>(ncomp, hipErrorInvalidValue, [&](auto nc) {
    return with_f64_class(run_class(plans, rf, rn), [&](auto k) { return launch_modup_mul<typename decltype(k)::A, decltype(k)::KSH, decltype(nc)::value>(ma); });
  });
  if(e != hipSuccess) return fail(NTT_ERR_HIP, std::string(ncomp == 2 ? "modup_mul2_kernel: " : "modup_mul_kernel: ") + hipGetErrorString(e));
  return NTT_OK;
}

static int rns_mod_up_mul(int nlimbs, ntt_plan *const *plans, uint64_t *d_c, uint64_t *d_ext, int first, int count, const uint64_t *d_keyhat,
                          uint64_t batch, unsigned flags, void *stream, const Layout &lay)
{
  int rc = rns_check(nlimbs, plans);
  if(rc) return rc;
  if(count < 1 || count > kBconvLimbs || first < 0 || first > nlimbs - count) return fail(NTT_ERR_ARG, "the digit's limbs are out of range");
  if(flags & ~(unsigned)(NTT_MUL_LAZY_IN | NTT_MUL_B_BROADCAST | NTT_MUL_ACCUMULATE)) return fail(NTT_ERR_ARG, "unknown flag");
  if(!d_c || !d_ext || !d_keyhat) return fail(NTT_ERR_ARG, "null argument");
  rc = layout_check(plans[0]->N, nlimbs, batch, lay);
  if(!rc) rc = distinct_primes(nlimbs, plans);
  if(rc) return rc;
  for(int l = 0; l < nlimbs; l++) {
    if(!plans[l]->has_fwd) return fail(NTT_ERR_ARG, "a limb's plan lacks the forward table");
  }
  if(batch == 0) return NTT_OK;
  const uint64_t N = plans[0]->N;
  /* every limb's workgroups read the digit while others write c^ */
  if(galois_overlap(galois_span(d_c, N, nlimbs, batch, lay.limb, lay.poly), galois_span(d_ext, N, nlimbs, batch, lay.limb, lay.poly)))
    return fail(NTT_ERR_ARG, "mod_up_mul: c^ overlaps the extended operand");
  USE_DEVICE(plans[0]->device);
  const uint64_t bslab = (flags & NTT_MUL_B_BROADCAST) ? N : lay.limb; /* a broadcast key is [limb][N] */
  uint64_t       b[kBconvLimbs];
  BconvArgs      ba{};
  modup_args(plans, d_ext, first, count, batch, stream, lay, b, ba);
  const std::vector<std::pair<int, int>> runs = rns_runs(nlimbs, plans);
  std::vector<char>                      fused(runs.size(), 0);
  for(size_t r = 0; r < runs.size(); r++) fused[r] = modup_fused_applies(plans[0], plans[runs[r].first], count) ? 1 : 0;
  /* the composition runs' destination limbs as ranges of ModUp's destination index */
  const std::vector<std::pair<int, int>> dst = modup_dst_ranges(runs, fused, first, count);
  rc = modup_launches(plans, b, ba, dst.data(), dst.size());
  for(size_t r = 0; !rc && r < runs.size(); r++) {
    if(fused[r]) rc = modup_mul_launch(plans, runs[r].first, runs[r].second, first, count, 1, &d_c, d_ext, &d_keyhat, bslab, batch, flags, stream, lay, ba.sl);
  }
  for(size_t r = 0; !rc && r < runs.size(); r++) {
    if(fused[r]) continue;
    const int rf = runs[r].first, rn = runs[r].second;
    rc = rns_fwd_mul(rn, plans + rf, d_c + (uint64_t)rf * lay.limb, d_ext + (uint64_t)rf * lay.limb, d_keyhat + (uint64_t)rf * bslab, batch, flags, stream,
                     lay);
  }
  return rc;
}

extern "C" int ntt_rns_mod_up_mul_batch(int nlimbs, ntt_plan *const *plans, uint64_t *d_c, uint64_t *d_ext, int first, int count,
                                        const uint64_t *d_keyhat, uint64_t batch, unsigned flags, void *stream)
{
  return rns_mod_up_mul(nlimbs, plans, d_c, d_ext, first, count, d_keyhat, batch, flags, stream, limb_major(plans, nlimbs, batch));
}

extern "C" int ntt_rns_mod_up_mul_batch_strided(int nlimbs, ntt_plan *const *plans, uint64_t *d_c, uint64_t *d_ext, int first, int count,
                                                const uint64_t *d_keyhat, uint64_t limb_stride, uint64_t poly_stride, uint64_t batch, unsigned flags,
                                                void *stream)
{
  return rns_mod_up_mul(nlimbs, plans, d_c, d_ext, first, count, d_keyhat, batch, flags, stream, Layout{limb_stride, poly_stride});
}
