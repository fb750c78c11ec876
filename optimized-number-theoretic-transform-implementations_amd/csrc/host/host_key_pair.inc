/* host/host_key_pair.inc -- the key products for BOTH components of a key-switching key in one call: ntt_rns_fwd_mul_pair_batch,
 * ntt_rns_mod_up_mul_pair_batch and their strided forms,
 *     c0^ (+)= fwd(x) (.) key0^,   c1^ (+)= fwd(x) (.) key1^,   x = the operand (fwd_mul_pair) or ModUp(digit) (mod_up_mul_pair),
 * the shared operand read, converted and transformed ONCE.  A section of ntt_host.hip (one translation unit, included from there in
 * order); not compiled by itself.  The fused kernel is in the modup_mul2_f64*.hip units (launched by host_modup_mul.inc's
 * modup_mul_launch with two components), the two-output element-wise kernel in keypair_dot2.hip; this section sees their launchers
 * only (ntt_keyswitch.h, ntt_galois.h).  The pair form of the rotation key
 * product is in host_galois.inc.
 *
 * Per run of compatible limbs (rns_runs):
 *   fused        FP64 policies, N = 2^6..2^14, where NTT_OPT_PAIR_FUSED on plans[0] allows it: ONE modup_mul2_kernel launch.  The operand
 *                is only read: d_a, the digit and d_ext's other slots stay as they were.
 *   composition  anything else (integer policies, N < 2^6, N >= 2^15, option 0): bconv_kernel into the operand's other slots of the
 *                run (not for fwd_mul_pair), ONE forward transform of the run in place, then keypair_dot2_kernel with g = 1 and one
 *                operand pair per 16 limbs: c_j[s] (+)= x^[s] * key_j[s], the exact 128-bit sum reduced once -- canonical for lazy key
 *                words too (x^ < 2^61, key < 2^63, c < 2^64) and for every policy.  No launch reads x after the transform has
 *                overwritten it: the products read x^, which both components share.
 * Every read of the digit by a base conversion -- the bconv launches, then the fused launches -- is issued in front of the first
 * transform of a composition run, which overwrites its limbs of the operand.  Nothing is allocated, the host is not synchronised and
 * no memset is issued. */

/* The automatic choice (NTT_OPT_PAIR_FUSED -1).  count = 0 stands for ntt_rns_fwd_mul_pair_batch (no conversion).  From
 * profiles/r11/key_pair_bench.txt (24 limbs of 50-bit primes, broadcast keys, accumulating; call rate over that of the better of the
 * PARENT commit's two compositions -- A: the single call twice, B: ntt_rns_mod_up_batch + ntt_rns_fwd_batch + two element-wise
 * accumulates --, ranges over eight rounds of alternating processes; the parent's own spread 1.01-1.03 at 64 and 1024 polynomials,
 * up to 1.05 at 2):
 *   fused    count   2^14 x 2     2^14 x 64    2^14 x 1024   2^13 x 64    2^13 x 1024
 *              0     0.98-1.04    1.26-1.38    1.29-1.38     1.31-1.34    1.47-1.52
 *              1     1.27-1.31    1.21-1.31    1.21-1.32     1.28-1.32    1.24-1.29
 *              2     0.78-0.83    1.15-1.23    1.11-1.16     1.56-1.61    1.23-1.26
 *              3     0.71-0.74    1.04-1.11    0.99-1.03     1.42-1.47    1.09-1.11
 *              4     0.63-0.66    0.95-1.00    0.90-0.92     1.29-1.33    0.98-0.99
 *              8     0.40-0.42    0.66-0.68    0.62-0.63     0.88-0.93    0.67-0.67
 *   composition
 *              0     1.09-1.18    1.08-1.16    1.03-1.08     0.91-0.97    1.04-1.06
 *              1     1.07-1.13    0.82-0.87    0.80-0.83     0.61-0.64    0.71-0.73
 *              2     1.06-1.13    1.06-1.14    1.06-1.09     1.07-1.12    1.04-1.07
 *              3     1.06-1.14    1.06-1.13    1.06-1.08     1.06-1.12    1.06-1.08
 *              4     1.03-1.11    1.06-1.10    1.06-1.08     1.05-1.12    1.06-1.08
 *              8     1.06-1.11    1.01-1.07    1.05-1.08     1.06-1.12    1.05-1.08
 * With the re-conversion spread over two products the fused kernel's crossover moves from round 10's count 1 to count 2: at 2^14 it
 * is not slower than the better baseline at both 64 and 1024 polynomials for count 0, 1 and 2 -- C = 2.  At count 3 it is 0.99-1.03
 * at 1024 polynomials, inside the parent's spread of 1.01 and below 1 in a round (no win, and the composition is ahead of both there:
 * 1.06-1.08); from count 4 on it is behind.  (For count 1 the better baseline is A, whose single call takes round 10's fused kernel;
 * the composition re-materialises the extended digit and loses to it.)  The 2-polynomial rows are launch-bound: count 0 is inside
 * the spread, count 1 gains, and at count 2 the fused kernel reads 0.78-0.83 where the composition reads 1.06-1.13 -- the rule looks
 * at 64 and 1024 polynomials, so the default loses there; a batch-dependent rule has not been measured at the sizes between.  So:
 * fused for count <= 2, the composition otherwise. */
static bool pair_fused_pays(int count) { return count <= 2; }

static bool pair_fused_applies(const ntt_plan *p0, const ntt_plan *p, int count)
{
  if(!modup_mul_built(p)) return false;
  if(p0->pair_fused >= 0) return p0->pair_fused == 1;
  return pair_fused_pays(count);
}

/* what one call works on; count = 0: fwd_mul_pair, x is the operand as it stands */
struct KeyPair {
  uint64_t *      c[2];
  uint64_t *      x; /* d_a / d_ext */
  const uint64_t *key[2];
  int             first, count;
  uint64_t        bslab, batch;
  unsigned        flags;
  void *          stream;
  Layout          lay;
};

/* c_j^ (+)= x^ (.) key_j^ over limbs [rf, rf + rn): keypair_dot2_kernel with the identity permutation, one launch per 16 limbs */
static int pair_products(ntt_plan *const *plans, int rf, int rn, const KeyPair &kp)
{
  const bool     bcast = (kp.flags & NTT_MUL_B_BROADCAST) != 0;
  GaloisDot2Args da{};
  da.k               = 1;
  da.limb_stride     = kp.lay.limb;
  da.poly_stride     = kp.lay.poly;
  da.key_limb_stride = kp.bslab;
  da.key_poly_stride = bcast ? 0 : kp.lay.poly;
  da.batch           = kp.batch;
  da.logn            = (uint32_t)plans[rf]->m;
  da.g               = 1;
  da.accumulate      = (kp.flags & NTT_MUL_ACCUMULATE) != 0;
  da.max_grid        = plans[rf]->max_grid;
  da.stream          = (hipStream_t)kp.stream;
  for(int f = rf; f < rf + rn; f += kGaloisLimbs) {
    da.nlimbs = rf + rn - f < kGaloisLimbs ? rf + rn - f : kGaloisLimbs;
    da.a[0]   = kp.x + (uint64_t)f * kp.lay.limb;
    for(int j = 0; j < 2; j++) {
      da.c[j]      = kp.c[j] + (uint64_t)f * kp.lay.limb;
      da.key[j][0] = kp.key[j] + (uint64_t)f * kp.bslab;
    }
    for(int l = 0; l < da.nlimbs; l++) da.ql[l] = bconv_dst(plans[f + l]->q);
    const hipError_t e = launch_galois_dot2(da);
    if(e != hipSuccess) return fail(NTT_ERR_HIP, std::string("keypair_dot2_kernel: ") + hipGetErrorString(e));
  }
  return NTT_OK;
}

static int rns_key_pair(int nlimbs, ntt_plan *const *plans, KeyPair kp)
{
  const char *const what = kp.count ? "mod_up_mul_pair" : "fwd_mul_pair";
  int               rc   = rns_check(nlimbs, plans);
  if(rc) return rc;
  const int first = kp.first, count = kp.count;
  if(count && (count < 1 || count > kBconvLimbs || first < 0 || first > nlimbs - count)) return fail(NTT_ERR_ARG, "the digit's limbs are out of range");
  if(kp.flags & ~(unsigned)(NTT_MUL_LAZY_IN | NTT_MUL_B_BROADCAST | NTT_MUL_ACCUMULATE)) return fail(NTT_ERR_ARG, "unknown flag");
  if(!kp.c[0] || !kp.c[1] || !kp.x || !kp.key[0] || !kp.key[1]) return fail(NTT_ERR_ARG, "null argument");
  rc = layout_check(plans[0]->N, nlimbs, kp.batch, kp.lay);
  if(!rc && count) rc = distinct_primes(nlimbs, plans);
  if(rc) return rc;
  if(plans[0]->m < 1 || plans[0]->m > 30) return fail(NTT_ERR_ARG, std::string(what) + ": N out of range");
  for(int l = 0; l < nlimbs; l++) {
    if(!plans[l]->has_fwd) return fail(NTT_ERR_ARG, "a limb's plan lacks the forward table");
  }
  if(kp.batch == 0) return NTT_OK;
  const uint64_t N     = plans[0]->N;
  const bool     bcast = (kp.flags & NTT_MUL_B_BROADCAST) != 0;
  kp.bslab             = bcast ? N : kp.lay.limb; /* a broadcast key is [limb][N] */
  const auto words = [&](const uint64_t *p) { return galois_span(p, N, nlimbs, kp.batch, kp.lay.limb, kp.lay.poly); };
  const auto keyws = [&](const uint64_t *p) { return galois_span(p, N, nlimbs, bcast ? 1 : kp.batch, kp.bslab, bcast ? 0 : kp.lay.poly); };
  if(galois_overlap(words(kp.c[0]), words(kp.c[1]))) return fail(NTT_ERR_ARG, std::string(what) + ": c0^ overlaps c1^");
  /* every limb's workgroups read the operand while others write c0^ and c1^ */
  if(galois_overlap(words(kp.c[0]), words(kp.x)) || galois_overlap(words(kp.c[1]), words(kp.x)))
    return fail(NTT_ERR_ARG, std::string(what) + ": an output overlaps the operand");
  /* c0^ is stored before key1^ is read, c1^ while other workgroups still read key0^ */
  if(galois_overlap(words(kp.c[0]), keyws(kp.key[1])) || galois_overlap(words(kp.c[1]), keyws(kp.key[0])))
    return fail(NTT_ERR_ARG, std::string(what) + ": an output overlaps the other component's key");
  USE_DEVICE(plans[0]->device);
  uint64_t  b[kBconvLimbs];
  BconvArgs ba{};
  const std::vector<std::pair<int, int>> runs = rns_runs(nlimbs, plans);
  std::vector<char>                      fused(runs.size(), 0);
  for(size_t r = 0; r < runs.size(); r++) fused[r] = pair_fused_applies(plans[0], plans[runs[r].first], count) ? 1 : 0;
  if(count) {
    modup_args(plans, kp.x, first, count, kp.batch, kp.stream, kp.lay, b, ba);
    const std::vector<std::pair<int, int>> dst = modup_dst_ranges(runs, fused, first, count);
    rc                                         = modup_launches(plans, b, ba, dst.data(), dst.size());
  }
  for(size_t r = 0; !rc && r < runs.size(); r++) {
    if(fused[r])
      rc = modup_mul_launch(plans, runs[r].first, runs[r].second, first, count, 2, kp.c, kp.x, kp.key, kp.bslab, kp.batch, kp.flags, kp.stream, kp.lay, ba.sl);
  }
  for(size_t r = 0; !rc && r < runs.size(); r++) {
    if(fused[r]) continue;
    const int rf = runs[r].first, rn = runs[r].second;
    rc = rns_transform(rn, plans + rf, kp.x + (uint64_t)rf * kp.lay.limb, kp.batch, false, kp.stream, kp.lay);
    if(!rc) rc = pair_products(plans, rf, rn, kp);
  }
  return rc;
}

extern "C" int ntt_rns_fwd_mul_pair_batch(int nlimbs, ntt_plan *const *plans, uint64_t *d_c0, uint64_t *d_c1, uint64_t *d_a, const uint64_t *d_b0hat,
                                          const uint64_t *d_b1hat, uint64_t batch, unsigned flags, void *stream)
{
  return rns_key_pair(nlimbs, plans, KeyPair{{d_c0, d_c1}, d_a, {d_b0hat, d_b1hat}, 0, 0, 0, batch, flags, stream, limb_major(plans, nlimbs, batch)});
}

extern "C" int ntt_rns_fwd_mul_pair_batch_strided(int nlimbs, ntt_plan *const *plans, uint64_t *d_c0, uint64_t *d_c1, uint64_t *d_a,
                                                  const uint64_t *d_b0hat, const uint64_t *d_b1hat, uint64_t limb_stride, uint64_t poly_stride,
                                                  uint64_t batch, unsigned flags, void *stream)
{
  return rns_key_pair(nlimbs, plans, KeyPair{{d_c0, d_c1}, d_a, {d_b0hat, d_b1hat}, 0, 0, 0, batch, flags, stream, Layout{limb_stride, poly_stride}});
}

extern "C" int ntt_rns_mod_up_mul_pair_batch(int nlimbs, ntt_plan *const *plans, uint64_t *d_c0, uint64_t *d_c1, uint64_t *d_ext, int first, int count,
                                             const uint64_t *d_key0hat, const uint64_t *d_key1hat, uint64_t batch, unsigned flags, void *stream)
{
  if(count < 1) return fail(NTT_ERR_ARG, "the digit's limbs are out of range");
  return rns_key_pair(nlimbs, plans,
                      KeyPair{{d_c0, d_c1}, d_ext, {d_key0hat, d_key1hat}, first, count, 0, batch, flags, stream, limb_major(plans, nlimbs, batch)});
}

extern "C" int ntt_rns_mod_up_mul_pair_batch_strided(int nlimbs, ntt_plan *const *plans, uint64_t *d_c0, uint64_t *d_c1, uint64_t *d_ext, int first,
                                                     int count, const uint64_t *d_key0hat, const uint64_t *d_key1hat, uint64_t limb_stride,
                                                     uint64_t poly_stride, uint64_t batch, unsigned flags, void *stream)
{
  if(count < 1) return fail(NTT_ERR_ARG, "the digit's limbs are out of range");
  return rns_key_pair(nlimbs, plans,
                      KeyPair{{d_c0, d_c1}, d_ext, {d_key0hat, d_key1hat}, first, count, 0, batch, flags, stream, Layout{limb_stride, poly_stride}});
}
