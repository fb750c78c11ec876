/* host/host_ntt_domain.inc -- products of operands that are in the NTT domain (inner products, forward transform with the product at its output), their RNS forms, strided and pointer batches, fills / checksums / probes.
 * A section of ntt_host.hip (one translation unit, included from there in order); not compiled by itself. */

/* ------------------------------------------------------------------ */
/* products of operands that are in the NTT domain (SURVEY 8f, f1)      */
/* ------------------------------------------------------------------ */
static hipError_t dispatch_dot(const ntt_plan *p, const DotArgs &da)
{
  return with_class(p, [&](auto k) { return launch_dot<typename decltype(k)::A, decltype(k)::KSH>(da); });
}
static hipError_t dispatch_mul(const ntt_plan *p, const MulArgs &ma)
{
  return with_class(p, [&](auto k) { return launch_fwd_mul<typename decltype(k)::A, decltype(k)::KSH>(ma); });
}

/* The two records of the NTT-domain products over ls, operands and operand flags (NTT_MUL_*) in place; b_limb_stride: words
 * between the limbs of a b operand (0: one limb).  What a route adds: block_log and oversub, set_team, set_ptrs. */
static DotArgs dot_args(const ntt_plan *p, const LimbSet &ls, uint64_t *out, int k, const uint64_t *const *a, const uint64_t *const *b, uint64_t batch,
                        unsigned flags, uint64_t b_limb_stride, void *stream)
{
  DotArgs da{};
  launch_common(da, p, ls, batch, stream);
  da.out           = out;
  da.a             = a;
  da.b             = b;
  da.npairs        = k;
  da.lazy_in       = (flags & NTT_MUL_LAZY_IN) != 0;
  da.b_bcast       = (flags & NTT_MUL_B_BROADCAST) != 0;
  da.b_limb_stride = b_limb_stride;
  return da;
}
static MulArgs mul_args(const ntt_plan *p, const LimbSet &ls, uint64_t *out, uint64_t *a, const uint64_t *b, uint64_t batch, unsigned flags,
                        uint64_t b_limb_stride, void *stream)
{
  MulArgs ma{};
  launch_common(ma, p, ls, batch, stream);
  ma.a             = a;
  ma.b             = b;
  ma.out           = out;
  ma.lazy_in       = (flags & NTT_MUL_LAZY_IN) != 0;
  ma.b_bcast       = (flags & NTT_MUL_B_BROADCAST) != 0;
  ma.accumulate    = (flags & NTT_MUL_ACCUMULATE) != 0;
  ma.b_limb_stride = b_limb_stride;
  return ma;
}

/* plans the fused kernel serves: the radix-2 policies on blocks of 2^6 points and more */
static bool dot_kernel_applies(const ntt_plan *p)
{
  return (p->arith == NTT_ARITH_F64 || p->arith == NTT_ARITH_U64) && !p->generic && p->m >= kFusedMin && p->dot_fused != 0;
}

/* the automatic choice between the one-launch form of the NTT-domain products at N = 2^15..2^17 and the per-chunk launches, as
 * measured (profiles/r05/domain_bench_xcd_local.txt) */
static bool dot_team_pays(const ntt_plan *p, uint64_t polys, int k, bool bcast)
{
  /* (profiles/r05/domain_bench_xcd_local.txt, _batch.txt: +11..26 % from 2^25 coefficients per operand on -- 1024 / 512 / 512
   * polynomials at 2^15 / 2^16 / 2^17; half of that is even or a loss, the queues then being as long as the lag) */
  if(polys < 512 || (polys << p->m) < (1ull << 25)) return false;
  /* a key shared by the batch: its words come from the L2 and the row items get short -- the gain ends at three pairs (2^17: -3 %,
   * eight pairs -18 %) and between four and eight pairs at 2^16 (+12 % at three, -12 % at eight); 2^15 keeps +6 % at eight */
  if(bcast) return p->m == kTeamBlock + 3 || k <= (p->m == kTeamBlock + 4 ? 4 : 2);
  return true;
}

/* Polynomials between the two passes of a queue in team_dot_kernel.  Measured optimum: lag x polynomial size = 5-6 MiB per
 * queue at all three sizes (24 / 12 / 6 polynomials), a little more for one or two pairs, a shared key and the integer policy,
 * whose row items are short -- too short a lag and second-pass items wait for rows still in flight, too long and c has left the
 * Infinity Cache slice when it is read back.  Fine sweep, k = 1..4, three operand kinds: profiles/r05/teamdot_lag_fine.txt,
 * teamdot_lag_other.txt (a lag two steps off the optimum costs 5-15 %; the plain transform's 8-10 polynomials lose 22 % at 2^15). */
static int dot_team_lag(const ntt_plan *p, int k, bool bcast)
{
  const bool longer = k <= 2 || bcast || p->arith == NTT_ARITH_U64;
  switch(p->m - kTeamBlock) {
    case 3: return longer ? 24 : 20;
    case 4: return bcast ? 14 : longer ? 12 : 10;
    default: return (k == 1 || bcast) ? 8 : 6;
  }
}

/* c = inv(sum_i a_i^ (.) b_i^).  One launch up to N = 2^14: the products are formed where the inverse transform would
 * convert its input words (dot_inv_kernel).  Above: per 256 MiB chunk of c that kernel over the blocks (the product rides in
 * the inverse's first pass), then the inverse's column passes on c -- 16kN + 24N bytes instead of 24kN + 32N.  Plans the
 * kernel is not built for (column-pass-only, radix-4 formulation, N < 2^6) accumulate the products with pointwise
 * launches and run their own inverse transform.  ls: the limbs one launch serves; b_limb_stride: words between the limbs
 * of a b operand. */
static int inv_dot(const ntt_plan *p, uint64_t *d_c, int k, const uint64_t *const *a, const uint64_t *const *b, uint64_t batch,
                   unsigned flags, void *stream, const LimbSet *set = nullptr, uint64_t b_limb_stride = 0)
{
  if(!p || !d_c || !a || !b) return fail(NTT_ERR_ARG, "null argument");
  if(k < 1 || k > kMaxDot) return fail(NTT_ERR_ARG, "number of operand pairs must be 1 .. 32");
  if(flags & ~(unsigned)(NTT_MUL_LAZY_IN | NTT_MUL_B_BROADCAST)) return fail(NTT_ERR_ARG, "unknown flag");
  for(int i = 0; i < k; i++) {
    if(!a[i] || !b[i]) return fail(NTT_ERR_ARG, "null operand");
  }
  if(batch == 0) return NTT_OK;
  if(!p->has_inv) return fail(NTT_ERR_ARG, "plan lacks the inverse table");
  const bool lazy = (flags & NTT_MUL_LAZY_IN) != 0, bcast = (flags & NTT_MUL_B_BROADCAST) != 0;
  const LimbSet ls = set ? *set : LimbSet{p->limbrec.data(), 1, 0, 0};
  USE_DEVICE(p->device);
  if(!dot_kernel_applies(p) || (ls.n > 1 && !multi_limb_plan(p))) {
    if(ls.n != 1) return fail(NTT_ERR_UNSUPPORTED, "one launch over several limbs needs the FP64 policies or the wide integer policy");
    for(int i = 0; i < k; i++) {
      int rc = pointwise_acc(p, d_c, a[i], b[i], batch, ls, lazy, i > 0, bcast, stream);
      if(rc) return rc;
    }
    return run_transform(p, d_c, batch, true, false, stream, false, &ls);
  }
  const uint64_t bls = ls.n > 1 ? b_limb_stride : 0;
  /* N = 2^15..2^17, batches that keep the eight queues busy: the blocks with the products AND the inverse's column stages as
   * the items of ONE launch (team_dot_kernel) instead of two launches per 128 / 256 MiB chunk.  NTT_OPT_XCD_LOCAL 1 / 0 forces
   * either form; while a stream is being captured without a control block of its own the per-chunk launches serve (team_buffer). */
  const uint64_t polys = batch * (uint64_t)ls.n;
  void *         ctl   = nullptr;
  if(team_pays(p, polys, ls.n, [&] { return dot_team_pays(p, polys, k, bcast); })) {
    int rc = team_buffer(p, stream, polys, &ctl);
    if(rc) return rc;
  }
  if(ctl) {
    DotArgs da = dot_args(p, ls, d_c, k, a, b, batch, flags, bls, stream);
    set_team(da, p, ctl, dot_team_lag(p, k, bcast));
    return launched(dispatch_dot(p, da));
  }
  const int      pblk = p->m > kFusedMax ? (p->block_log ? p->block_log : multi_pass_block(p->m, true, p->arith == NTT_ARITH_F64)) : p->m;
  const PassList L    = make_passes(p->m, false, pblk);
  /* the chunk is what must still be in the Infinity Cache when the column pass reads c back; here the operands stream
   * through that cache as well (two to 2k times the chunk), so a smaller chunk than the transforms' 256 MiB pays at
   * N = 2^15 and 2^16 (measured: 128 MiB +4..7 %, 64 MiB the same for k = 3 and slower for k = 1, none at 2^17;
   * profiles/r04/dot_chunk.txt).  An explicit NTT_OPT_CHUNK_MIB is honoured as given. */
  const uint64_t mib = p->chunk_mib == 256 && p->m <= kFusedMax + 2 ? 128 : (uint64_t)p->chunk_mib;
  return for_chunks(p, ls, batch, mib, L.n, [&](uint64_t, uint64_t nb, uint64_t off) -> int {
    const uint64_t *ca[kMaxDot], *cb[kMaxDot];
    for(int i = 0; i < k; i++) {
      ca[i] = a[i] + off;
      cb[i] = bcast ? b[i] : b[i] + off;
    }
    DotArgs da   = dot_args(p, ls, d_c + off, k, ca, cb, nb, flags, bls, stream);
    da.block_log = (uint32_t)pblk;
    da.oversub   = p->block_oversub;
    int rc       = launched(dispatch_dot(p, da));
    for(int j = L.n - 2; !rc && j >= 0; j--) { /* the inverse's column passes on c; the last one ends the transform (N^-1) */
      rc = launch_one_pass(p, L.p[j], d_c + off, nb, true, false, false, j == 0, stream, ls);
    }
    return rc;
  });
}

extern "C" int ntt_inv_dot_batch(const ntt_plan *p, uint64_t *d_c, int k, const uint64_t *const *d_ahat,
                                 const uint64_t *const *d_bhat, uint64_t batch, unsigned flags, void *stream)
{
  return inv_dot(p, d_c, k, d_ahat, d_bhat, batch, flags, stream);
}

extern "C" int ntt_inv_product_batch(const ntt_plan *p, uint64_t *d_c, const uint64_t *d_ahat, const uint64_t *d_bhat,
                                     uint64_t batch, unsigned flags, void *stream)
{
  return inv_dot(p, d_c, 1, &d_ahat, &d_bhat, batch, flags, stream);
}

/* c = inv(fwd(a) (.) b^): the product kernels' form with one operand already transformed (fused_product_kernel /
 * team_product_kernel without BOTH / FOUR); plans those kernels are not built for take fwd, pointwise, inv */
static int mul_transformed(const ntt_plan *p, uint64_t *d_c, uint64_t *d_a, const uint64_t *d_bhat, uint64_t batch, unsigned flags,
                           void *stream, const LimbSet *set = nullptr)
{
  if(!p || !d_c || !d_a || !d_bhat) return fail(NTT_ERR_ARG, "null argument");
  if(flags & ~(unsigned)NTT_MUL_LAZY_IN) return fail(NTT_ERR_ARG, "unknown flag");
  if(batch == 0) return NTT_OK;
  if(!p->has_fwd || !p->has_inv) return fail(NTT_ERR_ARG, "plan lacks a table");
  if(d_a == d_bhat) return fail(NTT_ERR_ARG, "the coefficient operand and the transformed operand must be different buffers");
  /* (the kernels take b^ as lazy words v + 2q: a canonical word c is the lazy word of v = c - 2q, so one form serves both) */
  if(fused_product_applies(p, d_c, d_bhat, d_a, batch)) {
    return fused_product(p, d_c, const_cast<uint64_t *>(d_bhat), d_a, batch, stream, set, true);
  }
  const bool lazy = (flags & NTT_MUL_LAZY_IN) != 0;
  if(set && set->n > 1) {
    /* a limb set of the wide integer policy: a's forward transform over the set (lazy words), then the products inside the
     * inverse transform's first pass (dot_inv_kernel) -- two launches for all limbs */
    if(!multi_limb_plan(p) || !dot_kernel_applies(p)) {
      return fail(NTT_ERR_UNSUPPORTED, "one launch over several limbs needs the FP64 policies or the wide integer policy");
    }
    int rcs = run_transform(p, d_a, batch, false, false, stream, true, set);
    const uint64_t *pa = d_a;
    if(!rcs) rcs = inv_dot(p, d_c, 1, &pa, &d_bhat, batch, NTT_MUL_LAZY_IN, stream, set, set->stride);
    return rcs;
  }
  const LimbSet own = set ? *set : LimbSet{p->limbrec.data(), 1, 0, 0};
  int rc = run_transform(p, d_a, batch, false, false, stream, p->arith != NTT_ARITH_U64_R4, &own);
  if(!rc) rc = pointwise_launch(p, d_c, d_a, d_bhat, batch, stream, lazy || p->arith != NTT_ARITH_U64_R4, own.pstride);
  if(!rc) rc = run_transform(p, d_c, batch, true, false, stream, false, &own);
  return rc;
}

extern "C" int ntt_mul_transformed_batch(const ntt_plan *p, uint64_t *d_c, uint64_t *d_a, const uint64_t *d_bhat, uint64_t batch,
                                         unsigned flags, void *stream)
{
  return mul_transformed(p, d_c, d_a, d_bhat, batch, flags, stream);
}

/* c^ = fwd(a) (.) b^ (+ c^), the result staying in the NTT domain: the forward transform with the product where it would
 * reduce and store its outputs (fwd_mul_kernel).  One launch up to N = 2^14; above, the forward column passes run on a in
 * place (a is scratch there) and the product rides in the block pass, the forward transform's last one.  Plans without the
 * kernel: forward transform of a in place, then a pointwise (accumulate) launch. */
/* the one-launch form of c^ = fwd(a) (.) b^ (+ c^) at N = 2^15..2^17 against the per-chunk launches: the automatic choice and the lag
 * between the two passes of a queue, as measured (profiles/r05/domain_bench_xcd_local_mul.txt) */
static bool mul_team_pays(const ntt_plan *p, uint64_t polys, bool bcast, bool acc)
{
  /* +8..16 % (FP64), +16..28 % (wide integer policy) on large batches, all four operand kinds alike; even at 2^26 coefficients
   * per operand (2048 / 1024 / 512 polynomials at 2^15 / 2^16 / 2^17: +0 / +5 / +9 %), a loss below
   * (domain_bench_xcd_local_mul_batch.txt) */
  (void)bcast, (void)acc;
  return polys >= 512 && (polys << p->m) >= (1ull << 26);
}
/* (flat between 8 and 16 polynomials at 2^15 and 2^16; 2^17 loses 1-2 % per step beyond 8) */
static int mul_team_lag(const ntt_plan *p) { return p->m == kTeamBlock + 3 ? 10 : 8; }

static int fwd_mul(const ntt_plan *p, uint64_t *d_c, uint64_t *d_a, const uint64_t *d_bhat, uint64_t batch, unsigned flags,
                   void *stream, const LimbSet *set = nullptr, uint64_t b_limb_stride = 0)
{
  if(!p || !d_c || !d_a || !d_bhat) return fail(NTT_ERR_ARG, "null argument");
  if(flags & ~(unsigned)(NTT_MUL_LAZY_IN | NTT_MUL_B_BROADCAST | NTT_MUL_ACCUMULATE)) return fail(NTT_ERR_ARG, "unknown flag");
  if(batch == 0) return NTT_OK;
  if(!p->has_fwd) return fail(NTT_ERR_ARG, "plan lacks the forward table");
  const bool lazy = (flags & NTT_MUL_LAZY_IN) != 0, bcast = (flags & NTT_MUL_B_BROADCAST) != 0, acc = (flags & NTT_MUL_ACCUMULATE) != 0;
  if(acc && d_c == d_a) return fail(NTT_ERR_ARG, "an accumulator cannot alias the coefficient operand");
  const LimbSet ls = set ? *set : LimbSet{p->limbrec.data(), 1, 0, 0};
  USE_DEVICE(p->device);
  if(!dot_kernel_applies(p) || (ls.n > 1 && !multi_limb_plan(p))) {
    if(ls.n != 1) return fail(NTT_ERR_UNSUPPORTED, "one launch over several limbs needs the FP64 policies or the wide integer policy");
    int rc = run_transform(p, d_a, batch, false, false, stream, false, &ls);
    if(rc) return rc;
    return pointwise_acc(p, d_c, d_a, d_bhat, batch, ls, lazy, acc, bcast, stream);
  }
  const uint64_t bls = ls.n > 1 ? b_limb_stride : 0;
  /* N = 2^15, FP64 policies: the one-pass transform with the product at its output (onepass_mul_kernel) -- a is left as it was.
   * Same choice as the plain transform's (NTT_OPT_ONE_PASS; -1: batches that give every second CU a polynomial).  (The record names
   * no block size and no oversubscription.) */
  if(p->m == kFusedMax + 1 && p->arith == NTT_ARITH_F64 && !p->generic && ls.n <= kMaxLimbs && !ls.ptab &&
     one_pass_pays(p, batch * (uint64_t)ls.n)) {
    MulArgs ma  = mul_args(p, ls, d_c, d_a, d_bhat, batch, flags, bls, stream);
    ma.one_pass = 1;
    return launched(dispatch_mul(p, ma));
  }
  /* N = 2^15..2^17, batches that keep the eight queues busy: the forward column stages of a and the blocks with the product as
   * the items of ONE launch (team_mul_kernel) instead of two launches per chunk.  NTT_OPT_XCD_LOCAL 1 / 0 forces either form; a
   * stream being captured without a control block of its own takes the per-chunk launches (team_buffer). */
  const uint64_t polys = batch * (uint64_t)ls.n;
  void *         ctl   = nullptr;
  if(team_pays(p, polys, ls.n, [&] { return mul_team_pays(p, polys, bcast, acc); })) {
    int rc = team_buffer(p, stream, polys, &ctl);
    if(rc) return rc;
  }
  if(ctl) {
    MulArgs ma = mul_args(p, ls, d_c, d_a, d_bhat, batch, flags, bls, stream);
    set_team(ma, p, ctl, mul_team_lag(p));
    return launched(dispatch_mul(p, ma));
  }
  const int      pblk = p->m > kFusedMax ? (p->block_log ? p->block_log : multi_pass_block(p->m, false, p->arith == NTT_ARITH_F64)) : p->m;
  const PassList L    = make_passes(p->m, false, pblk);
  return for_chunks(p, ls, batch, (uint64_t)p->chunk_mib, L.n, [&](uint64_t, uint64_t nb, uint64_t off) -> int {
    for(int j = 0; j + 1 < L.n; j++) { /* forward column passes of a (every pass but the last, which is the block pass) */
      int rc = launch_one_pass(p, L.p[j], d_a + off, nb, false, false, false, false, stream, ls);
      if(rc) return rc;
    }
    MulArgs ma   = mul_args(p, ls, d_c + off, d_a + off, bcast ? d_bhat : d_bhat + off, nb, flags, bls, stream);
    ma.block_log = (uint32_t)pblk;
    ma.oversub   = p->block_oversub;
    return launched(dispatch_mul(p, ma));
  });
}

extern "C" int ntt_fwd_mul_batch(const ntt_plan *p, uint64_t *d_c, uint64_t *d_a, const uint64_t *d_bhat, uint64_t batch,
                                 unsigned flags, void *stream)
{
  return fwd_mul(p, d_c, d_a, d_bhat, batch, flags, stream);
}

static int rns_fwd_mul(int nlimbs, ntt_plan *const *plans, uint64_t *d_c, uint64_t *d_a, const uint64_t *d_bhat, uint64_t batch, unsigned flags,
                       void *stream, const Layout &lay)
{
  const auto call = [&](int first, const LimbSet &ls, bool run) {
    const uint64_t bslab = b_slab(plans, lay, flags);
    return fwd_mul(plans[first], d_c + (uint64_t)first * lay.limb, d_a + (uint64_t)first * lay.limb, d_bhat + (uint64_t)first * bslab, batch, flags, stream,
                   &ls, run ? bslab : 0);
  };
  return rns_slab_runs(
    nlimbs, plans, batch, lay, [&] { return all_given(d_c && d_a && d_bhat); },
    [&](const ntt_plan *p, int) { return rns_one_launch_pays(p, batch) && dot_kernel_applies(p); },
    [&](int first, const LimbSet &ls) { return call(first, ls, true); }, [&](int l) { return call(l, own_set(plans[l], lay), false); });
}

extern "C" int ntt_rns_fwd_mul_batch(int nlimbs, ntt_plan *const *plans, uint64_t *d_c, uint64_t *d_a, const uint64_t *d_bhat,
                                     uint64_t batch, unsigned flags, void *stream)
{
  return rns_fwd_mul(nlimbs, plans, d_c, d_a, d_bhat, batch, flags, stream, limb_major(plans, nlimbs, batch));
}

extern "C" int ntt_rns_fwd_mul_batch_strided(int nlimbs, ntt_plan *const *plans, uint64_t *d_c, uint64_t *d_a, const uint64_t *d_bhat,
                                             uint64_t limb_stride, uint64_t poly_stride, uint64_t batch, unsigned flags, void *stream)
{
  return rns_fwd_mul(nlimbs, plans, d_c, d_a, d_bhat, batch, flags, stream, Layout{limb_stride, poly_stride});
}

static int rns_inv_dot(int nlimbs, ntt_plan *const *plans, uint64_t *d_c, int k, const uint64_t *const *d_ahat, const uint64_t *const *d_bhat,
                       uint64_t batch, unsigned flags, void *stream, const Layout &lay)
{
  const auto operands = [&]() -> int {
    if(k < 1 || k > kMaxDot || !d_ahat || !d_bhat) return fail(NTT_ERR_ARG, "number of operand pairs must be 1 .. 32");
    if(!d_c) return fail(NTT_ERR_ARG, "null argument");
    for(int i = 0; i < k; i++) {
      if(!d_ahat[i] || !d_bhat[i]) return fail(NTT_ERR_ARG, "null operand");
    }
    return NTT_OK;
  };
  const auto call = [&](int first, const LimbSet &ls, bool run) {
    const uint64_t  bslab = b_slab(plans, lay, flags);
    const uint64_t *la[kMaxDot], *lb[kMaxDot];
    for(int i = 0; i < k; i++) {
      la[i] = d_ahat[i] + (uint64_t)first * lay.limb;
      lb[i] = d_bhat[i] + (uint64_t)first * bslab;
    }
    return inv_dot(plans[first], d_c + (uint64_t)first * lay.limb, k, la, lb, batch, flags, stream, &ls, run ? bslab : 0);
  };
  return rns_slab_runs(
    nlimbs, plans, batch, lay, operands, [&](const ntt_plan *p, int) { return rns_one_launch_pays(p, batch) && dot_kernel_applies(p); },
    [&](int first, const LimbSet &ls) { return call(first, ls, true); }, [&](int l) { return call(l, own_set(plans[l], lay), false); });
}

extern "C" int ntt_rns_inv_dot_batch(int nlimbs, ntt_plan *const *plans, uint64_t *d_c, int k, const uint64_t *const *d_ahat,
                                     const uint64_t *const *d_bhat, uint64_t batch, unsigned flags, void *stream)
{
  return rns_inv_dot(nlimbs, plans, d_c, k, d_ahat, d_bhat, batch, flags, stream, limb_major(plans, nlimbs, batch));
}

extern "C" int ntt_rns_inv_dot_batch_strided(int nlimbs, ntt_plan *const *plans, uint64_t *d_c, int k, const uint64_t *const *d_ahat,
                                             const uint64_t *const *d_bhat, uint64_t limb_stride, uint64_t poly_stride, uint64_t batch,
                                             unsigned flags, void *stream)
{
  return rns_inv_dot(nlimbs, plans, d_c, k, d_ahat, d_bhat, batch, flags, stream, Layout{limb_stride, poly_stride});
}

static int rns_mul_transformed(int nlimbs, ntt_plan *const *plans, uint64_t *d_c, uint64_t *d_a, const uint64_t *d_bhat, uint64_t batch,
                               unsigned flags, void *stream, const Layout &lay)
{
  /* one launch over a run: the fused product kernels (FP64 policies), or -- limbs of the wide integer policy -- the forward
   * transform and the products-inside-the-inverse launch, each over the whole run */
  return rns_slab_runs(
    nlimbs, plans, batch, lay, [&] { return all_given(d_c && d_a && d_bhat); },
    [&](const ntt_plan *p, int) {
      const bool int_set = p->arith == NTT_ARITH_U64 && dot_kernel_applies(p) && d_a != d_bhat;
      return rns_one_launch_pays(p, batch) && (fused_product_applies(p, d_c, d_bhat, d_a, batch) || int_set);
    },
    [&](int first, const LimbSet &ls) {
      const uint64_t off = (uint64_t)first * lay.limb;
      return mul_transformed(plans[first], d_c + off, d_a + off, d_bhat + off, batch, flags, stream, &ls);
    },
    [&](int l) {
      const uint64_t off = (uint64_t)l * lay.limb;
      const LimbSet  own = own_set(plans[l], lay);
      return mul_transformed(plans[l], d_c + off, d_a + off, d_bhat + off, batch, flags, stream, &own);
    });
}

extern "C" int ntt_rns_mul_transformed_batch(int nlimbs, ntt_plan *const *plans, uint64_t *d_c, uint64_t *d_a, const uint64_t *d_bhat,
                                             uint64_t batch, unsigned flags, void *stream)
{
  return rns_mul_transformed(nlimbs, plans, d_c, d_a, d_bhat, batch, flags, stream, limb_major(plans, nlimbs, batch));
}

extern "C" int ntt_rns_mul_transformed_batch_strided(int nlimbs, ntt_plan *const *plans, uint64_t *d_c, uint64_t *d_a, const uint64_t *d_bhat,
                                                     uint64_t limb_stride, uint64_t poly_stride, uint64_t batch, unsigned flags, void *stream)
{
  return rns_mul_transformed(nlimbs, plans, d_c, d_a, d_bhat, batch, flags, stream, Layout{limb_stride, poly_stride});
}

/* ---- one plan, polynomials poly_stride words apart (one limb of a caller-native layout) ---- */
extern "C" int ntt_transform_batch_strided(const ntt_plan *p, uint64_t *d_a, uint64_t poly_stride, uint64_t batch, unsigned flags, void *stream)
{
  if(flags & ~(unsigned)(NTT_FLAG_INVERSE | NTT_FLAG_WIDE_IN | NTT_FLAG_LAZY_OUT)) return fail(NTT_ERR_ARG, "unknown flag");
  if(!p) return fail(NTT_ERR_ARG, "null argument");
  if(poly_stride < p->N || poly_stride > (1ull << 40)) return fail(NTT_ERR_ARG, "layout: the polynomial stride must be at least N words");
  const LimbSet own{p->limbrec.data(), 1, 0, poly_stride};
  return run_transform(p, d_a, batch, (flags & NTT_FLAG_INVERSE) != 0, (flags & NTT_FLAG_WIDE_IN) != 0, stream, (flags & NTT_FLAG_LAZY_OUT) != 0, &own);
}

/* ---- pointer batches: one device pointer per polynomial ----
 * The reference's batching precedent hands over one array per polynomial: fwd_ntt_ref_harvey_lazy_dbl(a1[], a2[], ...)
 * (include/ntt_reference.h:44-49, src/ntt_reference.c:71-91).  Generalised to `count` pointers placed anywhere: ONE launch chain
 * for the whole batch -- the kernels read a polynomial's address from a device table where they would multiply its index by the
 * stride (ntt_core.h poly_offset; round 6: rounds 1-5 cut the sorted pointers into arithmetic progressions and launched every
 * progression by itself, i.e. 4096 separately allocated polynomials = 4096 launches).
 *   host array  (ntt_transform_ptrs):     sorted (the polynomials are independent and transformed in place: their order is free, and
 *                address order is what the memory system likes), checked for overlap, uploaded through the plan's staging buffer of
 *                the stream.  A batch that IS one arithmetic progression keeps the strided launch (no table).  While the stream is
 *                being captured nothing can be uploaded: progression by progression then -- use the device-array form in graphs.
 *   device array (ntt_transform_dev_ptrs): taken as it is -- no copy, no check (overlaps are the caller's business), capturable. */
/* ascending order.  The host side of a pointer batch is on the caller's clock (the kernels wait for the table): a batch that arrives
 * sorted costs one pass; large shuffled batches an LSD radix sort over the bits in which the addresses differ (65536 pointers: 0.3 ms
 * where std::sort took 2.3) */
static void sort_addresses(std::vector<uintptr_t> &v)
{
  if(std::is_sorted(v.begin(), v.end())) return;
  if(v.size() < 4096) {
    std::sort(v.begin(), v.end());
    return;
  }
  uintptr_t lo = v[0], hi = v[0];
  for(uintptr_t a : v) lo = a < lo ? a : lo, hi = a > hi ? a : hi;
  std::vector<uintptr_t> tmp(v.size());
  for(unsigned shift = 3; shift < 64 && ((hi - lo) >> shift) != 0; shift += 11) { /* (8-byte aligned: the low three bits carry nothing) */
    size_t count[2049] = {};
    for(uintptr_t a : v) count[(((a - lo) >> shift) & 2047u) + 1]++;
    for(int i = 0; i < 2048; i++) count[i + 1] += count[i];
    for(uintptr_t a : v) tmp[count[((a - lo) >> shift) & 2047u]++] = a;
    v.swap(tmp);
  }
}

struct PtrRun {
  uint64_t *first;
  uint64_t  stride, count; /* words between consecutive polynomials (0: a single one), polynomials */
};
static int ptr_sorted(uint64_t N, int nlimbs, uint64_t limb_stride, uint64_t *const *h_polys, uint64_t count, std::vector<uintptr_t> &v)
{
  if(!h_polys) return fail(NTT_ERR_ARG, "null argument");
  v.resize(count);
  for(uint64_t i = 0; i < count; i++) {
    if(!h_polys[i] || ((uintptr_t)h_polys[i] & 7)) return fail(NTT_ERR_ARG, "pointer batch: null or misaligned polynomial pointer");
    v[i] = (uintptr_t)h_polys[i];
  }
  sort_addresses(v);
  /* overlap: every limb image [pointer + l * limb_stride, + N) of every polynomial is an interval of N words; sorted by start,
   * two of them intersect iff two neighbours do.  (Exact also for pointers INTO a [limb][batch][N] slab, whose polynomials
   * interleave without overlapping.) */
  std::vector<uintptr_t> img;
  const std::vector<uintptr_t> *starts = &v;
  if(nlimbs > 1) {
    img.reserve((size_t)count * (size_t)nlimbs);
    for(uint64_t i = 0; i < count; i++) {
      for(int l = 0; l < nlimbs; l++) img.push_back(v[i] + (uintptr_t)l * (uintptr_t)limb_stride * 8u);
    }
    sort_addresses(img);
    starts = &img;
  }
  for(size_t i = 0; i + 1 < starts->size(); i++) {
    if((*starts)[i + 1] - (*starts)[i] < N * 8) return fail(NTT_ERR_ARG, "pointer batch: polynomials overlap (or a pointer is listed twice)");
  }
  return NTT_OK;
}
/* the sorted addresses as maximal arithmetic progressions (the fallback while capturing, and the test for "one progression").  A
 * run of two is not taken greedily: {0, 100N, 101N, 102N} is 1 + 3, not 2 + 2 -- when the pair's successor starts a longer
 * progression of another step, the first pointer goes by itself.  Steps beyond the strided entry points' bound (2^40 words)
 * never join a run. */
static void ptr_runs(const std::vector<uintptr_t> &v, std::vector<PtrRun> &runs)
{
  const uint64_t count = v.size();
  const auto     step  = [&](uint64_t i) { return (uint64_t)(v[i + 1] - v[i]); };
  const auto     ok    = [&](uint64_t d) { return d / 8 <= (1ull << 40); };
  for(uint64_t i = 0; i < count;) {
    uint64_t j = i, d = 0;
    if(i + 1 < count && ok(step(i))) {
      d = step(i);
      j = i + 1;
      while(j + 1 < count && step(j) == d) j++;
      if(j == i + 1 && j + 2 < count && step(j) != d && step(j) == step(j + 1)) j = i, d = 0; /* the pair's second member starts a longer run */
    }
    runs.push_back(PtrRun{reinterpret_cast<uint64_t *>(v[i]), d / 8, j - i + 1});
    i = j + 1;
  }
}
/* uploads the sorted addresses into the (plan, stream) device table; *out = the table, or null while the stream is being captured */
static int ptr_table(const ntt_plan *p, void *stream, const std::vector<uintptr_t> &v, const uint64_t **out)
{
  *out = nullptr;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if(hipStreamIsCapturing((hipStream_t)stream, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) return NTT_OK;
  std::lock_guard<std::mutex> lock(p->team_mu);
  ntt_plan::PtrBuf *pb = nullptr;
  for(ntt_plan::PtrBuf &b : p->ptr_bufs) {
    if(b.stream == stream) pb = &b;
  }
  if(!pb) {
    p->ptr_bufs.push_back(ntt_plan::PtrBuf{stream, nullptr, nullptr, 0, nullptr});
    pb = &p->ptr_bufs.back();
    HIP_TRY(hipEventCreateWithFlags(&pb->copied, hipEventDisableTiming));
  }
  if(pb->words < v.size()) {
    const size_t words = v.size() * 2;
    uint64_t *   d = nullptr, *h = nullptr;
    HIP_TRY(hipMalloc(&d, words * 8));
    if(hipHostMalloc(&h, words * 8, hipHostMallocDefault) != hipSuccess) {
      (void)hipFree(d);
      return fail(NTT_ERR_NOMEM, "pointer batch: pinned staging buffer");
    }
    if(pb->d) p->ptr_retired.push_back({pb->d, pb->h}); /* launches and copies still queued may be using them */
    pb->d = d, pb->h = h, pb->words = words;
  } else {
    HIP_TRY(hipEventSynchronize(pb->copied)); /* the previous upload has left the staging buffer (an event never recorded is complete) */
  }
  for(size_t i = 0; i < v.size(); i++) pb->h[i] = (uint64_t)v[i];
  HIP_TRY(hipMemcpyAsync(pb->d, pb->h, v.size() * 8, hipMemcpyHostToDevice, (hipStream_t)stream));
  HIP_TRY(hipEventRecord(pb->copied, (hipStream_t)stream));
  *out = pb->d;
  return NTT_OK;
}
/* typical distance between neighbours of a sorted batch, in words: the hint the XCD-local launches number their queues by */
static uint64_t ptr_spacing(const std::vector<uintptr_t> &v, uint64_t fallback)
{
  return v.size() > 1 ? (uint64_t)(v[v.size() / 2] - v[v.size() / 2 - 1]) / 8 : fallback;
}

extern "C" int ntt_transform_ptrs(const ntt_plan *p, uint64_t *const *h_polys, uint64_t count, unsigned flags, void *stream)
{
  if(flags & ~(unsigned)(NTT_FLAG_INVERSE | NTT_FLAG_WIDE_IN | NTT_FLAG_LAZY_OUT)) return fail(NTT_ERR_ARG, "unknown flag");
  if(!p) return fail(NTT_ERR_ARG, "null argument");
  if(count == 0) return NTT_OK;
  USE_DEVICE(p->device);
  std::vector<uintptr_t> v;
  int rc = ptr_sorted(p->N, 1, 0, h_polys, count, v);
  if(rc) return rc;
  std::vector<PtrRun> runs;
  ptr_runs(v, runs);
  const bool inverse = (flags & NTT_FLAG_INVERSE) != 0, wide = (flags & NTT_FLAG_WIDE_IN) != 0, lazy = (flags & NTT_FLAG_LAZY_OUT) != 0;
  const uint64_t *tab = nullptr;
  if(runs.size() > 1) {
    rc = ptr_table(p, stream, v, &tab);
    if(rc) return rc;
  }
  if(tab) {
    const LimbSet set{p->limbrec.data(), 1, 0, 0, tab};
    return run_transform(p, nullptr, count, inverse, wide, stream, lazy, &set);
  }
  for(size_t r = 0; !rc && r < runs.size(); r++) {
    const LimbSet own{p->limbrec.data(), 1, 0, runs[r].stride};
    rc = run_transform(p, runs[r].first, runs[r].count, inverse, wide, stream, lazy, &own);
  }
  return rc;
}

extern "C" int ntt_transform_dev_ptrs(const ntt_plan *p, const uint64_t *const *d_polys, uint64_t count, unsigned flags, void *stream)
{
  if(flags & ~(unsigned)(NTT_FLAG_INVERSE | NTT_FLAG_WIDE_IN | NTT_FLAG_LAZY_OUT)) return fail(NTT_ERR_ARG, "unknown flag");
  if(!p || (!d_polys && count)) return fail(NTT_ERR_ARG, "null argument");
  if(count == 0) return NTT_OK;
  const LimbSet set{p->limbrec.data(), 1, 0, 0, reinterpret_cast<const uint64_t *>(d_polys)};
  return run_transform(p, nullptr, count, (flags & NTT_FLAG_INVERSE) != 0, (flags & NTT_FLAG_WIDE_IN) != 0, stream, (flags & NTT_FLAG_LAZY_OUT) != 0, &set);
}

/* the same for RNS polynomials: h_polys[i] points at limb 0 of polynomial i, its limbs limb_stride words apart */
extern "C" int ntt_rns_transform_ptrs(int nlimbs, ntt_plan *const *plans, uint64_t *const *h_polys, uint64_t count, uint64_t limb_stride,
                                      unsigned flags, void *stream)
{
  if(flags & ~(unsigned)NTT_FLAG_INVERSE) return fail(NTT_ERR_ARG, "unknown flag (RNS transforms take NTT_FLAG_INVERSE only)");
  int rc = rns_check(nlimbs, plans);
  if(rc || count == 0) return rc;
  const uint64_t N = plans[0]->N;
  if(limb_stride < N || limb_stride > (1ull << 40)) return fail(NTT_ERR_ARG, "layout: the limb stride must be at least N words");
  USE_DEVICE(plans[0]->device);
  const uint64_t span = (uint64_t)(nlimbs - 1) * limb_stride + N; /* words one RNS polynomial covers */
  const bool inverse  = (flags & NTT_FLAG_INVERSE) != 0;
  std::vector<uintptr_t> v;
  rc = ptr_sorted(N, nlimbs, limb_stride, h_polys, count, v);
  if(rc) return rc;
  std::vector<PtrRun> runs;
  ptr_runs(v, runs);
  /* a progression the strided entry point takes whole is limb-major (the limbs' slabs apart: pointers into a [limb][batch][N]
   * slab) or polynomial-major (every polynomial's limbs inside its own record); any other spacing is legal here -- the
   * images were checked one by one above -- but not expressible as ONE layout */
  const auto whole = [&](const PtrRun &r) { return r.count <= 1 || limb_stride >= (r.count - 1) * r.stride + N || r.stride >= span; };
  const uint64_t *tab = nullptr;
  if(runs.size() > 1 || !whole(runs[0])) {
    rc = ptr_table(plans[0], stream, v, &tab);
    if(rc) return rc;
  }
  if(tab) return rns_transform(nlimbs, plans, nullptr, count, inverse, stream, Layout{limb_stride, ptr_spacing(v, span), tab});
  for(size_t r = 0; !rc && r < runs.size(); r++) {
    const uint64_t d = runs[r].stride ? runs[r].stride : span;
    if(whole(runs[r])) {
      rc = rns_transform(nlimbs, plans, runs[r].first, runs[r].count, inverse, stream, Layout{limb_stride, runs[r].count > 1 ? d : span});
    } else {
      for(uint64_t i = 0; !rc && i < runs[r].count; i++) rc = rns_transform(nlimbs, plans, runs[r].first + i * d, 1, inverse, stream, Layout{limb_stride, span});
    }
  }
  return rc;
}

extern "C" int ntt_rns_transform_dev_ptrs(int nlimbs, ntt_plan *const *plans, const uint64_t *const *d_polys, uint64_t count, uint64_t limb_stride,
                                          unsigned flags, void *stream)
{
  if(flags & ~(unsigned)NTT_FLAG_INVERSE) return fail(NTT_ERR_ARG, "unknown flag (RNS transforms take NTT_FLAG_INVERSE only)");
  int rc = rns_check(nlimbs, plans);
  if(rc || count == 0) return rc;
  if(!d_polys) return fail(NTT_ERR_ARG, "null argument");
  const uint64_t N = plans[0]->N;
  if(limb_stride < N || limb_stride > (1ull << 40)) return fail(NTT_ERR_ARG, "layout: the limb stride must be at least N words");
  /* (spacing hint: a polynomial's limbs side by side unless the limb stride says they are slabs apart) */
  const uint64_t span = (uint64_t)(nlimbs - 1) * limb_stride + N;
  return rns_transform(nlimbs, plans, nullptr, count, (flags & NTT_FLAG_INVERSE) != 0, stream,
                       Layout{limb_stride, limb_stride >= count * N ? N : span, reinterpret_cast<const uint64_t *>(d_polys)});
}

/* ---- products over pointer batches (round 6): every operand a DEVICE array of `count` device pointers ----
 * Up to N = 2^14 the fused product kernels read every operand through its own table (their PTRS forms, ntt_kernels_products.h:
 * tab_poly) -- ONE launch per limb at the slab forms' bytes: 24N for a coefficient-domain product, (2k + 1) 8N for an inner product
 * of k pairs, 24N / 32N for fwd(a) (.) b^ (+ c^).  Above 2^14 (and for plans those kernels are not built for) the pieces that take
 * tables serve -- an element-wise product (-accumulate) kernel that reads c, a_i and b_i through their tables, and the transforms
 * over a table: k + 1 launch chains whatever the batch (not one per polynomial). */
static bool ptrs_fused(const ntt_plan *p) { return p->m <= kFusedMax && dot_kernel_applies(p); }
/* (internal) a limb run handed to one of the *_ptrs_limb functions found no one-launch kernel: the caller takes the chain over the run */
constexpr int kRunNotServed = 1;
/* the RNS twins: a run of compatible limbs as ONE launch (chain) when a limb's share cannot fill the chip by itself (the slab forms'
 * rule: rns_one_launch_pays) -- the fused kernels' MULTI instances up to 2^14, the chain (table-reading element-wise kernel and the
 * transforms over the tables, each ONE launch over the run's limbs) otherwise; above 2^14 the XCD-local one-launch kernels over the
 * whole run from 64 polynomials x limbs on (ptrs_team) */
static bool ptrs_run_pays(const ntt_plan *p, uint64_t count)
{
  if(p->m <= kFusedMax) return rns_one_launch_pays(p, count);
  /* above 2^14: the XCD-local kernels take the limb as part of the queue entry (as for the slab forms: no launch tails between the
   * limbs, and a few polynomials x many primes feed the eight queues together where one limb's share could not), the chain serves
   * what they do not */
  return p->rns_launch != 1;
}
/* `ls` with another operand's table */
static LimbSet with_table(const LimbSet &ls, const void *tab)
{
  LimbSet r = ls;
  r.ptab    = reinterpret_cast<const uint64_t *>(tab);
  return r;
}
/* N = 2^15..2^17: the one-launch (XCD-local) product kernels read tables too; they want a control block (not while a stream is being
 * captured without a reserved one: team_buffer) and enough polynomials to feed the eight queues.  *ctl stays null otherwise: the
 * caller takes the chain.  entries: counters the launch needs (polynomials; twice that for the three-pass product). */
static int ptrs_team(const ntt_plan *p, void *stream, uint64_t count, uint64_t entries, void **ctl)
{
  *ctl = nullptr;
  /* (no measured rule here: the one-launch form wherever NTT_OPT_XCD_LOCAL does not switch it off) */
  if(p->generic || !dot_kernel_applies(p) || !team_pays(p, count, 1, [] { return true; })) return NTT_OK;
  return team_buffer(p, stream, entries, ctl);
}
/* the limbs a *_ptrs_limb launch serves: a run's records, or p's own; hint: the typical spacing of the polynomials for the XCD-local
 * launches' queue numbering (the limbs of a polynomial lie side by side) */
static LimbSet ptrs_set(const ntt_plan *p, const LimbSet *run, bool hint)
{
  return LimbSet{run ? run->d : p->limbrec.data(), run ? run->n : 1, run ? run->stride : 0, run && hint ? (uint64_t)run->n * run->stride : 0};
}

/* the limbs of a run: blockIdx.y = the limb, its operands limb_stride (a broadcast b: b_limb_stride) words further behind every table
 * entry, its modulus and constants in the kernel arguments (one limb: gridDim.y = 1) */
template <class A> struct PwLimbs {
  uint64_t           q[kMaxLimbs];
  typename A::consts k[kMaxLimbs];
};
template <class A, bool LAZYIN, bool ACC, bool BCAST>
__global__ void __launch_bounds__(256) pointwise_ptrs_kernel(const uint64_t *const *ctab, const uint64_t *const *atab, const uint64_t *const *btab,
                                                             uint64_t n, uint32_t logn, uint64_t limb_off, uint64_t b_limb_off, uint64_t limb_stride,
                                                             uint64_t b_limb_stride, const PwLimbs<A> L)
{
  const uint32_t           limb = blockIdx.y;
  const uint64_t           q    = L.q[limb];
  const typename A::consts k    = L.k[limb];
  limb_off += (uint64_t)limb * limb_stride;
  b_limb_off += (uint64_t)limb * b_limb_stride;
  for(uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t  poly = i >> logn, off = limb_off + (i & ((1ull << logn) - 1ull));
    uint64_t *      c    = const_cast<uint64_t *>(ctab[poly]) + off;
    const uint64_t  av   = atab[poly][off];
    /* a broadcast b: `btab` IS the one polynomial (limb l of it b_limb_off words in) */
    const uint64_t  bv   = BCAST ? reinterpret_cast<const uint64_t *>(btab)[b_limb_off + (i & ((1ull << logn) - 1ull))] : btab[poly][off];
    const uint64_t  t    = LAZYIN ? A::mulmod_full_lazy4(av, bv, k) : A::mulmod_full(av, bv, k);
    if constexpr(ACC) {
      const uint64_t v = *c + t; /* both canonical: < 2q < 2^64 */
      *c               = v < q ? v : v - q;
    } else {
      *c = t;
    }
  }
}

/* run / nrun: the plans of a run of compatible limbs (p = its first), their operands limb_stride words apart behind every table entry
 * (a broadcast b: N apart) -- one launch over all of them; null: p alone */
static int pointwise_ptrs(const ntt_plan *p, const uint64_t *const *ctab, const uint64_t *const *atab, const uint64_t *const *btab, uint64_t count,
                          bool lazy, bool acc, bool bcast, uint64_t limb_off, uint64_t b_limb_off, void *stream, ntt_plan *const *run = nullptr,
                          int nrun = 1, uint64_t limb_stride = 0)
{
  const uint64_t n = count * p->N;
  if(nrun < 1 || nrun > kMaxLimbs) return fail(NTT_ERR_ARG, "internal: limbs of one launch");
  uint64_t gx = grid_pw(n, p->max_grid);
  gx          = gx / (uint64_t)nrun > 0 ? gx / (uint64_t)nrun : 1;
  const dim3     g((unsigned)gx, (unsigned)nrun), t(256);
  const uint64_t bls = bcast ? p->N : 0;
  (void)with_bools(
    [&](auto f64, auto lazy_in, auto accumulate, auto b_bcast) {
      using A = PwArith<decltype(f64)::value>;
      PwLimbs<A> L{};
      for(int l = 0; l < nrun; l++) {
        const ntt_plan *pl = run ? run[l] : p;
        L.q[l]             = pl->q;
        L.k[l]             = pw_consts<A>(pl);
      }
      hipLaunchKernelGGL((pointwise_ptrs_kernel<A, decltype(lazy_in)::value, decltype(accumulate)::value, decltype(b_bcast)::value>), g, t, 0,
                         (hipStream_t)stream, ctab, atab, btab, n, (uint32_t)p->m, limb_off, b_limb_off, limb_stride, bls, L);
      return hipSuccess;
    },
    p->arith == NTT_ARITH_F64, lazy, acc, bcast);
  HIP_TRY(hipGetLastError());
  return NTT_OK;
}

/* one limb of the three product forms; limb_off: words from every table entry to this limb (RNS: l * limb_stride) */
/* run (RNS twins, fused kernels only): the records of a run of compatible limbs whose first one is p's -- ONE launch over all of them,
 * every polynomial's limbs run->stride words apart behind its table entry (limb_off / b_limb_off then name the run's first limb) */
static int inv_dot_ptrs_limb(const ntt_plan *p, const uint64_t *const *d_c, int k, const uint64_t *const *const *h_a, const uint64_t *const *const *h_b,
                             uint64_t count, unsigned flags, uint64_t limb_off, uint64_t b_limb_off, void *stream, const LimbSet *run = nullptr)
{
  if(!p->has_inv) return fail(NTT_ERR_ARG, "plan lacks the inverse table");
  USE_DEVICE(p->device);
  const bool lazy = (flags & NTT_MUL_LAZY_IN) != 0, bcast = (flags & NTT_MUL_B_BROADCAST) != 0;
  const uint64_t nrun = run ? (uint64_t)run->n : 1;
  void *ctl = nullptr;
  if(!ptrs_fused(p)) {
    int rc = ptrs_team(p, stream, nrun * count, nrun * count, &ctl);
    if(rc) return rc;
  }
  if(ptrs_fused(p) || ctl) {
    /* dot_inv_kernel's PTRS form (up to 2^14): the operand pointers ARE the tables (a broadcast b_i^: the polynomial, this limb of
     * it); team_dot_kernel's (above): products, block stages and the inverse's column stages as the items of one launch (a run: over
     * all of its limbs) */
    const uint64_t *ta[kMaxDot], *tb[kMaxDot];
    for(int i = 0; i < k; i++) {
      ta[i] = as_words(h_a[i]);
      tb[i] = as_words(h_b[i]) + (bcast ? b_limb_off : 0);
    }
    /* (a broadcast operand is [limb][N]) */
    DotArgs da = dot_args(p, ptrs_set(p, run, ctl != nullptr), as_words(d_c), k, ta, tb, count, flags, run && bcast ? p->N : 0, stream);
    set_ptrs(da, limb_off);
    if(ctl) {
      set_team(da, p, ctl, dot_team_lag(p, k, bcast));
    } else {
      da.block_log = (uint32_t)p->m;
      da.oversub   = p->block_oversub;
    }
    return launched(dispatch_dot(p, da));
  }
  if(run) return kRunNotServed;
  for(int i = 0; i < k; i++) {
    int rc = pointwise_ptrs(p, d_c, h_a[i], h_b[i], count, lazy, i > 0, bcast, limb_off, b_limb_off, stream);
    if(rc) return rc;
  }
  const LimbSet set{p->limbrec.data(), 1, 0, 0, reinterpret_cast<const uint64_t *>(d_c)};
  return run_transform(p, advance(nullptr, limb_off), count, true, false, stream, false, &set);
}

/* a run of compatible limbs (run[0 .. ls.n), records in ls): the fused kernel over all of them, or the chain -- k element-wise launches
 * and the inverse transform over c's table, each over the whole run */
static int inv_dot_ptrs_run(ntt_plan *const *run, const LimbSet &ls, const uint64_t *const *d_c, int k, const uint64_t *const *const *h_a,
                            const uint64_t *const *const *h_b, uint64_t count, unsigned flags, uint64_t limb_off, uint64_t b_limb_off, void *stream)
{
  const ntt_plan *p = run[0];
  for(int l = 0; l < ls.n; l++) {
    if(!run[l]->has_inv) return fail(NTT_ERR_ARG, "plan lacks the inverse table");
  }
  {
    const int r = inv_dot_ptrs_limb(p, d_c, k, h_a, h_b, count, flags, limb_off, b_limb_off, stream, &ls);
    if(r != kRunNotServed) return r;
  }
  USE_DEVICE(p->device);
  const bool lazy = (flags & NTT_MUL_LAZY_IN) != 0, bcast = (flags & NTT_MUL_B_BROADCAST) != 0;
  for(int i = 0; i < k; i++) {
    int rc = pointwise_ptrs(p, d_c, h_a[i], h_b[i], count, lazy, i > 0, bcast, limb_off, b_limb_off, stream, run, ls.n, ls.stride);
    if(rc) return rc;
  }
  const LimbSet sc = with_table(ls, d_c);
  return run_transform(p, advance(nullptr, limb_off), count, true, false, stream, false, &sc);
}

static int dot_ptrs_check(const void *d_c, int k, const void *const *a, const void *const *b, unsigned flags)
{
  if(!d_c || !a || !b) return fail(NTT_ERR_ARG, "null argument");
  if(k < 1 || k > kMaxDot) return fail(NTT_ERR_ARG, "number of operand pairs must be 1 .. 32");
  if(flags & ~(unsigned)(NTT_MUL_LAZY_IN | NTT_MUL_B_BROADCAST)) return fail(NTT_ERR_ARG, "unknown flag");
  for(int i = 0; i < k; i++) {
    if(!a[i] || !b[i]) return fail(NTT_ERR_ARG, "null operand");
  }
  return NTT_OK;
}

static int mul_ptrs_check(bool operands, unsigned flags)
{
  if(!operands) return fail(NTT_ERR_ARG, "null argument");
  if(flags & ~(unsigned)(NTT_MUL_LAZY_IN | NTT_MUL_B_BROADCAST | NTT_MUL_ACCUMULATE)) return fail(NTT_ERR_ARG, "unknown flag");
  return NTT_OK;
}

/* The RNS pointer-batch products, from their arguments to their runs: the limb list, the entry point's own operand and flag checks
 * (operands()), an empty batch (nothing to do), the limb stride; then rns_for_runs over tables whose entries are N words apart. */
template <class Operands, class Pays, class SetFn, class OneFn>
static int rns_ptrs_runs(int nlimbs, ntt_plan *const *plans, uint64_t count, uint64_t limb_stride, Operands operands, Pays pays, SetFn set_fn, OneFn one_fn)
{
  int rc = rns_check(nlimbs, plans);
  if(!rc) rc = operands();
  if(rc || count == 0) return rc;
  if(limb_stride < plans[0]->N || limb_stride > (1ull << 40)) return fail(NTT_ERR_ARG, "layout: the limb stride must be at least N words");
  return rns_for_runs(nlimbs, plans, Layout{limb_stride, plans[0]->N}, pays, set_fn, one_fn);
}

extern "C" int ntt_inv_dot_dev_ptrs(const ntt_plan *p, const uint64_t *const *d_c, int k, const uint64_t *const *const *h_ahat,
                                    const uint64_t *const *const *h_bhat, uint64_t count, unsigned flags, void *stream)
{
  if(!p) return fail(NTT_ERR_ARG, "null argument");
  int rc = dot_ptrs_check(d_c, k, reinterpret_cast<const void *const *>(h_ahat), reinterpret_cast<const void *const *>(h_bhat), flags);
  if(rc || count == 0) return rc;
  return inv_dot_ptrs_limb(p, d_c, k, h_ahat, h_bhat, count, flags, 0, 0, stream);
}

extern "C" int ntt_rns_inv_dot_dev_ptrs(int nlimbs, ntt_plan *const *plans, const uint64_t *const *d_c, int k, const uint64_t *const *const *h_ahat,
                                        const uint64_t *const *const *h_bhat, uint64_t count, uint64_t limb_stride, unsigned flags, void *stream)
{
  /* a run of compatible limbs whose share of the batch cannot fill the chip limb by limb (a few ciphertexts x many primes): ONE launch
   * over the run -- the fused kernels' MULTI instances, the limb an index of the grid, as for the slab forms (rns_one_launch_pays) */
  return rns_ptrs_runs(
    nlimbs, plans, count, limb_stride,
    [&] { return dot_ptrs_check(d_c, k, reinterpret_cast<const void *const *>(h_ahat), reinterpret_cast<const void *const *>(h_bhat), flags); },
    [&](const ntt_plan *p, int) { return ptrs_run_pays(p, count); },
    [&](int first, const LimbSet &ls) {
      return inv_dot_ptrs_run(plans + first, ls, d_c, k, h_ahat, h_bhat, count, flags, (uint64_t)first * limb_stride, (uint64_t)first * plans[0]->N, stream);
    },
    [&](int l) { return inv_dot_ptrs_limb(plans[l], d_c, k, h_ahat, h_bhat, count, flags, (uint64_t)l * limb_stride, (uint64_t)l * plans[0]->N, stream); });
}

/* N = 2^15, FP64 plans: fwd(a) (.) b^ in ONE pass with the tables read at its output (the slab form's choice: batches that give every
 * second CU a polynomial) */
static bool ptrs_one_pass_mul(const ntt_plan *p, uint64_t count)
{
  return p->m == kFusedMax + 1 && p->arith == NTT_ARITH_F64 && !p->generic && dot_kernel_applies(p) &&
         one_pass_pays(p, count);
}

/* c^ = fwd(a) (.) b^ (+ c^): a is transformed in place first (scratch, as for plans without the fused kernel) */
static int fwd_mul_ptrs_limb(const ntt_plan *p, const uint64_t *const *d_c, const uint64_t *const *d_a, const uint64_t *const *d_bhat, uint64_t count,
                             unsigned flags, uint64_t limb_off, uint64_t b_limb_off, void *stream, const LimbSet *run = nullptr)
{
  if(!p->has_fwd) return fail(NTT_ERR_ARG, "plan lacks the forward table");
  if((flags & NTT_MUL_ACCUMULATE) && d_c == d_a) return fail(NTT_ERR_ARG, "an accumulator cannot alias the coefficient operand");
  const uint64_t nrun = run ? (uint64_t)run->n : 1;
  USE_DEVICE(p->device);
  /* (N = 2^15, FP64 plans: the one-pass transform with the product at its output takes tables as well -- the slab form's choice) */
  /* (a limb run: one_pass_mul_kernel's table form carries one limb -- the twin hands such batches over limb by limb) */
  const bool one_pass = !run && ptrs_one_pass_mul(p, count);
  void *ctl = nullptr;
  if(!ptrs_fused(p) && !one_pass) {
    int rc = ptrs_team(p, stream, nrun * count, nrun * count, &ctl);
    if(rc) return rc;
  }
  if(ptrs_fused(p) || one_pass || ctl) {
    /* fwd_mul_kernel's (onepass_mul_kernel's) PTRS form: a is left as it was; team_mul_kernel's (2^15..2^17, a's column stages in
     * place: a is scratch) */
    const bool bcast = (flags & NTT_MUL_B_BROADCAST) != 0;
    /* (a broadcast operand is [limb][N]; the spacing hint, the lag and the oversubscription on all three forms, as ever) */
    MulArgs ma = mul_args(p, ptrs_set(p, run, true), as_words(d_c), as_words(d_a), as_words(d_bhat) + (bcast ? b_limb_off : 0), count, flags,
                          run && bcast ? p->N : 0, stream);
    set_ptrs(ma, limb_off);
    /* (also without a control block -- the fused and one-pass forms: their record has always carried the lag and the workgroups per CU;
     * set_team's block size is then replaced by the whole polynomial) */
    set_team(ma, p, ctl, mul_team_lag(p));
    if(!ctl) ma.block_log = (uint32_t)p->m;
    ma.oversub  = p->block_oversub;
    ma.one_pass = one_pass;
    return launched(dispatch_mul(p, ma));
  }
  if(run) return kRunNotServed;
  const LimbSet set{p->limbrec.data(), 1, 0, 0, reinterpret_cast<const uint64_t *>(d_a)};
  int rc = run_transform(p, advance(nullptr, limb_off), count, false, false, stream, false, &set);
  if(rc) return rc;
  return pointwise_ptrs(p, d_c, d_a, d_bhat, count, (flags & NTT_MUL_LAZY_IN) != 0, (flags & NTT_MUL_ACCUMULATE) != 0, (flags & NTT_MUL_B_BROADCAST) != 0,
                        limb_off, b_limb_off, stream);
}

extern "C" int ntt_fwd_mul_dev_ptrs(const ntt_plan *p, const uint64_t *const *d_c, const uint64_t *const *d_a, const uint64_t *const *d_bhat,
                                    uint64_t count, unsigned flags, void *stream)
{
  const int rc = mul_ptrs_check(p && d_c && d_a && d_bhat, flags);
  if(rc || count == 0) return rc;
  return fwd_mul_ptrs_limb(p, d_c, d_a, d_bhat, count, flags, 0, 0, stream);
}

extern "C" int ntt_rns_fwd_mul_dev_ptrs(int nlimbs, ntt_plan *const *plans, const uint64_t *const *d_c, const uint64_t *const *d_a,
                                        const uint64_t *const *d_bhat, uint64_t count, uint64_t limb_stride, unsigned flags, void *stream)
{
  return rns_ptrs_runs(
    nlimbs, plans, count, limb_stride, [&] { return mul_ptrs_check(d_c && d_a && d_bhat, flags); },
    [&](const ntt_plan *p, int) { return ptrs_run_pays(p, count) && !ptrs_one_pass_mul(p, count); },
    [&](int first, const LimbSet &ls) {
      const ntt_plan *p   = plans[first];
      const uint64_t  off = (uint64_t)first * limb_stride, N = p->N;
      for(int l = 0; l < ls.n; l++) {
        if(!plans[first + l]->has_fwd) return fail(NTT_ERR_ARG, "plan lacks the forward table");
      }
      if((flags & NTT_MUL_ACCUMULATE) && d_c == d_a) return fail(NTT_ERR_ARG, "an accumulator cannot alias the coefficient operand");
      {
        /* the fused kernel (up to 2^14) or the XCD-local one (above) over the whole run */
        const int r = fwd_mul_ptrs_limb(p, d_c, d_a, d_bhat, count, flags, off, (uint64_t)first * N, stream, &ls);
        if(r != kRunNotServed) return r;
      }
      /* the chain over the run: a's forward transform (in place: scratch), then the element-wise launch */
      const LimbSet sa = with_table(ls, d_a);
      int           r  = run_transform(p, advance(nullptr, off), count, false, false, stream, false, &sa);
      if(r) return r;
      return pointwise_ptrs(p, d_c, d_a, d_bhat, count, (flags & NTT_MUL_LAZY_IN) != 0, (flags & NTT_MUL_ACCUMULATE) != 0, (flags & NTT_MUL_B_BROADCAST) != 0, off,
                            (uint64_t)first * N, stream, plans + first, ls.n, ls.stride);
    },
    [&](int l) { return fwd_mul_ptrs_limb(plans[l], d_c, d_a, d_bhat, count, flags, (uint64_t)l * limb_stride, (uint64_t)l * plans[0]->N, stream); });
}

/* c = a * b in Z_q[X]/(X^N+1).  FP64 plans up to 2^14: fused_product_kernel's PTRS form -- both operands through the forward stages,
 * product, inverse stages in ONE launch, 24N bytes, a and b left as they were.  Otherwise both operands are transformed in place
 * (left in the NTT domain), the products ride in the inverse's first pass where dot_inv_kernel serves (up to 2^14) or go into c
 * before the inverse over c's table.  d_c may be d_a's or d_b's table (the product then lands where that operand was); d_a == d_b
 * squares. */
static bool ptrs_fused_product(const ntt_plan *p, const void *d_a, const void *d_b)
{
  return p->m <= kFusedMax && d_a != d_b && p->fused_product == 1 && p->arith == NTT_ARITH_F64 && p->m >= 8 && !p->generic;
}
static int negacyclic_mul_ptrs_limb(const ntt_plan *p, const uint64_t *const *d_c, const uint64_t *const *d_a, const uint64_t *const *d_b, uint64_t count,
                                    uint64_t limb_off, void *stream, const LimbSet *run = nullptr)
{
  if(!p->has_fwd || !p->has_inv) return fail(NTT_ERR_ARG, "plan lacks a table for this direction");
  const uint64_t nrun = run ? (uint64_t)run->n : 1;
  USE_DEVICE(p->device);
  if(ptrs_fused_product(p, d_a, d_b)) {
    ProdArgs pa  = prod_args(p, ptrs_set(p, run, false), as_words(d_c), as_words(d_a), as_words(d_b), count, stream);
    pa.block_log = (uint32_t)p->m;
    pa.both      = 1;
    set_ptrs(pa, limb_off);
    return launched(dispatch_product(p, pa));
  }
  if(d_a != d_b && p->fused_product == 1 && p->arith == NTT_ARITH_F64) {
    void *ctl = nullptr;
    int   rc  = ptrs_team(p, stream, nrun * count, 2 * nrun * count, &ctl);
    if(rc) return rc;
    if(ctl) {
      /* 2^15..2^17: team_product_kernel's PTRS form -- column stages of both operands, block products, inverse column stages of c
       * as the items of ONE launch; a and b are scratch (their column stages run in place) */
      ProdArgs pa = prod_args(p, ptrs_set(p, run, true), as_words(d_c), as_words(d_a), as_words(d_b), count, stream);
      pa.four     = 1;
      set_ptrs(pa, limb_off);
      set_team(pa, p, ctl, p->m == kTeamBlock + 3 ? 20 : (p->m == kTeamBlock + 4 ? 14 : 8)); /* (fused_product's lags with `four`) */
      return launched(dispatch_product(p, pa));
    }
  }
  if(run) return kRunNotServed;
  uint64_t *const base = advance(nullptr, limb_off);
  const LimbSet   sa{p->limbrec.data(), 1, 0, 0, reinterpret_cast<const uint64_t *>(d_a)};
  const LimbSet   sb{p->limbrec.data(), 1, 0, 0, reinterpret_cast<const uint64_t *>(d_b)};
  const LimbSet   sc{p->limbrec.data(), 1, 0, 0, reinterpret_cast<const uint64_t *>(d_c)};
  int rc = run_transform(p, base, count, false, false, stream, false, &sa);
  if(!rc && d_b != d_a) rc = run_transform(p, base, count, false, false, stream, false, &sb);
  if(!rc && (ptrs_fused(p) || (p->m > kFusedMax && dot_kernel_applies(p)))) {
    /* (inv_dot_ptrs_limb: the fused kernels up to 2^14, the one-launch form or its own chain above) */
    const uint64_t *const *ta = d_a, *const *tb = d_b;
    return inv_dot_ptrs_limb(p, d_c, 1, &ta, &tb, count, 0, limb_off, 0, stream);
  }
  if(!rc) rc = pointwise_ptrs(p, d_c, d_a, d_b, count, false, false, false, limb_off, 0, stream);
  if(!rc) rc = run_transform(p, base, count, true, false, stream, false, &sc);
  return rc;
}

extern "C" int ntt_negacyclic_mul_dev_ptrs(const ntt_plan *p, const uint64_t *const *d_c, const uint64_t *const *d_a, const uint64_t *const *d_b,
                                           uint64_t count, void *stream)
{
  if(!p || !d_c || !d_a || !d_b) return fail(NTT_ERR_ARG, "null argument");
  if(count == 0) return NTT_OK;
  return negacyclic_mul_ptrs_limb(p, d_c, d_a, d_b, count, 0, stream);
}

extern "C" int ntt_rns_negacyclic_mul_dev_ptrs(int nlimbs, ntt_plan *const *plans, const uint64_t *const *d_c, const uint64_t *const *d_a,
                                               const uint64_t *const *d_b, uint64_t count, uint64_t limb_stride, void *stream)
{
  return rns_ptrs_runs(
    nlimbs, plans, count, limb_stride, [&] { return all_given(d_c && d_a && d_b); }, [&](const ntt_plan *p, int) { return ptrs_run_pays(p, count); },
    [&](int first, const LimbSet &ls) {
      const ntt_plan *p   = plans[first];
      const uint64_t  off = (uint64_t)first * limb_stride;
      for(int l = 0; l < ls.n; l++) {
        if(!plans[first + l]->has_fwd || !plans[first + l]->has_inv) return fail(NTT_ERR_ARG, "plan lacks a table for this direction");
      }
      {
        /* fused_product_kernel (up to 2^14) or team_product_kernel (above) over the whole run */
        const int r = negacyclic_mul_ptrs_limb(p, d_c, d_a, d_b, count, off, stream, &ls);
        if(r != kRunNotServed) return r;
      }
      /* both operands into the NTT domain in place, the products in the inverse's first pass (the fused inner-product kernel) or as an
       * element-wise launch in front of the inverse over c's table -- every launch over the whole run */
      const LimbSet sa = with_table(ls, d_a), sb = with_table(ls, d_b);
      int           r  = run_transform(p, advance(nullptr, off), count, false, false, stream, false, &sa);
      if(!r && d_b != d_a) r = run_transform(p, advance(nullptr, off), count, false, false, stream, false, &sb);
      if(r) return r;
      const uint64_t *const *ta = d_a, *const *tb = d_b;
      return inv_dot_ptrs_run(plans + first, ls, d_c, 1, &ta, &tb, count, 0, off, 0, stream);
    },
    [&](int l) { return negacyclic_mul_ptrs_limb(plans[l], d_c, d_a, d_b, count, (uint64_t)l * limb_stride, stream); });
}

extern "C" int ntt_fill_uniform(int device, uint64_t *d_a, uint64_t n, uint64_t q, uint64_t seed, uint64_t offset,
                                void *stream)
{
  int rc = check_device(device);
  if(rc) return rc;
  if(!d_a || q == 0) return fail(NTT_ERR_ARG, "bad argument");
  USE_DEVICE(device);
  hipLaunchKernelGGL(fill_uniform_kernel, dim3(grid_for(n, 256 * 32)), dim3(256), 0, (hipStream_t)stream, d_a, n, q, seed,
                     offset);
  HIP_TRY(hipGetLastError());
  return NTT_OK;
}

extern "C" int ntt_poly_checksum(int device, uint64_t *d_out, const uint64_t *d_a, uint64_t N, uint64_t batch,
                                 void *stream)
{
  int rc = check_device(device);
  if(rc) return rc;
  if(!d_out || !d_a) return fail(NTT_ERR_ARG, "null argument");
  if(batch == 0) return NTT_OK;
  USE_DEVICE(device);
  const unsigned g = batch > 8192 ? 8192u : (unsigned)batch;
  hipLaunchKernelGGL(checksum_kernel, dim3(g), dim3(256), 0, (hipStream_t)stream, d_out, d_a, N, batch);
  HIP_TRY(hipGetLastError());
  return NTT_OK;
}

struct alignas(16) U64x2 {
  uint64_t a, b;
};
__global__ void __launch_bounds__(256) rmw_probe_kernel(U64x2 *a, uint64_t n2, uint64_t mask)
{
  for(uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (uint64_t)gridDim.x * blockDim.x) {
    U64x2 v = a[i];
    v.a ^= mask;
    v.b ^= mask;
    a[i] = v;
  }
}

extern "C" int ntt_rmw_probe(int device, uint64_t *d_a, uint64_t n, uint64_t mask, void *stream)
{
  int rc = check_device(device);
  if(rc) return rc;
  if(!d_a || (n & 1) || ((uintptr_t)d_a & 15)) return fail(NTT_ERR_ARG, "rmw probe: null, odd length or unaligned buffer");
  if(n == 0) return NTT_OK;
  USE_DEVICE(device);
  /* one workgroup per 4 KiB up to 65536 workgroups: the fastest of the grids tried (profiles/r02/skeleton.txt) */
  hipLaunchKernelGGL(rmw_probe_kernel, dim3(grid_for(n / 2, 65536u)), dim3(256), 0, (hipStream_t)stream, (U64x2 *)d_a, n / 2, mask);
  HIP_TRY(hipGetLastError());
  return NTT_OK;
}

/* out-of-place copy, 16 bytes per lane, plain grid-stride: the shape the microarchitecture guide quotes its achievable HBM rate
 * for (MI355X_MICROARCH.md: about 6.3 TB/s of read + written bytes) */
__global__ void __launch_bounds__(256) copy_probe_kernel(U64x2 *dst, const U64x2 *src, uint64_t n2)
{
  /* (one 16-byte word per thread where the grid allows it, i.e. always in practice: the fastest of eight copy shapes measured,
   * 6.3 TB/s -- a grid-stride loop over the same slab 4.8-5.5, tools/copy_variants.hip) */
  for(uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (uint64_t)gridDim.x * blockDim.x) dst[i] = src[i];
}

extern "C" int ntt_copy_probe(int device, uint64_t *d_dst, const uint64_t *d_src, uint64_t n, void *stream)
{
  int rc = check_device(device);
  if(rc) return rc;
  if(!d_dst || !d_src || (n & 1) || (((uintptr_t)d_dst | (uintptr_t)d_src) & 15)) return fail(NTT_ERR_ARG, "copy probe: null, odd length or unaligned buffer");
  if(n == 0) return NTT_OK;
  USE_DEVICE(device);
  hipLaunchKernelGGL(copy_probe_kernel, dim3(grid_for(n / 2, 1u << 24)), dim3(256), 0, (hipStream_t)stream, (U64x2 *)d_dst, (const U64x2 *)d_src, n / 2);
  HIP_TRY(hipGetLastError());
  return NTT_OK;
}

/* The memory shape of the 2^14 block kernels without their arithmetic (tools/skel.hip "T1024 C16 ld16 st1 mode1": the best
 * memory-only skeleton measured, profiles/r02/skeleton.txt): one persistent 1024-thread workgroup per CU, a block of 2^14
 * words per iteration as eight 16-byte loads per thread with the NEXT block's loads in flight (register prefetch), XOR,
 * eight 16-byte stores -- every load and store instruction of a wave covers one contiguous KiB. */
__global__ void __launch_bounds__(1024, 4) shape_probe_kernel(uint64_t *a, uint64_t nblocks, uint64_t mask)
{
  constexpr int  LOGN = 14;
  const uint32_t t    = threadIdx.x;
  uint64_t       b    = blockIdx.x;
  if(b >= nblocks) return;
  u64x2 raw[8];
  {
    const __amdgpu_buffer_rsrc_t r = block_rsrc<LOGN>(a + (b << LOGN));
#pragma unroll
    for(int h = 0; h < 8; h++) raw[h] = buffer_load_u64x2(r, t * 16u, (uint32_t)h * 16384u);
  }
  typedef unsigned int v4u32 __attribute__((ext_vector_type(4)));
  for(; b < nblocks; b += gridDim.x) {
    u64x2 x[8];
#pragma unroll
    for(int h = 0; h < 8; h++) x[h] = u64x2{raw[h].a ^ mask, raw[h].b ^ mask};
    const bool     more = b + gridDim.x < nblocks;
    const uint64_t nb   = more ? b + gridDim.x : b;
    {
      const __amdgpu_buffer_rsrc_t r = block_rsrc<LOGN>(a + (nb << LOGN), more);
#pragma unroll
      for(int h = 0; h < 8; h++) raw[h] = buffer_load_u64x2(r, t * 16u, (uint32_t)h * 16384u);
    }
    const __amdgpu_buffer_rsrc_t w = block_rsrc<LOGN>(a + (b << LOGN));
#pragma unroll
    for(int h = 0; h < 8; h++) {
      v4u32 v;
      v.x = (unsigned)x[h].a;
      v.y = (unsigned)(x[h].a >> 32);
      v.z = (unsigned)x[h].b;
      v.w = (unsigned)(x[h].b >> 32);
      __builtin_amdgcn_raw_buffer_store_b128(v, w, (int)(t * 16u), (int)((uint32_t)h * 16384u), 0);
    }
  }
}

extern "C" int ntt_shape_probe(int device, uint64_t *d_a, uint64_t n, uint64_t mask, void *stream)
{
  int rc = check_device(device);
  if(rc) return rc;
  if(!d_a || (n & ((1ull << 14) - 1)) || ((uintptr_t)d_a & 15)) return fail(NTT_ERR_ARG, "shape probe: null, unaligned or not a multiple of 2^14 words");
  if(n == 0) return NTT_OK;
  USE_DEVICE(device);
  int cus = 256;
  {
    hipDeviceProp_t prop;
    if(hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) cus = prop.multiProcessorCount;
  }
  const uint64_t nblocks = n >> 14;
  const unsigned grid    = (unsigned)(nblocks < (uint64_t)cus ? nblocks : (uint64_t)cus);
  hipLaunchKernelGGL(shape_probe_kernel, dim3(grid), dim3(1024), 0, (hipStream_t)stream, d_a, nblocks, mask);
  HIP_TRY(hipGetLastError());
  return NTT_OK;
}
