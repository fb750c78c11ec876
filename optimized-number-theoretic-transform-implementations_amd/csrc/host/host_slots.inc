/* host/host_slots.inc -- BFV / BGV slots: ntt_plan_enable_slots, ntt_slot_position, ntt_slots_encode_batch, ntt_slots_decode_batch and the
 * strided forms.  A section of ntt_host.hip (one translation unit, included from there in order); not compiled by itself.  The kernels are
 * in slots.hip and the slots_f64*.hip units; this section sees their launchers only (ntt_slots.h, which states the slot order).
 *
 *   fused        FP64 policies at N = 2^6..2^14, where NTT_OPT_SLOTS_FUSED on the plan allows it: ONE launch -- slots_inv_kernel (encode:
 *                the inverse transform reading v through ipos) or slots_fwd_kernel (decode: the forward transform storing through
 *                ipos; d_a is only read).  16N bytes per polynomial.
 *   composition  anything else (integer or radix-4 plans, N < 2^6, N >= 2^15, NTT_OPT_SLOTS_FUSED 0): slots_perm_kernel and the plan's
 *                transform in place on d_a -- encode gathers through ipos into d_a, then the inverse; decode runs the forward on d_a,
 *                then gathers through pos into d_v.  32N bytes per polynomial.
 * Both give the same words.  Everything is checked before the first launch.  Nothing is allocated, the host is not synchronised and no
 * memset is issued: the calls can be captured into a graph (ntt_plan_enable_slots allocates and synchronises: outside capture). */

extern "C" uint64_t ntt_slot_position(uint64_t N, uint64_t i)
{
  if(N < 2 || (N & (N - 1)) || N > (1ull << 62) || i >= N) return UINT64_MAX;
  return slot_position((unsigned)h_log2(N), i);
}

extern "C" int ntt_plan_enable_slots(ntt_plan *p)
{
  if(!p) return fail(NTT_ERR_ARG, "null plan");
  if(p->d_pos && p->d_ipos) return NTT_OK;
  if(p->m < 1 || p->m > 28) return fail(NTT_ERR_ARG, "slots: N out of range");
  USE_DEVICE(p->device);
  uint32_t * pos = nullptr, *ipos = nullptr;
  hipStream_t bs = nullptr; /* a private non-blocking stream, as the plan's other tables (device_build_direction) */
  hipError_t  e  = hipMalloc((void **)&pos, p->N * sizeof(uint32_t));
  if(e == hipSuccess) e = hipMalloc((void **)&ipos, p->N * sizeof(uint32_t));
  if(e == hipSuccess) e = hipStreamCreateWithFlags(&bs, hipStreamNonBlocking);
  if(e == hipSuccess) e = launch_slots_tables(pos, ipos, (uint32_t)p->m, bs);
  if(bs) {
    const hipError_t es = hipStreamSynchronize(bs);
    if(e == hipSuccess) e = es;
    (void)hipStreamDestroy(bs);
  }
  if(e != hipSuccess) {
    if(pos) (void)hipFree(pos);
    if(ipos) (void)hipFree(ipos);
    return fail(e == hipErrorOutOfMemory ? NTT_ERR_NOMEM : NTT_ERR_HIP, std::string("slot table build: ") + hipGetErrorString(e));
  }
  p->d_pos  = pos;
  p->d_ipos = ipos;
  return NTT_OK;
}

/* where the fused kernels are built */
static bool slots_fused_built(const ntt_plan *p) { return p->arith == NTT_ARITH_F64 && !p->generic && p->m >= kFusedMin && p->m <= kFusedMax; }

/* The automatic choice (NTT_OPT_SLOTS_FUSED -1), from profiles/r21/slots_bench.txt: t = 65537, 2^13 and 2^14, 64 and 1024 polynomials,
 * composition time / fused time as ranges over five rounds of alternating processes; a figure's own spread over the rounds is
 * 1.00-1.04.  The fused kernel is the default where it is not slower by more than that spread at both batch sizes:
 *   encode   2^13: 1.54-1.61 (64) and 2.33-2.36 (1024); 2^14: 1.40-1.42 and 2.37-2.39.  Fused.
 *   decode   2^13: 1.19-1.20 and 1.84-1.86.  Fused through 2^13 (smaller sizes follow 2^13: not measured).
 *            2^14: 1.30-1.33 at 64 polynomials, but 0.96-0.98 at 1024 (spread 1.02): the scattered 8-byte stores of a full chip cost
 *            more than the launch and the 16N bytes they save.  Composition.
 * The fused kernels run at 0.15-0.30 (64 polynomials) and 0.24-0.40 (1024) of ntt_copy_probe's rate at 16N bytes per polynomial, the
 * composition at 0.12-0.19 and 0.17-0.25: untuned (the gathers are 8-byte accesses behind a dependent table load). */
static bool slots_fused_applies(const ntt_plan *p, bool encode)
{
  if(!slots_fused_built(p)) return false;
  if(p->slots_fused >= 0) return p->slots_fused == 1;
  return encode || p->m <= 13;
}

static int slots_perm_launch(const ntt_plan *pt, uint64_t *out, uint64_t out_stride, const uint64_t *in, uint64_t in_stride, const uint32_t *tab,
                             uint64_t batch, void *stream)
{
  SlotsPermArgs sa{};
  sa.out        = out;
  sa.in         = in;
  sa.tab        = tab;
  sa.out_stride = out_stride;
  sa.in_stride  = in_stride;
  sa.batch      = batch;
  sa.logn       = (uint32_t)pt->m;
  sa.max_grid   = pt->max_grid;
  sa.stream     = (hipStream_t)stream;
  const hipError_t e = launch_slots_perm(sa);
  if(e != hipSuccess) return fail(NTT_ERR_HIP, std::string("slots_perm_kernel: ") + hipGetErrorString(e));
  return NTT_OK;
}

static int slots_call(const ntt_plan *pt, uint64_t *d_a, uint64_t *d_v, bool encode, uint64_t v_stride, uint64_t a_stride, uint64_t batch,
                      unsigned flags, void *stream)
{
  if(!pt) return fail(NTT_ERR_ARG, "null plan");
  if(flags) return fail(NTT_ERR_ARG, "unknown flag");
  if(!pt->d_pos || !pt->d_ipos) return fail(NTT_ERR_ARG, "slots: the plan has no slot tables (ntt_plan_enable_slots)");
  if(encode ? !pt->has_inv : !pt->has_fwd) return fail(NTT_ERR_ARG, encode ? "slots: the plan lacks the inverse table" : "slots: the plan lacks the forward table");
  const uint64_t N = pt->N;
  if(v_stride < N || a_stride < N || v_stride > (1ull << 40) || a_stride > (1ull << 40))
    return fail(NTT_ERR_ARG, "layout: the polynomial strides must be N .. 2^40 words");
  if(batch == 0) return NTT_OK;
  if(!d_a || !d_v) return fail(NTT_ERR_ARG, "null argument");
  /* gathers and scatters cross the whole polynomial while other workgroups run: no overlap at all */
  if(galois_overlap(galois_span(d_v, N, 1, batch, 0, v_stride), galois_span(d_a, N, 1, batch, 0, a_stride)))
    return fail(NTT_ERR_ARG, "slots: the slot side overlaps the coefficient side");
  USE_DEVICE(pt->device);
  if(slots_fused_applies(pt, encode)) {
    SlotsArgs sa{};
    sa.a        = d_a;
    sa.v        = d_v;
    sa.ipos     = pt->d_ipos;
    sa.limb     = pt->limbrec.data();
    sa.a_stride = a_stride;
    sa.v_stride = v_stride;
    sa.batch    = batch;
    sa.logn     = (uint32_t)pt->m;
    sa.encode   = encode;
    sa.max_grid = pt->max_grid;
    sa.num_cus  = pt->num_cus;
    sa.stream   = (hipStream_t)stream;
    const hipError_t e = with_f64_class(pt->kcls, [&](auto k) { return launch_slots<typename decltype(k)::A, decltype(k)::KSH>(sa); });
    if(e != hipSuccess) return fail(NTT_ERR_HIP, std::string(encode ? "slots_inv_kernel: " : "slots_fwd_kernel: ") + hipGetErrorString(e));
    return NTT_OK;
  }
  const LimbSet own{pt->limbrec.data(), 1, 0, a_stride};
  if(encode) {
    const int rc = slots_perm_launch(pt, d_a, a_stride, d_v, v_stride, pt->d_ipos, batch, stream);
    return rc ? rc : run_transform(pt, d_a, batch, true, false, stream, false, &own);
  }
  const int rc = run_transform(pt, d_a, batch, false, false, stream, false, &own);
  return rc ? rc : slots_perm_launch(pt, d_v, v_stride, d_a, a_stride, pt->d_pos, batch, stream);
}

extern "C" int ntt_slots_encode_batch(const ntt_plan *pt, uint64_t *d_a, const uint64_t *d_v, uint64_t batch, unsigned flags, void *stream)
{
  const uint64_t N = pt ? pt->N : 0;
  return slots_call(pt, d_a, const_cast<uint64_t *>(d_v), true, N, N, batch, flags, stream);
}

extern "C" int ntt_slots_encode_batch_strided(const ntt_plan *pt, uint64_t *d_a, const uint64_t *d_v, uint64_t v_poly_stride,
                                              uint64_t a_poly_stride, uint64_t batch, unsigned flags, void *stream)
{
  return slots_call(pt, d_a, const_cast<uint64_t *>(d_v), true, v_poly_stride, a_poly_stride, batch, flags, stream);
}

extern "C" int ntt_slots_decode_batch(const ntt_plan *pt, uint64_t *d_v, uint64_t *d_a, uint64_t batch, unsigned flags, void *stream)
{
  const uint64_t N = pt ? pt->N : 0;
  return slots_call(pt, d_a, d_v, false, N, N, batch, flags, stream);
}

extern "C" int ntt_slots_decode_batch_strided(const ntt_plan *pt, uint64_t *d_v, uint64_t *d_a, uint64_t v_poly_stride, uint64_t a_poly_stride,
                                              uint64_t batch, unsigned flags, void *stream)
{
  return slots_call(pt, d_a, d_v, false, v_poly_stride, a_poly_stride, batch, flags, stream);
}
