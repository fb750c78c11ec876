/* host/host_plan.inc -- plans: on-device table construction, plan creation / destruction / info, options, the control blocks of the XCD-local launches.
 * A section of ntt_host.hip (one translation unit, included from there in order); not compiled by itself. */

/* ------------------------------------------------------------------ */
/* on-device table construction (SURVEY f2)                             */
/* ------------------------------------------------------------------ */
/*
 * The reference builds its tables on the host with % and / on 128-bit integers (tests/test_cases.h:212-311,
 * include/internal/pre_compute.h:38-105: "we don't care about the performance").  A plan for N = 2^17 needs
 * 2 x 2^17 modular powers plus one 128-by-64-bit division (integer policies) or one FP64 division (FP64 policy)
 * per entry -- milliseconds on one host core per plan, times primes, times GPUs.  Here the host only squares
 * the root log2 N times; every table entry is produced by one GPU thread:
 *   w[k] = root^bitrev(k) = product of root^(2^j) over the set bits j of bitrev(k)   (reference layout, :38-51)
 *   con  = floor(w * 2^64 / q) by 64 steps of shift-and-subtract (exact)                 (:68-77)
 *   FP64 : balanced w and its correctly rounded quotient by q (v_div: IEEE division)
 *   radix-4 expanded table e[2k] = w[k], e[4k+1] = w[k] w[2k], e[4k+3] = q - w[k] w[2k+1]  (:85-105)
 * Caller-supplied tables (ntt_plan_create_from_tables, the reference-signature entry points) still take the host
 * route: their entries are data, not something to regenerate.
 */
struct PowBasis {
  uint64_t p[32]; /* base^(2^j) mod q */
};

__device__ __forceinline__ uint64_t dev_precon64(uint64_t w, uint64_t q)
{
  uint64_t r = w, con = 0; /* w < q < 2^61: 2r never overflows */
  for(int i = 0; i < 64; i++) {
    r <<= 1;
    const uint64_t ge = r >= q;
    r -= ge ? q : 0;
    con = (con << 1) | ge;
  }
  return con;
}

__device__ __forceinline__ uint64_t dev_brev(uint64_t v, unsigned bits) { return bits ? (__brevll(v) >> (64 - bits)) : 0; }

__global__ void __launch_bounds__(256) power_table_kernel(uint64_t *w, uint64_t N, unsigned m, PowBasis basis, ArithU64::consts c)
{
  for(uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < N; k += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t e = dev_brev(k, m);
    uint64_t       acc = 1 % c.q;
    for(unsigned j = 0; j < m; j++) {
      if((e >> j) & 1) acc = ArithU64::mulmod_full(acc, basis.p[j], c);
    }
    w[k] = acc;
  }
}

/* records N .. N+15 behind an inverse table: N^-1 * winv[k] (run_group0_folded) */
__device__ __forceinline__ uint64_t folded_word(const uint64_t *w, uint64_t N, uint64_t k, uint64_t ninv, const ArithU64::consts &c)
{
  if(k < N) return w[k];
  const uint64_t j = k - N;
  return j < N ? ArithU64::mulmod_full(ninv, w[j], c) : ninv;
}

__global__ void __launch_bounds__(256) records_u64_kernel(TwU64 *out, const uint64_t *w, uint64_t N, uint64_t total, uint64_t ninv,
                                                          ArithU64::consts c)
{
  for(uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t v = folded_word(w, N, k, ninv, c);
    out[k]           = TwU64{v, dev_precon64(v, c.q)};
  }
}

__global__ void __launch_bounds__(256) records_f64_kernel(TwF64 *out, double *out8, const uint64_t *w, uint64_t N, uint64_t total,
                                                          uint64_t ninv, ArithU64::consts c)
{
  const double qd = (double)c.q; /* q < 2^52: exact */
  for(uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t v  = folded_word(w, N, k, ninv, c);
    const double   wb = v > c.q / 2 ? -(double)(c.q - v) : (double)v;
    out[k]            = TwF64{wb, wb / qd};
    if(k < N) out8[k] = wb;
  }
}

__global__ void __launch_bounds__(256) records_r4_kernel(TwU64 *out, const uint64_t *w, uint64_t N, ArithU64::consts c)
{
  for(uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < 2 * N; i += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t v;
    if((i & 1) == 0) {
      v = w[i >> 1];
    } else {
      const uint64_t k = i >> 2;
      if(k == 0) {
        v = 0; /* slots 1 and 3 stay 0 as in the reference (pre_compute.h:90-93) */
      } else if((i & 3) == 1) {
        v = ArithU64::mulmod_full(w[k], w[2 * k], c);
      } else {
        v = c.q - ArithU64::mulmod_full(w[k], w[2 * k + 1], c);
      }
    }
    out[i] = TwU64{v, dev_precon64(v, c.q)};
  }
}

/* ------------------------------------------------------------------ */
/* plan                                                                */
/* ------------------------------------------------------------------ */
constexpr int kWideClass = -1; /* ntt_plan::kcls of the FP64 policy for 2^51(1+2^-10) < q < 2^52 (ArithF64W) */

/* a headroom class as the template arguments of the FP64 kernel instances built for it, in the style of with_int:
 * f(KernelClass<policy, class>{}), so that a launcher template L is reached as L<typename decltype(k)::A, decltype(k)::KSH>
 * (with_class, host_transforms.inc: the same over a plan's policy, the integer ones included) */
template <class Arith, int K> struct KernelClass {
  using A                  = Arith;
  static constexpr int KSH = K;
};
template <class F> static hipError_t with_f64_class(int kc, F &&f)
{
  return kc == kWideClass ? f(KernelClass<ArithF64W, 0>{}) : kc == 18 ? f(KernelClass<ArithF64, 18>{}) : kc == 1 ? f(KernelClass<ArithF64, 1>{}) : f(KernelClass<ArithF64, 0>{});
}

struct ntt_plan {
  int      device  = 0;
  uint64_t N       = 0, q = 0, root = 0;
  int      m       = 0;
  int      arith   = NTT_ARITH_U64; /* resolved: U64, F64 or U64_R4 */
  int      kcls    = 0;             /* instantiated FP64 headroom class */
  int      int_cls = -1;            /* integer policy: -1 = the reference's butterflies (ArithU64), else the headroom class K of
                                     * ArithU64X<K> the transforms run with (same tables, same canonical results) */
  bool     generic = false;
  bool     has_fwd = false, has_inv = false;
  void *   d_fwd   = nullptr; /* U64/F64: N records (+16 folded N^-1 records, inverse); U64_R4: 2N expanded records */
  void *   d_inv   = nullptr;
  void *   d_fwd8  = nullptr; /* compact forward twiddles (FP64 policy) */
  void *   d_inv8  = nullptr; /* compact inverse twiddles (FP64 policy) */
  ArithU64::consts cu{};
  F64Consts        cf{};
  std::vector<unsigned char> limbrec; /* this plan's LimbRec<A> (table pointers + constants): copied into the kernel arguments of every launch */
  std::vector<unsigned char> limbrec_mid; /* radix-4 policy: the same with the record of 1 in place of N^-1 -- what the block pass of a
                                           * two-pass INVERSE multiplies by (the reference's N^-1 pass, src/ntt_radix4.c:111-113, comes
                                           * once, after the last level: in the column pass's store) */
  /* XCD-local two-pass launches (team_kernel, N = 2^15..2^17): queue heads and per-polynomial counters in device memory,
   * one buffer per stream the plan is used on (launches on one stream are ordered; two streams must not share counters) */
  int        xcd_local = -1; /* 1 on, 0 off, -1 automatic */
  int        team_lag = 0, team_wpc = 0; /* 0 = the kernel's defaults */
  struct TeamBuf {
    void * stream;
    void * d;       /* block of the direct launches on this stream */
    size_t bytes;
    void * g;       /* block of the launches CAPTURED on this stream: its address is baked into graph nodes, so it is never
                     * freed, regrown or shared with direct launches before the plan is destroyed */
    size_t gbytes;
  };
  /* The control blocks are the ONE piece of plan state a batched call (const ntt_plan *) may touch: mutable, every access
   * under team_mu.  ntt_plan_reserve / NTT_OPT_MAX_BATCH_HINT size them ahead of time so that no batched call allocates. */
  mutable std::vector<TeamBuf> team_bufs;
  mutable std::vector<void *>  team_retired; /* outgrown direct blocks: launches still queued may use them, freed with the plan */
  mutable std::mutex           team_mu;
  uint64_t                     batch_hint = 0; /* NTT_OPT_MAX_BATCH_HINT: polynomials x limbs of the largest call; blocks of new streams start at this size */
  mutable uint64_t             ctl_allocs = 0; /* hipMalloc calls team_buffer has made for this plan (NTT_OPT_CTL_ALLOCATIONS, read-only) */
  /* pointer batches handed over as HOST arrays (ntt_transform_ptrs): the sorted addresses travel to the device through a pinned
   * staging buffer and live in a device table, one pair per stream the plan is used on (stream order makes the reuse safe: the next
   * call's copy queues behind the previous call's kernels); grown by retiring, like the control blocks; under team_mu */
  struct PtrBuf {
    void *     stream;
    uint64_t * d;      /* device table */
    uint64_t * h;      /* pinned host staging */
    size_t     words;
    hipEvent_t copied; /* the last upload from h has completed (h may be rewritten) */
  };
  mutable std::vector<PtrBuf> ptr_bufs;
  mutable std::vector<std::pair<void *, void *>> ptr_retired; /* {device, pinned host} */
  hipStream_t      own_stream = nullptr; /* used by ntt_batch_multi */
  int              max_grid   = 0;
  int              rns_launch = -1; /* ntt_rns_*: 0 = one launch over a run of limbs wherever it is built, 1 = one launch chain per limb,
                                     * -1 = where it pays (rns_one_launch_pays); read from the run's first plan */
  int              dot_fused  = 1;  /* the NTT-domain product kernels (dot_inv_kernel, fwd_mul_kernel): 0 = pointwise launches + transform */
  int              rescale_fused = 1; /* ntt_rns_rescale_batch in the NTT domain: 1 = rescale_fwd_kernel where it is built,
                                      * 0 = the inverse / element-wise / forward sandwich everywhere; read from plans[0] */
  int              modup_fused = -1; /* ntt_rns_mod_up_mul_batch: 1 = modup_mul_kernel where it is built, 0 = the composition everywhere,
                                      * -1 = where the recorded measurement says it is not slower (modup_fused_pays); read from plans[0] */
  int              pair_fused = -1;  /* the pair key products: 1 = modup_mul2_kernel where it is built, 0 = the composition everywhere,
                                      * -1 = where the recorded measurement says it is not slower (pair_fused_pays); read from plans[0] */
  int              moddown_add_fused = -1; /* ntt_rns_mod_down_add_batch: 1 = ksfold_fwd_kernel where it is built, 0 = the composition
                                      * everywhere, -1 = where the recorded measurement says it is not slower (ksfold_pays); plans[0] */
  int              bgv_fused = -1;   /* the BGV ModDown calls: 1 = moddown_bgv_fwd_kernel where it is built, 0 = the sandwich everywhere,
                                      * -1 = where the recorded measurement says it is not slower (bgv_fused_applies); plans[0] */
  int              lift_fused = -1;  /* the lifts with NTT_LIFT_TRANSFORMED: 1 = lift_fwd_kernel where it is built, 0 = the composition
                                      * everywhere, -1 = the default rule (lift_fused_applies); plans[0] */
  int              slots_fused = -1; /* ntt_slots_encode_batch, ntt_slots_decode_batch: 1 = slots_inv_kernel / slots_fwd_kernel where they are
                                      * built, 0 = the composition everywhere, -1 = the default rule (slots_fused_applies) */
  int              sample_fused = -1; /* ntt_rns_sample_batch with NTT_SAMPLE_TRANSFORMED: 1 = sample_fwd_kernel where it is built, 0 = the
                                      * composition everywhere, -1 = the default rule (sample_fused_applies); plans[0] */
  uint32_t *       d_pos  = nullptr; /* slot tables (ntt_plan_enable_slots; ntt_slots.h): pos and its inverse, N words each; null */
  uint32_t *       d_ipos = nullptr; /* until enabled */
  int              block_oversub = 0; /* persistent block kernels: workgroups per resident slot (0 = the kernels' defaults) */
  int              num_cus    = 256;
  int              chunk_mib  = 256; /* bytes of one multi-pass chunk (Infinity Cache residency) */
  int              block_log  = 0;     /* multi-pass transforms: block size below the column passes (0 = multi_pass_block's choice) */
  int              fused_product = 1; /* N = 2^8..2^17, FP64: ntt_negacyclic_mul_batch through the fused product kernels (0: four-launch
                                       * chain; 2: as 1, but a's forward transform always as a launch of its own) */
  int              one_pass   = -1;    /* 2^15, FP64 policies: the transform in ONE pass, the polynomial in the registers of one workgroup
                                        * (onepass_kernel): 1 on, 0 off, -1 = batches that give every second CU a polynomial, unless
                                        * xcd_local or block_log is set explicitly (one_pass_pays) */
  int              two_phase  = -1;    /* 2^16, 2^17: both passes of a polynomial inside one workgroup (twophase_kernel):
                                        * 1 on, 0 off, -1 where it measured faster (forward 2^16, scheduled FP64 policy: +3 %) */
};

static bool is_pow2(uint64_t n) { return n && !(n & (n - 1)); }

/* N = 2^15, FP64 policies: whether a call over `polys` polynomials (batch x limbs) takes the one-pass kernels (onepass_kernel,
 * onepass_mul_kernel).  NTT_OPT_ONE_PASS 1 / 0 decides; the automatic choice (-1) wants a polynomial for every second CU and yields to
 * an explicit NTT_OPT_XCD_LOCAL 1 or NTT_OPT_BLOCK_LOG, which ask for the two-pass forms. */
static bool one_pass_pays(const ntt_plan *p, uint64_t polys)
{
  if(p->one_pass >= 0) return p->one_pass == 1;
  return p->xcd_local != 1 && p->block_log == 0 && 2 * polys >= (uint64_t)p->num_cus;
}
static bool h_is_prime(uint64_t n); /* deterministic Miller-Rabin (below) */

/* headroom class of ArithU64X for q (ntt_arith.h): B = 8 * 2^K multiples of q below 2^64; -1 = not served (reduce_any
 * wants q >= 2^40 -- smaller moduli belong to the FP64 policies anyway -- and 8q < 2^64) */
static int int_wide_class(uint64_t q)
{
  if(q < (1ull << 40) || q >= (1ull << 61)) return -1;
  return q < (1ull << 58) ? 3 : (q < (1ull << 60) ? 1 : 0);
}

static int resolve_arith(int requested, uint64_t q, int m, int *out)
{
  /* FP64: the scheduled policy up to 2^51(1+2^-10), the reduce-both-operands policy (ArithF64W) up to 2^52 */
  if(requested == NTT_ARITH_AUTO) requested = (h_f64_eligible(q) || h_f64w_eligible(q)) ? NTT_ARITH_F64 : NTT_ARITH_U64;
  if(requested == NTT_ARITH_F64 && !h_f64_eligible(q) && !h_f64w_eligible(q)) {
    return fail(NTT_ERR_UNSUPPORTED, "FP64 arithmetic needs q < 2^52");
  }
  if(requested == NTT_ARITH_U64_R4 && (m < kFusedMin || m > kRadix4Max)) {
    return fail(NTT_ERR_UNSUPPORTED, "the radix-4 policy covers 2^6..2^18");
  }
  if(requested == NTT_ARITH_U64_R4 && q >= (1ull << 60)) return fail(NTT_ERR_UNSUPPORTED, "radix-4 lazy range needs 16q < 2^64");
  if(requested != NTT_ARITH_F64 && requested != NTT_ARITH_U64 && requested != NTT_ARITH_U64_R4) return fail(NTT_ERR_ARG, "bad arith");
  *out = requested;
  return NTT_OK;
}

template <class TW> static int upload_records(void **d_out, const std::vector<TW> &host)
{
  HIP_TRY(hipMalloc(d_out, host.size() * sizeof(TW)));
  HIP_TRY(hipMemcpy(*d_out, host.data(), host.size() * sizeof(TW), hipMemcpyHostToDevice));
  return NTT_OK;
}

template <class TW, class MK>
static int upload_table(void **d_out, const std::vector<uint64_t> &w, uint64_t q, MK mk)
{
  std::vector<TW> host(w.size());
  for(size_t i = 0; i < w.size(); i++) host[i] = mk(w[i], q);
  return upload_records(d_out, host);
}

/* integer records {w, con}: con from the caller's own precomputation when given (the reference passes
 * w_con next to every table, tests/test_cases.h:226-251), else floor(w * 2^64 / q) */
static int upload_u64(void **d_out, const std::vector<uint64_t> &w, const std::vector<uint64_t> &con, uint64_t q)
{
  std::vector<TwU64> host(w.size());
  for(size_t i = 0; i < w.size(); i++) host[i] = i < con.size() ? TwU64{w[i], con[i]} : h_tw_u64(w[i], q);
  return upload_records(d_out, host);
}

/* What a plan is built from: radix-2 power tables in bit-reversed order (either may be empty), optionally
 * the caller's Shoup precomputation for them, and -- radix-4 policy built from caller tables -- the 2N-entry
 * expanded tables as they are (pre_compute.h:85-105). */
struct TableSet {
  std::vector<uint64_t> fwd, inv, fwd_con, inv_con;
  std::vector<uint64_t> efwd, einv, efwd_con, einv_con;
  uint64_t gen_root = 0, gen_root_inv = 0; /* both non-zero: generate every table on the device from these roots */
};

/* one direction's tables of plan p from `base` (root or its inverse), on the device */
static int device_build_direction(ntt_plan *p, uint64_t base, bool inverse, uint64_t ninv)
{
  const uint64_t N = p->N, q = p->q;
  PowBasis       basis{};
  uint64_t       sq = base % q;
  for(int j = 0; j < p->m && j < 32; j++) {
    basis.p[j] = sq;
    sq         = h_mulmod(sq, sq, q);
  }
  /* a private non-blocking stream: the build neither waits for nor stalls the caller's streams (the legacy NULL stream
   * + hipDeviceSynchronize of round 2 did both).  Plans must still be created outside stream capture: hipMalloc and
   * the synchronisation below are not capturable (INTEGRATION.md). */
  hipStream_t bs = nullptr;
  HIP_TRY(hipStreamCreateWithFlags(&bs, hipStreamNonBlocking));
  uint64_t *d_w = nullptr;
  {
    hipError_t em = hipMalloc((void **)&d_w, N * sizeof(uint64_t));
    if(em != hipSuccess) {
      (void)hipStreamDestroy(bs);
      return fail(em == hipErrorOutOfMemory ? NTT_ERR_NOMEM : NTT_ERR_HIP, std::string("device table build: ") + hipGetErrorString(em));
    }
  }
  const unsigned g = (unsigned)((N + 255) / 256 > 4096 ? 4096 : (N + 255) / 256);
  hipLaunchKernelGGL(power_table_kernel, dim3(g), dim3(256), 0, bs, d_w, N, (unsigned)p->m, basis, p->cu);
  int         rc    = NTT_OK;
  void **     d_rec = inverse ? &p->d_inv : &p->d_fwd;
  void **     d_cmp = inverse ? &p->d_inv8 : &p->d_fwd8;
  hipError_t  e     = hipSuccess;
  if(p->arith == NTT_ARITH_U64_R4) {
    e = hipMalloc(d_rec, 2 * N * sizeof(TwU64));
    if(e == hipSuccess) hipLaunchKernelGGL(records_r4_kernel, dim3(g), dim3(256), 0, bs, (TwU64 *)*d_rec, d_w, N, p->cu);
  } else {
    const uint64_t total = inverse ? N + 16 : N;
    if(p->arith == NTT_ARITH_F64) {
      e = hipMalloc(d_rec, total * sizeof(TwF64));
      if(e == hipSuccess) e = hipMalloc(d_cmp, N * sizeof(double));
      if(e == hipSuccess)
        hipLaunchKernelGGL(records_f64_kernel, dim3(g), dim3(256), 0, bs, (TwF64 *)*d_rec, (double *)*d_cmp, d_w, N, total, ninv, p->cu);
    } else {
      e = hipMalloc(d_rec, total * sizeof(TwU64));
      if(e == hipSuccess) hipLaunchKernelGGL(records_u64_kernel, dim3(g), dim3(256), 0, bs, (TwU64 *)*d_rec, d_w, N, total, ninv, p->cu);
    }
  }
  if(e == hipSuccess) e = hipGetLastError();
  {
    const hipError_t es = hipStreamSynchronize(bs); /* always: d_w is freed below */
    if(e == hipSuccess) e = es;
  }
  (void)hipStreamDestroy(bs);
  (void)hipFree(d_w);
  if(e != hipSuccess) rc = fail(e == hipErrorOutOfMemory ? NTT_ERR_NOMEM : NTT_ERR_HIP, std::string("device table build: ") + hipGetErrorString(e));
  return rc;
}

/* the plan's LimbRec as raw bytes (host copy): the layout the kernels read (ntt_kernels.h) */
static std::vector<unsigned char> limbrec_bytes(const ntt_plan *p)
{
  std::vector<unsigned char> b;
  if(p->arith == NTT_ARITH_F64) {
    LimbRec<ArithF64> r{};
    r.tw_f  = static_cast<const TwF64 *>(p->d_fwd);
    r.tw8_f = static_cast<const double *>(p->d_fwd8);
    r.tw_i  = static_cast<const TwF64 *>(p->d_inv);
    r.tw8_i = static_cast<const double *>(p->d_inv8);
    r.c     = p->cf;
    b.resize(sizeof r);
    memcpy(b.data(), &r, sizeof r);
  } else {
    LimbRec<ArithU64> r{};
    r.tw_f = static_cast<const TwU64 *>(p->d_fwd);
    r.tw_i = static_cast<const TwU64 *>(p->d_inv);
    r.c    = p->cu;
    b.resize(sizeof r);
    memcpy(b.data(), &r, sizeof r);
  }
  return b;
}
static_assert(sizeof(LimbRec<ArithU64>) == sizeof(LimbRec<ArithU64R4>) && sizeof(LimbRec<ArithF64>) == sizeof(LimbRec<ArithF64W>),
              "the policies of one family share a record layout");


/* ninv_override: 0 = derive N^-1 */
static int plan_build(ntt_plan **out, int device, uint64_t N, uint64_t q, uint64_t root, const TableSet &ts, int arith,
                      uint64_t ninv_override)
{
  if(!out) return fail(NTT_ERR_ARG, "null plan pointer");
  *out = nullptr;
  if(!is_pow2(N) || N < 2 || N > (1ull << 28)) return fail(NTT_ERR_ARG, "N must be a power of two in [2,2^28]");
  if(q < 3 || !(q & 1) || q >= (1ull << 61)) return fail(NTT_ERR_ARG, "q must be odd, 3 <= q < 2^61");
  if((q - 1) % (2 * N) != 0) return fail(NTT_ERR_ARG, "2N must divide q-1");
  int ar = 0;
  int rc = resolve_arith(arith, q, (int)h_log2(N), &ar);
  if(rc) return rc;
  rc = check_device(device);
  if(rc) return rc;
  USE_DEVICE(device);
  ntt_plan *p = new ntt_plan();
  p->device   = device;
  p->N        = N;
  p->q        = q;
  p->root     = root;
  p->m        = (int)h_log2(N);
  p->arith    = ar;
  /* NTT_ARITH_AUTO on a modulus the FP64 policies cannot serve: the throughput form of the integer arithmetic; an
   * explicit NTT_ARITH_U64 keeps the reference's butterflies and lazy words (NTT_OPT_INT_WIDE switches either way) */
  p->int_cls  = (arith == NTT_ARITH_AUTO && ar == NTT_ARITH_U64) ? int_wide_class(q) : -1;
  {
    hipDeviceProp_t prop;
    if(hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) {
      p->num_cus = prop.multiProcessorCount;
    }
  }
  const bool r4  = ar == NTT_ARITH_U64_R4;
  const bool gen = ts.gen_root != 0 && ts.gen_root_inv != 0;
  p->has_fwd     = gen || (r4 ? !(ts.efwd.empty() && ts.fwd.empty()) : !ts.fwd.empty());
  p->has_inv     = gen || (r4 ? !(ts.einv.empty() && ts.inv.empty()) : !ts.inv.empty());
  /* inverse power table slot 1 (w^-N/2) is all the constants need */
  std::vector<uint64_t> inv_for_consts(2, 1);
  if(gen) inv_for_consts[1] = h_powmod(ts.gen_root_inv, N / 2, q);
  else if(!ts.inv.empty()) inv_for_consts.assign(ts.inv.begin(), ts.inv.begin() + 2);
  else if(ts.einv.size() >= 4) inv_for_consts[1] = ts.einv[2]; /* e[2k] = w[k] */
  p->cu = h_consts_u64(q, N, inv_for_consts);
  if(ninv_override) {
    p->cu.ninv  = h_tw_u64(ninv_override % q, q);
    p->cu.wninv = h_tw_u64(h_mulmod(ninv_override % q, inv_for_consts[1], q), q);
  }
  if(ar == NTT_ARITH_F64) {
    p->cf = h_consts_f64(q, N, inv_for_consts);
    if(ninv_override) {
      p->cf.ninv  = h_tw_f64(ninv_override % q, q);
      p->cf.wninv = h_tw_f64(h_mulmod(ninv_override % q, inv_for_consts[1], q), q);
    }
    const int k = h_f64_ksh(q);
    p->kcls     = !h_f64_eligible(q) ? kWideClass : (k >= 18 ? 18 : (k >= 1 ? 1 : 0));
  }
  rc = NTT_OK;
  if(gen) {
    const uint64_t ninv = ninv_override ? ninv_override % q : h_powmod(N % q, q - 2, q);
    rc                  = device_build_direction(p, ts.gen_root, false, ninv);
    if(!rc) rc = device_build_direction(p, ts.gen_root_inv, true, ninv);
  } else if(r4) {
    /* expanded tables: the caller's, or derived from the power tables */
    if(p->has_fwd) {
      const std::vector<uint64_t> e = ts.efwd.empty() ? h_expand_radix4(ts.fwd, q) : ts.efwd;
      rc                            = upload_u64(&p->d_fwd, e, ts.efwd_con, q);
    }
    if(!rc && p->has_inv) {
      const std::vector<uint64_t> e = ts.einv.empty() ? h_expand_radix4(ts.inv, q) : ts.einv;
      rc                            = upload_u64(&p->d_inv, e, ts.einv_con, q);
    }
  } else {
    /* the full inverse table carries 16 extra records behind its N slots: N^-1 * winv[k], k < 16,
     * the twiddles of the last inverse group with the scaling folded in (run_group0_folded) */
    const std::vector<uint64_t> inv_ext =
      p->has_inv ? h_with_folded_ninv(ts.inv, ninv_override ? ninv_override % q : h_powmod(N % q, q - 2, q), q) : ts.inv;
    if(ar == NTT_ARITH_F64) {
      if(p->has_fwd) rc = upload_table<TwF64>(&p->d_fwd, ts.fwd, q, h_tw_f64);
      if(!rc && p->has_fwd) rc = upload_table<double>(&p->d_fwd8, ts.fwd, q, [](uint64_t w, uint64_t qq) { return h_tw_f64(w, qq).w; });
      if(!rc && p->has_inv) rc = upload_table<TwF64>(&p->d_inv, inv_ext, q, h_tw_f64);
      if(!rc && p->has_inv) rc = upload_table<double>(&p->d_inv8, ts.inv, q, [](uint64_t w, uint64_t qq) { return h_tw_f64(w, qq).w; });
    } else {
      if(p->has_fwd) rc = upload_u64(&p->d_fwd, ts.fwd, ts.fwd_con, q);
      if(!rc && p->has_inv) rc = upload_u64(&p->d_inv, inv_ext, ts.inv_con, q); /* caller precons cover the first N records */
    }
  }
  if(!rc) p->limbrec = limbrec_bytes(p);
  if(!rc && p->arith == NTT_ARITH_U64_R4) {
    LimbRec<ArithU64> r{};
    memcpy(&r, p->limbrec.data(), sizeof r);
    r.c.ninv = h_tw_u64(1, p->q);
    p->limbrec_mid.resize(sizeof r);
    memcpy(p->limbrec_mid.data(), &r, sizeof r);
  }
  if(rc) {
    ntt_plan_destroy(p);
    return rc;
  }
  *out = p;
  return NTT_OK;
}

extern "C" int ntt_plan_create(ntt_plan **out, int device, uint64_t N, uint64_t q, uint64_t root, int arith)
{
  if(!is_pow2(N) || q < 3 || root == 0 || root >= q) return fail(NTT_ERR_ARG, "bad N, q or root");
  if(h_powmod(root, N, q) != q - 1) return fail(NTT_ERR_ARG, "root is not a primitive 2N-th root of unity mod q");
  /* root^-1 and N^-1 come from Fermat's little theorem, which holds only for a prime q (a composite q can pass
   * 2N | q-1 and root^N == -1, and Carmichael-type composites even pass a Fermat test): deterministic Miller-Rabin
   * for 64-bit integers, then the two inverses are checked for what they are */
  if(!h_is_prime(q)) return fail(NTT_ERR_ARG, "q is not prime");
  const uint64_t rinv = h_powmod(root, q - 2, q);
  if(h_mulmod(root, rinv, q) != 1 || h_mulmod(N % q, h_powmod(N % q, q - 2, q), q) != 1) {
    return fail(NTT_ERR_ARG, "q is not prime (root^(q-2) is not the inverse of root)");
  }
  TableSet ts;
  ts.gen_root     = root;
  ts.gen_root_inv = rinv;
  return plan_build(out, device, N, q, root, ts, arith, 0);
}

extern "C" int ntt_plan_create_from_tables(ntt_plan **out, int device, uint64_t N, uint64_t q,
                                           const uint64_t *w_powers, const uint64_t *w_inv_powers, int arith)
{
  if(!w_powers && !w_inv_powers) return fail(NTT_ERR_ARG, "no table given");
  if(!is_pow2(N)) return fail(NTT_ERR_ARG, "N must be a power of two");
  if(N < 2 || q < 3) return fail(NTT_ERR_ARG, "bad N or q");
  /* cheap consistency checks of the caller's tables (reference layout, pre_compute.h:38-66): slot 0 is
   * root^0, slot 1 is root^(N/2) -- a square root of -1 -- and the two tables are inverses of each other */
  for(const uint64_t *t : {w_powers, w_inv_powers}) {
    if(!t) continue;
    if(t[0] != 1 || t[1] >= q || h_mulmod(t[1], t[1], q) != q - 1) {
      return fail(NTT_ERR_ARG, "table is not a bit-reversed power table of a primitive 2N-th root of unity mod q");
    }
  }
  if(w_powers && w_inv_powers) {
    const uint64_t last = N - 1; /* root^(bitrev(N-1)) = root^(N-1) */
    if(h_mulmod(w_powers[1], w_inv_powers[1], q) != 1 || h_mulmod(w_powers[last], w_inv_powers[last], q) != 1) {
      return fail(NTT_ERR_ARG, "w_inv_powers is not the inverse of w_powers");
    }
  }
  TableSet ts;
  if(w_powers) ts.fwd.assign(w_powers, w_powers + N);
  if(w_inv_powers) ts.inv.assign(w_inv_powers, w_inv_powers + N);
  return plan_build(out, device, N, q, 0, ts, arith, 0);
}

extern "C" void ntt_plan_destroy(ntt_plan *p)
{
  if(!p) return;
  DeviceGuard guard_(p->device);
  if(p->d_fwd) (void)hipFree(p->d_fwd);
  if(p->d_inv) (void)hipFree(p->d_inv);
  if(p->d_fwd8) (void)hipFree(p->d_fwd8);
  if(p->d_inv8) (void)hipFree(p->d_inv8);
  if(p->d_pos) (void)hipFree(p->d_pos);
  if(p->d_ipos) (void)hipFree(p->d_ipos);
  for(const ntt_plan::TeamBuf &tb : p->team_bufs) {
    if(tb.d) (void)hipFree(tb.d);
    if(tb.g) (void)hipFree(tb.g);
  }
  for(void *d : p->team_retired) (void)hipFree(d);
  for(const ntt_plan::PtrBuf &pb : p->ptr_bufs) {
    if(pb.d) (void)hipFree(pb.d);
    if(pb.h) (void)hipHostFree(pb.h);
    if(pb.copied) (void)hipEventDestroy(pb.copied);
  }
  for(const std::pair<void *, void *> &r : p->ptr_retired) {
    (void)hipFree(r.first);
    (void)hipHostFree(r.second);
  }
  if(p->own_stream) (void)hipStreamDestroy(p->own_stream);
  delete p;
}

extern "C" int ntt_plan_info(const ntt_plan *p, uint64_t info[8])
{
  if(!p || !info) return fail(NTT_ERR_ARG, "null argument");
  info[0] = p->N;
  info[1] = p->q;
  info[2] = (uint64_t)p->m;
  info[3] = (uint64_t)p->arith;
  info[4] = p->kcls == kWideClass ? 52u : (uint64_t)p->kcls; /* 52: the reduce-both-operands policy for q up to 2^52 */
  if(p->arith == NTT_ARITH_U64) info[4] = p->int_cls < 0 ? 0u : 100u + (uint64_t)p->int_cls; /* 100 + K: ArithU64X<K> */
  /* launches (= passes over the data) of one forward transform of a large batch: 1 where one launch carries both passes --
   * the XCD-local kernel (FP64 policies, N = 2^15..2^17, unless switched off: its automatic choice takes forward
   * transforms of 512 polynomials or more) or the two-phase kernel where it is forced -- else the pass list's length */
  {
    const bool f64big = !p->generic && p->arith == NTT_ARITH_F64;
    const bool team   = (f64big || (!p->generic && p->arith == NTT_ARITH_U64 && p->int_cls >= 0)) && p->m >= kTeamBlock + 3 &&
                      p->m <= kTeamBlock + 5 && p->xcd_local != 0;
    const bool tp     = f64big && p->m >= kFusedMax + 2 && p->m <= kFusedMax + 3 &&
                    (p->two_phase == 1 || (p->two_phase < 0 && p->m == kFusedMax + 2 && p->kcls != kWideClass));
    /* 2^15: one pass, the polynomial in registers -- for a batch that fills the chip, unless explicit options ask for two passes */
    const bool op     = f64big && p->m == kFusedMax + 1 && one_pass_pays(p, (uint64_t)p->num_cus);
    info[5] = (team || tp || op) ? 1u : (uint64_t)make_passes(p->m, p->generic).n;
  }
  info[6] = (uint64_t)p->device;
  info[7] = p->root;
  return NTT_OK;
}

extern "C" int ntt_plan_export_table(const ntt_plan *p, int which, void *h_dst, size_t bytes)
{
  if(!p || !h_dst) return fail(NTT_ERR_ARG, "null argument");
  if(which == 4 || which == 5) { /* the slot tables: N uint32_t each */
    const void *tab = which == 4 ? p->d_pos : p->d_ipos;
    if(!tab) return fail(NTT_ERR_ARG, "the plan has no such table");
    if(bytes > p->N * sizeof(uint32_t)) return fail(NTT_ERR_ARG, "table is smaller than the request");
    USE_DEVICE(p->device);
    HIP_TRY(hipMemcpy(h_dst, tab, bytes, hipMemcpyDeviceToHost));
    return NTT_OK;
  }
  const void *src = which == 0 ? p->d_fwd : which == 1 ? p->d_inv : which == 2 ? p->d_fwd8 : which == 3 ? p->d_inv8 : nullptr;
  if(!src) return fail(NTT_ERR_ARG, "the plan has no such table");
  const size_t rec  = p->arith == NTT_ARITH_F64 ? sizeof(TwF64) : sizeof(TwU64);
  const size_t have = which >= 2 ? p->N * sizeof(double)
                                 : (p->arith == NTT_ARITH_U64_R4 ? 2 * p->N : p->N + (which == 1 ? 16 : 0)) * rec;
  if(bytes > have) return fail(NTT_ERR_ARG, "table is smaller than the request");
  USE_DEVICE(p->device);
  HIP_TRY(hipMemcpy(h_dst, src, bytes, hipMemcpyDeviceToHost));
  return NTT_OK;
}

extern "C" int ntt_plan_set_generic(ntt_plan *p, int on)
{
  if(!p) return fail(NTT_ERR_ARG, "null plan");
  if(on && p->arith == NTT_ARITH_U64_R4) return fail(NTT_ERR_UNSUPPORTED, "the radix-4 policy has no column-pass form");
  p->generic = on != 0;
  return NTT_OK;
}

extern "C" int ntt_plan_set_option(ntt_plan *p, int option, int64_t value)
{
  if(!p) return fail(NTT_ERR_ARG, "null plan");
  switch(option) {
    case NTT_OPT_MAX_GRID:
      if(value < 0) return fail(NTT_ERR_ARG, "max grid must be >= 0");
      p->max_grid = (int)value;
      return NTT_OK;
    case NTT_OPT_RNS_LAUNCH:
      p->rns_launch = value < 0 ? -1 : (value != 0);
      return NTT_OK;
    case NTT_OPT_DOT_FUSED:
      p->dot_fused = value != 0;
      return NTT_OK;
    case NTT_OPT_RESCALE_FUSED:
      p->rescale_fused = value != 0;
      return NTT_OK;
    case NTT_OPT_MODUP_FUSED:
      p->modup_fused = value < 0 ? -1 : (value != 0);
      return NTT_OK;
    case NTT_OPT_PAIR_FUSED:
      p->pair_fused = value < 0 ? -1 : (value != 0);
      return NTT_OK;
    case NTT_OPT_MODDOWN_ADD_FUSED:
      p->moddown_add_fused = value < 0 ? -1 : (value != 0);
      return NTT_OK;
    case NTT_OPT_BGV_FUSED:
      p->bgv_fused = value < 0 ? -1 : (value != 0);
      return NTT_OK;
    case NTT_OPT_LIFT_FUSED:
      p->lift_fused = value < 0 ? -1 : (value != 0);
      return NTT_OK;
    case NTT_OPT_SLOTS_FUSED:
      p->slots_fused = value < 0 ? -1 : (value != 0);
      return NTT_OK;
    case NTT_OPT_SAMPLE_FUSED:
      p->sample_fused = value < 0 ? -1 : (value != 0);
      return NTT_OK;
    case NTT_OPT_MAX_BATCH_HINT:
      if(value < 0) return fail(NTT_ERR_ARG, "batch hint must be >= 0");
      {
        std::lock_guard<std::mutex> lock(p->team_mu); /* team_buffer reads it under this mutex */
        p->batch_hint = (uint64_t)value;
      }
      return value ? ntt_plan_reserve(p, nullptr, (uint64_t)value) : NTT_OK;
    case NTT_OPT_BLOCK_OVERSUB:
      if(value < 0 || value > 256) return fail(NTT_ERR_ARG, "workgroups per resident slot: 0 (default) .. 256");
      p->block_oversub = (int)value;
      return NTT_OK;
    case NTT_OPT_CHUNK_MIB:
      if(value < 1) return fail(NTT_ERR_ARG, "chunk must be >= 1 MiB");
      p->chunk_mib = (int)value;
      return NTT_OK;
    case NTT_OPT_TWO_PHASE:
      p->two_phase = value < 0 ? -1 : (value != 0);
      return NTT_OK;
    case NTT_OPT_ONE_PASS:
      p->one_pass = value < 0 ? -1 : (value != 0);
      return NTT_OK;
    case NTT_OPT_FUSED_PRODUCT:
      if(value < 0 || value > 2) return fail(NTT_ERR_ARG, "fused product: 0, 1 or 2");
      p->fused_product = (int)value;
      return NTT_OK;
    case NTT_OPT_XCD_LOCAL:
      p->xcd_local = value < 0 ? -1 : (value != 0);
      return NTT_OK;
    case NTT_OPT_XCD_LOCAL_LAG:
      if(value < 0 || value > 64) return fail(NTT_ERR_ARG, "lag must be 0 (default) .. 64 polynomials");
      p->team_lag = (int)value;
      return NTT_OK;
    case NTT_OPT_XCD_LOCAL_WGS_PER_CU:
      if(value < 0 || value > 4) return fail(NTT_ERR_ARG, "workgroups per CU: 0 (default) .. 4");
      p->team_wpc = (int)value;
      return NTT_OK;
    case NTT_OPT_BLOCK_LOG:
      if(value != 0 && value != kFusedSmallBlock && value != kFusedLarge) return fail(NTT_ERR_ARG, "block size must be 0 (automatic), 12 or 14");
      if(value == kFusedSmallBlock && p->m > kFusedSmallBlock + 4) return fail(NTT_ERR_ARG, "2^12-point blocks need at most 4 leading stages");
      p->block_log = (int)value;
      return NTT_OK;
    case NTT_OPT_F64_CLASS: {
      /* a coarser (smaller) headroom class than the modulus allows is always valid: it only reduces more often */
      if(p->arith != NTT_ARITH_F64 || p->kcls == kWideClass) return fail(NTT_ERR_ARG, "not a plan of the scheduled FP64 policy");
      const int k = h_f64_ksh(p->q);
      if(value == 0 || (value == 1 && k >= 1) || (value == 18 && k >= 18)) {
        p->kcls = (int)value;
        return NTT_OK;
      }
      return fail(NTT_ERR_ARG, "headroom class not instantiated or not valid for this modulus");
    }
    case NTT_OPT_INT_WIDE: {
      /* 0: the reference's butterflies; 1: the widest headroom class q permits; 10 + K: class K (tests: a narrower class
       * than q permits is always valid, it only folds more often) */
      if(p->arith != NTT_ARITH_U64) return fail(NTT_ERR_ARG, "not a plan of the integer policy");
      const int best = int_wide_class(p->q);
      if(value == 0) {
        p->int_cls = -1;
        return NTT_OK;
      }
      if(best < 0) return fail(NTT_ERR_UNSUPPORTED, "the wide integer policy serves 2^40 <= q < 2^61");
      if(value == 1) {
        p->int_cls = best;
        return NTT_OK;
      }
      if((value == 10 || value == 11 || value == 13) && value - 10 <= best) {
        p->int_cls = (int)value - 10;
        return NTT_OK;
      }
      return fail(NTT_ERR_ARG, "integer headroom class not instantiated or not valid for this modulus");
    }
    default: return fail(NTT_ERR_ARG, "unknown option");
  }
}

extern "C" int ntt_plan_get_option(const ntt_plan *p, int option, int64_t *value)
{
  if(!p || !value) return fail(NTT_ERR_ARG, "null argument");
  switch(option) {
    case NTT_OPT_MAX_GRID: *value = p->max_grid; return NTT_OK;
    case NTT_OPT_CHUNK_MIB: *value = p->chunk_mib; return NTT_OK;
    case NTT_OPT_F64_CLASS: *value = p->arith == NTT_ARITH_F64 ? p->kcls : -1; return NTT_OK;
    case NTT_OPT_TWO_PHASE: *value = p->two_phase; return NTT_OK;
    case NTT_OPT_ONE_PASS: *value = p->one_pass; return NTT_OK;
    case NTT_OPT_FUSED_PRODUCT: *value = p->fused_product; return NTT_OK;
    case NTT_OPT_BLOCK_LOG: *value = p->block_log; return NTT_OK;
    case NTT_OPT_XCD_LOCAL: *value = p->xcd_local; return NTT_OK;
    case NTT_OPT_XCD_LOCAL_LAG: *value = p->team_lag; return NTT_OK;
    case NTT_OPT_XCD_LOCAL_WGS_PER_CU: *value = p->team_wpc; return NTT_OK;
    case NTT_OPT_INT_WIDE: *value = p->arith == NTT_ARITH_U64 ? (p->int_cls < 0 ? 0 : 10 + p->int_cls) : -1; return NTT_OK;
    case NTT_OPT_BLOCK_OVERSUB: *value = p->block_oversub; return NTT_OK;
    case NTT_OPT_RNS_LAUNCH: *value = p->rns_launch; return NTT_OK;
    case NTT_OPT_DOT_FUSED: *value = p->dot_fused; return NTT_OK;
    case NTT_OPT_RESCALE_FUSED: *value = p->rescale_fused; return NTT_OK;
    case NTT_OPT_MODUP_FUSED: *value = p->modup_fused; return NTT_OK;
    case NTT_OPT_PAIR_FUSED: *value = p->pair_fused; return NTT_OK;
    case NTT_OPT_MODDOWN_ADD_FUSED: *value = p->moddown_add_fused; return NTT_OK;
    case NTT_OPT_BGV_FUSED: *value = p->bgv_fused; return NTT_OK;
    case NTT_OPT_LIFT_FUSED: *value = p->lift_fused; return NTT_OK;
    case NTT_OPT_SLOTS_FUSED: *value = p->slots_fused; return NTT_OK;
    case NTT_OPT_SAMPLE_FUSED: *value = p->sample_fused; return NTT_OK;
    case NTT_OPT_MAX_BATCH_HINT: *value = (int64_t)p->batch_hint; return NTT_OK;
    case NTT_OPT_CTL_ALLOCATIONS: {
      std::lock_guard<std::mutex> lock(p->team_mu);
      *value = (int64_t)p->ctl_allocs;
      return NTT_OK;
    }
    default: return fail(NTT_ERR_ARG, "unknown option");
  }
}
