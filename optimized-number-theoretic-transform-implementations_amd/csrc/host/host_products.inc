/* host/host_products.inc -- utility kernels, pointwise products, the coefficient-domain product launches, RNS limb sets and their layouts.
 * A section of ntt_host.hip (one translation unit, included from there in order); not compiled by itself. */

/* ------------------------------------------------------------------ */
/* utility kernels                                                     */
/* ------------------------------------------------------------------ */
__device__ __forceinline__ uint64_t splitmix64_dev(uint64_t x)
{
  x += 0x9e3779b97f4a7c15ULL;
  x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ULL;
  x = (x ^ (x >> 27)) * 0x94d049bb133111ebULL;
  return x ^ (x >> 31);
}

__global__ void __launch_bounds__(256) fill_uniform_kernel(uint64_t *a, uint64_t n, uint64_t q, uint64_t seed,
                                                           uint64_t offset)
{
  for(uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    a[i] = splitmix64_dev(seed ^ (offset + i)) % q;
  }
}

/* one workgroup per polynomial: sum_i splitmix64(i) * a[i] mod 2^64 */
__global__ void __launch_bounds__(256) checksum_kernel(uint64_t *out, const uint64_t *a, uint64_t N, uint64_t batch)
{
  __shared__ uint64_t part[256];
  for(uint64_t p = blockIdx.x; p < batch; p += gridDim.x) {
    const uint64_t *src = a + p * N;
    uint64_t        acc = 0;
    for(uint64_t i = threadIdx.x; i < N; i += blockDim.x) acc += splitmix64_dev(i) * src[i];
    part[threadIdx.x] = acc;
    __syncthreads();
    for(int s = 128; s > 0; s >>= 1) {
      if((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
      __syncthreads();
    }
    if(threadIdx.x == 0) out[p] = part[0];
    __syncthreads();
  }
}

/* Element i of a batch of polynomials of 2^logn words: polynomial i >> logn starts (i >> logn) * stride words into its operand
 * (ntt_core.h block_offset with whole polynomials as blocks).  pstride: a, c and every operand laid out like them; bstride: the b
 * operand -- 0 when it is ONE polynomial shared by the batch (a broadcast key). */
struct PwLayout {
  uint32_t logn;
  uint64_t pstride, bstride;
};
__device__ __forceinline__ uint64_t pw_index(uint64_t i, uint32_t logn, uint64_t stride)
{
  return (i >> logn) * stride + (i & ((1ull << logn) - 1ull));
}

/* LAZYIN: operands in [0,4q) as ntt_fwd_batch_lazy leaves them; the product is always fully reduced */
template <class A, bool LAZYIN>
__global__ void __launch_bounds__(256) pointwise_kernel(uint64_t *c, const uint64_t *a, const uint64_t *b, uint64_t n, const PwLayout lay,
                                                        const typename A::consts k)
{
  for(uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t j = pw_index(i, lay.logn, lay.pstride);
    c[j]             = LAZYIN ? A::mulmod_full_lazy4(a[j], b[j], k) : A::mulmod_full(a[j], b[j], k);
  }
}

/* c = (ACC ? c : 0) + a * b: the unfused form of the inner product in the NTT domain (plans the fused kernel is not built
 * for: column-pass-only plans, the radix-4 formulation, N < 2^6).  lay.bstride = 0 when b is ONE polynomial shared by the batch. */
template <class A, bool LAZYIN, bool ACC>
__global__ void __launch_bounds__(256) pointwise_acc_kernel(uint64_t *c, const uint64_t *a, const uint64_t *b, uint64_t n, const PwLayout lay,
                                                            uint64_t q, const typename A::consts k)
{
  for(uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t j = pw_index(i, lay.logn, lay.pstride), jb = pw_index(i, lay.logn, lay.bstride);
    const uint64_t t = LAZYIN ? A::mulmod_full_lazy4(a[j], b[jb], k) : A::mulmod_full(a[j], b[jb], k);
    if constexpr(ACC) {
      const uint64_t v = c[j] + t; /* both canonical: < 2q < 2^64 */
      c[j]             = v < q ? v : v - q;
    } else {
      c[j] = t;
    }
  }
}

static unsigned grid_for(uint64_t n, unsigned cap = 256 * 32)
{
  uint64_t g = (n + 255) / 256;
  if(g > cap) g = cap;
  /* a launch's threads per dimension must stay below 2^32 (hipErrorInvalidConfiguration otherwise: the 128 GiB slab of
   * `bench.py --scaling strong --gpus 1` asked the one-word-per-thread copy probe for exactly 2^32); the kernels that use this are
   * grid-stride loops, so a smaller grid only means a second iteration */
  if(g > (1u << 24) - 1u) g = (1u << 24) - 1u;
  if(g == 0) g = 1;
  return (unsigned)g;
}
/* The grid of the pointwise kernels (element-wise, memory-bound, grid-stride loop): about FOUR iterations per workgroup.  Workgroups
 * that loop over a slab in step produce their traffic in bursts: with the 8192 workgroups of rounds 1-4 (dozens of iterations
 * each) these kernels reached 0.66-0.68 of the roofline, with four iterations each 0.73-0.75 at 0.25, 1 and 4 GB per operand, and
 * one-shot workgroups (no loop, what the dispatcher staggers best for a plain copy: 6.3 TB/s, tools/copy_variants.hip) 0.65-0.70
 * (profiles/r05/pointwise_grid.txt).  max_grid: NTT_OPT_MAX_GRID (0 = this rule). */
static unsigned grid_pw(uint64_t n, int max_grid)
{
  const uint64_t total = (n + 255) / 256;
  if(max_grid > 0) return (unsigned)(total < (uint64_t)max_grid ? (total ? total : 1) : (uint64_t)max_grid);
  uint64_t g = (total + 3) / 4;
  if(g < 2048) g = total < 2048 ? total : 2048;
  if(g > (1u << 22)) g = 1u << 22;
  return (unsigned)(g ? g : 1);
}

/* The element-wise kernels are built for two policies -- FP64 plans multiply in FP64, every integer policy with the reference's
 * Barrett product -- and take their run-time flags as template arguments: with_bools(f, p->arith == NTT_ARITH_F64, flags...) hands f
 * the policy as its first constant (PwArith). */
template <bool F64> using PwArith = std::conditional_t<F64, ArithF64, ArithU64>;
template <class A> static const typename A::consts &pw_consts(const ntt_plan *p)
{
  if constexpr(std::is_same_v<A, ArithF64>) return p->cf;
  else return p->cu;
}

/* pstride: words between consecutive polynomials of all three operands (0 = dense: N) */
static int pointwise_launch(const ntt_plan *p, uint64_t *d_c, const uint64_t *d_a, const uint64_t *d_b, uint64_t batch,
                            void *stream, bool lazy_in, uint64_t pstride = 0)
{
  if(!p || !d_c || !d_a || !d_b) return fail(NTT_ERR_ARG, "null argument");
  if(batch == 0) return NTT_OK;
  USE_DEVICE(p->device);
  const uint64_t n = batch * p->N;
  const dim3     g(grid_pw(n, p->max_grid)), t(256);
  const PwLayout lay{(uint32_t)p->m, pstride ? pstride : p->N, pstride ? pstride : p->N};
  (void)with_bools(
    [&](auto f64, auto lazy) {
      using A = PwArith<decltype(f64)::value>;
      hipLaunchKernelGGL((pointwise_kernel<A, decltype(lazy)::value>), g, t, 0, (hipStream_t)stream, d_c, d_a, d_b, n, lay, pw_consts<A>(p));
      return hipSuccess;
    },
    p->arith == NTT_ARITH_F64, lazy_in);
  HIP_TRY(hipGetLastError());
  return NTT_OK;
}

/* c = (acc ? c : 0) + a (.) b, element by element over a slab of ls's (one) limb: the unfused form of the NTT-domain products.
 * bcast: b is ONE polynomial shared by the batch. */
static int pointwise_acc(const ntt_plan *p, uint64_t *d_c, const uint64_t *d_a, const uint64_t *d_b, uint64_t batch, const LimbSet &ls, bool lazy_in,
                         bool acc, bool bcast, void *stream)
{
  const uint64_t n = batch * p->N;
  const dim3     g(grid_pw(n, p->max_grid)), t(256);
  const PwLayout lay{(uint32_t)p->m, poly_words(p, ls), bcast ? 0 : poly_words(p, ls)};
  (void)with_bools(
    [&](auto f64, auto lazy, auto accumulate) {
      using A = PwArith<decltype(f64)::value>;
      hipLaunchKernelGGL((pointwise_acc_kernel<A, decltype(lazy)::value, decltype(accumulate)::value>), g, t, 0, (hipStream_t)stream, d_c, d_a, d_b, n, lay,
                         p->q, pw_consts<A>(p));
      return hipSuccess;
    },
    p->arith == NTT_ARITH_F64, lazy_in, acc);
  HIP_TRY(hipGetLastError());
  return NTT_OK;
}

extern "C" int ntt_pointwise_mul_batch(const ntt_plan *p, uint64_t *d_c, const uint64_t *d_a, const uint64_t *d_b,
                                       uint64_t batch, void *stream)
{
  return pointwise_launch(p, d_c, d_a, d_b, batch, stream, false);
}
extern "C" int ntt_pointwise_mul_batch_lazy(const ntt_plan *p, uint64_t *d_c, const uint64_t *d_a, const uint64_t *d_b,
                                            uint64_t batch, void *stream)
{
  return pointwise_launch(p, d_c, d_a, d_b, batch, stream, true);
}

/* a ProdArgs record over ls: c = inv(fwd(b) (.) a^), a^ in lazy words -- or, its `both` / `four` set, inv(fwd(b) (.) fwd(a)) */
static ProdArgs prod_args(const ntt_plan *p, const LimbSet &ls, uint64_t *out, const uint64_t *ahat, uint64_t *b, uint64_t batch, void *stream)
{
  ProdArgs pa{};
  launch_common(pa, p, ls, batch, stream);
  pa.b       = b;
  pa.ahat    = ahat;
  pa.out     = out;
  pa.a_lazy  = 1;
  pa.oversub = p->block_oversub;
  return pa;
}
/* (the product kernels are built for the FP64 policies; with a control block: the XCD-local one-launch form) */
static hipError_t dispatch_product(const ntt_plan *p, const ProdArgs &pa)
{
  return with_f64_class(eff_kcls(p), [&](auto k) {
    using K = decltype(k);
    return pa.team_ctl ? launch_team_product<typename K::A, K::KSH>(pa) : launch_product<typename K::A, K::KSH>(pa);
  });
}

/* c = a * b with the fused product kernels (FP64, N = 2^8 .. 2^17).
 *   N <= 2^14: ONE launch: a -> fwd, b -> fwd, product in registers, -> inv -> c.            24N bytes, 1 launch
 *              (NTT_OPT_FUSED_PRODUCT 2: a^ = fwd(a) (lazy words) by a launch of its own first: 40N bytes, 2 launches).
 *   N > 2^14 : a^ = fwd(a); per chunk: column stages on b, ONE launch over its 2^14- or 2^12-point blocks (fwd block * a^ block
 *              -> inverse block: the product is element-wise, so it fuses block by block), column stages of the
 *              inverse on c.                                                                   88N bytes, 5 launches
 *              (120N and 7 launches for fwd, fwd, pointwise, inv).
 *   N > 2^14, 2^23 coefficients per operand or more: everything, both forward transforms included, as the items of
 *              ONE launch (team_product_kernel<..., FOUR>): a^ never exists in memory.        48N bytes, 1 launch. */
/* ahat_given: d_a already holds a^ = fwd(a) (canonical or lazy words below 2^53): c = inv(fwd(b) (.) a^), the three-pass
 * forms of the kernels (ntt_mul_transformed_batch) */
static int fused_product(const ntt_plan *p, uint64_t *d_c, uint64_t *d_a, uint64_t *d_b, uint64_t batch, void *stream,
                         const LimbSet *set = nullptr, bool ahat_given = false)
{
  const LimbSet ls = set ? *set : LimbSet{p->limbrec.data(), 1, 0, 0};
  /* a^ = fwd(a).  The product kernels take a^ as lazy words v + 2q, v in (-2q, 2q); a canonical word c is the lazy word of
   * v = c - 2q, so the reduced forward transform is a valid producer too -- used where it is the faster launch (the
   * XCD-local kernel, N >= 2^15, large batches: +13..20 % over the per-pass lazy transform) */
  const bool canonical_a = team_applies(p, batch, false, false, false, ls.n, true);
  /* N >= 2^15, large batches: the chain as the item kinds of ONE launch (ntt_kernels.h: team_product_kernel) -- column
   * stages of b AND a, block products (both blocks through their twelve stages, product, inverse stages), inverse column
   * stages of c: a^ never exists in memory (48N instead of 64N bytes across the fabric).  NTT_OPT_FUSED_PRODUCT 2 keeps a's
   * forward transform as a launch of its own in front of the three-pass form (measurements, tests). */
  void *ctl  = nullptr;
  int   rc   = NTT_OK;
  if(canonical_a && !p->block_log) {
    rc = team_buffer(p, stream, 2 * batch * (uint64_t)ls.n, &ctl);
    if(rc) return rc;
  }
  const bool four = !ahat_given && ctl && p->fused_product != 2;
  /* N <= 2^14: a's coefficients go straight into the fused kernel, which takes both operands through the forward
   * stages (24N instead of 40N bytes, one launch; a is left as it was) */
  /* N > 2^14 below the one-launch form's batch: the same inside the block launch of every chunk -- a gets b's column
   * passes and the blocks of both operands meet in registers (72N instead of 88N bytes, 6 launches per chunk, no
   * transform of a in front) */
  const bool both = !ahat_given && !four && p->fused_product != 2;
  if(!four && !both && !ahat_given) {
    rc = run_transform(p, d_a, batch, false, false, stream, !canonical_a, &ls);
    if(rc) return rc;
  }
  USE_DEVICE(p->device);
  if(ctl) {
    ProdArgs pa = prod_args(p, ls, d_c, d_a, d_b, batch, stream);
    pa.four     = four;
    /* three passes, four workgroups per CU: the lag that keeps second- and third-pass items from waiting is larger than
     * the transform's (measured, profiles/r03/sweep_product_lag.txt: flat optimum 12-14 at 2^17, 12-20 at 2^16, 20-24 at 2^15;
     * with both operands' column tiles in the first pass: 8 at 2^17, 12-16 at 2^16, 20-24 at 2^15) */
    set_team(pa, p, ctl, p->m == kTeamBlock + 3 ? 20 : (p->m == kTeamBlock + 4 ? 14 : (four ? 8 : 12)));
    return launched(dispatch_product(p, pa));
  }
  /* blocks of the fused launch for N > 2^14: as for the transforms, stages are cheaper in the memory-bound column
   * passes than in the FP64-bound fused launch -- 2^12-point blocks where 4 column stages reach (measured +3..5 % at
   * 2^15 and 2^16; 2^13-point blocks at 2^17: -1 %, not used) */
  const int      pblk   = p->m > kFusedMax ? (p->block_log ? p->block_log : (p->m <= kFusedSmallBlock + 4 ? kFusedSmallBlock : kFusedLarge)) : p->m;
  const PassList L     = make_passes(p->m, false, pblk);
  return for_chunks(p, ls, batch, (uint64_t)p->chunk_mib, L.n, [&](uint64_t, uint64_t nb, uint64_t off) -> int {
    for(int k = 0; k + 1 < L.n; k++) { /* forward column passes of b (every pass but the last, which is the block pass) */
      rc = launch_one_pass(p, L.p[k], d_b + off, nb, false, false, false, false, stream, ls);
      if(!rc && both) rc = launch_one_pass(p, L.p[k], d_a + off, nb, false, false, false, false, stream, ls); /* ... and of a */
      if(rc) return rc;
    }
    ProdArgs pa  = prod_args(p, ls, d_c + off, d_a + off, d_b + off, nb, stream);
    pa.block_log = (uint32_t)pblk;
    pa.both      = both;
    rc           = launched(dispatch_product(p, pa));
    for(int k = L.n - 2; !rc && k >= 0; k--) { /* inverse column passes of c, the last one ends the transform (N^-1) */
      rc = launch_one_pass(p, L.p[k], d_c + off, nb, true, false, false, k == 0, stream, ls);
    }
    return rc;
  });
}

static bool fused_product_applies(const ntt_plan *p, const uint64_t *d_c, const uint64_t *d_a, const uint64_t *d_b, uint64_t batch)
{
  return p && p->fused_product && p->arith == NTT_ARITH_F64 && p->m >= 8 && p->m <= kFusedMax + 3 && !p->generic && p->has_fwd &&
         p->has_inv && d_a != d_b && d_a && d_b && d_c && batch;
}

static bool dot_kernel_applies(const ntt_plan *p);
static int  inv_dot(const ntt_plan *p, uint64_t *d_c, int k, const uint64_t *const *a, const uint64_t *const *b, uint64_t batch,
                    unsigned flags, void *stream, const LimbSet *set, uint64_t b_limb_stride);

/* pstride: words between consecutive polynomials of all three operands (0 = dense) */
static int negacyclic_mul_one(const ntt_plan *p, uint64_t *d_c, uint64_t *d_a, uint64_t *d_b, uint64_t batch, void *stream, uint64_t pstride)
{
  /* the chain never leaves the lazy domain (SURVEY f4): both forward transforms skip their final reduction,
   * the pointwise product takes [0,4q) operands, only the inverse's output is reduced.
   * d_a == d_b is a squaring: the operand is transformed once (transforming the shared buffer twice
   * would multiply fwd(fwd(a)) with itself) */
  if(!p) return fail(NTT_ERR_ARG, "null argument");
  const LimbSet own{p->limbrec.data(), 1, 0, pstride};
  if(p->arith == NTT_ARITH_U64_R4) {
    /* the reference's radix-4 formulation end to end: fwd_ntt_radix4 on both operands (canonical outputs), the pointwise
     * product, inv_ntt_radix4 */
    int rc4 = run_transform(p, d_a, batch, false, false, stream, false, &own);
    if(!rc4 && d_b != d_a) rc4 = run_transform(p, d_b, batch, false, false, stream, false, &own);
    if(!rc4) rc4 = pointwise_launch(p, d_c, d_a, d_b, batch, stream, false, pstride);
    if(!rc4) rc4 = run_transform(p, d_c, batch, true, false, stream, false, &own);
    return rc4;
  }
  if(fused_product_applies(p, d_c, d_a, d_b, batch)) return fused_product(p, d_c, d_a, d_b, batch, stream, &own);
  int rc = run_transform(p, d_a, batch, false, false, stream, true, &own);
  if(!rc && d_b != d_a) rc = run_transform(p, d_b, batch, false, false, stream, true, &own);
  if(!rc && dot_kernel_applies(p) && p->has_inv && d_c) {
    /* the products inside the inverse transform's first pass (dot_inv_kernel): 24N bytes instead of 40N for the last two
     * steps -- the integer policies (no one-launch product kernel), squarings, plans with the fused product switched off */
    const uint64_t *pa = d_a, *pb = d_b;
    return inv_dot(p, d_c, 1, &pa, &pb, batch, NTT_MUL_LAZY_IN, stream, &own, 0);
  }
  if(!rc) rc = pointwise_launch(p, d_c, d_a, d_b, batch, stream, true, pstride);
  if(!rc) rc = run_transform(p, d_c, batch, true, false, stream, false, &own);
  return rc;
}

extern "C" int ntt_negacyclic_mul_batch(const ntt_plan *p, uint64_t *d_c, uint64_t *d_a, uint64_t *d_b,
                                        uint64_t batch, void *stream)
{
  return negacyclic_mul_one(p, d_c, d_a, d_b, batch, stream, 0);
}

static int rns_check(int nlimbs, ntt_plan *const *plans)
{
  if(nlimbs <= 0 || !plans) return fail(NTT_ERR_ARG, "bad limb list");
  for(int l = 0; l < nlimbs; l++) {
    if(!plans[l] || plans[l]->N != plans[0]->N || plans[l]->device != plans[0]->device) {
      return fail(NTT_ERR_ARG, "RNS limbs must share N and device");
    }
  }
  return NTT_OK;
}

/* One launch chain for all limbs (VERDICT r02 item 4, SURVEY 8e "split primes"): possible when the limbs' plans agree in
 * everything a launch is shaped by -- size, device, arithmetic policy and headroom class (one kernel instantiation serves
 * every limb), and the plan options.  Primes of the same bit size always do.  Otherwise the limbs are looped. */
/* plans whose kernels have MULTI variants (several limbs per launch): the FP64 policies and the wide integer policy */
static bool multi_limb_plan(const ntt_plan *p)
{
  return p->arith == NTT_ARITH_F64 || (p->arith == NTT_ARITH_U64 && p->int_cls >= 0 && !p->generic);
}

static std::vector<unsigned char> rns_records(ntt_plan *const *plans, int first, int n);
static bool rns_compatible(const ntt_plan *a, const ntt_plan *b)
{
  /* (the headroom class may differ inside a policy: the run takes the coarsest one -- but the reduce-as-scheduled FP64 policy
   * for 52-bit moduli and the reference's integer butterflies are policies of their own) */
  return multi_limb_plan(a) && b->arith == a->arith && (b->kcls == kWideClass) == (a->kcls == kWideClass) &&
         (b->int_cls >= 0) == (a->int_cls >= 0) && b->m == a->m &&
         b->generic == a->generic && b->block_log == a->block_log && b->chunk_mib == a->chunk_mib && b->two_phase == a->two_phase &&
         b->fused_product == a->fused_product && b->max_grid == a->max_grid && b->block_oversub == a->block_oversub && b->rns_launch == a->rns_launch && b->dot_fused == a->dot_fused && b->has_fwd == a->has_fwd && b->has_inv == a->has_inv &&
         b->xcd_local == a->xcd_local && b->team_lag == a->team_lag && b->team_wpc == a->team_wpc && b->one_pass == a->one_pass;
}

/* Where the limbs and polynomials of an RNS operand live (words): polynomial p of limb l starts l * limb + p * poly words in.
 * [limb][batch][N] (the layout of the plain ntt_rns_* entry points): {batch * N, N}; SURVEY 8(d)'s [batch][prime][N] -- what an
 * FHE library holds: a ciphertext polynomial = its limbs side by side --: {N, limbs * N}.  Padded forms of either are fine. */
struct Layout {
  uint64_t limb, poly;
  const uint64_t *ptab = nullptr; /* pointer batch: device table of the polynomials' limb-0 addresses (poly = typical spacing, a hint) */
};
/* the strides must keep the (limb, polynomial) ranges apart: limb-major (a limb's polynomials inside its slab) or
 * polynomial-major (a polynomial's limbs inside its record) */
static int layout_check(uint64_t N, int nlimbs, uint64_t batch, const Layout &lay)
{
  if(lay.poly < N || lay.limb < N) return fail(NTT_ERR_ARG, "layout: strides must be at least N words");
  if(lay.poly > (1ull << 40) || lay.limb > (1ull << 40)) return fail(NTT_ERR_ARG, "layout: stride too large");
  /* (128-bit: strides go up to 2^40 words and the batch is the caller's number -- (batch - 1) * stride must not wrap) */
  const bool limb_major = batch <= 1 || (unsigned __int128)lay.limb >= (unsigned __int128)(batch - 1) * lay.poly + N;
  const bool poly_major = nlimbs <= 1 || (unsigned __int128)lay.poly >= (unsigned __int128)(nlimbs - 1) * lay.limb + N;
  if(!limb_major && !poly_major) return fail(NTT_ERR_ARG, "layout: limbs and polynomials overlap");
  return NTT_OK;
}

/* The limb list as maximal RUNS of consecutive compatible limbs, at most kMaxLimbs each (the records one launch carries): a
 * modulus chain with one prime of another size -- a 60-bit first prime in front of 50-bit ones -- is served as that limb by
 * itself plus one launch per pass for the others, not limb by limb altogether.  {first, count}. */
static std::vector<std::pair<int, int>> rns_runs(int nlimbs, ntt_plan *const *plans)
{
  std::vector<std::pair<int, int>> runs;
  for(int i = 0; i < nlimbs;) {
    int j = i + 1;
    while(j < nlimbs && j - i < kMaxLimbs && rns_compatible(plans[i], plans[j])) j++;
    runs.emplace_back(i, j - i);
    i = j;
  }
  return runs;
}

/* calls set_fn(first, LimbSet) for every run that `pays(plan of the run's first limb, run length)` says one launch should
 * serve, one_fn(limb) for every other limb; stops at the first error */
template <class Pays, class SetFn, class OneFn>
static int rns_for_runs(int nlimbs, ntt_plan *const *plans, const Layout &lay, Pays pays, SetFn set_fn, OneFn one_fn)
{
  int rc = NTT_OK;
  for(const std::pair<int, int> &run : rns_runs(nlimbs, plans)) {
    const int first = run.first, n = run.second;
    if(n > 1 && pays(plans[first], n)) {
      const std::vector<unsigned char> recs = rns_records(plans, first, n);
      const LimbSet                    ls{recs.data(), n, lay.limb, lay.poly, lay.ptab};
      int kc = plans[first]->kcls, ic = plans[first]->int_cls;
      for(int l = first + 1; l < first + n; l++) {
        kc = plans[l]->kcls < kc ? plans[l]->kcls : kc;
        ic = plans[l]->int_cls < ic ? plans[l]->int_cls : ic;
      }
      t_run_kcls    = kc;
      t_run_int_cls = ic;
      rc            = set_fn(first, ls);
      t_run_kcls = t_run_int_cls = INT_MIN;
    } else {
      for(int l = first; !rc && l < first + n; l++) rc = one_fn(l);
    }
    if(rc) break;
  }
  return rc;
}

/* The slab drivers of the RNS products, from their arguments to their runs: the limb list, an empty batch (nothing to do), the
 * driver's own operand checks -- operands(), before any limb offset is added --, the layout; then rns_for_runs. */
static int all_given(bool operands) { return operands ? NTT_OK : fail(NTT_ERR_ARG, "null argument"); }
template <class Operands, class Pays, class SetFn, class OneFn>
static int rns_slab_runs(int nlimbs, ntt_plan *const *plans, uint64_t batch, const Layout &lay, Operands operands, Pays pays, SetFn set_fn, OneFn one_fn)
{
  int rc = rns_check(nlimbs, plans);
  if(rc || batch == 0) return rc;
  rc = operands();
  if(!rc) rc = layout_check(plans[0]->N, nlimbs, batch, lay);
  if(rc) return rc;
  return rns_for_runs(nlimbs, plans, lay, pays, set_fn, one_fn);
}
/* the words between the limbs of a b operand: a broadcast one is [limb][N] */
static uint64_t b_slab(ntt_plan *const *plans, const Layout &lay, unsigned flags) { return (flags & NTT_MUL_B_BROADCAST) ? plans[0]->N : lay.limb; }

/* One launch for all limbs pays when a single limb's share cannot fill the chip by itself (a ciphertext: a few
 * polynomials x tens of primes); with thousands of polynomials per limb every per-limb launch fills it, and the
 * single-set kernels are the faster ones (no run-time limb index: ntt_kernels.h, MULTI).  NTT_OPT_RNS_LAUNCH 0 / 1 on the
 * run's first plan forces the one-launch / the per-limb form (tests, measurements). */
static bool rns_one_launch_pays(const ntt_plan *p, uint64_t batch)
{
  if(p->rns_launch >= 0) return p->rns_launch == 0;
  const uint64_t wg_equivalents = (batch * p->N) >> 12; /* 256-thread workgroups' worth of coefficients per limb */
  return wg_equivalents < 8ull * (uint64_t)p->num_cus;
}

/* Large per-limb batches at N = 2^15..2^17: the XCD-local launches (team_kernel, team_product_kernel) take the limb as part
 * of the queue entry, so a whole RNS set is ONE launch there too -- no launch tails between the limbs (measured 3.5 % of a
 * config-5 step, profiles/r03/ablations.txt (f)).  NTT_OPT_RNS_LAUNCH 1 keeps the per-limb launches. */
static bool rns_team_launch(const ntt_plan *p, int nlimbs, uint64_t batch, bool inverse, bool product)
{
  if(p->rns_launch == 1) return false;
  return team_applies(p, batch, inverse, false, false, nlimbs < kMaxLimbs ? nlimbs : kMaxLimbs, product) &&
         team_applies(p, batch, inverse, false, false, 1, product); /* (a limb's own share qualifies: same lag tuning) */
}

/* the records of limbs [first, first + n) as one host array */
static std::vector<unsigned char> rns_records(ntt_plan *const *plans, int first, int n)
{
  std::vector<unsigned char> all;
  for(int l = first; l < first + n; l++) all.insert(all.end(), plans[l]->limbrec.begin(), plans[l]->limbrec.end());
  return all;
}

/* the coarsest headroom class of the run [first, first + n) (rns_for_runs); a run of 52-bit primes is all of the wide policy
 * (rns_compatible) */
static int run_class(ntt_plan *const *plans, int first, int n)
{
  int kc = plans[first]->kcls;
  for(int l = first + 1; l < first + n; l++) kc = plans[l]->kcls < kc ? plans[l]->kcls : kc;
  return kc;
}

/* the plan's own record as a one-limb set whose polynomials are lay.poly words apart */
static LimbSet own_set(const ntt_plan *p, const Layout &lay) { return LimbSet{p->limbrec.data(), 1, 0, lay.poly, lay.ptab}; }

static int rns_transform(int nlimbs, ntt_plan *const *plans, uint64_t *d_a, uint64_t batch, bool inverse, void *stream, const Layout &lay)
{
  int rc = rns_check(nlimbs, plans);
  if(rc || batch == 0) return rc;
  if(!d_a && !lay.ptab) return fail(NTT_ERR_ARG, "null argument");
  /* (a pointer batch: the images were checked one by one where the pointers were visible -- ptr_runs) */
  rc = lay.ptab ? NTT_OK : layout_check(plans[0]->N, nlimbs, batch, lay);
  if(rc) return rc;
  return rns_for_runs(
    nlimbs, plans, lay,
    [&](const ntt_plan *p, int n) { return rns_one_launch_pays(p, batch) || rns_team_launch(p, n, batch, inverse, false); },
    [&](int first, const LimbSet &ls) { return run_transform(plans[first], advance(d_a, (uint64_t)first * lay.limb), batch, inverse, false, stream, false, &ls); },
    [&](int l) {
      const LimbSet own = own_set(plans[l], lay);
      return run_transform(plans[l], advance(d_a, (uint64_t)l * lay.limb), batch, inverse, false, stream, false, &own);
    });
}

/* [limb][batch][N]: what the plain ntt_rns_* entry points take */
static Layout limb_major(ntt_plan *const *plans, int nlimbs, uint64_t batch)
{
  const uint64_t N = (nlimbs > 0 && plans && plans[0]) ? plans[0]->N : 0;
  return Layout{batch * N, N};
}

extern "C" int ntt_rns_fwd_batch(int nlimbs, ntt_plan *const *plans, uint64_t *d_a, uint64_t batch, void *stream)
{
  return rns_transform(nlimbs, plans, d_a, batch, false, stream, limb_major(plans, nlimbs, batch));
}

extern "C" int ntt_rns_inv_batch(int nlimbs, ntt_plan *const *plans, uint64_t *d_a, uint64_t batch, void *stream)
{
  return rns_transform(nlimbs, plans, d_a, batch, true, stream, limb_major(plans, nlimbs, batch));
}

extern "C" int ntt_rns_fwd_batch_strided(int nlimbs, ntt_plan *const *plans, uint64_t *d_a, uint64_t limb_stride, uint64_t poly_stride,
                                         uint64_t batch, void *stream)
{
  return rns_transform(nlimbs, plans, d_a, batch, false, stream, Layout{limb_stride, poly_stride});
}

extern "C" int ntt_rns_inv_batch_strided(int nlimbs, ntt_plan *const *plans, uint64_t *d_a, uint64_t limb_stride, uint64_t poly_stride,
                                         uint64_t batch, void *stream)
{
  return rns_transform(nlimbs, plans, d_a, batch, true, stream, Layout{limb_stride, poly_stride});
}

static int rns_negacyclic_mul(int nlimbs, ntt_plan *const *plans, uint64_t *d_c, uint64_t *d_a, uint64_t *d_b, uint64_t batch, void *stream,
                              const Layout &lay)
{
  /* a run of the wide integer policy: both forward transforms (lazy words, in place -- the operands are scratch on this path as
   * they are for a single plan) and the products inside the inverse transform's first pass, each ONE launch over the run */
  auto int_run = [&](const ntt_plan *p) {
    return p->arith == NTT_ARITH_U64 && dot_kernel_applies(p) && p->has_fwd && p->has_inv;
  };
  return rns_slab_runs(
    nlimbs, plans, batch, lay, [&] { return all_given(d_c && d_a && d_b); },
    [&](const ntt_plan *p, int n) {
      if(fused_product_applies(p, d_c, d_a, d_b, batch)) {
        return rns_one_launch_pays(p, batch) || (rns_team_launch(p, n, batch, false, true) && !p->block_log);
      }
      return int_run(p) && rns_one_launch_pays(p, batch);
    },
    [&](int first, const LimbSet &ls) {
      const ntt_plan *p   = plans[first];
      const uint64_t  off = (uint64_t)first * lay.limb;
      if(fused_product_applies(p, d_c, d_a, d_b, batch)) return fused_product(p, d_c + off, d_a + off, d_b + off, batch, stream, &ls);
      int r = run_transform(p, d_a + off, batch, false, false, stream, true, &ls);
      if(!r && d_b != d_a) r = run_transform(p, d_b + off, batch, false, false, stream, true, &ls);
      const uint64_t *pa = d_a + off, *pb = d_b + off;
      if(!r) r = inv_dot(p, d_c + off, 1, &pa, &pb, batch, NTT_MUL_LAZY_IN, stream, &ls, ls.stride);
      return r;
    },
    [&](int l) {
      const uint64_t off = (uint64_t)l * lay.limb;
      return negacyclic_mul_one(plans[l], d_c + off, d_a + off, d_b + off, batch, stream, lay.poly);
    });
}

extern "C" int ntt_rns_negacyclic_mul_batch(int nlimbs, ntt_plan *const *plans, uint64_t *d_c, uint64_t *d_a,
                                            uint64_t *d_b, uint64_t batch, void *stream)
{
  return rns_negacyclic_mul(nlimbs, plans, d_c, d_a, d_b, batch, stream, limb_major(plans, nlimbs, batch));
}

extern "C" int ntt_rns_negacyclic_mul_batch_strided(int nlimbs, ntt_plan *const *plans, uint64_t *d_c, uint64_t *d_a, uint64_t *d_b,
                                                    uint64_t limb_stride, uint64_t poly_stride, uint64_t batch, void *stream)
{
  return rns_negacyclic_mul(nlimbs, plans, d_c, d_a, d_b, batch, stream, Layout{limb_stride, poly_stride});
}
