/* host/host_plain.inc -- out of the RNS, the last step of a decryption: ntt_rns_to_plain_batch, ntt_rns_to_double_batch and their strided
 * forms.  A section of ntt_host.hip (one translation unit, included from there in order); not compiled by itself.  The kernels are in
 * plain.hip; this section sees their launchers and argument records only (ntt_plain.h, which states the arithmetic and its band).
 *
 *   to_plain    m = [x_c]_t (BGV), or round(t x / Q) mod t with NTT_PLAIN_SCALE (BFV): plain_kernel, ONE launch, 8N(L + 1) bytes per
 *               polynomial; integer and FP64 arithmetic of its own for every policy and every N >= 2.
 *   to_double   y = fl(x_c) * scale for one or two limbs (CKKS): plain_double_kernel, ONE launch.
 * Everything is checked before the launch.  Nothing is allocated, the host is not synchronised and no memset is issued: the calls can
 * be captured into a graph. */

/* The plaintext modulus as bconv_reduce's divisor: t, floor(2^128 / t) in two words and h.  bconv_reduce's comment proves its result
 * for odd q; what the proof uses is the estimate x/t - 2 < floor(x mu / 2^128) <= x/t, which holds for every mu with
 * 2^128/t - 1 < mu <= 2^128/t and every x < 2^128, and that 2t fits a word.  Oddness served only to make floor((2^128 - 1) / q) that
 * mu.  Here t may divide 2^128: mu is formed as floor(2^128 / t) itself, which fits two words because t >= 2 (2^127 at most), and
 * 2t < 2^62.  (bar, the 64-bit Barrett word, is not used by to_plain.) */
static BconvDst plain_dst(uint64_t t, uint64_t h)
{
  BconvDst                d{};
  const unsigned __int128 all = ~(unsigned __int128)0;
  const unsigned __int128 mu  = all / t + (all % t == t - 1 ? 1u : 0u);
  d.q                         = t;
  d.mu_lo                     = (uint64_t)mu;
  d.mu_hi                     = (uint64_t)(mu >> 64);
  d.h                         = h;
  return d;
}

/* a^-1 mod t for gcd(a, t) = 1, t >= 2 any integer (extended Euclid; the coefficients stay below t in magnitude); 0 if no inverse */
static uint64_t plain_invmod(uint64_t a, uint64_t t)
{
  __int128 r0 = t, r1 = a % t, s0 = 0, s1 = 1;
  while(r1) {
    const __int128 q = r0 / r1, r2 = r0 - q * r1, s2 = s0 - q * s1;
    r0 = r1, r1 = r2, s0 = s1, s1 = s2;
  }
  if(r0 != 1) return 0;
  return (uint64_t)(s0 < 0 ? s0 + (__int128)t : s0);
}

/* what both calls check first: the limb list, its size and primes, the source layout and the output's stride */
static int plain_check(int nlimbs, int max_limbs, ntt_plan *const *plans, const void *d_out, const void *d_a, uint64_t batch, const Layout &lay,
                       uint64_t out_poly_stride)
{
  if(nlimbs < 1 || nlimbs > max_limbs) return fail(NTT_ERR_ARG, max_limbs == 2 ? "to_double: 1 or 2 limbs" : "to_plain: 1 .. 16 limbs");
  int rc = rns_check(nlimbs, plans);
  if(rc) return rc;
  if(plans[0]->m < 1 || plans[0]->m > 30) return fail(NTT_ERR_ARG, "to_plain: N out of range");
  for(int l = 0; l < nlimbs; l++)
    if(plans[l]->q >= (1ull << 61)) return fail(NTT_ERR_ARG, "to_plain: every prime must be below 2^61");
  rc = distinct_primes(nlimbs, plans);
  if(rc) return rc;
  if(batch > 0 && (!d_out || !d_a)) return fail(NTT_ERR_ARG, "null argument");
  const uint64_t N = plans[0]->N;
  rc               = layout_check(N, nlimbs, batch, lay);
  if(rc) return rc;
  if(out_poly_stride < N || out_poly_stride > (1ull << 40)) return fail(NTT_ERR_ARG, "layout: the output's polynomial stride must be N .. 2^40 words");
  if(batch == 0) return NTT_OK;
  /* the output may BE limb 0 of the source (every lane reads all its words before its one store); any other overlap is refused */
  const bool same = d_out == d_a && out_poly_stride == lay.poly;
  if(!same && galois_overlap(galois_span((const uint64_t *)d_out, N, 1, batch, 0, out_poly_stride),
                             galois_span((const uint64_t *)d_a, N, nlimbs, batch, lay.limb, lay.poly)))
    return fail(NTT_ERR_ARG, "to_plain: the output overlaps the source without being its limb 0");
  return NTT_OK;
}

static int rns_to_plain(int nlimbs, ntt_plan *const *plans, uint64_t *d_m, const uint64_t *d_a, uint64_t t, uint64_t batch, unsigned flags,
                        void *stream, const Layout &lay, uint64_t m_poly_stride)
{
  if(flags & ~(unsigned)NTT_PLAIN_SCALE) return fail(NTT_ERR_ARG, "unknown flag");
  if(t < 2 || t >= (1ull << 61)) return fail(NTT_ERR_ARG, "to_plain: the plaintext modulus must satisfy 2 <= t < 2^61");
  int rc = plain_check(nlimbs, kPlainLimbs, plans, d_m, d_a, batch, lay, m_poly_stride);
  if(rc) return rc;
  const bool scale = (flags & NTT_PLAIN_SCALE) != 0;
  PlainArgs  pa{};
  uint64_t   b[kPlainLimbs];
  for(int i = 0; i < nlimbs; i++) b[i] = plans[i]->q;
  BconvSrc src[kPlainLimbs];
  uint64_t g[kPlainLimbs];
  double   rho[kPlainLimbs];
  bconv_sources(b, nlimbs, false, src); /* [q^_i^-1]_{q_i} */
  exact_rhos(b, nlimbs, rho);
  uint64_t h = 1;
  if(scale) {
    /* c_i = [t q^_i^-1]_{q_i}, g_i = [-q_i^-1]_t (in [1, t): the inverse is not 0), h = 1 */
    for(int i = 0; i < nlimbs; i++) {
      const uint64_t inv = plain_invmod(b[i], t);
      if(!inv) return fail(NTT_ERR_ARG, "to_plain: NTT_PLAIN_SCALE needs every prime coprime to t");
      src[i].inv = h_mulmod(src[i].inv, t % b[i], b[i]);
      g[i]       = t - inv;
    }
  } else {
    /* c_i = [q^_i^-1]_{q_i}, g_i = [q^_i]_t, h = [-Q]_t */
    const uint64_t qt = bconv_hats(b, nlimbs, t, g);
    h                 = qt ? t - qt : 0;
  }
  for(int i = 0; i < nlimbs; i++) pa.k.l[i] = PlainLimb{b[i], src[i].inv, shoup_of(src[i].inv, b[i]), g[i], rho[i]};
  pa.k.d = plain_dst(t, h);
  if(batch == 0) return NTT_OK;
  USE_DEVICE(plans[0]->device);
  pa.m             = d_m;
  pa.a             = d_a;
  pa.a_limb_stride = lay.limb;
  pa.a_poly_stride = lay.poly;
  pa.m_poly_stride = m_poly_stride;
  pa.batch         = batch;
  pa.logn          = (uint32_t)plans[0]->m;
  pa.nlimbs        = nlimbs;
  pa.max_grid      = plans[0]->max_grid;
  pa.stream        = (hipStream_t)stream;
  const hipError_t e = launch_plain(pa);
  if(e != hipSuccess) return fail(NTT_ERR_HIP, std::string("plain_kernel: ") + hipGetErrorString(e));
  return NTT_OK;
}

static int rns_to_double(int nlimbs, ntt_plan *const *plans, double *d_y, const uint64_t *d_a, double scale, uint64_t batch, void *stream,
                         const Layout &lay, uint64_t y_poly_stride)
{
  int rc = plain_check(nlimbs, 2, plans, d_y, d_a, batch, lay, y_poly_stride);
  if(rc || batch == 0) return rc;
  USE_DEVICE(plans[0]->device);
  PlainDoubleArgs pa{};
  const uint64_t  q0 = plans[0]->q;
  pa.k.q_lo          = q0;
  if(nlimbs == 2) {
    const uint64_t          q1 = plans[1]->q;
    const uint64_t          b[2] = {q0, q1};
    const unsigned __int128 Q    = (unsigned __int128)q0 * q1;
    bconv_sources(b, 2, false, pa.k.sl); /* {q_0, 0, [q_1^-1]_{q_0}}, {q_1, 0, [q_0^-1]_{q_1}} */
    pa.k.q_lo = (uint64_t)Q;
    pa.k.q_hi = (uint64_t)(Q >> 64);
  }
  pa.k.scale       = scale;
  pa.y             = d_y;
  pa.a             = d_a;
  pa.a_limb_stride = lay.limb;
  pa.a_poly_stride = lay.poly;
  pa.y_poly_stride = y_poly_stride;
  pa.batch         = batch;
  pa.logn          = (uint32_t)plans[0]->m;
  pa.nlimbs        = nlimbs;
  pa.max_grid      = plans[0]->max_grid;
  pa.stream        = (hipStream_t)stream;
  const hipError_t e = launch_plain_double(pa);
  if(e != hipSuccess) return fail(NTT_ERR_HIP, std::string("plain_double_kernel: ") + hipGetErrorString(e));
  return NTT_OK;
}

extern "C" int ntt_rns_to_plain_batch(int nlimbs, ntt_plan *const *plans, uint64_t *d_m, const uint64_t *d_a, uint64_t t, uint64_t batch,
                                      unsigned flags, void *stream)
{
  return rns_to_plain(nlimbs, plans, d_m, d_a, t, batch, flags, stream, limb_major(plans, nlimbs, batch),
                      (nlimbs > 0 && plans && plans[0]) ? plans[0]->N : 0);
}

extern "C" int ntt_rns_to_plain_batch_strided(int nlimbs, ntt_plan *const *plans, uint64_t *d_m, const uint64_t *d_a, uint64_t t,
                                              uint64_t a_limb_stride, uint64_t a_poly_stride, uint64_t m_poly_stride, uint64_t batch,
                                              unsigned flags, void *stream)
{
  return rns_to_plain(nlimbs, plans, d_m, d_a, t, batch, flags, stream, Layout{a_limb_stride, a_poly_stride}, m_poly_stride);
}

extern "C" int ntt_rns_to_double_batch(int nlimbs, ntt_plan *const *plans, double *d_y, const uint64_t *d_a, double scale, uint64_t batch,
                                       void *stream)
{
  return rns_to_double(nlimbs, plans, d_y, d_a, scale, batch, stream, limb_major(plans, nlimbs, batch),
                       (nlimbs > 0 && plans && plans[0]) ? plans[0]->N : 0);
}

extern "C" int ntt_rns_to_double_batch_strided(int nlimbs, ntt_plan *const *plans, double *d_y, const uint64_t *d_a, double scale,
                                               uint64_t a_limb_stride, uint64_t a_poly_stride, uint64_t y_poly_stride, uint64_t batch,
                                               void *stream)
{
  return rns_to_double(nlimbs, plans, d_y, d_a, scale, batch, stream, Layout{a_limb_stride, a_poly_stride}, y_poly_stride);
}
