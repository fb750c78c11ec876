/* host/host_galois.inc -- the Galois automorphisms sigma_g: a(X) -> a(X^g) and the rotation key product: ntt_galois_rotation,
 * ntt_galois_batch, ntt_rns_galois_batch, ntt_rns_galois_dot_batch, ntt_rns_galois_dot_pair_batch and the strided forms.  A section of ntt_host.hip (one translation
 * unit, included from there in order); not compiled by itself.  The kernels are in galois_coef.hip and keypair_dot2.hip; this section sees their launchers
 * and the index functions only (ntt_galois.h).
 *
 *   galois       out of place; NTT domain -- galois_ntt_kernel, a permutation of words (lazy words pass through); coefficients --
 *                galois_coef_kernel (canonical words).  One launch per 16 limbs.
 *   galois_dot   c^ (+)= sum_i sigma_g(a_i^) (.) key_i^ in the NTT domain -- galois_dot_kernel, one launch per 16 limbs: the hoisted
 *                digits are permuted on their way into the product, never materialised.  The pair form (both components of the
 *                rotation key) -- keypair_dot2_kernel, likewise: each permuted digit word read once for the two sums.
 * Nothing is allocated, the host is not synchronised and no memset is issued: the calls can be captured into a graph. */

/* the words [p, p + extent) an operand spans: limbs x polynomials of N words under the layout (a broadcast key: [limb][N]) */
struct GaloisSpan {
  uintptr_t         lo;
  unsigned __int128 bytes;
};
static GaloisSpan galois_span(const uint64_t *p, uint64_t N, int nlimbs, uint64_t batch, uint64_t limb_stride, uint64_t poly_stride)
{
  const unsigned __int128 words = (unsigned __int128)(nlimbs - 1) * limb_stride + (unsigned __int128)(batch - 1) * poly_stride + N;
  return GaloisSpan{(uintptr_t)p, words * 8};
}
static bool galois_overlap(const GaloisSpan &a, const GaloisSpan &b)
{
  return (unsigned __int128)a.lo < (unsigned __int128)b.lo + b.bytes && (unsigned __int128)b.lo < (unsigned __int128)a.lo + a.bytes;
}

/* what every form checks first: the limb list, g odd in (0, 2N), the layout */
static int galois_check(int nlimbs, ntt_plan *const *plans, uint64_t g, uint64_t batch, const Layout &lay)
{
  int rc = rns_check(nlimbs, plans);
  if(rc) return rc;
  const uint64_t N = plans[0]->N;
  if(plans[0]->m < 1 || plans[0]->m > 30) return fail(NTT_ERR_ARG, "galois: N out of range");
  if(!(g & 1) || g >= 2 * N) return fail(NTT_ERR_ARG, "galois: g must be odd and below 2N");
  return layout_check(N, nlimbs, batch, lay);
}

static int rns_galois(int nlimbs, ntt_plan *const *plans, uint64_t *d_out, const uint64_t *d_in, uint64_t g, uint64_t batch, unsigned flags,
                      void *stream, const Layout &lay)
{
  if(flags & ~(unsigned)NTT_GALOIS_TRANSFORMED) return fail(NTT_ERR_ARG, "unknown flag");
  if(!d_out || !d_in) return fail(NTT_ERR_ARG, "null argument");
  int rc = galois_check(nlimbs, plans, g, batch, lay);
  if(rc || batch == 0) return rc;
  const uint64_t N = plans[0]->N;
  if(galois_overlap(galois_span(d_out, N, nlimbs, batch, lay.limb, lay.poly), galois_span(d_in, N, nlimbs, batch, lay.limb, lay.poly)))
    return fail(NTT_ERR_ARG, "galois: the output overlaps the input (the call is out of place)");
  USE_DEVICE(plans[0]->device);
  GaloisArgs ga{};
  ga.limb_stride = lay.limb;
  ga.poly_stride = lay.poly;
  ga.batch       = batch;
  ga.logn        = (uint32_t)plans[0]->m;
  ga.g           = (uint32_t)g;
  ga.ntt_domain  = (flags & NTT_GALOIS_TRANSFORMED) != 0;
  ga.max_grid    = plans[0]->max_grid;
  ga.stream      = (hipStream_t)stream;
  for(int first = 0; first < nlimbs; first += kGaloisLimbs) {
    ga.nlimbs = nlimbs - first < kGaloisLimbs ? nlimbs - first : kGaloisLimbs;
    ga.out    = d_out + (uint64_t)first * lay.limb;
    ga.in     = d_in + (uint64_t)first * lay.limb;
    for(int l = 0; l < ga.nlimbs; l++) ga.q[l] = plans[first + l]->q;
    const hipError_t e = launch_galois(ga);
    if(e != hipSuccess) return fail(NTT_ERR_HIP, std::string(ga.ntt_domain ? "galois_ntt_kernel: " : "galois_coef_kernel: ") + hipGetErrorString(e));
  }
  return NTT_OK;
}

extern "C" uint64_t ntt_galois_rotation(uint64_t N, int64_t steps)
{
  if(N < 2 || (N & (N - 1)) || N > (1ull << 62)) return 0;
  /* 5 has order N / 2 in (Z / 2N)^* (order 1 for N = 2) */
  const uint64_t ord = N >= 4 ? N / 2 : 1, mod = 2 * N;
  int64_t        r   = steps % (int64_t)ord;
  uint64_t       e   = (uint64_t)(r < 0 ? r + (int64_t)ord : r), b = 5 % mod, x = 1;
  for(; e; e >>= 1) {
    if(e & 1) x = (uint64_t)((unsigned __int128)x * b % mod);
    b = (uint64_t)((unsigned __int128)b * b % mod);
  }
  return x;
}

extern "C" int ntt_galois_batch(const ntt_plan *p, uint64_t *d_out, const uint64_t *d_in, uint64_t g, uint64_t batch, unsigned flags, void *stream)
{
  ntt_plan *const one[1] = {const_cast<ntt_plan *>(p)};
  return rns_galois(1, one, d_out, d_in, g, batch, flags, stream, limb_major(one, 1, batch));
}

extern "C" int ntt_rns_galois_batch(int nlimbs, ntt_plan *const *plans, uint64_t *d_out, const uint64_t *d_in, uint64_t g, uint64_t batch,
                                    unsigned flags, void *stream)
{
  return rns_galois(nlimbs, plans, d_out, d_in, g, batch, flags, stream, limb_major(plans, nlimbs, batch));
}

extern "C" int ntt_rns_galois_batch_strided(int nlimbs, ntt_plan *const *plans, uint64_t *d_out, const uint64_t *d_in, uint64_t g,
                                            uint64_t limb_stride, uint64_t poly_stride, uint64_t batch, unsigned flags, void *stream)
{
  return rns_galois(nlimbs, plans, d_out, d_in, g, batch, flags, stream, Layout{limb_stride, poly_stride});
}

/* nc = 1: c^ = d_c[0] with the keys d_keyhat[0]; nc = 2: the pair form, both components of the key in one launch per 16 limbs */
static int rns_galois_dot(int nlimbs, ntt_plan *const *plans, int nc, uint64_t *const *d_c, int k, const uint64_t *const *d_ahat,
                          const uint64_t *const *const *d_keyhat, uint64_t g, uint64_t batch, unsigned flags, void *stream, const Layout &lay)
{
  if(flags & ~(unsigned)(NTT_GALOIS_TRANSFORMED | NTT_GALOIS_ACCUMULATE | NTT_GALOIS_KEY_BROADCAST)) return fail(NTT_ERR_ARG, "unknown flag");
  if(k < 1 || k > kGaloisDot || !d_ahat) return fail(NTT_ERR_ARG, "number of operand pairs must be 1 .. 32");
  for(int j = 0; j < nc; j++) {
    if(!d_keyhat[j]) return fail(NTT_ERR_ARG, "number of operand pairs must be 1 .. 32");
    if(!d_c[j]) return fail(NTT_ERR_ARG, "null argument");
  }
  for(int i = 0; i < k; i++) {
    if(!d_ahat[i]) return fail(NTT_ERR_ARG, "null operand"); /* (before any limb offset is added) */
    for(int j = 0; j < nc; j++) {
      if(!d_keyhat[j][i]) return fail(NTT_ERR_ARG, "null operand");
    }
  }
  int rc = galois_check(nlimbs, plans, g, batch, lay);
  if(rc || batch == 0) return rc;
  const uint64_t   N      = plans[0]->N;
  const bool       bcast  = (flags & NTT_GALOIS_KEY_BROADCAST) != 0;
  const uint64_t   kls    = bcast ? N : lay.limb, kps = bcast ? 0 : lay.poly; /* a broadcast key is [limb][N] */
  for(int j = 0; j < nc; j++) {
    const GaloisSpan out = galois_span(d_c[j], N, nlimbs, batch, lay.limb, lay.poly);
    if(j == 1 && galois_overlap(out, galois_span(d_c[0], N, nlimbs, batch, lay.limb, lay.poly)))
      return fail(NTT_ERR_ARG, "galois_dot: the two outputs overlap");
    for(int i = 0; i < k; i++) {
      bool hit = galois_overlap(out, galois_span(d_ahat[i], N, nlimbs, batch, lay.limb, lay.poly));
      for(int jj = 0; jj < nc; jj++) hit = hit || galois_overlap(out, galois_span(d_keyhat[jj][i], N, nlimbs, bcast ? 1 : batch, kls, kps));
      if(hit) return fail(NTT_ERR_ARG, "galois_dot: the output overlaps an operand (the call is out of place)");
    }
  }
  USE_DEVICE(plans[0]->device);
  GaloisDotArgs  da{};
  GaloisDot2Args da2{};
  da.k = da2.k                             = k;
  da.limb_stride = da2.limb_stride         = lay.limb;
  da.poly_stride = da2.poly_stride         = lay.poly;
  da.key_limb_stride = da2.key_limb_stride = kls;
  da.key_poly_stride = da2.key_poly_stride = kps;
  da.batch = da2.batch                     = batch;
  da.logn = da2.logn                       = (uint32_t)plans[0]->m;
  da.g = da2.g                             = (uint32_t)g;
  da.accumulate = da2.accumulate           = (flags & NTT_GALOIS_ACCUMULATE) != 0;
  da.max_grid = da2.max_grid               = plans[0]->max_grid;
  da.stream = da2.stream                   = (hipStream_t)stream;
  for(int first = 0; first < nlimbs; first += kGaloisLimbs) {
    da.nlimbs = da2.nlimbs = nlimbs - first < kGaloisLimbs ? nlimbs - first : kGaloisLimbs;
    da.c                   = d_c[0] + (uint64_t)first * lay.limb;
    for(int j = 0; j < nc; j++) da2.c[j] = d_c[j] + (uint64_t)first * lay.limb;
    for(int i = 0; i < k; i++) {
      da.a[i] = da2.a[i] = d_ahat[i] + (uint64_t)first * lay.limb;
      da.key[i]          = d_keyhat[0][i] + (uint64_t)first * kls;
      for(int j = 0; j < nc; j++) da2.key[j][i] = d_keyhat[j][i] + (uint64_t)first * kls;
    }
    for(int l = 0; l < da.nlimbs; l++) da.ql[l] = da2.ql[l] = bconv_dst(plans[first + l]->q);
    const hipError_t e = nc == 2 ? launch_galois_dot2(da2) : launch_galois_dot(da);
    if(e != hipSuccess) return fail(NTT_ERR_HIP, std::string(nc == 2 ? "keypair_dot2_kernel: " : "galois_dot_kernel: ") + hipGetErrorString(e));
  }
  return NTT_OK;
}

extern "C" int ntt_rns_galois_dot_batch(int nlimbs, ntt_plan *const *plans, uint64_t *d_c, int k, const uint64_t *const *d_ahat,
                                        const uint64_t *const *d_keyhat, uint64_t g, uint64_t batch, unsigned flags, void *stream)
{
  return rns_galois_dot(nlimbs, plans, 1, &d_c, k, d_ahat, &d_keyhat, g, batch, flags, stream, limb_major(plans, nlimbs, batch));
}

extern "C" int ntt_rns_galois_dot_batch_strided(int nlimbs, ntt_plan *const *plans, uint64_t *d_c, int k, const uint64_t *const *d_ahat,
                                                const uint64_t *const *d_keyhat, uint64_t g, uint64_t limb_stride, uint64_t poly_stride,
                                                uint64_t batch, unsigned flags, void *stream)
{
  return rns_galois_dot(nlimbs, plans, 1, &d_c, k, d_ahat, &d_keyhat, g, batch, flags, stream, Layout{limb_stride, poly_stride});
}

/* the pair form: c0^ (+)= sum_i sigma_g(a_i^) (.) key0_i^ and c1^ (+)= sum_i sigma_g(a_i^) (.) key1_i^, every permuted digit read once */
extern "C" int ntt_rns_galois_dot_pair_batch(int nlimbs, ntt_plan *const *plans, uint64_t *d_c0, uint64_t *d_c1, int k, const uint64_t *const *d_ahat,
                                             const uint64_t *const *d_key0hat, const uint64_t *const *d_key1hat, uint64_t g, uint64_t batch,
                                             unsigned flags, void *stream)
{
  uint64_t *const              c[2]   = {d_c0, d_c1};
  const uint64_t *const *const key[2] = {d_key0hat, d_key1hat};
  return rns_galois_dot(nlimbs, plans, 2, c, k, d_ahat, key, g, batch, flags, stream, limb_major(plans, nlimbs, batch));
}

extern "C" int ntt_rns_galois_dot_pair_batch_strided(int nlimbs, ntt_plan *const *plans, uint64_t *d_c0, uint64_t *d_c1, int k,
                                                     const uint64_t *const *d_ahat, const uint64_t *const *d_key0hat,
                                                     const uint64_t *const *d_key1hat, uint64_t g, uint64_t limb_stride, uint64_t poly_stride,
                                                     uint64_t batch, unsigned flags, void *stream)
{
  uint64_t *const              c[2]   = {d_c0, d_c1};
  const uint64_t *const *const key[2] = {d_key0hat, d_key1hat};
  return rns_galois_dot(nlimbs, plans, 2, c, k, d_ahat, key, g, batch, flags, stream, Layout{limb_stride, poly_stride});
}
