/*
 * emu_scaled.cpp -- the checked twin of ArithF64S (csrc/ntt_arith.h) run through the emulator's block and column passes
 * (TEST INFRASTRUCTURE, built by tests/test_scaled_cpu.py with the flags of tests/emu/Makefile, one translation unit per
 * modulus class: -DEMU_SCALED_KSH=0 | 1 | 18).  Every claim of the scaled representation is asserted with 128-bit integers:
 * every value is an integer multiple of S = 2^-1074 below 2^53 S, every sum, product and reduction is exact, and the products
 * obey rho(B) = 1/2 + B theta2 / 2 (full record), 1/2 + B theta2 (compact twiddle), theta2 = q / 2^53.
 */
#define EMU_PART 99 /* a part the emulator's own build does not use: the templates, no instantiation, no C interface */
#include "emu.cpp"

#ifndef EMU_SCALED_KSH
#  error "build with -DEMU_SCALED_KSH=0, 1 or 18"
#endif

struct ArithF64SChk : ArithF64S {
  /* v = V * 2^-1074 with |V| < 2^53: every double below 2^53 S in magnitude is a multiple of S, so the range is the claim */
  static __int128 as_int(double v)
  {
    if(!(__builtin_fabs(v) < 0x1p-1021)) g_chk_fail++;
    return (__int128)__builtin_ldexp(v, 1074); /* exact: an integer below 2^53 */
  }
  static double units(double v) { return __builtin_ldexp(v, 1074); }
  static void   see(double v, const consts &c)
  {
    (void)as_int(v);
    const double b = __builtin_fabs(units(v)) / c.q;
    if(b > g_chk_maxb) g_chk_maxb = b;
  }
  /* r == y * w (mod q) exactly, |r| <= (1/2 + cc |y|/q theta2) q */
  static void product_claims(double r, double y, double w, double cc, const consts &c)
  {
    const __int128 ex = as_int(y) * (__int128)w;
    if(w != __builtin_rint(w)) g_chk_fail++;
    if((ex - as_int(r)) % (__int128)c.qi != 0) g_chk_fail++;
    const double by = __builtin_fabs(units(y)) / c.q, th2 = c.q / 9007199254740992.0;
    if(__builtin_fabs(units(r)) > (0.5 + cc * by * th2) * c.q * (1.0 + 1e-12) + 1.0) g_chk_fail++;
    const double rb = __builtin_fabs(units(r)) / c.q;
    if(rb > g_chk_maxr) g_chk_maxr = rb;
  }
  static double mulmod(const tw &t, double y, const consts &c)
  {
    const double r = ArithF64S::mulmod(t, y, c);
    product_claims(r, y, t.w, 0.5, c);
    return r;
  }
  static double mulmod_c(ctw w, double y, const consts &c)
  {
    const double r = ArithF64S::mulmod_c(w, y, c);
    product_claims(r, y, w, 1.0, c);
    return r;
  }
  static double reduce(double v, const consts &c)
  {
    const double r = ArithF64S::reduce(v, c);
    if((as_int(v) - as_int(r)) % (__int128)c.qi != 0) g_chk_fail++;
    if(__builtin_fabs(units(r)) > 0.5 * c.q + 2.0) g_chk_fail++;
    return r;
  }
  /* a sum or difference of two scaled values is exact */
  static double add(double a, double b, const consts &c)
  {
    const double s = a + b;
    see(s, c);
    if(as_int(a) + as_int(b) != as_int(s)) g_chk_fail++;
    return s;
  }
  template <bool RED> static void fwd_bfly(val &x, val &y, const tw &t, const consts &c)
  {
    see(x, c);
    see(y, c);
    const double xr = RED ? reduce(x, c) : x;
    const double m  = mulmod(t, y, c);
    x               = add(xr, m, c);
    y               = add(xr, -m, c);
  }
  template <bool RED> static void fwd_bfly(val &x, val &y, ctw w, const consts &c)
  {
    see(x, c);
    see(y, c);
    const double xr = RED ? reduce(x, c) : x;
    const double m  = mulmod_c(w, y, c);
    x               = add(xr, m, c);
    y               = add(xr, -m, c);
  }
  template <bool RED> static void inv_bfly(val &x, val &y, const tw &t, const consts &c)
  {
    const double s = add(x, y, c);
    const double d = add(x, -y, c);
    x              = RED ? reduce(s, c) : s;
    y              = mulmod(t, d, c);
  }
  template <bool RED> static void inv_bfly(val &x, val &y, ctw w, const consts &c)
  {
    const double s = add(x, y, c);
    const double d = add(x, -y, c);
    x              = RED ? reduce(s, c) : s;
    y              = mulmod_c(w, d, c);
  }
  static void inv_bfly_last(val &x, val &y, const consts &c)
  {
    const double s = add(x, y, c);
    const double d = add(x, -y, c);
    x              = mulmod(c.ninv, s, c);
    y              = mulmod(c.wninv, d, c);
  }
  static val      scale_ninv(val v, const consts &c) { return mulmod(c.ninv, v, c); }
  static uint64_t store_fwd(val v, const consts &c)
  {
    const uint64_t u = ArithF64S::to_canonical(v, c);
    __int128       m = as_int(v) % (__int128)c.qi;
    if(m < 0) m += c.qi;
    if(u >= c.qi || (__int128)u != m) g_chk_fail++;
    return u;
  }
  static uint64_t store_inv(val v, const consts &c) { return store_fwd(v, c); }
  static uint64_t store_inv_lazy(val v, const consts &c) { return store_fwd(v, c); }
  static uint64_t store_fwd_lazy(val v, const consts &c)
  {
    const uint64_t u = ArithF64S::store_fwd_lazy(v, c);
    if((__int128)u != as_int(v) + 2 * (__int128)c.qi || u >= 4 * c.qi) g_chk_fail++;
    return u;
  }
};

#define EMU_SCALED_CAT2(a, b) a##b
#define EMU_SCALED_CAT(a, b) EMU_SCALED_CAT2(a, b)

extern "C" {
/* one transform of `batch` polynomials of 2^m points in the checked scaled policy of this unit's class; -3: q belongs to another
 * class; lazy: forward outputs in [0,4q) */
int EMU_SCALED_CAT(emu_scaled_transform_k, EMU_SCALED_KSH)(uint64_t *a, uint64_t batch, int m, uint64_t q, uint64_t root, int inverse, int wide,
                                                          int lazy)
{
  if(!h_f64_eligible(q)) return -2;
  const int kk = h_f64_ksh(q) >= 18 ? 18 : (h_f64_ksh(q) >= 1 ? 1 : 0);
  if(kk != EMU_SCALED_KSH) return -3;
  const uint64_t N    = 1ull << m;
  const uint64_t rinv = h_powmod(root, q - 2, q);
  const auto     w    = h_power_table(root, N, q);
  const auto     wi   = h_power_table(rinv, N, q);
  const auto     wix  = h_with_folded_ninv(wi, h_powmod(N % q, q - 2, q), q);
  const auto &   src  = inverse ? wix : w;
  std::vector<TwF64>  tab(src.size());
  std::vector<double> tab8(src.size());
  for(uint64_t i = 0; i < src.size(); i++) {
    tab[i]  = h_tw_f64(src[i], q);
    tab8[i] = tab[i].w;
  }
  const auto c = h_consts_f64(q, N, wi);
  g_lazy       = lazy != 0;
  const int rc = inverse ? emu_run<ArithF64SChk, true, EMU_SCALED_KSH>(a, batch, m, tab.data(), c, false, wide != 0, tab8.data())
                         : emu_run<ArithF64SChk, false, EMU_SCALED_KSH>(a, batch, m, tab.data(), c, false, wide != 0, tab8.data());
  g_lazy       = false;
  return rc;
}

#if EMU_SCALED_KSH == 0
/* {violated claims, 1e6 * max |value| / q, 1e6 * max |product| / q} since the last reset */
void emu_scaled_stats(uint64_t *out, int reset)
{
  out[0] = g_chk_fail;
  out[1] = (uint64_t)(g_chk_maxb * 1e6);
  out[2] = (uint64_t)(g_chk_maxr * 1e6);
  if(reset) {
    g_chk_fail = 0;
    g_chk_maxb = g_chk_maxr = 0;
  }
}
#endif
}
