/*
 * launch_probe.hip -- what every launcher of csrc/ntt_kernels_launch.h, ntt_kernels_rescale.h and the four fused ModDown headers
 * (ntt_kernels_keyswitch.h, ntt_kernels_ksfold.h, ntt_kernels_bgv.h, ntt_kernels_exact.h) WOULD launch, recorded instead of launched: a host-only program (no device, no HIP call) for comparing two versions of the launch layer.
 *
 *   make launch-probe            builds build/launch_probe_<pair> for every (policy, class) pair the library instantiates
 *   make launch-probe PROBE_CSRC=<another csrc> PROBE_OUT=build/other      the same source against another version of the headers
 *   build/launch_probe_f64k0 > new.txt ; build/other/launch_probe_f64k0 > old.txt ; cmp old.txt new.txt
 *
 * hipLaunchKernelGGL is redefined to print the kernel instance (the mangled name of Tag<&kernel>, which carries every template
 * argument), grid.x, grid.y, block.x and an FNV-1a hash over the bytes of the kernel arguments; after every call the launcher's
 * return code follows, so refused calls are part of the record.  The sweep uses only the type-erased interface (the *Args structs,
 * launch_*<A, KSH>, the NTT_DEFINE_LAUNCH_* macros), null data pointers, zeroed limb records and a fake non-null control block.
 * The last line on stderr is the number of distinct kernel instances reached; -names prints them (one per line) instead of the record.
 *
 * Compile with -DPROBE_POLICY=<policy> -DPROBE_KSH=<class> -DPROBE_KIND=<1: FP64 policies, every family; 2: integer policies:
 * passes, dot, forward-multiply; 3: the radix-4 formulation: passes>.
 */
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <typeinfo>

namespace probe {
template <auto K> struct Tag {};
static std::set<std::string> names;
static bool                  quiet = false;
static uint64_t fnv(uint64_t h, const void *p, size_t n)
{
  const unsigned char *b = static_cast<const unsigned char *>(p);
  for(size_t i = 0; i < n; i++) h = (h ^ b[i]) * 1099511628211ull;
  return h;
}
template <class... T> static void record(const char *name, dim3 g, dim3 b, const T &...args)
{
  uint64_t h = 14695981039346656037ull;
  ((h = fnv(h, &args, sizeof args)), ...);
  names.insert(name);
  if(!quiet) printf(" %s %u %u %u %016llx\n", name, g.x, g.y, b.x, (unsigned long long)h);
}
} /* namespace probe */

#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(k, g, b, shm, st, ...) ::probe::record(typeid(::probe::Tag<&k>).name(), g, b, __VA_ARGS__)
#define hipGetLastError() hipSuccess

#include "ntt_kernels.h"
#if PROBE_KIND == 1
#include "ntt_kernels_rescale.h"
#include "ntt_kernels_keyswitch.h"
#include "ntt_kernels_ksfold.h"
#include "ntt_kernels_bgv.h"
#include "ntt_kernels_exact.h"
#endif

namespace ntt {
#if PROBE_KIND == 3
NTT_DEFINE_LAUNCH_PASS_RADIX4(PROBE_POLICY, PROBE_KSH)
#else
NTT_DEFINE_LAUNCH_PASS(PROBE_POLICY, PROBE_KSH)
#endif
#if PROBE_KIND != 3
NTT_DEFINE_LAUNCH_DOT(PROBE_POLICY, PROBE_KSH)
NTT_DEFINE_LAUNCH_FWD_MUL(PROBE_POLICY, PROBE_KSH)
#endif
#if PROBE_KIND == 1
NTT_DEFINE_LAUNCH_PRODUCT(PROBE_POLICY, PROBE_KSH)
NTT_DEFINE_LAUNCH_TEAM_PRODUCT(PROBE_POLICY, PROBE_KSH)
NTT_DEFINE_LAUNCH_RESCALE_FWD(PROBE_POLICY, PROBE_KSH)
NTT_DEFINE_LAUNCH_MODDOWN_FWD(PROBE_POLICY, PROBE_KSH)
NTT_DEFINE_LAUNCH_KSFOLD_FWD(PROBE_POLICY, PROBE_KSH)
NTT_DEFINE_LAUNCH_MODDOWN_BGV_FWD(PROBE_POLICY, PROBE_KSH)
NTT_DEFINE_LAUNCH_MODDOWN_EXACT_FWD(PROBE_POLICY, PROBE_KSH)
#endif
} /* namespace ntt */

using namespace ntt;
using A = PROBE_POLICY;
constexpr int KSH = PROBE_KSH;

static LimbRec<A>      recs[kMaxLimbs]; /* zeroed */
static const uint64_t *dot_ptrs[kMaxDot + 1];
static void *const     fake_ctl = reinterpret_cast<void *>(uintptr_t(0x10000)); /* never dereferenced: nothing is launched */

static const uint64_t kBatch[]  = {0, 1, 2, 7, 255, 256, 257, 1000, 4097, 1ull << 20};
static const int      kLimbs[]  = {1, 3};
static const int      kCus[]    = {0, 8, 256};
static const int      kGrid[]   = {0, 5, 64};
static const int      kOversub[] = {0, 1, 16};

/* the axes every launcher shares */
struct Common {
  uint64_t batch;
  int      nlimbs, num_cus, max_grid, oversub;
  /* the corner every flag combination is crossed with; the other points see the launcher's primary flags only */
  bool poly_major() const { return nlimbs > 1 && num_cus == 8; } /* [batch][limb][N] instead of [limb][batch][N] */
  uint64_t limb_stride(uint32_t logn) const { return poly_major() ? 1ull << logn : batch << logn; }
  uint64_t poly_stride(uint32_t logn) const { return poly_major() ? (uint64_t)nlimbs << logn : 0; }
  bool small() const { return (batch == 0 || batch == 7 || batch == 4097) && num_cus == 256 && max_grid != 64 && oversub == 0; }
};
template <class F> static void for_common(F &&f)
{
  for(uint64_t batch : kBatch)
    for(int nl : kLimbs)
      for(int cus : kCus)
        for(int mg : kGrid)
          for(int os : kOversub) f(Common{batch, nl, cus, mg, os});
}
static void done(hipError_t e)
{
  if(!probe::quiet) printf("-> %d\n", (int)e);
}

static void sweep_pass(uint32_t logn)
{
  for(int fused = 0; fused <= 4; fused++)
    for(int r = 1; r <= 14; r++)
      for(int s = 0; s <= 5; s++) {
        if(s + r > (int)logn) continue;
        if(fused == 0 && (r > 4 || s > 3)) continue;
        if(fused == 1 && !(r >= 6 && (logn <= 14 ? (r == (int)logn && s == 0) : ((r == 12 || r == 14) && s + r == (int)logn)))) continue;
        if(fused == 2 && !(s == 0 && r <= 3 && (int)logn == 14 + r)) continue;
        if(fused == 3 && !(s == 0 && r >= 3 && r <= 5 && (int)logn == 12 + r)) continue;
        if(fused == 4 && !(s == 0 && r == 1)) continue;
        for(int flags = 0; flags < 32; flags++)
          for_common([&](const Common &c) {
            const bool primary = (flags & 1) == 0 ? (flags >> 1) == 0 : (flags >> 1) == 15; /* forward, plain; inverse, every flag */
            if(!primary && !c.small()) return;
            PassArgs pa{};
            pa.limbs = recs, pa.nlimbs = c.nlimbs, pa.limb_stride = c.limb_stride(logn), pa.poly_stride = c.poly_stride(logn), pa.batch = c.batch, pa.logn = logn;
            pa.fused = fused, pa.r = r, pa.s = s;
            pa.inverse = flags & 1, pa.wide = (flags >> 1) & 1, pa.lastinv = (flags >> 2) & 1, pa.lazy = (flags >> 3) & 1, pa.ends = (flags >> 4) & 1;
            pa.max_grid = c.max_grid, pa.num_cus = c.num_cus, pa.oversub = c.oversub;
            pa.team_ctl = fused == 3 ? fake_ctl : nullptr;
            if(!probe::quiet) printf("pass %u f%d r%d s%d fl%d b%llu l%d c%d g%d o%d\n", logn, fused, r, s, flags, (unsigned long long)c.batch, c.nlimbs, c.num_cus, c.max_grid, c.oversub);
            done(launch_pass<A, KSH>(pa));
          });
      }
}

#if PROBE_KIND != 3
static void sweep_dot_mul(uint32_t logn)
{
  static const int kPairs[] = {1, kMaxDot, 0, kMaxDot + 1};
  for(uint32_t block_log : {0u, 12u, 13u, 14u})
    for(int team = 0; team < 2; team++)
      for(int ptrs = 0; ptrs < 2; ptrs++)
        for(int flags = 0; flags < 4; flags++)
          for(int np : kPairs)
            for_common([&](const Common &c) {
              if(((flags != 0 && flags != 3) || np < 1 || np > kMaxDot) && !c.small()) return;
              DotArgs da{};
              da.a = dot_ptrs, da.b = dot_ptrs, da.npairs = np, da.lazy_in = flags & 1, da.b_bcast = flags >> 1;
              da.limbs = recs, da.nlimbs = c.nlimbs, da.limb_stride = c.limb_stride(logn), da.b_limb_stride = (flags >> 1) ? (1ull << logn) : da.limb_stride;
              da.poly_stride = c.poly_stride(logn), da.batch = c.batch, da.logn = logn, da.block_log = block_log;
              da.max_grid = c.max_grid, da.num_cus = c.num_cus, da.oversub = c.oversub, da.team_ctl = team ? fake_ctl : nullptr;
              da.team_lag = c.oversub, da.team_wpc = c.oversub == 16 ? 2 : 0, da.ptrs = ptrs, da.ptr_limb_off = ptrs ? 3ull << logn : 0;
              if(!probe::quiet) printf("dot %u k%u t%d p%d fl%d n%d b%llu l%d c%d g%d o%d\n", logn, block_log, team, ptrs, flags, np, (unsigned long long)c.batch, c.nlimbs, c.num_cus, c.max_grid, c.oversub);
              done(launch_dot<A, KSH>(da));
            });
  for(uint32_t block_log : {0u, 12u, 13u, 14u})
    for(int mode = 0; mode < 3; mode++) /* blocks, team, one pass */
      for(int ptrs = 0; ptrs < 2; ptrs++)
        for(int flags = 0; flags < 8; flags++)
          for_common([&](const Common &c) {
            if(flags != 0 && flags != 7 && !c.small()) return;
            MulArgs ma{};
            ma.lazy_in = flags & 1, ma.b_bcast = (flags >> 1) & 1, ma.accumulate = flags >> 2;
            ma.limbs = recs, ma.nlimbs = c.nlimbs, ma.limb_stride = c.limb_stride(logn), ma.b_limb_stride = ma.b_bcast ? (1ull << logn) : ma.limb_stride;
            ma.poly_stride = c.poly_stride(logn), ma.batch = c.batch, ma.logn = logn, ma.block_log = block_log;
            ma.max_grid = c.max_grid, ma.num_cus = c.num_cus, ma.oversub = c.oversub, ma.team_ctl = mode == 1 ? fake_ctl : nullptr;
            ma.team_lag = c.oversub, ma.team_wpc = c.oversub == 16 ? 2 : 0, ma.one_pass = mode == 2, ma.ptrs = ptrs, ma.ptr_limb_off = ptrs ? 3ull << logn : 0;
            if(!probe::quiet) printf("mul %u k%u m%d p%d fl%d b%llu l%d c%d g%d o%d\n", logn, block_log, mode, ptrs, flags, (unsigned long long)c.batch, c.nlimbs, c.num_cus, c.max_grid, c.oversub);
            done(launch_fwd_mul<A, KSH>(ma));
          });
}
#endif

#if PROBE_KIND == 1
static void sweep_product(uint32_t logn)
{
  for(uint32_t block_log : {0u, 12u, 13u, 14u})
    for(int team = 0; team < 2; team++)
      for(int flags = 0; flags < 16; flags++)
        for_common([&](const Common &c) {
          ProdArgs pa{};
          pa.limbs = recs, pa.nlimbs = c.nlimbs, pa.limb_stride = c.limb_stride(logn);
          pa.poly_stride = c.poly_stride(logn), pa.batch = c.batch, pa.logn = logn, pa.block_log = block_log;
          pa.a_lazy = flags & 1, pa.both = (flags >> 1) & 1, pa.ptrs = (flags >> 2) & 1, pa.four = flags >> 3;
          pa.max_grid = c.max_grid, pa.num_cus = c.num_cus, pa.oversub = c.oversub, pa.team_ctl = team ? fake_ctl : nullptr;
          pa.team_lag = c.oversub, pa.team_wpc = c.oversub == 16 ? 2 : 0, pa.ptr_limb_off = pa.ptrs ? 3ull << logn : 0;
          if(!probe::quiet) printf("prod %u k%u t%d fl%d b%llu l%d c%d g%d o%d\n", logn, block_log, team, flags, (unsigned long long)c.batch, c.nlimbs, c.num_cus, c.max_grid, c.oversub);
          done(team ? launch_team_product<A, KSH>(pa) : launch_product<A, KSH>(pa));
        });
}

static void sweep_rescale_moddown(uint32_t logn)
{
  for(int nlimbs : {0, 1, 3, 16, 17})
    for(uint64_t batch : kBatch)
      for(int cus : kCus)
        for(int mg : kGrid) {
          RescaleFwdArgs ra{};
          ra.limbs = recs, ra.nlimbs = nlimbs, ra.limb_stride = batch << logn, ra.batch = batch, ra.logn = logn, ra.qL = 97, ra.hL = 48;
          ra.max_grid = mg, ra.num_cus = cus;
          if(!probe::quiet) printf("rescale %u b%llu l%d c%d g%d\n", logn, (unsigned long long)batch, nlimbs, cus, mg);
          done(launch_rescale_fwd<A, KSH>(ra));
          for(int np : {0, 1, 3, 16, 17}) {
            ModDownFwdArgs ma{};
            ma.limbs = recs, ma.nlimbs = nlimbs, ma.np = np, ma.limb_stride = batch << logn, ma.batch = batch, ma.logn = logn;
            ma.max_grid = mg, ma.num_cus = cus;
            if(!probe::quiet) printf("moddown %u b%llu l%d p%d c%d g%d\n", logn, (unsigned long long)batch, nlimbs, np, cus, mg);
            done(launch_moddown_fwd<A, KSH>(ma));
            /* the other variants of the fused ModDown over the same record: distinct constants in every array a launcher copies */
            for(int i = 0; i < kBconvLimbs; i++) {
              ma.pl[i].p = 1000003 + 2 * i, ma.pl[i].inv = 7 + i;
              ma.ql[i].q = 2000003 + 2 * i, ma.ql[i].s = 11 + i;
            }
            for(int form = 0; form < 3; form++) { /* overwrite, dense; accumulate, dense; accumulate, padded strides */
              KsFoldArgs ka{};
              ka.m = ma, ka.accumulate = form > 0;
              ka.out_limb_stride = form == 2 ? (batch << logn) + 64 : batch << logn, ka.out_poly_stride = form == 2 ? (1ull << logn) + 8 : 0;
              if(!probe::quiet) printf("ksfold %u b%llu l%d p%d c%d g%d f%d\n", logn, (unsigned long long)batch, nlimbs, np, cus, mg, form);
              done(launch_ksfold_fwd<A, KSH>(ka));
              ModDownBgvArgs ba{};
              ba.k = ka;
              for(int i = 0; i < kBconvLimbs; i++) ba.ts[i] = BgvScale{65537ull + i, 3ull + i};
              if(!probe::quiet) printf("bgv %u b%llu l%d p%d c%d g%d f%d\n", logn, (unsigned long long)batch, nlimbs, np, cus, mg, form);
              done(launch_moddown_bgv_fwd<A, KSH>(ba));
            }
            ModDownExactFwdArgs xa{};
            xa.ma = ma;
            for(int i = 0; i < kBconvLimbs; i++) xa.rho[i] = 1.0 / (double)(1000003 + 2 * i), xa.mq[i] = 5 + i;
            if(!probe::quiet) printf("exact %u b%llu l%d p%d c%d g%d\n", logn, (unsigned long long)batch, nlimbs, np, cus, mg);
            done(launch_moddown_exact_fwd<A, KSH>(xa));
          }
        }
}
#endif

int main(int argc, char **argv)
{
  probe::quiet = argc > 1 && !strcmp(argv[1], "-names");
  for(uint32_t logn = 6; logn <= 17; logn++) {
    sweep_pass(logn);
#if PROBE_KIND != 3
    sweep_dot_mul(logn);
#endif
#if PROBE_KIND == 1
    sweep_product(logn);
    sweep_rescale_moddown(logn);
#endif
  }
  if(probe::quiet)
    for(const std::string &n : probe::names) printf("%s\n", n.c_str());
  fprintf(stderr, "%zu kernel instances reached\n", probe::names.size());
  return 0;
}
