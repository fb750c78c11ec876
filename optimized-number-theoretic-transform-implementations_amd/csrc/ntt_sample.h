/*
 * ntt_sample.h -- random polynomials in the RNS, drawn on the device (ntt_rns_sample_batch): the generator, the three kinds, the
 * argument records and the launchers of the kernels (sample.hip, sample_f64*.hip), the host layer's view of them, and one output word
 * stated for host and device (sample_block, sample_small, sample_small_digit, sample_uniform_digit).
 *
 * Integer arithmetic only; the definition fixes every output word on every route, so the coefficient kernel, the fused kernel, the host
 * statement and the tests' Python model agree bit for bit.
 *
 * NOT A CRYPTOGRAPHIC GENERATOR.  Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) is a
 * statistical generator: it passes the statistical batteries and is predictable by design.  These calls serve reproducible workloads,
 * benchmarks, tests and simulation.  A deployment that needs a CSPRNG keeps sampling on its side and uploads through the lifts
 * (ntt_rns_from_plain_batch).  Callers separate u, e0, e1, ... by seed or by disjoint first_poly ranges.
 *
 * ONE 128-bit block per output coefficient, independent of layout, batch split, launch chunking and route:
 *   key     = (seed & 0xffffffff, seed >> 32)
 *   counter = (s, P & 0xffffffff, P >> 32, tag)      s: the position in [0, N);  P = first_poly + p mod 2^64, p the polynomial's index
 *   tag     = the kind for the small kinds;  2 | (l << 8) for the uniform kind, l the limb's index in the call's plans array
 * With out0..out3 the block's words:
 *   ternary (0)   w = out0 | out1 << 32;  v = mulhi64(w, 3) - 1 in {-1, 0, 1}, each with probability 1/3 within 2^-64
 *   cbd21 (1)     v = popcount(out0 & 0x1FFFFF) - popcount(out1 & 0x1FFFFF): the centred binomial, eta = 21, sigma = sqrt(10.5), |v| <= 21
 *                 both: c_l = [mult v]_{q_l} in every limb (the same v), 1 <= mult < 2^61 reduced per limb on the host, Shoup product
 *   uniform (2)   c_l = (out0 | out1 << 32 | out2 << 64 | out3 << 96) mod q_l: bconv_reduce takes any 128-bit value; the bias is below
 *                 2^-67; the limbs are independent through the tag
 */
#pragma once
#include "ntt_lift.h"

namespace ntt {

constexpr int kSampleLimbs = kLiftLimbs; /* limbs of one launch (= kMaxLimbs) */

enum SampleKind : uint32_t { kSampleTernary = 0, kSampleCbd21 = 1, kSampleUniform = 2 };

/* limb l: BconvDst with q, bar, mu as bconv_dst forms them and [mult]_q in s (s_shoup its Shoup word); h is not used */
using SampleLimb = BconvDst;

/* what the limbs share: the kind, the key, the first polynomial's number, and the index in the call's plans array of limb 0 of the launch */
struct SampleCall {
  uint32_t kind, accumulate;
  uint32_t key0, key1;
  uint64_t first_poly;
  uint32_t limb0, pad_;
};

struct SampleBlock {
  uint32_t w[4];
};

constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u; /* on word 0, on word 2 */
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u; /* the key increments   */

/* Philox4x32-10: ten rounds (c0, c1, c2, c3) -> (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)), the key bumped
 * between rounds */
NTT_HD SampleBlock philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
#pragma unroll
  for(int r = 0; r < 10; r++) {
    const uint64_t p0 = (uint64_t)kPhiloxM0 * c0, p1 = (uint64_t)kPhiloxM1 * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1                = (uint32_t)p1;
    c3                = (uint32_t)p0;
    c0                = n0;
    c2                = n2;
    k0 += kPhiloxW0;
    k1 += kPhiloxW1;
  }
  return SampleBlock{{c0, c1, c2, c3}};
}

/* the tag of limb l (its index in the call's plans array) */
NTT_HD uint32_t sample_tag(uint32_t kind, uint32_t l) { return kind == kSampleUniform ? (2u | (l << 8)) : kind; }

/* the block of coefficient s of polynomial P */
NTT_HD SampleBlock sample_block(const SampleCall &c, uint64_t P, uint32_t s, uint32_t tag)
{
  return philox4x32_10(s, (uint32_t)P, (uint32_t)(P >> 32), tag, c.key0, c.key1);
}

NTT_HD int sample_popcount21(uint32_t x)
{
#if defined(__HIP_DEVICE_COMPILE__)
  return __popc(x & 0x1FFFFFu);
#else
  return __builtin_popcount(x & 0x1FFFFFu);
#endif
}

/* the centred value of a small kind */
NTT_HD int sample_small(uint32_t kind, const SampleBlock &b)
{
  if(kind == kSampleCbd21) return sample_popcount21(b.w[0]) - sample_popcount21(b.w[1]);
  return (int)mulhi64((uint64_t)b.w[0] | ((uint64_t)b.w[1] << 32), 3) - 1;
}

/* [mult v]_q for |v| <= 21: Shoup's product of |v| with [mult]_q (any word times s lands in [0, 2q)), negated for v < 0 */
NTT_HD uint64_t sample_small_digit(int v, const SampleLimb &l)
{
  const uint64_t a = (uint64_t)(v < 0 ? -v : v);
  uint64_t       z = a * l.s - mulhi64(a, l.s_shoup) * l.q;
  z                = z >= l.q ? z - l.q : z;
  return v < 0 && z ? l.q - z : z;
}

/* the 128-bit block mod q */
NTT_HD uint64_t sample_uniform_digit(const SampleBlock &b, const SampleLimb &l)
{
  const uint64_t v = bconv_reduce((uint64_t)b.w[2] | ((uint64_t)b.w[3] << 32), (uint64_t)b.w[0] | ((uint64_t)b.w[1] << 32), l);
  return v >= l.q ? v - l.q : v;
}

/* one output word: limb li of the launch (li + limb0 of the call), position s of polynomial P */
NTT_HD uint64_t sample_digit(const SampleCall &c, uint64_t P, uint32_t s, uint32_t li, const SampleLimb &l)
{
  if(c.kind == kSampleUniform) return sample_uniform_digit(sample_block(c, P, s, sample_tag(c.kind, c.limb0 + li)), l);
  return sample_small_digit(sample_small(c.kind, sample_block(c, P, s, c.kind)), l);
}

/* coefficients: c_l (+)= the sample for up to kSampleLimbs limbs, nothing read (sample_coef_kernel; sample.hip) */
using SampleCoefArgs = ProduceArgs<SampleCall>;
hipError_t launch_sample_coef(const SampleCoefArgs &sa);

/* NTT domain, FP64 policies, N = 2^6..2^14: c_l^ (+)= fwd(the sample) in ONE launch over a run of limbs (sample_fwd_kernel;
 * sample_f64*.hip) */
using SampleFwdArgs = ProduceArgs<SampleCall>;
template <class A, int KSH> hipError_t launch_sample_fwd(const SampleFwdArgs &sa);
template <> hipError_t launch_sample_fwd<ArithF64, 0>(const SampleFwdArgs &);
template <> hipError_t launch_sample_fwd<ArithF64, 1>(const SampleFwdArgs &);
template <> hipError_t launch_sample_fwd<ArithF64, 18>(const SampleFwdArgs &);
template <> hipError_t launch_sample_fwd<ArithF64W, 0>(const SampleFwdArgs &);

} // namespace ntt
