/*
 * ntt_ct_mul.h -- launchers of the kernels that open and close a homomorphic multiplication on NTT-domain ciphertexts
 * (ntt_rns_tensor_batch, ntt_rns_mod_down_add_batch): the host layer's view of them.
 *
 * The kernel template lives in ntt_kernels_ksfold.h (ksfold_fwd_kernel, instantiated in ksfold_f64*.hip), the two element-wise
 * kernels in ct_elem.hip (tensor_kernel, ct_fold_kernel); this header declares the argument records and the launchers, nothing that
 * the host translation unit would instantiate.  The integer arithmetic is ntt_keyswitch.h's (bconv_mac, bconv_reduce).
 */
#pragma once
#include "ntt_keyswitch.h"

namespace ntt {

constexpr int kCtLimbs = 16; /* limbs of one element-wise launch (blockIdx.y; the records sit in the kernel arguments) */

/* the ciphertext tensor product, element-wise: c0 = a0 b0, c1 = a0 b1 + a1 b0, c2 = a1 b1 mod q_l for up to 16 limbs
 * (tensor_kernel; ct_elem.hip).  square: b_j is a_j, every input word is loaded once. */
struct TensorArgs {
  uint64_t *      c[3];
  const uint64_t *a[2];
  const uint64_t *b[2];
  bool            square;
  uint64_t        limb_stride, poly_stride, batch;
  uint32_t        logn;
  int             nlimbs;
  BconvDst        ql[kCtLimbs];
  int             max_grid;
  hipStream_t     stream;
};
hipError_t launch_tensor(const TensorArgs &ta);

/* c_l (+)= a_l mod q_l for up to 16 limbs, each operand in a layout of its own (ct_fold_kernel; ct_elem.hip): the second half of
 * ntt_rns_mod_down_add_batch's composition route.  Canonical words in and out. */
struct CtFoldArgs {
  uint64_t *      c;
  const uint64_t *a;
  uint64_t        c_limb_stride, c_poly_stride, a_limb_stride, a_poly_stride, batch;
  uint32_t        logn;
  int             nlimbs;
  bool            accumulate;
  uint64_t        q[kCtLimbs];
  int             max_grid;
  hipStream_t     stream;
};
hipError_t launch_ct_fold(const CtFoldArgs &fa);

/* ModDown into a ciphertext, NTT domain, FP64 policies, N = 2^6..2^14: out_l^ (+)= (c_l^ - fwd(u_l)) * P^-1 in ONE launch over a run
 * of Q limbs (ksfold_fwd_kernel; ksfold_f64*.hip).  m is moddown_fwd_kernel's record: m.c (the accumulator's Q limbs) is only read. */
struct KsFoldArgs {
  ModDownFwdArgs m;
  uint64_t *     out; /* the run's first limb of the ciphertext */
  uint64_t       out_limb_stride, out_poly_stride;
  bool           accumulate;
};
template <class A, int KSH> hipError_t launch_ksfold_fwd(const KsFoldArgs &ka);
template <> hipError_t launch_ksfold_fwd<ArithF64, 0>(const KsFoldArgs &);
template <> hipError_t launch_ksfold_fwd<ArithF64, 1>(const KsFoldArgs &);
template <> hipError_t launch_ksfold_fwd<ArithF64, 18>(const KsFoldArgs &);
template <> hipError_t launch_ksfold_fwd<ArithF64W, 0>(const KsFoldArgs &);

} // namespace ntt
