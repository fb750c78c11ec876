/*
 * ntt_mi355x.h -- batched, device-resident negacyclic NTT engine for MI355X (gfx950).
 *
 * This is the throughput API of libntt_mi355x.so.  The reference package
 * (IBM/optimized-number-theoretic-transform-implementations) has no batch API:
 * its only precedent is the two-polynomial fwd_ntt_ref_harvey_lazy_dbl
 * (reference include/ntt_reference.h:44-49, src/ntt_reference.c:71-91).  The
 * functions below generalise that to `batch` independent polynomials that stay
 * in HBM, with exactly the reference's transform semantics, so results compare
 * element-for-element with
 *
 *   fwd_ntt_ref_harvey / fwd_ntt_radix4      (include/ntt_reference.h:19-31,
 *                                             include/ntt_radix4.h:16-28)
 *   inv_ntt_ref_harvey / inv_ntt_radix4      (src/ntt_reference.c:33-66,
 *                                             src/ntt_radix4.c:64-114)
 *
 * i.e. forward: natural order in -> bit-reversed order out, values in [0,q);
 * inverse: bit-reversed in -> natural out, scaled by N^-1, values in [0,q).
 * The single-polynomial reference signatures themselves are exported by the same
 * library (include/ntt_reference.h, ntt_radix4.h, ntt_radix4x4.h, ntt_seal.h).
 *
 * Plain C ABI: pointers and sizes only.  `stream` arguments are hipStream_t
 * passed as void* (NULL = the device's default stream).  All functions return
 * NTT_OK (0) or a negative ntt_status; ntt_last_error() describes the failure.
 * There is no CPU fallback: without a HIP device every compute entry point
 * fails with NTT_ERR_NO_DEVICE.
 */
#ifndef NTT_MI355X_H
#define NTT_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#  define NTT_API __attribute__((visibility("default")))
#else
#  define NTT_API
#endif

typedef enum ntt_status {
  NTT_OK              = 0,
  NTT_ERR_ARG         = -1, /* bad argument (N not a power of two, q not NTT-friendly ...) */
  NTT_ERR_NO_DEVICE   = -2, /* no HIP device / HIP runtime unusable                        */
  NTT_ERR_HIP         = -3, /* a HIP call failed; see ntt_last_error()                     */
  NTT_ERR_UNSUPPORTED = -4, /* e.g. FP64 arithmetic requested for q > 2^51                 */
  NTT_ERR_NOMEM       = -5
} ntt_status;

typedef enum ntt_arith {
  NTT_ARITH_AUTO = 0, /* FP64 path when q allows it (q < 2^52), else 64-bit integer Shoup in its throughput form
                       * (NTT_OPT_INT_WIDE) */
  NTT_ARITH_U64  = 1, /* reference-identical Harvey/Shoup lazy arithmetic, any q<2^61 */
  NTT_ARITH_F64  = 2, /* balanced FP64 arithmetic: q <= 2^51(1+2^-10) with a compile-time reduction schedule,
                       * up to q < 2^52 with both operands of every butterfly reduced (info[4] == 52)  */
  NTT_ARITH_U64_R4 = 3 /* the reference's radix-4 butterflies with the shared-quotient double
                        * product (include/internal/fast_mul_operators.h:62-70,108-149) on the 2N-entry
                        * expanded table (src/ntt_radix4.c:7-114); q < 2^60; 2^6..2^18 (two passes above 2^14).
                        * Never chosen by AUTO. */
} ntt_arith;

typedef enum ntt_option {
  NTT_OPT_MAX_GRID  = 1, /* cap on workgroups per launch (0 = the kernels' own choice)             */
  NTT_OPT_CHUNK_MIB = 2, /* bytes of one chunk of a multi-pass transform, MiB (default 256)        */
  NTT_OPT_F64_CLASS = 3, /* force a coarser FP64 headroom class (0, 1 or 18) than q permits: tests  */
  NTT_OPT_TWO_PHASE = 4, /* N = 2^16, 2^17 (FP64): 1 = both passes of a polynomial in one workgroup (one launch),
                          * 0 = one launch per pass over the whole batch, -1 (default) = the faster of the two as
                          * measured: one launch for the forward transform at 2^16, per pass elsewhere */
  NTT_OPT_BLOCK_LOG = 6, /* N = 2^15, 2^16: log2 of the blocks the fused pass works on below the column pass: 12
                          * (3 or 4 column stages), 14 (1 or 2), 0 (default) = the faster one as measured.  Results
                          * are identical. */
  NTT_OPT_XCD_LOCAL = 7,  /* N = 2^15..2^17 (FP64 policies; wide integer policy): 1 = both passes of a transform as items of ONE launch, every polynomial
                           * handled by the workgroups of one XCD, the intermediate handed over inside that XCD (MEASURED
                           * fabric traffic per transform, FETCH x2 + WRITE counters: 24N bytes at 2^15, where the L2 retains
                           * the intermediate at the shipped lag; 32N at 2^16 and 2^17, where it does not and the second pass is
                           * served by the Infinity Cache -- the gain there is one launch instead of two per chunk);
                           * 0 = one launch per pass; -1 (default) = where it measured faster: forward transforms of 512
                           * polynomials or more (wide integer policy: +18..23 %, where the memory-bound column items overlap the
                           * multiplier-bound row items; also its inverse at 2^17).  The NTT-domain products (ntt_inv_product_batch,
                           * ntt_inv_dot_batch, their RNS forms) follow the same switch: 1 = the k products with the inverse's block
                           * stages and the inverse's column stages as the items of one launch, 0 = two launches per 128 / 256 MiB
                           * chunk, -1 = one launch from 2^25 coefficients per operand on (measured +11..26 %,
                           * profiles/r05/domain_bench_xcd_local.txt); so does ntt_fwd_mul_batch (the forward column stages of a and
                           * the blocks with the product as one launch: +8..28 %, automatic from 2^26 coefficients on).  Results are
                           * identical. */
  NTT_OPT_XCD_LOCAL_LAG = 8,        /* tuning: polynomials between the two passes of a queue (0 = default: transforms 10, 8, 10 at 2^15,
                                     * 2^16, 2^17; NTT-domain products 20-24, 10-14, 6-8 -- about 5-6 MiB of c per queue) */
  NTT_OPT_XCD_LOCAL_WGS_PER_CU = 9, /* tuning: resident workgroups per CU, 1..4 (0 = default 4) */
  NTT_OPT_INT_WIDE = 10, /* integer policy, 2^40 <= q < 2^61: 1 = transforms through the throughput form of the integer
                          * arithmetic (estimated Shoup quotient, no conditional subtraction per butterfly: the bits between q
                          * and 2^64 absorb the growth; 19 instead of 28 instructions per butterfly, +16 % measured) -- same
                          * tables, same canonical results, lazy outputs inside the same ranges but NOT the reference's lazy
                          * words; 0 = the reference's Harvey butterflies.  Default: 1 for NTT_ARITH_AUTO plans (q >= 2^52),
                          * 0 for plans created with NTT_ARITH_U64.  10 + K forces headroom class K in {0, 1, 3} (tests) */
  NTT_OPT_RNS_LAUNCH = 12, /* ntt_rns_*: how a run of compatible limbs is launched -- 0 = ONE launch (per pass) over the run wherever
                          * the kernels have the variant, 1 = one launch chain per limb, -1 (default) = one launch where a limb's share
                          * alone cannot fill the chip and for the XCD-local launches.  Read from the run's first plan; results are
                          * identical (tests, measurements) */
  NTT_OPT_DOT_FUSED = 13, /* NTT-domain products (ntt_inv_dot_batch, ntt_fwd_mul_batch, ...): 1 (default) = the products inside the
                          * transform's first / last pass; 0 = pointwise(-accumulate) launches around a plain transform (measurements) */
  NTT_OPT_MAX_BATCH_HINT = 14, /* polynomials x limbs of the largest batched call the plan will serve: the control blocks of the
                          * XCD-local launches (N >= 2^15) are sized for it -- for the null stream at once, for any other stream at its
                          * first call or by ntt_plan_reserve -- so that no later call allocates (an allocation synchronises the device).
                          * 0 (default): sized by the first call, doubled when outgrown */
  NTT_OPT_CTL_ALLOCATIONS = 15, /* READ-ONLY (ntt_plan_get_option): device allocations the plan has made for its control blocks so far --
                          * unchanged across a call = that call did not allocate (what ntt_plan_reserve promises) */
  NTT_OPT_BLOCK_OVERSUB = 11, /* persistent block kernels: workgroups launched per resident slot (0 = default: 8 for the 2^12-point
                          * block kernels, whose four workgroups per CU otherwise run in phase -- measured +5 % forward, +4 % inverse,
                          * profiles/r05/grid_sweep.txt --, 1 elsewhere: 2^13 and 2^14 measured no gain) */
  NTT_OPT_ONE_PASS = 16, /* N = 2^15, FP64 policies (q < 2^52): 1 = the transform in ONE pass over the data -- a 1024-thread workgroup holds
                          * the whole polynomial (32 words per thread) in its registers, the stage on pairs 2^14 apart runs thread-locally
                          * and the two halves go through the 2^14-point block stages one after the other: 16N bytes cross HBM, where the
                          * two-pass forms move 24N..32N across the fabric (measured forward 0.43 -> see profiles/r06/onepass_2p15.txt);
                          * 0 = the two-pass forms (XCD-local launch / per-pass launches); -1 (default) = one pass when the batch gives
                          * every second CU a polynomial (measured crossover: 64..96 polynomials) and neither NTT_OPT_XCD_LOCAL 1 nor
                          * NTT_OPT_BLOCK_LOG is set (explicit options win).  Calls that ask for lazy outputs get canonical words from it
                          * (inside the lazy ranges).  Results are identical. */
  NTT_OPT_RESCALE_FUSED = 17, /* ntt_rns_rescale_batch in the NTT domain: 1 (default) = one forward-transform launch per run of
                          * kept limbs with the rescale in its prologue and epilogue where it is built (FP64 policies, N = 2^6..2^14);
                          * 0 = inverse, element-wise kernel and forward transform around every run.  Read from plans[0]; results
                          * are identical.  The same switch selects the route of ntt_rns_mod_down_batch in the NTT domain */
  NTT_OPT_MODUP_FUSED = 18, /* ntt_rns_mod_up_mul_batch: 1 = every run of limbs the fused kernel is built for (FP64 policies,
                          * N = 2^6..2^14) takes it: one forward-transform launch with ModUp in its prologue and the key product in
                          * its epilogue; 0 = every run takes the composition (the base-conversion launches into the operand's other
                          * slots, then the ntt_rns_fwd_mul_batch route); -1 (default) = the fused kernel where the recorded
                          * measurement says it is not slower (the rule is quoted at ntt_rns_mod_up_mul_batch).  Read from plans[0];
                          * results are identical */
  NTT_OPT_PAIR_FUSED = 19, /* ntt_rns_fwd_mul_pair_batch, ntt_rns_mod_up_mul_pair_batch: 1 = every run of limbs the fused pair kernel is built
                          * for (FP64 policies, N = 2^6..2^14) takes it: one forward-transform launch whose epilogue multiplies by both
                          * key components; 0 = every run takes the composition (base-conversion launches, ONE forward transform in
                          * place, one two-output element-wise product); -1 (default) = the fused kernel where the recorded
                          * measurement says it is not slower (the rule is quoted at ntt_rns_mod_up_mul_pair_batch).  Read from
                          * plans[0]; results are identical */
  NTT_OPT_MODDOWN_ADD_FUSED = 20, /* ntt_rns_mod_down_add_batch in the NTT domain: 1 = every run of Q limbs the fused kernel is built for
                          * (FP64 policies, N = 2^6..2^14) takes it: one forward-transform launch with the base conversion in its
                          * prologue, whose epilogue reads the accumulator and stores into the ciphertext; 0 = every run takes the
                          * composition (ntt_rns_mod_down_batch's route in place on the accumulator, then one element-wise launch per
                          * 16 limbs; NTT_OPT_RESCALE_FUSED keeps selecting that route); -1 (default) = the fused kernel where the
                          * recorded measurement says it is not slower (the rule is quoted at ntt_rns_mod_down_add_batch).  Read from
                          * plans[0]; results are identical */
  NTT_OPT_BGV_FUSED = 21, /* ntt_rns_mod_down_bgv_batch, ntt_rns_mod_down_bgv_add_batch in the NTT domain: 1 = every run of Q limbs the
                          * fused kernel is built for (FP64 policies, N = 2^6..2^14) takes it, at any np <= 16: one forward-transform
                          * launch with the BGV conversion in its prologue; 0 = every run takes the sandwich (inverse, the coefficient
                          * launch, forward; the add form then one element-wise launch per 16 limbs); -1 (default) = the fused kernel
                          * where the recorded measurement says it is not slower (the rule is quoted at ntt_rns_mod_down_bgv_batch).
                          * Read from plans[0]; results are identical.  NTT_OPT_RESCALE_FUSED and NTT_OPT_MODDOWN_ADD_FUSED keep their
                          * meaning for the other calls; the BGV calls do not read them */
  NTT_OPT_LIFT_FUSED = 22, /* ntt_rns_from_plain_batch, ntt_rns_from_double_batch with NTT_LIFT_TRANSFORMED: 1 = every run of limbs the
                          * fused kernel is built for (FP64 policies, N = 2^6..2^14) takes it: one forward-transform launch with the
                          * lift in its prologue; 0 = every run takes the composition (the element-wise launch, then the forward
                          * transform; accumulating, the inverse transform first); -1 (default) = the rule quoted at
                          * ntt_rns_from_plain_batch.  Read from plans[0]; results are identical */
  NTT_OPT_SLOTS_FUSED = 23, /* ntt_slots_encode_batch, ntt_slots_decode_batch: 1 = the fused kernels wherever they are built (FP64
                          * policies, N = 2^6..2^14): ONE launch, the slot permutation applied by the transform's own loads / stores;
                          * 0 = the composition everywhere (the element-wise permutation launch and the plan's transform in place);
                          * -1 (default) = the rule quoted at ntt_slots_encode_batch.  Results are identical */
  NTT_OPT_SAMPLE_FUSED = 24, /* ntt_rns_sample_batch with NTT_SAMPLE_TRANSFORMED: 1 = every run of limbs the fused kernel is built for (FP64
                          * policies, N = 2^6..2^14) takes it: one forward-transform launch with the generator in its prologue; 0 = every
                          * run takes the composition (the element-wise launch, then the forward transform; accumulating, the inverse
                          * transform first); -1 (default) = the rule quoted at ntt_rns_sample_batch.  Read from plans[0]; results are
                          * identical */
  NTT_OPT_FUSED_PRODUCT = 5 /* N = 2^8..2^17, FP64: 1 (default) = ntt_negacyclic_mul_batch as ONE launch that takes both
                          * operands through the forward stages, multiplies in registers and runs the inverse: 24N bytes up to
                          * 2^14; from 2^23 coefficients per operand of N >= 2^15 on likewise one launch (all limbs of an RNS set
                          * included), whose MEASURED fabric traffic is about 85N bytes per product at 2^17 (a, b, two of the
                          * three intermediates and the twiddles: the L2 retains nothing at that size) against 56N algorithmic;
                          * smaller batches of N >= 2^15: block by block between the column passes of both operands, 72N
                          * bytes); 2 = a's forward transform always as a launch of its own in front of the fused
                          * fwd(b)*a^ -> inverse kernel (40N bytes up to 2^14); 0 = fwd, fwd, then the products inside the inverse's
                          * first pass (three launches, 56N bytes up to 2^14: what plans of the integer policies and squarings
                          * always take).  Results are identical. */
} ntt_option;

typedef struct ntt_plan ntt_plan; /* opaque: tables for one (device, N, q, root) */

/* ---- library / device ---- */
NTT_API const char *ntt_last_error(void);
NTT_API int         ntt_device_count(void);             /* <0: ntt_status */
NTT_API const char *ntt_version(void);

/* ---- plans ----
 * root must be a primitive 2N-th root of unity mod q (the `w` column of
 * reference tests/test_cases.h:145-208).  The plan derives every table itself
 * with the reference's layouts (include/internal/pre_compute.h:38-105) -- ON THE DEVICE: the host squares the
 * root log2 N times, one GPU thread produces each table entry. */
NTT_API int  ntt_plan_create(ntt_plan **out, int device, uint64_t N, uint64_t q,
                             uint64_t root, int arith);
/* build from caller tables in the reference's radix-2 layout: w_powers[k] =
 * root^bitrev(k), N entries each; w_inv_powers may be NULL (forward-only plan) */
NTT_API int  ntt_plan_create_from_tables(ntt_plan **out, int device, uint64_t N, uint64_t q,
                                         const uint64_t *w_powers,
                                         const uint64_t *w_inv_powers, int arith);
NTT_API void ntt_plan_destroy(ntt_plan *p);
/* info[0..7] = {N, q, log2N, arith actually used, FP64 headroom class,
 *               number of HBM passes, device, root (0 if built from tables)} */
NTT_API int  ntt_plan_info(const ntt_plan *p, uint64_t info[8]);
/* copy a device table back (tests / debugging): which = 0 forward records, 1 inverse records (+16 folded N^-1 records),
 * 2 / 3 the FP64 policy's compact forward / inverse tables.  Records are 16 bytes: {w, floor(w 2^64/q)} as two
 * uint64_t (integer policies; 2N records of the expanded table for NTT_ARITH_U64_R4) or {balanced w, w/q} as two
 * doubles (FP64).  which = 4 / 5: the slot tables pos / ipos (after ntt_plan_enable_slots), N uint32_t each. */
NTT_API int  ntt_plan_export_table(const ntt_plan *p, int which, void *h_dst, size_t bytes);
/* force the strided multi-pass path (self-check of the fused kernels) */
NTT_API int  ntt_plan_set_generic(ntt_plan *p, int on);
/* tuning / test knobs of one plan (ntt_option).  The batched API reads NO environment variable; the reference-signature entry points
 * (which have no argument to carry a choice) read NTT_DEVICE, NTT_COMPAT_ARITH and NTT_COMPAT_ZERO_COPY (0 = stage single-pass
 * transforms through device memory instead of running them on a pinned, device-mapped host buffer) once, at their first call. */
NTT_API int  ntt_plan_set_option(ntt_plan *p, int option, int64_t value);
NTT_API int  ntt_plan_get_option(const ntt_plan *p, int option, int64_t *value); /* the value in force (0 / -1 = the default, as set) */
/* Allocates the control blocks (queue heads + one counter per polynomial, 4 bytes each; the direct one and the one captured
 * launches use) the XCD-local launches of this plan need on `stream` for batches of up to `polys` polynomials x limbs.  The
 * batched entry points take a const plan; these blocks are the one thing they may create or grow (under the plan's mutex), and
 * after this call they do not.  Call it outside stream capture. */
NTT_API int  ntt_plan_reserve(const ntt_plan *p, void *stream, uint64_t polys);

/* ---- batched transforms: d_a is device memory laid out [batch][N], in place ----
 * Input contract: ntt_fwd_batch / ntt_inv_batch (and every entry point that does not say otherwise) take CANONICAL words, 0 <= a < q.
 * The library does not check it, and plans for 2^51 < q < 2^52 (info[4] == 52) rely on it: the first inverse stage multiplies the
 * unreduced difference of two inputs, exact only while that difference is below q in magnitude -- words in [q, 2q) handed to
 * ntt_inv_batch give wrong results there (rounds 3-4 happened to tolerate them).  Lazy words of any range this header names go
 * through the *_wide entry points (NTT_FLAG_WIDE_IN), which fold them first. */
NTT_API int ntt_fwd_batch(const ntt_plan *p, uint64_t *d_a, uint64_t batch, void *stream);
NTT_API int ntt_inv_batch(const ntt_plan *p, uint64_t *d_a, uint64_t batch, void *stream);
/* lazy outputs: the reference's *_lazy contract (include/ntt_reference.h:13-17, tests/bench.c:123-137) --
 * the final reduction is left to the consumer.  Forward: values in [0,4q) (radix-4 policy: [0,8q), bit-identical
 * to fwd_ntt_radix4_lazy); inverse: [0,2q).  Feed them to the *_wide entry points, to
 * ntt_pointwise_mul_batch... after reduce_*_to_q, or to the fused product below.  A policy that has no
 * cheaper lazy form for a direction (FP64 inverse) returns reduced values, which satisfy the contract. */
NTT_API int ntt_fwd_batch_lazy(const ntt_plan *p, uint64_t *d_a, uint64_t batch, void *stream);
NTT_API int ntt_inv_batch_lazy(const ntt_plan *p, uint64_t *d_a, uint64_t batch, void *stream);
/* every combination in one call: flags = NTT_FLAG_* or'ed together */
enum { NTT_FLAG_INVERSE = 1, NTT_FLAG_WIDE_IN = 2, NTT_FLAG_LAZY_OUT = 4 };
NTT_API int ntt_transform_batch(const ntt_plan *p, uint64_t *d_a, uint64_t batch, unsigned flags, void *stream);
/* same as ntt_fwd_batch / ntt_inv_batch, but inputs may be lazy values in [0,8q) (what the reference's *_lazy
 * entry points accept and emit); outputs are still in [0,q) */
NTT_API int ntt_fwd_batch_wide(const ntt_plan *p, uint64_t *d_a, uint64_t batch, void *stream);
NTT_API int ntt_inv_batch_wide(const ntt_plan *p, uint64_t *d_a, uint64_t batch, void *stream);

/* ---- callers either side of the path ---- */
/* d_c[i] = d_a[i]*d_b[i] mod q over n = batch*N values in [0,q); c may alias a or b */
NTT_API int ntt_pointwise_mul_batch(const ntt_plan *p, uint64_t *d_c, const uint64_t *d_a,
                                    const uint64_t *d_b, uint64_t batch, void *stream);
/* the same with LAZY operands in [0,4q) (ntt_fwd_batch_lazy outputs); the product is fully reduced */
NTT_API int ntt_pointwise_mul_batch_lazy(const ntt_plan *p, uint64_t *d_c, const uint64_t *d_a,
                                         const uint64_t *d_b, uint64_t batch, void *stream);
/* c = a*b in Z_q[X]/(X^N+1) for every polynomial of the batch:
 * ONE launch (FP64 policies, NTT_OPT_FUSED_PRODUCT), else fwd(a), fwd(b) and the products inside the inverse transform's first
 * pass -- the chain stays in the lazy domain until the inverse's output.
 * d_a is overwritten (left in the NTT domain as LAZY values in [0,4q), congruent to the reference's
 * transform -- or, large batches of N >= 2^15, holding only the column stages of it -- or, the one-launch form up to
 * 2^14, not written at all); d_b is overwritten likewise
 * (three-launch chain), overwritten by the column passes of its forward transform
 * (fused product, N = 2^15 .. 2^17) or left as it was (fused product, N = 2^8 .. 2^14); callers must not rely on any of these.  Aliasing rules: d_c may alias d_a or d_b; d_a == d_b computes the square
 * a*a (the shared operand is transformed once); any other overlap is undefined.
 * NTT_ARITH_U64_R4 plans run the reference's radix-4 formulation end to end (fwd_ntt_radix4 on both operands, the
 * pointwise product, inv_ntt_radix4): d_a and d_b are left canonical there. */
NTT_API int ntt_negacyclic_mul_batch(const ntt_plan *p, uint64_t *d_c, uint64_t *d_a,
                                     uint64_t *d_b, uint64_t batch, void *stream);

/* ---- operands that already ARE in the NTT domain ("fusing the multiply into the inverse's first load
 * saves 16N bytes").  Keys, plaintexts and ciphertexts of an FHE caller live in the NTT domain (bit-reversed order, as
 * ntt_fwd_batch leaves them); what such a caller issues is the element-wise product of two transformed operands, or the
 * inner product of a digit-decomposed ciphertext with a key, followed by ONE inverse transform.  The reference's
 * primitive for it is fast_mul_mod_q (include/internal/fast_mul_operators.h:56-60) in a loop of its own in front of
 * inv_ntt_*; here the products are formed inside the inverse transform's first pass, so neither the product nor the sum
 * ever exists in memory.
 *   flags: NTT_MUL_LAZY_IN      transformed operand words may be LAZY -- anywhere in [0,4q) (ntt_fwd_batch_lazy outputs, the
 *                               reference's *_lazy range, include/ntt_reference.h:13-17) -- instead of canonical
 *                               ([0,q)); ntt_mul_transformed_batch additionally needs them below 2^53
 *          NTT_MUL_B_BROADCAST  every d_bhat[i] is ONE polynomial (N words; RNS: [limb][N]) shared by all polynomials of
 *                               the batch: a key.  Traffic 8kN + 8N instead of 16kN + 8N bytes per output polynomial.
 * Outputs are canonical coefficients in natural order, exactly inv_ntt_ref_harvey(pointwise products) of the reference. */
enum { NTT_MUL_LAZY_IN = 1, NTT_MUL_B_BROADCAST = 2,
       NTT_MUL_ACCUMULATE = 4 /* ntt_fwd_mul_batch: c^ += ... instead of c^ = ... (c^ canonical on entry) */ };
/* c = inv( a^ (.) b^ ): ONE launch up to N = 2^14 (24N bytes instead of 40N for pointwise + inverse); above, the product
 * rides in the first pass of the inverse (40N instead of 56N).  d_c may alias d_ahat or d_bhat (not a broadcast b^). */
NTT_API int ntt_inv_product_batch(const ntt_plan *p, uint64_t *d_c, const uint64_t *d_ahat, const uint64_t *d_bhat,
                                  uint64_t batch, unsigned flags, void *stream);
/* c = inv( sum_{i<k} a_i^ (.) b_i^ ), 1 <= k <= 32 (key switching: digits x key): d_ahat / d_bhat are HOST arrays of k
 * device pointers, each operand laid out [batch][N].  Reads 16kN bytes (8kN with a broadcast key), writes 8N, one
 * inverse transform.  For k > 1 d_c must not overlap any operand. */
NTT_API int ntt_inv_dot_batch(const ntt_plan *p, uint64_t *d_c, int k, const uint64_t *const *d_ahat,
                              const uint64_t *const *d_bhat, uint64_t batch, unsigned flags, void *stream);
/* c = inv( fwd(a) (.) b^ ): a in coefficients, b^ transformed beforehand (a plaintext or key kept in the NTT domain).  One
 * launch that takes a through the forward stages, multiplies by b^ in registers and runs the inverse (24N bytes up to
 * 2^14).  d_a is left as it was up to N = 2^14 and OVERWRITTEN (scratch) above -- and at every size by plans the fused kernels
 * are not built for (integer and radix-4 policies, column-only plans: forward transform in place, pointwise, inverse): treat
 * it as scratch unless you know the plan.  d_c may alias d_a or d_bhat. */
NTT_API int ntt_mul_transformed_batch(const ntt_plan *p, uint64_t *d_c, uint64_t *d_a, const uint64_t *d_bhat, uint64_t batch,
                                      unsigned flags, void *stream);
/* c^ = fwd(a) (.) b^, or with NTT_MUL_ACCUMULATE c^ += fwd(a) (.) b^: a in coefficients, the result STAYS in the NTT domain
 * (canonical words, bit-reversed order as ntt_fwd_batch leaves them): a plaintext or key-switching key kept transformed is
 * multiplied in where the forward transform would reduce and store its outputs -- the multiply-accumulate of a key-switching
 * inner product, digit by digit.  ONE launch up to N = 2^14: 24N bytes (16N with NTT_MUL_B_BROADCAST) instead of 40N for
 * ntt_fwd_batch + ntt_pointwise_mul_batch; accumulating 32N (24N) instead of 48N.  N = 2^15 (FP64 policies, NTT_OPT_ONE_PASS): the
 * one-pass transform with the product at its output, 24N bytes, d_a left as it was (round 6).  Else above 2^14 the product rides in
 * the block pass of the forward transform: one launch over both passes from 2^26 coefficients per operand on (NTT_OPT_XCD_LOCAL), else a column and a
 * block launch per 256 MiB chunk.  d_a is left as it was up to 2^14 and
 * OVERWRITTEN (scratch) above -- and at every size by plans without the fused kernel (radix-4 policy, column-only plans, N <
 * 2^6: forward transform in place, then a pointwise launch); d_c may alias d_a (not when accumulating) or d_bhat. */
NTT_API int ntt_fwd_mul_batch(const ntt_plan *p, uint64_t *d_c, uint64_t *d_a, const uint64_t *d_bhat, uint64_t batch, unsigned flags,
                              void *stream);

/* ---- RNS limbs (BASELINE config 5: 4-prime RNS pipeline).  plans[l] is the plan of
 * prime q_l (same N, same device); data layout is [limb][batch][N], i.e. limb l of
 * every polynomial is the contiguous [batch][N] slab at d_x + l*batch*N.  Each limb is
 * an independent transform -- the reference has no counterpart; its closest
 * primitive is fast_mul_mod_q (include/internal/fast_mul_operators.h:56-60).
 * When one limb's share alone cannot fill the GPU (a ciphertext: a few polynomials x tens of primes) and the limbs'
 * plans agree in policy and options (the headroom class may differ: the launch takes the coarsest), ONE launch per pass serves up to 16 limbs: a
 * workgroup picks its limb's tables and constants from an array in the kernel arguments -- for the FP64 policies (q < 2^52)
 * and for the wide integer policy (NTT_ARITH_AUTO plans of 2^52 <= q < 2^61; a product of such a set is three launches:
 * both forward transforms and the products inside the inverse's first pass).  At N = 2^15..2^17 (FP64 policies) large per-limb
 * batches are ONE launch over the limbs too (the XCD-local kernels take the limb as part of their queue entries); other large
 * batches are served limb by limb.  A modulus chain with primes of several sizes (a 60-bit first prime in front of 50-bit
 * ones) is served as maximal RUNS of consecutive compatible limbs: one launch per pass and run, single limbs by themselves.
 * Results are identical either way (NTT_OPT_RNS_LAUNCH on the limbs' plans forces either form). ---- */
NTT_API int ntt_rns_fwd_batch(int nlimbs, ntt_plan *const *plans, uint64_t *d_a, uint64_t batch, void *stream);
NTT_API int ntt_rns_inv_batch(int nlimbs, ntt_plan *const *plans, uint64_t *d_a, uint64_t batch, void *stream);
NTT_API int ntt_rns_negacyclic_mul_batch(int nlimbs, ntt_plan *const *plans, uint64_t *d_c, uint64_t *d_a,
                                         uint64_t *d_b, uint64_t batch, void *stream);
/* the NTT-domain products above over RNS limbs: every operand laid out [limb][batch][N] (a broadcast b^: [limb][N]) */
NTT_API int ntt_rns_inv_dot_batch(int nlimbs, ntt_plan *const *plans, uint64_t *d_c, int k, const uint64_t *const *d_ahat,
                                  const uint64_t *const *d_bhat, uint64_t batch, unsigned flags, void *stream);
NTT_API int ntt_rns_mul_transformed_batch(int nlimbs, ntt_plan *const *plans, uint64_t *d_c, uint64_t *d_a, const uint64_t *d_bhat,
                                          uint64_t batch, unsigned flags, void *stream);
NTT_API int ntt_rns_fwd_mul_batch(int nlimbs, ntt_plan *const *plans, uint64_t *d_c, uint64_t *d_a, const uint64_t *d_bhat,
                                  uint64_t batch, unsigned flags, void *stream);

/* ---- RNS rescale (modulus drop; the CKKS step after every multiplication).  An RNS polynomial of nlimbs = L+1 limbs with
 * primes q_0 .. q_L (plans[l], same N and device) holds x in [0, Q), Q = q_0 * ... * q_L.  After the call limbs 0 .. L-1 hold
 * y = round(x / q_L) mod Q / q_L (q_L is odd: no ties), or floor(x / q_L) with NTT_RESCALE_FLOOR, in the domain they came in;
 * for a centred x the result is the same modulo Q / q_L.  Limb l is (c_l - u_l) * q_L^-1 mod q_l with t = limb L's
 * coefficients and u_l = ((t + h) mod q_L) mod q_l - (h mod q_l), h = (q_L - 1) / 2 (floor: u_l = t mod q_l); in the NTT
 * domain c_l^ - fwd(u_l).  In place, canonical inputs and outputs, the layouts of the RNS forms ([limb][batch][N]; _strided:
 * any strides the forms above accept).  The dropped limb's slot: after an NTT_RESCALE_TRANSFORMED call it holds t (its
 * inverse transform), after a coefficient call it is unchanged.  Coefficients: one launch per 16 kept limbs, 8N(2L+1) bytes.
 * NTT domain: the inverse of limb L, then per run of compatible kept limbs one forward-transform launch that reduces t in its
 * prologue and subtracts and scales in its epilogue (FP64 policies, N = 2^6..2^14: 8N(2L+3) bytes in all, against 8N(6L+3)
 * for inverse + element-wise + forward), else that sandwich for the run (NTT_OPT_RESCALE_FUSED).  NTT_ERR_ARG, nothing
 * written: nlimbs < 2, plans that differ in N or device, q_L equal to a kept prime, overlapping strides, an unknown flag, a
 * missing table (the inverse of plans[L], the forward tables of the kept limbs, the inverse tables where the sandwich
 * serves).  Allocates nothing, does not synchronise the host, issues no memset: capturable. ---- */
enum { NTT_RESCALE_TRANSFORMED = 1, /* operands in the NTT domain (bit-reversed, as ntt_fwd_batch leaves them) */
       NTT_RESCALE_FLOOR       = 2  /* floor(x / q_L) instead of round(x / q_L) */ };
NTT_API int ntt_rns_rescale_batch(int nlimbs, ntt_plan *const *plans, uint64_t *d_a, uint64_t batch, unsigned flags,
                                  void *stream);
NTT_API int ntt_rns_rescale_batch_strided(int nlimbs, ntt_plan *const *plans, uint64_t *d_a, uint64_t limb_stride,
                                          uint64_t poly_stride, uint64_t batch, unsigned flags, void *stream);

/* ---- RNS base conversion for hybrid key switching (relinearisation, rotation): ModUp and ModDown.  A basis B = {b_i} with
 * product B, b^_i = B / b_i; fast base conversion (the HPS / BEHZ form, integer sums, bit-exact):
 *     FastBConv_{B->p}(x) = ( sum_i [x_i * b^_i^-1]_{b_i} * b^_i ) mod p,
 * which for x in [0, B) equals x + u B (mod p) for an integer 0 <= u < |B|.
 * ModUp: the operand is one RNS polynomial set over the extended basis Q u P, plans[0 .. nlimbs-1] (same N and device), in the
 * layouts of the RNS forms ([limb][batch][N]; _strided: any strides those accept).  Limbs [first, first + count), 1 <= count <= 16,
 * are the digit (the source basis B); afterwards every other limb l holds FastBConv_{B->q_l} of the digit, the digit's limbs are
 * unchanged.  Without NTT_MODUP_TRANSFORMED everything is in coefficients; with it everything comes and goes in the NTT domain:
 * the digit's limbs are inverse-transformed in place and converted, then every limb is forward-transformed (the digit's limbs
 * come back bit-identical: both transforms are exact bijections on canonical words).  In place on one operand because the
 * destination limbs of an FHE library's ciphertext ([batch][limb][N]) sit below the digit, above it and in P -- no regular
 * spacing.  Coefficients: one launch per 16 destination limbs, the digit read once per launch.
 * ModDown: plans[0 .. nq-1] are the Q primes, plans[nq .. nq+np-1] the P primes, 1 <= np <= 16; with t_j the coefficients of P limb
 * j and h = (P - 1) / 2 (0 with NTT_MODDOWN_FLOOR), Q limb l becomes ( c_l - FastBConv_{P->q_l}([t + h]_P) + [h]_{q_l} ) * P^-1 mod
 * q_l -- in the NTT domain the subtrahend is the forward transform of that coefficient vector.  For x in [0, QP) that is
 * round(x / P) - v (floor: floor(x / P) - v) mod Q with 0 <= v < np; with np = 1 it is exactly ntt_rns_rescale_batch with the same
 * flags.  The P slots follow the rescale: after a TRANSFORMED call they hold their coefficients, after a coefficient call they are
 * unchanged.  Coefficients: one launch per 16 Q limbs, the P limbs read once per launch (8N(2nq + np) bytes); NTT domain: the
 * inverse of the P limbs, then per run of compatible Q limbs one forward-transform launch that forms the subtrahend in its
 * prologue and subtracts and scales in its epilogue (FP64 policies, N = 2^6..2^14: 8N(2nq + 3np) bytes in all), else inverse,
 * element-wise kernel and forward transform for the run (NTT_OPT_RESCALE_FUSED on plans[0]).
 * All four: in place, canonical inputs and outputs.  NTT_ERR_ARG, nothing written: counts out of range, plans that differ in N or
 * device, a prime that appears twice among the operand's plans, an unknown flag, overlapping strides, a table the route needs
 * that a plan lacks.  Allocate nothing, do not synchronise the host, issue no memset: capturable. ---- */
enum { NTT_MODUP_TRANSFORMED = 1 /* the operand in the NTT domain (bit-reversed, as ntt_fwd_batch leaves it) */ };
enum { NTT_MODDOWN_TRANSFORMED = 1, NTT_MODDOWN_FLOOR = 2 }; /* the values of NTT_RESCALE_* on purpose */
NTT_API int ntt_rns_mod_up_batch(int nlimbs, ntt_plan *const *plans, uint64_t *d_a, int first, int count, uint64_t batch,
                                 unsigned flags, void *stream);
NTT_API int ntt_rns_mod_up_batch_strided(int nlimbs, ntt_plan *const *plans, uint64_t *d_a, int first, int count,
                                         uint64_t limb_stride, uint64_t poly_stride, uint64_t batch, unsigned flags, void *stream);
NTT_API int ntt_rns_mod_down_batch(int nq, int np, ntt_plan *const *plans, uint64_t *d_a, uint64_t batch, unsigned flags,
                                   void *stream);
NTT_API int ntt_rns_mod_down_batch_strided(int nq, int np, ntt_plan *const *plans, uint64_t *d_a, uint64_t limb_stride,
                                           uint64_t poly_stride, uint64_t batch, unsigned flags, void *stream);

/* ---- ModUp fused into the key product: one digit's term of the key-switching inner product in ONE call,
 *     c^ (+)= fwd( ModUp(digit) ) (.) key^   for every limb of Q u P.
 * d_ext is an operand over the extended basis as for ntt_rns_mod_up_batch: limbs [first, first + count), 1 <= count <= 16, hold the
 * digit's COEFFICIENTS, canonical.  Its other limb slots are scratch: the caller must treat them as undefined after the call.  Where
 * every run of limbs of the call is served by the fused kernel those slots are NOT WRITTEN AT ALL (nor read).  The digit's own limbs
 * follow ntt_rns_fwd_mul_batch's rule for d_a: left as they were up to N = 2^14, scratch above.  d_c and d_keyhat are NTT-domain
 * operands in the call's layout; flags are NTT_MUL_B_BROADCAST (the key is [limb][N]), NTT_MUL_ACCUMULATE and NTT_MUL_LAZY_IN (key
 * words), with ntt_rns_fwd_mul_batch's meaning.  The result is, bit for bit, ntt_rns_mod_up_batch(..., flags = 0) on d_ext followed
 * by ntt_rns_fwd_mul_batch(nlimbs, plans, d_c, d_ext, d_keyhat, batch, flags); outputs are canonical.
 * Per run of compatible limbs: FP64 policies at N = 2^6..2^14 -- one launch of the forward block kernel with the integer base
 * conversion in its prologue and the product in its epilogue (the extended digit never exists in memory: 8N count bytes of the
 * digit, 8N of the key, 8N or 16N of c^ per limb-polynomial); anything else (integer policies, N < 2^6, N >= 2^15) -- the
 * composition: the base-conversion launches into d_ext's slots of the run, then the ntt_rns_fwd_mul_batch route.  NTT_OPT_MODUP_FUSED
 * on plans[0]: 1 / 0 force the fused kernel (where built) / the composition for every run; the default, -1, takes the fused kernel
 * where the measurement recorded in profiles/r10/modup_mul_bench.txt says it is not slower than the two calls:
 *     fused for count == 1, the composition for count >= 2.
 * (Call rate of the fused route over ntt_rns_mod_up_batch + ntt_rns_fwd_mul_batch of the parent commit, 24 50-bit limbs, broadcast
 * key, accumulating, 2^14 x 2 / 64 / 1024 polynomials: count 1: 1.22-1.33 / 1.86-1.96 / 1.47-1.49; count 2: 0.70-0.74 / 1.10-1.13 /
 * 0.85-0.86; count 3: 0.59-0.64 / 0.96-0.99 / 0.73-0.74; count 8: 0.35-0.54 throughout.  The largest count not slower at both 64 and
 * 1024 polynomials is 1, and the 2-polynomial rows show no gain beyond it, so small calls get no rule of their own.)
 * NTT_ERR_ARG, nothing written: everything ntt_rns_mod_up_batch and ntt_rns_fwd_mul_batch refuse (the digit out of range, plans that
 * differ in N or device, a prime that appears twice, an unknown flag, a null pointer, overlapping strides, a plan without its
 * forward table), and d_c's span of words under the layout (first word to last) overlapping d_ext's: every limb's workgroups read
 * the digit while others write c^.  d_c against d_keyhat follows ntt_rns_fwd_mul_batch (c^ may alias key^).  Allocates nothing,
 * does not synchronise the host, issues no memset: capturable. ---- */
NTT_API int ntt_rns_mod_up_mul_batch(int nlimbs, ntt_plan *const *plans, uint64_t *d_c, uint64_t *d_ext, int first, int count,
                                     const uint64_t *d_keyhat, uint64_t batch, unsigned flags, void *stream);
NTT_API int ntt_rns_mod_up_mul_batch_strided(int nlimbs, ntt_plan *const *plans, uint64_t *d_c, uint64_t *d_ext, int first, int count,
                                             const uint64_t *d_keyhat, uint64_t limb_stride, uint64_t poly_stride, uint64_t batch,
                                             unsigned flags, void *stream);

/* ---- The key products for BOTH components of a key-switching key.  A key-switching key is a pair (key0_j, key1_j) per digit and the
 * result of a key switch a pair (c0, c1); the expensive operand -- the extended, forward-transformed digit -- is the same for both:
 *     c0^ (+)= fwd(x) (.) key0^,   c1^ (+)= fwd(x) (.) key1^,
 * x = d_a as it stands (ntt_rns_fwd_mul_pair_batch) or ModUp of the digit in d_ext (ntt_rns_mod_up_mul_pair_batch); x is read,
 * converted and transformed ONCE.  c0^ and c1^ are, bit for bit, what ntt_rns_fwd_mul_batch / ntt_rns_mod_up_mul_batch give with
 * (d_c0, key0) and with (d_c1, key1) on copies of the operand; flags (NTT_MUL_B_BROADCAST, NTT_MUL_ACCUMULATE, NTT_MUL_LAZY_IN: one
 * word for both components), layouts, limits (count <= 16) and canonical outputs are those of the single calls.
 * d_a, and the slots of d_ext outside the digit, are scratch after the call.  Where the fused pair kernel serves every run of the call
 * they are neither read nor written, and d_a / the digit's limbs are left as they were.
 * Per run of compatible limbs: FP64 policies at N = 2^6..2^14 -- one launch of the forward block kernel (the base conversion in its
 * prologue) whose epilogue runs once per component: 8N count + 16N (keys) + 16N or 32N (c0^, c1^) bytes per limb-polynomial, one set
 * of forward stages; anything else (integer policies, N < 2^6, N >= 2^15) -- the composition: the base-conversion launches into
 * d_ext's slots of the run, ONE forward transform of the run in place, one element-wise launch per 16 limbs that forms both
 * products.  NTT_OPT_PAIR_FUSED on plans[0]: 1 / 0 force the fused kernel (where built) / the composition for every run; the
 * default, -1, applies the rule recorded in profiles/r11/key_pair_bench.txt:
 *     fused for ntt_rns_fwd_mul_pair_batch and for count <= 2, the composition for count >= 3.
 * (Call rate over the better of the parent commit's two compositions -- the single call twice; ModUp + forward transform + two
 * element-wise accumulates --, 24 50-bit limbs, broadcast keys, accumulating, 2^14 x 64 / 1024 polynomials, ranges over eight rounds,
 * the parent's own spread 1.01-1.03.  Fused: no conversion 1.26-1.38 / 1.29-1.38; count 1: 1.21-1.31 / 1.21-1.32; count 2: 1.15-1.23 /
 * 1.11-1.16; count 3: 1.04-1.11 / 0.99-1.03; count 4: 0.95-1.00 / 0.90-0.92; count 8: 0.66-0.68 / 0.62-0.63.  Composition: 1.01-1.14 /
 * 1.05-1.09 for count 2..8, 0.82-0.87 / 0.80-0.83 for count 1.  The largest count at which the fused kernel is not slower at both is
 * 2; at count 3 it is inside the spread at 1024 polynomials and the composition is ahead.  At 2 polynomials, launch-bound, the fused
 * kernel reads 1.27-1.31 for count 1 and 0.78-0.83 for count 2, where the composition reads 1.06-1.13: the default loses there.)
 * NTT_ERR_ARG, nothing written: everything the single call refuses; a null pointer; c0^'s span of words under the layout (first word
 * to last) overlapping c1^'s; either output's span overlapping d_a / d_ext; either output's span overlapping the OTHER component's
 * key.  c_j^ against its own key_j^ follows ntt_rns_fwd_mul_batch.  Allocate nothing, do not synchronise the host, issue no memset:
 * capturable.  The pair form of the rotation key product is ntt_rns_galois_dot_pair_batch below. ---- */
NTT_API int ntt_rns_fwd_mul_pair_batch(int nlimbs, ntt_plan *const *plans, uint64_t *d_c0, uint64_t *d_c1, uint64_t *d_a,
                                       const uint64_t *d_b0hat, const uint64_t *d_b1hat, uint64_t batch, unsigned flags, void *stream);
NTT_API int ntt_rns_fwd_mul_pair_batch_strided(int nlimbs, ntt_plan *const *plans, uint64_t *d_c0, uint64_t *d_c1, uint64_t *d_a,
                                               const uint64_t *d_b0hat, const uint64_t *d_b1hat, uint64_t limb_stride,
                                               uint64_t poly_stride, uint64_t batch, unsigned flags, void *stream);
NTT_API int ntt_rns_mod_up_mul_pair_batch(int nlimbs, ntt_plan *const *plans, uint64_t *d_c0, uint64_t *d_c1, uint64_t *d_ext, int first,
                                          int count, const uint64_t *d_key0hat, const uint64_t *d_key1hat, uint64_t batch, unsigned flags,
                                          void *stream);
NTT_API int ntt_rns_mod_up_mul_pair_batch_strided(int nlimbs, ntt_plan *const *plans, uint64_t *d_c0, uint64_t *d_c1, uint64_t *d_ext,
                                                  int first, int count, const uint64_t *d_key0hat, const uint64_t *d_key1hat,
                                                  uint64_t limb_stride, uint64_t poly_stride, uint64_t batch, unsigned flags, void *stream);

/* ---- The first and the last step of a homomorphic multiplication on ciphertexts held in the NTT domain.
 * ntt_rns_tensor_batch: for ciphertexts (a0, a1) and (b0, b1), per limb l and word s,
 *     c0 = a0 b0,   c1 = a0 b1 + a1 b0,   c2 = a1 b1   (mod q_l),
 * outputs canonical.  Element-wise, so any domain; meant for NTT-domain operands.  All seven operands share one layout ([limb][batch][N];
 * _strided: any strides the RNS forms accept).  Integer arithmetic for every policy and every N >= 2: the products are exact 128-bit
 * integers, one Barrett reduction and one conditional subtraction per output word.  NTT_MUL_LAZY_IN allows input words anywhere in
 * [0, 4q) (2 (4q)^2 < 2^127 for q < 2^61); no other flag is accepted.  One launch per 16 limbs: 32N bytes read and 24N written per
 * limb-polynomial; when d_b0 == d_a0 and d_b1 == d_a1 (a squaring) every input word is loaded once, 16N read -- the result is bit for
 * bit that of the general path.  An output may BE an input (the same pointer: c0 = a0, c1 = a1 works in place; every thread reads its
 * four words before it stores its three); any other overlap of an output's span of words under the layout (first word to last) with an
 * input's or with another output's is refused.  NTT_ERR_ARG, nothing written: nlimbs < 1, a null pointer, plans that differ in N or
 * device, an unknown flag, overlapping strides, the overlaps above.
 * ntt_rns_mod_down_add_batch: ModDown of an accumulator INTO a ciphertext.  d_a is an operand over Q u P exactly as for
 * ntt_rns_mod_down_batch ([nq + np][batch][N]; _strided: a_limb_stride, a_poly_stride); d_c is an operand over the nq Q limbs with strides of
 * its own ([nq][batch][N]; c_limb_stride, c_poly_stride).  With r_l what ntt_rns_mod_down_batch with the same NTT_MODDOWN_TRANSFORMED /
 * NTT_MODDOWN_FLOOR flags leaves in Q limb l of a copy of d_a:
 *     c_l = r_l                       without NTT_MODDOWN_ACCUMULATE (an out-of-place ModDown: a rotation's c1'),
 *     c_l = (c_l + r_l) mod q_l       with it (c canonical on entry: relinearisation's (d0, d1) += ModDown(acc0, acc1), batch 2),
 * bit for bit the existing call followed by the addition.  Afterwards d_a's Q limbs are scratch (where the fused kernel serves every
 * run they are not written); its P limbs follow ModDown's rule (coefficients after a TRANSFORMED call, unchanged after a coefficient
 * call).  Per run of compatible Q limbs: TRANSFORMED, FP64 policies, N = 2^6..2^14 -- ONE launch of the forward block kernel with the
 * base conversion in its prologue, whose epilogue reads c^ from d_a, (when accumulating) the addend from d_c, adds in integer arithmetic
 * and stores to d_c: 8N np + 16N bytes per Q limb-polynomial (24N when accumulating); anything else (integer policies, N < 2^6,
 * N >= 2^15, coefficients) -- the composition: ntt_rns_mod_down_batch's route of that run in place on d_a, then one element-wise launch
 * per 16 limbs.  NTT_OPT_MODDOWN_ADD_FUSED on plans[0]: 1 / 0 force the fused kernel (where built) / the composition for every run; the
 * default, -1, applies the rule recorded in profiles/r14/ct_mul_bench.txt:
 *     fused wherever the kernel is built.
 * (Call rate of the fused route over the composition route, 24 50-bit Q limbs, accumulating, 2^14 x 2 / 64 / 1024 polynomials, ranges over
 * five rounds of alternating processes: np 1: 1.08 / 1.27-1.32 / 1.51-1.52; np 2: 1.05-1.06 / 1.17-1.19 / 1.29-1.30; np 4: 1.04 /
 * 1.15-1.16 / 1.21-1.22; 2^13 likewise, 0.99-1.06 at 2 polynomials.  The fused kernel is not slower at both 64 and 1024 polynomials for
 * every np measured.  Over the parent commit's ntt_rns_mod_down_batch followed by the addition with torch integer ops, parent's own
 * spread 1.01-1.02: fused np 1: 1.30-1.31 / 2.34-2.42 / 2.79-2.81; np 2: 1.19-1.20 / 1.88-1.91 / 2.05-2.07; np 4: 1.15 / 1.66-1.69 /
 * 1.76-1.79; the composition 1.11-1.22 / 1.43-1.85 / 1.44-1.86.  The fused call takes 6-16 % longer than the parent's ModDown alone at
 * 1024 polynomials, 20-37 % longer at 2^14 x 64.)
 * The tensor against 4 L ntt_pointwise_mul_batch calls plus the sum with torch integer ops, the same shape: 34-41 / 3.37-3.46 / 2.80-2.88
 * x at 2^14 (squaring by aliasing: 3.69-3.88 / 3.76-3.80 x at 64 / 1024); its time is 3.8-4.1 x ntt_copy_probe of one operand at 1024
 * polynomials (3.5 by the algorithmic bytes), the squaring's 3.0-3.1 x (2.5).  A two-words-per-lane form with 16-byte accesses measured
 * 3-5 % SLOWER than the one-word form (squaring: within 1.5 %), so one form ships (profiles/r14/tensor_width.txt).
 * NTT_ERR_ARG, nothing written: everything ntt_rns_mod_down_batch refuses, a null d_c, overlapping strides in either layout, d_c's span
 * of words overlapping d_a's, a table the chosen route needs that a plan lacks.
 * All four: allocate nothing, do not synchronise the host, issue no memset: capturable. ---- */
enum { NTT_MODDOWN_ACCUMULATE = 4 }; /* ntt_rns_mod_down_add_batch only (ntt_rns_mod_down_batch refuses it): c += ..., c canonical on entry */
NTT_API int ntt_rns_tensor_batch(int nlimbs, ntt_plan *const *plans, uint64_t *d_c0, uint64_t *d_c1, uint64_t *d_c2, const uint64_t *d_a0,
                                 const uint64_t *d_a1, const uint64_t *d_b0, const uint64_t *d_b1, uint64_t batch, unsigned flags,
                                 void *stream);
NTT_API int ntt_rns_tensor_batch_strided(int nlimbs, ntt_plan *const *plans, uint64_t *d_c0, uint64_t *d_c1, uint64_t *d_c2,
                                         const uint64_t *d_a0, const uint64_t *d_a1, const uint64_t *d_b0, const uint64_t *d_b1,
                                         uint64_t limb_stride, uint64_t poly_stride, uint64_t batch, unsigned flags, void *stream);
NTT_API int ntt_rns_mod_down_add_batch(int nq, int np, ntt_plan *const *plans, uint64_t *d_c, uint64_t *d_a, uint64_t batch, unsigned flags,
                                       void *stream);
NTT_API int ntt_rns_mod_down_add_batch_strided(int nq, int np, ntt_plan *const *plans, uint64_t *d_c, uint64_t *d_a, uint64_t c_limb_stride,
                                               uint64_t c_poly_stride, uint64_t a_limb_stride, uint64_t a_poly_stride, uint64_t batch,
                                               unsigned flags, void *stream);

/* ---- Exact RNS base conversion and scaled ModDown: what BFV multiplication (Halevi, Polyakov, Shoup) needs beyond the approximate
 * conversions above, which leave x + u B and round(x / P) - v.  For a basis B = {b_i} of n <= 16 primes, b^_i = B / b_i and
 * z_i = [x_i b^_i^-1]_{b_i}:
 *     ExactBConv_{B->q}(x) = ( sum_i z_i [b^_i]_q  -  v [B]_q ) mod q,      v = rint(s),
 *     s = ((fl(z_0) rho_0 + fl(z_1) rho_1) + ...) left to right,            rho_i = 1.0 / (double)b_i,
 * every operation one IEEE double operation rounded to nearest (no fused multiply-add), rint to even.  The FP64 error of s is below
 * 2^-44 (at most 2^-51 per term, 2^-49 per sum of a partial sum below 16; n <= 16), so for x in [0, B) with |2x - B| > 2^-43 B the
 * result is the CENTRED representative of x -- x below B / 2, x - B above -- reduced mod q; inside that band it is x or x - B, the
 * same choice in every destination limb of the call (v depends on the source words only).
 * ntt_rns_mod_up_exact_batch: ntt_rns_mod_up_batch with ExactBConv_{digit->q_l} for FastBConv: the same operand, layouts, in-place
 * rule, 1 <= count <= 16, flag (NTT_MODUP_TRANSFORMED only), routes (coefficients: one launch per 16 destination limbs, 8N(count + ndst)
 * bytes per polynomial; NTT domain: the inverse of the digit, those launches, the forward of every limb) and refusals.
 * ntt_rns_mod_down_exact_batch: the operand of ntt_rns_mod_down_batch (plans[0 .. nq-1] kept, plans[nq .. nq+np-1] divided out,
 * 1 <= np <= 16) and a multiplier 1 <= mult < 2^61, reduced per prime on the host.  With t the P limbs' coefficients,
 *     c_l <- ( mult c_l - ExactBConv_{P->q_l}([mult t]_P) ) P^-1  mod q_l,
 * which for the x in [0, QP) behind the operand is round(mult x / P) mod Q exactly (P is odd: no ties; floor or ceiling inside the band
 * above, taken for [mult x]_P).  With BFV's Q as the divided-out basis and mult = t this is BFV's scaling round(t x / Q); mult = 1 is an exact ModDown.  The multiplier costs
 * nothing in the conversion (it is folded into [mult b^_j^-1]_{p_j}) and one more modular product per word at the end.  Flags:
 * NTT_MODDOWN_TRANSFORMED only.  The P slots follow ModDown's rule (coefficients after a TRANSFORMED call, unchanged otherwise).
 * Routes: coefficients -- one launch per 16 Q limbs, 8N(2nq + np) bytes per polynomial; NTT domain -- the inverse of the P limbs, then per
 * run of compatible Q limbs: FP64 policies at N = 2^6..2^14 -- ONE launch of the forward block kernel with the exact conversion in its
 * prologue (the FP64 sum beside the 128-bit sum of every word) and (c^ [mult]_q - x) P^-1 in its epilogue: 8N np + 16N bytes per Q
 * limb-polynomial, as for ntt_rns_mod_down_batch; anything else (integer-policy limbs, N < 2^6, N >= 2^15: no fused kernel is built for
 * those) -- the sandwich of the inverse, the coefficient launch and the forward.  NTT_OPT_RESCALE_FUSED on plans[0] selects the route as
 * for ntt_rns_mod_down_batch (0: the sandwich everywhere), under the rule recorded in profiles/r15/exact_bench.txt:
 *     fused wherever the kernel is built, for np <= 4; the sandwich for np >= 5.
 * (The fused kernel redoes the conversion in every Q limb's workgroup.  Call rate of the fused route over its own sandwich, 24 50-bit Q
 * limbs, mult 65537, 2 / 64 / 1024 polynomials, ranges over five rounds of alternating processes, 2^13 then 2^14: np 1: 1.12-1.14 /
 * 1.78-1.80 / 1.85-1.86, 1.17-1.19 / 1.64-1.65 / 1.51-1.52; np 2: 0.98-0.99 / 1.55-1.57 / 1.57-1.58, 1.03-1.06 / 1.41-1.42 / 1.26; np 4:
 * 0.79-0.80 / 1.26-1.29 / 1.23, 0.84-0.85 / 1.12-1.13 / 0.97-0.98; np 8: 0.58-0.60 / 0.95-0.97 / 0.89-0.90, 0.63 / 0.84 / 0.72-0.73: slower
 * at both 64 and 1024 polynomials at np 8 only; np 5..7 were not measured and go with 8.  Over the parent commit's approximate
 * ntt_rns_mod_down_batch at the same shape, parent's own spread 1.00-1.03: fused np 1: 0.66-0.75 -- the approximate call has the rescale's
 * one-prime path, the exact one the general path --, np 2 / 4: 0.91-0.97 at 2 and 64 polynomials, 0.95-1.03 at 1024.  The exact ModUp in
 * coefficients over the parent's ntt_rns_mod_up_batch, 24 limbs, count 1 / 4 / 8: 0.91-0.98 at 2 polynomials, 0.79-0.86 / 0.84-0.89 /
 * 0.89-0.95 at 64 and 1024 (spread 1.00-1.05): the correction costs 5-21 %.  The four-call sequence below, 16 / 256 multiplications at
 * 2^13 and 2^14, over the same sequence from the parent's approximate calls plus the multiplication by t with torch integer ops:
 * 1.36-1.47 x, one multiplication 1.21-1.29 x (spread 1.01-1.05).)
 * NTT_ERR_ARG, nothing written: everything the approximate call refuses, mult == 0 or mult >= 2^61, NTT_MODDOWN_FLOOR,
 * NTT_MODDOWN_ACCUMULATE, any other flag.  All four: allocate nothing (ntt_plan_reserve covers the transforms they issue), do not
 * synchronise the host, issue no memset: capturable.
 * A BFV tensor-and-scale over buffers [R limbs][Q limbs] (R FIRST, so that the ModDown keeps it): exact ModUp of the operands Q -> R,
 * ntt_rns_tensor_batch over all limbs, ntt_rns_mod_down_exact_batch(nr, nq, mult = t), exact ModUp R -> Q (examples/rns_bfv_mul.c). ---- */
NTT_API int ntt_rns_mod_up_exact_batch(int nlimbs, ntt_plan *const *plans, uint64_t *d_a, int first, int count, uint64_t batch,
                                       unsigned flags, void *stream);
NTT_API int ntt_rns_mod_up_exact_batch_strided(int nlimbs, ntt_plan *const *plans, uint64_t *d_a, int first, int count,
                                               uint64_t limb_stride, uint64_t poly_stride, uint64_t batch, unsigned flags, void *stream);
NTT_API int ntt_rns_mod_down_exact_batch(int nq, int np, ntt_plan *const *plans, uint64_t *d_a, uint64_t mult, uint64_t batch,
                                         unsigned flags, void *stream);
NTT_API int ntt_rns_mod_down_exact_batch_strided(int nq, int np, ntt_plan *const *plans, uint64_t *d_a, uint64_t mult,
                                                 uint64_t limb_stride, uint64_t poly_stride, uint64_t batch, unsigned flags, void *stream);

/* ---- BGV modulus switching: ModDown that keeps the plaintext mod T.  The tensor, the approximate ModUp, the key products and the
 * Galois calls above are scheme-agnostic (for BGV the ModUp overshoot u D cancels mod QP and the key noise is T e); what BGV needs
 * beyond them is a division by primes whose correction is = x mod P and = 0 mod T -- ntt_rns_rescale_batch and ntt_rns_mod_down_batch
 * subtract [x]_P, which scrambles the plaintext, and ntt_rns_mod_down_exact_batch's one multiplier cannot express [T^-1]_{p_j}.
 * Operand as for ntt_rns_mod_down_batch: plans[0 .. nq-1] kept (Q), plans[nq .. nq+np-1] divided out (P), 1 <= np <= 16, product P,
 * p^_j = P / p_j, h = (P - 1) / 2; a plaintext modulus 1 <= t < 2^61 that no P prime divides (it need not be coprime to the kept primes:
 * [t]_{q_l} = 0 is legal).  With t_j the coefficients of P limb j:
 *     z_j = [ ( t_j [t^-1]_{p_j} + [h]_{p_j} ) [p^_j^-1]_{p_j} ]_{p_j}         canonical, [h]_{p_j} = (p_j - 1) / 2
 *     F_l = ( sum_j z_j [p^_j]_{q_l} ) mod q_l                                 the exact integer sum, reduced once
 *     c_l <- ( c_l - [t]_{q_l} (F_l - [h]_{q_l}) ) [P^-1]_{q_l}  mod q_l       canonical
 * Every output word is unique: all intermediates are canonical residues, so the routes below agree bit for bit.  For the x in [0, QP)
 * behind the operand, w the centred residue of x t^-1 mod P and y = (x - t w) / P (an integer, y = x P^-1 mod t), the Q limbs hold
 * y - v t mod Q with ONE integer 0 <= v < np for all limbs (v = 0 for np = 1): the deviation is a multiple of t, the plaintext is
 * untouched and the noise grows by at most (np - 1) t.  THE CALLER OWNS THE FACTOR P^-1 mod t that the plaintext picks up: choose
 * primes = 1 mod t, or track a correction factor per ciphertext.  t = 1 gives ntt_rns_mod_down_batch's words, word for word.
 * ntt_rns_mod_down_bgv_batch: in place on d_a ([nq + np][batch][N]; _strided: the strides of ntt_rns_mod_down_batch).  np = 1 is BGV's
 * modulus switch by the last prime, np > 1 drops several levels at once.  Flags: NTT_MODDOWN_TRANSFORMED only.
 * ntt_rns_mod_down_bgv_add_batch: into a ciphertext d_c over the nq Q limbs with strides of its own, exactly as
 * ntt_rns_mod_down_add_batch: c_l = r_l, or c_l = (c_l + r_l) mod q_l with NTT_MODDOWN_ACCUMULATE (c canonical on entry), r_l what the
 * in-place form leaves in Q limb l of a copy of d_a -- the last step of a BGV relinearisation or rotation.  Flags:
 * NTT_MODDOWN_TRANSFORMED, NTT_MODDOWN_ACCUMULATE.  Afterwards d_a's Q limbs are scratch (not written where the fused kernel serves
 * every run).  Both: the P slots hold coefficients after a TRANSFORMED call and are unchanged otherwise; NTT_MODDOWN_FLOOR is refused
 * (the correction is centred).
 * Routes.  Coefficients: ntt_rns_mod_down_batch's coefficient kernel with the constants folded on the host ([h t]_{p_j},
 * [t^-1 p^_j^-1]_{p_j}, [t p^_j]_{q_l}, [t h]_{q_l}), one launch per 16 Q limbs, the P limbs read once per launch, np = 1 on the general
 * path; the add form then one element-wise launch per 16 limbs.  NTT domain: the inverse of the P limbs, then per run of compatible Q
 * limbs: FP64 policies at N = 2^6..2^14 -- ONE launch of the forward block kernel (moddown_bgv_fwd_kernel, one template for both forms)
 * with the conversion in its prologue: [t]_{q_l} is multiplied into the np table entries [p^_j]_{q_l} and into [h]_{q_l} once per
 * workgroup, so the per-word work is that of ntt_rns_mod_down_add_batch's kernel (np = 1: no table, one more Shoup product per word);
 * anything else (integer-policy limbs, N < 2^6, N >= 2^15) -- the sandwich of the inverse, the coefficient launch and the forward.
 * NTT_OPT_BGV_FUSED on plans[0]: 1 / 0 force the fused kernel (where built, any np) / the sandwich for every run; the default, -1,
 * applies the rule recorded in profiles/r16/bgv_bench.txt:
 *     in place: fused for np <= 4 up to N = 2^13 and for np <= 2 at 2^14; into a ciphertext: fused for np <= 4; the sandwich beyond.
 * (The fused kernel redoes the conversion in every Q limb's workgroup, the sandwich once per 16 Q limbs.  Call rate of the fused route
 * over its own sandwich, 24 50-bit Q limbs, T = 65537, 64 / 1024 polynomials, ranges over five rounds of alternating processes, 2^13
 * then 2^14.  In place: np 1: 1.99-2.08 / 2.19-2.21, 1.86-1.93 / 1.87-1.88; np 2: 1.56-1.57 / 1.42-1.43, 1.40-1.42 / 1.26; np 4:
 * 1.26-1.27 / 1.11, 1.13-1.14 / 0.98; np 8: 0.97 / 0.82-0.83, 0.88 / 0.73-0.74.  Add form: np 1: 2.25-2.32 / 2.54-2.56, 1.86-1.93 /
 * 2.26-2.27; np 2: 1.78-1.81 / 1.65-1.68, 1.48-1.50 / 1.54-1.55; np 4: 1.46-1.48 / 1.30-1.32, 1.23-1.24 / 1.21-1.22; np 8: 1.11-1.12 /
 * 0.97, 0.95 / 0.89.  The default takes the fused kernel for exactly those np at which it is not slower at both 64 and 1024
 * polynomials; np 3 goes with 4 and 5..7 with 8, sizes below 2^13 with 2^13.  At 2 polynomials the fused kernel reads 1.27-1.47 at
 * np 1, 1.00-1.16 at np 2, 0.82-0.94 at np 4.  Cost of the correction, fused over the parent commit's approximate
 * ntt_rns_mod_down_batch / ntt_rns_mod_down_add_batch at the same shape, parent's own spread 1.00-1.06: np 2, 4, 8: 0.95-1.04 at every
 * batch size; np 1: 0.81-0.92 -- the approximate calls have the rescale's one-prime path, which skips the source product and the
 * product by [t]_q.)
 * NTT_ERR_ARG, nothing written: everything ntt_rns_mod_down_batch / ntt_rns_mod_down_add_batch refuse, t == 0, t >= 2^61, a P prime that
 * divides t, NTT_MODDOWN_FLOOR, NTT_MODDOWN_ACCUMULATE in the in-place form, any other flag.  All four: allocate nothing
 * (ntt_plan_reserve covers the transforms they issue), do not synchronise the host, issue no memset: capturable.
 * A BGV multiplication with relinearisation and one modulus switch through public calls: examples/rns_bgv_mul.c. ---- */
NTT_API int ntt_rns_mod_down_bgv_batch(int nq, int np, ntt_plan *const *plans, uint64_t *d_a, uint64_t t, uint64_t batch, unsigned flags,
                                       void *stream);
NTT_API int ntt_rns_mod_down_bgv_batch_strided(int nq, int np, ntt_plan *const *plans, uint64_t *d_a, uint64_t t, uint64_t limb_stride,
                                               uint64_t poly_stride, uint64_t batch, unsigned flags, void *stream);
NTT_API int ntt_rns_mod_down_bgv_add_batch(int nq, int np, ntt_plan *const *plans, uint64_t *d_c, uint64_t *d_a, uint64_t t, uint64_t batch,
                                           unsigned flags, void *stream);
NTT_API int ntt_rns_mod_down_bgv_add_batch_strided(int nq, int np, ntt_plan *const *plans, uint64_t *d_c, uint64_t *d_a, uint64_t t,
                                                   uint64_t c_limb_stride, uint64_t c_poly_stride, uint64_t a_limb_stride,
                                                   uint64_t a_poly_stride, uint64_t batch, unsigned flags, void *stream);

/* ---- Galois automorphisms (rotation, conjugation) and the rotation key product.  For odd g, 0 < g < 2N,
 *     sigma_g(a)(X) = a(X^g)  in Z_q[X] / (X^N + 1).
 * g = 5^steps mod 2N rotates the CKKS / BGV slots by `steps` (ntt_galois_rotation; negative steps: the inverse power),
 * g = 2N - 1 is the conjugation, g = 1 is a copy.
 * Coefficients (without NTT_GALOIS_TRANSFORMED; natural order, canonical words in and out): with u = g^-1 t mod 2N for t in [0, N),
 *     out[t] = a[u] if u < N, else (q - a[u - N]) mod q  (a zero stays zero);
 * equivalently a[i] goes to position g i mod N, negated when (g i mod 2N) >= N.
 * NTT domain (NTT_GALOIS_TRANSFORMED; bit-reversed storage, as ntt_fwd_batch leaves it): storage slot s holds the evaluation at
 * psi^(2i+1), i = bitrev_m(s), m = log2 N, and sigma_g is a permutation of words without arithmetic:
 *     out[s] = in[bitrev_m(j)],  j = (g i + (g - 1) / 2) mod N,  i = bitrev_m(s).
 * Words are copied bit for bit, so lazy words (ntt_fwd_batch_lazy) pass through.  ntt_galois_batch is the one-limb case
 * ([batch][N]); the RNS forms take the layouts of the other RNS forms ([limb][batch][N]; _strided: any strides those accept, both
 * operands in the same layout).  One launch per 16 limbs.
 * ntt_rns_galois_dot_batch is the inner loop of hoisted rotations: the ModUp'd digits a_i^ (NTT domain, over Q u P) are formed once
 * per ciphertext, and each rotation needs c^ = sum_{i<k} sigma_g(a_i^) (.) key_i^ per limb (NTT_GALOIS_ACCUMULATE: c^ += ..., c^
 * canonical on entry), then ModDown.  One element-wise kernel, the permutation applied while the digits are read:
 *     c[s] (+)= sum_i a_i[bitrev_m(j(s))] * key_i[s] mod q,
 * canonical words in and out, the sum exact in 128 bits and reduced once.  d_ahat and d_keyhat are HOST arrays of k device pointers,
 * 1 <= k <= 32, as for ntt_rns_inv_dot_batch; every operand is in the call's layout, except that with NTT_GALOIS_KEY_BROADCAST
 * every key_i^ is ONE polynomial per limb ([limb][N]) shared by the batch, as for NTT_MUL_B_BROADCAST.  The dot is always in the NTT
 * domain: NTT_GALOIS_TRANSFORMED is accepted there and changes nothing.
 * All calls are OUT OF PLACE.  NTT_ERR_ARG, nothing written: g even, 0 or >= 2N; nlimbs < 1, k out of range, a null pointer; plans
 * that differ in N or device; an unknown flag (NTT_GALOIS_ACCUMULATE or NTT_GALOIS_KEY_BROADCAST passed to galois included);
 * strides under which two (limb, polynomial) ranges overlap; an output whose span of words under the layout (first word to last)
 * overlaps that of an input (d_out with d_in; d_c with any a_i^ or key_i^; inputs may overlap each other).  Allocate nothing, do
 * not synchronise the host, issue no memset: capturable. ---- */
enum { NTT_GALOIS_TRANSFORMED = 1,   /* operands in the NTT domain (bit-reversed, as ntt_fwd_batch leaves them) */
       NTT_GALOIS_ACCUMULATE = 2,    /* galois_dot: c^ += ... (c^ canonical on entry) */
       NTT_GALOIS_KEY_BROADCAST = 4  /* galois_dot: every key_i^ is ONE polynomial per limb ([limb][N]) shared by the batch */ };
NTT_API uint64_t ntt_galois_rotation(uint64_t N, int64_t steps); /* 5^steps mod 2N (negative steps: the inverse power); 0 on a bad N */
NTT_API int ntt_galois_batch(const ntt_plan *p, uint64_t *d_out, const uint64_t *d_in, uint64_t g, uint64_t batch, unsigned flags,
                             void *stream);
NTT_API int ntt_rns_galois_batch(int nlimbs, ntt_plan *const *plans, uint64_t *d_out, const uint64_t *d_in, uint64_t g, uint64_t batch,
                                 unsigned flags, void *stream);
NTT_API int ntt_rns_galois_batch_strided(int nlimbs, ntt_plan *const *plans, uint64_t *d_out, const uint64_t *d_in, uint64_t g,
                                         uint64_t limb_stride, uint64_t poly_stride, uint64_t batch, unsigned flags, void *stream);
NTT_API int ntt_rns_galois_dot_batch(int nlimbs, ntt_plan *const *plans, uint64_t *d_c, int k, const uint64_t *const *d_ahat,
                                     const uint64_t *const *d_keyhat, uint64_t g, uint64_t batch, unsigned flags, void *stream);
NTT_API int ntt_rns_galois_dot_batch_strided(int nlimbs, ntt_plan *const *plans, uint64_t *d_c, int k, const uint64_t *const *d_ahat,
                                             const uint64_t *const *d_keyhat, uint64_t g, uint64_t limb_stride, uint64_t poly_stride,
                                             uint64_t batch, unsigned flags, void *stream);

/* the rotation key product for both components of the rotation key: c_j^ (+)= sum_{i<k} sigma_g(a_i^) (.) key_j,i^, j = 0, 1, bit for bit
 * two ntt_rns_galois_dot_batch calls; every permuted digit word is loaded once and enters two 128-bit sums (8N(k + 4) bytes per
 * limb-polynomial accumulating with broadcast keys, against 2 * 8N(k + 2)).  One launch per 16 limbs, every policy.  Refused as
 * ntt_rns_galois_dot_batch refuses, and: a null pointer among the new arguments, d_c0's span overlapping d_c1's, either output
 * overlapping any a_i^ or any key of either component.
 * Measured (profiles/r11/key_pair_bench.txt, 24 50-bit limbs, broadcast keys, accumulating, 2^14 x 64 / 1024 polynomials): k = 3:
 * 1.23-1.31 / 1.28-1.37 x the call rate of two ntt_rns_galois_dot_batch calls of the parent commit, k = 8: 1.43-1.54 / 1.44-1.55 x;
 * the call takes 4.4-4.5 (k = 3) and 8.2-8.5 (k = 8) times ntt_copy_probe of one operand. */
NTT_API int ntt_rns_galois_dot_pair_batch(int nlimbs, ntt_plan *const *plans, uint64_t *d_c0, uint64_t *d_c1, int k,
                                          const uint64_t *const *d_ahat, const uint64_t *const *d_key0hat, const uint64_t *const *d_key1hat,
                                          uint64_t g, uint64_t batch, unsigned flags, void *stream);
NTT_API int ntt_rns_galois_dot_pair_batch_strided(int nlimbs, ntt_plan *const *plans, uint64_t *d_c0, uint64_t *d_c1, int k,
                                                  const uint64_t *const *d_ahat, const uint64_t *const *d_key0hat,
                                                  const uint64_t *const *d_key1hat, uint64_t g, uint64_t limb_stride, uint64_t poly_stride,
                                                  uint64_t batch, unsigned flags, void *stream);

/* ---- the linear layer: linear combinations of RNS operands with a Galois map and a multiplier per term.
 * ntt_rns_lincomb_batch: per limb l, polynomial p and storage slot s (m = log2 N),
 *     c[l,p,s] = ( [ACCUMULATE: c[l,p,s]] + bias_l + sum_{i<k} a_i[l,p,src_{g_i}(s)] * mu_i(l,p,s) ) mod q_l,   canonical,
 *     mu_i     = m_i[l,p,s]  (m_i[l,s] with NTT_LINCOMB_M_BROADCAST)   if d_m && d_m[i]
 *              = s_{i,l} = h_s[i * nlimbs + l]                         otherwise (h_s NULL: 1)
 *     src_g(s) = bitrev_m((g bitrev_m(s) + (g - 1) / 2) mod N)         (the NTT-domain map of ntt_rns_galois_batch; g = 1: s).
 * In the NTT domain (bit-reversed storage, as ntt_fwd_batch leaves it) this is c (+)= bias + sum_i sigma_{g_i}(a_i) * mu_i; the
 * multiplier is read unpermuted, as the key of ntt_rns_galois_dot_batch.  With every g = 1 the call is element-wise and serves
 * either domain.  The bias is added to EVERY word: it is the constant polynomial bias_l only in the NTT domain (in coefficients a
 * constant is one word, position 0).
 * d_a and d_m are HOST arrays of k device pointers (entries of d_m may be NULL, and d_m itself); h_s ([k][nlimbs], read only where
 * term i has no polynomial multiplier), h_g (k Galois elements, NULL: all 1) and h_bias (nlimbs words, NULL: none) are host arrays,
 * copied into the launch: they may be reused as soon as the call returns.  Every operand is in the call's layout ([limb][batch][N];
 * _strided: any strides the other RNS forms accept), except that with NTT_LINCOMB_M_BROADCAST every polynomial multiplier is ONE
 * polynomial per limb ([limb][N]) shared by the batch.
 * The sum is the exact integer in 128 bits, reduced once, then one conditional subtraction: every output word is the one canonical
 * residue.  1 <= k <= 16 with canonical inputs (16 (2^61)^2 + 2^61 + 2^61 < 2^127).  With NTT_LINCOMB_LAZY_IN the a_i words may lie
 * anywhere in [0, 4q) (< 2^63; ntt_fwd_batch_lazy's words), the multipliers, scalars, bias and c stay canonical, and 1 <= k <= 8
 * (8 2^63 2^61 = 2^127).
 * One launch per 16 limbs, integer arithmetic for every policy and every N >= 2; NTT_OPT_MAX_GRID of plans[0] is honoured.  Allocates
 * nothing, does not synchronise the host, issues no memset: capturable.
 * d_c may be the same pointer as an a_i with g_i = 1, or as an m_i in c's layout (not a broadcast one): every thread reads all its
 * words before it stores its own position.  Any other overlap between d_c's span of words under the layout (first word to last) and
 * an input's is refused, an a_i with g_i != 1 that is d_c included; inputs may overlap each other.
 * NTT_ERR_ARG, nothing written: nlimbs < 1; k out of range for the flags; a null d_c, d_a or d_a[i]; a g_i that is even, 0 or >= 2N;
 * a scalar that is read, or a bias, not below its q_l; plans that differ in N or device; an unknown flag; NTT_LINCOMB_M_BROADCAST
 * without a polynomial multiplier; strides under which two (limb, polynomial) ranges overlap; the overlaps above.
 * Bytes moved per limb and polynomial: 8N(k + n_m + 1) for n_m polynomial multipliers, 8N(k + 1) with broadcast multipliers, 8N
 * more when accumulating.  Recipes (everything not named is NULL / 0; q_l the limb's prime):
 *     add          c = a + b            k = 2, d_a = {a, b}                                         24N
 *     sub          c = a - b            k = 2, h_s = {1.., (q_l - 1)..}                             24N
 *     negate       c = -a               k = 1, h_s = {(q_l - 1)..}                                  16N
 *     scale        c = w a              k = 1, h_s = {[w]_q_l..}                                    16N
 *     axpy         c += w a             k = 1, h_s = {[w]_q_l..}, ACCUMULATE                        24N
 *     add constant c = a + w            k = 1, h_bias = {[w]_q_l..}        (NTT domain)             16N
 *     polynomial   c = sum w_i ct_i + w_0   k terms, h_s, h_bias                                    8N(k + 1)
 *     plaintext multiply-accumulate  c += pt (.) a     k = 1, d_m = {pt}, ACCUMULATE                32N (24N: M_BROADCAST)
 *     hoisted transform   c0 = sum_i pt_i (.) sigma_{g_i}(a)   d_a = {a..}, d_m = {pt_i}, h_g = {g_i}, M_BROADCAST   8N(k + 1)
 *     inner sum    c = sum_i sigma_{g_i}(a)                    d_a = {a..}, h_g = {g_i}                              8N(k + 1)
 * (a listed k times is read k times through different permutations: the count is of requests, most of them served on chip.)
 * Measured: 24 x 50-bit limbs, 2^13 / 2^14, ranges over five rounds of alternating processes (profiles/r17/lincomb_bench.txt; the parent's own spread
 * 1.00-1.05 at 64 and 1024 polynomials).  The addition runs at 0.87-0.88 of ntt_copy_probe's rate at the same bytes at 1024 polynomials
 * (0.72-0.83 at 64), the 4-term scalar combination with bias at 0.89-0.93; against torch integer ops beside the parent commit's library
 * 2.16-2.97 x and 2.58-3.14 x.  sum_i pt_i (.) sigma_{g_i}(a), broadcast multipliers, distinct g: 2.18-2.27 x (k = 3) and 3.27-3.55 x (k = 8)
 * k accumulating ntt_rns_galois_dot_batch calls of the parent; all g equal, against ONE such call: 0.95-1.15 x at k = 3, 0.86-1.00 x at
 * k = 8 (1.00 at 1024 polynomials).  2 polynomials are launch-bound.  The addition's ratio lies inside the tensor kernel's 0.86-0.92, so no
 * +-1 specialisation (additions with conditional subtractions) was built: one general kernel ships. ---- */
enum { NTT_LINCOMB_ACCUMULATE = 1,   /* c += ... (c canonical on entry) */
       NTT_LINCOMB_M_BROADCAST = 2,  /* every polynomial multiplier is ONE polynomial per limb ([limb][N]) shared by the batch */
       NTT_LINCOMB_LAZY_IN = 4       /* a_i words anywhere in [0, 4q) */ };
NTT_API int ntt_rns_lincomb_batch(int nlimbs, ntt_plan *const *plans, uint64_t *d_c, int k, const uint64_t *const *d_a,
                                  const uint64_t *const *d_m, const uint64_t *h_s, const uint64_t *h_g, const uint64_t *h_bias,
                                  uint64_t batch, unsigned flags, void *stream);
NTT_API int ntt_rns_lincomb_batch_strided(int nlimbs, ntt_plan *const *plans, uint64_t *d_c, int k, const uint64_t *const *d_a,
                                          const uint64_t *const *d_m, const uint64_t *h_s, const uint64_t *h_g, const uint64_t *h_bias,
                                          uint64_t limb_stride, uint64_t poly_stride, uint64_t batch, unsigned flags, void *stream);

/* ---- out of the RNS: the last step of a decryption.  d_a holds nlimbs limbs in COEFFICIENTS, canonical ([limb][batch][N]); x in
 * [0, Q) is the integer behind the nlimbs words of one coefficient, Q = prod q_l, x_c its centred representative (x, or x - Q from
 * Q / 2 on).  Every q_l < 2^61, the primes pairwise distinct.
 *
 * ntt_rns_to_plain_batch: d_m ([batch][N]) receives one word in [0, t) per coefficient, 1 <= nlimbs <= 16, 2 <= t < 2^61, t ANY
 * integer (powers of two and composites included):
 *     flags = 0 (BGV)          m = [x_c]_t.  The exact base conversion of ntt_rns_mod_up_exact_batch with t for the destination
 *                              prime; nothing has to be coprime.  Exact for |2x - Q| > 2^-43 Q; inside that band [x]_t or [x - Q]_t.
 *     NTT_PLAIN_SCALE (BFV)    m = round(t x / Q) mod t; every q_l coprime to t.  Q is odd: no ties.  With rho = t x mod Q exact for
 *                              |2 rho - Q| > 2^-43 Q; inside that band one of the two neighbouring integers (mod t).
 * The band is that of the exact conversions: one FP64 sum of at most 16 terms below 1 decides the rounding, with an error below
 * 2^-44.  A decryption's noise keeps x (rho) far from Q / 2 -- it is where decryption fails anyway.  The FP64 operations and their
 * order are fixed (csrc/ntt_plain.h), so the result is a function of the input words alone, on every device and in the tests' model.
 *
 * ntt_rns_to_double_batch: d_y ([batch][N] doubles) receives y = fl(x_c) * scale, nlimbs 1 or 2 (Q < 2^122: where CKKS decrypts): fl
 * is the round-to-nearest-even conversion of the exact signed integer -- one rounding, also above 2^64 --, then one IEEE product.
 * No band: the two-limb reconstruction is exact in 128 bits.  x_c = 0 gives +0.0 * scale.  What follows is the decoding FFT.
 *
 * _strided: the source's limbs a_limb_stride and polynomials a_poly_stride words apart (any strides the other RNS forms accept), the
 * output's polynomials m_poly_stride (y_poly_stride) >= N words apart.
 * The output may be d_a itself -- limb 0's slots, with the source's polynomial stride: every thread reads all its words before its
 * one store.  Any other overlap between the output's span of words (first to last) and the source's is the caller's error, refused.
 * ONE launch per call, integer and FP64 arithmetic of its own for every policy and every N >= 2; NTT_OPT_MAX_GRID of plans[0] is
 * honoured.  Allocates nothing, does not synchronise the host, issues no memset: capturable.  8N(nlimbs + 1) bytes per polynomial.
 * NTT_ERR_ARG, nothing written: nlimbs outside 1..16 (to_double: 1..2); plans that differ in N or device; a prime >= 2^61 or listed
 * twice; t < 2 or t >= 2^61; NTT_PLAIN_SCALE with a prime that divides t; any other flag; a null d_m / d_y or d_a with batch > 0;
 * strides under which two (limb, polynomial) ranges overlap, or an output stride below N; the overlap above.
 *
 * Decryption is two calls.  With the secret key s^ and the constant polynomial 1^ (every word 1) in the NTT domain, [limb][N], and the
 * ciphertext (c0^, c1^) in the NTT domain, the phase c0 + c1 s in coefficients is
 *     ntt_rns_inv_dot_batch(L, plans, d_x, 2, {c0^, c1^}, {1^, s^}, batch, NTT_MUL_B_BROADCAST, stream)
 * and then
 *     BFV    ntt_rns_to_plain_batch(L, plans, d_m, d_x, t, batch, NTT_PLAIN_SCALE, stream)      m = round(t [c0 + c1 s]_Q / Q) mod t
 *     BGV    ntt_rns_to_plain_batch(L, plans, d_m, d_x, t, batch, 0, stream)                    m = [[c0 + c1 s]_Q centred]_t
 *     CKKS   ntt_rns_to_double_batch(L <= 2, plans, d_y, d_x, 1 / Delta, batch, stream)         y = [c0 + c1 s]_Q centred / Delta
 * (examples/rns_decrypt.c).  A ciphertext held in coefficients takes ntt_rns_negacyclic_mul_batch and an addition instead of the dot.
 * Measured (profiles/r18/plain_bench.txt: 50-bit primes, t = 65537, 2^13 / 2^14, ranges over five rounds of alternating processes; the
 * parent's own spread 1.00-1.03): at 1024 polynomials the call runs at 0.49-0.52 (L = 1), 0.63-0.75 (L = 4) and 0.74-0.80 (L = 16) of
 * ntt_copy_probe's rate at the same bytes, both modes alike (0.39-0.76 at 64 polynomials, 5-36 us calls) -- below the 0.86-0.92 of the
 * other element-wise kernels: the waves spend 72-75 % of their cycles issuing or stalled at issue and 25-28 % waiting for memory (the
 * probe: 96 %), about 57 vector instructions per limb and 114 per output word, nearly all of them the 64-bit integer products.  Against
 * the detour the parent commit can express (exact ModUp onto an auxiliary prime, exact ModDown with mult = t, a centred reduction with
 * torch integer ops) the SCALE mode is 8.2-8.9 x (L = 1), 3.7-6.2 x (L = 4) and 2.2-3.6 x (L = 16) faster. ---- */
enum { NTT_PLAIN_SCALE = 1 /* m = round(t x / Q) mod t (BFV) instead of [x_c]_t (BGV) */ };
NTT_API int ntt_rns_to_plain_batch(int nlimbs, ntt_plan *const *plans, uint64_t *d_m, const uint64_t *d_a, uint64_t t, uint64_t batch,
                                   unsigned flags, void *stream);
NTT_API int ntt_rns_to_plain_batch_strided(int nlimbs, ntt_plan *const *plans, uint64_t *d_m, const uint64_t *d_a, uint64_t t,
                                           uint64_t a_limb_stride, uint64_t a_poly_stride, uint64_t m_poly_stride, uint64_t batch,
                                           unsigned flags, void *stream);
NTT_API int ntt_rns_to_double_batch(int nlimbs, ntt_plan *const *plans, double *d_y, const uint64_t *d_a, double scale, uint64_t batch,
                                    void *stream);
NTT_API int ntt_rns_to_double_batch_strided(int nlimbs, ntt_plan *const *plans, double *d_y, const uint64_t *d_a, double scale,
                                            uint64_t a_limb_stride, uint64_t a_poly_stride, uint64_t y_poly_stride, uint64_t batch,
                                            void *stream);

/* ---- into the RNS: the first step of an encryption, and every plaintext operand.  One plaintext word per coefficient ([batch][N])
 * becomes one canonical word per limb in d_c ([limb][batch][N]); any limb count (16 limbs per launch), every q_l < 2^61.  Integer
 * arithmetic only: every definition fixes every output word, on every route (csrc/ntt_lift.h).
 *
 * ntt_rns_from_plain_batch: d_m holds words in [0, t), 2 <= t < 2^61, t ANY integer:
 *     flags = 0 (BGV; plaintext operands of every scheme; a signed integer v passed as v mod t)
 *                              c_l = [m_c]_{q_l},  m_c = m for 2m < t, else m - t: the centred representative, in [-ceil(t/2), t/2).
 *     NTT_LIFT_SCALE (BFV)     c_l = [floor((Q m + floor(t/2)) / t)]_{q_l} = [round(Q m / t)]_{q_l} (ties up), Q the product of the given
 *                              primes, every prime coprime to t.  It is Delta m + floor((r m + floor(t/2)) / t) with Delta = floor(Q / t)
 *                              and r = Q mod t: the rounding term that Delta m alone drops.
 *   A word m >= t is the caller's error: the result word is unspecified, but lies in [0, q_l).
 * ntt_rns_from_double_batch (CKKS): d_y holds doubles; p = fl(y * scale), one IEEE product; v = rint(p), ties to even; c_l = [v]_{q_l}.
 *   v = 0 for NaN, +-inf and |p| >= 2^127 (defined, not a precondition); below that the integer is exact in 128 bits.  What precedes
 *   it is the encoding FFT.
 * Flags:
 *     NTT_LIFT_SCALE         from_plain only (see above)
 *     NTT_LIFT_TRANSFORMED   the output is in the NTT domain, canonical words
 *     NTT_LIFT_ACCUMULATE    c_l <- c_l + the lift (mod q_l); c canonical and in the domain the call writes
 * _strided: d_c's limbs c_limb_stride and polynomials c_poly_stride words apart (any strides the other RNS forms accept), the
 * plaintext's polynomials m_poly_stride (y_poly_stride) >= N words apart.  batch = 1 yields the [limb][N] shape that
 * NTT_LINCOMB_M_BROADCAST and NTT_MUL_B_BROADCAST read.  Any overlap of the plaintext's span of words with d_c's is refused.
 * Routes: coefficients -- one element-wise launch per 16 limbs (every policy, every N >= 2, NTT_OPT_MAX_GRID of plans[0] honoured),
 * 8N(L + 1) bytes per polynomial (8N(2L + 1) accumulating).  NTT_LIFT_TRANSFORMED -- per run of compatible limbs ONE launch of the
 * forward transform with the lift in its prologue and the addition in its epilogue (FP64 policies, N = 2^6..2^14; the plaintext is
 * read once per run, nothing else but the output moves), or the composition: the element-wise launch and the run's forward transform
 * in place; accumulating: the run's inverse transform, the accumulating element-wise launch, the forward transform.  Both give the
 * same words.  NTT_OPT_LIFT_FUSED on plans[0]: 1 / 0 force the fused kernel (where built) / the composition for every run; the
 * default, -1, follows the measurement (profiles/r19/lift_bench.txt; the rule with its figures: csrc/host/host_lift.inc): the fused
 * kernel when accumulating (1.13-2.27 x the composition's rate) and for the centred lift through N = 2^13 (1.06-1.37 x), the
 * composition otherwise (storing, the scaled and double modes and the centred one at 2^14 are 0.73-0.97 x somewhere).
 * Allocates nothing, does not synchronise the host, issues no memset: capturable.
 * NTT_ERR_ARG, nothing written: plans that differ in N or device; a prime >= 2^61; t < 2 or t >= 2^61; NTT_LIFT_SCALE with a prime
 * that divides t, or on from_double; any other flag; a null d_c or plaintext with batch > 0; strides under which two (limb,
 * polynomial) ranges overlap, or a plaintext stride below N; the overlap above; NTT_LIFT_TRANSFORMED with a plan that lacks the
 * forward table (composition with NTT_LIFT_ACCUMULATE: or the inverse table).
 *
 * Recipes (Delta = floor(Q / t) for BFV, the scale for CKKS; pk^ in the NTT domain; u^, e0^, e1^ drawn by ntt_rns_sample_batch below --
 * u^: NTT_SAMPLE_TERNARY with NTT_SAMPLE_TRANSFORMED; + e0^: NTT_SAMPLE_CBD21 with NTT_SAMPLE_TRANSFORMED | NTT_SAMPLE_ACCUMULATE onto
 * pk0^ (.) u^ (BGV: mult = t), each under a seed or a first_poly range of its own -- or sampled by a caller that needs a CSPRNG and
 * uploaded through the lifts):
 *     BFV encrypt    c0^ = pk0^ (.) u^ + e0^ by the products above, then
 *                    ntt_rns_from_plain_batch(L, plans, d_c0, d_m, t, batch, NTT_LIFT_SCALE | NTT_LIFT_TRANSFORMED | NTT_LIFT_ACCUMULATE, s)
 *     BGV encrypt    c0^ = pk0^ (.) u^ + t e0^, then from_plain(.., NTT_LIFT_TRANSFORMED | NTT_LIFT_ACCUMULATE, s)
 *     CKKS encrypt   c0^ likewise, then ntt_rns_from_double_batch(L, plans, d_c0, d_y, Delta, batch, NTT_LIFT_TRANSFORMED | NTT_LIFT_ACCUMULATE, s)
 *     ct + pt        the same call on c0^ (BFV: NTT_LIFT_SCALE; BGV: none; CKKS: from_double)
 *     ct (.) pt      pt^ = from_plain(.., batch = 1, NTT_LIFT_TRANSFORMED) into a [limb][N] buffer, then ntt_rns_lincomb_batch with pt^ as
 *                    a multiplier and NTT_LINCOMB_M_BROADCAST
 * (examples/rns_encrypt.c). ---- */
enum {
  NTT_LIFT_SCALE       = 1, /* from_plain: round(Q m / t) (BFV) instead of the centred [m_c] (BGV, plaintext operands) */
  NTT_LIFT_TRANSFORMED = 2, /* the output is in the NTT domain */
  NTT_LIFT_ACCUMULATE  = 4  /* c_l <- c_l + the lift */
};
NTT_API int ntt_rns_from_plain_batch(int nlimbs, ntt_plan *const *plans, uint64_t *d_c, const uint64_t *d_m, uint64_t t, uint64_t batch,
                                     unsigned flags, void *stream);
NTT_API int ntt_rns_from_plain_batch_strided(int nlimbs, ntt_plan *const *plans, uint64_t *d_c, const uint64_t *d_m, uint64_t t,
                                             uint64_t c_limb_stride, uint64_t c_poly_stride, uint64_t m_poly_stride, uint64_t batch,
                                             unsigned flags, void *stream);
NTT_API int ntt_rns_from_double_batch(int nlimbs, ntt_plan *const *plans, uint64_t *d_c, const double *d_y, double scale, uint64_t batch,
                                      unsigned flags, void *stream);
NTT_API int ntt_rns_from_double_batch_strided(int nlimbs, ntt_plan *const *plans, uint64_t *d_c, const double *d_y, double scale,
                                              uint64_t c_limb_stride, uint64_t c_poly_stride, uint64_t y_poly_stride, uint64_t batch,
                                              unsigned flags, void *stream);

/* ---- random polynomials in the RNS, drawn on the device: secrets, masks and noise of key generation and encryption without a host
 * round trip per polynomial.  d_c ([limb][batch][N]) receives one canonical word per limb and coefficient; nothing is read.  Any limb
 * count (16 limbs per launch), every q_l < 2^61.  Integer arithmetic only: the definition (csrc/ntt_sample.h) fixes every output word
 * on every route.
 *
 * NOT A CRYPTOGRAPHIC GENERATOR: Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3") is a statistical,
 * counter-based generator.  The calls serve reproducible workloads, benchmarks, tests and simulation; a deployment that needs a CSPRNG
 * keeps sampling on its side and uses the lifts above.
 *
 * ONE 128-bit block per output coefficient, independent of layout, batch split, launch chunking and route:
 *     key = (seed & 0xffffffff, seed >> 32),   counter = (s, P & 0xffffffff, P >> 32, tag)
 *   s the coefficient's position in [0, N); P = first_poly + p mod 2^64, p the polynomial's index in the call; tag = the kind for the
 *   small kinds, 2 | (l << 8) for the uniform kind, l the limb's index in plans.  A batch of 5 at first_poly = F is the batch of 2 at F
 *   followed by the batch of 3 at F + 2.  Callers separate u, e0, e1, ... by seed or by disjoint first_poly ranges.  out0..out3: the block.
 *     NTT_SAMPLE_TERNARY   v = mulhi64(out0 | out1 << 32, 3) - 1 in {-1, 0, 1}, each with probability 1/3 within 2^-64
 *     NTT_SAMPLE_CBD21     v = popcount(out0 & 0x1FFFFF) - popcount(out1 & 0x1FFFFF): centred binomial, eta = 21, sigma = sqrt(10.5) = 3.24
 *                          (the HE-standard error width), |v| <= 21
 *                          both: c_l = [mult v]_{q_l}, the SAME v in every limb; 1 <= mult < 2^61 (1: plain noise; t: BGV's t e)
 *     NTT_SAMPLE_UNIFORM   c_l = (out0 | out1 << 32 | out2 << 64 | out3 << 96) mod q_l, the limbs independent through the tag; the bias
 *                          is below 2^-67; mult must be 1.  Uniform is uniform in either domain: NTT_SAMPLE_TRANSFORMED is accepted
 *                          and changes nothing.
 * Flags:
 *     NTT_SAMPLE_TRANSFORMED   the output is in the NTT domain, canonical words (the small kinds: the forward transform of the sample)
 *     NTT_SAMPLE_ACCUMULATE    c_l <- c_l + the sample (mod q_l); c canonical and in the domain the call writes
 * _strided: d_c's limbs c_limb_stride and polynomials c_poly_stride words apart (any strides the other RNS forms accept).
 * Routes: coefficients (and the uniform kind always) -- one element-wise launch per 16 limbs, sample_coef_kernel (every policy, every
 * N >= 2, NTT_OPT_MAX_GRID of plans[0] honoured), 8NL bytes per polynomial (16NL accumulating).  NTT_SAMPLE_TRANSFORMED with a small
 * kind -- per run of compatible limbs ONE launch of the forward transform with the generator in its prologue and the addition in its
 * epilogue (sample_fwd_kernel; FP64 policies, N = 2^6..2^14), or the composition: the element-wise launch and the run's forward
 * transform in place; accumulating: the run's inverse transform, the accumulating element-wise launch, the forward transform.  Both
 * give the same words.  NTT_OPT_SAMPLE_FUSED on plans[0]: 1 / 0 force the fused kernel (where built) / the composition for every run;
 * the default, -1, follows the measurement (profiles/r23/sample_bench.txt; the rule with its figures: csrc/host/host_sample.inc):
 * 2^13 and 2^14, L = 1, 4, 16 of 24 50-bit primes, 64 / 1024 polynomials, composition time / fused time as ranges over five rounds, a
 * figure's own spread 1.00-1.08): the fused kernel when accumulating (1.46-2.34 x the composition's rate) and, storing, for every run of
 * two or more limbs (1.05-1.38 x; 0.98-1.02 x, not different, at 2^14 x 16 limbs x 64 polynomials) and for a single limb at 2^14
 * (1.09-1.44 x); a single-limb run through N = 2^13 stores through the composition (1.47-1.53 x at 1024 polynomials but 0.94-0.97 x at 64).
 * The coefficient kernel reaches 0.28-0.93 (uniform: 0.23-0.74) of ntt_copy_probe's rate at 8NL bytes per polynomial, the fused kernel
 * 0.14-0.49 at its own; against small values drawn with torch and lifted by ntt_rns_from_plain_batch the fused kernel takes
 * 1/1.11-1/2.43 (ternary) and 1/2.27-1/20.4 (centred binomial) of the time.
 * Allocates nothing, does not synchronise the host, issues no memset: capturable.
 * NTT_ERR_ARG, nothing written: plans that differ in N or device; a prime >= 2^61; an unknown kind or flag; mult = 0 or >= 2^61;
 * mult != 1 with the uniform kind; a null d_c with batch > 0; strides under which two (limb, polynomial) ranges overlap;
 * NTT_SAMPLE_TRANSFORMED with a small kind and a plan that lacks the forward table (composition with NTT_SAMPLE_ACCUMULATE: or the
 * inverse table).
 *
 * Recipe, key generation (RLWE):  s^ = sample(TERNARY, NTT_SAMPLE_TRANSFORMED),  a^ = sample(UNIFORM),  then b^ = -a^ (.) s^ + e^:
 *     ntt_rns_lincomb_batch / the NTT-domain products for -a^ (.) s^, then sample(CBD21, NTT_SAMPLE_TRANSFORMED | NTT_SAMPLE_ACCUMULATE)
 * (examples/rns_sample.c). ---- */
enum { NTT_SAMPLE_TERNARY = 0, NTT_SAMPLE_CBD21 = 1, NTT_SAMPLE_UNIFORM = 2 };
enum {
  NTT_SAMPLE_TRANSFORMED = 2, /* the output is in the NTT domain (the NTT_LIFT_* bit values) */
  NTT_SAMPLE_ACCUMULATE  = 4  /* c_l <- c_l + the sample */
};
NTT_API int ntt_rns_sample_batch(int nlimbs, ntt_plan *const *plans, uint64_t *d_c, int kind, uint64_t mult, uint64_t seed,
                                 uint64_t first_poly, uint64_t batch, unsigned flags, void *stream);
NTT_API int ntt_rns_sample_batch_strided(int nlimbs, ntt_plan *const *plans, uint64_t *d_c, int kind, uint64_t mult, uint64_t seed,
                                         uint64_t first_poly, uint64_t c_limb_stride, uint64_t c_poly_stride, uint64_t batch,
                                         unsigned flags, void *stream);

/* ---- BFV / BGV slots: encode and decode, fused with the transform mod t.  Everything above speaks of a plaintext as N coefficients
 * mod t; a BFV / BGV user holds N SLOTS, a 2 x N/2 matrix of values mod t.  pt is a plan for (N, t, psi): t prime, 2N | t - 1, psi its
 * primitive 2N-th root, m = log2 N, h = N / 2.  The forward transform stores a(psi^(2 bitrev_m(s) + 1)) at word s (the fact the
 * NTT-domain Galois formula above rests on).  The convention: generator 5, rows = the sign of the exponent.
 *     slot index   i = r h + j, row r in {0, 1}, column 0 <= j < h
 *     exponent     e(i) = 5^j mod 2N for r = 0,  2N - (5^j mod 2N) for r = 1
 *     position     pos(i) = bitrev_m((e(i) - 1) / 2): a permutation of 0..N-1, the identity for N = 2 (ntt_slot_position)
 *     decode       v[i] = fwd(a)[pos(i)] = a(psi^e(i))
 *     encode       a = inv(a^) with a^[pos(i)] = v[i]: the unique a of degree < N with a(psi^e(i)) = v[i]; decode(encode(v)) = v
 * Consequences: products of polynomials (ntt_negacyclic_mul_batch on pt; the RNS products after a lift) are slot-wise products;
 * sigma_g with g = ntt_galois_rotation(N, r) rotates BOTH rows left by r -- new (row, j) holds the old (row, (j + r) mod h); g = 2N - 1
 * swaps the two rows.
 * ntt_plan_enable_slots builds the two index tables pos and ipos (N uint32_t each) on the device, one thread per slot (5^j by
 * square-and-multiply, ipos by scattering); idempotent; it allocates and synchronises, so call it outside stream capture; the tables
 * are freed with the plan, and a plan that never calls it costs nothing more.  ntt_slot_position(N, i) is pos(i) on the host
 * (UINT64_MAX for an N that is no power of two >= 2, or i >= N).
 * ntt_slots_encode_batch: d_a ([batch][N] coefficients) = encode(d_v ([batch][N] slots)); d_v is left untouched.
 * ntt_slots_decode_batch: d_v = decode(d_a).  It CONSUMES d_a: on return its words are unspecified (the fused route leaves them, the
 * composition has transformed them in place).  Words are canonical in [0, t) on both sides (unchecked).  flags must be 0.
 * _strided: the slot side's polynomials v_poly_stride and the coefficient side's a_poly_stride words apart, each >= N.
 * Routes (identical words; NTT_OPT_SLOTS_FUSED on pt selects):
 *     fused        FP64 policies, N = 2^6..2^14, ONE launch: slots_inv_kernel -- the inverse block stages, each lane loading v[ipos[s]]
 *                  for the positions s it would have loaded --, slots_fwd_kernel -- the forward block stages storing word s to
 *                  v[ipos[s]].  One polynomial is one workgroup, so every gathered or scattered line is in that workgroup's own
 *                  <= 128 KiB; the 4N-byte table is shared by the batch.  16N bytes per polynomial.
 *     composition  every policy, every N >= 2 (N < 2^6, N >= 2^15, NTT_ARITH_U64 plans for t >= 2^52): the element-wise
 *                  slots_perm_kernel (out[p][s] = in[p][tab[s]]) and the plan's transform in place on d_a.  32N bytes.
 * The default (-1) follows the measurement (profiles/r21/slots_bench.txt, t = 65537, 2^13 / 2^14, 64 / 1024 polynomials, composition
 * time / fused time as ranges over five alternating rounds, a figure's own spread 1.00-1.04; the rule with its figures:
 * csrc/host/host_slots.inc): encode is fused wherever built (1.40-1.61 at 64 polynomials, 2.33-2.39 at 1024); decode is fused through
 * 2^13 (1.19-1.20 / 1.84-1.86) and composed at 2^14 (1.30-1.33 at 64, but 0.96-0.98 at 1024: the scattered stores of a full chip cost
 * more than the launch they save).  Against the detour a caller had before (a torch gather with an index tensor of its own around
 * ntt_inv_batch / ntt_fwd_batch) the fused calls take 1/1.15-1/3.92 of the time.  They reach 0.15-0.40 of ntt_copy_probe's rate at
 * 16N bytes per polynomial (the composition 0.12-0.25).
 * NTT_OPT_MAX_GRID of pt is honoured.  Allocate nothing, do not synchronise the host, issue no memset: capturable.
 * NTT_ERR_ARG, nothing written: a plan without slot tables; a plan that lacks the inverse (encode) or forward (decode) table; a null
 * pointer with batch > 0; a stride below N; any overlap of the two spans of words; any flag.  batch = 0 is NTT_OK.
 *
 * Recipes (BGV; BFV with NTT_LIFT_SCALE / NTT_PLAIN_SCALE):
 *     slots -> plaintext operand   ntt_slots_encode_batch(pt, d_m, d_v, batch, 0, s), then ntt_rns_from_plain_batch(L, plans, d_c, d_m, t, ..)
 *     decryption -> slots          ntt_rns_to_plain_batch(L, plans, d_m, d_a, t, ..), then ntt_slots_decode_batch(pt, d_v, d_m, batch, 0, s)
 * (examples/rns_slots.c). ---- */
NTT_API int      ntt_plan_enable_slots(ntt_plan *p);
NTT_API uint64_t ntt_slot_position(uint64_t N, uint64_t i);
NTT_API int ntt_slots_encode_batch(const ntt_plan *pt, uint64_t *d_a, const uint64_t *d_v, uint64_t batch, unsigned flags, void *stream);
NTT_API int ntt_slots_encode_batch_strided(const ntt_plan *pt, uint64_t *d_a, const uint64_t *d_v, uint64_t v_poly_stride,
                                           uint64_t a_poly_stride, uint64_t batch, unsigned flags, void *stream);
NTT_API int ntt_slots_decode_batch(const ntt_plan *pt, uint64_t *d_v, uint64_t *d_a, uint64_t batch, unsigned flags, void *stream);
NTT_API int ntt_slots_decode_batch_strided(const ntt_plan *pt, uint64_t *d_v, uint64_t *d_a, uint64_t v_poly_stride, uint64_t a_poly_stride,
                                           uint64_t batch, unsigned flags, void *stream);

/* ---- caller-native layouts (round 5).  The entry points above take RNS operands as [limb][batch][N].  SURVEY 8(d) config 5
 * -- and every FHE library -- keeps a polynomial's limbs side by side: [batch][prime][N].  The *_strided forms take the two
 * distances in WORDS instead of assuming either:
 *     coefficient i of limb l of polynomial p  =  d_x[l * limb_stride + p * poly_stride + i]
 *   [limb][batch][N]:  limb_stride = batch * N, poly_stride = N           (what the plain entry points pass)
 *   [batch][limb][N]:  limb_stride = N,         poly_stride = nlimbs * N  (no transpose on either side of the call)
 * Padded variants of either are accepted; strides under which two (limb, polynomial) ranges would overlap are refused
 * (NTT_ERR_ARG).  All operands of one call (a, b, c, every a_i^ / b_i^) share the layout; a broadcast b^ (NTT_MUL_B_BROADCAST) stays
 * [limb][N].  Same kernels, same launch choices (one launch over the limbs where it pays, the XCD-local launches for large
 * batches of N >= 2^15), same results: the layout is one address computation per block (csrc/ntt_core.h block_offset).
 * The reference's own batching precedent is two caller arrays side by side, fwd_ntt_ref_harvey_lazy_dbl(a1[], a2[], ...)
 * (include/ntt_reference.h:44-49, src/ntt_reference.c:71-91); these generalise it to any regular placement. ---- */
NTT_API int ntt_rns_fwd_batch_strided(int nlimbs, ntt_plan *const *plans, uint64_t *d_a, uint64_t limb_stride, uint64_t poly_stride,
                                      uint64_t batch, void *stream);
NTT_API int ntt_rns_inv_batch_strided(int nlimbs, ntt_plan *const *plans, uint64_t *d_a, uint64_t limb_stride, uint64_t poly_stride,
                                      uint64_t batch, void *stream);
NTT_API int ntt_rns_negacyclic_mul_batch_strided(int nlimbs, ntt_plan *const *plans, uint64_t *d_c, uint64_t *d_a, uint64_t *d_b,
                                                 uint64_t limb_stride, uint64_t poly_stride, uint64_t batch, void *stream);
NTT_API int ntt_rns_inv_dot_batch_strided(int nlimbs, ntt_plan *const *plans, uint64_t *d_c, int k, const uint64_t *const *d_ahat,
                                          const uint64_t *const *d_bhat, uint64_t limb_stride, uint64_t poly_stride, uint64_t batch,
                                          unsigned flags, void *stream);
NTT_API int ntt_rns_mul_transformed_batch_strided(int nlimbs, ntt_plan *const *plans, uint64_t *d_c, uint64_t *d_a, const uint64_t *d_bhat,
                                                  uint64_t limb_stride, uint64_t poly_stride, uint64_t batch, unsigned flags, void *stream);
NTT_API int ntt_rns_fwd_mul_batch_strided(int nlimbs, ntt_plan *const *plans, uint64_t *d_c, uint64_t *d_a, const uint64_t *d_bhat,
                                          uint64_t limb_stride, uint64_t poly_stride, uint64_t batch, unsigned flags, void *stream);
/* one plan, `batch` polynomials poly_stride words apart (one limb of a [batch][limb][N] operand; a column of a caller's
 * matrix of polynomials): ntt_transform_batch with a stride */
NTT_API int ntt_transform_batch_strided(const ntt_plan *p, uint64_t *d_a, uint64_t poly_stride, uint64_t batch, unsigned flags,
                                        void *stream);

/* ---- pointer batches: one DEVICE pointer per polynomial.  The reference's own batch form is one array per polynomial --
 * fwd_ntt_ref_harvey_lazy_dbl(a1[], a2[], ...) (include/ntt_reference.h:44-49, src/ntt_reference.c:71-91) --; this is that form for
 * `count` polynomials resident on the device and placed ANYWHERE: ONE launch chain serves the whole batch, the kernels read each
 * polynomial's address from a device table (separately allocated ciphertexts, a shuffled pool, rows of several matrices: 4096
 * separately held 2^14-point polynomials run at the rate of one contiguous slab; rounds 1-5 launched every arithmetic progression
 * of the sorted pointers by itself).  Pointers must be 8-byte aligned.  flags = NTT_FLAG_*.
 *   ntt_transform_ptrs      h_polys is a HOST array.  The polynomials are independent and transformed in place, so the call is free
 *                           to reorder them: the pointers are sorted (address order), checked -- overlapping polynomials or a pointer
 *                           listed twice are refused, NTT_ERR_ARG -- and uploaded through a pinned staging buffer the plan keeps per
 *                           stream (asynchronous; its first use on a stream allocates).  A batch that is one arithmetic progression
 *                           takes the strided launch, no table.  While `stream` is being captured into a HIP graph nothing can be
 *                           uploaded: the call then launches progression by progression (no regularity: one launch chain per
 *                           polynomial) -- in graphs use
 *   ntt_transform_dev_ptrs  d_polys is a DEVICE array of `count` device pointers, used as it is: no copy, no allocation, no check
 *                           (overlapping polynomials are the caller's responsibility), capturable; it must stay valid and unchanged
 *                           until the call's kernels have run.
 * ntt_rns_transform_ptrs / _dev_ptrs: entry i points at limb 0 of RNS polynomial i, whose limbs are limb_stride words apart ([limb][N]
 * per polynomial: limb_stride = N; pointers INTO a [limb][batch][N] slab: limb_stride = batch * N -- the polynomials then interleave
 * without overlapping, which the host form's check, made limb image by limb image, accepts); flags: NTT_FLAG_INVERSE only. ---- */
NTT_API int ntt_transform_ptrs(const ntt_plan *p, uint64_t *const *h_polys, uint64_t count, unsigned flags, void *stream);
NTT_API int ntt_transform_dev_ptrs(const ntt_plan *p, const uint64_t *const *d_polys, uint64_t count, unsigned flags, void *stream);
NTT_API int ntt_rns_transform_ptrs(int nlimbs, ntt_plan *const *plans, uint64_t *const *h_polys, uint64_t count, uint64_t limb_stride,
                                   unsigned flags, void *stream);
NTT_API int ntt_rns_transform_dev_ptrs(int nlimbs, ntt_plan *const *plans, const uint64_t *const *d_polys, uint64_t count,
                                       uint64_t limb_stride, unsigned flags, void *stream);

/* ---- products over pointer batches (round 6).  Every operand is a DEVICE array of `count` device pointers (entry p = polynomial p of
 * that operand; RNS: its limb 0, the limbs limb_stride words apart), taken as it is: no copy, no overlap check, capturable.
 * Up to N = 2^14 the fused product kernels read every operand through its own table: ONE launch per call and limb at the slab forms'
 * bytes (24N for c = a * b, (2k + 1) 8N for an inner product of k pairs, 24N / 32N for fwd(a) (.) b^ (+ c^)) -- measured 0.84-1.14 x the
 * rate of the same product over contiguous slabs (profiles/r06/pointer_products.txt).  fwd(a) (.) b^ at 2^15 takes the one-pass kernel
 * the same way, and at 2^15..2^17 the XCD-local one-launch kernels read the tables from 64 polynomials on (they need the plan's control
 * block: ntt_plan_reserve before capturing such a call into a graph).  Smaller batches of those sizes, and plans the fused kernels are
 * not built for, run the element-wise products as a table-reading kernel of their own and the transforms over the tables: k + 1 launch
 * chains per call whatever the batch.  The ntt_rns_* twins: a run of compatible limbs (as for the slab forms: same policy and size
 * class; up to 16) whose per-limb share cannot fill the chip -- a few ciphertext polynomials x many primes -- goes out as ONE launch of
 * the fused kernels over all of its limbs up to N = 2^14 (the limb an index of the grid; NTT_OPT_RNS_LAUNCH 0 / 1 forces the
 * one-launch / the per-limb form; large batches up to 2^14 take one launch per limb); above 2^14 a run is ONE XCD-local launch from 64
 * polynomials x limbs on (the limb part of the queue entry) and one chain over all of its limbs below that.  Semantics, flags and operand ranges
 * are those of the slab forms:
 *   ntt_inv_dot_dev_ptrs         c_p = inv( sum_{i<k} a_{i,p}^ (.) b_{i,p}^ ); h_ahat / h_bhat: HOST arrays of k device tables;
 *                                NTT_MUL_B_BROADCAST: h_bhat[i] is a device pointer to ONE polynomial (RNS: [limb][N]); k = 1: c's table
 *                                may be an operand's
 *   ntt_fwd_mul_dev_ptrs         c_p^ = fwd(a_p) (.) b_p^ (NTT_MUL_ACCUMULATE: += ...); a is SCRATCH: left as it was where a fused kernel
 *                                serves (up to 2^14; 2^15 in one pass), overwritten otherwise
 *   ntt_negacyclic_mul_dev_ptrs  c_p = a_p * b_p; a and b are SCRATCH: left as they were by the one-launch form up to 2^14 (FP64 plans),
 *                                overwritten otherwise; c's table may be a's or b's (the table itself, entry for entry -- not a
 *                                permutation of it); d_a == d_b squares ---- */
NTT_API int ntt_inv_dot_dev_ptrs(const ntt_plan *p, const uint64_t *const *d_c, int k, const uint64_t *const *const *h_ahat,
                                 const uint64_t *const *const *h_bhat, uint64_t count, unsigned flags, void *stream);
NTT_API int ntt_fwd_mul_dev_ptrs(const ntt_plan *p, const uint64_t *const *d_c, const uint64_t *const *d_a, const uint64_t *const *d_bhat,
                                 uint64_t count, unsigned flags, void *stream);
NTT_API int ntt_negacyclic_mul_dev_ptrs(const ntt_plan *p, const uint64_t *const *d_c, const uint64_t *const *d_a, const uint64_t *const *d_b,
                                        uint64_t count, void *stream);
NTT_API int ntt_rns_inv_dot_dev_ptrs(int nlimbs, ntt_plan *const *plans, const uint64_t *const *d_c, int k, const uint64_t *const *const *h_ahat,
                                     const uint64_t *const *const *h_bhat, uint64_t count, uint64_t limb_stride, unsigned flags, void *stream);
NTT_API int ntt_rns_fwd_mul_dev_ptrs(int nlimbs, ntt_plan *const *plans, const uint64_t *const *d_c, const uint64_t *const *d_a,
                                     const uint64_t *const *d_bhat, uint64_t count, uint64_t limb_stride, unsigned flags, void *stream);
NTT_API int ntt_rns_negacyclic_mul_dev_ptrs(int nlimbs, ntt_plan *const *plans, const uint64_t *const *d_c, const uint64_t *const *d_a,
                                            const uint64_t *const *d_b, uint64_t count, uint64_t limb_stride, void *stream);

/* ---- device memory / streams / timing (thin HIP wrappers for C callers) ---- */
NTT_API int ntt_dev_malloc(int device, void **d_ptr, size_t bytes);
NTT_API int ntt_dev_free(int device, void *d_ptr);
NTT_API int ntt_dev_mem_info(int device, size_t *free_bytes, size_t *total_bytes); /* hipMemGetInfo */
NTT_API int ntt_h2d(int device, void *d_dst, const void *h_src, size_t bytes);
NTT_API int ntt_d2h(int device, void *h_dst, const void *d_src, size_t bytes);
NTT_API int ntt_stream_create(int device, void **stream); /* hipStreamNonBlocking: does NOT synchronise with the null stream (ntt_h2d / ntt_d2h are blocking copies on the null stream: ntt_stream_sync first) */
NTT_API int ntt_stream_destroy(int device, void *stream);
NTT_API int ntt_stream_sync(int device, void *stream);
NTT_API int ntt_event_create(int device, void **event);
NTT_API int ntt_event_destroy(int device, void *event);
NTT_API int ntt_event_record(int device, void *event, void *stream);
NTT_API int ntt_event_elapsed_ms(int device, void *start, void *stop, float *ms); /* syncs stop */

/* ---- synthetic data and digests, device side ----
 * d_a[i] = splitmix64(seed ^ (offset + i)) mod q : the same function as the
 * oracle's orc_fill_uniform, so a host can regenerate any sampled polynomial */
NTT_API int ntt_fill_uniform(int device, uint64_t *d_a, uint64_t n, uint64_t q, uint64_t seed,
                             uint64_t offset, void *stream);
/* d_out[p] = sum_i splitmix64(i) * d_a[p*N+i]  (mod 2^64): position-sensitive
 * per-polynomial checksum for full-size parity checks */
NTT_API int ntt_poly_checksum(int device, uint64_t *d_out, const uint64_t *d_a, uint64_t N,
                              uint64_t batch, void *stream);
/* measured ceiling of the transform's memory shape (SURVEY 8d "fraction of a measured copy-kernel ceiling"):
 * every 16 bytes of d_a[0..n) are read, XORed with mask and written back in place by a plain grid-stride kernel
 * -- no arithmetic, no LDS, the same 8 B in + 8 B out per coefficient as an in-place NTT.  mask = 0 leaves the
 * data unchanged.  n must be even. */
NTT_API int ntt_rmw_probe(int device, uint64_t *d_a, uint64_t n, uint64_t mask, void *stream);
/* out-of-place copy of n words (16 bytes per lane, grid-stride): the copy shape the microarchitecture guide quotes the achievable
 * HBM rate for (about 6.3 TB/s of read + written bytes); 2 x 8 x n bytes move.  n must be even. */
NTT_API int ntt_copy_probe(int device, uint64_t *d_dst, const uint64_t *d_src, uint64_t n, void *stream);
/* the same measurement in the memory shape of the 2^14 block kernels themselves: one persistent 1024-thread workgroup per CU,
 * 2^14-word blocks as 16-byte loads with the next block prefetched in registers, XOR, 16-byte stores (whole KiB per wave and
 * instruction) -- the best memory-only skeleton of the transform kernels (profiles/r02/skeleton.txt), measured in the run
 * that quotes it.  n must be a multiple of 2^14. */
NTT_API int ntt_shape_probe(int device, uint64_t *d_a, uint64_t n, uint64_t mask, void *stream);

/* ---- multi-GPU: one call drives every listed device (per-device streams, no
 * collective -- polynomials are independent).  plans[g], d_a[g] and
 * batch[g] describe the shard resident on plans[g]'s device; the call returns
 * when all shards are done.  inverse != 0 selects the inverse transform. */
NTT_API int ntt_batch_multi(int ndev, ntt_plan *const *plans, uint64_t *const *d_a,
                            const uint64_t *batch, int inverse);
/* the same for RNS products c = a * b (BASELINE config 5 on several GPUs): plans[g * nlimbs + l] is limb l's plan on
 * shard g's device; d_c[g], d_a[g], d_b[g] are that shard's [limb][batch[g]][N] slabs (aliasing rules of
 * ntt_rns_negacyclic_mul_batch) */
NTT_API int ntt_rns_mul_multi(int ndev, int nlimbs, ntt_plan *const *plans, uint64_t *const *d_c, uint64_t *const *d_a,
                              uint64_t *const *d_b, const uint64_t *batch);

/* ---- reference-signature entry points: housekeeping ----
 * The single-polynomial functions of ntt_reference.h / ntt_radix4.h / ntt_radix4x4.h / ntt_seal.h keep
 * device tables for the caller tables they have seen (keyed on a hash of every entry, at most 32 plans,
 * least recently used evicted) and one staging buffer.  ntt_compat_release() frees all of it. */
NTT_API void ntt_compat_release(void);
NTT_API int  ntt_compat_cached_plans(void);

/* ---- parameter helpers (reference: SageMath script, tests/test_cases.h:113-142) ---- */
/* smallest primitive 2N-th root of unity mod q ("minimum root" rule); 0 if none */
NTT_API uint64_t ntt_min_root(uint64_t q, uint64_t N);
/* skip-th largest prime p < 2^bits with p = 1 (mod 2N); 0 if none */
NTT_API uint64_t ntt_find_prime(unsigned bits, uint64_t N, unsigned skip);

#ifdef __cplusplus
}
#endif
#endif /* NTT_MI355X_H */
