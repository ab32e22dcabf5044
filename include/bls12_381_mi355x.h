/*
 * bls12_381_mi355x.h -- C ABI of the MI355X (gfx950) BLS12-381 prover hot path.
 *
 * This is the drop-in boundary.  Every entry point below replaces one exported by the
 * reference backend (riusricardo/midnight-bls12-381-cuda, bls12-381/src/...) with the same
 * name, argument meaning and error behaviour; the citation on each declaration is the
 * reference definition it replaces.  Plain C: pointers, sizes, POD config structs, no C++ or
 * torch types.  Streams are hipStream_t passed as void* (NULL = the default stream).
 *
 * Byte layouts (identical to blst / the reference, little-endian u64 limbs):
 *   Fr          32 B   canonical, Montgomery (R = 2^256) unless a flag says standard
 *   Fq          48 B   canonical, Montgomery (R = 2^384)
 *   G1 affine   96 B   x || y;             identity = all zero
 *   G2 affine  192 B   x.c0||x.c1||y.c0||y.c1; identity = all zero
 *   G1 proj.   144 B   X || Y || Z          (meaning depends on the entry point, see below)
 *   G2 proj.   288 B
 */
#ifndef BLS12_381_MI355X_H
#define BLS12_381_MI355X_H

#include <stddef.h>
#include <stdint.h>
#include <stdbool.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------ */
/* errors: ICICLE v4 numbering (reference include/icicle/errors.h:37-52).  The reference's
 * own icicle_types.cuh:47-63 renumbers UNKNOWN_ERROR to 999; we follow real ICICLE.       */
/* ------------------------------------------------------------------------------------ */
typedef enum {
    MBLS_SUCCESS = 0,
    MBLS_INVALID_DEVICE = 1,
    MBLS_OUT_OF_MEMORY = 2,
    MBLS_INVALID_POINTER = 3,
    MBLS_ALLOCATION_FAILED = 4,
    MBLS_DEALLOCATION_FAILED = 5,
    MBLS_COPY_FAILED = 6,
    MBLS_SYNCHRONIZATION_FAILED = 7,
    MBLS_STREAM_CREATION_FAILED = 8,
    MBLS_STREAM_DESTRUCTION_FAILED = 9,
    MBLS_API_NOT_IMPLEMENTED = 10,
    MBLS_INVALID_ARGUMENT = 11,
    MBLS_BACKEND_LOAD_FAILED = 12,
    MBLS_LICENSE_CHECK_ERROR = 13,
    MBLS_UNKNOWN_ERROR = 14
} eIcicleError;

/* ------------------------------------------------------------------------------------ */
/* element types (opaque byte containers with the layouts above)                         */
/* ------------------------------------------------------------------------------------ */
typedef struct { uint64_t limbs[4]; } mbls_fr_t;
typedef struct { uint64_t limbs[6]; } mbls_fq_t;
typedef struct { mbls_fq_t c0, c1; } mbls_fq2_t;
typedef struct { mbls_fq_t x, y; } mbls_g1_affine_t;
typedef struct { mbls_fq_t x, y, z; } mbls_g1_projective_t;
typedef struct { mbls_fq2_t x, y; } mbls_g2_affine_t;
typedef struct { mbls_fq2_t x, y, z; } mbls_g2_projective_t;

/* ------------------------------------------------------------------------------------ */
/* configs: byte-compatible with ICICLE v4 (reference icicle_types.cuh:102-201)           */
/* ------------------------------------------------------------------------------------ */
typedef enum { MBLS_NTT_FORWARD = 0, MBLS_NTT_INVERSE = 1 } NTTDir;   /* icicle_types.cuh:83-86 */
typedef enum {                                                      /* icicle_types.cuh:88-95 */
    MBLS_ORDERING_NN = 0, MBLS_ORDERING_NR = 1, MBLS_ORDERING_RN = 2,
    MBLS_ORDERING_RR = 3, MBLS_ORDERING_NM = 4, MBLS_ORDERING_MN = 5
} Ordering;

/* MSMConfig -- icicle_types.cuh:155-169 */
typedef struct {
    void* stream;
    int precompute_factor;
    int c;                            /* window bits, 0 = auto                         */
    int bitsize;                      /* scalar bits, 0 = 255                          */
    int batch_size;                   /* number of MSMs (scalars/results are batched)   */
    bool are_points_shared_in_batch;
    bool are_scalars_on_device;
    bool are_scalars_montgomery_form;
    bool are_points_on_device;
    bool are_points_montgomery_form;
    bool are_results_on_device;
    bool is_async;
    void* ext;
} MSMConfig;

/* NTTConfig<Fr> -- icicle_types.cuh:102-113 (coset_gen is a 32-byte Fr) */
typedef struct {
    void* stream;
    mbls_fr_t coset_gen;
    int batch_size;
    bool columns_batch;
    Ordering ordering;
    bool are_inputs_on_device;
    bool are_outputs_on_device;
    bool is_async;
    void* ext;
} NTTConfig;

/* NTTInitDomainConfig -- icicle_types.cuh:136-140 */
typedef struct {
    void* stream;
    bool is_async;
    void* ext;
} NTTInitDomainConfig;

/* VecOpsConfig -- ICICLE v4 layout (icicle_types.cuh:194-201 plus v4's batch fields,
 * which core/vecops.rs:346 sets) */
typedef struct {
    void* stream;
    bool is_a_on_device;
    bool is_b_on_device;
    bool is_result_on_device;
    bool is_async;
    int batch_size;
    bool columns_batch;
    void* ext;
} VecOpsConfig;

MSMConfig mbls_default_msm_config(void);
NTTConfig mbls_default_ntt_config(void);
VecOpsConfig mbls_default_vec_ops_config(void);

/* ------------------------------------------------------------------------------------ */
/* MSM                                                                                    */
/* ------------------------------------------------------------------------------------ */
/* Every MSM entry below splits its scalars with the endomorphisms (G1: phi = [lambda], G2:
 * psi = [z]); both identities hold only on the order-r subgroup, so the bases are ASSUMED to lie
 * in it (not checked here; see mbls_g*_check_points).                                       */
/* Raw kernel-level MSM, reference icicle_curve_api.cu:679-705 (bls12_381_g1_msm_cuda /
 * bls12_381_g2_msm_cuda -> msm::msm_cuda, msm_kernels.cu:603-903):
 *   scalars STANDARD form, bases Montgomery affine, result = Jacobian Montgomery point
 *   (identity: Z = 0).  Host/device placement from config->are_*_on_device.           */
eIcicleError bls12_381_g1_msm_cuda(const mbls_fr_t* scalars, const mbls_g1_affine_t* bases, int msm_size,
                                   const MSMConfig* config, mbls_g1_projective_t* result);
eIcicleError bls12_381_g2_msm_cuda(const mbls_fr_t* scalars, const mbls_g2_affine_t* bases, int msm_size,
                                   const MSMConfig* config, mbls_g2_projective_t* result);

/* ICICLE-registered MSM semantics, reference icicle_curve_api.cu:243-407 (msm_cuda_impl) and
 * :454-618 (msm_g2_cuda_impl): honours are_scalars_montgomery_form /
 * are_points_montgomery_form, returns ICICLE standard-form projective (x, y, 1) with
 * identity (0, 1, 0).  batch_size > 1 computes batch_size MSMs (the reference silently
 * computes only the first, SURVEY.md finding 3): scalars are batch_size*msm_size, bases are
 * msm_size (shared) or batch_size*msm_size, results batch_size.                          */
eIcicleError bls12_381_icicle_g1_msm(const mbls_fr_t* scalars, const mbls_g1_affine_t* bases, int msm_size,
                                     const MSMConfig* config, mbls_g1_projective_t* results);
eIcicleError bls12_381_icicle_g2_msm(const mbls_fr_t* scalars, const mbls_g2_affine_t* bases, int msm_size,
                                     const MSMConfig* config, mbls_g2_projective_t* results);

/* precompute_bases, reference icicle_curve_api.cu:415-440 (there a plain byte copy, so its
 * factor > 1 gives wrong MSMs).  Here factor F = config->precompute_factor in 1..64 writes the
 * point-major table out[i*F + f] = 2^(s*f) * P_i with s = ceil(256 / F) (core/msm.rs:164-165):
 * the shift depends on F only, so ONE table serves MSMs of any c (config->c is ignored here)
 * and any msm_size <= bases_size.  Output: Montgomery affine; standard-form input
 * (are_points_montgomery_form = false) is converted first.  An MSM with precompute_factor
 * F > 1 reads such a table (n*F entries, the full buffer may be passed) and treats it as
 * Montgomery whatever are_points_montgomery_form says -- core/msm.rs:641-643 passes false
 * with a precomputed table.                                                               */
eIcicleError bls12_381_icicle_g1_msm_precompute_bases(const mbls_g1_affine_t* input_bases, int bases_size,
                                                      const MSMConfig* config, mbls_g1_affine_t* output_bases);
eIcicleError bls12_381_icicle_g2_msm_precompute_bases(const mbls_g2_affine_t* input_bases, int bases_size,
                                                      const MSMConfig* config, mbls_g2_affine_t* output_bases);

/* ------------------------------------------------------------------------------------ */
/* NTT (reference ntt_kernels.cu:1907-1943, icicle_field_api.cu:363-383)                  */
/* Semantics follow the CPU path (core/ntt.rs:1488-1603, best_fft): forward
 * out_j = sum_i in_i w^(ij), inverse = n^-1 sum_j in_j w^(-ij), w = ROOT_OF_UNITY^(2^(32-k))
 * for size 2^k, natural order in and out (kNN).
 * Input contract: every input element is canonical (< r, Montgomery form).  The transform keeps
 * lazy values in [0, 2r) and its first butterflies add the raw inputs, so a larger value breaks
 * that invariant and the result is unspecified; outputs are always canonical.  A coset generator
 * (NTTConfig.coset_gen, or the argument of bls12_381_coset_ntt_cuda) that is zero mod r -- a
 * zero-initialised NTTConfig -- is rejected with INVALID_ARGUMENT; Montgomery one means no coset. */
/* ------------------------------------------------------------------------------------ */
eIcicleError bls12_381_ntt_init_domain_cuda(const mbls_fr_t* root_of_unity, const NTTInitDomainConfig* config);
eIcicleError bls12_381_ntt_release_domain_cuda(void);
eIcicleError bls12_381_ntt_cuda(const mbls_fr_t* input, int size, NTTDir dir, const NTTConfig* config,
                                mbls_fr_t* output);
eIcicleError bls12_381_coset_ntt_cuda(const mbls_fr_t* input, int size, NTTDir dir, const mbls_fr_t* coset_gen,
                                      const NTTConfig* config, mbls_fr_t* output);
eIcicleError bls12_381_field_ntt_cuda(const mbls_fr_t* input, int size, NTTDir dir, const NTTConfig* config,
                                      mbls_fr_t* output);
eIcicleError bls12_381_field_ntt_init_domain_cuda(const mbls_fr_t* root_of_unity, const NTTInitDomainConfig* config);
eIcicleError bls12_381_field_ntt_release_domain_cuda(void);
/* w_(2^logn) of the initialised domain (Montgomery); INVALID_ARGUMENT without a domain or past
 * its order.  Backs ICICLE's NttGetRouFromDomainImpl (icicle_backend_api.cuh:135-138). */
eIcicleError bls12_381_ntt_get_rou_from_domain(uint64_t logn, mbls_fr_t* rou);

/* ------------------------------------------------------------------------------------ */
/* vecops (reference vec_ops.cu:393-524 and :693-840; icicle_field_api.cu:194-334)        */
/* raw-limb semantics: add/sub representation-agnostic, mul = Montgomery product.         */
/* ------------------------------------------------------------------------------------ */
eIcicleError bls12_381_vector_add(const mbls_fr_t* a, const mbls_fr_t* b, size_t size, const VecOpsConfig* config,
                                  mbls_fr_t* output);
eIcicleError bls12_381_vector_sub(const mbls_fr_t* a, const mbls_fr_t* b, size_t size, const VecOpsConfig* config,
                                  mbls_fr_t* output);
eIcicleError bls12_381_vector_mul(const mbls_fr_t* a, const mbls_fr_t* b, size_t size, const VecOpsConfig* config,
                                  mbls_fr_t* output);
/* scalar_{mul,add}_vec: `scalar` is ONE element on the host unless config->is_a_on_device
 * (icicle_field_api.cu:227-334). */
eIcicleError bls12_381_scalar_mul_vec(const mbls_fr_t* scalar, const mbls_fr_t* vec, size_t size,
                                      const VecOpsConfig* config, mbls_fr_t* output);
eIcicleError bls12_381_scalar_add_vec(const mbls_fr_t* scalar, const mbls_fr_t* vec, size_t size,
                                      const VecOpsConfig* config, mbls_fr_t* output);
/* device-pointer kernel entry points, vec_ops.cu:393-476 (output first, device pointers;
 * `scalar` is a HOST pointer to one element as in the reference). */
eIcicleError vec_add_cuda(mbls_fr_t* output, const mbls_fr_t* a, const mbls_fr_t* b, int size, const VecOpsConfig* config);
eIcicleError vec_sub_cuda(mbls_fr_t* output, const mbls_fr_t* a, const mbls_fr_t* b, int size, const VecOpsConfig* config);
eIcicleError vec_mul_cuda(mbls_fr_t* output, const mbls_fr_t* a, const mbls_fr_t* b, int size, const VecOpsConfig* config);
eIcicleError scalar_mul_vec_cuda(mbls_fr_t* output, const mbls_fr_t* scalar, const mbls_fr_t* vec, int size,
                                 const VecOpsConfig* config);
eIcicleError scalar_add_vec_cuda(mbls_fr_t* output, const mbls_fr_t* scalar, const mbls_fr_t* vec, int size,
                                 const VecOpsConfig* config);
/* sum of `size` device elements; output on device or host per config->is_result_on_device.
 * Replaces vec_sum_cuda (vec_ops.cu:479-524; the reference takes `const VecOpsConfig&`). */
eIcicleError vec_sum_cuda(mbls_fr_t* output, const mbls_fr_t* input, int size, const VecOpsConfig* config);
/* element-wise inverses (0 -> 0), device pointers, in place allowed.  Replaces the C++
 * template vec_ops::batch_inv_cuda<Fr> (vec_ops.cu:606-673); a C symbol here. */
eIcicleError bls12_381_batch_inv_cuda(mbls_fr_t* output, const mbls_fr_t* input, int size, const VecOpsConfig* config);

/* ------------------------------------------------------------------------------------ */
/* Fr prefix scans along a column: the grand product of the permutation and lookup arguments, and
 * polynomial evaluation with division by X - z (KZG openings).  (No reference counterpart: the
 * reference computes these on the CPU -- compute_product, eval_polynomial, kate_division -- and
 * uploads the column afterwards.)
 *   elements: Montgomery and canonical (< r), in and out; z and init likewise.  init == NULL means
 *     Montgomery one.
 *   batch: config->batch_size members (0 counts as 1), row-major, each of `size` elements; z, init,
 *     total and eval hold one element per member.  columns_batch gives API_NOT_IMPLEMENTED, as
 *     bls12_381_vector_sum does.
 *   zero denominators: the inverse of 0 is 0, as in bls12_381_batch_inv_cuda, so a zero in num or
 *     in den makes every later product of that member 0.
 *   placement: config->is_a_on_device num and den (or coeffs), is_b_on_device init (or z),
 *     is_result_on_device output and total (or quotient and eval).  Host buffers are staged through
 *     the leased scratch context, which also holds the work arrays (no allocation per call once it
 *     is large enough); a host result makes the call synchronous, otherwise it synchronises unless
 *     is_async.
 *   optional outputs: total may be NULL, output may not.  Either of quotient and eval may be NULL,
 *     not both; quotient == NULL is pure evaluation and writes no vector.
 *   in place: output may equal num or den, quotient may equal coeffs (the same pointer); any other
 *     overlap is undefined.
 *   errors, before any device work: INVALID_POINTER for a null num / coeffs, z, config or a missing
 *     required output (the vecops' convention); INVALID_ARGUMENT for size == 0 or
 *     size * batch > 2^26.
 *   timing: no branch and no address depends on a field value; the denominators go through the
 *     fixed Fermat chain with mask selects for zeros, as in bls12_381_batch_inv_cuda.            */
/* ------------------------------------------------------------------------------------ */
/* out[k*size + i] = init[k] * prod_{j < i} r[k*size + j]   (exclusive; inclusive: j <= i)
 * r[j] = num[j] * den[j]^-1, or num[j] when den == NULL;  total[k] = init[k] * prod_{all j} r[j] */
eIcicleError mbls_fr_prefix_product(const mbls_fr_t* num, const mbls_fr_t* den, size_t size, const mbls_fr_t* init,
                                    bool inclusive, const VecOpsConfig* config, mbls_fr_t* output, mbls_fr_t* total);
/* quotient[k*size + i] = sum_{j > i} a[k*size + j] * z[k]^(j-i-1)   (so quotient[size-1] = 0)
 * eval[k] = a[k*size] + z[k] * quotient[k*size] = p_k(z[k]);   p_k = quotient_k * (X - z[k]) + eval[k] */
eIcicleError mbls_fr_poly_divide_linear(const mbls_fr_t* coeffs, size_t size, const mbls_fr_t* z,
                                        const VecOpsConfig* config, mbls_fr_t* quotient, mbls_fr_t* eval);
/* host only, no device work: out[0] = K (elements per thread), out[1] = tile elements,
 * out[2] = workgroups launched per member for `size`, out[3] = elements per workgroup span.
 * size in 1..2^26. */
eIcicleError mbls_fr_scan_geometry(size_t size, int32_t* out);

/* ------------------------------------------------------------------------------------ */
/* Extended-coset transforms: the EvaluationDomain steps of a halo2-style prover, coeff_to_extended
 * (zero-pad a polynomial of n = 2^k coefficients to N = 2^extended_k and evaluate it on the coset
 * g * H_N) and extended_to_coeff (divide by the vanishing polynomial, interpolate, undo the coset,
 * truncate).  The padding, the coset powers, the vanishing division, the N^-1 scaling and the
 * truncation ride in the first and last passes of the transform, and the forward transform skips
 * the butterfly stages whose second input is a padding zero.  The NTT entries above are unchanged.
 * (No reference counterpart: the reference composes these from a coset NTT and CPU passes.)
 *   elements: Montgomery and canonical (< r), in and out, as for the NTT; every output is canonical.
 *   sizes: extended_size a power of two, 1 .. 2^30 and within the initialised domain's order, as
 *     bls12_381_ntt_cuda; size and out_size any value in 1..extended_size, not only powers of two;
 *     period a power of two <= extended_size (halo2's t_evaluations: 2^(extended_k - k) entries).
 *     The forward pruning uses E = log2(extended_size / next_pow2(size)).
 *   coset generator: coset_gen is ONE Montgomery element in HOST memory; NULL or Montgomery one
 *     means no coset, zero mod r gives INVALID_ARGUMENT as in the NTT.  config->coset_gen is not
 *     read.  The same g goes into both calls: the inverse derives g^-1 itself.  The library keeps
 *     the power tables of the last 8 (generator, size, direction) triples with the domain
 *     (bls12_381_ntt_release_domain_cuda frees them); the first call with a new triple builds its
 *     tables and waits for them.
 *   config: stream, batch_size (0 counts as 1; members row-major, `size` / `extended_size` elements
 *     apart on the input side and `extended_size` / `out_size` apart on the output side),
 *     are_inputs_on_device, are_outputs_on_device and is_async as in the NTT.  vanishing_inv is
 *     placed like the input and shared by every member.  columns_batch, or an ordering other than
 *     kNN, gives INVALID_ARGUMENT (mbls_g1_ecntt's convention).
 *   overlap: the output must not overlap the input; undefined.
 *   scratch: the forward call works in its output and takes none; the inverse call of more than
 *     one pass (extended_size > 2^8) works in extended_size * batch elements of the leased scratch
 *     context, which also stages host operands (no allocation per call once it is large enough).
 *   errors, before any device work and before the first HIP call: INVALID_POINTER for a null input,
 *     output or config; INVALID_ARGUMENT for the size rules, the config rules, a zero generator, and
 *     a period that is not a power of two in 1..extended_size with a non-null vanishing_inv.
 *     extended_size past the domain's order gives INVALID_ARGUMENT once the domain is consulted.
 *   timing: no branch and no address depends on a field value.                                   */
/* ------------------------------------------------------------------------------------ */
/* out[k*extended_size + j] = sum_{i < size} coeffs[k*size + i] * (g * W^j)^i,  j < extended_size,
 * W = the NTT's root of extended_size */
eIcicleError mbls_fr_coeff_to_extended(const mbls_fr_t* coeffs, int size, int extended_size,
                                       const mbls_fr_t* coset_gen, const NTTConfig* config, mbls_fr_t* output);
/* e[j] = evals[k*extended_size + j] * vanishing_inv[j mod period]   (vanishing_inv == NULL: e = evals)
 * c[i] = g^-i * N^-1 * sum_j e[j] * W^(-ij);   output[k*out_size + i] = c[i] for i < out_size */
eIcicleError mbls_fr_extended_to_coeff(const mbls_fr_t* evals, int extended_size, int out_size,
                                       const mbls_fr_t* coset_gen, const mbls_fr_t* vanishing_inv, int period,
                                       const NTTConfig* config, mbls_fr_t* output);
/* host only, no device work: what the calls do for (size, extended_size).  `out` holds 18 words:
 * out[0] = passes (0 for extended_size 1), out[1] = E, out[2] = DIT stages the forward call skips as
 * replication = min(E, L of the first pass) (for E beyond it the pruning stops at the first pass: the
 * second runs in full), out[3] = input rows the first pass reads per tile = 2^(L - out[2]) of 2^L,
 * out[4] = scratch elements (32 bytes each) of the forward call per member (0), out[5] = scratch
 * elements of the inverse call per member (staging of host operands not counted; elements, not
 * bytes: 2^30 of them would not fit the word as bytes), out[6 + 3p ..] = (s0, L, logC) of pass p:
 * stages s0+1 .. s0+L on tiles of 2^L rows by 2^logC columns, the NTT's own plan.  Words past the
 * last pass are left alone. */
eIcicleError mbls_fr_domain_plan(int size, int extended_size, int32_t* out);

/* ------------------------------------------------------------------------------------ */
/* Fr column sort, and the lookup argument's permuted pair on top of it (step 2 of a halo2-style
 * lookup_prover: permute_expression_pair, between the theta-compression -- mbls_fr_eval_program --
 * and the commitments and grand product -- the MSM and mbls_fr_prefix_product).  (No reference
 * counterpart: the reference sorts on the CPU and uploads the Permuted columns afterwards.)
 *   elements: 32 bytes, canonical (< r), Montgomery when `montgomery` is set, else standard form.
 *     Outputs are the input elements themselves, moved, byte for byte: nothing is converted.
 *   order: ascending by the element's standard-form integer value -- what Ord gives on the
 *     blst-backed scalar type.  This is this library's definition (the reference tree holds none); a
 *     proof is valid under any total order, the order matters only for reproducing a CPU transcript.
 *     With `montgomery` set the key is still the standard value, from_mont(x), not the stored words.
 *     A non-canonical element has an unspecified position; it never causes an out-of-range access.
 *   batch: config->batch_size members (0 counts as 1), row-major, each of `size` elements, sorted
 *     independently.  columns_batch gives API_NOT_IMPLEMENTED, as the scans do.
 *   placement: config->is_a_on_device input and table (both alike), is_result_on_device the vector
 *     outputs.  Host buffers are staged through the leased scratch context, which also holds every
 *     work array (no allocation per call once it is large enough; mbls_fr_sort_plan reports the
 *     bytes); a host output makes the call synchronous, otherwise it synchronises unless is_async.
 *   errors, before any device work: INVALID_POINTER for a null input, table, config or a missing
 *     required output; INVALID_ARGUMENT for size == 0 or size * batch > 2^26.
 *   overlap: outputs must not overlap inputs; undefined.
 *   timing: NOT constant time.  Digit bins, the skipping of key words that are the same in every
 *     element, and the lookup's binary search depend on the values, as the MSM's bucket sort over
 *     witness scalars does.                                                                      */
/* ------------------------------------------------------------------------------------ */
/* sorted[k*size + i] = the i-th smallest element of member k; perm[k*size + i] = its index within
 * member k.  Equal elements come in ascending original index (the sort is stable).  Either of
 * sorted and perm may be NULL, not both. */
eIcicleError mbls_fr_sort(const mbls_fr_t* input, size_t size, bool montgomery, const VecOpsConfig* config,
                          mbls_fr_t* sorted, uint32_t* perm);
/* Per member, over size = the caller's usable rows (the caller writes the blinding rows after them):
 *   permuted_input = A' = the sorted input; T = the sorted table.
 *   A row of A' is FIRST when it is row 0 or differs from the row above it, else REPEATED.
 *   For every first row with value v: if v occurs in T, the first occurrence of v in T is consumed;
 *   otherwise v is missing.  L = the unconsumed entries of T, ascending; R_0 < .. < R_{m-1} = the
 *   repeated rows.
 *   permuted_table[i] = A'[i] on first rows, permuted_table[R_q] = L[m-1-q] on repeated rows.
 * This is permute_expression_pair exactly: its ordered map is walked in ascending order and the
 * repeated rows are popped from the back.  Both vector outputs are required.
 * n_missing: a HOST pointer to `batch` counts, n_missing[k] = the distinct input values of member k
 * that its table lacks; may be NULL; non-NULL makes the call synchronous.  A member with missing
 * values is data, not an error (SUCCESS): its outputs are still the formulas' (L then has at least m
 * entries), and the caller must treat it as a failed lookup (the CPU's ConstraintSystemFailure). */
eIcicleError mbls_fr_lookup_permute(const mbls_fr_t* input, const mbls_fr_t* table, size_t size, bool montgomery,
                                    const VecOpsConfig* config, mbls_fr_t* permuted_input,
                                    mbls_fr_t* permuted_table, uint64_t* n_missing);
/* host only, no device work.  For size in 1..2^26 and batch >= 1 with size * batch <= 2^26:
 * out[0] = bits per digit, out[1] = digit passes of mbls_fr_sort when no key word is skipped (the
 * key's, plus those over the member number for batch > 1), out[2] = elements per workgroup tile,
 * out[3] = workgroups per pass of mbls_fr_sort (all members together: they ride in one array),
 * out[4] = scratch bytes of mbls_fr_sort, out[5] = scratch bytes of mbls_fr_lookup_permute (staging
 * of host operands not counted).  A workgroup takes a whole number of tiles; the lookup sorts
 * 2 * size * batch elements and scans 2 * size * batch + 1 rank words with the same tile. */
eIcicleError mbls_fr_sort_plan(size_t size, int batch, int64_t* out);

/* ------------------------------------------------------------------------------------ */
/* Log-derivative lookup ("mv-lookup", LogUp) of halo2 forks: the multiplicity column m, an Fr running
 * sum, and the running sum phi of the lookup's terms.  After the theta-compression
 * (mbls_fr_eval_program) a lookup is mbls_fr_lookup_multiplicities then mbls_fr_logup_sum on one
 * stream; the MSMs for m and phi read device memory.  (No reference counterpart: the reference tree
 * uses the classic lookup, on the CPU.  The definitions are this library's own.)
 *   elements: 32 bytes, canonical (< r).  mbls_fr_lookup_multiplicities reads Montgomery elements when
 *     `montgomery` is set, else standard form, and writes m in the same form; the two sums read and
 *     write Montgomery elements.  Every output element is canonical.
 *   equality (the join): of the canonical 32-byte elements.  A non-canonical element gets an
 *     unspecified count; it never causes an out-of-range access.
 *   pointer table: `inputs` is HOST memory, always: n_inputs column pointers, as `columns` is for
 *     mbls_fr_eval_program; n_inputs in 1..64.
 *   batch: config->batch_size members (0 counts as 1), row-major, each of `size` elements, in the
 *     table, the multiplicities, the output and every input column alike; a member's cells are
 *     matched against that member's table only.  beta, init, total and n_missing hold one entry per
 *     member.  columns_batch gives API_NOT_IMPLEMENTED, as the scans do.
 *   placement: config->is_a_on_device every input column, table and multiplicities-as-input (all
 *     alike; mbls_fr_prefix_sum: input), is_b_on_device beta and init, is_result_on_device the vector
 *     output and total.  Host operands are staged through the leased scratch context, which also
 *     holds every work array (no allocation per call once it is large enough); a host output makes
 *     the call synchronous, otherwise it synchronises unless is_async.
 *   scratch bytes, n = size * batch, staging of host operands not counted (each staged column is
 *     32 n): mbls_fr_lookup_multiplicities out[4] of mbls_fr_sort_plan(size, batch) + 8 (n + batch),
 *     about 56 n; mbls_fr_prefix_sum 64 * batch * G for G = out[2] of mbls_fr_scan_geometry(size);
 *     mbls_fr_logup_sum 64 n + 64 * batch * G.  Every block is rounded up to 256 bytes.
 *   errors, all before any device work: INVALID_POINTER for a null inputs, table, multiplicities,
 *     beta, input, output or config, or a null entry of inputs; INVALID_ARGUMENT for size == 0,
 *     size * batch > 2^26, or n_inputs outside 1..64.
 *   in place and overlap: mbls_fr_prefix_sum's output may equal its input, mbls_fr_logup_sum's output
 *     may equal multiplicities (the same pointer); any other overlap is undefined.
 *   timing: mbls_fr_lookup_multiplicities is NOT constant time: the sort's digit bins and skipped
 *     key words, the search path and the merging of equal rows depend on the values, as in
 *     mbls_fr_sort.  mbls_fr_prefix_sum and mbls_fr_logup_sum have no branch and no address that
 *     depends on a field value; zero denominators go through mask selects and the fixed Fermat chain,
 *     as in bls12_381_batch_inv_cuda.                                                            */
/* ------------------------------------------------------------------------------------ */
/* m[k*size + j] = #{ (c, i) : c < n_inputs, i < size, inputs[c][k*size + i] == table[k*size + j] }
 *                 if j is the CREDITED row of its value in member k's table, else 0.
 * The credited row of a value is the lowest row of the member's table that holds it
 * (credit_last: the highest).  m is written as an Fr element: the count, Montgomery when
 * `montgomery` is set, else standard form; always canonical.
 * n_missing: HOST pointer to `batch` counts, n_missing[k] = the cells (c, i) of member k whose
 * value its table lacks; may be NULL; non-NULL makes the call synchronous.  Missing cells are
 * data, not an error (SUCCESS), as in mbls_fr_lookup_permute: sum_j m[j] + n_missing[k] =
 * n_inputs * size for every member. */
eIcicleError mbls_fr_lookup_multiplicities(const mbls_fr_t* const* inputs, int n_inputs, const mbls_fr_t* table,
                                           size_t size, bool montgomery, bool credit_last,
                                           const VecOpsConfig* config, mbls_fr_t* multiplicities,
                                           uint64_t* n_missing);
/* out[k*size + i] = init[k] + sum_{j < i} in[k*size + j]   (inclusive: j <= i);
 * total[k] = init[k] + sum over all j.  init == NULL means zero.  total may be NULL.  The geometry is
 * mbls_fr_scan_geometry's; a step is one modular addition. */
eIcicleError mbls_fr_prefix_sum(const mbls_fr_t* input, size_t size, const mbls_fr_t* init, bool inclusive,
                                const VecOpsConfig* config, mbls_fr_t* output, mbls_fr_t* total);
/* term[i] = sum_{c < n_inputs} (inputs[c][i] + beta[k])^-1  -  m[i] * (table[i] + beta[k])^-1
 * output = the EXCLUSIVE prefix sum of term from init[k] (phi[0] = init, phi[i+1] = phi[i] + term[i]);
 * total[k] = phi[size].  Montgomery elements throughout.  0^-1 = 0, as bls12_381_batch_inv_cuda.
 * init == NULL means zero, total may be NULL.  With phi[0] = 0 a satisfied lookup has total == 0. */
eIcicleError mbls_fr_logup_sum(const mbls_fr_t* const* inputs, int n_inputs, const mbls_fr_t* table,
                               const mbls_fr_t* multiplicities, size_t size, const mbls_fr_t* beta,
                               const mbls_fr_t* init, const VecOpsConfig* config, mbls_fr_t* output,
                               mbls_fr_t* total);

/* ------------------------------------------------------------------------------------ */
/* Fr expression evaluator: one caller-supplied straight-line stack program run once per row over
 * a set of columns read at rotated rows -- the permutation numerators and denominators that feed
 * mbls_fr_prefix_product, the theta-compression of lookup columns, the gate / permutation / lookup
 * folds of the quotient on the extended coset, linear combinations of polynomials.  One launch,
 * one read of every column an op names, one write per output; the intermediates stay on chip.  (No
 * reference counterpart: the reference composes these on the CPU.)
 *   elements: Montgomery and canonical (< r), in and out; every output element is canonical.
 *   rows: size in 1..2^26, any value, not only a power of two.  COLUMN reads row
 *     (i + b * rot_stride) mod size: rot_stride is 1 on the base domain and 2^(extended_k - k) on
 *     the extended one.  Any b and any rot_stride in 1..2^26 are legal: the host reduces
 *     b * rot_stride modulo size (in 64-bit arithmetic, which holds every such product) and the
 *     kernel only sees an offset in [0, size).
 *   program: `program`, the `columns` pointer table and the counts are host memory, always.  The
 *     columns themselves are placed by config->is_a_on_device (all alike), `constants` by
 *     is_b_on_device, `output` (n_outputs * size elements, member-major: output k at k * size) by
 *     is_result_on_device.  Host buffers are staged through the leased scratch context, which also
 *     holds the resolved program (no allocation per call once it is large enough); a host output
 *     makes the call synchronous, otherwise it synchronises unless is_async.  batch_size and
 *     columns_batch are not read.
 *   limits: n_ops in 1..4096, n_columns in 1..1024, n_constants in 0..1024, n_outputs in 1..8,
 *     stack depth at most 8.
 *   errors, all before any device work (the host simulates the stack): INVALID_POINTER for a null
 *     columns, program, config or output, a null entry of columns, or a null constants with
 *     n_constants > 0; INVALID_ARGUMENT for a size or count outside its limit, an unknown opcode, a
 *     column, constant or output index out of range, a pop from an empty stack, a depth above 8, an
 *     output emitted twice or never, a stack that is not empty after the last op.
 *     mbls_fr_expr_check applies exactly the program rules: it is the same function.
 *   overlap: output must not overlap any column (a rotated read of a row another lane has already
 *     written); undefined.
 *   timing: no branch and no address depends on a field value; the program and the rotations are
 *     public.                                                                                    */
/* ------------------------------------------------------------------------------------ */
typedef enum {
    MBLS_EXPR_COLUMN = 0, /* push columns[a][(i + b * rot_stride) mod size]   (b signed)  */
    MBLS_EXPR_CONST  = 1, /* push constants[a]                                            */
    MBLS_EXPR_ADD    = 2, /* pop y, pop x, push x + y                                     */
    MBLS_EXPR_SUB    = 3, /* pop y, pop x, push x - y                                     */
    MBLS_EXPR_MUL    = 4, /* pop y, pop x, push x * y                                     */
    MBLS_EXPR_NEG    = 5, /* top = -top                                                   */
    MBLS_EXPR_DOUBLE = 6, /* top = 2 top                                                  */
    MBLS_EXPR_SQUARE = 7, /* top = top^2                                                  */
    MBLS_EXPR_SCALE  = 8, /* top = top * constants[a]                                     */
    MBLS_EXPR_HORNER = 9, /* pop t, pop acc, push acc * constants[a] + t                  */
    MBLS_EXPR_EMIT   = 10 /* pop v, output[a * size + i] = v                              */
} mbls_fr_expr_opcode;
typedef struct { int32_t op, a, b; } mbls_fr_expr_op;   /* b is read by COLUMN only */

eIcicleError mbls_fr_eval_program(const mbls_fr_t* const* columns, int n_columns, size_t size, size_t rot_stride,
                                  const mbls_fr_t* constants, int n_constants,
                                  const mbls_fr_expr_op* program, int n_ops, int n_outputs,
                                  const VecOpsConfig* config, mbls_fr_t* output);
/* host only, no device work: validates and describes a program.
 * out[0] = maximum stack depth, out[1] = COLUMN loads per row, out[2] = field multiplications per row
 * (MUL, SQUARE, SCALE, HORNER), out[3] = distinct (column, rotation) pairs. */
eIcicleError mbls_fr_expr_check(const mbls_fr_expr_op* program, int n_ops, int n_columns, int n_constants,
                                int n_outputs, int32_t* out);

/* ------------------------------------------------------------------------------------ */
/* Fr graph evaluator: the same work as mbls_fr_eval_program for a program in three-address form
 * over named values -- the form of halo2's GraphEvaluator, whose calculations each write one
 * intermediate that any later calculation may read.  Op k defines value k (single assignment), so a
 * subexpression shared by several constraints is computed once.  One launch.  (No reference
 * counterpart.)
 *   as mbls_fr_eval_program: the element form (Montgomery, canonical, in and out), the rotation
 *     arithmetic (a COLUMN source reads row (i + rot * rot_stride) mod size, any rot, rot_stride in
 *     1..2^26), size in 1..2^26, the placement flags (columns by is_a_on_device, constants by
 *     is_b_on_device, output by is_result_on_device), the staging of host buffers, is_async, the
 *     output layout (n_outputs members of size elements), and that output may overlap no column
 *     (nor the constants, which the kernel reads through the scalar cache).
 *   sources: `a` is read by every op, `b` by ADD, SUB, MUL and HORNER only and must be NONE on the
 *     others.  idx of a NONE source, rot of a source that is no COLUMN, and c of an op that is
 *     neither HORNER nor EMIT are not read.
 *   limits: n_ops in 1..16384, n_columns in 1..1024, n_constants in 0..1024, n_outputs in 1..8,
 *     at most 32 values resident at once (below).
 *   residency: let last(j) be the largest op index that reads value j.  A read of value j by op
 *     j + 1 is forwarded from the register that still holds it.  Value j is resident iff
 *     last(j) > j + 1, and then occupies one slot of on-chip memory while ops j + 1 .. last(j) run.
 *     The peak is the largest number of values resident during any one op; the budget is 32.  A
 *     value nobody reads is allowed and costs nothing.  There is no spilling: a caller whose peak
 *     is too high cuts the program at the op mbls_fr_graph_check names, emits the live values as
 *     outputs and reads them back as columns in a second call.
 *   errors, all before any device work: INVALID_POINTER as mbls_fr_eval_program; INVALID_ARGUMENT
 *     for a size or count outside its limit, an unknown opcode or source kind, a b other than NONE
 *     on SQUARE, DOUBLE, NEG, STORE or EMIT, NONE where an operand is needed, a VALUE index that is
 *     negative, not smaller than the op's own, or names an EMIT, a column, constant or output index
 *     out of range, an output emitted twice or never, a peak above the budget.
 *   timing: no branch and no address depends on a field value.                                   */
/* ------------------------------------------------------------------------------------ */
typedef enum { MBLS_GRAPH_ADD = 0, MBLS_GRAPH_SUB, MBLS_GRAPH_MUL, MBLS_GRAPH_SQUARE, MBLS_GRAPH_DOUBLE,
               MBLS_GRAPH_NEG, MBLS_GRAPH_HORNER /* a * constants[c] + b */, MBLS_GRAPH_STORE /* a */,
               MBLS_GRAPH_EMIT /* output[c * size + i] = a, defines no value */ } mbls_fr_graph_opcode;
typedef enum { MBLS_GRAPH_NONE = 0, MBLS_GRAPH_VALUE /* result of op idx, idx < this op */,
               MBLS_GRAPH_COLUMN /* columns[idx][(i + rot * rot_stride) mod size] */,
               MBLS_GRAPH_CONST  /* constants[idx] */ } mbls_fr_graph_source;
typedef struct { int32_t kind, idx, rot; } mbls_fr_graph_src;
typedef struct { int32_t op; mbls_fr_graph_src a, b; int32_t c; } mbls_fr_graph_op;   /* 32 bytes */

eIcicleError mbls_fr_eval_graph(const mbls_fr_t* const* columns, int n_columns, size_t size, size_t rot_stride,
                                const mbls_fr_t* constants, int n_constants, const mbls_fr_graph_op* program,
                                int n_ops, int n_outputs, const VecOpsConfig* config, mbls_fr_t* output);
/* host only, no device work: the same validation, and a description of the program.
 * out[0] = peak, out[1] = the first op index at which the peak is reached, out[2] = resident values,
 * out[3] = forwarded operands, out[4] = column loads per row, out[5] = distinct (column, rot) pairs,
 * out[6] = products per row (MUL, SQUARE, HORNER), out[7] = the budget.  A program refused only for
 * its peak still gets all eight written, so that the caller knows where to cut. */
eIcicleError mbls_fr_graph_check(const mbls_fr_graph_op* program, int n_ops, int n_columns, int n_constants,
                                 int n_outputs, int32_t* out);

/* ------------------------------------------------------------------------------------ */
/* Fr inner products and multi-point polynomial evaluation: the phase between the quotient and the
 * multi-open of a halo2-style prover, where every committed polynomial is evaluated at the challenge
 * x and its rotations omega^r x.  p(z) = sum_i a_i z^i is an inner product with the powers of z, and
 * the powers are shared by every polynomial opened at z.  (No reference counterpart: the reference
 * evaluates on the CPU, eval_polynomial, one Horner pass per polynomial and point.)
 *   elements: Montgomery and canonical (< r), in and out; points, base and init likewise.  Every
 *     output is canonical; a field sum is unique, so the result does not depend on the order of
 *     summation.  init == NULL means Montgomery one.  z^0 = 1 for every z, 0 included.
 *   pointer tables: `columns` and `vectors` are host arrays of pointers, always, as `columns` is for
 *     mbls_fr_eval_program; what they point to is placed by the config.
 *   placement: config->is_a_on_device the columns (all alike), is_b_on_device the vectors (all
 *     alike), points, base and init, is_result_on_device the output.  Host operands are staged
 *     through the leased scratch context, which also holds every work array (no allocation per call
 *     once it is large enough; mbls_fr_inner_plan reports the bytes); a host output makes the call
 *     synchronous, otherwise it synchronises unless is_async.
 *   batch: mbls_fr_inner_products and mbls_fr_multi_eval do not read batch_size or columns_batch.
 *     mbls_fr_powers reads batch_size (0 counts as 1): member k fills rows k * size .. (k + 1) * size
 *     from base[k] and init[k]; columns_batch gives API_NOT_IMPLEMENTED, as the scans do.
 *   limits: size in 1..2^26 (mbls_fr_powers: size * batch <= 2^26), n_columns in 1..1024,
 *     n_vectors and n_points in 1..16.
 *   errors, all before any device work: INVALID_POINTER for a null table, points, base, config or
 *     output and for a null table entry; INVALID_ARGUMENT for a size or count outside its limit.
 *   overlap: the output must not overlap any input; otherwise the result is undefined.
 *   timing: the columns are witness polynomials: no branch and no address depends on a field value.
 *     The conditions are on thread, block and row indices and on the counts; the power tables are
 *     built by square-and-multiply over the bits of a row index, never of a base.
 *   work: a workgroup takes CB columns x VB vectors and loads each element of a row once for the
 *     CB * VB products; the products are radix 2^29 and a thread adds the unreduced columns of 7 of
 *     them into 64-bit accumulators before one Montgomery reduction (7 * 9 * 2^58 < 2^64).  Each
 *     workgroup writes one partial sum per output of its block and a second launch folds them;
 *     their number is bounded by the plan, not by `size`.  mbls_fr_multi_eval writes the powers of
 *     each point to scratch (mbls_fr_powers' kernels, 32 * size * n_points bytes) and runs the same
 *     inner products over them, so it equals mbls_fr_powers followed by mbls_fr_inner_products.
 *     mbls_fr_powers costs one product per element: base^i = hi[i >> s] * lo[i & (2^s - 1)] with two
 *     tables of about sqrt(size) entries per member, hi carrying init.
 *   which call: for ONE polynomial at ONE point mbls_fr_poly_divide_linear with quotient == NULL
 *     does not write the powers and may be as fast; mbls_fr_multi_eval is for several polynomials
 *     sharing their points.                                                       */
/* ------------------------------------------------------------------------------------ */
/* output[p * n_vectors + k] = sum_{i < size} columns[p][i] * vectors[k][i] */
eIcicleError mbls_fr_inner_products(const mbls_fr_t* const* columns, int n_columns,
                                    const mbls_fr_t* const* vectors, int n_vectors, size_t size,
                                    const VecOpsConfig* config, mbls_fr_t* output);
/* output[p * n_points + k] = sum_{i < size} columns[p][i] * points[k]^i   (z^0 = 1, also for z = 0) */
eIcicleError mbls_fr_multi_eval(const mbls_fr_t* const* columns, int n_columns, size_t size,
                                const mbls_fr_t* points, int n_points,
                                const VecOpsConfig* config, mbls_fr_t* output);
/* output[k * size + i] = init[k] * base[k]^i, k < batch;  init == NULL means Montgomery one */
eIcicleError mbls_fr_powers(const mbls_fr_t* base, const mbls_fr_t* init, size_t size,
                            const VecOpsConfig* config, mbls_fr_t* output);
/* host only, no device work: the geometry the three calls use for `size` rows, n_columns columns and
 * n_vectors vectors (or points).  Twelve words:
 *   out[0] = T, rows per tile (threads * out[1]),
 *   out[1] = products a thread defers before one reduction = rows it takes from a tile,
 *   out[2] = CB, columns per block,  out[3] = VB, vectors per block,
 *   out[4] = the maximum number of workgroups of the product launch, whatever the size,
 *   out[5] = the most row groups these counts may take; a workgroup takes more than one tile only
 *            for size > out[5] * T,
 *   out[6] = consecutive tiles per workgroup,  out[7] = G, row groups = partial sums per output,
 *   out[8] = workgroups launched = G * ceil(n_columns / CB) * ceil(n_vectors / VB),
 *   out[9] = scratch bytes of mbls_fr_inner_products (staging not counted):
 *            up256(32 * G * n_columns * n_vectors) + up256(8 * (n_columns + n_vectors)),
 *   out[10] = scratch bytes of mbls_fr_multi_eval with n_points = n_vectors (staging not counted):
 *            out[9] + up256(32 * n_vectors * (2^s + ceil(size / 2^s))) + up256(32 * size * n_vectors),
 *   out[11] = s of the power tables;  up256 rounds up to a multiple of 256. */
eIcicleError mbls_fr_inner_plan(size_t size, int n_columns, int n_vectors, int64_t* out);

/* ------------------------------------------------------------------------------------ */
/* batch point-form conversions, reference point_ops.cu:759 / :844 / :924 (exported there as
 * extern "C").  Montgomery in, Montgomery out; Jacobian projective (x = X/Z^2, y = Y/Z^3).
 * affine_to_projective: (x, y) -> (x, y, 1), identity (0, 0) -> (0, 1, 0).
 * projective_to_affine: Z = 0 -> (0, 0).  Input placement config->is_a_on_device, output
 * config->is_result_on_device; a host output is synchronous.  size in 1..2^26, null pointers
 * or other sizes give INVALID_ARGUMENT (as the reference).  Input and output must not overlap. */
/* ------------------------------------------------------------------------------------ */
eIcicleError bls12_381_g1_affine_to_projective(const mbls_g1_affine_t* input, int size, const VecOpsConfig* config,
                                               mbls_g1_projective_t* output);
eIcicleError bls12_381_g1_projective_to_affine(const mbls_g1_projective_t* input, int size, const VecOpsConfig* config,
                                               mbls_g1_affine_t* output);
eIcicleError bls12_381_g2_projective_to_affine(const mbls_g2_projective_t* input, int size, const VecOpsConfig* config,
                                               mbls_g2_affine_t* output);

/* ------------------------------------------------------------------------------------ */
/* batch scalar multiplication: output[i] = scalars[i] * bases[i], independent variable-base
 * multiplications.  The reference declares bls12_381_g1_scalar_mul (point_ops.cu:1149) and
 * bls12_381_g1_scalar_mul_glv (:1019) behind GLV_ENABLED, which its build leaves off; here both
 * names run one implementation (always the GLV split).  The G2 entry has no reference counterpart.
 *   scalars: 32 bytes, STANDARD form; any 256-bit value k is accepted and the result is k * P
 *     for the integer k, which on the order-r subgroup is (k mod r) * P (the reduction the raw MSM
 *     entry applies).  The mbls_* forms read Montgomery scalars when scalars_montgomery is set.
 *   bases: Montgomery affine; the identity is the all-zero point and gives the identity for every
 *     scalar.  Bases are ASSUMED to lie in the order-r subgroup, as for the MSM: the GLV / psi
 *     splits rely on phi = [lambda] and psi = [z], which hold only there (not checked here; see
 *     mbls_g*_check_points).
 *   output: Jacobian Montgomery (X, Y, Z), x = X/Z^2, y = Y/Z^3, identity Z = 0 -- the form
 *     bls12_381_g*_projective_to_affine takes.  Input and output must not overlap.
 *   placement: config->is_a_on_device the bases, is_b_on_device the scalars, is_result_on_device
 *     the output (point_ops.cu:1044-1046).  Host buffers are staged through the leased scratch
 *     context; a host output is synchronous, a device output synchronises unless is_async.
 *     batch_size and columns_batch are not read.
 *   errors: a null pointer, a null config, size <= 0 or size > 2^26 give INVALID_ARGUMENT before
 *     any device work (point_ops.cu:1027-1035).
 *   timing: NOT constant time -- table lookups and branches depend on the scalar's digits, like
 *     the MSM's bucket sort.  Do not use with secret scalars where timing is observable.       */
/* ------------------------------------------------------------------------------------ */
eIcicleError bls12_381_g1_scalar_mul(const mbls_g1_affine_t* bases, const mbls_fr_t* scalars, int size,
                                     const VecOpsConfig* config, mbls_g1_projective_t* output);
eIcicleError bls12_381_g1_scalar_mul_glv(const mbls_g1_affine_t* bases, const mbls_fr_t* scalars, int size,
                                         const VecOpsConfig* config, mbls_g1_projective_t* output);
eIcicleError bls12_381_g2_scalar_mul(const mbls_g2_affine_t* bases, const mbls_fr_t* scalars, int size,
                                     const VecOpsConfig* config, mbls_g2_projective_t* output);
eIcicleError mbls_g1_scalar_mul(const mbls_g1_affine_t* bases, const mbls_fr_t* scalars, int size,
                                bool scalars_montgomery, const VecOpsConfig* config, mbls_g1_projective_t* output);
eIcicleError mbls_g2_scalar_mul(const mbls_g2_affine_t* bases, const mbls_fr_t* scalars, int size,
                                bool scalars_montgomery, const VecOpsConfig* config, mbls_g2_projective_t* output);

/* ------------------------------------------------------------------------------------ */
/* G1 EC-NTT: the NTT over G1 points (no reference counterpart: the reference derives the Lagrange
 * SRS on the CPU, g_to_lagrange).  For size = 2^k and w = ROOT_OF_UNITY^(2^(32-k)), the root of the
 * Fr NTT of that size (bls12_381_ntt_get_rou_from_domain(k)):
 *   forward  out_j = sum_i [w^(ij)] P_i
 *   inverse  out_i = [n^-1] sum_j [w^(-ij)] P_j
 * natural order in and out.  The inverse of a monomial SRS P_j = [s^j] G is the Lagrange SRS
 * [L_i(s)] G.
 *   points: Montgomery affine, 96 bytes, identity = all zero, in and out.  The output is canonical
 *     affine: a result has exactly one byte representation.  Inputs are ASSUMED to lie in the
 *     order-r subgroup, as for scalar_mul and the MSM: the GLV split relies on phi = [lambda],
 *     which holds only there (not checked here; see mbls_g*_check_points).
 *   config: stream, are_inputs_on_device, are_outputs_on_device and is_async are honoured.  Host
 *     buffers are staged through the leased scratch context, which also holds the work arrays; a
 *     host output is synchronous, a device output synchronises unless is_async.  input == output
 *     (the same device pointer) is allowed; a partial overlap is undefined.
 *   errors, before any device work: a null input, output or config gives INVALID_POINTER (the
 *     NTT's convention); INVALID_ARGUMENT for size < 1, not a power of two or > 2^26, for log2 size
 *     above the order of the initialised NTT domain (32 with none initialised), for batch_size
 *     other than 0 or 1, for columns_batch, for an ordering other than NN and for a coset_gen other
 *     than Montgomery one (a zero-initialised config included, as for the NTT).  The call reads the
 *     domain's order only: it neither needs nor builds the Fr twiddle tables.
 *   timing: NOT constant time -- table lookups and branches depend on the scalars' digits.  Here
 *     the scalars are public roots of unity, so nothing secret is exposed.                     */
/* ------------------------------------------------------------------------------------ */
eIcicleError mbls_g1_ecntt(const mbls_g1_affine_t* input, int size, NTTDir dir, const NTTConfig* config,
                           mbls_g1_affine_t* output);

/* ------------------------------------------------------------------------------------ */
/* fixed-base batch multiplication: output[i] = [scalars[i] mod r] base for ONE base, and a KZG SRS
 * from a secret (no reference counterpart; halo2's ParamsKZG::unsafe_setup computes g[i] =
 * [s^i] G, g_lagrange[i] = [L_i(s)] G and s_g2 = [s] G2 this way).  The doublings are paid once, in
 * a table of the base; a scalar then costs at most W mixed additions.
 *   plan: mbls_fixed_base_plan(group, out) is host only; group 1 = G1, 2 = G2.  out[0] = c (digit
 *     width), out[1] = windows W = ceil(255 / c), out[2] = entries per window = 2^(c-1), out[3] =
 *     table entries = W * 2^(c-1), out[4] = bytes per entry (96 / 192), out[5] = lanes per
 *     workgroup, out[6] = most lanes per launch (a larger batch runs as several launches over one
 *     work array; 0 would mean no chunking), out[7] = scratch bytes per output point of a launch.
 *   table: table[w * 2^(c-1) + (d-1)] = [d * 2^(c w)] base for d = 1..2^(c-1), canonical
 *     Montgomery affine.  It is a caller-owned DEVICE buffer of out[3] entries; nothing is cached in
 *     the library.  `base` is placed by is_a_on_device.  A base equal to the identity (all zero)
 *     gives an all-zero table, and every product of it is the identity.  The base is ASSUMED to lie
 *     in the order-r subgroup: the table build runs mbls_g*_scalar_mul (GLV / psi), and the
 *     multiplication reduces k mod r.  The multiplication itself uses no endomorphism.
 *   scalars: 32 bytes, any 256-bit value; reduced mod r first (Montgomery scalars, when
 *     scalars_montgomery is set, go through from_mont first).  Placed by is_b_on_device.
 *   output: canonical Montgomery AFFINE, identity = all zero, placed by is_result_on_device: a
 *     result has exactly one byte representation.  Host operands are staged through the leased
 *     scratch context, which also holds the Jacobian work array: no allocation per call once it is
 *     large enough.  A host output is synchronous, a device output synchronises unless is_async
 *     (as scalar_mul).  batch_size and columns_batch are not read.
 *   mbls_fixed_base_recode (host only): the W signed digits of scalar mod r (standard form), lowest
 *     window first, by the function the kernels run: digits in [-2^(c-1), 2^(c-1) - 1], the top
 *     one in [0, 2^(c-1)], sum digits[w] 2^(c w) = scalar mod r.
 *   mbls_g1_srs_from_secret: `tau` is ONE Montgomery element in HOST memory (as coset_gen is).
 *     basis 0: output[i] = [tau^i] base, size in 1..2^26, 0^0 = 1.
 *     basis 1: output[i] = [L_i(tau)] base, L_i(tau) = (tau^n - 1)/n * w^i / (tau - w^i), n = size =
 *       2^k within the order of the initialised NTT domain (mbls_g1_ecntt's rule; 32 with none
 *       initialised: no domain is needed), w the Fr NTT's root of that size.  The formula has a
 *       pole where tau^n = 1 (halo2 panics): INVALID_ARGUMENT, decided on the host by k squarings.
 *       It equals mbls_g1_ecntt(inverse) of basis 0, byte for byte, without an EC-NTT.
 *     The scalars are made on the device (mbls_fr_powers, bls12_381_batch_inv_cuda, the vecops),
 *     then one multiplication runs over them; `table` is that of the base.
 *   The table build, the G2 normalisation and the SRS call run other entries of this library,
 *   which lease a scratch context of their own while the call holds one.  A thread that already
 *   holds a context never waits for a second: when none is free it gets one past
 *   MBLS_SCRATCH_CONTEXTS, so these calls are safe from any number of threads and with any limit
 *   (the pool then holds up to one context more per thread that is inside them at once).
 *   errors, before any device work: INVALID_POINTER for a null table, base, scalars, tau, config,
 *     output or plan / digit array; INVALID_ARGUMENT for size <= 0 or size > 2^26, a group other
 *     than 1 or 2, a basis other than 0 or 1, and for basis 1 a size that is no power of two or
 *     past the domain's order, and tau^size = 1.
 *   timing: NOT constant time -- table addresses depend on the scalar's digits, and zero digits are
 *     skipped.  Do not multiply a secret key, or the secret of a real ceremony, with these calls
 *     where timing or cache behaviour is observable; they serve unsafe_setup, public scalars and
 *     tests.  A ceremony SRS is read, decompressed and checked instead (mbls_g*_decompress,
 *     mbls_g*_check_points).                                                                    */
/* ------------------------------------------------------------------------------------ */
eIcicleError mbls_fixed_base_plan(int group, int64_t* out);
eIcicleError mbls_fixed_base_recode(const mbls_fr_t* scalar, int32_t* digits);
eIcicleError mbls_g1_fixed_base_table(const mbls_g1_affine_t* base, const VecOpsConfig* config, mbls_g1_affine_t* table);
eIcicleError mbls_g2_fixed_base_table(const mbls_g2_affine_t* base, const VecOpsConfig* config, mbls_g2_affine_t* table);
eIcicleError mbls_g1_fixed_base_mul(const mbls_g1_affine_t* table, const mbls_fr_t* scalars, int size,
                                    bool scalars_montgomery, const VecOpsConfig* config, mbls_g1_affine_t* output);
eIcicleError mbls_g2_fixed_base_mul(const mbls_g2_affine_t* table, const mbls_fr_t* scalars, int size,
                                    bool scalars_montgomery, const VecOpsConfig* config, mbls_g2_affine_t* output);
eIcicleError mbls_g1_srs_from_secret(const mbls_g1_affine_t* table, const mbls_fr_t* tau, int size, int basis,
                                     const VecOpsConfig* config, mbls_g1_affine_t* output);

/* ------------------------------------------------------------------------------------ */
/* batch point validation: is every point canonical, on the curve and in the order-r subgroup?
 * (No reference counterpart: the reference has g1_is_on_curve, point.cuh:339, as a device helper
 * only and no subgroup test.)  The MSM, scalar_mul and EC-NTT entries assume subgroup members
 * because their GLV / psi splits are wrong elsewhere; this is the call that establishes it, once,
 * when an SRS is uploaded.  status[i] is the FIRST failing test of point i in the order of the
 * enum; 0 and 1 are valid, >= 2 invalid.
 *   membership: the endomorphism criteria of M. Scott, "A note on group membership tests for G1,
 *     G2 and GT on BLS pairing-friendly curves" -- G1: [z^2] P - P == phi(P), a 128-bit chain;
 *     G2: psi(P) == [z] P, a 64-bit chain -- exact on curve points for the library's beta / psi.
 *   points: affine, Montgomery when points_montgomery, else standard form (as the MSM's
 *     are_points_montgomery_form = false).  The canonical test reads the raw words either way, the
 *     conversion follows it.  The identity is only the all-zero encoding: (0, p) is NONCANONICAL.
 *   outputs: status, `size` bytes, placed by config->is_result_on_device; n_invalid, a HOST
 *     pointer, receives the number of points with status >= 2.  Either may be NULL, not both.
 *   placement: config->is_a_on_device the points.  Host buffers are staged through the leased
 *     scratch context; a host output (a host status, or a non-NULL n_invalid) makes the call
 *     synchronous, otherwise it synchronises unless is_async.  batch_size and columns_batch are
 *     not read.
 *   errors: a null points or config, both outputs null, size <= 0 or size > 2^26 give
 *     INVALID_ARGUMENT before any device work (scalar_mul's convention).  Invalid points are data,
 *     not an error: the call returns SUCCESS.
 *   timing: NOT constant time -- a lane leaves at its first failing test.  Points to validate are
 *     public, so nothing secret is involved.                                                   */
/* ------------------------------------------------------------------------------------ */
typedef enum {
    MBLS_POINT_OK = 0,            /* canonical, on the curve, in the order-r subgroup          */
    MBLS_POINT_IDENTITY = 1,      /* the all-zero identity encoding: a member, reported apart  */
    MBLS_POINT_NONCANONICAL = 2,  /* some coordinate (G2: some component) is >= p             */
    MBLS_POINT_OFF_CURVE = 3,     /* canonical, but y^2 != x^3 + b                             */
    MBLS_POINT_OFF_SUBGROUP = 4   /* on the curve, but [r]P != O                               */
} mbls_point_status;

eIcicleError mbls_g1_check_points(const mbls_g1_affine_t* points, int size, bool points_montgomery,
                                  const VecOpsConfig* config, uint8_t* status, uint64_t* n_invalid);
eIcicleError mbls_g2_check_points(const mbls_g2_affine_t* points, int size, bool points_montgomery,
                                  const VecOpsConfig* config, uint8_t* status, uint64_t* n_invalid);

/* ------------------------------------------------------------------------------------ */
/* batch point compression and decompression, in the ZCash encoding that ceremony transcripts, SRS
 * files and the blst-backed crates' to_compressed / from_compressed use.  (No reference
 * counterpart: the reference has no serialization and no square root.)
 *   format: a G1 record is 48 bytes, x as a big-endian integer; a G2 record is 96 bytes, x.c1 in
 *     bytes 0..47 then x.c0 in bytes 48..95.  The top three bits of byte 0 are flags: C (bit 7),
 *     the compressed form, always 1; I (bit 6), infinity, with every other bit of the record zero
 *     (c0 00 .. 00); S (bit 5), y is the larger of {y, p - y} as standard-form integers,
 *     y > (p - 1) / 2 -- for G2 comparing y.c1 first and y.c0 only when y.c1 == 0.
 *   decompress: status[i] is the FIRST failing test of record i in the order BAD_FLAGS, IDENTITY,
 *     NONCANONICAL, NO_POINT; 0 and 1 are valid, >= 2 invalid, and 0..3 line up with
 *     mbls_point_status, so the maximum of this status and a later check_points status is
 *     meaningful.  Status 0 writes the canonical (x, y) with the root chosen by S, Montgomery when
 *     points_montgomery, else standard form; every other status writes the all-zero point, so the
 *     output is deterministic and the status tells a rejected record from a real identity.
 *     y = sqrt(x^3 + b) by one fixed exponent chain (p == 3 mod 4), in G2 through the norm; a point
 *     that is written satisfies the curve equation by construction.  NO SUBGROUP TEST is made:
 *     for untrusted input mbls_g*_check_points on the output is the next step.
 *   compress: the inverse.  Inputs are assumed to be canonical curve points or the all-zero
 *     identity, which gives the infinity encoding; NOTHING IS VALIDATED (a point off the curve or
 *     a non-canonical coordinate gives a record that does not decode to it).
 *   outputs of decompress: points, `size` affine points; status, `size` bytes; both placed by
 *     config->is_result_on_device; n_invalid, a HOST pointer, receives the number of records with
 *     status >= 2.  status and n_invalid may each be NULL, also both.
 *   placement: config->is_a_on_device the input (bytes for decompress, points for compress),
 *     config->is_result_on_device the output.  Host buffers are staged through the leased scratch
 *     context; a host output (or a non-NULL n_invalid) makes the call synchronous, otherwise it
 *     synchronises unless is_async.  batch_size and columns_batch are not read.
 *   errors: INVALID_ARGUMENT before any device work (scalar_mul's convention) for a null bytes,
 *     points or config, for size <= 0 or size > 2^26, and for a DEVICE byte or point buffer that is
 *     not 16-byte aligned (records move as 16-byte vectors; host buffers are staged and have no
 *     alignment rule).  Malformed records are data, not an error: the call returns SUCCESS.
 *   timing: NOT constant time -- a lane leaves at its first failing test.  Encoded points are
 *     public, so nothing secret is involved.                                                   */
/* ------------------------------------------------------------------------------------ */
typedef enum {
    MBLS_DECODE_OK = 0,           /* a curve point was written                                   */
    MBLS_DECODE_IDENTITY = 1,     /* the infinity encoding: the all-zero point was written       */
    MBLS_DECODE_NONCANONICAL = 2, /* x (G2: a component of x) >= p                               */
    MBLS_DECODE_NO_POINT = 3,     /* x^3 + b is not a square: no curve point has this x          */
    /* 4 is left unused: it is MBLS_POINT_OFF_SUBGROUP, which decoding does not test            */
    MBLS_DECODE_BAD_FLAGS = 5     /* C clear, or I set with S set or with any other bit set      */
} mbls_decode_status;

eIcicleError mbls_g1_decompress(const uint8_t* bytes, int size, bool points_montgomery, const VecOpsConfig* config,
                                mbls_g1_affine_t* points, uint8_t* status, uint64_t* n_invalid);
eIcicleError mbls_g2_decompress(const uint8_t* bytes, int size, bool points_montgomery, const VecOpsConfig* config,
                                mbls_g2_affine_t* points, uint8_t* status, uint64_t* n_invalid);
eIcicleError mbls_g1_compress(const mbls_g1_affine_t* points, int size, bool points_montgomery,
                              const VecOpsConfig* config, uint8_t* bytes);
eIcicleError mbls_g2_compress(const mbls_g2_affine_t* points, int size, bool points_montgomery,
                              const VecOpsConfig* config, uint8_t* bytes);

/* ------------------------------------------------------------------------------------ */
/* library utilities (no reference counterpart; used by the host API, tests and bench)   */
/* ------------------------------------------------------------------------------------ */
const char* mbls_version(void);
const char* mbls_error_string(eIcicleError e);
/* Fill `out` (device) with n synthetic scalars of stream `seed` (standard form if
 * montgomery == false).  Same stream as the oracle's orc_gen_scalars. */
eIcicleError mbls_gen_scalars(mbls_fr_t* out_device, uint64_t seed, size_t n, bool montgomery, void* stream);
/* Fill `out` (device) with P_i = k_i * G, k_i = scalar stream `seed` (affine Montgomery). */
eIcicleError mbls_gen_g1_bases(mbls_g1_affine_t* out_device, uint64_t seed, size_t n, void* stream);
eIcicleError mbls_gen_g2_bases(mbls_g2_affine_t* out_device, uint64_t seed, size_t n, void* stream);
/* The same streams from element `start` on (out[j] = element start + j): one rank of a sharded
 * run generates exactly its slice of the global inputs. */
eIcicleError mbls_gen_scalars_range(mbls_fr_t* out_device, uint64_t seed, size_t start, size_t n, bool montgomery,
                                    void* stream);
eIcicleError mbls_gen_g1_bases_range(mbls_g1_affine_t* out_device, uint64_t seed, size_t start, size_t n, void* stream);
eIcicleError mbls_gen_g2_bases_range(mbls_g2_affine_t* out_device, uint64_t seed, size_t start, size_t n, void* stream);
/* One rank's step of the sharded multi-GPU MSM (the reference has no
 * multi-GPU path): the inputs and flags of bls12_381_icicle_g*_msm, but the result is left
 * as the Jacobian Montgomery partial sum (no (x, y, 1) normalisation), so the partials of all
 * ranks can be all-gathered, added with mbls_g*_sum_jacobian and normalised once with
 * mbls_g*_jacobian_to_icicle. */
eIcicleError mbls_g1_msm_jacobian(const mbls_fr_t* scalars, const mbls_g1_affine_t* bases, int msm_size,
                                  const MSMConfig* config, mbls_g1_projective_t* results);
eIcicleError mbls_g2_msm_jacobian(const mbls_fr_t* scalars, const mbls_g2_affine_t* bases, int msm_size,
                                  const MSMConfig* config, mbls_g2_projective_t* results);
/* Sum `count` Jacobian-Montgomery points on device (the EC reduction after the multi-GPU
 * all-gather of partial MSM results). result: device pointer, Jacobian Montgomery. */
eIcicleError mbls_g1_sum_jacobian(const mbls_g1_projective_t* points_device, int count,
                                  mbls_g1_projective_t* result_device, void* stream);
eIcicleError mbls_g2_sum_jacobian(const mbls_g2_projective_t* points_device, int count,
                                  mbls_g2_projective_t* result_device, void* stream);
/* Jacobian Montgomery -> ICICLE standard projective (x, y, 1) / (0, 1, 0), in place on
 * device (reference icicle_curve_api.cu:134-229). */
eIcicleError mbls_g1_jacobian_to_icicle(mbls_g1_projective_t* points_device, int count, void* stream);
eIcicleError mbls_g2_jacobian_to_icicle(mbls_g2_projective_t* points_device, int count, void* stream);

/* Scratch ownership.  Device scratch comes from a small per-device pool of contexts (arena +
 * side streams) LEASED per call, never keyed by the caller's stream: the reference's async
 * MSM creates a stream per call and destroys it afterwards (core/msm.rs:742, stream.rs:189),
 * and the reference itself allocates and frees scratch inside every call
 * (msm_kernels.cu:705-719, :872-902).  Here a context's arena grows to the high-water mark and
 * is reused by later calls on any stream; no hipMalloc happens once it is large enough.
 *   mbls_release_stream: the stream is about to be destroyed (ICICLE DeviceAPI
 *     destroy_stream calls it): forget it as a context's last stream, so a new stream that
 *     reuses the handle value is never taken to be ordered after the old one's work.
 *   mbls_release_scratch: free the arenas of all idle contexts (after their last work).
 *   mbls_scratch_stats: library hipMalloc / hipFree counts of scratch arenas, bytes held,
 *     number of pool contexts (any pointer may be NULL). */
eIcicleError mbls_release_stream(void* stream);
eIcicleError mbls_release_scratch(void);
void mbls_scratch_stats(uint64_t* mallocs, uint64_t* frees, uint64_t* bytes, int* contexts);

/* Multi-device G1 MSM for a single-process caller (SURVEY.md section 8e in one process; the
 * reference's Rust core binds one device per process, core/config.rs:529-531, core/msm.rs:284).
 * Shard k = points [k*n/ndev, (k+1)*n/ndev) runs on device devs[k] against bases_per_dev[k]
 * (that shard's bases, resident on devs[k]; flags as config->are_points_*); `scalars` holds all
 * n scalars, on the host or on device devs[0] per config->are_scalars_on_device.  Each shard
 * leaves its Jacobian partial sum on its device, the partials (144 B each) are copied peer to
 * peer to devs[0], summed there and normalised once to ICICLE's (x, y, 1).  devs may repeat a
 * device (shards then run one after another on it).  `result`: host or device (devs[0]) per
 * config->are_results_on_device.  config->stream, if set, is a stream of devs[0]; the other
 * shards use library streams forked from it.  batch_size must be 1 and precompute_factor 1.
 * Concurrent multi-device calls from several host threads serialise (one library lock). */
eIcicleError mbls_g1_msm_multi_device(const mbls_fr_t* scalars, const mbls_g1_affine_t* const* bases_per_dev,
                                      const int* devs, int ndev, int msm_size, const MSMConfig* config,
                                      mbls_g1_projective_t* result);
/* the same for G2 (288-byte partials) */
eIcicleError mbls_g2_msm_multi_device(const mbls_fr_t* scalars, const mbls_g2_affine_t* const* bases_per_dev,
                                      const int* devs, int ndev, int msm_size, const MSMConfig* config,
                                      mbls_g2_projective_t* result);

/* ICICLE vector_sum with the staged semantics of the other vecops (host or device input,
 * batch_size sums of `size` elements, row-major batches; result host or device). */
eIcicleError bls12_381_vector_sum(const mbls_fr_t* a, size_t size, const VecOpsConfig* config, mbls_fr_t* output);

/* The MSM schedule the library picks for msm_size points under `config` (make_plan; host
 * only, no device work): out[0..9] = window bits c, windows W, windows per table block Wg, the
 * plan's precompute factor F (1 once a split plan takes the table), block shift sF (0: none),
 * split (1 none, 2 G1 GLV, 4 G2 psi), prepared endomorphism table (0 / 1), slot-0 stride (1:
 * none; F: the split plan on entry i F of a shift table), buckets, reduction levels.
 * group: 1 = G1, 2 = G2.  Diagnostics (tests/test_plan.py, tools/). */
eIcicleError mbls_msm_plan(int group, int msm_size, const MSMConfig* config, int32_t* out);

/* The bucket reduction's kernel schedule of that plan (plan_levels; host only, no device work,
 * the argument checks of mbls_msm_plan).  *count = the words of the answer, 2 + 7 x levels; with
 * capacity (the int32 words `out` holds) below that nothing else is written and the call returns
 * INVALID_ARGUMENT.  out[0] = bucket record format (0 Jacobian words, 1 raw XYZZ
 * limbs), out[1] = bytes of a level record, then per level l at out[2 + 7 l ..]: kernel (0
 * k_reduce_scaled, the generic chain in the level's mode; 1 k_reduce_tree4; 2 k_reduce_scaled_r28x;
 * 3 k_reduce_tree8_r28x; 4 k_reduce_scaled_r28px), index of the launch the level belongs to (the
 * tree8 launch covers two levels), mode (0 lane, 1 row, 2 wave), log2 of the segment length, inputs
 * per window, input record format, output record format.  Diagnostics (tests/test_plan.py). */
eIcicleError mbls_msm_reduce_plan(int group, int msm_size, const MSMConfig* config, int32_t* out, int capacity,
                                  int32_t* count);

/* The tables the MSM's front (digits, sort, chunk tables: msm_front) hands the accumulation and the
 * bucket sums, for one MSM of msm_size > 0 points under `config` (batch_size 1, the ICICLE entry's
 * flags).  The call does what an MSM does up to the front -- the same plan, chunk length, operand
 * staging and scratch region of the stream's leased arena --, fills the region with the byte 0xA5,
 * runs the front and copies table k out at the full capacity of its scratch block.
 * info[0..14] = c, W, Wg, F, sF, split, prepared, bstride, buckets per window B, buckets TB, chunk
 * length, point indices, contributions, partitioned sort (0 / 1), fused chunk counts (0 / 1);
 * info[15 + k] = the 32-bit words of table k: 0 sorted, 1 offsets, 2 nchunks (word TB the maximum,
 * TB + 1 the heavy buckets, TB + 2 their slices), 3 chunk_off, 4 owner, 5 first, 6 perm, 7 binbase,
 * 8..12 the heavy-bucket table's bucket, first, nslices, done, owner, 13 its group counters.
 * tables == NULL: only `info` is written, no device work.  Otherwise tables[k] is a host buffer of
 * info[15 + k] words, or NULL to leave table k out.  `bases` may be NULL for every plan without a
 * per-call image table (info[5] == 1 or info[6] == 1).  Diagnostics (tests/test_gpu_front.py). */
eIcicleError mbls_msm_front_probe(int group, const mbls_fr_t* scalars, const void* bases, int msm_size,
                                  const MSMConfig* config, int64_t* info, void* const* tables);

/* Stage profiler (tracing): hipEvent pairs recorded on the caller's
 * stream around each pipeline stage ("msm.accumulate", "ntt.pass", ...) when enabled
 * (or MBLS_PROFILE=1).  read() synchronises the recorded events and returns, per stage,
 * the total milliseconds and the number of recorded launches. */
void mbls_profile_enable(int on);
void mbls_profile_reset(void);
int mbls_profile_read(const char** names, double* total_ms, long* counts, int max);

/* Scheduling extension (no reference counterpart): the NEXT MSM call on `stream` takes `event`
 * and records it on that stream once its (last member's) bucket accumulation has been enqueued,
 * i.e. the event completes when the MSM enters its latency-bound tail (bucket sums, reduction
 * levels, final fold: ~2.5 ms of few-wave chains for G2 2^20).  Work made to wait on it from
 * another stream -- a batch of NTTs, say -- then fills the SIMDs the tail leaves idle instead of
 * time-slicing them with the VALU-bound accumulation (config #5, bench.py mix leg; give the MSM's
 * stream the higher priority).  Every MSM call that gets past its argument checks takes the
 * pending event: a batch records it after the LAST member's accumulation; an empty MSM, a
 * multi-device call (at its end, on the caller's stream) and a call that fails after taking it
 * record it where they stop, so it never lingers for an unrelated later MSM.  One pending event
 * per stream; a later call replaces it; mbls_msm_accumulate_event(stream, NULL) clears it.  The
 * event is the caller's: mbls_msm_accumulate_event_drop(event) removes every pending
 * registration of it (call it before destroying an event that may still be pending). */
eIcicleError mbls_msm_accumulate_event(void* stream, void* event);
eIcicleError mbls_msm_accumulate_event_drop(void* event);

/* precompute_factor guard (no reference counterpart).  The reference's plain
 * device-bases MSMs pass MIDNIGHT_GPU_PRECOMPUTE as precompute_factor with n PLAIN bases
 * (core/msm.rs:897-913).  Default: a device allocation too short for n x F entries runs as plain
 * bases (a sub-allocated buffer of a larger pool is not caught).  Strict (on != 0, process-wide):
 * precompute_factor > 1 is honoured only for a table this library's precompute_bases wrote to
 * device memory (same pointer, same factor, entries covering the call) and every other buffer
 * runs as plain bases -- exact for pooled buffers; a table assembled elsewhere (copied or
 * concatenated) then needs precompute_factor = 1 semantics or its own precompute_bases call. */
eIcicleError mbls_msm_precompute_strict(int on);

#ifdef __cplusplus
}
#endif
#endif /* BLS12_381_MI355X_H */
