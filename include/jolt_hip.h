/*
 * include/jolt_hip.h -- C ABI of the MI355X-native Jolt prover hot path (libjolt_hip.so).
 *
 * This is the drop-in boundary: the entry points below are what a thin Rust FFI crate (`jolt-kernels-hip`,
 * sketched in INTEGRATION.md) binds in order to implement the reference's own trait surface for this path --
 * `ProveRounds`/`SumcheckKernel`/`PrepareKernel` (jolt-sumcheck, jolt-kernels), `JoltGroup::msm` (jolt-crypto) and
 * `CommitmentScheme::{commit,open}` for HyperKZG (jolt-openings / jolt-hyperkzg) and, for Dory (jolt-dory), the commitment
 * and the prover's side of an evaluation proof as one call each under the caller's transcript.  Every function cites the
 * reference interface it replaces (paths relative to the a16z/jolt checkout).
 *
 * Conventions:
 *  - plain pointers and sizes only; every function returns an int32 status and never unwinds/aborts;
 *  - jolt_fr_t  = 4 x u64 little-endian Montgomery limbs, canonical (< r)   == jolt_field::Fr::inner_limbs()
 *                 (crates/jolt-field/src/bn254/mod.rs:33-43);
 *  - jolt_g1_t  = Jacobian (x, y, z) of Montgomery Fq limbs, identity <=> z == 0 == ark_bn254::G1Projective, which
 *                 jolt_crypto::Bn254G1 wraps #[repr(transparent)] (crates/jolt-crypto/src/ec/bn254/mod.rs:17-24);
 *  - handles are opaque and owned by the context that created them; a kernel/member owns its tables
 *    (Box<dyn SumcheckKernel> semantics) and frees them on destroy;
 *  - all work is enqueued on the context's HIP stream; functions that return field elements or points to host
 *    memory synchronise that stream before returning (the per-round Fiat-Shamir sync point,
 *    crates/jolt-sumcheck/src/prover.rs:326);
 *  - there is NO CPU fallback: without a usable gfx950 device jolt_ctx_create fails with JOLT_ERR_NO_DEVICE.
 */
#ifndef JOLT_HIP_H
#define JOLT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JOLT_HIP_ABI_VERSION 1

typedef struct { uint64_t l[4]; } jolt_fr_t;
typedef struct { uint64_t l[4]; } jolt_fq_t;
typedef struct { jolt_fq_t x, y, z; } jolt_g1_t;
typedef struct { jolt_fq_t c0, c1; } jolt_fq2_t;  /* c0 + c1 u, u^2 = -1 == ark_bn254::Fq2 */
typedef struct { jolt_fq2_t x, y, z; } jolt_g2_t; /* Jacobian on the twist y^2 = x^3 + 3 / (9 + u), identity <=> z == 0 == ark_bn254::G2Projective (dory's ArkG2) */

typedef struct jolt_ctx jolt_ctx;       /* device + stream + scratch                                  */
typedef struct jolt_table jolt_table;   /* device-resident dense table of Fr (Polynomial<Fr>)         */
typedef struct jolt_member jolt_member; /* one sumcheck batch member (Box<dyn SumcheckKernel>)        */
typedef struct jolt_srs jolt_srs;       /* device-resident affine SRS prefix (HyperKZGProverSetup.g1_powers) */

/* Status codes.  Mapping to the reference's error types (crates/jolt-kernels/src/error.rs:11-90,
 * crates/jolt-sumcheck/src/error.rs, crates/jolt-hyperkzg/src/error.rs) is given per value. */
enum {
    JOLT_OK = 0,
    JOLT_ERR_INVALID_ARG = 1,     /* KernelError::InvariantViolation (caller bug)                       */
    JOLT_ERR_NO_DEVICE = 2,       /* KernelError::Unsupported -> caller falls back to another backend   */
    JOLT_ERR_OOM = 3,             /* KernelError::Unsupported                                           */
    JOLT_ERR_HIP = 4,             /* KernelError::InvariantViolation, message via jolt_last_error       */
    JOLT_ERR_SIZE_MISMATCH = 5,   /* KernelError::TableSizeMismatch / msm length-mismatch panic         */
    JOLT_ERR_UNSUPPORTED = 6,     /* KernelError::Unsupported (descriptor beyond compiled limits)       */
    JOLT_ERR_NOT_FULLY_BOUND = 7, /* SumcheckKernelError::NotFullyBound                                 */
    JOLT_ERR_ROUND_CHECK = 8,     /* SumcheckError::RoundCheckFailed                                    */
    JOLT_ERR_SRS_TOO_SMALL = 9,   /* HyperKZGError::SrsTooSmall                                         */
    JOLT_ERR_EMPTY_POINT = 10,    /* HyperKZGError::EmptyPoint                                          */
    JOLT_ERR_NOT_INVERTIBLE = 11  /* gruen_poly_deg_3 `expect` (split_eq.rs:403-405)                    */
};

/* BindingOrder (crates/jolt-poly/src/binding.rs) */
enum { JOLT_ORDER_LOW_TO_HIGH = 0, JOLT_ORDER_HIGH_TO_LOW = 1 };

const char *jolt_status_string(int32_t status);
int32_t jolt_abi_version(void);

/* ------------------------------------------------------------------------------------------------------------
 * Context.  One per GPU per process (one process per GPU; ranks shard the hypercube).
 * `stream` = an existing hipStream_t to enqueue on (e.g. the caller's), or NULL to create a private one.
 * ---------------------------------------------------------------------------------------------------------- */
int32_t jolt_ctx_create(int32_t device_id, void *stream, jolt_ctx **out);
int32_t jolt_ctx_destroy(jolt_ctx *ctx);
int32_t jolt_ctx_synchronize(jolt_ctx *ctx);
/* ... without the background stream (jolt_grid_hint_begin's class sums may outlive the leg that began them): what a caller timing a leg waits for */
int32_t jolt_ctx_synchronize_foreground(jolt_ctx *ctx);
/* Select the context's device on the CALLING host thread (the runtime's current device is per thread).  Contexts are single-threaded objects; two contexts on one device may be
 * driven from two threads at once -- the stage operators of one protocol stage beside that stage's batched sumcheck, as the reference batches them (crates/jolt-prover/src/stages). */
int32_t jolt_ctx_bind_thread(jolt_ctx *ctx);
const char *jolt_last_error(const jolt_ctx *ctx);
/* Device memory of tables, members and temporaries comes from a per-context pool (a proof builds and drops dozens of T-sized
 * derived tables -- the Vec<Fr> allocations of EqPolynomial::evals & co. in the reference; hipMalloc / hipFree cost 0.1-1 ms each
 * and synchronise the device).  _trim returns the cached blocks to the runtime (synchronises); _memory_stats reports the bytes held
 * by live handles, cached by the pool, and the high-water mark of both (any pointer may be NULL). */
int32_t jolt_ctx_trim(jolt_ctx *ctx);
int32_t jolt_ctx_memory_stats(const jolt_ctx *ctx, size_t *live_bytes, size_t *cached_bytes, size_t *peak_bytes);
/* ... and what the context holds outside the pool: the grow-only workspaces of its MSM lanes and of the batch of short MSMs (bytes). */
int32_t jolt_ctx_workspace_stats(const jolt_ctx *ctx, size_t *msm_lane_bytes, size_t *msm_batch_bytes);
/* ... and the pair tables of the commitment grid built on this context's SRSs (jolt_srs_precompute_grid_pairs), bytes. */
int32_t jolt_ctx_grid_pairs_stats(const jolt_ctx *ctx, size_t *bytes);
/* Which kernel path the batch rounds of this context took: host-side launch counts since the context was created or the counts were last zeroed (a test names the
 * kernel it means to reach with them; nothing on the device reads or writes them).  counts[k], k < min(cap, JOLT_ROUND_PATH_COUNT), is the count of the enum below;
 * reset != 0 zeroes all of them after the copy (counts may be NULL to zero only). */
enum {
    JOLT_ROUND_PATH_TAIL = 0,             /* k_round_evals_tail launches                                                                    */
    JOLT_ROUND_PATH_GROUP = 1,            /* k_round_evals_group launches: 8 counts at GROUP + 4 * order + 2 * skip_one + fused             */
    JOLT_ROUND_PATH_SMALL = 9,            /* k_round_evals_small launches (integer-backed round 0)                                          */
    JOLT_ROUND_PATH_SPLIT_EQ_PRODUCT = 10, /* k_split_eq_product launches: unfused, then (+1) with the pending bind fused                    */
    JOLT_ROUND_PATH_UNIFORM_ITEMS = 12,   /* dense uniform member on (product, pair) items                                                  */
    JOLT_ROUND_PATH_UNIFORM_ROWS = 13,    /* dense uniform member rows-major (one item per pair)                                            */
    JOLT_ROUND_PATH_LAZY = 14,            /* every index-encoded form (uniform first / LDS / rows / items, booleanity) together             */
    JOLT_ROUND_PATH_BIND = 15,            /* grouped separate binds (one per challenge and order): LowToHigh, then (+1) HighToLow           */
    JOLT_ROUND_PATH_COUNT = 17
};
int32_t jolt_ctx_round_path_stats(jolt_ctx *ctx, uint64_t *counts, size_t cap, int32_t reset);
/* Device-event timing of everything enqueued between begin and end on the context's stream (milliseconds). */
int32_t jolt_timer_begin(jolt_ctx *ctx);
int32_t jolt_timer_end(jolt_ctx *ctx, float *elapsed_ms);

/* ------------------------------------------------------------------------------------------------------------
 * Tables: Polynomial<Fr> resident in HBM (crates/jolt-poly/src/dense.rs:36-39).
 * Replaces the host Vec<Fr> that `witness.oracle_table(id)` / `dense_view` hand to kernels
 * (crates/jolt-witness/src/backend/mod.rs:50-53, crates/jolt-kernels/src/reference/views.rs:20-33).
 * ---------------------------------------------------------------------------------------------------------- */
int32_t jolt_table_upload(jolt_ctx *ctx, const jolt_fr_t *host, size_t len, jolt_table **out);
int32_t jolt_table_from_device(jolt_ctx *ctx, const void *device_ptr, size_t len, jolt_table **out); /* D2D copy */
int32_t jolt_table_alloc(jolt_ctx *ctx, size_t len, jolt_table **out);                               /* zeroed   */
int32_t jolt_table_clone(jolt_ctx *ctx, const jolt_table *src, jolt_table **out);
/* Small-scalar promotion on device: Ring::from_u64 / from_i64 per entry (crates/jolt-field/src/bn254/mod.rs:265-292),
 * the device twin of Polynomial<T>::bind_to_field's `From<T>` (dense.rs:129-142). */
int32_t jolt_table_from_u64(jolt_ctx *ctx, const uint64_t *host, size_t len, jolt_table **out);
int32_t jolt_table_from_i64(jolt_ctx *ctx, const int64_t *host, size_t len, jolt_table **out);
int32_t jolt_table_download(jolt_ctx *ctx, const jolt_table *t, size_t offset, size_t len, jolt_fr_t *host);
int32_t jolt_table_len(const jolt_table *t, size_t *len);
int32_t jolt_table_device_ptr(const jolt_table *t, void **device_ptr); /* current evaluations, len*32 bytes */
int32_t jolt_table_free(jolt_ctx *ctx, jolt_table *t);
/* A read-only view of entries [offset, offset+len) of `parent` (which must outlive it); overwrite a range from the host. */
int32_t jolt_table_slice(jolt_ctx *ctx, const jolt_table *parent, size_t offset, size_t len, jolt_table **out);
int32_t jolt_table_write(jolt_ctx *ctx, jolt_table *t, size_t offset, const jolt_fr_t *host, size_t len);

/* Polynomial::bind_with_order on k tables in ONE launch (dense.rs:178-263; optimized/support.rs:224-231 bind_all):
 *   LowToHigh: t[y] <- t[2y] + r*(t[2y+1]-t[2y]);   HighToLow: t[i] <- t[i] + r*(t[i+half]-t[i]); len halves. */
int32_t jolt_bind(jolt_ctx *ctx, jolt_table *const *tables, size_t k, const jolt_fr_t *r, int32_t order);

/* EqPolynomial::evals(r, scaling_factor) (crates/jolt-poly/src/eq.rs:221-231): 2^n entries, big-endian index
 * (r[0] pairs the MSB); scale may be NULL (= one). */
int32_t jolt_eq_evals(jolt_ctx *ctx, const jolt_fr_t *r, size_t n, const jolt_fr_t *scale, jolt_table **out);
/* EqPolynomial::evals_for_aligned_block (eq.rs:238-263): entries [start, start+block) only -- the per-GPU shard. */
int32_t jolt_eq_evals_aligned_block(jolt_ctx *ctx, const jolt_fr_t *r, size_t n, size_t start, size_t block,
                                    jolt_table **out);
/* LtPolynomial::evaluations (crates/jolt-poly/src/lt.rs:115-117,144-156) */
int32_t jolt_lt_evals(jolt_ctx *ctx, const jolt_fr_t *r, size_t n, jolt_table **out);
/* EqPlusOnePolynomial::evals (crates/jolt-poly/src/eq_plus_one.rs:71-130): (eq, eq+1) tables */
int32_t jolt_eq_plus_one_evals(jolt_ctx *ctx, const jolt_fr_t *r, size_t n, const jolt_fr_t *scale, jolt_table **eq_out,
                               jolt_table **eq_plus_one_out);
/* Derived-table builders of the reference tier (crates/jolt-kernels/src/reference/views.rs:35-138):
 *   address_fold: out[j] = sum_k w[k] * grid[(k << log_t) | j]      (grid address-major K x T, w has K entries)
 *   cycle_fold:   out[k] = sum_j w[j] * grid[(k << log_t) | j]      (w has T entries)
 *   tile: `copies` concatenated copies of base;  replicate_stream_lsb: out[(t << 1) | s] = base[t] */
int32_t jolt_address_fold(jolt_ctx *ctx, const jolt_table *grid, const jolt_table *weights, jolt_table **out);
int32_t jolt_cycle_fold(jolt_ctx *ctx, const jolt_table *grid, const jolt_table *weights, jolt_table **out);
int32_t jolt_tile(jolt_ctx *ctx, const jolt_table *base, size_t copies, jolt_table **out);
int32_t jolt_replicate_stream_lsb(jolt_ctx *ctx, const jolt_table *base, jolt_table **out);
/* Joint polynomial sum_i scalars[i] * f_i of a homomorphic batch opening: RlcSource::to_dense
 * (crates/jolt-poly/src/multilinear.rs:159-170,358-464) as consumed by HomomorphicBatch::prove_batch
 * (crates/jolt-openings/src/schemes.rs:487-524); k <= 40 tables of equal length. */
int32_t jolt_rlc(jolt_ctx *ctx, jolt_table *const *tables, size_t k, const jolt_fr_t *scalars, jolt_table **out);
/* Polynomial::evaluate (dense.rs:340-366): sum_x t[x] * eq(x, point) */
int32_t jolt_table_evaluate(jolt_ctx *ctx, const jolt_table *t, const jolt_fr_t *point, size_t n, jolt_fr_t *out);
/* Sum of all entries (input claims of linear members; DenseMember::with_sum, jolt-sumcheck/src/tests.rs:1129-1135) */
int32_t jolt_table_sum(jolt_ctx *ctx, const jolt_table *t, jolt_fr_t *out);

/* ------------------------------------------------------------------------------------------------------------
 * Sumcheck members: the device twin of NaiveSumcheckProver (crates/jolt-kernels/src/reference/naive.rs:53-377),
 * serving every cycle-domain relation of SURVEY.md section 8 a13 from one descriptor, plus the split-eq product
 * member (optimized/support.rs:391-411, ram_hamming_booleanity.rs:111-135).
 *
 * Summand = sum_k coeffs[k] * prod_{f in term k} table[factors[f]]   (jolt_claims::Expr, claims.rs:17-46 with
 * Challenge leaves pre-folded into coeffs).  A term with no factors is a constant.
 * ---------------------------------------------------------------------------------------------------------- */
#define JOLT_MAX_MEMBER_TABLES 40
#define JOLT_MAX_MEMBER_TERMS 16
#define JOLT_MAX_MEMBER_FACTORS 64
#define JOLT_MAX_DEGREE 7

typedef struct {
    uint32_t n_tables;
    uint32_t n_terms;
    uint32_t degree;              /* relation.degree(): round polynomials have degree+1 evaluations            */
    int32_t order;                /* JOLT_ORDER_*; every T-scale member of the reference binds LowToHigh        */
    const uint32_t *term_offsets; /* n_terms+1 entries into `factors`                                          */
    const uint32_t *factors;      /* table indices                                                             */
    const jolt_fr_t *coeffs;      /* n_terms                                                                   */
} jolt_member_desc;

/* NaiveSumcheckProver::new (naive.rs:136-205).  Takes OWNERSHIP of the tables (they are freed with the member). */
int32_t jolt_member_create_expr(jolt_ctx *ctx, jolt_table *const *tables, const jolt_member_desc *desc, jolt_member **out);

/* The optimized tier's fused summands as a descriptor rewrite instead of a new kernel:
 *   summand = sum_g prod_{f in group g} ( factor_consts[f] + sum_k lc_coeffs[k] * table[lc_tables[k]] )
 * e.g. inc_claim_reduction's A = s1*eq(p1) + s2*eq(p2) linear-leaf fusion
 * (crates/jolt-kernels/src/optimized/inc_claim_reduction.rs:68-89) is one factor with two entries.
 * flags bit 0 = evaluate t in {0,2,..,degree} only and let the caller recover s(1) = claim - s(0)
 * (optimized/support.rs:450-459 round_poly_from_skipped_evals); prove_round then returns `degree` values. */
#define JOLT_MEMBER_FLAG_SKIP_ONE 1u
/* flags bit 1 = BORROW: the member only READS the given tables (they stay owned by the caller and must outlive it) and
 * binds into scratch of its own (N/2 + N/4 entries per table).  One resident witness table can then serve every
 * relation that mentions it and the PCS opening afterwards, instead of one `oracle_table` materialisation per kernel
 * (crates/jolt-kernels/src/reference/views.rs:20-33).  Borrowing members can be rewound with jolt_member_reset. */
#define JOLT_MEMBER_FLAG_BORROW_TABLES 2u
typedef struct {
    uint32_t n_tables, n_groups, n_factors, n_lc;
    uint32_t degree;
    int32_t order;
    uint32_t flags;
    const uint32_t *group_factor_offsets; /* n_groups+1  */
    const uint32_t *factor_lc_offsets;    /* n_factors+1 */
    const jolt_fr_t *factor_consts;       /* n_factors, or NULL = all zero */
    const uint32_t *lc_tables;            /* n_lc */
    const jolt_fr_t *lc_coeffs;           /* n_lc */
} jolt_member_lc_desc;
int32_t jolt_member_create_lc(jolt_ctx *ctx, jolt_table *const *tables, const jolt_member_lc_desc *desc, jolt_member **out);
/* eq(w, j) * a(j) * b(j), eq served from split tables (GruenSplitEqPolynomial::new_with_scaling(w, LowToHigh, scale),
 * crates/jolt-poly/src/split_eq.rs:187-236).  Takes ownership of a and b. */
int32_t jolt_member_create_split_eq_product(jolt_ctx *ctx, jolt_table *a, jolt_table *b, const jolt_fr_t *w, size_t n,
                                            const jolt_fr_t *scale, jolt_member **out);
int32_t jolt_member_create_split_eq_product_borrowed(jolt_ctx *ctx, jolt_table *a, jolt_table *b, const jolt_fr_t *w, size_t n,
                                                     const jolt_fr_t *scale, jolt_member **out);
/* eq(w, j) * sum_{v<V} coeffs[v] * prod_{i<F} tables[v*F+i](j), eq served from split tables -- the optimized tier's form of
 * instruction_ra_virtualization / ram_ra_virtualization / ram_hamming_booleanity.  F in {2,3,4},
 * V <= 16, degree F+1.  prove_round returns the F eq-stripped sums q(0), q(2), .., q(F); aux_out = {current_scalar,
 * w[current_index-1], 0}; the caller recovers q(1) from the running claim and multiplies by the linear eq factor
 * (GruenSplitEqPolynomial::gruen_poly_from_evals, crates/jolt-poly/src/split_eq.rs:419-447).
 * flags: JOLT_MEMBER_FLAG_BORROW_TABLES.  shard_scale may be NULL (see the sharded product variant below). */
/* eq(w,j) * q(j) for an arbitrary inner summand q in jolt_member_lc_desc form (degree = the INNER degree dq): the optimized tier's
 * shape for every "eq times something" relation (GruenRoundMessage, crates/jolt-kernels/src/optimized/support.rs:340-412;
 * instruction_input.rs:1-22, instruction_claim_reduction.rs).  No T-sized eq table is read or bound; prove_round returns
 * q(0), q(2), .., q(dq) (dq values); the round polynomial is l(t)*q(t) (jolt_host_gruen_poly_from_q).  LowToHigh only.
 * shard_scale (may be NULL) as in jolt_member_create_split_eq_product_sharded.  final_values appends the bound eq scalar. */
int32_t jolt_member_create_split_eq_lc(jolt_ctx *ctx, jolt_table *const *tables, const jolt_member_lc_desc *desc, const jolt_fr_t *w, size_t n,
                                       const jolt_fr_t *scale, const jolt_fr_t *shard_scale, jolt_member **out);
/* The two constructors above over COMPACT-SCALAR polynomials: slot i is tables[i] (a field table) or ints[i] (a resident JOLT_INT_U64 witness column, borrowed:
 * it must outlive the member) -- exactly one of the two per slot.  Replaces the optimized tier's Polynomial<T> members: round 0 multiplies field elements with
 * machine integers through the deferred-reduction accumulator (FrSmallScalarAccumulator / mul_u64, crates/jolt-field/src/bn254/mont.rs:286-305,343-427) and the
 * FIRST bind produces the field tables (Polynomial::bind_to_field, crates/jolt-poly/src/dense.rs:129-142); no promotion pass, 8 instead of 32 bytes per entry in
 * round 0.  w == NULL: jolt_member_create_lc (flags of `desc` honoured, tables always borrowed); w != NULL: jolt_member_create_split_eq_lc.  LowToHigh only.
 * Identical round sums and final values to the member over promoted tables (jolt_table_from_ints).  Other integer kinds: JOLT_ERR_UNSUPPORTED. */
typedef struct jolt_ints jolt_ints;
int32_t jolt_member_create_lc_small(jolt_ctx *ctx, jolt_table *const *tables, const jolt_ints *const *ints, const jolt_member_lc_desc *desc, const jolt_fr_t *w,
                                    size_t n, const jolt_fr_t *scale, const jolt_fr_t *shard_scale, jolt_member **out);
/* test hook (CPU suite): the per-pair evaluation of the integer round kernel compiled for the host -- one LowToHigh pair of a member in `desc` form; slot i is an
 * integer column iff is_int[i] (entries int_pairs[2i], [2i+1]; otherwise fr_pairs[2i], [2i+1]); out[s], s < n_evals <= 4: the summand at 0, 1, 2, .. (skip_one: 0, 2, 3, ..) */
int32_t jolt_host_small_round_pair(const jolt_member_lc_desc *desc, const uint8_t *is_int, const uint64_t *int_pairs, const jolt_fr_t *fr_pairs, uint32_t n_evals,
                                   int32_t skip_one, jolt_fr_t *out);
int32_t jolt_member_create_split_eq_uniform(jolt_ctx *ctx, jolt_table *const *tables, uint32_t V, uint32_t F, const jolt_fr_t *coeffs,
                                            const jolt_fr_t *w, size_t n, const jolt_fr_t *scale, const jolt_fr_t *shard_scale,
                                            uint32_t flags, jolt_member **out);
/* Sharded variant (one process per GPU): this rank holds rows of the block selected by the top log2 G
 * variables; `w` are the n local coordinates (the low ones), `scale` the global initial scalar and `shard_scale` =
 * eq(w_hi, rank) multiplies the E_out tables so that the ranks' partial sums simply add. Borrows a and b. */
int32_t jolt_member_create_split_eq_product_sharded(jolt_ctx *ctx, jolt_table *a, jolt_table *b, const jolt_fr_t *w, size_t n,
                                                    const jolt_fr_t *scale, const jolt_fr_t *shard_scale, jolt_member **out);
/* Rewind a BORROW member to round 0 (no device work). */
int32_t jolt_member_reset(jolt_member *m);
/* New scaling factor for a split-eq member that has bound nothing yet (GruenSplitEqPolynomial::new_with_scaling,
 * crates/jolt-poly/src/split_eq.rs:180-215): lets a reset member serve the next proof with another eq scalar. */
int32_t jolt_member_set_scale(jolt_member *member, const jolt_fr_t *scale);
int32_t jolt_member_num_rounds(const jolt_member *m, size_t *rounds);
int32_t jolt_member_degree(const jolt_member *m, uint32_t *degree);

/* ProveRounds::prove_round (crates/jolt-sumcheck/src/prover.rs:57-66), device half: bind `bind` (NULL on the
 * member's first active round -- the fused contract, prover.rs:45-51) and return the round sums.
 *   expr member     : evals_out[t] = s(t), t = 0..degree           (n_evals must be degree+1)
 *   split-eq member : evals_out = { q(0), q(inf) }, the eq-stripped endpoints that
 *                     gruen_poly_deg_3 (split_eq.rs:383-417) completes on the host (n_evals must be 2);
 *                     aux_out (3 entries, may be NULL) receives {current_scalar, w[current_index-1], 0}.
 * The caller (Rust: UnivariatePoly::from_evals, univariate.rs:198-202) interpolates and checks s(0)+s(1). */
int32_t jolt_member_prove_round(jolt_member *m, const jolt_fr_t *bind, jolt_fr_t *evals_out, size_t n_evals,
                                jolt_fr_t *aux_out);
/* All members of one batch round with as few launches/syncs as possible -- the BuildRoundScheduler hook
 * (crates/jolt-kernels/src/backend.rs:68-70, RoundScheduler::batch_prove_round prover.rs:110-115).
 * binds[i] may be NULL; evals_out is the concatenation of each member's evals (same layout as above). */
int32_t jolt_round_group_prove(jolt_ctx *ctx, jolt_member *const *members, size_t n_members, const jolt_fr_t *const *binds,
                               jolt_fr_t *evals_out, size_t evals_capacity);
/* ProveRounds::finish_rounds (prover.rs:68-71) */
int32_t jolt_member_finish(jolt_member *m, const jolt_fr_t *bind);
/* RoundScheduler::batch_finish_rounds (prover.rs:116-119): the final binds of all members in as few launches as possible */
int32_t jolt_round_group_finish(jolt_ctx *ctx, jolt_member *const *members, size_t n_members, const jolt_fr_t *const *binds);
/* SumcheckKernel::output_claims (naive.rs:331-347): every table's fully bound value, in table order; the split-eq
 * member appends its bound eq scalar (k = n_tables (+1)).  JOLT_ERR_NOT_FULLY_BOUND before the last bind. */
int32_t jolt_member_final_values(jolt_member *m, jolt_fr_t *out, size_t k);
/* sum over the hypercube of the summand (the claim a stage would consume; test/bench convenience) */
int32_t jolt_member_input_claim(jolt_member *m, jolt_fr_t *out);
int32_t jolt_member_destroy(jolt_member *m);

/* ------------------------------------------------------------------------------------------------------------
 * G1 MSM and HyperKZG prover pieces.
 * ---------------------------------------------------------------------------------------------------------- */
/* Upload bases once and keep them affine on the device -- replaces the per-call `into_affine` of every base in
 * Bn254G1::msm (crates/jolt-crypto/src/ec/bn254/mod.rs:205).  An MSM over bases[..n] uses the prefix. */
int32_t jolt_srs_upload_g1(jolt_ctx *ctx, const jolt_g1_t *bases, size_t n, jolt_srs **out);
/* HyperKZGScheme::setup_from_secret (crates/jolt-hyperkzg/src/scheme.rs:54-73): g1_powers[i] = beta^i * g1,
 * generated on the device (count = max_degree + 1). */
int32_t jolt_srs_setup_from_secret(jolt_ctx *ctx, const jolt_fr_t *beta, size_t count, const jolt_g1_t *g1, jolt_srs **out);
int32_t jolt_srs_len(const jolt_srs *srs, size_t *n);
int32_t jolt_srs_download(jolt_ctx *ctx, const jolt_srs *srs, size_t offset, size_t n, jolt_g1_t *out); /* z = 1 */
int32_t jolt_srs_free(jolt_ctx *ctx, jolt_srs *srs);
/* Fixed-base tables for an SRS that outlives many MSMs (HyperKZGProverSetup.g1_powers is built once per setup,
 * crates/jolt-hyperkzg/src/types.rs:105-108, and every kzg_commit / kzg_open_batch MSM multiplies a prefix of it): keep
 * 2^(c*w) * srs[i] for every c-bit window w resident, so that all windows of an MSM share ONE bucket set and c can grow to 23-26 bits
 * (11 instead of 16 windows of point additions for 254-bit scalars: scalars above r/2 are negated, the top window is unsigned; DESIGN.md
 * section 3.5c).  Costs ceil(253/c) copies of the bases in HBM, stored in the limb-form Montgomery radix of the bucket kernels.
 * window_bits = 0 picks c from the SRS length (23 from 2^24 points, else <= 24); MSMs over fewer than min_terms terms (0 = 2^(c-2)) keep
 * the per-window method.  Results are the same points. */
int32_t jolt_srs_precompute_windows(jolt_ctx *ctx, jolt_srs *srs, uint32_t window_bits, size_t min_terms);
/* Pair tables of the K x T commitment grid, for an SRS that has its window tables: on that grid a one-hot column adds, per cycle, one of only k
 * bases, so two consecutive cycles add one of k^2 sums.  For every shift s set in shift_mask (s <= 4), with the domain length D = cycles >> s, keep
 * PT_D[(m * k + a) * k + b] = srs[a * D + 2m] + srs[b * D + 2m + 1] (m < D / 2; a, b < k) resident as affine points in the bucket kernels' radix:
 * jolt_grid_commit_onehot (s = 0), jolt_grid_commit_onehot_classes and jolt_grid_hint_begin (s = shift / level) then add one entry per pair of hot
 * cycles instead of two bases.  The tables depend on the SRS, k and D alone.  32 k^2 D bytes per table (k = 16, D = 2^22: 32 GiB).  Needs
 * k <= 16, cycles a power of two >= 2 << s and k * cycles <= the SRS; a table that cannot be built (shape, memory) is left out, the SRS stays as
 * it was and the call still returns JOLT_OK -- the sums then run on the single bases.  Results are the same points either way.
 * _bytes: the size of the table for (k, D), 0 when there is none. */
int32_t jolt_srs_precompute_grid_pairs(jolt_ctx *ctx, jolt_srs *srs, uint32_t k, size_t cycles, uint32_t shift_mask);
int32_t jolt_srs_grid_pairs_bytes(const jolt_srs *srs, uint32_t k, size_t domain, size_t *bytes);
/* The entry arithmetic and the index map of those tables compiled for the host (csrc/grid_pairs.hip.h): out_words = the 8 words (x, y) stored for
 * p + q -- (0, 0) for the point at infinity --, readable by jolt_host_g1_sum_limb_form. */
int32_t jolt_host_grid_pair_entry(const jolt_g1_t *p, const jolt_g1_t *q, uint64_t *out_words);
int32_t jolt_host_grid_pair_index(size_t m, uint32_t k, uint32_t a, uint32_t b, size_t *out);

/* Measurement hook (no reference counterpart): HIP events around the dominant kernel of a fixed-base MSM (the bucket sums, k_fx_buckets_ordered) on the stream it is
 * launched on, and the number of mixed additions of that launch (the non-zero signed digits of its scalars).  bench.py's `roofline_msm` divides the two. */
int32_t jolt_msm_profile_buckets(jolt_ctx *ctx, int32_t enable);
int32_t jolt_msm_profile_buckets_last(jolt_ctx *ctx, float *ms, uint64_t *additions);
/* Test hook (no reference counterpart): the plan of the context's last fixed-base MSM -- which sort kernels ran is a function of the window bits, the term count and
 * the caller's full-width mark, and a test that means one path must fail when the call took another.  words[cap >= JOLT_FX_PLAN_WORDS]: what the enqueue decided on
 * the host, then three words the sort left on the device (read after the MSM's stream has drained; JOLT_FX_PLAN_STALE once a later per-window MSM or Dory batch
 * has reused the workspace they live in).  An MSM the fixed-base method refused (JOLT_ERR_UNSUPPORTED inside, the per-window method ran) leaves the plan before it.
 * JOLT_ERR_INVALID_ARG while the context has run no fixed-base MSM. */
enum {
    JOLT_FX_PLAN_C = 0,               /* window bits of the table set                                                                      */
    JOLT_FX_PLAN_W = 1,               /* windows: ceil(253 / c)                                                                            */
    JOLT_FX_PLAN_LO_BITS = 2,         /* log2 of the buckets per segment: 8, or 11 above 24-bit windows                                    */
    JOLT_FX_PLAN_SOA = 3,             /* the scalar-fed sort with split entries (no key array)                                             */
    JOLT_FX_PLAN_WIDE = 4,            /* W = 13: the second instantiation of the scalar-fed passes                                         */
    JOLT_FX_PLAN_CAPACITY = 5,        /* capacity regions in place of the histogram pass                                                   */
    JOLT_FX_PLAN_TWO_PASS = 6,        /* the two partition passes are available (0: the one-pass k_fx_scatter on the key-array path)       */
    JOLT_FX_PLAN_GRID_REDUCE = 7,     /* reduction by rows and columns (0: running sums)                                                   */
    JOLT_FX_PLAN_HEAVY_THRESHOLD = 8, /* a bucket with more entries is summed in segments of 128                                           */
    JOLT_FX_PLAN_STAGE_CAP = 9,       /* entries of LDS stage handed to k_fx_segment_sort_staged (0: 11-bit segments, k_fx_segment_sort)   */
    JOLT_FX_PLAN_NB1 = 10,            /* segments                                                                                          */
    JOLT_FX_PLAN_MAX_LDS = 11,        /* the device's LDS bytes per workgroup the plan was made with                                       */
    JOLT_FX_PLAN_OVERFLOW = 12,       /* device: a capacity region overflowed and the exact passes redid the sort (0 without CAPACITY)     */
    JOLT_FX_PLAN_LARGEST_SEGMENT = 13, /* device: entries of the largest segment (the largest region after a capacity sort that held)      */
    JOLT_FX_PLAN_HEAVY_SEGMENTS = 14, /* device: 128-entry segments of over-full buckets                                                   */
    JOLT_FX_PLAN_WORDS = 15
};
#define JOLT_FX_PLAN_STALE 4294967295u
int32_t jolt_msm_fixed_last_plan(jolt_ctx *ctx, uint32_t *words, size_t cap);
/* Measurement hook (no reference counterpart; SURVEY.md section 8d: "the run must print the peak it divides by"): the chip-wide issue rate of v_mad_u64_u32 -- the
 * instruction the bucket sums are bound by -- measured now, on this context's device: a register-only loop of independent 64-bit multiply-adds launched until
 * >= target_ms of kernel time have been timed with HIP events on the context's stream; *mads_per_s = the best launch's lane-operations per second.
 * timed_ms / launches (optional): what was timed. */
int32_t jolt_ctx_measure_mad_peak(jolt_ctx *ctx, float target_ms, double *mads_per_s, float *timed_ms, uint32_t *launches);

/* JoltGroup::msm(bases, scalars) (crates/jolt-crypto/src/ec/group.rs:63-70, bn254/mod.rs:195-212) with the bases
 * = srs[..n].  Length mismatch (n > srs length) is JOLT_ERR_SRS_TOO_SMALL (the Rust shim asserts equal lengths
 * before calling, keeping the reference's panic).  Scalars from host memory or from a device table. */
int32_t jolt_msm_g1(jolt_ctx *ctx, const jolt_srs *srs, const jolt_fr_t *scalars, size_t n, jolt_g1_t *out);
int32_t jolt_msm_g1_table(jolt_ctx *ctx, const jolt_srs *srs, const jolt_table *scalars, size_t n, jolt_g1_t *out);
/* the same for scalars the caller knows to be full-width field elements (a polynomial folded by a challenge): mid-length MSMs may then use the mid window-table set */
int32_t jolt_msm_g1_table_full_width(jolt_ctx *ctx, const jolt_srs *srs, const jolt_table *scalars, size_t n, jolt_g1_t *out);
/* Up to three prefix MSMs in flight together on the side lanes, collected later: the dense columns of CommitWitness::commit_witness
 * (crates/jolt-kernels/src/commitment.rs:137-160, one kzg_commit per committed polynomial) while the caller commits its one-hot columns
 * (jolt_grid_commit_onehot) on the main stream in between.  begin: JOLT_ERR_UNSUPPORTED, with nothing enqueued, for count > 3 or a context with fewer lanes (the caller
 * then commits one by one).  Between begin and finish no other MSM entry point of the context may be called (JOLT_ERR_INVALID_ARG); finish frees the handle
 * whatever it returns; out[i] = sum_{k < n[i]} scalars[i][k] * srs[k]. */
typedef struct jolt_msm_pending jolt_msm_pending;
int32_t jolt_msm_g1_tables_begin(jolt_ctx *ctx, const jolt_srs *srs, const jolt_table *const *scalars, const size_t *n, size_t count, jolt_msm_pending **out);
int32_t jolt_msm_g1_tables_finish(jolt_ctx *ctx, jolt_msm_pending *pending, jolt_g1_t *out);

/* fold_polynomials (crates/jolt-hyperkzg/src/scheme.rs:88-114): levels_out[0] = clone of evals, then ell-1
 * LowToHigh folds with point[ell-1], ..., point[1]; ell output tables of length 2^ell, ..., 2. */
int32_t jolt_hyperkzg_fold(jolt_ctx *ctx, const jolt_table *evals, const jolt_fr_t *point, size_t ell, jolt_table **levels_out);
/* v[t][j] = P_j(u_t) (eval_univariate, crates/jolt-hyperkzg/src/kzg.rs:51-59,84-85): v_out is 3*ell, row-major */
int32_t jolt_hyperkzg_eval3(jolt_ctx *ctx, jolt_table *const *levels, size_t ell, const jolt_fr_t u[3], jolt_fr_t *v_out);
/* B = sum_j q^j * P_j (kzg.rs:95-105), length = len(levels[0]) */
int32_t jolt_hyperkzg_rlc(jolt_ctx *ctx, jolt_table *const *levels, size_t ell, const jolt_fr_t *q, jolt_table **out);
/* compute_witness_polynomial (kzg.rs:34-46): h = f / (x - u), len(f)-1 entries (parallel scan of the Horner
 * recurrence, exact). */
int32_t jolt_hyperkzg_witness_poly(jolt_ctx *ctx, const jolt_table *f, const jolt_fr_t *u, jolt_table **out);

/* ------------------------------------------------------------------------------------------------------------
 * Host-side mirror (C++ in this repo because the image has no Rust toolchain): the reference's callers of the path
 * restated above the C ABI so that the parity tests read like the reference's own.  In a Rust deployment these stay
 * in jolt-sumcheck / jolt-hyperkzg; they are exported here for tests and bench only.
 * ---------------------------------------------------------------------------------------------------------- */
/* Host field helpers used by round-message assembly (no GPU needed). */
int32_t jolt_host_fr_mul(const jolt_fr_t *a, const jolt_fr_t *b, jolt_fr_t *out);
int32_t jolt_host_fr_add(const jolt_fr_t *a, const jolt_fr_t *b, jolt_fr_t *out);
int32_t jolt_host_fr_sub(const jolt_fr_t *a, const jolt_fr_t *b, jolt_fr_t *out);
int32_t jolt_host_fr_inv(const jolt_fr_t *a, jolt_fr_t *out);
int32_t jolt_host_fr_from_u64(uint64_t v, jolt_fr_t *out);
int32_t jolt_host_fr_mul_shifted(const jolt_fr_t *a, const jolt_fr_t *c, jolt_fr_t *out); /* c low limbs must be 0 */
/* EqPolynomial::evals_serial (crates/jolt-poly/src/eq.rs:299-315) on the host, n <= 20: the K-entry address tables of one-hot members */
int32_t jolt_host_eq_evals(const jolt_fr_t *r, size_t n, const jolt_fr_t *scale, jolt_fr_t *out);
/* the kernels' multiplication algorithm (nine 29-bit limbs, product scanning) compiled for the host; field 0 = Fr, 1 = Fq */
int32_t jolt_host_mul_limbs29(int32_t field, const jolt_fr_t *a, const jolt_fr_t *b, jolt_fr_t *out);
/* The limb-form Fq arithmetic of the MSM's bucket sums (csrc/fq_limb.hip.h: 2^261 Montgomery radix, lazy reduction, dedicated squaring,
 * two-product reduction) and its XYZZ mixed addition, compiled for the host for the CPU suite.  Operands and results are canonical Fq /
 * affine points in STANDARD Montgomery form.  op: 0 a*b, 1 a^2, 2 a*b + c*d, 3 (a - b)*c, 4 (a - b - 2c)*d. */
int32_t jolt_host_fq_limb_op(int32_t op, const jolt_fr_t *a, const jolt_fr_t *b, const jolt_fr_t *c, const jolt_fr_t *d, jolt_fr_t *out);
int32_t jolt_host_g1_sum_limb_form(const uint64_t *points, const uint8_t *negate, size_t count, jolt_g1_t *out);
int32_t jolt_host_g1xl_add_paths(const uint32_t *acc, const uint32_t *q, int32_t negate, uint32_t *common, uint32_t *full, uint32_t *step, int32_t *suspect, uint32_t *canon);
/* The signed-digit recoding of the fixed-base MSM for one scalar (negation above r / 2, c-bit signed windows, unsigned top window), built for
 * the host: keys_out[w] = |digit_w| | sign << 31 for w < ceil(253 / c); *buckets_out = the bucket count of a table set with this c. */
int32_t jolt_host_fx_digits(const jolt_fr_t *scalar, uint32_t window_bits, uint32_t *keys_out, uint32_t *n_windows_out, uint32_t *buckets_out);
/* ... and the size of the REGION the capacity sort gives segment `segment` (256 buckets) of an n-term MSM over uniform scalars: expected digits + 8 standard deviations + 64
 * (msm_fixed.hip section 2d; the sort falls back to exact offsets on the device when a region overflows).  Host code, for the CPU suite. */
int32_t jolt_host_fx_segment_capacity(uint64_t n, uint32_t window_bits, uint32_t segment, uint32_t *capacity);
/* UnivariatePoly::from_evals / evaluate (crates/jolt-poly/src/univariate.rs:198-202) */
int32_t jolt_host_univariate_from_evals(const jolt_fr_t *evals, size_t n, jolt_fr_t *coeffs_out);
int32_t jolt_host_univariate_evaluate(const jolt_fr_t *coeffs, size_t n, const jolt_fr_t *x, jolt_fr_t *out);
/* s(t) = l(t) q(t) from q(0), q(2), .., q(dq) and the claim s(0)+s(1) (split_eq.rs:419-447 gruen_poly_from_evals, with the
 * evaluation set of the device kernel): dq + 2 coefficients. */
int32_t jolt_host_gruen_poly_from_q(const jolt_fr_t *current_scalar, const jolt_fr_t *point_i, const jolt_fr_t *q_evals, size_t dq,
                                    const jolt_fr_t *s0_plus_s1, jolt_fr_t *coeffs_out);
/* GruenSplitEqPolynomial::gruen_poly_deg_3 (split_eq.rs:383-417): 4 coefficients */
int32_t jolt_host_gruen_poly_deg_3(const jolt_fr_t *current_scalar, const jolt_fr_t *point_i, const jolt_fr_t *q_constant,
                                   const jolt_fr_t *q_quadratic, const jolt_fr_t *s0_plus_s1, jolt_fr_t *coeffs_out);
/* Booleanity address phase (stage 6a), host half: OptimizedBooleanityAddressKernel::{prove_round, bind} (crates/jolt-kernels/src/optimized/
 * booleanity.rs:320-398) over the K-entry pushforward masses of jolt_onehot_pushforward (K = 2^log_k_chunk = 16 .. 256 points: the reference
 * keeps this loop on the host, :46-49).  Tables are n_polys rows of `stride` entries with the first `len` live; weights[i] = gamma^(2i);
 * round returns s(0..3) for UnivariatePoly::from_evals; bind halves `len` (linear and eq as multilinears, squared with (1-r)^2 / r^2). */
int32_t jolt_host_booleanity_address_round(const jolt_fr_t *linear, const jolt_fr_t *squared, size_t n_polys, size_t stride, size_t len,
                                           const jolt_fr_t *weights, const jolt_fr_t *eq_address, jolt_fr_t *evals_out);
int32_t jolt_host_booleanity_address_bind(jolt_fr_t *linear, jolt_fr_t *squared, size_t n_polys, size_t stride, size_t len, jolt_fr_t *eq_address,
                                          const jolt_fr_t *challenge);
/* Hamming-weight claim reduction (stage 7), host half: HammingWeightKernel (crates/jolt-kernels/src/optimized/hamming_weight_claim_reduction.rs:150-300) over the
 * K_chunk-entry pushforward masses G_i of all RA columns (jolt_onehot_pushforward against eq(r_cycle, .): the relation's one T-scale pass, :83-117).
 *   weights: W_i(k) = gamma^(3i) + gamma^(3i+1) eq(r_address, k) + gamma^(3i+2) eq(virtualization_points[i], k)  (:187-207), n_polys rows of 2^log_k entries;
 *   round:   evals_out = {s(0), s(2), sum_i sum_k G_i(k) W_i(k)} of the summand sum_i G_i W_i (group_evals :255-266; the caller recovers s(1) from the running
 *            claim, round_poly_from_skipped_evals; the third value is the input claim before the first round);
 *   bind:    every table bound as a multilinear, low variable first (:243-252); the output claims are the bound G_i.
 * Tables are n_polys rows of `stride` entries with the first `len` live. */
int32_t jolt_host_hamming_weights(const jolt_fr_t *gamma, const jolt_fr_t *r_address, const jolt_fr_t *virtualization_points, size_t n_polys, size_t log_k,
                                  jolt_fr_t *out);
int32_t jolt_host_pair_tables_round(const jolt_fr_t *g, const jolt_fr_t *w, size_t n_polys, size_t stride, size_t len, jolt_fr_t *evals_out /* 3 */);
int32_t jolt_host_pair_tables_bind(jolt_fr_t *g, jolt_fr_t *w, size_t n_polys, size_t stride, size_t len, const jolt_fr_t *challenge);
/* The Fiat-Shamir surface of members the caller drives round by round outside prove_batch (RamReadWriteKernel's rounds, the read-RAF
 * phases): Transcript::{new, append_bytes, append, challenge, challenge_scalar, state} (crates/jolt-transcript/src/legacy.rs:32-100) and the
 * reference's encodings of what the path absorbs -- a field element as 32 BIG-endian bytes (legacy.rs:116-123), Label / LabelWithCount / U64Word
 * (legacy.rs:146-209), a compressed labelled round polynomial (crates/jolt-sumcheck/src/round_proof.rs:129-143: LabelWithCount(label, n - 1), the
 * constant, the coefficients of degree >= 2).  Three engines; every `transcript_label` argument of this header selects one with its two top bits:
 *   JOLT_TRANSCRIPT_TEST (0)            the deterministic test transcript of rounds 1-5;
 *   JOLT_TRANSCRIPT_BLAKE2B_LEGACY (1)  jolt_transcript::LegacyBlake2bTranscript = DigestTranscript<Blake2b<U32>> (crates/jolt-transcript/src/digest.rs:84-189),
 *                                       the transcript of the reference's benchmark profile (crates/jolt-prover/src/profile.rs:69,726);
 *   JOLT_TRANSCRIPT_KECCAK_SPONGE (2)   jolt_transcript::KeccakTranscript = SpongeTranscript<spongefish Keccak> (legacy.rs:211-305), pinned by the reference's
 *                                       known-answer vector (crates/jolt-transcript/tests/keccak_tests.rs:13-29).
 *   JOLT_TRANSCRIPT_BLAKE2B_SPONGE (3)  jolt_transcript::Blake2bTranscript = SpongeTranscript<spongefish Blake2b512> (lib.rs:63-66); the reference's vector
 *                                       (tests/blake2b_tests.rs:13-37) pins it through the first challenge only -- unpinned beyond, used by no parity claim.
 * For engines 1 - 3 an integer label L names the session "jolt-amd/<L mod 2^62>" (ASCII); _create_labelled takes the reference's byte labels (b"Jolt").
 * A Rust caller keeps its own transcript object and never calls these (jolt_round_transcript_fn / jolt_open_transcript_fn are its hooks). */
enum { JOLT_TRANSCRIPT_TEST = 0, JOLT_TRANSCRIPT_BLAKE2B_LEGACY = 1, JOLT_TRANSCRIPT_KECCAK_SPONGE = 2, JOLT_TRANSCRIPT_BLAKE2B_SPONGE = 3 };
#define JOLT_TRANSCRIPT_LABEL(kind, label) (((uint64_t)(kind) << 62) | ((uint64_t)(label) & (((uint64_t)1 << 62) - 1)))
typedef struct jolt_host_transcript jolt_host_transcript;
int32_t jolt_host_transcript_create(uint64_t label, jolt_host_transcript **out);
int32_t jolt_host_transcript_create_labelled(int32_t kind, const uint8_t *label, size_t label_len, jolt_host_transcript **out); /* label_len <= 32 (MAX_LABEL_LEN) */
int32_t jolt_host_transcript_append_fr(jolt_host_transcript *t, const jolt_fr_t *values, size_t count); /* 32 big-endian bytes each, one append per value */
int32_t jolt_host_transcript_append_bytes(jolt_host_transcript *t, const uint8_t *bytes, size_t count); /* e.g. a compressed G1 point (32 bytes) */
int32_t jolt_host_transcript_append_label(jolt_host_transcript *t, const char *label, int32_t with_count, uint64_t count); /* Label (<= 32 bytes) / LabelWithCount (<= 24) */
int32_t jolt_host_transcript_append_u64_word(jolt_host_transcript *t, uint64_t value);
int32_t jolt_host_transcript_append_round_poly(jolt_host_transcript *t, const char *label, const jolt_fr_t *coefficients, size_t count); /* all `count` coefficients in; the linear one is skipped */
int32_t jolt_host_transcript_challenge(jolt_host_transcript *t, int32_t full_width, jolt_fr_t *out);    /* 0: 125-bit challenge shape */
int32_t jolt_host_transcript_state(const jolt_host_transcript *t, uint8_t *out32);
int32_t jolt_host_transcript_destroy(jolt_host_transcript *t);
/* The framing of HomomorphicBatch::prove_batch (crates/jolt-openings/src/schemes.rs:487-524) around a scheme's own messages; scheme-agnostic, host only.
 *   _statement_absorb: LabelWithCount(b"rlc_claims", n), then each evaluation as a field element (VerifierRlcClaims, crates/jolt-openings/src/claims.rs:79-88);
 *     then challenge_scalar_powers(n) (crates/jolt-transcript/src/legacy.rs:82-91): powers_out = 1, gamma, gamma^2, ... from ONE challenge_scalar.  n == 0 is
 *     JOLT_ERR_INVALID_ARG (the reference refuses an empty batch).
 *   _claim_absorb: LabelWithCount(b"opening_point", n_vars), the coordinates in the order given, Label(b"opening_eval"), the value (EvaluationClaim, claims.rs:23-35).
 * A value that is not canonical is JOLT_ERR_INVALID_ARG, with nothing absorbed. */
int32_t jolt_host_opening_statement_absorb(jolt_host_transcript *t, const jolt_fr_t *evaluations, size_t n, jolt_fr_t *powers_out /* n */);
int32_t jolt_host_opening_claim_absorb(jolt_host_transcript *t, const jolt_fr_t *point, size_t n_vars, const jolt_fr_t *value);
/* the two hash primitives behind engines 1 and 2, for known-answer tests: BLAKE2b (RFC 7693, unkeyed, 1..64 digest bytes), Keccak-f[1600] on a 200-byte state */
int32_t jolt_host_blake2b(const uint8_t *in, size_t n, size_t outlen, uint8_t *out);
int32_t jolt_host_keccak_f1600(uint8_t *state200);
/* G1 helpers on the host: group law, equality as points, compressed serialisation
 * (crates/jolt-crypto/src/ec/bn254/mod.rs:139-171) */
int32_t jolt_host_g1_add(const jolt_g1_t *p, const jolt_g1_t *q, jolt_g1_t *out);
int32_t jolt_host_g1_eq(const jolt_g1_t *p, const jolt_g1_t *q, int32_t *equal);
/* canonical coordinates on y^2 = x^3 + 3 (Jacobian: Y^2 = X^3 + 3 Z^6) or the identity: the check applied to points supplied by the caller (known level commitments) */
int32_t jolt_host_g1_is_on_curve(const jolt_g1_t *p, int32_t *on_curve);
int32_t jolt_host_g1_serialize_compressed(const jolt_g1_t *p, uint8_t out[32]);

/* jolt_sumcheck::prove_batch (crates/jolt-sumcheck/src/prover.rs:193-362) over device members with the
 * deterministic test transcript of oracle/mock_transcript.h (spec in that header; re-implemented, not shared).
 *   out_polys         max_num_vars x (max_degree+1) batched coefficients
 *   out_challenges    max_num_vars
 *   out_member_claims n_members,  out_final_claim 1
 * challenge_mode 0 = Transcript::challenge (125-bit), 1 = challenge_scalar (full width). */
int32_t jolt_host_prove_batch(jolt_ctx *ctx, jolt_member *const *members, size_t n_members, const jolt_fr_t *input_claims,
                              const jolt_fr_t *coefficients, const size_t *offsets, size_t max_num_vars, size_t max_degree,
                              uint64_t transcript_label, int32_t challenge_mode, int32_t use_round_group,
                              jolt_fr_t *out_polys, jolt_fr_t *out_challenges, jolt_fr_t *out_member_claims,
                              jolt_fr_t *out_final_claim);
/* Resumable form of the same round loop for the hypercube-sharded prover: local round sums come
 * from the device members (local_fn == NULL) or from a callback, are all-gathered over the ranks through `gather` and added
 * mod r; the loop can be paused after the shard-local rounds and resumed on members built from the gathered tables.
 * kinds: 0 = expr (degree+1 sums), 1 = expr with skipped s(1) (degree sums), 2 = split-eq product (2 sums: q(0), q(inf) -> gruen_poly_deg_3),
 * 3 = split-eq uniform product or eq-weighted member (degrees[i] - 1 sums q(0), q(2), .., q(degree-1) -> gruen_poly_from_q). */
typedef struct jolt_batch jolt_batch;
typedef int32_t (*jolt_local_round_fn)(void *user, const size_t *active, size_t n_active, const jolt_fr_t *const *binds,
                                       jolt_fr_t *evals_out, size_t evals_count);
typedef int32_t (*jolt_gather_fn)(void *user, const jolt_fr_t *local, size_t count, jolt_fr_t *gathered /* world*count */);
int32_t jolt_host_batch_begin(jolt_ctx *ctx, size_t n_members, const jolt_fr_t *input_claims, const jolt_fr_t *coefficients,
                              const size_t *rounds, const size_t *offsets, const int32_t *kinds, const uint32_t *degrees,
                              const jolt_fr_t *const *split_eq_points, const jolt_fr_t *split_eq_scales, size_t max_num_vars,
                              size_t max_degree, uint64_t transcript_label, int32_t challenge_mode, jolt_batch **out);
int32_t jolt_host_batch_run(jolt_batch *b, jolt_member *const *members, size_t n_rounds, int32_t world, jolt_gather_fn gather,
                            jolt_local_round_fn local_fn, void *user);
/* The batch's Fiat-Shamir: by default the deterministic test transcript; with a callback the CALLER's transcript
 * (ClearSumcheckRecorder::absorb_round, crates/jolt-sumcheck/src/recorder.rs:118-130): every round the loop hands over the batched
 * round polynomial in compressed form (coefficients without the linear term) and takes the challenge back.  All ranks of a sharded
 * batch must return the same challenge (they absorb the same summed polynomial).  fn = NULL restores the test transcript. */
typedef int32_t (*jolt_round_transcript_fn)(void *user, const jolt_fr_t *compressed_coeffs, size_t n_coeffs, jolt_fr_t *challenge_out);
int32_t jolt_host_batch_set_transcript(jolt_batch *b, jolt_round_transcript_fn fn, void *user);
int32_t jolt_host_batch_flush_binds(jolt_batch *b, jolt_member *const *members, jolt_fr_t *binds_out, int32_t *has_bind_out);
int32_t jolt_host_batch_split_eq_scalar(const jolt_batch *b, size_t member, jolt_fr_t *out);
int32_t jolt_host_batch_end(jolt_batch *b, jolt_fr_t *out_polys, jolt_fr_t *out_challenges, jolt_fr_t *out_member_claims,
                            jolt_fr_t *out_final_claim);
/* SplitLt (crates/jolt-kernels/src/optimized/support.rs:640-760): LT(., r_cycle) + constant from ~sqrt(T) split tables, bound
 * low-to-high; values equal the dense jolt_lt_evals table (plus the constant) bound identically.  constant may be NULL. */
typedef struct jolt_split_lt jolt_split_lt;
int32_t jolt_split_lt_create(jolt_ctx *ctx, const jolt_fr_t *r_cycle, size_t n, const jolt_fr_t *constant, jolt_split_lt **out);
int32_t jolt_split_lt_bind(jolt_ctx *ctx, jolt_split_lt *s, const jolt_fr_t *r);
int32_t jolt_split_lt_len(const jolt_split_lt *s, size_t *len);
int32_t jolt_split_lt_to_dense(jolt_ctx *ctx, const jolt_split_lt *s, jolt_table **out); /* all current evaluations (pair(y) for every y) */
int32_t jolt_split_lt_final_value(jolt_ctx *ctx, const jolt_split_lt *s, jolt_fr_t *out); /* JOLT_ERR_NOT_FULLY_BOUND before the last bind */
int32_t jolt_split_lt_free(jolt_ctx *ctx, jolt_split_lt *s);

/* sum_k a[k]*b[k] with ONE deferred Montgomery reduction per block of products: the deferred-reduction accumulator the round
 * kernels use for sums of products (WideAccumulator, crates/jolt-field/src/bn254/mont.rs:334-602; Accumulator contract
 * crates/jolt-field/src/algebra.rs:362-433).  Host build of the kernels' code; the value equals the plain field sum. */
int32_t jolt_host_fr_wide_dot(const jolt_fr_t *a, const jolt_fr_t *b, size_t n, jolt_fr_t *out);
/* The same accumulator ON THE DEVICE: sum_i a[i] * b[i] over two tables with plain field sums (deferred = 0) or per-thread
 * unreduced 512-bit sums of products reduced once per block of products (deferred = 1) -- equal canonical values
 * (Accumulator contract, crates/jolt-field/src/algebra.rs:362-433). */
int32_t jolt_table_dot(jolt_ctx *ctx, const jolt_table *a, const jolt_table *b, int32_t deferred, jolt_fr_t *out);

/* One-hot (Twist/Shout) selector columns as per-cycle hot indices.  Replaces ChunkIndexSource /
 * LazyFoldedRa (crates/jolt-kernels/src/optimized/lazy_ra.rs:39-268) and the pushforward G tables of the booleanity address
 * phase (optimized/booleanity.rs:24-31).  indices[p*cycles + j] in [0, k) or 0xFF on a cold cycle; k <= 255 (jolt_onehot_upload16 beyond). */
typedef struct jolt_onehot jolt_onehot;
int32_t jolt_onehot_upload(jolt_ctx *ctx, const uint8_t *indices, size_t n_polys, size_t cycles, uint32_t k, jolt_onehot **out);
/* The same with 16-bit indices (0xFFFF on a cold cycle, k <= 1024): the K = 256 chunks of long traces (log_k_chunk = 8 at log T >= 25,
 * crates/jolt-prover/src/config.rs:175-186), where index 255 is a valid address.  Every operator below accepts either width; the
 * LDS-staged and pair-table kernels of the lazily bound members are K <= 16 specialisations and are simply not selected. */
int32_t jolt_onehot_upload16(jolt_ctx *ctx, const uint16_t *indices, size_t n_polys, size_t cycles, uint32_t k, jolt_onehot **out);
int32_t jolt_onehot_download16(jolt_ctx *ctx, const jolt_onehot *source, uint16_t *out /* n_polys * cycles */);
int32_t jolt_onehot_free(jolt_ctx *ctx, jolt_onehot *source);
/* dense address-folded column: out[j] = scale_table[index(poly, j)], zero on cold cycles (the N x T "direct shape") */
int32_t jolt_onehot_materialize(jolt_ctx *ctx, const jolt_onehot *source, size_t poly, const jolt_table *scale_table, jolt_table **out);
/* out[p*k + a] = sum_j weights[j] * [index(p, j) == a]   (G_p = pushforward of the cycle weights to the address domain) */
int32_t jolt_onehot_pushforward(jolt_ctx *ctx, const jolt_onehot *source, const jolt_table *weights, jolt_table **out);
/* Member eq(w,j) * sum_v coeffs[v] * prod_{i<F} ra_{vF+i}(j), ra_p(j) = scale_tables[p*k + index(p,j)] (host array n_polys*k), with
 * the selector columns bound lazily: rounds 0..3 gather through the indices, the fourth bind materialises cycles/16-entry tables
 * (LazyFoldedRa::bind).  Round sums, binds and final values are those of jolt_member_create_split_eq_uniform over the
 * materialised columns, bit for bit.  n = log2(cycles) >= 4.  The source must outlive the member. */
int32_t jolt_member_create_lazy_ra_uniform(jolt_ctx *ctx, const jolt_onehot *source, const jolt_fr_t *scale_tables, uint32_t V, uint32_t F,
                                           const jolt_fr_t *coeffs, const jolt_fr_t *w, size_t n, const jolt_fr_t *scale, jolt_member **out);

/* One shard of a hypercube-sharded batch: the source holds this rank's block of cycles, w its n local coordinates, shard_scale =
 * eq(w_hi, rank) (as jolt_member_create_split_eq_product_sharded).  After the fourth bind the tables (what
 * jolt_round_group_pack_tables hands over) carry coeffs[v] folded into the first factor of product v. */
int32_t jolt_member_create_lazy_ra_uniform_sharded(jolt_ctx *ctx, const jolt_onehot *source, const jolt_fr_t *scale_tables, uint32_t V, uint32_t F,
                                                   const jolt_fr_t *coeffs, const jolt_fr_t *w, size_t n, const jolt_fr_t *scale,
                                                   const jolt_fr_t *shard_scale, jolt_member **out);
/* Packed typed witness rows: ONE upload of the per-cycle records the committed columns derive from
 * (CommittedColumnsWitness, crates/jolt-kernels/src/commitment.rs:25-32; InstructionCycleRow) instead of a materialised field
 * column per polynomial; columns are expanded on the device.  Fields are little-endian integers inside a row of row_bytes bytes. */
typedef struct jolt_rows jolt_rows;
int32_t jolt_rows_upload(jolt_ctx *ctx, const void *rows, size_t n_rows, size_t row_bytes, jolt_rows **out);
/* The same copy in flight beside the context's kernels: the NEXT proof's rows moving over the link while the current proof runs (the witness is produced by the tracer
 * ahead of the prover, crates/jolt-witness/src/consumer.rs:129-143).  `rows` must be page-locked (jolt_host_pinned_alloc) and unchanged until _wait returned; _begin
 * returns at once, _wait blocks the host until the copy has landed (begun a proof earlier, it has); the handle then behaves like jolt_rows_upload's. */
int32_t jolt_rows_upload_begin(jolt_ctx *ctx, const void *rows, size_t n_rows, size_t row_bytes, jolt_rows **out);
int32_t jolt_rows_upload_wait(jolt_ctx *ctx, jolt_rows *rows);
/* Page-locked host memory for the row buffer the tracer fills (the Vec<CycleRow> of crates/jolt-host/src/program.rs's trace output, packed): jolt_rows_upload
 * from such a block runs at the link rate (no staging copy by the runtime).  Ordinary host memory in every other respect. */
int32_t jolt_host_pinned_alloc(jolt_ctx *ctx, size_t bytes, void **out);
int32_t jolt_host_pinned_free(jolt_ctx *ctx, void *p);
int32_t jolt_rows_free(jolt_ctx *ctx, jolt_rows *rows);
/* integer field (width 1/2/4/8 bytes at `offset`, optionally two's complement) -> Fr table (Polynomial::bind_to_field promotion) */
int32_t jolt_table_from_rows(jolt_ctx *ctx, const jolt_rows *rows, size_t offset, uint32_t width, int32_t is_signed, jolt_table **out);
/* the same field as a resident integer column (JOLT_INT_U64, or JOLT_INT_I64 sign-extended): the compact scalars of Polynomial<T> (crates/jolt-poly/src/dense.rs:
 * 129-142) straight from the uploaded rows -- what jolt_member_create_lc_small and the *_small operators read; freed with jolt_ints_free */
int32_t jolt_ints_from_rows(jolt_ctx *ctx, const jolt_rows *rows, size_t offset, uint32_t width, int32_t is_signed, jolt_ints **out);
/* ... and n_fields fields in ONE pass over the rows (a workgroup stages whole rows in LDS, every field is written from there): out[k] = field k.  The witness hand-over
 * of a proof extracts every typed column of WitnessBundle::from_row (crates/jolt-kernels/src/optimized/rows.rs:22-72) -- field by field the rows were read once per field. */
int32_t jolt_ints_from_rows_many(jolt_ctx *ctx, const jolt_rows *rows, const size_t *offsets, const uint32_t *widths, const int32_t *is_signed, size_t n_fields,
                                 jolt_ints **out);
/* n_polys hot-index columns from ONE address field (<= 16 bytes): index_i = (field >> shifts[i]) & (2^log_k - 1)
 * (RaChunkSelector::chunk_u128, crates/jolt-witness/src/witnesses/one_hot.rs:14-52); a row whose byte at valid_offset is 0 is a
 * cold cycle (Option::None, e.g. no RAM access); valid_offset = SIZE_MAX: every row is hot.  log_k <= 8 (log_k = 8 gives a 16-bit source). */
int32_t jolt_onehot_from_rows(jolt_ctx *ctx, const jolt_rows *rows, size_t offset, uint32_t width, const uint32_t *shifts, size_t n_polys,
                              uint32_t log_k, size_t valid_offset, jolt_onehot **out);
int32_t jolt_onehot_download(jolt_ctx *ctx, const jolt_onehot *source, uint8_t *out /* n_polys * cycles */);
/* The extractors' one-row lookahead window over a physical trace shorter than the padded cycle domain (RandomAccessRows::window /
 * WitnessBundle::from_row(current, next, env), crates/jolt-kernels/src/optimized/rows.rs:22-72): out[j], j < cycles, reads the field of
 * row j (lookahead = 0) or row j + 1 (lookahead = 1); rows at or beyond n_rows are padding rows (the field of TraceRow::default():
 * padding_value), and the last cycle has no next row (none_value).  n_rows > cycles is JOLT_ERR_SIZE_MISMATCH (rows.rs:44-53). */
int32_t jolt_table_from_rows_window(jolt_ctx *ctx, const jolt_rows *rows, size_t offset, uint32_t width, int32_t is_signed, int32_t lookahead,
                                    size_t cycles, int64_t padding_value, int64_t none_value, jolt_table **out);
/* Hot-index columns from a sentinel-packed address field (InstructionCycleRow::{pc_plus_one, ram_address_plus_one},
 * crates/jolt-kernels/src/optimized/instruction_read_raf.rs:82-123): 0 = no access (cold cycle), v > 0 = address v - 1 whose chunks
 * index_i = ((v - 1) >> shifts[i]) & (2^log_k - 1) become the columns; cycles beyond the physical rows are cold. */
int32_t jolt_onehot_from_rows_sentinel(jolt_ctx *ctx, const jolt_rows *rows, size_t offset, uint32_t width, const uint32_t *shifts, size_t n_polys,
                                       uint32_t log_k, size_t cycles, jolt_onehot **out);

/* Booleanity cycle phase over the same lazily bound columns (crates/jolt-kernels/src/optimized/booleanity.rs:436-633):
 * eq(w,j) * sum_i (H_i(j)^2 - rho[i]*H_i(j)), H_i(j) = scale_tables[i*k + index(i,j)] (the caller passes the gamma^i-pre-scaled
 * address tables and rho[i] = gamma^i).  prove_round returns (q(0), q(inf)) of the inner quadratic; the cubic is
 * gruen_poly_deg_3 on the host.  final_values: the bound H_i (the host divides by rho[i], booleanity.rs:652-657) + the eq scalar. */
int32_t jolt_member_create_lazy_booleanity(jolt_ctx *ctx, const jolt_onehot *source, const jolt_fr_t *scale_tables, const jolt_fr_t *rho,
                                           const jolt_fr_t *w, size_t n, const jolt_fr_t *scale, jolt_member **out);

/* Dory tier-1 (G1) streaming row commitments -- SURVEY.md section 8(f) row 2.  Replaces the MSM work of
 * DoryScheme::{feed_u64, feed_i128, feed_i128_rows_with} (crates/jolt-dory/src/streaming.rs:115-205: one ark msm_u64 / msm_i128
 * per row_width window over the first row_width G1 bases) and of process_one_hot_chunk(s_with) -> one_hot_chunk_commitments
 * (:230-275, :366-419: per chunk, commitment[k] = sum of the bases of the columns whose hot row is k).  The tier-2 pairing
 * product stays with the caller.  Integers are little-endian machine integers (i128 = two u64, low first, two's complement). */
enum { JOLT_INT_U64 = 0, JOLT_INT_I64 = 1, JOLT_INT_I128 = 2 };
int32_t jolt_ints_upload(jolt_ctx *ctx, const void *host, int32_t kind, size_t count, jolt_ints **out);
int32_t jolt_ints_free(jolt_ctx *ctx, jolt_ints *values);
/* out[r] = sum_j values[r*row_width + j] * srs[j] for the count / row_width rows, in row order.  row_width must be a power of
 * two (JOLT_ERR_INVALID_ARG, streaming.rs:99-102), <= the SRS length (JOLT_ERR_SRS_TOO_SMALL, :103-108) and divide count
 * (JOLT_ERR_SIZE_MISMATCH, :192-195). */
int32_t jolt_dory_commit_rows(jolt_ctx *ctx, const jolt_srs *srs, const jolt_ints *values, size_t row_width, jolt_g1_t *out);
/* out[chunk*k + row] for the cycles / chunk_width chunks of hot-index column `poly`; an empty row gives the identity
 * (Bn254G1::default(), streaming.rs:409-418).  Same argument checks as above (:376-392).
 * As an OpeningHint: finish_one_hot_column_major_chunks (streaming.rs:318-362) transposes the chunks, hint[row*chunks + chunk] =
 * out[chunk*k + row]; with chunk_width = 2^sigma that is row (k << (log_t - sigma)) + chunk of the cycle-major grid matrix of 2^sigma
 * columns -- the row order jolt_dory_fold_rows_grid's `left` and jolt_dory_combine_hints use.  A dense column's hint is
 * jolt_dory_commit_rows with row_width = 2^sigma: the first T / 2^sigma rows of that matrix (address 0). */
int32_t jolt_dory_commit_onehot(jolt_ctx *ctx, const jolt_srs *srs, const jolt_onehot *source, size_t poly, size_t chunk_width, jolt_g1_t *out);

/* The G1 and Fr work of a Dory opening ahead of the pairing rounds.  Cycle-major placement (TracePolynomialOrder::CycleMajor): grid
 * index k*T + j, dense columns at k = 0, as for the jolt_grid_* entry points below (the address-major twins are jolt_dory_*_am further down).  The tier-2 multi-pairing and the multi-pairings of the reduce-and-fold rounds of
 * dory::prove are jolt_dory_multi_pair / jolt_dory_multi_pair_g2_setup below, the rounds' group routines jolt_dory_g1_* / jolt_dory_g2_*; what stays on the host is
 * the transcript, the control flow and commit_blind (the verifier's GT scalings are jolt_dory_gt_multi_exp, further down).
 *
 * RlcSource::fold_rows over TraceOpeningPoly (optimized/opening.rs:491-510, multilinear.rs:452-462), cycle-major -- the
 * vector_matrix_product of dory::prove (crates/jolt-dory/src/scheme.rs:612-618), answered from the per-cycle columns without the K x T grid:
 *   out[c] = sum_p onehot_scalars[p] * sum_{j hot in p, ((hot_p(j) << log_t) | j) & (2^sigma - 1) == c} left[((hot_p(j) << log_t) | j) >> sigma]
 *          + sum_d dense_scalars[d]  * sum_{j & (2^sigma - 1) == c} left[j >> sigma] * dense[d][j]
 * Sources, scalars and dense columns as in jolt_grid_joint_polynomial; left has 2^(log_k + log_t - sigma) entries; out gets 2^sigma.
 * Every sigma in [0, log_k + log_t]; T must be a power of two.  JOLT_ERR_INVALID_ARG: sigma out of range, source->k > 2^log_k;
 * JOLT_ERR_SIZE_MISMATCH: left or a dense column of the wrong length, sources with different cycle counts; JOLT_ERR_UNSUPPORTED: more
 * than 4 sources or 8 dense columns, log_k > 8, or no column at all.  Temporary device memory is O(T), never O(K * T). */
int32_t jolt_dory_fold_rows_grid(jolt_ctx *ctx, const jolt_onehot *const *sources, size_t n_sources, const jolt_fr_t *onehot_scalars,
                                 jolt_table *const *dense, size_t n_dense, const jolt_fr_t *dense_scalars, uint32_t log_k, uint32_t sigma,
                                 const jolt_table *left, jolt_table **out);
/* DoryScheme::combine_hints (crates/jolt-dory/src/scheme.rs:325-360): out[row] = sum_i scalars[i] * hints[i][row] for row < max_i hint_rows[i];
 * a hint shorter than the widest contributes the identity to the rows it lacks (:330-338).  Host pointers in and out, like the commit entry points that produced the hints.
 * n_hints == 0 is JOLT_ERR_INVALID_ARG (the reference asserts).  The hint's commit_blind, a dot product of n_hints field elements, stays with the caller. */
int32_t jolt_dory_combine_hints(jolt_ctx *ctx, const jolt_g1_t *const *hints, const size_t *hint_rows, size_t n_hints, const jolt_fr_t *scalars,
                                jolt_g1_t *out /* max_i hint_rows[i] */);
/* One row of jolt_dory_combine_hints on the host, out = sum_i scalars[i] * points[i] (scheme.rs:339-356), through the code the device rows run: shared signed-digit
 * plan, per-window walk by descending digit, Horner recombination.  For the CPU suite. */
int32_t jolt_host_dory_combine_row(const jolt_g1_t *points, const jolt_fr_t *scalars, size_t n, jolt_g1_t *out);

/* The group and field routines of dory::prove's reduce-and-fold rounds: dory's DoryRoutines seam as the reference implements it for both groups,
 * JoltG1Routines (crates/jolt-dory/src/routines.rs:60-97) and JoltG2Routines (:101-147).  Host pointers in and out, like jolt_dory_combine_hints: the trait works
 * on host slices and the pairings need the vectors on the host every round.  `vs` / `left` are updated in place.  Results are the reference's group elements; the
 * Jacobian representative is free, the identity comes back as (1, 1, 0).  The rounds' multi-pairings are jolt_dory_multi_pair below; the control flow of
 * dory::prove stays with the caller (GT scalings, which only a verifier needs, are jolt_dory_gt_multi_exp).
 * Every entry refuses with JOLT_ERR_INVALID_ARG: a null pointer with n > 0, a scalar that is not canonical, a point whose coordinates are not canonical or that
 * is not on its curve.  For G2 that is the twist equation ONLY -- there is NO subgroup check (the twist has cofactor 2q - r); the routines are group-law
 * identities on the whole twist, so a point outside the order-r subgroup gets the answer the same formulas give on the CPU.  A refused call enqueues nothing,
 * writes nothing and leaves the context usable.  n = 0 succeeds and writes nothing (the MSM writes the empty sum, the identity).  n <= 2^30. */
/* DoryRoutines::msm (routines.rs:62-64, :103-105): out = sum_i scalars[i] * bases[i], bases projective */
int32_t jolt_dory_g1_msm(jolt_ctx *ctx, const jolt_g1_t *bases, const jolt_fr_t *scalars, size_t n, jolt_g1_t *out);
/* DoryRoutines::fixed_base_vector_scalar_mul (routines.rs:66-72, :107-122): out[i] = scalars[i] * base; an empty input gives an empty output */
int32_t jolt_dory_g1_fixed_base_mul(jolt_ctx *ctx, const jolt_g1_t *base, const jolt_fr_t *scalars, size_t n, jolt_g1_t *out);
/* DoryRoutines::fixed_scalar_mul_bases_then_add (routines.rs:74-82, :124-132): vs[i] = vs[i] + scalar * bases[i] */
int32_t jolt_dory_g1_scale_bases_add(jolt_ctx *ctx, const jolt_g1_t *bases, jolt_g1_t *vs, size_t n, const jolt_fr_t *scalar);
/* DoryRoutines::fixed_scalar_mul_vs_then_add (routines.rs:84-92, :134-142): vs[i] = scalar * vs[i] + addends[i] */
int32_t jolt_dory_g1_scale_vs_add(jolt_ctx *ctx, jolt_g1_t *vs, const jolt_g1_t *addends, size_t n, const jolt_fr_t *scalar);
int32_t jolt_dory_g2_msm(jolt_ctx *ctx, const jolt_g2_t *bases, const jolt_fr_t *scalars, size_t n, jolt_g2_t *out);
int32_t jolt_dory_g2_fixed_base_mul(jolt_ctx *ctx, const jolt_g2_t *base, const jolt_fr_t *scalars, size_t n, jolt_g2_t *out);
int32_t jolt_dory_g2_scale_bases_add(jolt_ctx *ctx, const jolt_g2_t *bases, jolt_g2_t *vs, size_t n, const jolt_fr_t *scalar);
int32_t jolt_dory_g2_scale_vs_add(jolt_ctx *ctx, jolt_g2_t *vs, const jolt_g2_t *addends, size_t n, const jolt_fr_t *scalar);
/* DoryRoutines::fold_field_vectors (routines.rs:94-96, :144-146; jolt_dory_routines.rs:10-18): left[i] = left[i] * scalar + right[i] in Fr, the same function for
 * both groups; every entry of left and right must be canonical too */
int32_t jolt_dory_fold_field_vectors(jolt_ctx *ctx, jolt_fr_t *left, const jolt_fr_t *right, size_t n, const jolt_fr_t *scalar);
/* Measurement aid of tools/bench_dory_routines.py: out_ms (may be NULL) receives the wall milliseconds of the phases of the last routine call made while timing was
 * on -- argument checks, host -> device, kernels, device -> host -- then timing is switched on or off.  While on, a call drains the stream between its phases. */
int32_t jolt_dory_routines_timing(jolt_ctx *ctx, int32_t enable, double *out_ms /* 4 */);
/* Fq2 and G2 on the host, as the kernels compute them (fq2.hip.h, g2.hip.h), for the CPU suite.  jolt_host_fq2_op refuses an operand that is not canonical
 * (b is ignored for SQR and NEG and may be NULL); the G2 functions take any coordinates, jolt_host_g2_is_on_curve is the check the entry points above apply. */
enum { JOLT_FQ2_ADD = 0, JOLT_FQ2_SUB = 1, JOLT_FQ2_MUL = 2, JOLT_FQ2_SQR = 3, JOLT_FQ2_NEG = 4 };
int32_t jolt_host_fq2_op(int32_t op, const jolt_fq2_t *a, const jolt_fq2_t *b, jolt_fq2_t *out);
int32_t jolt_host_g2_add(const jolt_g2_t *p, const jolt_g2_t *q, jolt_g2_t *out);
int32_t jolt_host_g2_double(const jolt_g2_t *p, jolt_g2_t *out);
int32_t jolt_host_g2_neg(const jolt_g2_t *p, jolt_g2_t *out);
int32_t jolt_host_g2_eq(const jolt_g2_t *p, const jolt_g2_t *q, int32_t *equal);
int32_t jolt_host_g2_is_on_curve(const jolt_g2_t *p, int32_t *on_curve);
int32_t jolt_host_g2_scalar_mul(const jolt_g2_t *p, const jolt_fr_t *scalar, jolt_g2_t *out); /* plain MSB-first double-and-add */
/* One element of the routines through the code the device lanes run: out = addend + scalar * scaled (both shared-scalar routines: the non-adjacent form of the
 * scalar and its walk), out = scalar * base (the fixed-base table and window walk), out = scalar * base (one MSM term).  Same refusals as the device entries. */
int32_t jolt_host_dory_g1_scale_add_one(const jolt_g1_t *scaled, const jolt_g1_t *addend, const jolt_fr_t *scalar, jolt_g1_t *out);
int32_t jolt_host_dory_g2_scale_add_one(const jolt_g2_t *scaled, const jolt_g2_t *addend, const jolt_fr_t *scalar, jolt_g2_t *out);
int32_t jolt_host_dory_g1_fixed_base_one(const jolt_g1_t *base, const jolt_fr_t *scalar, jolt_g1_t *out);
int32_t jolt_host_dory_g2_fixed_base_one(const jolt_g2_t *base, const jolt_fr_t *scalar, jolt_g2_t *out);
int32_t jolt_host_dory_g1_msm_term(const jolt_g1_t *base, const jolt_fr_t *scalar, jolt_g1_t *out);
int32_t jolt_host_dory_g2_msm_term(const jolt_g2_t *base, const jolt_fr_t *scalar, jolt_g2_t *out);

/* Dory's multi-pairings: the BN254 optimal ate pairing (pairing.hip.h), one Miller loop per pair on the device, their product by a halving tree, the final
 * exponentiation on the host.  jolt_gt_t == ark_bn254::Fq12 (Bn254GT, crates/jolt-crypto/src/ec/bn254/gt.rs:30-32): twelve Montgomery Fq in the order c0.c0.c0,
 * c0.c0.c1, c0.c1.c0, ..., c1.c2.c1; the Fq2 coefficient c_h.c_j multiplies w^(2 j + h), w^6 = 9 + u.  The final exponent is (p^12 - 1) / r * 2 z (6 z^2 + 3 z + 1),
 * the power ark-ec's BN model is recalled to compute: a convention that no reference vector pins (docs/parity.md).  Host pointers in and out, like the routines
 * above, and their refusals: JOLT_ERR_INVALID_ARG for a null pointer with n > 0, coordinates that are not canonical, a point off its curve; NO subgroup check,
 * as in arkworks (a G2 point outside the order-r subgroup traps nothing and gives an unspecified value).  A refused call enqueues nothing and writes nothing.
 * A pair with the identity on either side contributes one; n = 0 gives one.  n <= 2^20 (JOLT_ERR_UNSUPPORTED above: the line table takes 16.5 KiB per pair). */
typedef struct { jolt_fq_t c[12]; } jolt_gt_t;
typedef struct jolt_g2_prepared jolt_g2_prepared;
#define JOLT_PAIRING_LINES 88 /* lines of one prepared G2 point: 65 doublings and 21 additions of 6z + 2 in non-adjacent form, the two Frobenius steps */
/* PairingGroup::multi_pairing (crates/jolt-crypto/src/ec/bn254/mod.rs:274-284), dory's multi_pair in every round of dory::prove: out = prod_i e(g1s[i], g2s[i]) */
int32_t jolt_dory_multi_pair(jolt_ctx *ctx, const jolt_g1_t *g1s, const jolt_g2_t *g2s, size_t n, jolt_gt_t *out);
/* The same product BEFORE the final exponentiation: what the device computes, bit for bit what jolt_host_miller_loop gives (field arithmetic is exact) */
int32_t jolt_dory_multi_miller(jolt_ctx *ctx, const jolt_g1_t *g1s, const jolt_g2_t *g2s, size_t n, jolt_gt_t *out);
/* The line tables of n G2 points, resident on the device, step-major: built once per setup for the g2_vec bases (the G2 Miller preprocessing scheme.rs:147-153
 * remarks on).  Freed with jolt_g2_prepared_free; n = 0 gives an empty table. */
int32_t jolt_dory_g2_prepare(jolt_ctx *ctx, const jolt_g2_t *g2s, size_t n, jolt_g2_prepared **out);
int32_t jolt_g2_prepared_free(jolt_ctx *ctx, jolt_g2_prepared *prepared);
/* dory's multi_pair_g2_setup over srs_prefix (crates/jolt-dory/src/scheme.rs:543-552), the tier-2 commitment: out = prod_{i < n} e(g1s[i], prepared point i).
 * n beyond the prepared length is JOLT_ERR_INVALID_ARG. */
int32_t jolt_dory_multi_pair_g2_setup(jolt_ctx *ctx, const jolt_g1_t *g1s, const jolt_g2_prepared *prepared, size_t n, jolt_gt_t *out);
/* Measurement aid of tools/bench_dory_pairing.py, as jolt_dory_routines_timing: the wall milliseconds of the phases of the last multi-pairing or prepare call made
 * while timing was on -- argument checks, host -> device, prepare kernel, Miller kernel, product tree, device -> host, final exponentiation. */
int32_t jolt_dory_pairing_timing(jolt_ctx *ctx, int32_t enable, double *out_ms /* 7 */);
/* Fq12 and the pairing on the host through the code the kernels run (fq12.hip.h, pairing.hip.h), for the CPU suite.  jolt_host_fq12_op refuses operands that are
 * not canonical (JOLT_ERR_INVALID_ARG) and the inverse of zero (JOLT_ERR_NOT_INVERTIBLE); b is read by MUL and MUL_SPARSE only.  MUL_SPARSE multiplies through the
 * line routine (mul_by_034) and refuses a b that has a non-zero coefficient outside c0.c0, c1.c0, c1.c1. */
enum { JOLT_FQ12_MUL = 0, JOLT_FQ12_SQR = 1, JOLT_FQ12_INV = 2, JOLT_FQ12_CONJ = 3, JOLT_FQ12_FROBENIUS1 = 4, JOLT_FQ12_FROBENIUS2 = 5, JOLT_FQ12_FROBENIUS3 = 6,
       JOLT_FQ12_MUL_SPARSE = 7 };
int32_t jolt_host_fq12_op(int32_t op, const jolt_gt_t *a, const jolt_gt_t *b, jolt_gt_t *out);
/* The line table of one G2 point, lines[3 * step + {0, 1, 2}] = the coefficients (a, b, c) of a y_P + b x_P w + c w^3; *skip = 1 for the identity */
int32_t jolt_host_g2_prepare_one(const jolt_g2_t *g2, jolt_fq2_t *lines /* 3 * JOLT_PAIRING_LINES */, int32_t *skip);
/* prod_i of the Miller values of the pairs, before the final exponentiation */
int32_t jolt_host_miller_loop(const jolt_g1_t *g1s, const jolt_g2_t *g2s, size_t n, jolt_gt_t *out);
/* f^((p^12 - 1) / r * 2 z (6 z^2 + 3 z + 1)); zero is JOLT_ERR_NOT_INVERTIBLE */
int32_t jolt_host_final_exponentiation(const jolt_gt_t *f, jolt_gt_t *out);
/* gt^scalar by square-and-multiply over the canonical scalar: the host form of jolt_dory_gt_pow_many's powers (any canonical Fq12 is a valid base) */
int32_t jolt_host_gt_pow(const jolt_gt_t *gt, const jolt_fr_t *scalar, jolt_gt_t *out);

/* Dory's reduce-and-fold rounds on vectors that stay on the device.  A jolt_dory_vec is a device array of G1 points, G2 points or Fr elements from the context's
 * pool; the routines and multi-pairings above take host pointers, so a round through them uploads, runs alone, synchronises and downloads once per product.  Here
 * the argument checks of those entry points -- canonical coordinates, the curve or twist equation (no subgroup check), canonical scalars -- run ONCE, in
 * jolt_dory_vec_upload; nothing below re-checks a resident vector.  A view is (vector, first, n) with first <= len and n <= len - first.  Every entry refuses with
 * JOLT_ERR_INVALID_ARG: a null handle, a vector of another context or of the wrong kind, a view outside its vector; a refused call enqueues nothing and writes
 * nothing.  Resident operations and product batches take effect in call order on a context. */
typedef struct jolt_dory_vec jolt_dory_vec;
enum { JOLT_DORY_KIND_G1 = 0, JOLT_DORY_KIND_G2 = 1, JOLT_DORY_KIND_FR = 2 };
/* host: n elements of jolt_g1_t / jolt_g2_t / jolt_fr_t by kind; n = 0 gives an empty vector; n <= 2^30 */
int32_t jolt_dory_vec_upload(jolt_ctx *ctx, int32_t kind, const void *host, size_t n, jolt_dory_vec **out);
int32_t jolt_dory_vec_download(jolt_ctx *ctx, const jolt_dory_vec *vec, size_t first, size_t n, void *host);
int32_t jolt_dory_vec_len(const jolt_dory_vec *vec, size_t *len);
int32_t jolt_dory_vec_kind(const jolt_dory_vec *vec, int32_t *kind);
int32_t jolt_dory_vec_free(jolt_ctx *ctx, jolt_dory_vec *vec);
/* the vector becomes its first n elements (after a fold, its first half); n > len is refused */
int32_t jolt_dory_vec_truncate(jolt_dory_vec *vec, size_t n);
/* jolt_dory_g2_prepare from elements [first, first + n) of a resident G2 vector, with no host round trip: once per setup for the g2_vec bases -- a prefix of the
 * table serves every later round (jolt_dory_item.prepared_first) */
int32_t jolt_dory_g2_prepare_vec(jolt_ctx *ctx, const jolt_dory_vec *vec, size_t first, size_t n, jolt_g2_prepared **out);
/* The shared-scalar routines and the field fold in place on views, enqueued on the context's stream (no synchronisation): the per-element functions of
 * jolt_dory_g{1,2}_scale_bases_add, _scale_vs_add and jolt_dory_fold_field_vectors.  Both vectors of a call have the same kind (G1 or G2; Fr for the fold).  The
 * two views may lie in one vector if their ranges are disjoint -- the fold v <- alpha v_L + v_R; overlapping ranges are refused. */
/* vs[vs_first + i] += scalar * bases[bases_first + i] */
int32_t jolt_dory_vec_scale_bases_add(jolt_ctx *ctx, const jolt_dory_vec *bases, size_t bases_first, jolt_dory_vec *vs, size_t vs_first, size_t n, const jolt_fr_t *scalar);
/* vs[vs_first + i] = scalar * vs[vs_first + i] + addends[addends_first + i] */
int32_t jolt_dory_vec_scale_vs_add(jolt_ctx *ctx, jolt_dory_vec *vs, size_t vs_first, const jolt_dory_vec *addends, size_t addends_first, size_t n, const jolt_fr_t *scalar);
/* left[left_first + i] = left[left_first + i] * scalar + right[right_first + i] */
int32_t jolt_dory_vec_fold_field(jolt_ctx *ctx, jolt_dory_vec *left, size_t left_first, const jolt_dory_vec *right, size_t right_first, size_t n, const jolt_fr_t *scalar);
/* The state an opening's rounds start from, built on the device.  Same contract as the entries above: a null handle, a vector (or table) of another context or of
 * the wrong kind, a view or range outside its vector (or table), or a scalar that is not canonical is JOLT_ERR_INVALID_ARG, and a refused call enqueues nothing and
 * writes nothing.  The first two are enqueued on the context's stream like the in-place routines (no synchronisation); the last two stage a plan or a table of this
 * call from host memory and synchronise before they return. */
/* n neutral elements: the identity (1, 1, 0) for G1 / G2, zero for Fr; n = 0 gives an empty vector; n <= 2^30 */
int32_t jolt_dory_state_alloc(jolt_ctx *ctx, int32_t kind, size_t n, jolt_dory_vec **out);
/* dst[dst_first + i] = table[table_first + i] for i < n: entries of a device Fr table (jolt_dory_fold_rows_grid's output, an eq table) into an Fr vector view.
 * Both hold Montgomery words, so this is a device copy. */
int32_t jolt_dory_state_from_table(jolt_ctx *ctx, const jolt_table *table, size_t table_first, jolt_dory_vec *dst, size_t dst_first, size_t n);
/* DoryScheme::combine_hints (crates/jolt-dory/src/scheme.rs:325-360) as jolt_dory_combine_hints computes it, with resident G1 views in and a resident view out:
 *   out[out_first + row] = sum_i scalars[i] * hints[i][hint_first[i] + row]   for row < max_i hint_rows[i],
 * a hint shorter than the widest contributing the identity to the rows it lacks (:330-338).  The same digit plan and the same two kernels: the rows are the
 * group elements the host-pointer entry gives.  n_hints == 0 is JOLT_ERR_INVALID_ARG (the reference asserts), as is an `out` range that shares an element with a hint. */
int32_t jolt_dory_state_combine_hints(jolt_ctx *ctx, const jolt_dory_vec *const *hints, const size_t *hint_first, const size_t *hint_rows, size_t n_hints,
                                    const jolt_fr_t *scalars, jolt_dory_vec *out, size_t out_first);
/* DoryRoutines::fixed_base_vector_scalar_mul (crates/jolt-dory/src/routines.rs:66-72, :107-122) on resident views: out[out_first + i] = scalars[scalars_first + i] * base.
 * kind is JOLT_DORY_KIND_G1 or _G2 and names the group of `base` (one host jolt_g1_t / jolt_g2_t, checked as jolt_dory_g{1,2}_fixed_base_mul check it) and of `out`;
 * `scalars` is an Fr vector.  The elements come back as that entry's: the identity as (1, 1, 0). */
int32_t jolt_dory_state_fixed_base_mul(jolt_ctx *ctx, int32_t kind, const void *base, const jolt_dory_vec *scalars, size_t scalars_first, jolt_dory_vec *out,
                                     size_t out_first, size_t n);
/* A batch of inner products over resident views, one launch set for all of them: per item
 *   JOLT_DORY_PAIR    prod_i e(a[a_first + i], b[b_first + i]); a is a G1 vector, b a G2 vector -- or NULL, and the G2 side is points
 *                     [prepared_first, prepared_first + n) of `prepared`
 *   JOLT_DORY_MSM_G1  sum_i b[b_first + i] * a[a_first + i]; a is a G1 vector, b an Fr vector (`prepared` is NULL)
 *   JOLT_DORY_MSM_G2  the same with a G2 vector
 * The pairing chain (one prepare launch over the distinct G2 views, one Miller launch over all pairs, one product level per launch over all items' segments), the
 * G1 chain and the G2 chain (one term launch, one addition level per launch) run on three streams beside each other; one read-back, one synchronisation, then one
 * final exponentiation per PAIR item on up to 16 host threads.  outs[k] holds item k's result in its leading words: a jolt_gt_t (48 words, the canonical value,
 * bit for bit jolt_dory_multi_pair's), a jolt_g1_t (12) or a jolt_g2_t (24), normalised as jolt_dory_g{1,2}_msm normalises; the rest of outs[k] is not written.
 * An empty item gives one, or the identity (1, 1, 0).  The sum of the item lengths is at most 2^24 per chain (JOLT_ERR_UNSUPPORTED above). */
enum { JOLT_DORY_PAIR = 0, JOLT_DORY_MSM_G1 = 1, JOLT_DORY_MSM_G2 = 2 };
typedef struct {
    int32_t op;
    const jolt_dory_vec *a;
    size_t a_first;
    const jolt_dory_vec *b;
    size_t b_first;
    const jolt_g2_prepared *prepared;
    size_t prepared_first;
    size_t n;
} jolt_dory_item;
typedef struct { uint64_t w[48]; } jolt_dory_result;
int32_t jolt_dory_products(jolt_ctx *ctx, const jolt_dory_item *items, size_t n_items, jolt_dory_result *outs);
/* The launch plan of one chain of a batch, for the CPU suite: item k of length lens[k] is padded to whole wavefronts of 64 lanes, so a workgroup belongs to one
 * item; item_base[k] = the item's first slot in the chain's packed array (the padded lengths before it); workgroup w works on slots item_base[wg_item[w]] +
 * wg_first[w] + lane; *levels = ceil(log2) of the longest item, the launches of the segmented reduction.  wg_item / wg_first hold wg_cap entries and may be NULL
 * with wg_cap = 0 to ask for *n_wgs alone; more workgroups than wg_cap is JOLT_ERR_SIZE_MISMATCH, a padded total above 2^24 JOLT_ERR_UNSUPPORTED. */
int32_t jolt_host_dory_batch_plan(const size_t *lens, size_t n_items, size_t wg_cap, uint32_t *wg_item, uint32_t *wg_first, size_t *item_base, size_t *n_wgs, uint32_t *levels);

/* The witness commitment in front of an opening: the row commitments of jolt_dory_commit_onehot / jolt_dory_commit_rows written on the device, in OpeningHint order,
 * into views of resident G1 vectors (jolt_dory_state_alloc), where jolt_dory_state_combine_hints and jolt_dory_products (one PAIR item per column against Gamma2's
 * prepared table: the tier-2 commitments of a whole witness in one batch) read them.  Nothing crosses the link.  Every point is written normalised, (x / z^2, y / z^3, 1),
 * by one batched inversion; the identity is (1, 1, 0).  The ABI leaves the Jacobian representative free, so this is a promise of these two entries alone.
 * Contract of the resident entries above: a null handle, an `out` of another context or not of kind G1, or a view that does not hold the result is
 * JOLT_ERR_INVALID_ARG; the shape checks keep the codes of the host-pointer entries (power-of-two width, JOLT_ERR_SRS_TOO_SMALL, JOLT_ERR_SIZE_MISMATCH); a refused call
 * enqueues nothing and writes nothing.  Both are enqueued on the context's stream; jolt_dory_hints_rows synchronises once for the bit-length probe of its column. */
/* out[out_first + p*K*chunks + row*chunks + chunk] for columns [first_poly, first_poly + n_polys) of `source`, K = source->k, chunks = cycles / chunk_width:
 * the OpeningHint order of jolt_dory_commit_onehot's comment.  batch_points = 0: the default 2^26 keys per launch set; otherwise the cap (a whole number of
 * chunks, >= chunk_width), for the tests. */
int32_t jolt_dory_hints_onehot(jolt_ctx *ctx, const jolt_srs *srs, const jolt_onehot *source, size_t first_poly, size_t n_polys, size_t chunk_width,
                               jolt_dory_vec *out, size_t out_first, size_t batch_points);
/* out[out_first + r] = row commitment r of jolt_dory_commit_rows, normalised */
int32_t jolt_dory_hints_rows(jolt_ctx *ctx, const jolt_srs *srs, const jolt_ints *values, size_t row_width, jolt_dory_vec *out, size_t out_first);
/* The per-lane routine of the kernel behind both, on the host for the CPU suite: out[i] = points[i] normalised, the inversions batched by Montgomery's trick over runs
 * of `run` consecutive points (one inversion per run; a point with z = 0 enters the running product as one and comes back as (1, 1, 0)).  The points are not checked.
 * run = 0 or a null pointer with n > 0 is JOLT_ERR_INVALID_ARG. */
int32_t jolt_host_dory_g1_normalise(const jolt_g1_t *points, size_t n, size_t run, jolt_g1_t *out);
/* The kernel's index map for the one-hot columns, on the host: element e of a launch set that starts at window window0 (window = column * chunks + chunk) reads
 * workspace bucket *src = (e / k) * (k + 1) + e % k + 1 and is element *dst of the destination view */
int32_t jolt_host_dory_hint_map(uint32_t k, size_t chunks, size_t window0, size_t e, size_t *src, size_t *dst);

/* The same witness commitment and row fold in the ADDRESS-MAJOR trace placement.  The reference's prover proves in either layout
 * (crates/jolt-prover/src/dory/prover.rs:104-110; TracePolynomialOrder::{CycleMajor, AddressMajor}, crates/jolt-claims/src/protocols/jolt/geometry/dimensions.rs:20-59)
 * and places both with one formula (TracePlacement, crates/jolt-kernels/src/optimized/opening.rs:340-373): the coefficient of (cycle t, address k) sits at grid index
 *   (t << log_block) + (k << log_stride),   log_block = log2 CommitmentGrid::cycle_stride() = log_k + e,  log_stride = log2 CommitmentGrid::one_hot_stride() = e,
 * e >= 0 the embedding extra of a widened grid (0 otherwise: index = cycle * K + address, address_cycle_to_index); dense columns at k = 0; with 2^sigma matrix
 * columns row = index >> sigma, col = index & (2^sigma - 1).  For sigma >= log_block a row holds C = 2^(sigma - log_block) whole cycles, row r = the cycles
 * [r C, (r + 1) C), and EVERY column, one-hot or dense, has cycles / C rows: hint[r] by matrix row is the only hint order there is.
 * Contract of the resident entries above (views validated, null handles and foreign or non-G1 vectors JOLT_ERR_INVALID_ARG, a refused call enqueues nothing and writes
 * nothing), and for all three: sigma < log_block is JOLT_ERR_UNSUPPORTED (a cycle's block wider than a row; it does not occur for log_k <= 8 and T >= 2^9, where
 * sigma = ceil((log_k + log_t) / 2) >= log_k); log_stride > log_block, source->k > 2^(log_block - log_stride) and C not dividing the cycle count are
 * JOLT_ERR_INVALID_ARG; 2^sigma > the SRS length is JOLT_ERR_SRS_TOO_SMALL. */
/* out[out_first + p*rows + r] = sum_{j < C, hot_p(r C + j) not cold} srs[(j << log_block) + (hot_p(r C + j) << log_stride)] for the columns
 * [first_poly, first_poly + n_polys) of `source`, rows = cycles >> (sigma - log_block); normalised, the identity as (1, 1, 0), as jolt_dory_hints_onehot promises.
 * 8-bit and 16-bit sources.  Enqueued only. */
int32_t jolt_dory_hints_onehot_am(jolt_ctx *ctx, const jolt_srs *srs, const jolt_onehot *source, size_t first_poly, size_t n_polys,
                                  uint32_t sigma, uint32_t log_block, uint32_t log_stride, jolt_dory_vec *out, size_t out_first);
/* out[out_first + r] = sum_{j < C} values[r C + j] * srs[j << log_block], normalised: jolt_dory_hints_rows with row width C over the C strided bases, which are
 * gathered into a compact device array first (every integer kind; synchronises once for the bit-length probe, like jolt_dory_hints_rows). */
int32_t jolt_dory_hints_rows_am(jolt_ctx *ctx, const jolt_srs *srs, const jolt_ints *values, uint32_t sigma, uint32_t log_block,
                                jolt_dory_vec *out, size_t out_first);
/* RlcSource::fold_rows in the address-major placement, the limits and codes of jolt_dory_fold_rows_grid (log_k there = log_block - log_stride here):
 *   out[(j << log_block) + (k << log_stride)] = sum_p onehot_scalars[p] * sum_r [hot_p(r C + j) = k] * left[r]   (+ at k = 0: sum_d dense_scalars[d] * sum_r left[r] * dense_d[r C + j])
 * and zero at every other entry.  left has T >> (sigma - log_block) entries (JOLT_ERR_SIZE_MISMATCH otherwise), out gets 2^sigma.  Temporary device memory is
 * O(T + 2^sigma * T / (128 C)), never O(K * T). */
int32_t jolt_dory_fold_rows_grid_am(jolt_ctx *ctx, const jolt_onehot *const *sources, size_t n_sources, const jolt_fr_t *onehot_scalars,
                                    jolt_table *const *dense, size_t n_dense, const jolt_fr_t *dense_scalars,
                                    uint32_t log_block, uint32_t log_stride, uint32_t sigma, const jolt_table *left, jolt_table **out);
/* The placement on the host: *row and *col of (cycle, address).  log_stride > log_block or a null pointer is JOLT_ERR_INVALID_ARG. */
int32_t jolt_host_dory_am_place(uint32_t log_block, uint32_t log_stride, uint32_t sigma, size_t cycle, size_t address, size_t *row, size_t *col);
/* One row of jolt_dory_hints_onehot_am on the host, through the accumulation routine every lane of its kernel runs (limb-form mixed additions, the exceptional
 * cases out of line) and the normalisation: out = sum_{j < cycles_in_row, hot[j] != 0xFFFF} bases[(j << log_block) + (hot[j] << log_stride)].  A lane owns a whole row,
 * so there is no partition to pass.  JOLT_ERR_INVALID_ARG: a null pointer, k = 0 or k > 2^(log_block - log_stride), log_stride > log_block, or fewer bases than
 * ((cycles_in_row - 1) << log_block) + ((k - 1) << log_stride) + 1.  For the CPU suite. */
int32_t jolt_host_dory_am_row(const jolt_g1_t *bases /* z = 1 */, size_t n_bases, const uint16_t *hot, size_t cycles_in_row, uint32_t k, uint32_t log_block,
                              uint32_t log_stride, jolt_g1_t *out);

/* Dory for polynomials held as FIELD ELEMENTS: the first column kind of the reference's trait.  StreamingCommitment::feed(&[Fr]) per row
 * (crates/jolt-dory/src/streaming.rs:53-70), the dense arm of DoryScheme::commit (commit_rows_dense, scheme.rs:455-472), commit_advice
 * (crates/jolt-kernels/src/reference/commitment.rs:101-122):
 *   out[r] = sum_{j < row_width} table[first + r*row_width + j] * srs[j],   r < count / row_width.
 * The scalars are the table's Montgomery words; a scalar s is multiplied as its magnitude min(s, r - s) with the sign folded into the point, and only the windows
 * the stretch's largest magnitude needs are run (an OR-reduction, one synchronisation, as for the integer rows): a table of u64-range values or of small negatives
 * runs the windows jolt_dory_commit_rows runs for the same magnitudes and width.  Full-width scalars widen the digits until the windows fit the row fold
 * (c = max(log2(row_width) - 4, 6) there).  Codes of jolt_dory_commit_rows: a width that is not a power of two JOLT_ERR_INVALID_ARG, JOLT_ERR_SRS_TOO_SMALL,
 * JOLT_ERR_SIZE_MISMATCH when the width does not divide count; first + count beyond the table (wrap-around included) JOLT_ERR_INVALID_ARG.  An all-zero row is the
 * identity (1, 1, 0). */
int32_t jolt_dory_commit_rows_fr(jolt_ctx *ctx, const jolt_srs *srs, const jolt_table *table, size_t first, size_t count, size_t row_width, jolt_g1_t *out);
/* The same rows, normalised, in row order into a resident G1 view: the promises and the contract of jolt_dory_hints_rows. */
int32_t jolt_dory_hints_rows_fr(jolt_ctx *ctx, const jolt_srs *srs, const jolt_table *table, size_t first, size_t count, size_t row_width, jolt_dory_vec *out,
                                size_t out_first);
/* For the CPU suite, through the code the kernels run.  digits_out[w] = |digit| | (digit < 0) << 31 of window w < W of min(s, r - s) in signed c-bit digits
 * (3 <= c <= 13, W <= 85 = ceil(255 / 3): the host form is not held to the device's 48 window sums), *negative_out = 1 when r - s was taken: sum_w digit_w 2^(c w) is s, or r - s negated.  The plan: *c and *W for magnitudes of
 * bit_length bits (1..254) in rows of row_width values. */
int32_t jolt_host_dory_fr_digits(const jolt_fr_t *scalar, int32_t c, int32_t W, uint32_t *digits_out, uint32_t *negative_out);
int32_t jolt_host_dory_rows_fr_plan(uint32_t bit_length, size_t row_width, int32_t *c, int32_t *W);
/* fold_rows of dense field tables, whole or embedded top-left in the grid -- BlockOpeningPoly::fold_rows (crates/jolt-kernels/src/optimized/opening.rs:594-611):
 * coefficient r*2^sigma_d + c of table d sits at grid index r*2^sigma + c, so
 *   out[c] = (base ? base[c] : 0) + sum_d scalars[d] * sum_{r < 2^(m_d - sigma_d)} left[r] * tables[d][(r << sigma_d) + c]   for c < 2^sigma_d (nothing above).
 * With base = the output of jolt_dory_fold_rows_grid or _am it is the joint fold_rows of trace and block-embedded polynomials (advice, bytecode chunks, the program
 * image; the embedding is the same in both placements); with one table of sigma_d = sigma and no base, the dense vector_matrix_product of scheme.rs:612-618.
 * len(tables[d]) = 2^m_d with sigma_d <= min(m_d, sigma), else JOLT_ERR_INVALID_ARG; more rows than `left` has entries or a base not of 2^sigma entries
 * JOLT_ERR_SIZE_MISMATCH; n_tables = 0 JOLT_ERR_INVALID_ARG, more than 8 JOLT_ERR_UNSUPPORTED.  Temporary device memory O(2^sigma * rows / 64). */
int32_t jolt_dory_fold_rows_blocks(jolt_ctx *ctx, jolt_table *const *tables, const uint32_t *sigma_tables, size_t n_tables, const jolt_fr_t *scalars,
                                   uint32_t sigma, const jolt_table *left, const jolt_table *base /* may be NULL */, jolt_table **out /* 2^sigma */);
/* The same fold of up to 256 tables -- a committed program is up to 256 bytecode chunks and the image: a chain of launch sets of eight, each taking the running
 * output as its base.  Field addition is exact, so the output is the one jolt_dory_fold_rows_blocks gives for n_tables <= 8 (that entry is a call of this one) and
 * does not depend on the grouping.  Codes as there; more than 256 tables JOLT_ERR_UNSUPPORTED. */
int32_t jolt_dory_fold_rows_blocks_many(jolt_ctx *ctx, jolt_table *const *tables, const uint32_t *sigma_tables, size_t n_tables, const jolt_fr_t *scalars,
                                        uint32_t sigma, const jolt_table *left, const jolt_table *base /* may be NULL */, jolt_table **out /* 2^sigma */);
/* The claims of block-embedded tables from one pass -- what a stage-8 statement holds for advice, bytecode chunks and the program image (opening_claim * entry.scale,
 * crates/jolt-prover/src/dory/stages/stage8.rs:148-162; BlockOpeningPoly, crates/jolt-kernels/src/optimized/opening.rs:594-611):
 *   claims_out[d] = sum_i tables[d][i] * eq(point, jolt_host_dory_block_index(sigma_tables[d], sigma, i))
 *                 = sum_r L[r] * sum_c R[c] * tables[d][(r << sigma_d) + c],   L = eq(point[:nu]), R = eq(point[nu:]).
 * point is the grid-order opening point, nu + sigma coordinates, most significant first, as jolt_eq_evals indexes; the Lagrange factors of the high row and column
 * coordinates sit inside L[r] and R[c], so the claim is the scaled one.  One launch over all tables (descriptors in device memory) and a small one that adds the
 * workgroups' partial sums (no atomics: the claims do not depend on the grid); the claims are downloaded before the call returns.  Everything is checked before
 * anything is enqueued, codes of jolt_dory_fold_rows_blocks: JOLT_ERR_INVALID_ARG for a null pointer, a table of another context, a length that is not a power of
 * two, sigma_d > m_d or > sigma, a coordinate that is not canonical, n_point != nu + sigma, n_tables = 0; JOLT_ERR_SIZE_MISMATCH for a table of more than 2^nu rows;
 * JOLT_ERR_UNSUPPORTED for more than 256 tables. */
int32_t jolt_dory_evaluate_blocks(jolt_ctx *ctx, jolt_table *const *tables, const uint32_t *sigma_tables, size_t n_tables, const jolt_fr_t *point, size_t n_point,
                                  uint32_t nu, uint32_t sigma, jolt_fr_t *claims_out /* one per table */);
/* *index =((i >> sigma_table) << sigma_grid) | (i & (2^sigma_table - 1)); sigma_table > sigma_grid or an index past 64 bits is JOLT_ERR_INVALID_ARG */
int32_t jolt_host_dory_block_index(uint32_t sigma_table, uint32_t sigma_grid, size_t i, size_t *index);

/* Dory evaluation proofs as one call (dory_scheme.hip): the setup object, a round's in-place update as one call, the prover's side of Eval-VMV-RE under Fiat-Shamir,
 * and the byte forms a transcript absorbs.  The protocol is the one jolt_amd/dory_open.py and dory_reduce.py drive message by message (Dory paper, transparent mode;
 * alpha folds v1 and s1, 1/alpha folds v2 and s2); those drivers stay, as the second implementation the tests compare against.  Contract of the resident entries above:
 * a null handle, a vector, table or setup of another context or of the wrong kind, or a view outside its vector is JOLT_ERR_INVALID_ARG, and a refused call enqueues
 * nothing and writes nothing. */
/* Gamma1 (G1) and Gamma2 (G2) of n points each as resident vectors, Gamma2's prepared line table, H1 and H2: the C counterpart of dory_open.py's DorySetup.  The host
 * arrays pass the checks of jolt_dory_vec_upload once, here.  n = 0 or not a power of two is JOLT_ERR_INVALID_ARG. */
typedef struct jolt_dory_setup jolt_dory_setup;
int32_t jolt_dory_setup_create(jolt_ctx *ctx, const jolt_g1_t *gamma1, const jolt_g2_t *gamma2, size_t n, const jolt_g1_t *h1, const jolt_g2_t *h2, jolt_dory_setup **out);
int32_t jolt_dory_setup_free(jolt_ctx *ctx, jolt_dory_setup *setup);
int32_t jolt_dory_setup_size(const jolt_dory_setup *setup, size_t *n);
/* outs[k] = prod_{i < hint_rows[k]} e(hints[k][hint_first[k] + i], Gamma2[i]): the tier-2 commitments of n resident G1 views as ONE jolt_dory_products batch of PAIR
 * items against the prepared table (an empty view gives one).  A view longer than the setup is JOLT_ERR_INVALID_ARG. */
int32_t jolt_dory_setup_tier2(jolt_ctx *ctx, const jolt_dory_setup *setup, const jolt_dory_vec *const *hints, const size_t *hint_first, const size_t *hint_rows, size_t n,
                              jolt_gt_t *outs);
/* One of the two in-place updates of a Dory-Reduce round as one call.  The G1 work runs on the context's main stream and the G2 work beside it on a side stream,
 * forked and joined by events as jolt_dory_products forks its chains: two launches (k_dory_scale_add per group), in alpha mode followed on each stream by that group's
 * field fold.  Enqueued only, no host synchronisation.  The per-lane functions are the ones of jolt_dory_vec_scale_bases_add / _scale_vs_add / _fold_field, so the
 * vectors hold bit for bit what those separate calls write.
 *   JOLT_DORY_UPDATE_BETA   a = Gamma1 (G1), b = Gamma2 (G2):  v1[v1_first + i] += scalar * a[a_first + i],  v2[v2_first + i] += scalar_inv * b[b_first + i],  i < n
 *   JOLT_DORY_UPDATE_ALPHA  a = s1, b = s2 (Fr), n even, h = n / 2:  x[x_first + i] = c * x[x_first + i] + x[x_first + h + i] for i < h, with c = scalar for v1 and
 *                           s1 and c = scalar_inv for v2 and s2; then each of the four vectors is truncated to its x_first + h elements
 * Beyond the common contract, JOLT_ERR_INVALID_ARG for: an unknown mode, an odd n in alpha mode, overlapping views of one vector in beta mode, a scalar that is not
 * canonical, scalar * scalar_inv != 1. */
enum { JOLT_DORY_UPDATE_BETA = 0, JOLT_DORY_UPDATE_ALPHA = 1 };
int32_t jolt_dory_round_update(jolt_ctx *ctx, int32_t mode, jolt_dory_vec *v1, size_t v1_first, jolt_dory_vec *v2, size_t v2_first, jolt_dory_vec *a, size_t a_first,
                               jolt_dory_vec *b, size_t b_first, size_t n, const jolt_fr_t *scalar, const jolt_fr_t *scalar_inv);
/* The prover's side of one evaluation proof.  Inputs as dory_open.py's DoryOpening: n_hints >= 1 resident G1 views of at most 2^nu row commitments each with one scalar
 * per hint, the device tables v = L^T M (2^sigma entries), L (2^nu) and R (2^sigma); nu <= sigma <= 30.  Everything is checked before anything is enqueued:
 * JOLT_ERR_INVALID_ARG for the common contract, nu > sigma, a hint longer than 2^nu, a table of another length, a scalar that is not canonical;
 * JOLT_ERR_SRS_TOO_SMALL for 2^sigma above the setup's size.  The state is built by jolt_dory_state_*, each message is one jolt_dory_products batch, the updates are
 * jolt_dory_round_update.  After each message `fn` is called with the message's elements and returns the challenge that follows it:
 *   JOLT_DORY_PHASE_VMV     round 0          gts C, D2; g1s E1                                        no challenge
 *   JOLT_DORY_PHASE_FIRST   round k < sigma  gts D1L, D1R, D2L, D2R; g1s E1beta; g2s E2beta           beta_k
 *   JOLT_DORY_PHASE_SECOND  round k          gts C+, C-; g1s E1+, E1-; g2s E2+, E2-                   alpha_k
 *   JOLT_DORY_PHASE_GAMMA   round sigma      no elements                                              gamma
 *   JOLT_DORY_PHASE_FINAL   round sigma      g1s w1; g2s w2                                           no challenge
 * A transcript absorbs a phase's elements in that order (gts, then g1s, then g2s).  challenge_out is never NULL; what VMV and FINAL write there is ignored.  A non-zero
 * return aborts the opening with that status (as jolt_open_transcript_fn).  The library inverts the challenges: zero is JOLT_ERR_NOT_INVERTIBLE, a value that is not
 * canonical JOLT_ERR_INVALID_ARG.  Outputs in protocol order, sized by jolt_host_dory_proof_counts: gts 2 + 6 sigma, g1s 2 + 3 sigma, g2s 1 + 3 sigma,
 * challenges_out (beta_k, alpha_k) per round and then gamma.  GT values are the canonical values of jolt_dory_products, points as its MSM results and the in-place
 * routines leave them (the identity as (1, 1, 0)).  On every exit, an abort included, the streams are drained before the state vectors go back to the pool, and
 * the context stays usable; the inputs stay the caller's. */
enum { JOLT_DORY_PHASE_VMV = 0, JOLT_DORY_PHASE_FIRST = 1, JOLT_DORY_PHASE_SECOND = 2, JOLT_DORY_PHASE_GAMMA = 3, JOLT_DORY_PHASE_FINAL = 4,
       JOLT_DORY_PHASE_D = 5 /* the verifier's last challenge (jolt_host_dory_verify_with_transcript): no elements; the prover's side never sends it */ };
typedef int32_t (*jolt_dory_transcript_fn)(void *user, int32_t phase, size_t round, const jolt_gt_t *gts, size_t n_gt, const jolt_g1_t *g1s, size_t n_g1,
                                           const jolt_g2_t *g2s, size_t n_g2, jolt_fr_t *challenge_out);
int32_t jolt_host_dory_open_with_transcript(jolt_ctx *ctx, const jolt_dory_setup *setup, const jolt_dory_vec *const *hints, const size_t *hint_first,
                                            const size_t *hint_rows, size_t n_hints, const jolt_fr_t *scalars, const jolt_table *v_table, const jolt_table *left,
                                            const jolt_table *right, uint32_t nu, uint32_t sigma, jolt_dory_transcript_fn fn, void *user, jolt_gt_t *gts,
                                            jolt_g1_t *g1s, jolt_g2_t *g2s, jolt_fr_t *challenges_out);
/* The same under one of the library's engines: every element goes in as the reference's adapter absorbs a group element (JoltToDoryTranscript::append_group,
 * crates/jolt-dory/src/transcript.rs:46-53) -- jolt_host_dory_transcript_append_* below -- and every challenge is Transcript::challenge_scalar (full width).  The
 * order of the appends is this header's phase order; dory-pcs's own order is pinned by nothing in the reference checkout (docs/parity.md). */
int32_t jolt_host_dory_open(jolt_ctx *ctx, const jolt_dory_setup *setup, const jolt_dory_vec *const *hints, const size_t *hint_first, const size_t *hint_rows,
                            size_t n_hints, const jolt_fr_t *scalars, const jolt_table *v_table, const jolt_table *left, const jolt_table *right, uint32_t nu,
                            uint32_t sigma, jolt_host_transcript *t, jolt_gt_t *gts, jolt_g1_t *g1s, jolt_g2_t *g2s, jolt_fr_t *challenges_out);
/* HomomorphicBatch::<DoryScheme>::prove_batch (crates/jolt-openings/src/schemes.rs:487-524) on resident inputs: cycle-major placement, transparent mode, under one of
 * the library's engines.  n_claims resident G1 hint views with evaluations[i] as the statement holds them (already scaled, crates/jolt-prover/src/dory/stages/stage8.rs:
 * 148-162); the joint polynomial's columns as jolt_dory_fold_rows_grid takes them (n_claims = the one-hot columns of all sources + n_dense); column_of_claim[i] = claim
 * i's column in that entry's order (one-hot columns source by source, then dense), NULL = the identity -- the batch order (final_opening_polynomial_order) is the
 * caller's; point: log_k + log2(T) coordinates, most significant first, as jolt_eq_evals indexes.  The call
 *   1. absorbs the statement (jolt_host_opening_statement_absorb): scalars_out = 1, gamma, ..., gamma^(n_claims - 1);
 *   2. joint_eval_out = sum_i scalars[i] * evaluations[i];
 *   3. sigma = ceil(n / 2), nu = n - sigma for n = n_point (crates/jolt-dory/src/scheme.rs:242-243); L = eq(point[:nu]), R = eq(point[nu:]);
 *   4. v = jolt_dory_fold_rows_grid under the scalars in column order;
 *   5. checks <v, R> == joint_eval: JOLT_ERR_ROUND_CHECK otherwise, before any state vector is built (the reference's open trusts its eval argument; this entry does
 *      not return a proof of a false statement).  The transcript has absorbed the statement by then and is the caller's to discard;
 *   6. opens as jolt_host_dory_open, the hints weighted by the same scalars (outputs sized by jolt_host_dory_proof_counts(sigma));
 *   7. absorbs the closing claim (jolt_host_opening_claim_absorb) with joint_eval.
 * Contract of jolt_host_dory_open: everything -- this entry's checks, the row fold's, the opening's -- is checked before the transcript absorbs anything and before
 * anything is enqueued; on every exit the streams are drained before pool blocks go back; the inputs stay the caller's; the context stays usable.
 * JOLT_ERR_INVALID_ARG: the common contract, n_claims == 0 or != the number of columns, a column_of_claim that is not a permutation, a point of another length, a value
 * that is not canonical, a hint longer than 2^nu, T not a power of two; JOLT_ERR_SIZE_MISMATCH: columns of different cycle counts; JOLT_ERR_SRS_TOO_SMALL: 2^sigma
 * above the setup's size; JOLT_ERR_UNSUPPORTED: beyond jolt_dory_fold_rows_grid's limits. */
int32_t jolt_host_dory_prove_batch(jolt_ctx *ctx, const jolt_dory_setup *setup, const jolt_dory_vec *const *hints, const size_t *hint_first, const size_t *hint_rows,
                                   size_t n_claims, const jolt_fr_t *evaluations, const jolt_onehot *const *sources, size_t n_sources, jolt_table *const *dense,
                                   size_t n_dense, uint32_t log_k, const size_t *column_of_claim, const jolt_fr_t *point, size_t n_point, jolt_host_transcript *t,
                                   jolt_gt_t *gts, jolt_g1_t *g1s, jolt_g2_t *g2s, jolt_fr_t *challenges_out, jolt_fr_t *scalars_out /* n_claims */,
                                   jolt_fr_t *joint_eval_out);
/* The same over everything prove_stage8 hands to prove_batch (crates/jolt-prover/src/dory/stages/stage8.rs:164-258): the trace columns AND the block-embedded
 * polynomials (trusted and untrusted advice, bytecode chunks, the program image: BlockOpeningPoly, crates/jolt-kernels/src/optimized/opening.rs:594-611), in either
 * trace placement.  Arguments of jolt_host_dory_prove_batch plus
 *   blocks, sigma_blocks, n_blocks   tables of 2^m_d field elements, each 2^(m_d - sigma_d) rows of 2^sigma_d columns top-left in the grid, as
 *                                    jolt_dory_fold_rows_blocks takes them; at most 256;
 *   order                            JOLT_DORY_ORDER_CYCLE_MAJOR or JOLT_DORY_ORDER_ADDRESS_MAJOR (the trace as jolt_dory_fold_rows_grid_am places it, log_block =
 *                                    log_k + log_extra, log_stride = log_extra; a block's embedding is the same in both);
 *   log_extra                        the embedding extra of a widened address-major grid; 0 in the cycle-major placement.
 * n_claims = one-hot columns + n_dense + n_blocks; the columns are the one-hot columns source by source, then the dense columns, then the blocks, and
 * column_of_claim permutes over all of them.  A block's hint is a resident G1 view of its 2^(m_d - sigma_d) row commitments (hints shorter than 2^nu are padded as
 * combine_hints pads them).  point is the GRID-ORDER point as final_opening_point produces it: log_k + log2(T) coordinates cycle-major, log2(T) + log_k + log_extra
 * address-major.  The seven steps above with: step 4 the trace's fold in the chosen placement, then jolt_dory_fold_rows_blocks_many with that as base, gamma's powers
 * taken in claim order and mapped through column_of_claim; step 5 over all claims; step 6 weighting every hint, the blocks' included.  The contract above word for
 * word; beyond its codes JOLT_ERR_INVALID_ARG for an unknown order, log_extra != 0 cycle-major, a block of another context, a length that is not a power of two,
 * sigma_d > m_d or > sigma, a block's hint of another row count than the block; JOLT_ERR_SIZE_MISMATCH for a block of more than 2^nu rows; JOLT_ERR_UNSUPPORTED for
 * more than 256 blocks and for an address-major grid with sigma < log_k + log_extra.  jolt_host_dory_prove_batch is this entry with n_blocks = 0, cycle-major. */
enum { JOLT_DORY_ORDER_CYCLE_MAJOR = 0, JOLT_DORY_ORDER_ADDRESS_MAJOR = 1 };
int32_t jolt_host_dory_prove_batch_blocks(jolt_ctx *ctx, const jolt_dory_setup *setup, const jolt_dory_vec *const *hints, const size_t *hint_first, const size_t *hint_rows,
                                          size_t n_claims, const jolt_fr_t *evaluations, const jolt_onehot *const *sources, size_t n_sources, jolt_table *const *dense,
                                          size_t n_dense, jolt_table *const *blocks, const uint32_t *sigma_blocks, size_t n_blocks, uint32_t log_k, int32_t order,
                                          uint32_t log_extra, const size_t *column_of_claim, const jolt_fr_t *point, size_t n_point, jolt_host_transcript *t,
                                          jolt_gt_t *gts, jolt_g1_t *g1s, jolt_g2_t *g2s, jolt_fr_t *challenges_out, jolt_fr_t *scalars_out /* n_claims */,
                                          jolt_fr_t *joint_eval_out);
/* sigma > 30 is JOLT_ERR_INVALID_ARG; any of the four pointers may be NULL */
int32_t jolt_host_dory_proof_counts(uint32_t sigma, size_t *n_gt, size_t *n_g1, size_t *n_g2, size_t *n_challenges);
/* ark-serialize's compressed forms on the host.  G2: x.c0 then x.c1, 32 little-endian bytes of the canonical value each; the top two bits of the last byte hold the
 * flags: 0x80 when y > -y (c1 compared first, then c0), 0x40 for the identity (x zero).  GT: the twelve canonical Fq coefficients in jolt_gt_t order, 32
 * little-endian bytes each, no flags.  The elements are not checked beyond canonical coordinates (JOLT_ERR_INVALID_ARG).  The G1 form
 * (jolt_host_g1_serialize_compressed) is pinned through the oracle; these two rest on ark-serialize's definition alone (docs/parity.md). */
int32_t jolt_host_g2_serialize_compressed(const jolt_g2_t *p, uint8_t out[64]);
int32_t jolt_host_gt_serialize(const jolt_gt_t *f, uint8_t out[384]);
/* LabelWithCount(b"dory_group", len) and then the bytes above (len = 384, 32, 64) */
int32_t jolt_host_dory_transcript_append_gt(jolt_host_transcript *t, const jolt_gt_t *element);
int32_t jolt_host_dory_transcript_append_g1(jolt_host_transcript *t, const jolt_g1_t *element);
int32_t jolt_host_dory_transcript_append_g2(jolt_host_transcript *t, const jolt_g2_t *element);

/* Dory verification (dory_verify.hip): GT multi-exponentiation on the device, the verifier's precomputed GT values, DoryScheme::verify
 * (crates/jolt-dory/src/scheme.rs:277-308) and HomomorphicBatch::verify_batch (crates/jolt-openings/src/schemes.rs:526-551) as one call each.  The protocol is the
 * transparent Eval-VMV-RE of the entries above; its verifier is the one tests/dory_open_model.py states in log space. */
/* outs[i] = gts[i]^scalars[i]: n independent powers in one launch (k_gt_pow: one lane per element, 254 uniform steps of the GENERAL Fq12 squaring and
 * multiplication, so any canonical Fq12 is a valid base -- no cyclotomic shortcut).  Host pointers in and out.  Refusals as jolt_dory_multi_pair:
 * JOLT_ERR_INVALID_ARG for a null pointer with n > 0, a coordinate or a scalar that is not canonical; JOLT_ERR_UNSUPPORTED for n > 2^20; a refused call enqueues
 * nothing and writes nothing.  Values are canonical Montgomery words: bit for bit jolt_host_gt_pow's. */
int32_t jolt_dory_gt_pow_many(jolt_ctx *ctx, const jolt_gt_t *gts, const jolt_fr_t *scalars, size_t n, jolt_gt_t *outs);
/* DoryScheme::combine (scheme.rs:313-323): out = prod_i gts[i]^scalars[i], the powers as above and their product by the halving tree of the multi-pairings
 * (k_tree_level<Fq12, MulFq12>); n = 0 gives one.  Bit for bit the product of jolt_host_gt_pow's values under jolt_host_fq12_op(MUL). */
int32_t jolt_dory_gt_multi_exp(jolt_ctx *ctx, const jolt_gt_t *gts, const jolt_fr_t *scalars, size_t n, jolt_gt_t *out);
/* The GT values a verifier holds for a setup of n = 2^s bases (DoryVerifierSetup, crates/jolt-dory/src/types.rs), 3 s + 4 of them in this order:
 *   chi_k    = e(Gamma1[:n_k], Gamma2[:n_k]),  n_k = n / 2^k,  k = 0 ... s
 *   Delta1R_k = e(Gamma1[h:n_k], Gamma2[:h]),  h = n_k / 2,    k < s
 *   Delta2R_k = e(Gamma1[:h], Gamma2[h:n_k]),                  k < s
 *   HT = e(H1, H2),  e(H1, Gamma2[0]),  e(Gamma1[0], H2)
 * (Delta1L_k = Delta2L_k = chi_{k+1}).  All from ONE jolt_dory_products batch of PAIR items over the setup's resident vectors.  A proof with sigma < s uses levels
 * s - sigma ... s: the tables are prefixes.  The object belongs to the context of its setup and is freed on it. */
typedef struct jolt_dory_verifier_setup jolt_dory_verifier_setup;
int32_t jolt_dory_verifier_setup_create(jolt_ctx *ctx, const jolt_dory_setup *setup, jolt_dory_verifier_setup **out);
int32_t jolt_dory_verifier_setup_free(jolt_ctx *ctx, jolt_dory_verifier_setup *vs);
int32_t jolt_dory_verifier_setup_values(const jolt_dory_verifier_setup *vs, jolt_gt_t *out /* 3 log2(n) + 4 */);
/* Measurement aid of tools/bench_dory_verify.py, as jolt_dory_pairing_timing: the wall milliseconds of the phases of the last verification made with `vs` while timing
 * was on -- checks, replay, the folds of s1 / s2 and the exponents (host); the group folds (one batch of MSM items); the pairings with their final exponentiations
 * (one batch of PAIR items); the multi-exponentiation.  jolt_dory_gt_pow_many and jolt_dory_gt_multi_exp report into jolt_dory_pairing_timing's clock: checks,
 * host -> device, -, the power kernel (in the Miller kernel's place), the product tree, device -> host, -. */
int32_t jolt_dory_verifier_setup_timing(const jolt_dory_verifier_setup *vs, int32_t enable, double *out_ms /* 4 */);
/* an independent copy of a transcript in its current state (the verifier draws d from one) */
int32_t jolt_host_transcript_clone(const jolt_host_transcript *t, jolt_host_transcript **out);
/* Every exponent of the verifier's final equation, in Fr on the host.  challenges: (beta_k, alpha_k) per round, then gamma; s1, s2: the folded scalars (single
 * elements).  With d1_0 = the commitment, d2_0 = the VMV message's D2 and the recurrences
 *   c_{k+1} = c_k chi_k d2_k^beta d1_k^(1/beta) C+^alpha C-^(1/alpha),  d1_{k+1} = (D1L chi_{k+1}^beta)^alpha D1R Delta1R_k^beta,
 *   d2_{k+1} = (D2L chi_{k+1}^(1/beta))^(1/alpha) D2R Delta2R_k^(1/beta)
 * the right-hand side  chi_sigma c_sigma HT^(s1 s2) (d2_sigma e(Gamma1[0], H2)^(s2 / gamma))^d (d1_sigma e(H1, Gamma2[0])^(gamma s1))^(1/d)  is one product of powers:
 *   exp_proof_gt    2 + 6 sigma, the proof's GT elements in proof order (C, D2, then per round D1L, D1R, D2L, D2R, C+, C-)
 *   exp_commitment  one
 *   exp_setup       3 sigma + 4, in the order of jolt_dory_verifier_setup_values for a setup of 2^sigma bases
 * and the folds of the group elements are E1' = sum coef_g1 * (E1, then E1beta, E1+, E1- per round), E2' = coef_h2 * H2 + sum coef_g2 * (E2beta, E2+, E2- per round).
 * JOLT_ERR_INVALID_ARG: a null pointer, sigma > 30, a value that is not canonical; JOLT_ERR_NOT_INVERTIBLE: a zero challenge or d. */
int32_t jolt_host_dory_verify_exponents(uint32_t sigma, const jolt_fr_t *challenges, const jolt_fr_t *d, const jolt_fr_t *s1, const jolt_fr_t *s2, const jolt_fr_t *y,
                                        jolt_fr_t *exp_proof_gt, jolt_fr_t *exp_commitment, jolt_fr_t *exp_setup, jolt_fr_t *coef_g1, jolt_fr_t *coef_g2,
                                        jolt_fr_t *coef_h2);
/* DoryScheme::verify as one call.  commitment: the tier-2 commitment; y: the claimed evaluation L^T M R; left (2^nu) and right (2^sigma) host arrays; gts, g1s, g2s as
 * jolt_host_dory_open wrote them.  The call
 *   1. replays the transcript: `fn` is called phase by phase with the proof's elements in jolt_host_dory_open's order and returns beta_k, alpha_k, gamma; then once more
 *      with JOLT_DORY_PHASE_D (no elements) for d.  The prover's side never sends PHASE_D.  A zero challenge is JOLT_ERR_NOT_INVERTIBLE;
 *   2. folds s1 from `right` under alpha and s2 from `left` (padded with zeros) under 1 / alpha, on the host;
 *   3. computes every exponent (jolt_host_dory_verify_exponents);
 *   4. folds the group elements: E1', E2', w1 + d Gamma1[0], w2 + Gamma2[0] / d, -gamma H1, -E1' / gamma, as one jolt_dory_products batch of MSM items;
 *   5. checks (VMV) e(E1, H2) = D2 and (final) e(w1 + d Gamma1[0], w2 + Gamma2[0] / d) e(-gamma H1, E2') e(-E1' / gamma, H2) = ONE jolt_dory_gt_multi_exp over the
 *      proof's GT elements, the commitment and the setup values; both left-hand sides are PAIR items of one product batch.
 * *accepted = 1 only if both checks hold; a rejected proof is JOLT_OK with *accepted = 0 and *failed_check = 1 (VMV) or 2 (final), 0 when accepted.  Status codes are
 * for malformed input -- JOLT_ERR_INVALID_ARG for a null pointer, a value that is not canonical, a point off its curve, nu > sigma, sigma > 30, a setup of another
 * context or a verifier setup of another setup's size -- and JOLT_ERR_SRS_TOO_SMALL; everything is checked before the transcript absorbs anything. */
int32_t jolt_host_dory_verify_with_transcript(jolt_ctx *ctx, const jolt_dory_verifier_setup *vs, const jolt_dory_setup *setup, const jolt_gt_t *commitment,
                                              const jolt_fr_t *y, const jolt_fr_t *left, const jolt_fr_t *right, uint32_t nu, uint32_t sigma, const jolt_gt_t *gts,
                                              const jolt_g1_t *g1s, const jolt_g2_t *g2s, jolt_dory_transcript_fn fn, void *user, int32_t *accepted,
                                              int32_t *failed_check);
/* The same under one of the library's engines: elements absorbed as jolt_host_dory_open absorbs them; d is drawn from a COPY of the transcript taken after the final
 * message, so the caller's transcript ends in exactly the state jolt_host_dory_open leaves the prover's in (the prover draws no d). */
int32_t jolt_host_dory_verify(jolt_ctx *ctx, const jolt_dory_verifier_setup *vs, const jolt_dory_setup *setup, const jolt_gt_t *commitment, const jolt_fr_t *y,
                              const jolt_fr_t *left, const jolt_fr_t *right, uint32_t nu, uint32_t sigma, const jolt_gt_t *gts, const jolt_g1_t *g1s,
                              const jolt_g2_t *g2s, jolt_host_transcript *t, int32_t *accepted, int32_t *failed_check);
/* HomomorphicBatch::<DoryScheme>::verify_batch (schemes.rs:526-551): the statement (jolt_host_opening_statement_absorb) gives gamma's powers and the joint
 * evaluation; sigma = ceil(n_point / 2), nu = n_point - sigma, L = eq(point[:nu]), R = eq(point[nu:]) as jolt_host_dory_prove_batch splits the point; `combine` is
 * not a separate pass -- commitment i enters the one multi-exponentiation with exponent gamma^i * exp_commitment; then the closing claim
 * (jolt_host_opening_claim_absorb) on both outcomes.  The transcript ends in the state jolt_host_dory_prove_batch_blocks leaves.  The placement and the blocks do
 * not appear: a verifier sees commitments, evaluations and the grid-order point.  n_claims = 0 is JOLT_ERR_INVALID_ARG; otherwise the codes of jolt_host_dory_verify. */
int32_t jolt_host_dory_verify_batch(jolt_ctx *ctx, const jolt_dory_verifier_setup *vs, const jolt_dory_setup *setup, const jolt_gt_t *commitments,
                                    const jolt_fr_t *evaluations, size_t n_claims, const jolt_fr_t *point, size_t n_point, const jolt_gt_t *gts,
                                    const jolt_g1_t *g1s, const jolt_g2_t *g2s, jolt_host_transcript *t, int32_t *accepted, int32_t *failed_check,
                                    jolt_fr_t *joint_eval_out);

/* Promotion of device-resident integers (entries [offset, offset+len) of `values`) to a field table: Ring::from_u64 / from_i64 /
 * from_i128 per entry (crates/jolt-field/src/bn254/mod.rs:265-328), the From<T> of Polynomial<T>::bind_to_field (dense.rs:129-142)
 * for witness columns that already sit in HBM (no host round trip; jolt_table_from_u64 is the same from host memory). */
int32_t jolt_table_from_ints(jolt_ctx *ctx, const jolt_ints *values, size_t offset, size_t len, jolt_table **out);

/* The committed trace polynomials over the proof's shared commitment grid, for a KZG-type scheme (HyperKZG).  Every witness
 * polynomial is committed in one grid of log_k + log_t variables (crates/jolt-kernels/src/commitment.rs:1-8,86-130); cycle-major
 * placement: coefficient (address k, cycle j) at index k*T + j, dense columns at k = 0 (TracePlacement / TraceOpeningPoly::entry,
 * crates/jolt-kernels/src/optimized/opening.rs:340-372,404-420).
 *   jolt_grid_commit_onehot: out[p] = sum over the hot cycles j of column p of srs[hot_p(j)*T + j] -- kzg_commit
 *     (crates/jolt-hyperkzg/src/kzg.rs:15-27) of a polynomial whose coefficients are 0/1 with one 1 per hot cycle: additions only.
 *     source->k * T > srs length is JOLT_ERR_SRS_TOO_SMALL.
 *   jolt_grid_joint_polynomial: the joint polynomial of HomomorphicBatch::prove_batch (crates/jolt-openings/src/schemes.rs:487-524,
 *     RlcSource::to_dense crates/jolt-poly/src/multilinear.rs:159-170) over the 2^log_k * T grid:
 *     out[k*T + j] = sum_p onehot_scalars[p] * [hot_p(j) == k] + [k == 0] * sum_d dense_scalars[d] * dense[d][j];
 *     onehot_scalars runs over the polynomials of sources[0], sources[1], ... in order.  <= 4 sources, <= 8 dense columns. */
int32_t jolt_grid_commit_onehot(jolt_ctx *ctx, const jolt_srs *srs, const jolt_onehot *source, jolt_g1_t *out /* n_polys */);
int32_t jolt_grid_joint_polynomial(jolt_ctx *ctx, const jolt_onehot *const *sources, size_t n_sources, const jolt_fr_t *onehot_scalars,
                                   jolt_table *const *dense, size_t n_dense, const jolt_fr_t *dense_scalars, uint32_t log_k,
                                   jolt_table **out);
/* The claims of a stage-8 statement from one pass over the witness: claims_out[c] = the multilinear evaluation of column c of that grid at `point`, for the
 * columns jolt_dory_fold_rows_grid and jolt_grid_joint_polynomial take, in their order (one-hot columns source by source, then dense):
 *   one-hot p:  sum over the hot cycles j of eq_a[hot_p(j)] * eq_c[j]        dense d:  eq_a[0] * sum_j eq_c[j] * dense[d][j]
 * with eq_a = eq(point[:log_k]) and eq_c = eq(point[log_k:]); point has log_k + log2(T) coordinates, most significant first, as jolt_eq_evals indexes.  One launch over
 * the columns and a small one that adds the workgroups' partial sums (no atomics: the claims do not depend on the grid); the claims are downloaded before the call
 * returns.  Everything is checked before anything is enqueued: JOLT_ERR_INVALID_ARG for a null pointer, a source or table of another context, T not a power of two,
 * n_point != log_k + log2(T), a coordinate that is not canonical, source->k > 2^log_k; JOLT_ERR_SIZE_MISMATCH for columns of different cycle counts;
 * JOLT_ERR_UNSUPPORTED beyond the limits of jolt_grid_joint_polynomial (4 sources, 8 dense columns, log_k <= 8, at least one column). */
int32_t jolt_grid_evaluate_columns(jolt_ctx *ctx, const jolt_onehot *const *sources, size_t n_sources, jolt_table *const *dense, size_t n_dense, uint32_t log_k,
                                   const jolt_fr_t *point, size_t n_point, jolt_fr_t *claims_out /* one per column */);

/* Instruction read+RAF checking (stage 5) -- SURVEY.md section 8(f) row 4.  Replaces the T-scale scans of
 * OptimizedInstructionReadRafKernel (crates/jolt-kernels/src/optimized/instruction_read_raf.rs): per prefix-suffix phase the
 * condensation of the per-cycle mass (:750-758), the fused RAF scan (:770-812) and the per-table suffix accumulators
 * (init_suffix_tables :901-971), and after the address rounds the combined-value / ra_i columns of the cycle rounds
 * (pending_combined_base / pending_ra_base :1203-1232; sum them with jolt_member_create_split_eq_lc: one group of 1 + ra_count factors).
 * The 256-entry prefix polynomials, checkpoints and address-round messages are host code (jolt_host_read_raf_address_* below); the flag claims of output_claims are
 * jolt_onehot_pushforward over the table-index column.
 *   rows: lookup_index as (lo, hi) u64 pairs, table_index (0xFF = no lookup table; < n_tables <= 126), raf_flag (0 / 1).
 *   suffix_offsets[n_tables + 1] / suffix_kinds[]: LookupTableKind::suffixes() of every table, flattened; a kind is the discriminant of
 *     `enum Suffixes` (crates/jolt-lookup-tables/src/tables/suffixes/mod.rs:120-170, all 48 built; XLEN = 64).
 *   jolt_read_raf_phase_scan: raf_out[q * 256 + chunk], q = left, right, identity, shift_half, shift_full, upper_all_ones (raw sums: the
 *     caller applies mul_pow_2 to the shift sums, :814-823; upper_all_ones only with canonical != 0, the `akita` feature);
 *     suffix_out[(suffix_offsets[t] + s) * 256 + chunk]; chunk = (lookup_index >> suffix_len) & 255, suffix_len = address_bits - 8 (phase + 1).
 *   jolt_read_raf_condense: u[j] *= v_table[(lookup_index[j] >> shift) & 255].
 *   jolt_read_raf_cycle_tables: v_tables = the `phases` bound-challenge eq tables (256 entries each), phases * 8 = address_bits. */
typedef struct jolt_read_raf jolt_read_raf;
int32_t jolt_read_raf_create(jolt_ctx *ctx, const uint64_t *lookup_index, const uint8_t *table_index, const uint8_t *raf_flag, size_t cycles, uint32_t n_tables,
                             jolt_read_raf **out);
int32_t jolt_read_raf_destroy(jolt_ctx *ctx, jolt_read_raf *rr);
int32_t jolt_read_raf_cycles(const jolt_read_raf *rr, size_t *cycles, uint32_t *n_tables);
int32_t jolt_read_raf_phase_scan(jolt_ctx *ctx, jolt_read_raf *rr, const jolt_table *u, uint32_t suffix_len, uint32_t address_bits, int32_t canonical,
                                 const uint32_t *suffix_offsets, const uint8_t *suffix_kinds, jolt_fr_t *raf_out, jolt_fr_t *suffix_out);
int32_t jolt_read_raf_condense(jolt_ctx *ctx, jolt_read_raf *rr, jolt_table *u, const jolt_fr_t *v_table, uint32_t shift);
int32_t jolt_read_raf_cycle_tables(jolt_ctx *ctx, jolt_read_raf *rr, const jolt_fr_t *table_values, const jolt_fr_t *raf_interleaved, const jolt_fr_t *raf_identity,
                                   const jolt_fr_t *v_tables, uint32_t phases, uint32_t address_bits, uint32_t ra_count, jolt_table **combined_out,
                                   jolt_table **ra_out);
/* suffix_mle.hip.h (Suffixes::suffix_mle for the kind's discriminant) built for the host, for the CPU suite; bits are masked to `len`. */
int32_t jolt_host_suffix_mle(uint32_t kind, uint64_t lo, uint64_t hi, uint32_t len, uint64_t *out);

/* The address rounds of the same kernel (host code, no device work): the 256-entry prefix polynomials of a phase, the per-table `combine`, the four RAF
 * decompositions, the round messages and binds, checkpoints.  Replaces instruction_read_raf.rs address_message (:973-1050), the address branch of bind
 * (:1235-1282), the prefix half of init_phase (:824-898) and init_cycle_rounds' table values (:1140-1160), and what they call in jolt-lookup-tables:
 * Prefixes::{default_checkpoint, evaluate} (tables/prefixes/mod.rs:236-250 + the 44 prefix files) and LookupTableKind::{prefixes, suffixes, combine}
 * (tables/mod.rs:228-246 + the 42 table files).  Table / prefix / suffix ids are the discriminants of `enum LookupTableKind` (tables/mod.rs:121-166),
 * `enum Prefixes` (prefixes/mod.rs:104-154) and `enum Suffixes`; XLEN = 64, phases of 8 address bits.
 *   jolt_lookup_suffix_layout: offsets[43] / kinds[]: the suffix_offsets / suffix_kinds arguments of jolt_read_raf_phase_scan for n_tables = 42 real tables.
 *   per phase p = 0 .. 15:  jolt_read_raf_phase_scan (device) -> jolt_host_read_raf_address_init_phase(p, raf_out, suffix_out) -> 8 x { message, bind };
 *     message: evals_out = s(0), s(1) = previous_claim - s(0), s(2) (UnivariatePoly::from_evals order); bind: *phase_done = 1 after the 8th, when
 *     jolt_host_read_raf_address_v_table(p) is eq(phase challenges, .) for jolt_read_raf_condense / jolt_read_raf_cycle_tables.
 *     message with previous_claim == NULL sums s(1) from the tables: in round 0, s(0) + s(1) is then the relation's input claim.
 *   jolt_host_read_raf_address_prove_phase: the 8 rounds of the open phase in one call (message -> from_evals coefficients c0, c1, c2 -> transcript ->
 *     bind); the transcript is the caller's jolt_round_transcript_fn or, with fn == NULL, the library's TEST transcript (append c0..c2, Transcript::challenge).
 *   jolt_host_read_raf_address_finish: after phase 15: table_values[42], raf_interleaved, raf_identity = the arguments of jolt_read_raf_cycle_tables.
 *   canonical != 0 is the `akita` feature's upper-all-ones term (CANONICAL_INSTRUCTION_ADDRESS).
 * jolt_host_lookup_prefix_evaluate / jolt_host_lookup_table_combine expose the two building blocks for the decomposition test
 * (tables/test_utils.rs prefix_suffix_test): b of b_len <= 16 bits (even), checkpoints / prefixes = all 49 slots. */
typedef struct jolt_read_raf_address jolt_read_raf_address;
uint32_t jolt_lookup_table_count(void);
uint32_t jolt_lookup_prefix_count(void);
int32_t jolt_lookup_table_suffixes(uint32_t kind, uint8_t *kinds_out /* <= 5 */, uint32_t *n_out);
int32_t jolt_lookup_table_prefixes(uint32_t kind, uint8_t *prefixes_out /* <= 4 */, uint32_t *n_out);
int32_t jolt_lookup_suffix_layout(uint32_t *offsets_out /* 43 */, uint8_t *kinds_out /* offsets_out[42]; may be NULL */);
int32_t jolt_host_lookup_prefix_default_checkpoints(jolt_fr_t *out /* 49 */);
int32_t jolt_host_lookup_prefix_evaluate(uint32_t prefix, const jolt_fr_t *checkpoints, uint32_t b, uint32_t b_len, uint32_t suffix_len, jolt_fr_t *out);
int32_t jolt_host_lookup_prefix_table(uint32_t prefix, const jolt_fr_t *checkpoints, uint32_t b_len, uint32_t suffix_len, jolt_fr_t *out /* 2^b_len */);
int32_t jolt_host_lookup_table_combine(uint32_t kind, const jolt_fr_t *prefixes, const jolt_fr_t *suffixes, jolt_fr_t *out);
int32_t jolt_host_read_raf_address_create(const jolt_fr_t *gamma, const uint8_t *table_present /* 42 */, int32_t canonical, jolt_read_raf_address **out);
int32_t jolt_host_read_raf_address_destroy(jolt_read_raf_address *h);
int32_t jolt_host_read_raf_address_init_phase(jolt_read_raf_address *h, uint32_t phase, const jolt_fr_t *raf_sums, const jolt_fr_t *suffix_sums);
int32_t jolt_host_read_raf_address_message(jolt_read_raf_address *h, const jolt_fr_t *previous_claim, jolt_fr_t *evals_out /* 3 */);
int32_t jolt_host_read_raf_address_bind(jolt_read_raf_address *h, const jolt_fr_t *challenge, int32_t *phase_done);
/* bind + the next round's message in one hand-off (ProveRounds::prove_round with Some(bind), prover.rs:45-51), for the 1st .. 7th bind of a phase */
int32_t jolt_host_read_raf_address_bind_message(jolt_read_raf_address *h, const jolt_fr_t *challenge, const jolt_fr_t *previous_claim, jolt_fr_t *evals_out /* 3 */);
int32_t jolt_host_read_raf_address_prove_phase(jolt_read_raf_address *h, jolt_fr_t *claim, jolt_round_transcript_fn fn, void *user, jolt_host_transcript *test_transcript,
                                               jolt_fr_t *coeffs_out /* 8 x 3; may be NULL */, jolt_fr_t *challenges_out /* 8; may be NULL */);
int32_t jolt_host_read_raf_address_v_table(const jolt_read_raf_address *h, uint32_t phase, jolt_fr_t *out /* 256 */);
int32_t jolt_host_read_raf_address_finish(const jolt_read_raf_address *h, jolt_fr_t *table_values /* 42 */, jolt_fr_t *raf_interleaved, jolt_fr_t *raf_identity);

/* Spartan outer (stage 1) T-scale sums -- SURVEY.md section 8(f) row 3 (crates/jolt-kernels/src/{reference,optimized}/spartan_outer.rs).
 * The constraint list, spartan_outer_row_weights and the Lagrange interpolation stay in Rust (O(rows) work); the caller folds the
 * per-(node, stream) row weights into per-column weights (ConstraintMatrices::weighted_columns + public_column_contributions,
 * reference/spartan_outer.rs:246-256): weights are laid out [node][stream][1 + n_inputs], column 0 = the constant.
 *   jolt_r1cs_uniskip_sums: out[node] = sum_t sum_s eq[(t << 1) | s] * Az(node,s,t) * Bz(node,s,t), Az(node,s,t) = c_0 + sum_v c_v z_v(t)
 *     -- the extended-node evaluations t1 of uniskip_first_round_poly (:172-221); eq has 2 * cycles entries (tau_low, stream = LSB).
 *   jolt_r1cs_materialize: az[(t << 1) | s], bz[(t << 1) | s] for ONE (node =) uni-skip challenge: the remainder member's linear
 *     forms over the joint (cycle || stream) domain (:236-300); feed them to jolt_member_create_split_eq_product with w = tau_low
 *     and scale = the Lagrange kernel value for all log_t + 1 remainder rounds.
 *   jolt_tables_evaluate: out[k] = tables[k] evaluated at `point`, all from one eq expansion (the post-hoc opening evaluation of
 *     the 35 inputs, optimized/spartan_outer.rs:41-43; Polynomial::evaluate, dense.rs:340-366).  <= 64 tables. */
int32_t jolt_r1cs_uniskip_sums(jolt_ctx *ctx, jolt_table *const *inputs, size_t n_inputs, const jolt_table *eq, const jolt_fr_t *a_weights,
                               const jolt_fr_t *b_weights, size_t n_nodes, jolt_fr_t *out);
int32_t jolt_r1cs_materialize(jolt_ctx *ctx, jolt_table *const *inputs, size_t n_inputs, const jolt_fr_t *a_weights, const jolt_fr_t *b_weights,
                              jolt_table **az_out, jolt_table **bz_out);
int32_t jolt_tables_evaluate(jolt_ctx *ctx, jolt_table *const *tables, size_t k, const jolt_fr_t *point, size_t n, jolt_fr_t *out);

/* The same three operators straight off the INTEGER witness columns (jolt_ints of kind u64 / i64 / i128), as the optimized tier runs
 * them (crates/jolt-kernels/src/optimized/spartan_outer.rs:6-43,276-370,780-850) on FrSmallScalarAccumulator-style deferred reduction
 * (crates/jolt-field/src/bn254/mont.rs:286-305,343-427): the 35 inputs are never promoted to field tables.
 *   jolt_r1cs_uniskip_sums_small: INTEGER weights (the exact integer Lagrange extension coefficients folded into column weights,
 *     extension_coefficients :276-306): Az / Bz are integer dot products, their product times eq is one field multiply per
 *     (node, cycle, stream).  Contract (the caller's, as in the reference: |az| < 2^22, |bz| < 2^152 there): |Az| < 2^127,
 *     |Bz| < 2^255, |Az * Bz| < 2^254, no weight equal to INT64_MIN.
 *   jolt_r1cs_materialize_small: FIELD weights (they carry the Lagrange kernel at the uni-skip challenge) x integer values, one
 *     reduction per output (fold_group :363-370).
 *   jolt_ints_evaluate: out[k] = sum_t eq(point, t) * z_k(t) (compute_claimed_inputs :780-850; Polynomial::<T>::evaluate).
 * n_streams = 2: Spartan outer (weights [node][stream][1 + n], eq over (cycle || stream), outputs az[(t << 1) | s]).
 * n_streams = 1: Spartan PRODUCT virtualization (stage 2, crates/jolt-kernels/src/optimized/spartan_product.rs:86-230,321-437): "A" = the
 *   left factor lanes, "B" = the right factor lanes, 5 extended nodes of the 3-node window, eq = eq(tau_low, .) over the cycles, and the
 *   two outputs of jolt_r1cs_materialize_small are the remainder's left / right tables (feed jolt_member_create_split_eq_product).
 * Results equal the field-arithmetic operators above on the promoted columns (exact algebra). */
int32_t jolt_r1cs_uniskip_sums_small(jolt_ctx *ctx, const jolt_ints *const *inputs, size_t n_inputs, const jolt_table *eq, uint32_t n_streams,
                                     const int64_t *a_weights, const int64_t *b_weights, size_t n_nodes, jolt_fr_t *out);
int32_t jolt_r1cs_materialize_small(jolt_ctx *ctx, const jolt_ints *const *inputs, size_t n_inputs, uint32_t n_streams, const jolt_fr_t *a_weights,
                                    const jolt_fr_t *b_weights, jolt_table **az_out, jolt_table **bz_out);
int32_t jolt_ints_evaluate(jolt_ctx *ctx, const jolt_ints *const *columns, size_t k, const jolt_fr_t *point, size_t n, jolt_fr_t *out);

/* ------------------------------------------------------------------------------------------------------------
 * A constraint system as ROWS over a centred uni-skip domain, and the first round off the rows.
 *
 * The column form above takes the rows already folded with the integer extension coefficients into int64 column weights.  The reference's own system cannot be
 * folded that way: row 8's B side is right_lookup - left + right - 2^64 (crates/jolt-kernels/src/optimized/spartan_outer.rs:243-247), and that constant times an
 * extension coefficient of about 2^18 has no int64.  A jolt_r1cs_rows keeps the rows: n_streams in {1, 2} (spartan_outer has two row groups selected by the stream
 * variable, crates/jolt-r1cs/src/constraints/jolt.rs:69-92; spartan_product has one), the uni-skip domain_size D (2 <= D <= 16), per stream at most D rows at the
 * domain positions 0, 1, ... (rows_per_stream; the rows are listed stream 0 first), n_inputs columns (<= 64), and per row the A and the B side as a sparse linear
 * form over z = (1, inputs): entries [offsets[r], offsets[r + 1]) of columns (0-based input index) / coefficients (int64, not INT64_MIN), an int64 constant for A
 * and a signed 128-bit constant (lo, hi; two's complement) for B.  zero_on_domain: the rows hold on every cycle, so t1 vanishes on the D domain nodes and only the
 * D - 1 nodes outside are evaluated (reference/spartan_outer.rs:183-188); without it all 2D - 1 nodes are (reference/spartan_product.rs:180-200).
 * Creation computes the integer extension coefficients L_i(node) of the 2D - 1 centred extended nodes -(D - 1) .. D - 1 in 128-bit arithmetic and refuses a
 * system whose coefficients leave int64 (JOLT_ERR_UNSUPPORTED); an out-of-range column, an INT64_MIN coefficient, more than D rows in a stream or a D outside the
 * range is JOLT_ERR_INVALID_ARG.
 *   jolt_r1cs_rows_extension: the (2D - 1) x D coefficients.  jolt_r1cs_rows_fold_small: the column form [node][stream][1 + n_inputs] of the evaluated nodes (what
 *     jolt_r1cs_uniskip_sums_small takes) where every folded weight has an int64, JOLT_ERR_UNSUPPORTED otherwise; NULL outputs ask for the node count.
 *   jolt_r1cs_uniskip_sums_rows: sums_out[node] (2D - 1 entries, skipped nodes 0) = sum_t sum_s eq[t * S + s] * Az(node,s,t) * Bz(node,s,t) with
 *     Az(node,s,t) = sum_i L_i(node) a_{s,i}(t), Bz likewise: per cycle and stream the row values once as exact integers, per node a D-term integer extension, one
 *     exact product and one field multiplication (optimized/spartan_outer.rs:183-340).  Columns: jolt_ints of kind U64 / I64 / I128, n_cols = n_inputs.
 *   Range contract (the caller's, as for the column form): |row A value| and |Az(node)| < 2^127, |row B value| and |Bz(node)| < 2^191, |Az * Bz| < 2^254; the
 *     reference's rows stay below 2^22, 2^152 and 2^174.
 *   jolt_host_r1cs_rows_cycle: the same per-cycle text built for the host (no device): Az (128-bit) and Bz (256-bit) two's complement, |Az * Bz| and its sign, for
 *     one cycle's inputs (2 words per input as the column kind stores them), one stream and one extended-node position.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct jolt_r1cs_rows jolt_r1cs_rows;
int32_t jolt_r1cs_rows_create(uint32_t n_streams, uint32_t domain_size, const uint32_t *rows_per_stream, uint32_t n_inputs, const uint32_t *a_offsets,
                              const uint32_t *a_columns, const int64_t *a_coefficients, const int64_t *a_constants, const uint32_t *b_offsets,
                              const uint32_t *b_columns, const int64_t *b_coefficients, const uint64_t *b_constants /* 2 per row */, int32_t zero_on_domain,
                              jolt_r1cs_rows **out);
int32_t jolt_r1cs_rows_destroy(jolt_r1cs_rows *rows);
int32_t jolt_r1cs_rows_extension(const jolt_r1cs_rows *rows, int64_t *out /* (2D - 1) x D */);
int32_t jolt_r1cs_rows_fold_small(const jolt_r1cs_rows *rows, int64_t *a_weights, int64_t *b_weights, size_t *n_nodes);
int32_t jolt_r1cs_uniskip_sums_rows(jolt_ctx *ctx, const jolt_r1cs_rows *rows, const jolt_ints *const *cols, size_t n_cols, const jolt_table *eq,
                                    jolt_fr_t *sums_out /* 2D - 1 */);
int32_t jolt_host_r1cs_rows_cycle(const jolt_r1cs_rows *rows, const uint64_t *values, const int32_t *kinds, uint32_t stream, uint32_t node, uint64_t *az_out /* 2 */,
                                  uint64_t *bz_out /* 4 */, uint64_t *product_out /* 4 */, int32_t *negative_out);

/* The uni-skip first round above the sums (host; any transcript engine of this header).
 *   jolt_host_centered_lagrange_evals: L_0(r) .. L_{D-1}(r) over the centred domain -((D - 1) / 2) .. (crates/jolt-poly/src/lagrange.rs:25-77; a grid point gives the
 *     unit vector).  jolt_host_centered_lagrange_kernel: LK(x, y) = sum_i L_i(x) L_i(y) (:92-104).  jolt_host_interpolate_to_coeffs: the monomial coefficients of
 *     the polynomial through `values` at domain_start, domain_start + 1, ... (:567-608).
 *   jolt_host_uniskip_first_round_poly: s1 = interpolate_to_coeffs(domain_start, centered_lagrange_evals(D, tau_high)) x interpolate_to_coeffs(extended_start, t1),
 *     3D - 2 coefficients (crates/jolt-kernels/src/reference/spartan_outer.rs:217-225).
 *   jolt_host_prove_uniskip: prove_uniskip_clear (crates/jolt-sumcheck/src/prover.rs:415-440): the degree bound 3D - 3 (n - 1 above it: JOLT_ERR_UNSUPPORTED), the
 *     centred-domain round check sum_k c_k S_k = input_claim with the i128 power sums (domain.rs:11-41, lagrange.rs:499-534; JOLT_ERR_ROUND_CHECK; a power sum that
 *     leaves i128 is the reference's InvalidIntegerDomain, JOLT_ERR_UNSUPPORTED), LabelWithCount("uniskip_poly", n) and ALL n coefficients absorbed
 *     (round_proof.rs:70-86), Transcript::challenge, the output claim s1(r0), append_labeled("opening_claim", claim).
 *   jolt_host_r1cs_rows_remainder_weights: what jolt_stage_spartan_remainder_rows_create derives, without a device: a_weights / b_weights [stream][1 + n_inputs]. */
int32_t jolt_host_centered_lagrange_evals(size_t domain_size, const jolt_fr_t *r, jolt_fr_t *out);
int32_t jolt_host_centered_lagrange_kernel(size_t domain_size, const jolt_fr_t *x, const jolt_fr_t *y, jolt_fr_t *out);
int32_t jolt_host_interpolate_to_coeffs(int64_t domain_start, const jolt_fr_t *values, size_t n, jolt_fr_t *out);
int32_t jolt_host_uniskip_first_round_poly(size_t domain_size, const jolt_fr_t *tau_high, const jolt_fr_t *t1 /* 2D - 1 */, jolt_fr_t *coeffs_out /* 3D - 2 */);
int32_t jolt_host_prove_uniskip(jolt_host_transcript *transcript, const jolt_fr_t *coeffs, size_t n, size_t domain_size, const jolt_fr_t *input_claim, jolt_fr_t *r0_out,
                                jolt_fr_t *output_claim_out);
int32_t jolt_host_r1cs_rows_remainder_weights(const jolt_r1cs_rows *rows, const jolt_fr_t *r0, const jolt_fr_t *tau_high, jolt_fr_t *a_weights, jolt_fr_t *b_weights,
                                              jolt_fr_t *scale);
/* csrc/small_scalar.hip.h built for the host (CPU suite): sum_k values[k] * scalars[k], scalars as signed 128-bit (lo, hi) pairs. */
int32_t jolt_host_small_scalar_dot(const jolt_fr_t *values, const uint64_t *scalars, size_t n, jolt_fr_t *out);

/* Sparse (K x T) read-write matrix of RAM read/write checking (stage 2) -- SURVEY.md section 8(f) row 4.  Replaces
 * CycleMajorMatrix / AddressMajorMatrix and the round messages of RamReadWriteKernel (crates/jolt-kernels/src/optimized/rw_matrix.rs,
 * optimized/ram_read_write.rs:58-330): summand eq(tau_low, j) * ra(k,j) * (val(k,j) + gamma * (val(k,j) + inc(j))) over
 * (address || cycle), bound low-to-high with the log_t cycle variables first (the default read-write config, the only one the
 * reference kernels support, ram_read_write.rs:281-286); one entry per RAM access, never a K x T grid.
 *   create: addresses[j] = remapped word address of cycle j or UINT64_MAX (RamAccessColumns, optimized/ram_trace.rs:22-75),
 *     pre / post = the word before / after the access; inc (T entries) and val_init (K entries) are copied.
 *   prove_round: ProveRounds::prove_round, device half.  Rounds < log_t return (q(0), q_inf) of the quadratic factor and
 *     aux_out = {current_scalar, tau_low[current_index - 1], 0}: the caller completes the cubic with gruen_poly_deg_3
 *     (split_eq.rs:383-417); later rounds return (s(0), s(2)), s(1) comes from the claim (UnivariatePoly::from_evals_and_hint).
 *   final_values: {ra, val, inc, bound cycle-eq factor} (RamReadWriteOutputClaims + validate_derived_tables). */
typedef struct jolt_rw_matrix jolt_rw_matrix;
int32_t jolt_rw_matrix_create(jolt_ctx *ctx, const uint64_t *addresses, const uint64_t *pre_values, const uint64_t *post_values, size_t cycles,
                              const jolt_table *inc, const jolt_table *val_init, const jolt_fr_t *tau_low, const jolt_fr_t *gamma,
                              jolt_rw_matrix **out);
/* The same member over access columns already resident in HBM (three JOLT_INT_U64 jolt_ints of `cycles` entries, uploaded once per trace):
 * no host pass over the columns and no upload per proof. */
int32_t jolt_rw_matrix_create_resident(jolt_ctx *ctx, const jolt_ints *addresses, const jolt_ints *pre_values, const jolt_ints *post_values,
                                       const jolt_table *inc, const jolt_table *val_init, const jolt_fr_t *tau_low, const jolt_fr_t *gamma,
                                       jolt_rw_matrix **out);

/* Registers read/write checking (stage 4) -- SURVEY.md section 8(f) row 4.  Replaces the sparse cycle-major matrix and the round messages of
 * OptimizedRegistersReadWrite (crates/jolt-kernels/src/optimized/registers_read_write/{mod.rs:79-402, sparse.rs, rows.rs}): summand
 *   eq(r_cycle, j) * ( rd_wa * (rd_inc + val) + gamma * rs1_ra * val + gamma^2 * rs2_ra * val )(k, j)   (reference/registers_read_write.rs:3-10)
 * over (register || cycle), bound low-to-high, the log T cycle variables first; <= 3 cells per cycle (RegisterCycleRow::entries), the
 * gamma-combined read coefficient and the write coefficient as two columns of the same sparse matrix as jolt_rw_matrix, K-sized dense
 * arrays on the host for the log K address rounds.  All inputs are resident: `regs` holds the hot-index columns rs1, rs2, rd (polys 0, 1, 2;
 * k = 2^REGISTER_ADDRESS_BITS), the value columns are JOLT_INT_U64 jolt_ints, `inc` is RdInc (copied).
 *   prove_round: cycle rounds return (q(0), leading coefficient) in evals_out[0..1] and aux_out = {current_scalar, r_cycle[current_index - 1], 0}
 *     (the caller completes the cubic with gruen_poly_deg_3); address rounds return s(0), s(1), s(2), s(3) in evals_out[0..3]
 *     (UnivariatePoly::from_evals).  finish / destroy / len: jolt_rw_matrix_finish / _destroy / _len.
 *   final_values: {registers_val, rd_wa, gamma * rs1_ra + gamma^2 * rs2_ra, rd_inc, bound cycle-eq factor}; the operand claims rs1_ra / rs2_ra
 *     are evaluations of the index columns at the bound point: jolt_onehot_materialize(regs, p, eq(r_address, .)) then jolt_evaluate at r_cycle. */
int32_t jolt_registers_rw_create(jolt_ctx *ctx, const jolt_onehot *regs, const jolt_ints *rs1_val, const jolt_ints *rs2_val, const jolt_ints *rd_pre,
                                 const jolt_ints *rd_post, const jolt_table *inc, const jolt_fr_t *r_cycle, const jolt_fr_t *gamma, jolt_rw_matrix **out);
int32_t jolt_registers_rw_prove_round(jolt_rw_matrix *m, const jolt_fr_t *bind, jolt_fr_t *evals_out /* 4 */, jolt_fr_t *aux_out /* 3, may be NULL */);
int32_t jolt_registers_rw_final_values(jolt_rw_matrix *m, jolt_fr_t *out /* 5 */);
/* test hook: the cells of the cycle phase */
int32_t jolt_registers_rw_download(jolt_rw_matrix *m, uint64_t *rows, uint64_t *cols, jolt_fr_t *val, jolt_fr_t *ra, jolt_fr_t *wa, uint64_t *prev, uint64_t *next);
int32_t jolt_rw_matrix_prove_round(jolt_rw_matrix *m, const jolt_fr_t *bind, jolt_fr_t *evals_out /* 2 */, jolt_fr_t *aux_out /* 3 or NULL */);
int32_t jolt_rw_matrix_finish(jolt_rw_matrix *m, const jolt_fr_t *bind);
int32_t jolt_rw_matrix_final_values(jolt_rw_matrix *m, jolt_fr_t *out /* 4 */);

/* Pushforwards of cycle weights onto a LARGE address domain (bytecode PCs, RAM words; K up to 2^24): the T-scale half of the joint-domain
 * relations whose rounds run over K-sized tables.  Replaces stage_pushforwards of the bytecode read+RAF address phase
 * (crates/jolt-kernels/src/optimized/bytecode_read_raf.rs:152-237: F_s(k) = sum_{j: pc(j) = k} eq(r_cycle_s, j) for the five stages in one
 * trace walk) and RamAccessColumns::fold_cycles (optimized/ram_trace.rs:150-162, used by optimized/ram_raf_evaluation.rs:44-48).
 *   jolt_key_index_create: sorts the rows of a resident key column (JOLT_INT_U64, one key per cycle; a key >= K is a cold cycle and
 *     contributes nothing: NO_ACCESS, unmapped PCs) by key, once per trace column -- the reference shares the same scan through its
 *     ProofSession (PcRow::shared :92-150, RamAccessColumns::shared).
 *   jolt_key_index_pushforward: out[s][k] = sum_{j: key(j) = k} weights[s][j] for n_weights <= 8 tables of `cycles` entries at once; new
 *     tables of K entries (the caller frees them).
 *   jolt_key_index_last_value: out[k] = values[latest cycle with key k] as a field element, init[k] for a key that never occurs: the final
 *     state of a memory that is only ever overwritten (the ram_val_final column of the RAM output check, optimized/ram_output_check.rs:91). */
typedef struct jolt_key_index jolt_key_index;
int32_t jolt_key_index_create(jolt_ctx *ctx, const jolt_ints *keys, uint64_t k, jolt_key_index **out);
int32_t jolt_key_index_size(const jolt_key_index *index, size_t *cycles, uint64_t *k, uint32_t *items);
int32_t jolt_key_index_pushforward(jolt_ctx *ctx, const jolt_key_index *index, jolt_table *const *weights, size_t n_weights, jolt_table **out);
int32_t jolt_key_index_last_value(jolt_ctx *ctx, const jolt_key_index *index, const jolt_ints *values, const jolt_table *init, jolt_table **out);
int32_t jolt_key_index_destroy(jolt_ctx *ctx, jolt_key_index *index);

/* The hypercube-sharded form of both matrices (one process per GPU; the reference has no multi-GPU code: this is north_star's "the 2^n boolean hypercube shards
 * across the GPUs" for rw_matrix.rs / registers_read_write/sparse.rs).  Cycles are dealt to the ranks in contiguous blocks and bind low to high, so rank g runs the
 * first log T_local cycle rounds on a LOCAL matrix over its block (the constructors above with the low log T_local coordinates of the cycle point; its round sums,
 * scaled by eq(w_hi, g), add over the ranks).  jolt_rw_matrix_hold_row (before the rounds) keeps the single row those rounds leave in cycle-major form;
 * jolt_rw_matrix_bind ingests the last local challenge; jolt_rw_matrix_export_row reads the row out (cells in column order, raw checkpoints, the bound increment, the
 * bound eq factor).  The rows of all ranks stacked in rank order are the matrix of the remaining log G cycle variables: jolt_rw_matrix_create_merged builds it on
 * every rank (w = the log_rows HIGH coordinates, inc = the ranks' bound increments in rank order) and the ordinary prove_round / finish / final_values continue. */
int32_t jolt_rw_matrix_hold_row(jolt_rw_matrix *m);
int32_t jolt_rw_matrix_bind(jolt_rw_matrix *m, const jolt_fr_t *bind);
int32_t jolt_rw_matrix_export_row(jolt_rw_matrix *m, size_t cap, uint64_t *cols, uint64_t *prev, uint64_t *next, jolt_fr_t *val, jolt_fr_t *ra, jolt_fr_t *wa /* registers */,
                                  jolt_fr_t *inc_out, jolt_fr_t *scalar_out, size_t *n_out);
int32_t jolt_rw_matrix_create_merged(jolt_ctx *ctx, int32_t registers, size_t log_rows, size_t log_k, size_t n, const uint64_t *rows, const uint64_t *cols,
                                     const uint64_t *prev, const uint64_t *next, const jolt_fr_t *val, const jolt_fr_t *ra, const jolt_fr_t *wa, const jolt_fr_t *inc,
                                     const jolt_table *val_init, const jolt_fr_t *w, const jolt_fr_t *scalar, const jolt_fr_t *gamma, jolt_rw_matrix **out);
int32_t jolt_rw_matrix_len(const jolt_rw_matrix *m, size_t *entries);
int32_t jolt_rw_matrix_download(jolt_rw_matrix *m, uint64_t *rows, uint64_t *cols, jolt_fr_t *val, jolt_fr_t *ra, jolt_fr_t *prev, jolt_fr_t *next);
int32_t jolt_rw_matrix_destroy(jolt_rw_matrix *m);

/* Multi-GPU data path (one process per GPU).  The collectives are RCCL calls on the context's stream;
 * librccl.so.1 is resolved with dlopen at first use (`rccl_path` may name it explicitly, NULL = the copy already mapped into
 * the process / the default search path).  Rank 0 draws the id, the launcher broadcasts its 128 bytes (torch.distributed
 * in this repo, any side channel in the Rust host), every rank then calls jolt_comm_create (collective).
 * Replaces nothing in the reference -- the reference prover is single-process. */
typedef struct jolt_comm jolt_comm;
int32_t jolt_comm_unique_id(const char *rccl_path, uint8_t out[128]);
int32_t jolt_comm_create(jolt_ctx *ctx, const char *rccl_path, const uint8_t unique_id[128], int32_t rank, int32_t world, jolt_comm **out);
int32_t jolt_comm_destroy(jolt_comm *comm);
int32_t jolt_comm_world(const jolt_comm *comm, int32_t *rank, int32_t *world);
/* gathered = world blocks of `bytes` in rank order.  _host: small host payload (per-round partial sums), synchronous;
 * _device / _table: device buffers, asynchronous on the context stream. */
int32_t jolt_comm_all_gather_host(jolt_comm *comm, const void *local, size_t bytes, void *gathered);
int32_t jolt_comm_all_gather_device(jolt_comm *comm, const void *d_local, size_t bytes, void *d_gathered);
int32_t jolt_comm_all_gather_table(jolt_comm *comm, const jolt_table *local, size_t n, jolt_table *gathered);
/* A jolt_gather_fn for jolt_host_batch_run with user = jolt_comm*. */
int32_t jolt_comm_gather_round_sums(void *user, const jolt_fr_t *local, size_t count, jolt_fr_t *gathered);
/* The same exchange between the ranks of ONE node through POSIX shared memory (host memory only; ~1 us instead of an RCCL
 * all-gather on the critical path of every sharded round).  Collective: rank 0 creates the segment `name`
 * ("/..."), the others attach; JOLT_ERR_UNSUPPORTED when the segment cannot be created / mapped (the launcher then keeps the
 * RCCL exchange on every rank).  max_bytes bounds one rank's payload. */
typedef struct jolt_shm jolt_shm;
int32_t jolt_shm_create(const char *name, int32_t rank, int32_t world, size_t max_bytes, jolt_shm **out);
/* The same with a per-run nonce (non-zero; the launcher draws it on rank 0 and distributes it with the name): an attaching rank
 * accepts only the segment rank 0 initialised with this value, never a stale one a crashed run left under the same name. */
int32_t jolt_shm_create_nonce(const char *name, uint64_t nonce, int32_t rank, int32_t world, size_t max_bytes, jolt_shm **out);
int32_t jolt_shm_destroy(jolt_shm *shm);
int32_t jolt_shm_all_gather(jolt_shm *shm, const void *local, size_t bytes, void *gathered);
/* A jolt_gather_fn for jolt_host_batch_run with user = jolt_shm*. */
int32_t jolt_shm_gather_round_sums(void *user, const jolt_fr_t *local, size_t count, jolt_fr_t *gathered);
/* Hand-over to the redundant tail: pack the current tables (`entries` values each) of several members table-major into dst;
 * after the all-gather, dst[t][r*entries + j] = gathered[r][t][j] (rank = top variables). */
int32_t jolt_round_group_pack_tables(jolt_ctx *ctx, jolt_member *const *members, size_t n_members, size_t entries, jolt_table *dst);
int32_t jolt_tail_interleave(jolt_ctx *ctx, const jolt_table *gathered, size_t world, size_t n_tables, size_t entries, jolt_table *dst);
/* The fully bound values of several members with one copy and one synchronisation (concatenated in member order). */
int32_t jolt_round_group_final_values(jolt_ctx *ctx, jolt_member *const *members, size_t n_members, jolt_fr_t *out, size_t capacity);

/* HyperKZGScheme::commit / open (crates/jolt-hyperkzg/src/scheme.rs:122-158,302-325, kzg.rs:69-126) over the device
 * kernels with the same test transcript.  com: ell-1 points, w: 3 points, v: 3*ell, challenges: {r, q, d_0}. */
int32_t jolt_host_hyperkzg_commit(jolt_ctx *ctx, const jolt_srs *srs, const jolt_table *evals, jolt_g1_t *out);
int32_t jolt_host_hyperkzg_open(jolt_ctx *ctx, const jolt_srs *srs, const jolt_table *evals, const jolt_fr_t *point, size_t ell,
                                uint64_t transcript_label, jolt_g1_t *com, jolt_g1_t *w, jolt_fr_t *v, jolt_fr_t *challenges_out);
/* The combination that turns the commitments of ONE polynomial against shifted bases into the three witness commitments of kzg_open_batch (kzg.rs:108-116), as the
 * opening runs it after its three bucket passes over one digit sort; host code, no GPU.  With u = r^2, B = q (X^2 - u) + alpha X + beta and q = Q3 (X - u) + a:
 * c[k] = commit(X^k Q3) (k = 0, 1, 2), g0 / g1 = the first two SRS points;  w[0], w[1], w[2] = commit of the witness polynomial at r, -r, r^2. */
int32_t jolt_host_hyperkzg_witness_triple(const jolt_g1_t *c /* 3 */, const jolt_g1_t *g0, const jolt_g1_t *g1, const jolt_fr_t *r, const jolt_fr_t *a,
                                          const jolt_fr_t *alpha, jolt_g1_t *w /* 3 */);

/* The same opening under the CALLER's Fiat-Shamir transcript -- CommitmentScheme::open(poly, point, eval, setup, hint, transcript) (crates/jolt-openings/src/
 * schemes.rs:66-72; impl crates/jolt-hyperkzg/src/scheme.rs:314-325) with the polynomial resident in HBM.  `fn` is called three times per opening, in order:
 *   phase 0: points = the ell - 1 level commitments (scheme.rs:148-152)        -> challenge r
 *   phase 1: values = v[t][j], 3 * ell field elements row-major (kzg.rs:88-95) -> challenge q
 *   phase 2: points = the three witness commitments (kzg.rs:118-124)            -> challenge d_0
 * it absorbs them (transcript.append per element, in order) and returns the challenge; a non-zero return aborts the opening with that status. */
typedef int32_t (*jolt_open_transcript_fn)(void *user, int32_t phase, const jolt_g1_t *points, size_t n_points, const jolt_fr_t *values, size_t n_values,
                                           jolt_fr_t *challenge_out);
int32_t jolt_host_hyperkzg_open_with_transcript(jolt_ctx *ctx, const jolt_srs *srs, const jolt_table *evals, const jolt_fr_t *point, size_t ell,
                                                jolt_open_transcript_fn fn, void *user, jolt_g1_t *com, jolt_g1_t *w, jolt_fr_t *v, jolt_fr_t *challenges_out);
/* ... and with its first n_known level commitments supplied by the caller (HyperKZGScheme::open commits every folded polynomial by MSM, scheme.rs:141-145; for the
 * joint polynomial of one-hot and dense columns the first folds' commitments follow by linearity from jolt_grid_commit_onehot_classes): known_levels[i] is absorbed and
 * returned as com[i], the MSMs of those levels are skipped.  fn == NULL: the library's test transcript with transcript_label.  Single-process opening only. */
int32_t jolt_host_hyperkzg_open_with_levels(jolt_ctx *ctx, const jolt_srs *srs, const jolt_table *evals, const jolt_fr_t *point, size_t ell, uint64_t transcript_label,
                                            jolt_open_transcript_fn fn, void *user, const jolt_g1_t *known_levels, size_t n_known, jolt_g1_t *com, jolt_g1_t *w,
                                            jolt_fr_t *v, jolt_fr_t *challenges_out);

/* Term-range pieces of a commitment / opening sharded over the ranks of a node (the reference is single
 * process): an MSM of n terms against srs[base_offset .. base_offset + n) with the scalars scalars[scalar_offset ..]; the partial
 * one-hot commitments over cycles [cycle_lo, cycle_hi); and HyperKZGScheme::open with EVERY MSM split by term range over `world`
 * ranks -- each rank holds the polynomial and the bases, multiplies terms [n*rank/world, n*(rank+1)/world), the partial points are
 * all-gathered through `gather` (a jolt_gather_fn moving 32-byte words: jolt_comm_gather_round_sums, jolt_shm_gather_round_sums)
 * and added in rank order, so every rank absorbs the same commitments and returns the same proof as jolt_host_hyperkzg_open. */
int32_t jolt_msm_g1_table_range(jolt_ctx *ctx, const jolt_srs *srs, size_t base_offset, const jolt_table *scalars, size_t scalar_offset,
                                size_t n, jolt_g1_t *out);
/* One window of a STREAMED commitment: StreamingCommitment::{feed, feed_u64, feed_i128, feed_i128_rows_with} for a KZG-type scheme
 * (crates/jolt-openings/src/schemes.rs:167-222; the callers: crates/jolt-kernels/src/reference/commitment.rs:86-121, optimized/commitment.rs:317-352).  The
 * polynomial arrives in coefficient order as host slices; out = acc + sum_{i<n} values[i] * srs[base_offset + i] (acc == NULL: the identity), values being n field
 * elements (kind JOLT_SCALAR_FR) or machine integers promoted by Ring::from_u64 / from_i64 / from_i128 (kind JOLT_INT_*).  Stateless: the caller's PartialCommitment is
 * the pair (point, next coefficient index).  base_offset + n beyond the SRS is JOLT_ERR_SRS_TOO_SMALL. */
enum { JOLT_SCALAR_FR = 3 };
int32_t jolt_msm_g1_window(jolt_ctx *ctx, const jolt_srs *srs, size_t base_offset, int32_t kind, const void *host, size_t n, const jolt_g1_t *acc, jolt_g1_t *out);
int32_t jolt_grid_commit_onehot_range(jolt_ctx *ctx, const jolt_srs *srs, const jolt_onehot *source, size_t cycle_lo, size_t cycle_hi,
                                      jolt_g1_t *out /* n_polys */);
/* out[c * n_polys + p] = sum over the cycles j = c (mod 2^shift) of srs[(hot_p(j) * T + j) >> shift]: the commitments of the 2^shift residue-class parts of every column
 * on the grid of a polynomial folded `shift` times low to high (shift <= 4, T a power of two).  com(fold of the joint polynomial) is a linear combination of them:
 * for shift = 1 and the fold variable x, sum_p s_p ((1 - x) out[0][p] + x out[1][p]) + com(the dense columns' fold). */
int32_t jolt_grid_commit_onehot_classes(jolt_ctx *ctx, const jolt_srs *srs, const jolt_onehot *source, uint32_t shift, jolt_g1_t *out);
int32_t jolt_host_hyperkzg_open_sharded(jolt_ctx *ctx, const jolt_srs *srs, const jolt_table *evals, const jolt_fr_t *point, size_t ell,
                                        uint64_t transcript_label, int32_t rank, int32_t world, jolt_gather_fn gather, void *user,
                                        jolt_g1_t *com, jolt_g1_t *w, jolt_fr_t *v, jolt_fr_t *challenges_out);
/* The BLOCK-CYCLIC term assignment, the one that keeps the fixed-base window tables at any world size: term i
 * of every MSM belongs to rank (i / block) % world, and a rank's jolt_srs holds exactly the bases of its terms, compacted in index
 * order (count_global / world points; upload them with jolt_srs_upload_g1, or generate them from a test secret here).  The terms a rank
 * owns of any prefix [0, n) are then a prefix of its compact SRS, so jolt_srs_precompute_windows over the compact SRS serves every
 * level of an opening.  With block = the rank's cycle count T, a rank's compact SRS is the commitment grid of ITS cycles (position
 * k*T + j), so its share of a commitment is jolt_grid_commit_onehot / jolt_msm_g1_table_range over local columns.
 * jolt_msm_g1_table_blocks: the rank's share of sum_{i<n} scalars[i]*SRS[i] (the shares of all ranks add up to the MSM);
 * jolt_host_hyperkzg_open_sharded_blocks: jolt_host_hyperkzg_open_sharded with this assignment. */
/* how many of the terms [0, n) rank owns = the length of its compact prefix (host only, no GPU) */
int32_t jolt_host_owned_terms(size_t n, size_t block, int32_t rank, int32_t world, size_t *out);
int32_t jolt_srs_setup_from_secret_blocks(jolt_ctx *ctx, const jolt_fr_t *beta, size_t count_global, const jolt_g1_t *g1, size_t block,
                                          int32_t rank, int32_t world, jolt_srs **out);
int32_t jolt_msm_g1_table_blocks(jolt_ctx *ctx, const jolt_srs *srs, const jolt_table *scalars, size_t n, size_t block, int32_t rank,
                                 int32_t world, jolt_g1_t *out);
int32_t jolt_host_hyperkzg_open_sharded_blocks(jolt_ctx *ctx, const jolt_srs *srs, const jolt_table *evals, const jolt_fr_t *point,
                                               size_t ell, uint64_t transcript_label, int32_t rank, int32_t world, size_t block,
                                               jolt_gather_fn gather, void *user, jolt_g1_t *com, jolt_g1_t *w, jolt_fr_t *v,
                                               jolt_fr_t *challenges_out);
/* The SUBTREE assignment (world = 2^gamma ranks): the gamma bits below the leading one of an index name its owner
 * (indices below `world`: owner = the index, slot 0; otherwise slot = the index with those bits removed).  Like the block-cyclic one it
 * keeps every prefix of the indices a prefix of every rank's compact arrays -- one compact SRS and one set of window tables per rank
 * -- and it is also closed under LowToHigh folding (slots 2c, 2c+1 of a level fold into slot c of the next), so the POLYNOMIAL of an
 * opening is sharded too: jolt_host_hyperkzg_open_subtree takes the rank's compact array of the evaluations (2^ell / world
 * coefficients: jolt_grid_joint_polynomial_subtree builds it for the commitment grid; jolt_host_subtree_term_index gives the index
 * of a slot for any other source) and the rank's compact SRS, runs folds / RLC / Horner passes / quotient scans / MSMs on 1 / world
 * of the data, exchanges O(ell) field elements and O(ell) points through `gather`, and returns on every rank the proof
 * jolt_host_hyperkzg_open returns for the whole polynomial (world >= 2, ell > log2 world; one rank: jolt_host_hyperkzg_open).
 * tests/subtree_model.py is the executable specification. */
int32_t jolt_host_subtree_owned_terms(size_t n, int32_t rank, int32_t world, size_t *out);
int32_t jolt_host_subtree_term_index(size_t slot, int32_t rank, int32_t world, size_t *out);
int32_t jolt_srs_setup_from_secret_subtree(jolt_ctx *ctx, const jolt_fr_t *beta, size_t count_global, const jolt_g1_t *g1, int32_t rank,
                                           int32_t world, jolt_srs **out);
int32_t jolt_msm_g1_table_subtree(jolt_ctx *ctx, const jolt_srs *srs, const jolt_table *scalars, size_t n, int32_t rank, int32_t world,
                                  jolt_g1_t *out);
int32_t jolt_grid_joint_polynomial_subtree(jolt_ctx *ctx, const jolt_onehot *const *sources, size_t n_sources,
                                           const jolt_fr_t *onehot_scalars, jolt_table *const *dense, size_t n_dense,
                                           const jolt_fr_t *dense_scalars, uint32_t log_k, int32_t rank, int32_t world, jolt_table **out);
int32_t jolt_host_hyperkzg_open_subtree(jolt_ctx *ctx, const jolt_srs *srs, const jolt_table *evals, const jolt_fr_t *point, size_t ell,
                                        uint64_t transcript_label, int32_t rank, int32_t world, jolt_gather_fn gather, void *user,
                                        jolt_g1_t *com, jolt_g1_t *w, jolt_fr_t *v, jolt_fr_t *challenges_out);

/* The commitment grid's OPENING HINT -- CommitmentScheme::commit returns (Commitment, OpeningHint) (crates/jolt-openings/src/schemes.rs:60-72): what the committer can
 * precompute for the opening from the polynomials and the setup alone.  For the grid's one-hot columns: per fold depth s = 1 .. levels (<= 4) the residue-class sums
 * S_p^(s, c) = sum over the cycles j = c mod 2^s of srs[(hot_p(j) * T + j) >> s] (what jolt_grid_commit_onehot_classes returns to the host), kept on the device.
 * None of it depends on a challenge.  background != 0: enqueued on the context's lowest-priority stream at one wavefront per SIMD and returned at once -- the sums run
 * under the latency-bound legs between the commitment and the opening; 0: on the main stream.  jolt_host_hyperkzg_open_grid turns them into the opening's first level
 * commitments by linearity (same points as scheme.rs:141-145 commits by MSM).  The sources must outlive the hint's sums (jolt_grid_hint_wait, or the opening). */
typedef struct jolt_grid_hint jolt_grid_hint;
int32_t jolt_grid_hint_begin(jolt_ctx *ctx, const jolt_srs *srs, const jolt_onehot *const *sources, size_t n_sources, uint32_t levels, int32_t background,
                             jolt_grid_hint **out);
int32_t jolt_grid_hint_wait(jolt_ctx *ctx, jolt_grid_hint *hint);
int32_t jolt_grid_hint_download(jolt_ctx *ctx, jolt_grid_hint *hint, uint32_t level, jolt_g1_t *out /* 2^level x n_cols, [class][column] */); /* test hook */
int32_t jolt_grid_hint_free(jolt_ctx *ctx, jolt_grid_hint *hint);
/* HyperKZGScheme::open (crates/jolt-hyperkzg/src/scheme.rs:122-158) of the grid's joint polynomial `evals` (jolt_grid_joint_polynomial over the same sources, scalars and
 * dense columns) with the first `levels` level commitments by linearity: one-hot part from the hint, dense part as (T >> s)-term MSMs of the dense columns' folds inside
 * the same MSM pipeline as the remaining levels.  fn == NULL: the library's test transcript under transcript_label.  Proof identical to jolt_host_hyperkzg_open(evals). */
int32_t jolt_host_hyperkzg_open_grid(jolt_ctx *ctx, const jolt_srs *srs, const jolt_table *evals, const jolt_fr_t *point, size_t ell, uint64_t transcript_label,
                                     jolt_open_transcript_fn fn, void *user, const jolt_grid_hint *hint, uint32_t levels, const jolt_fr_t *onehot_scalars,
                                     jolt_table *const *dense, size_t n_dense, const jolt_fr_t *dense_scalars, jolt_g1_t *com, jolt_g1_t *w, jolt_fr_t *v,
                                     jolt_fr_t *challenges_out);

/* HyperKZG VERIFICATION (hyperkzg_verify.hip).  No kernel of its own: a verification is two jolt_dory_products batches -- L and -R as two MSM_G1 items, then
 * e(L, g2) e(-R, beta g2) as one PAIR item against a line table prepared once -- and the host final exponentiation.  Proofs are the opening entries' above:
 * com (ell - 1 points), w (3 points), v (3 * ell values, v[t][j] row-major).
 *
 * HyperKZGVerifierSetup (crates/jolt-hyperkzg/src/types.rs:112-146): g1, g2 and beta * g2.  _create checks canonical coordinates and the curve / twist equation (NO
 * subgroup check, as the Dory entries make none), refuses the identity for any of the three (JOLT_ERR_INVALID_ARG), uploads (g2, beta g2) as one resident G2 vector
 * and prepares their line table once (jolt_dory_g2_prepare_vec).  _from_secret is the G2 side of setup_from_secret (scheme.rs:54-73): beta * g2 by
 * jolt_host_g2_scalar_mul -- the twin of jolt_srs_setup_from_secret for test setups.  The G2 generator is the caller's: which point of the twist a deployment's
 * setup names is a convention no reference vector pins (docs/parity.md).  The object belongs to its context; _free(ctx, NULL) is JOLT_OK. */
typedef struct jolt_hyperkzg_verifier_setup jolt_hyperkzg_verifier_setup;
int32_t jolt_hyperkzg_verifier_setup_create(jolt_ctx *ctx, const jolt_g1_t *g1, const jolt_g2_t *g2, const jolt_g2_t *beta_g2, jolt_hyperkzg_verifier_setup **out);
int32_t jolt_hyperkzg_verifier_setup_from_secret(jolt_ctx *ctx, const jolt_fr_t *beta, const jolt_g1_t *g1, const jolt_g2_t *g2, jolt_hyperkzg_verifier_setup **out);
int32_t jolt_hyperkzg_verifier_setup_points(const jolt_hyperkzg_verifier_setup *vs, jolt_g1_t *g1, jolt_g2_t *g2, jolt_g2_t *beta_g2);
int32_t jolt_hyperkzg_verifier_setup_free(jolt_ctx *ctx, jolt_hyperkzg_verifier_setup *vs);
/* The verifier's scalars in Fr on the host, no GPU.  point: ell coordinates; eval: the claimed evaluation; v: 3 * ell; r, q, d0: the three challenges.
 *   *folding_ok, *failed_level  the folding check of scheme.rs:203-234: 2 r y_next = r (1 - x) (y_pos + y_neg) + x (y_pos - y_neg) per level, y_next = v[2][level + 1]
 *                               and the claimed evaluation at the last level, x = point[ell - 1 - level]; the FIRST failing level (0 when none fails)
 *   l_scalars                   the ell + 4 scalars of L in the order of kzg.rs:182-200: q^j (1 + d_0 + d_1) for the ell commitments (C_0 first), then r, -r d_0,
 *                               r^2 d_1 for the witness points, then -(B(r) + d_0 B(-r) + d_1 B(r^2)) for g1, B(u_t) = sum_j q^j v[t][j]
 *   d_out                       d_0 and d_1 = d_0^2, the scalars of R = w_0 + d_0 w_1 + d_1 w_2 (kzg.rs:204-205)
 * The scalars are written whether or not the folding check holds.  JOLT_ERR_INVALID_ARG: a null pointer, ell = 0 (HyperKZGError::EmptyPoint) or ell > 40, a value
 * that is not canonical; JOLT_ERR_NOT_INVERTIBLE: r = 0 (HyperKZGError::DegenerateChallenge, scheme.rs:194-196). */
int32_t jolt_host_hyperkzg_verify_scalars(size_t ell, const jolt_fr_t *point, const jolt_fr_t *eval, const jolt_fr_t *v /* 3 * ell */, const jolt_fr_t *r,
                                          const jolt_fr_t *q, const jolt_fr_t *d0, int32_t *folding_ok, size_t *failed_level, jolt_fr_t *l_scalars /* ell + 4 */,
                                          jolt_fr_t *d_out /* 2 */);
/* HyperKZGScheme::verify (scheme.rs:162-242) with kzg_verify_batch (kzg.rs:132-210) as one call.  n_commitments = 1 with scalar one is `verify`; n_commitments > 1 is
 * verify after AdditivelyHomomorphic::combine (scheme.rs:346-352) -- C_0 = sum_i s_i commitments[i] is never built: commitment i enters L's MSM with scalar
 * s_i (1 + d_0 + d_1).  In order:
 *   1. every check of the input: canonical values, points on the curve (the identity allowed), ell >= 1 (JOLT_ERR_EMPTY_POINT; ell > 40 or n_commitments > 2^20
 *      JOLT_ERR_UNSUPPORTED: inside these limits the MSM batch below cannot refuse for its size), n_commitments >= 1, a setup of this context.  A refused call absorbs nothing, enqueues nothing and writes nothing;
 *   2. `fn` phase 0 over com gives r -- the same three phases, in the same order, with the same elements as jolt_host_hyperkzg_open_with_transcript calls it, so a
 *      caller's prover callback serves the verifier unchanged; at ell = 1 phase 0 is called with no point, as the opening calls it.  r = 0 is
 *      JOLT_ERR_NOT_INVERTIBLE (DegenerateChallenge);
 *   3. the folding check on the host.  On failure *accepted = 0, *failed_check = 1, *failed_level = the level, and phases 1 and 2 are NOT run (scheme.rs:231-233);
 *   4. phase 1 over v gives q, phase 2 over w gives d_0;
 *   5. ONE jolt_dory_products batch of two MSM_G1 items: L (n_commitments + ell - 1 + 4 terms) and -R (w under -1, -d_0, -d_1);
 *   6. ONE batch of one PAIR item: (L, -R) against the prepared (g2, beta g2);
 *   7. *accepted = 1 only if that product is one after the final exponentiation, otherwise *failed_check = 2.
 * Two synchronisations.  A rejected proof is JOLT_OK; status codes are for malformed input only. */
int32_t jolt_host_hyperkzg_verify_with_transcript(jolt_ctx *ctx, const jolt_hyperkzg_verifier_setup *vs, const jolt_g1_t *commitments,
                                                  const jolt_fr_t *commitment_scalars, size_t n_commitments, const jolt_fr_t *point, size_t ell, const jolt_fr_t *eval,
                                                  const jolt_g1_t *com, const jolt_g1_t *w, const jolt_fr_t *v, jolt_open_transcript_fn fn, void *user,
                                                  int32_t *accepted, int32_t *failed_check, size_t *failed_level);
/* The same under one of the library's engines.  The opening's own transcript is a jolt_host_transcript's engine and both sides absorb through one routine
 * (hyperkzg_transcript.hpp): a fresh jolt_host_transcript_create(label) draws the challenges jolt_host_hyperkzg_open(..., label) reports in challenges_out. */
int32_t jolt_host_hyperkzg_verify(jolt_ctx *ctx, const jolt_hyperkzg_verifier_setup *vs, const jolt_g1_t *commitments, const jolt_fr_t *commitment_scalars,
                                  size_t n_commitments, const jolt_fr_t *point, size_t ell, const jolt_fr_t *eval, const jolt_g1_t *com, const jolt_g1_t *w,
                                  const jolt_fr_t *v, jolt_host_transcript *t, int32_t *accepted, int32_t *failed_check, size_t *failed_level);
/* HomomorphicBatch::<HyperKZGScheme>::prove_batch (crates/jolt-openings/src/schemes.rs:487-524) over the commitment grid's columns:
 *   1. absorbs the statement (jolt_host_opening_statement_absorb): gamma's powers; claim i is column i in jolt_grid_evaluate_columns' order (one-hot columns source
 *      by source, then dense); *joint_eval_out = sum_i gamma^i evaluations[i];
 *   2. deals the powers to onehot_scalars and dense_scalars and builds the joint polynomial (jolt_grid_joint_polynomial);
 *   3. runs the body of jolt_host_hyperkzg_open_grid under t.  The commit-time hint is a function of the columns alone and serves any scalars; hint = NULL or
 *      levels = 0: every level commitment by MSM.  After the folds the last level (two entries, one small read-back) gives the joint polynomial's value at the point:
 *      a statement that does not hold is JOLT_ERR_ROUND_CHECK before the transcript absorbs a level commitment (as jolt_host_dory_prove_batch refuses one);
 *   4. absorbs the closing claim (jolt_host_opening_claim_absorb).
 * Checked before the transcript absorbs anything: the arguments as jolt_grid_joint_polynomial and jolt_grid_evaluate_columns check them (contexts, limits, one cycle
 * count), n_claims = the number of columns, n_point = log_k + log2(T) >= 1, canonical values, an SRS of at least 2^n_point bases (JOLT_ERR_SRS_TOO_SMALL), and a hint
 * that is read (levels > 0, one-hot columns) made on this grid: its k = 2^log_k, its cycle count and its column count.  What the opening itself can still refuse comes
 * AFTER the statement has been absorbed: a device error, an allocation that fails, a failure of the hint's background sums.  A hint made over other sources of the same
 * shape is not detected: it yields a proof the verifier rejects.  challenges_out ({r, q, d_0}) may be NULL. */
int32_t jolt_host_hyperkzg_prove_batch(jolt_ctx *ctx, const jolt_srs *srs, const jolt_onehot *const *sources, size_t n_sources, jolt_table *const *dense,
                                       size_t n_dense, uint32_t log_k, const jolt_fr_t *evaluations, size_t n_claims, const jolt_fr_t *point, size_t n_point,
                                       const jolt_grid_hint *hint, uint32_t levels, jolt_host_transcript *t, jolt_g1_t *com, jolt_g1_t *w, jolt_fr_t *v,
                                       jolt_fr_t *challenges_out, jolt_fr_t *joint_eval_out);
/* HomomorphicBatch::<HyperKZGScheme>::verify_batch (schemes.rs:526-551): after jolt_host_hyperkzg_verify's checks the statement is absorbed (gamma's powers), the
 * joint evaluation formed, and the verifier above runs with the powers as commitment scalars.  The closing claim is absorbed ONLY AFTER AN ACCEPTED PROOF: the
 * reference returns early through `?` (schemes.rs:541-549).  jolt_host_dory_verify_batch absorbs it on both outcomes; the two entries differ there.  After an accepted
 * proof the transcript ends in the state jolt_host_hyperkzg_prove_batch leaves.  n_claims = 0 is JOLT_ERR_INVALID_ARG. */
int32_t jolt_host_hyperkzg_verify_batch(jolt_ctx *ctx, const jolt_hyperkzg_verifier_setup *vs, const jolt_g1_t *commitments, const jolt_fr_t *evaluations,
                                        size_t n_claims, const jolt_fr_t *point, size_t n_point, const jolt_g1_t *com, const jolt_g1_t *w, const jolt_fr_t *v,
                                        jolt_host_transcript *t, int32_t *accepted, int32_t *failed_check, size_t *failed_level, jolt_fr_t *joint_eval_out);

/* ------------------------------------------------------------------------------------------------------------
 * Stage operators as ProveRounds objects -- one per backend slot (crates/jolt-kernels/src/backend.rs:126-171).
 *
 * A slot is a PrepareKernel<F, R> whose prepare(..) returns Box<dyn SumcheckKernel<F, Relation = R>> (backend.rs:98-111, kernel.rs:72-126):
 * ProveRounds (crates/jolt-sumcheck/src/prover.rs:52-72) + output_claims.  jolt_stage_<operator>_create IS that prepare: every T-scale pass that
 * depends on no round challenge runs there, over inputs that are resident in HBM (borrowed: they must outlive the operator).  The object then
 * follows the fused contract (prover.rs:45-51): prove_round(bind = the PREVIOUS round's challenge or NULL in the first active round, round,
 * previous_claim) returns the round message as UnivariatePoly coefficients c_0 .. c_{n-1} (n <= degree + 1; s(0) + s(1) = previous_claim),
 * finish_rounds(bind) applies the last challenge, output_claims are SumcheckKernel::output_claims in the order each constructor documents.
 * Errors as everywhere in this header; a message that fails its own round check is JOLT_ERR_ROUND_CHECK.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct jolt_stage_op jolt_stage_op;
int32_t jolt_stage_op_num_rounds(const jolt_stage_op *op, size_t *rounds);                  /* ProveRounds::num_rounds */
int32_t jolt_stage_op_degree(const jolt_stage_op *op, size_t *degree);                      /* the largest degree of a round message */
int32_t jolt_stage_op_input_claim(jolt_stage_op *op, jolt_fr_t *claim);                     /* test / bench convenience: a prover holds it from the earlier stages */
int32_t jolt_stage_op_prove_round(jolt_stage_op *op, const jolt_fr_t *bind, size_t round, const jolt_fr_t *previous_claim, jolt_fr_t *coeffs_out, size_t cap,
                                  size_t *n_coeffs);                                        /* ProveRounds::prove_round (prover.rs:57-66) */
int32_t jolt_stage_op_finish_rounds(jolt_stage_op *op, const jolt_fr_t *bind);              /* ProveRounds::finish_rounds (prover.rs:68-71) */
int32_t jolt_stage_op_output_claims(jolt_stage_op *op, jolt_fr_t *out, size_t cap, size_t *n); /* SumcheckKernel::output_claims (kernel.rs:86-92) */
/* Intermediate values an operator keeps on the host for parity tests, by name: "masses" (pushforwards: n_polys x K), "scan_raf" / "scan_suffix" (the 16 read-RAF
 * phase scans), "v_tables", "table_values", "raf_values", "cycle_claim".  out == NULL asks for the count. */
int32_t jolt_stage_op_kept(const jolt_stage_op *op, const char *key, jolt_fr_t *out, size_t cap, size_t *n);
/* Rounds [first, first + n) of `parent` as an operator of its own (the parent stays alive and owns the state): a caller can put the phases of one kernel under
 * different transcripts or drivers; a window's last challenge is handed to the parent with the next window's first round. */
int32_t jolt_stage_op_window(jolt_stage_op *parent, size_t first, size_t n, jolt_stage_op **out);
int32_t jolt_stage_op_destroy(jolt_stage_op *op);

/* UniskipKernel (crates/jolt-kernels/src/uniskip.rs:28-54) of Spartan outer (n_streams = 2) / product (n_streams = 1): the extended-node sums t1 of the uni-skip
 * first round off the integer columns (jolt_r1cs_uniskip_sums_small) against eq(tau, .) expanded here.  tau: n_tau coordinates (cycle variables, then the stream). */
int32_t jolt_stage_spartan_uniskip_sums(jolt_ctx *ctx, const jolt_ints *const *cols, size_t n_cols, uint32_t n_streams, const jolt_fr_t *tau, size_t n_tau,
                                        const int64_t *a_weights, const int64_t *b_weights, size_t n_nodes, jolt_fr_t *sums_out);
/* spartan_outer / spartan_product remainder (optimized/spartan_outer.rs:236-300,780-850; spartan_product.rs:321-437): Az / Bz at the uni-skip challenge
 * (field weights [stream][1 + n_cols]), the split-eq product member over them, n_tau rounds of degree 3.  output_claims: the n_cols claimed inputs at the cycle point. */
int32_t jolt_stage_spartan_remainder_create(jolt_ctx *ctx, const jolt_ints *const *cols, size_t n_cols, uint32_t n_streams, const jolt_fr_t *a_weights,
                                            const jolt_fr_t *b_weights, const jolt_fr_t *tau, size_t n_tau, const jolt_fr_t *scale, jolt_stage_op **out);
/* The remainder of a row system at the DRAWN uni-skip challenge r0: column weights fa[s][v] = sum_i L_i(r0) A_{s,i}[v] (constants in column 0), fb likewise
 * (spartan_outer_row_weights, crates/jolt-r1cs/src/constraints/jolt.rs:141-170; weighted_columns + public_column_contributions, reference/spartan_outer.rs:239-262),
 * the scale LK(tau_high, r0) (:240-244), then jolt_r1cs_materialize_small and the split-eq product member: an ordinary operator with the output claims of
 * jolt_stage_spartan_remainder_create.  tau: the n_tau coordinates of the rounds (cycle variables, then the stream).  jolt_stage_op_kept: "a_weights", "b_weights", "scale". */
int32_t jolt_stage_spartan_remainder_rows_create(jolt_ctx *ctx, const jolt_r1cs_rows *rows, const jolt_ints *const *cols, size_t n_cols, const jolt_fr_t *tau, size_t n_tau,
                                                 const jolt_fr_t *tau_high, const jolt_fr_t *r0, jolt_stage_op **out);
/* ram_read_write (optimized/ram_read_write.rs:58-330): RamAccessColumns (u64 jolt_ints of T entries), RamInc (i64, T), the initial memory (u64, K); log T cycle rounds
 * (cubic, gruen_poly_deg_3) then log K address rounds (quadratic).  output_claims: {ra, val, inc, bound cycle-eq factor}. */
int32_t jolt_stage_ram_read_write_create(jolt_ctx *ctx, const jolt_ints *addresses, const jolt_ints *pre_values, const jolt_ints *post_values, const jolt_ints *inc,
                                         const jolt_ints *val_init, const jolt_fr_t *tau_low, const jolt_fr_t *gamma, jolt_stage_op **out);
/* registers_read_write (optimized/registers_read_write/mod.rs:79-402): `regs` = the hot-index columns rs1, rs2, rd (K = 128), the value columns, RdInc (i128).
 * output_claims: {registers_val, rd_wa, gamma rs1_ra + gamma^2 rs2_ra, rd_inc, bound cycle-eq factor, rs1_ra, rs2_ra}. */
int32_t jolt_stage_registers_read_write_create(jolt_ctx *ctx, const jolt_onehot *regs, const jolt_ints *rs1_val, const jolt_ints *rs2_val, const jolt_ints *rd_pre,
                                               const jolt_ints *rd_post, const jolt_ints *inc, const jolt_fr_t *r_cycle, const jolt_fr_t *gamma, jolt_stage_op **out);
/* booleanity_address (optimized/booleanity.rs:152-427): the pushforward masses of all RA columns against eq(reference_cycle, .) (T-scale, here), then log K rounds
 * of degree 3 over K-entry tables.  Input claim zero.  output_claims: {the phase's intermediate claim}. */
int32_t jolt_stage_booleanity_address_create(jolt_ctx *ctx, const jolt_onehot *cols, const jolt_fr_t *reference_cycle, size_t n_cycle, const jolt_fr_t *reference_address,
                                             const jolt_fr_t *gamma, jolt_stage_op **out);
/* booleanity_cycle (optimized/booleanity.rs:436-690, stage 6b): eq(reference_cycle, j) eq(r_address, reference_address) sum_i (H_i(j)^2 - gamma^i H_i(j)) over the lazily bound
 * RA columns, H_i(j) = gamma^i eq(r_address, hot_i(j)); r_address = the address phase's bound point (log K coordinates, most significant first).  log T rounds of degree 3
 * (gruen_poly_deg_3 of the member's two sums); the input claim is the address phase's intermediate claim (the caller's; no input_claim helper); output claims: the n_polys bound columns unscaled, ra_i(r_address, r_cycle). */
int32_t jolt_stage_booleanity_cycle_create(jolt_ctx *ctx, const jolt_onehot *cols, const jolt_fr_t *r_address, const jolt_fr_t *reference_address, const jolt_fr_t *reference_cycle,
                                           size_t n_cycle, const jolt_fr_t *gamma, jolt_stage_op **out);
/* hamming_weight_claim_reduction (optimized/hamming_weight_claim_reduction.rs:83-300): virtualization_points = n_polys x log K.  output_claims: the bound G_i. */
int32_t jolt_stage_hamming_weight_create(jolt_ctx *ctx, const jolt_onehot *cols, const jolt_fr_t *r_cycle, size_t n_cycle, const jolt_fr_t *r_address,
                                         const jolt_fr_t *virtualization_points, const jolt_fr_t *gamma, jolt_stage_op **out);
/* instruction_read_raf (optimized/instruction_read_raf.rs:736-1456), ONE kernel of 128 + log T rounds: 16 address phases (condensation + scans on the device at each
 * phase's first round, 8 quadratic rounds over 256-entry polynomials on the host) and the cycle rounds over combined * prod ra_i (degree ra_count + 2).
 * claim_columns: the packed flag facts as four K = 16 hot-index columns (tables 0..15, 16..31, 32..41; RAF rows on 0).
 * output_claims: {lookup_table_flags of the present tables, instruction_raf_flag, the ra_count bound ra_i}. */
int32_t jolt_stage_instruction_read_raf_create(jolt_ctx *ctx, jolt_read_raf *rows, const jolt_onehot *claim_columns, const jolt_fr_t *r_reduction, size_t n_vars,
                                               const jolt_fr_t *gamma, const uint8_t *table_present /* 42 */, uint32_t ra_count, jolt_stage_op **out);
/* bytecode_read_raf_address (optimized/bytecode_read_raf.rs:152-437): the five stage pushforwards onto the bytecode domain in one walk over the PC index, log K
 * rounds of degree 2 over 13 K-sized tables.  output_claims: {the 13 bound tables (F_0..4, V_0..4, Int, entry_trace, entry_expected), the intermediate claim}.
 * bytecode_read_raf_cycle (:440-690) is prepared from the finished address operator (its parked eq tables are consumed): log T rounds of C * prod ra_i;
 * output_claims: the bound ra_i. */
int32_t jolt_stage_bytecode_read_raf_address_create(jolt_ctx *ctx, const jolt_key_index *pc_index, const jolt_fr_t *stage_points /* 5 x n_vars */, size_t n_vars,
                                                    const jolt_fr_t *stage_values /* 5 x K */, const jolt_fr_t *gamma, uint64_t first_pc, uint64_t entry_index,
                                                    jolt_stage_op **out);
int32_t jolt_stage_bytecode_read_raf_cycle_create(jolt_ctx *ctx, jolt_stage_op *address, const jolt_onehot *pc_chunks, uint32_t chunk_bits, jolt_stage_op **out);
/* ram_raf_evaluation (optimized/ram_raf_evaluation.rs:17-62): log K rounds of ra_folded * unmap.  output_claims: {ra_folded, unmap} bound. */
int32_t jolt_stage_ram_raf_evaluation_create(jolt_ctx *ctx, const jolt_key_index *ram_index, const jolt_fr_t *tau_low, size_t n_vars, uint64_t lowest_address,
                                             jolt_stage_op **out);
/* ram_output_check (optimized/ram_output_check.rs:50-215): val_final from the access columns (T-scale, here), log K rounds of degree 3.
 * output_claims: {val_final at the bound address point}. */
int32_t jolt_stage_ram_output_check_create(jolt_ctx *ctx, const jolt_key_index *ram_index, const jolt_ints *post_values, const uint64_t *val_init /* K */,
                                           const uint64_t *val_io /* K */, uint64_t io_lo, uint64_t io_len, const jolt_fr_t *r_address, jolt_stage_op **out);
/* A device jolt_member as a stage operator: what a slot's prepare returns for a relation that is ONE batch member (Box<dyn SumcheckKernel>, crates/jolt-kernels/src/kernel.rs:72-126;
 * reference tier crates/jolt-kernels/src/reference/naive.rs:53-377) -- every member kind of this header (expr / lc, split-eq lc / product / uniform, lazily bound RA columns,
 * compact-scalar columns).  rounds and degree (the message degree) are the member's, input_claim is jolt_member_input_claim, output_claims are jolt_member_final_values: the
 * bound tables in table order, then the bound eq scalar of a member that carries a split eq.  `member` must belong to `ctx` (JOLT_ERR_INVALID_ARG otherwise) and may be
 * one operator of a batch only once.
 * Ownership: by default the operator BORROWS the member -- destroy the operator first, then the member; after jolt_stage_op_destroy the member is as the rounds left it
 * and jolt_member_reset makes it provable again.  With JOLT_STAGE_MEMBER_OWN jolt_stage_op_destroy destroys the member too.  Either way: operator, then member, then
 * the tables the member borrows, then the context. */
#define JOLT_STAGE_MEMBER_OWN 1u
int32_t jolt_stage_member_create(jolt_ctx *ctx, jolt_member *member, uint32_t flags, jolt_stage_op **out);
/* Test hook (CPU suite; no device, no context): the reference tier's dense member (NaiveSumcheckProver, crates/jolt-kernels/src/reference/naive.rs:53-377, LowToHigh) over HOST
 * tables as a stage operator, so that the contract and the two drivers below run without a GPU against the oracle's prove_batch.  Tables are copied. */
int32_t jolt_stage_host_expr_create(const jolt_fr_t *const *tables, size_t len, const jolt_member_desc *desc, jolt_stage_op **out);
/* Drivers for the tests and the bench (a Rust host calls the contract above from its own prove_batch; `ctx` may be NULL for host-only operators): prove_batch (prover.rs:193-362) over operators with the
 * library's test transcript; and one operator driven alone -- per round the message, every coefficient absorbed, Transcript::challenge -- with
 * coeffs_out = rounds x stride (tails zeroed), n_coeffs_out[r] = the coefficients of round r, claim in = input claim / out = the final claim. */
int32_t jolt_host_prove_batch_ops(jolt_ctx *ctx, jolt_stage_op *const *ops, size_t n_ops, const jolt_fr_t *input_claims, const jolt_fr_t *coefficients,
                                  const size_t *offsets, size_t max_num_vars, size_t max_degree, uint64_t transcript_label, int32_t challenge_mode,
                                  jolt_fr_t *out_polys, jolt_fr_t *out_challenges, jolt_fr_t *out_member_claims, jolt_fr_t *out_final_claim);
/* jolt_host_prove_batch_ops on a transcript the caller already holds (the same bytes when that transcript is fresh under the same label). */
int32_t jolt_host_prove_batch_ops_on(jolt_ctx *ctx, jolt_stage_op *const *ops, size_t n_ops, const jolt_fr_t *input_claims, const jolt_fr_t *coefficients,
                                     const size_t *offsets, size_t max_num_vars, size_t max_degree, jolt_host_transcript *transcript, int32_t challenge_mode,
                                     jolt_fr_t *out_polys, jolt_fr_t *out_challenges, jolt_fr_t *out_member_claims, jolt_fr_t *out_final_claim);
/* A Spartan stage on ONE transcript (crates/jolt-prover/src/stages/stage1.rs:63-111): jolt_r1cs_uniskip_sums_rows against eq(tau_low, .), the first-round polynomial,
 * jolt_host_prove_uniskip, the remainder operator at the drawn challenge, and a one-member batch (degree 3, n_tau - 1 rounds) whose input claim is the uni-skip output
 * claim.  tau: log T cycle coordinates, the stream coordinate of a two-stream system, then tau_high (n_tau = log T + n_streams).  The caller draws tau and the batch
 * coefficient.  Outputs: the 3D - 2 uni-skip coefficients, r0, the uni-skip output claim, the remainder's round polynomials ((n_tau - 1) x 4), challenges, final
 * claim and the n_cols output claims.  An unsatisfied witness fails the remainder's first round check (JOLT_ERR_ROUND_CHECK): the remainder's sum is taken
 * once over its tables and compared with the uni-skip output claim, because the split-eq round message is assembled from the claim and would pass its own check.  Everything is released. */
int32_t jolt_host_prove_spartan_stage(jolt_ctx *ctx, const jolt_r1cs_rows *rows, const jolt_ints *const *cols, size_t n_cols, const jolt_fr_t *tau, size_t n_tau,
                                      const jolt_fr_t *input_claim, const jolt_fr_t *coefficient, jolt_host_transcript *transcript, jolt_fr_t *uniskip_coeffs_out,
                                      jolt_fr_t *r0_out, jolt_fr_t *uniskip_claim_out, jolt_fr_t *polys_out, jolt_fr_t *challenges_out, jolt_fr_t *final_claim_out,
                                      jolt_fr_t *output_claims_out);
int32_t jolt_host_stage_op_prove_alone(jolt_stage_op *op, jolt_host_transcript *transcript, jolt_fr_t *claim, jolt_fr_t *coeffs_out, size_t stride,
                                       uint32_t *n_coeffs_out, jolt_fr_t *challenges_out);
/* jolt_host_prove_batch_ops under the backend's round scheduler (BuildRoundScheduler, crates/jolt-kernels/src/backend.rs:68-70; RoundScheduler, prover.rs:110-120): per round the
 * operators made by jolt_stage_member_create go into ONE jolt_round_group_prove (one launch set, one wait) and their last binds into ONE jolt_round_group_finish; every other
 * operator runs as under SequentialRounds.  Same arguments, same outputs, the same bytes.  An operator or a member listed twice is JOLT_ERR_INVALID_ARG. */
int32_t jolt_host_prove_batch_ops_grouped(jolt_ctx *ctx, jolt_stage_op *const *ops, size_t n_ops, const jolt_fr_t *input_claims, const jolt_fr_t *coefficients,
                                          const size_t *offsets, size_t max_num_vars, size_t max_degree, uint64_t transcript_label, int32_t challenge_mode,
                                          jolt_fr_t *out_polys, jolt_fr_t *out_challenges, jolt_fr_t *out_member_claims, jolt_fr_t *out_final_claim);

/* ------------------------------------------------------------------------------------------------------------
 * Precommitted claim reductions (crates/jolt-kernels/src/precommitted_reduction.rs; builders crates/jolt-kernels/src/optimized/precommitted_reduction.rs):
 * the stage-6b cycle phases and stage-7 address phases of the trusted-advice, untrusted-advice, committed-bytecode and program-image reductions as ONE generic
 * operator pair.  The round schedule (which rounds of a phase's window bind a variable) and the variable permutation are the CALLER's inputs, as they are relation
 * accessors in the reference (PrecommittedClaimReduction::cycle_phase_rounds / address_phase_rounds / poly_opening_round_permutation_be).
 *
 * State (:76-85): `value` and `eq` of 2^n entries ALREADY in opening-round order, n_aux passenger tables of the same length that bind alongside without entering
 * the summand, a running scale (1/2 per inactive round ingested) and its inverse.  The operator is head-aligned (batch offset 0): it is consulted in every round
 * of its window and `bind` is NULL in round 0 only.
 *   prove_round(bind, round, previous_claim) (:140-151): the pending challenge belongs to round - 1 -- active: bind every table LowToHigh; inactive: scale *= 1/2,
 *     scale_inv *= 2 (:160-172).  Then the message (:96-133): inactive -> the ONE coefficient previous_claim / 2; active -> e0 = sum_j value[2j] eq[2j],
 *     e2 = sum_j (2 value[2j+1] - value[2j]) (2 eq[2j+1] - eq[2j]), the HINT e1 = previous_claim scale_inv - e0, c2 = (e0 - 2 e1 + e2) / 2, c1 = e1 - e0 - c2, and the
 *     THREE coefficients (e0, c1, c2) scale.  e1 comes from the claim, not from the tables: under a batch's 2^(max - rounds) padding the emitted quadratic carries the
 *     padding factor (module doc :30-37), and there is no round check to fail.
 *   finish_rounds(bind) (:154-156): the bind of the last round.
 *   output_claims, cycle operator (:359-365, :492-510): with an address phase scheduled (n_address_active > 0) the intermediate claim sum value eq scale over the
 *     bound tables (:176-192); without one the bound value[0], then the bound aux[i][0] -- JOLT_ERR_NOT_FULLY_BOUND while a variable is unbound (:194-202).
 *   output_claims, address operator (:536-590): the bound value[0], then the aux[i][0]; JOLT_ERR_NOT_FULLY_BOUND likewise.
 * Degree 2; num_rounds = the phase's total; jolt_stage_op_input_claim = sum value eq scale (the cycle operator before a round: sum value eq).
 *
 * jolt_stage_precommitted_cycle_create: the operator works on its OWN copies of the tables (the caller's stay intact and need not outlive it).  n_aux <= 256.
 *   cycle_active / address_active: strictly ascending round indices below cycle_total / address_total (JOLT_ERR_INVALID_ARG otherwise); cycle_total >= 1.
 *   JOLT_ERR_SIZE_MISMATCH: tables of unequal length, n_cycle_active + n_address_active != n (:317-329 TableSizeMismatch); JOLT_ERR_INVALID_ARG: a length that is
 *   not a power of two, a null or foreign table, n_aux > 256.
 * jolt_stage_precommitted_address_create: reclaims the carry -- the bound tables AND the running scale (:225-234, :418-426) -- out of a FINISHED cycle operator, the
 *   way jolt_stage_bytecode_read_raf_cycle_create consumes its address operator.  A cycle operator without an address phase, one whose rounds are not finished, or
 *   one whose carry has been reclaimed is JOLT_ERR_INVALID_ARG with the reference's diagnostic in jolt_last_error ("stage 6b parked no precommitted reduction state
 *   for the scheduled address phase").  The cycle operator keeps answering output_claims (its intermediate claim is kept).
 * jolt_stage_host_precommitted_create / _address_create: the same contract over HOST tables with no device and no context (tables copied), as
 *   jolt_stage_host_expr_create is for the dense member: what the CPU suite drives against the definition.
 * ---------------------------------------------------------------------------------------------------------- */
int32_t jolt_stage_precommitted_cycle_create(jolt_ctx *ctx, const jolt_table *value, const jolt_table *eq, const jolt_table *const *aux, size_t n_aux,
                                             const size_t *cycle_active, size_t n_cycle_active, size_t cycle_total, const size_t *address_active,
                                             size_t n_address_active, size_t address_total, jolt_stage_op **out);
int32_t jolt_stage_precommitted_address_create(jolt_ctx *ctx, jolt_stage_op *cycle_op, jolt_stage_op **out);
int32_t jolt_stage_host_precommitted_create(const jolt_fr_t *value, const jolt_fr_t *eq, const jolt_fr_t *const *aux, size_t n_aux, size_t len,
                                            const size_t *cycle_active, size_t n_cycle_active, size_t cycle_total, const size_t *address_active,
                                            size_t n_address_active, size_t address_total, jolt_stage_op **out);
int32_t jolt_stage_host_precommitted_address_create(jolt_stage_op *cycle_op, jolt_stage_op **out);
/* The prepare side (optimized/precommitted_reduction.rs), each a small kernel or a composition of entries above; the bytecode value fold sum_c w_c chunk_c is
 * jolt_rlc (in groups above 40 chunks), the program image jolt_table_from_ints then jolt_table_permute_bits, advice_opening jolt_table_evaluate.
 * jolt_host_precommitted_lsb_permutation: lsb_permutation (precommitted_reduction.rs:595-609).  perm_be[be_index] = the opening round of big-endian variable be_index,
 *   all distinct (a duplicate is JOLT_ERR_INVALID_ARG); the variables sorted by round become the new LSB order, old_lsb_to_new_lsb[n - 1 - be_index] = new_lsb.
 *   *is_identity = 1 when the relabeling moves nothing (the reference's None).  n <= 40.
 * jolt_host_precommitted_permute_challenges: permute_challenges (:641-652): out[n - 1 - map[n - 1 - old_be]] = challenges_be[old_be].
 * jolt_table_permute_bits: permute_coefficients (:615-636): out[new] = table[old] with bit b of `new` moved to its pre-image position; a pure gather into a fresh
 *   table.  table length 2^n (JOLT_ERR_SIZE_MISMATCH); a map that is not a permutation of 0 .. n-1 is JOLT_ERR_INVALID_ARG.
 * jolt_eq_evals_shifted: shifted_eq_slice (optimized/precommitted_reduction.rs:337-360): out[i] = eq(r, (start_index + i) mod 2^n), big-endian as jolt_eq_evals, for
 *   1 <= len <= 2^n, assembled from maximal aligned blocks (jolt_eq_evals_aligned_block), wrap included; the full 2^n table is never built.
 * jolt_table_outer: the bytecode eq template lane_weights[lane] * cycle_table[cycle] at index -> (lane, cycle) = TracePolynomialOrder::index_to_address_cycle
 *   (crates/jolt-claims/src/protocols/jolt/geometry/dimensions.rs:48-58): JOLT_TRACE_CYCLE_MAJOR (index / cycles, index % cycles), JOLT_TRACE_ADDRESS_MAJOR
 *   (index % lanes, index / lanes); cycles = the length of cycle_table. */
enum { JOLT_TRACE_CYCLE_MAJOR = 0, JOLT_TRACE_ADDRESS_MAJOR = 1 }; /* TracePolynomialOrder::transcript_scalar (dimensions.rs:28-33) */
int32_t jolt_host_precommitted_lsb_permutation(const size_t *perm_be, size_t n, size_t *old_lsb_to_new_lsb, int32_t *is_identity);
int32_t jolt_host_precommitted_permute_challenges(const jolt_fr_t *challenges_be, size_t n, const size_t *map, jolt_fr_t *out);
int32_t jolt_table_permute_bits(jolt_ctx *ctx, const jolt_table *table, const size_t *old_lsb_to_new_lsb, size_t n, jolt_table **out);
int32_t jolt_eq_evals_shifted(jolt_ctx *ctx, const jolt_fr_t *r, size_t n, size_t start_index, size_t len, jolt_table **out);
int32_t jolt_table_outer(jolt_ctx *ctx, const jolt_fr_t *lane_weights, size_t n_lanes, const jolt_table *cycle_table, int32_t order, jolt_table **out);

/* ---- TESTS ONLY: device twins of the host forms above (csrc/device_probe.hip).  A jolt_host_* form compiles a function the kernels call for the CPU so that the
 * CPU suite can hold it to an independent reference at corner operands; the jolt_probe_* entry of the same name runs that function on the device, one lane per
 * operand tuple: host arrays of n tuples in, one launch, n results out.  Nothing on the product path calls these.  Every entry refuses n > 2^20
 * (JOLT_ERR_UNSUPPORTED), a null array with n > 0, an unknown op, and the operands its host form refuses, with the host form's status; a refused call launches
 * nothing and writes nothing; n = 0 is JOLT_OK.
 * jolt_probe_field_op: field 0 = Fr, 1 = Fq as in jolt_host_mul_limbs29; unary ops ignore b; MUL_SHIFTED is Fr only and refuses a b whose four low u32 limbs are
 *   not zero, as jolt_host_fr_mul_shifted does.  jolt_host_field_op is the same ops over the same arrays on the host, with the device's multiplication algorithm
 *   (mul_limbs29) wherever the device multiplies.
 * jolt_probe_fq_limb_op / jolt_probe_g1xl_add_paths: jolt_host_fq_limb_op / jolt_host_g1xl_add_paths per tuple (acc n x 36 limbs, q n x 18, negate n; common, full,
 *   step n x 36 each, suspect n, canon n x 64 words).
 * jolt_probe_fq2_op: JOLT_FQ2_*.  jolt_probe_fq12_op: JOLT_FQ12_MUL, _SQR, _CONJ, _MUL_SPARSE; _INV and the Frobenius maps exist for the host only (the final
 *   exponentiation runs there): JOLT_ERR_UNSUPPORTED.  jolt_probe_g2_op: JOLT_PROBE_G2_ADD and _DOUBLE write n points to out, JOLT_PROBE_G2_EQ n flags to equal.
 * jolt_probe_suffix_mle: jolt_host_suffix_mle per tuple.  jolt_probe_dory_fr_digits: jolt_host_dory_fr_digits per scalar, digits_out n rows of W words.
 * jolt_probe_small_scalar_dots / jolt_host_small_scalar_dots: n dot products over slices of one column of n_terms machine integers of `kind` (JOLT_INT_*; 8 bytes a term,
 *   16 for JOLT_INT_I128) against n_terms field elements through the small-scalar accumulator: out[i] = sum of values[k] * ints[k] over offsets[i] <= k < offsets[i + 1];
 *   offsets holds n + 1 ascending entries, the last at most n_terms <= 2^20 (anything else is JOLT_ERR_INVALID_ARG).  One slice of kind I128 is
 *   jolt_host_small_scalar_dot. */
enum { JOLT_PROBE_MUL = 0, JOLT_PROBE_SQR = 1, JOLT_PROBE_ADD = 2, JOLT_PROBE_SUB = 3, JOLT_PROBE_NEG = 4, JOLT_PROBE_DBL = 5, JOLT_PROBE_FROM_MONT = 6,
       JOLT_PROBE_TO_MONT = 7, JOLT_PROBE_MUL_SHIFTED = 8 };
enum { JOLT_PROBE_G2_ADD = 0, JOLT_PROBE_G2_DOUBLE = 1, JOLT_PROBE_G2_EQ = 2 };
int32_t jolt_host_field_op(int32_t field, int32_t op, const jolt_fr_t *a, const jolt_fr_t *b, size_t n, jolt_fr_t *out);
int32_t jolt_probe_field_op(jolt_ctx *ctx, int32_t field, int32_t op, const jolt_fr_t *a, const jolt_fr_t *b, size_t n, jolt_fr_t *out);
int32_t jolt_probe_fq_limb_op(jolt_ctx *ctx, int32_t op, const jolt_fr_t *a, const jolt_fr_t *b, const jolt_fr_t *c, const jolt_fr_t *d, size_t n, jolt_fr_t *out);
int32_t jolt_probe_g1xl_add_paths(jolt_ctx *ctx, const uint32_t *acc, const uint32_t *q, const int32_t *negate, size_t n, uint32_t *common, uint32_t *full, uint32_t *step,
                                  int32_t *suspect, uint32_t *canon);
int32_t jolt_probe_fq2_op(jolt_ctx *ctx, int32_t op, const jolt_fq2_t *a, const jolt_fq2_t *b, size_t n, jolt_fq2_t *out);
int32_t jolt_probe_g2_op(jolt_ctx *ctx, int32_t op, const jolt_g2_t *p, const jolt_g2_t *q, size_t n, jolt_g2_t *out, int32_t *equal);
int32_t jolt_probe_fq12_op(jolt_ctx *ctx, int32_t op, const jolt_gt_t *a, const jolt_gt_t *b, size_t n, jolt_gt_t *out);
int32_t jolt_probe_suffix_mle(jolt_ctx *ctx, const uint32_t *kind, const uint64_t *lo, const uint64_t *hi, const uint32_t *len, size_t n, uint64_t *out);
int32_t jolt_probe_dory_fr_digits(jolt_ctx *ctx, const jolt_fr_t *scalars, size_t n, int32_t c, int32_t W, uint32_t *digits_out, uint32_t *negative_out);
int32_t jolt_host_small_scalar_dots(const jolt_fr_t *values, const void *ints, int32_t kind, const uint64_t *offsets, size_t n_terms, size_t n, jolt_fr_t *out);
int32_t jolt_probe_small_scalar_dots(jolt_ctx *ctx, const jolt_fr_t *values, const void *ints, int32_t kind, const uint64_t *offsets, size_t n_terms, size_t n, jolt_fr_t *out);

#ifdef __cplusplus
}
#endif
#endif /* JOLT_HIP_H */
