// jolt_amd/csrc/hyperkzg_verify.hip -- HyperKZG verification as one call, the verifier's setup, and stage 8's batch framing over the commitment grid's columns.
//
// Replaces:
//   HyperKZGVerifierSetup (crates/jolt-hyperkzg/src/types.rs:112-146)                    -> jolt_hyperkzg_verifier_setup_*
//   HyperKZGScheme::verify (scheme.rs:162-242) + kzg_verify_batch (kzg.rs:132-210)       -> jolt_host_hyperkzg_verify_scalars (host), jolt_host_hyperkzg_verify,
//                                                                                           jolt_host_hyperkzg_verify_with_transcript
//   AdditivelyHomomorphic::combine (scheme.rs:346-352)                                   -> the commitments' scalars inside L's MSM (no separate pass)
//   HomomorphicBatch::prove_batch / verify_batch (crates/jolt-openings/src/schemes.rs:487-551) -> jolt_host_hyperkzg_prove_batch, jolt_host_hyperkzg_verify_batch
//
// NO kernel here.  A verification is host control flow over two jolt_dory_products batches (dory_resident.hip): L and -R as two MSM_G1 items (about ell + 40 scalar
// multiplications, one term per lane, an addition tree), then e(L, g2) e(-R, beta g2) as one PAIR item against the setup's prepared line table, the final
// exponentiation on the host.  Latency bound throughout: two synchronisations per verification.
#include <vector>

#include "ctx.hpp"
#include "dory_batch_plan.hpp"
#include "dory_host.hpp"
#include "dory_kernels.hip.h"
#include "fq12.hip.h"
#include "grid_hint.hpp"
#include "hyperkzg_transcript.hpp"
#include "onehot.hpp"
#include "srs.hpp"

using namespace jolt;
using namespace jolt::dory_host;
using namespace jolt::dory_dev;
using namespace jolt::hyperkzg_host;

struct jolt_hyperkzg_verifier_setup {
    jolt_ctx* ctx = nullptr;
    jolt_g1_t g1;
    jolt_g2_t g2, beta_g2;
    jolt_dory_vec* g2_vec = nullptr;       // (g2, beta g2), resident
    jolt_g2_prepared* prepared = nullptr;  // their line tables, built once
};

namespace {

constexpr size_t kMaxEll = 40;                          // the opening's limit
constexpr size_t kMaxCommitments = (size_t)1 << 20;
// the MSM batch of a verification packs L (n_commitments + ell + 3 terms) and -R (3 terms), each padded to whole wavefronts, into one chain of jolt_dory_products: with
// both limits above it stays inside the chain's capacity, so the batch cannot refuse for its size after the transcript has absorbed the proof
static_assert(kMaxCommitments + kMaxEll + 3 + 2 * 64 + 64 <= dory_plan::kMaxPacked, "the verifier's input limits keep its MSM batch inside one chain of a product batch");

void destroy(jolt_hyperkzg_verifier_setup* vs) {
    if (vs->prepared) (void)jolt_g2_prepared_free(vs->ctx, vs->prepared);
    if (vs->g2_vec) (void)jolt_dory_vec_free(vs->ctx, vs->g2_vec);
    delete vs;
}

// resident vectors of one verification, freed on every path (jolt_dory_products synchronises before it returns: nothing of this call is in flight by then)
struct Resident {
    jolt_ctx* ctx;
    std::vector<jolt_dory_vec*> vecs;
    explicit Resident(jolt_ctx* c) : ctx(c) {}
    ~Resident() {
        for (jolt_dory_vec* v : vecs) (void)jolt_dory_vec_free(ctx, v);
    }
    int32_t upload(int32_t kind, const void* host, size_t n, jolt_dory_vec** out) {
        JOLT_TRY(jolt_dory_vec_upload(ctx, kind, host, n, out));
        vecs.push_back(*out);
        return JOLT_OK;
    }
};

// scheme.rs:203-234: level i relates P_i(r), P_i(-r) and P_{i+1}(r^2); the claimed evaluation closes the chain (y_sq.push(claimed_eval)) and level i uses
// point[ell - 1 - i].  Returns the first failing level, or ell when every level holds.
size_t folding_check(size_t ell, const jolt_fr_t* point, const Fr& eval, const jolt_fr_t* v, const Fr& r) {
    const Fr two_r = dbl(r), one = Fr::one();
    for (size_t level = 0; level < ell; ++level) {
        const Fr y_next = level + 1 < ell ? fr_from_abi(&v[2 * ell + level + 1]) : eval;
        const Fr y_pos = fr_from_abi(&v[level]), y_neg = fr_from_abi(&v[ell + level]), x = fr_from_abi(&point[ell - 1 - level]);
        const Fr lhs = mul(two_r, y_next);
        const Fr rhs = add(mul(mul(r, sub(one, x)), add(y_pos, y_neg)), mul(x, sub(y_pos, y_neg)));
        if (!(lhs == rhs)) return level;
    }
    return ell;
}

// kzg.rs:159-200 with k = ell commitments
void batch_scalars(size_t ell, const jolt_fr_t* v, const Fr& r, const Fr& q, const Fr& d0, jolt_fr_t* l_scalars, jolt_fr_t* d_out) {
    const Fr d1 = sqr(d0), mult = add(add(Fr::one(), d0), d1);
    Fr qp = Fr::one(), b[3] = {Fr::zero(), Fr::zero(), Fr::zero()};
    for (size_t j = 0; j < ell; ++j) {
        fr_to_abi(&l_scalars[j], mul(qp, mult));
        for (int t = 0; t < 3; ++t) b[t] = add(b[t], mul(fr_from_abi(&v[(size_t)t * ell + j]), qp));
        qp = mul(qp, q);
    }
    fr_to_abi(&l_scalars[ell], r);                                 // u_0
    fr_to_abi(&l_scalars[ell + 1], mul(neg(r), d0));               // u_1 d_0
    fr_to_abi(&l_scalars[ell + 2], mul(sqr(r), d1));               // u_2 d_1
    fr_to_abi(&l_scalars[ell + 3], neg(add(add(b[0], mul(d0, b[1])), mul(d1, b[2]))));
    fr_to_abi(&d_out[0], d0);
    fr_to_abi(&d_out[1], d1);
}

int32_t challenge_checked(jolt_ctx* ctx, const jolt_fr_t* c) {
    JOLT_REQUIRE(ctx, fr_is_canonical(fr_from_abi(c)), "the transcript returned a challenge that is not a canonical Fr");
    return JOLT_OK;
}

// every check of a verification's input (scheme.rs:170-186 and the entry points' own): a refused call absorbs nothing, enqueues nothing and writes nothing
int32_t verify_checked(jolt_ctx* ctx, const jolt_hyperkzg_verifier_setup* vs, const jolt_g1_t* commitments, const jolt_fr_t* commitment_scalars, size_t n_commitments,
                       const jolt_fr_t* point, size_t ell, const jolt_fr_t* eval, const jolt_g1_t* com, const jolt_g1_t* w, const jolt_fr_t* v) {
    if (!ctx || !vs) return JOLT_ERR_INVALID_ARG;
    JOLT_REQUIRE(ctx, vs->ctx == ctx, "the verifier setup belongs to another context");
    if (ell == 0) return JOLT_ERR_EMPTY_POINT;  // (an empty point and an empty v may come as null pointers)
    if (!commitments || !commitment_scalars || !point || !eval || !w || !v || (ell > 1 && !com)) return JOLT_ERR_INVALID_ARG;
    if (ell > kMaxEll || n_commitments > kMaxCommitments) return JOLT_ERR_UNSUPPORTED;
    JOLT_REQUIRE(ctx, n_commitments != 0, "no commitment");
    JOLT_REQUIRE(ctx, all_canonical(point, ell) && all_canonical(eval, 1) && all_canonical(v, 3 * ell) && all_canonical(commitment_scalars, n_commitments),
                 "a field element is not a canonical Fr");
    JOLT_REQUIRE(ctx, all_on_curve<G1Ops>(commitments, n_commitments) && all_on_curve<G1Ops>(com, ell - 1) && all_on_curve<G1Ops>(w, 3), "a point is not on the curve or not canonical");
    return JOLT_OK;
}

// commitments[i] enters L with scalar commitment_scalars[i] (1 + d_0 + d_1): one commitment under scalar one is HyperKZGScheme::verify, a batch's commitments under
// gamma's powers are verify after combine -- C_0 is never built
int32_t verify_impl(jolt_ctx* ctx, const jolt_hyperkzg_verifier_setup* vs, const jolt_g1_t* commitments, const jolt_fr_t* commitment_scalars, size_t n_commitments,
                    const jolt_fr_t* point, size_t ell, const jolt_fr_t* eval, const jolt_g1_t* com, const jolt_g1_t* w, const jolt_fr_t* v, jolt_open_transcript_fn fn,
                    void* user, int32_t* accepted, int32_t* failed_check, size_t* failed_level) {
    if (!fn || !accepted || !failed_check || !failed_level) return JOLT_ERR_INVALID_ARG;
    JOLT_TRY(verify_checked(ctx, vs, commitments, commitment_scalars, n_commitments, point, ell, eval, com, w, v));
    // ---- phase 0: the level commitments -> r (scheme.rs:188-196) ----
    jolt_fr_t r_abi, q_abi, d0_abi;
    JOLT_TRY(fn(user, 0, com, ell - 1, nullptr, 0, &r_abi));
    JOLT_TRY(challenge_checked(ctx, &r_abi));
    const Fr r = fr_from_abi(&r_abi);
    if (r.is_zero()) {
        ctx->last_error = "the transcript returned a zero challenge r (HyperKZGError::DegenerateChallenge)";
        return JOLT_ERR_NOT_INVERTIBLE;
    }
    // ---- the folding check; on failure the transcript goes no further (scheme.rs:231-233) ----
    const size_t level = folding_check(ell, point, fr_from_abi(eval), v, r);
    if (level < ell) {
        *accepted = 0;
        *failed_check = 1;
        *failed_level = level;
        return JOLT_OK;
    }
    // ---- phase 1: the evaluations -> q; phase 2: the witness commitments -> d_0 (kzg.rs:152-166) ----
    JOLT_TRY(fn(user, 1, nullptr, 0, v, 3 * ell, &q_abi));
    JOLT_TRY(challenge_checked(ctx, &q_abi));
    JOLT_TRY(fn(user, 2, w, 3, nullptr, 0, &d0_abi));
    JOLT_TRY(challenge_checked(ctx, &d0_abi));
    std::vector<jolt_fr_t> ls(ell + 4);
    jolt_fr_t d[2];
    batch_scalars(ell, v, r, fr_from_abi(&q_abi), fr_from_abi(&d0_abi), ls.data(), d);
    // ---- L over (commitments, com, w, g1) and -R over w: one batch of two MSM items ----
    const size_t n_l = n_commitments + (ell - 1) + 4;
    std::vector<jolt_g1_t> pts;
    pts.reserve(n_l);
    pts.insert(pts.end(), commitments, commitments + n_commitments);
    pts.insert(pts.end(), com, com + (ell - 1));
    pts.insert(pts.end(), w, w + 3);
    pts.push_back(vs->g1);
    std::vector<jolt_fr_t> sc(n_l + 3);
    const Fr mult = fr_from_abi(&ls[0]);  // q^0 (1 + d_0 + d_1)
    for (size_t i = 0; i < n_commitments; ++i) fr_to_abi(&sc[i], mul(fr_from_abi(&commitment_scalars[i]), mult));
    for (size_t j = 1; j < ell + 4; ++j) sc[n_commitments + j - 1] = ls[j];
    fr_to_abi(&sc[n_l], neg(Fr::one()));
    fr_to_abi(&sc[n_l + 1], neg(fr_from_abi(&d[0])));
    fr_to_abi(&sc[n_l + 2], neg(fr_from_abi(&d[1])));
    Resident res(ctx);
    jolt_dory_vec *v_pts = nullptr, *v_sc = nullptr, *v_lr = nullptr;
    JOLT_TRY(res.upload(JOLT_DORY_KIND_G1, pts.data(), pts.size(), &v_pts));
    JOLT_TRY(res.upload(JOLT_DORY_KIND_FR, sc.data(), sc.size(), &v_sc));
    jolt_dory_result sums[2];
    {
        const jolt_dory_item items[2] = {jolt_dory_item{JOLT_DORY_MSM_G1, v_pts, 0, v_sc, 0, nullptr, 0, n_l},            // L (kzg.rs:182-202)
                                         jolt_dory_item{JOLT_DORY_MSM_G1, v_pts, n_l - 4, v_sc, n_l, nullptr, 0, 3}};     // -R (kzg.rs:204-208)
        JOLT_TRY(jolt_dory_products(ctx, items, 2, sums));
    }
    // ---- e(L, g2) e(-R, beta g2): one batch of one PAIR item against the prepared (g2, beta g2) ----
    jolt_g1_t lr[2];
    std::memcpy(&lr[0], &sums[0], sizeof(jolt_g1_t));
    std::memcpy(&lr[1], &sums[1], sizeof(jolt_g1_t));
    JOLT_TRY(res.upload(JOLT_DORY_KIND_G1, lr, 2, &v_lr));
    jolt_dory_result product;
    {
        const jolt_dory_item item{JOLT_DORY_PAIR, v_lr, 0, nullptr, 0, vs->prepared, 0, 2};
        JOLT_TRY(jolt_dory_products(ctx, &item, 1, &product));
    }
    const Fq12 one = Fq12::one();
    const bool ok = std::memcmp(&product, &one, sizeof(one)) == 0;
    *accepted = ok ? 1 : 0;
    *failed_check = ok ? 0 : 2;
    *failed_level = 0;
    return JOLT_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------------ the verifier's setup
extern "C" int32_t jolt_hyperkzg_verifier_setup_free(jolt_ctx* ctx, jolt_hyperkzg_verifier_setup* vs) {
    if (!ctx) return JOLT_ERR_INVALID_ARG;
    if (!vs) return JOLT_OK;
    JOLT_REQUIRE(ctx, vs->ctx == ctx, "the verifier setup belongs to another context");
    destroy(vs);
    return JOLT_OK;
}

extern "C" int32_t jolt_hyperkzg_verifier_setup_create(jolt_ctx* ctx, const jolt_g1_t* g1, const jolt_g2_t* g2, const jolt_g2_t* beta_g2, jolt_hyperkzg_verifier_setup** out) {
    if (!ctx || !g1 || !g2 || !beta_g2 || !out) return JOLT_ERR_INVALID_ARG;
    const jolt_g2_t pair[2] = {*g2, *beta_g2};
    JOLT_REQUIRE(ctx, all_on_curve<G1Ops>(g1, 1) && all_on_curve<G2Ops>(pair, 2), "a point is not on its curve or not canonical");
    JOLT_REQUIRE(ctx, !g1_is_identity(pt_from_abi<G1Jac>(g1)) && !g2_is_identity(pt_from_abi<G2Jac>(g2)) && !g2_is_identity(pt_from_abi<G2Jac>(beta_g2)),
                 "a point of the verifier setup is the identity");
    jolt_hyperkzg_verifier_setup* vs = new (std::nothrow) jolt_hyperkzg_verifier_setup();
    if (!vs) return JOLT_ERR_OOM;
    vs->ctx = ctx;
    vs->g1 = *g1;
    vs->g2 = *g2;
    vs->beta_g2 = *beta_g2;
    int32_t rc = jolt_dory_vec_upload(ctx, JOLT_DORY_KIND_G2, pair, 2, &vs->g2_vec);
    if (rc == JOLT_OK) rc = jolt_dory_g2_prepare_vec(ctx, vs->g2_vec, 0, 2, &vs->prepared);
    if (rc != JOLT_OK) {
        destroy(vs);
        return rc;
    }
    *out = vs;
    return JOLT_OK;
}

extern "C" int32_t jolt_hyperkzg_verifier_setup_from_secret(jolt_ctx* ctx, const jolt_fr_t* beta, const jolt_g1_t* g1, const jolt_g2_t* g2, jolt_hyperkzg_verifier_setup** out) {
    if (!ctx || !beta || !g1 || !g2 || !out) return JOLT_ERR_INVALID_ARG;
    JOLT_REQUIRE(ctx, all_canonical(beta, 1), "beta is not a canonical Fr");
    JOLT_REQUIRE(ctx, all_on_curve<G2Ops>(g2, 1), "a point is not on its curve or not canonical");
    jolt_g2_t beta_g2;
    JOLT_TRY(jolt_host_g2_scalar_mul(g2, beta, &beta_g2));  // scheme.rs:67
    return jolt_hyperkzg_verifier_setup_create(ctx, g1, g2, &beta_g2, out);
}

extern "C" int32_t jolt_hyperkzg_verifier_setup_points(const jolt_hyperkzg_verifier_setup* vs, jolt_g1_t* g1, jolt_g2_t* g2, jolt_g2_t* beta_g2) {
    if (!vs || !g1 || !g2 || !beta_g2) return JOLT_ERR_INVALID_ARG;
    *g1 = vs->g1;
    *g2 = vs->g2;
    *beta_g2 = vs->beta_g2;
    return JOLT_OK;
}

// ------------------------------------------------------------------------------------------------------------------ the verifier's scalars
extern "C" int32_t jolt_host_hyperkzg_verify_scalars(size_t ell, const jolt_fr_t* point, const jolt_fr_t* eval, const jolt_fr_t* v, const jolt_fr_t* r, const jolt_fr_t* q,
                                                     const jolt_fr_t* d0, int32_t* folding_ok, size_t* failed_level, jolt_fr_t* l_scalars, jolt_fr_t* d_out) {
    if (!point || !eval || !v || !r || !q || !d0 || !folding_ok || !failed_level || !l_scalars || !d_out) return JOLT_ERR_INVALID_ARG;
    if (ell == 0 || ell > kMaxEll) return JOLT_ERR_INVALID_ARG;  // HyperKZGError::EmptyPoint
    if (!all_canonical(point, ell) || !all_canonical(eval, 1) || !all_canonical(v, 3 * ell) || !all_canonical(r, 1) || !all_canonical(q, 1) || !all_canonical(d0, 1))
        return JOLT_ERR_INVALID_ARG;
    const Fr rr = fr_from_abi(r);
    if (rr.is_zero()) return JOLT_ERR_NOT_INVERTIBLE;  // HyperKZGError::DegenerateChallenge
    const size_t level = folding_check(ell, point, fr_from_abi(eval), v, rr);
    *folding_ok = level == ell ? 1 : 0;
    *failed_level = level == ell ? 0 : level;
    batch_scalars(ell, v, rr, fr_from_abi(q), fr_from_abi(d0), l_scalars, d_out);
    return JOLT_OK;
}

// ------------------------------------------------------------------------------------------------------------------ the verifier
extern "C" int32_t jolt_host_hyperkzg_verify_with_transcript(jolt_ctx* ctx, const jolt_hyperkzg_verifier_setup* vs, const jolt_g1_t* commitments,
                                                             const jolt_fr_t* commitment_scalars, size_t n_commitments, const jolt_fr_t* point, size_t ell, const jolt_fr_t* eval,
                                                             const jolt_g1_t* com, const jolt_g1_t* w, const jolt_fr_t* v, jolt_open_transcript_fn fn, void* user,
                                                             int32_t* accepted, int32_t* failed_check, size_t* failed_level) {
    return verify_impl(ctx, vs, commitments, commitment_scalars, n_commitments, point, ell, eval, com, w, v, fn, user, accepted, failed_check, failed_level);
}

extern "C" int32_t jolt_host_hyperkzg_verify(jolt_ctx* ctx, const jolt_hyperkzg_verifier_setup* vs, const jolt_g1_t* commitments, const jolt_fr_t* commitment_scalars,
                                             size_t n_commitments, const jolt_fr_t* point, size_t ell, const jolt_fr_t* eval, const jolt_g1_t* com, const jolt_g1_t* w,
                                             const jolt_fr_t* v, jolt_host_transcript* t, int32_t* accepted, int32_t* failed_check, size_t* failed_level) {
    if (!t || !t->t.inner) return JOLT_ERR_INVALID_ARG;
    return verify_impl(ctx, vs, commitments, commitment_scalars, n_commitments, point, ell, eval, com, w, v, open_engine_fn, t, accepted, failed_check, failed_level);
}

// ------------------------------------------------------------------------------------------------------------------ stage 8's batch framing
extern "C" int32_t jolt_host_hyperkzg_verify_batch(jolt_ctx* ctx, const jolt_hyperkzg_verifier_setup* vs, const jolt_g1_t* commitments, const jolt_fr_t* evaluations,
                                                   size_t n_claims, const jolt_fr_t* point, size_t n_point, const jolt_g1_t* com, const jolt_g1_t* w, const jolt_fr_t* v,
                                                   jolt_host_transcript* t, int32_t* accepted, int32_t* failed_check, size_t* failed_level, jolt_fr_t* joint_eval_out) {
    if (!ctx || !evaluations || !t || !t->t.inner || !accepted || !failed_check || !failed_level || !joint_eval_out) return JOLT_ERR_INVALID_ARG;
    // ---- the verifier's checks before the transcript absorbs the statement; gamma's powers and the joint evaluation do not exist yet, the evaluations stand in ----
    JOLT_TRY(verify_checked(ctx, vs, commitments, evaluations, n_claims, point, n_point, evaluations, com, w, v));
    // ---- the statement: gamma's powers, joint_eval = sum_i gamma^i y_i ----
    std::vector<jolt_fr_t> powers(n_claims);
    JOLT_TRY(jolt_host_opening_statement_absorb(t, evaluations, n_claims, powers.data()));
    Fr joint = Fr::zero();
    for (size_t i = 0; i < n_claims; ++i) joint = add(joint, mul(fr_from_abi(&powers[i]), fr_from_abi(&evaluations[i])));
    jolt_fr_t joint_abi;
    fr_to_abi(&joint_abi, joint);
    JOLT_TRY(verify_impl(ctx, vs, commitments, powers.data(), n_claims, point, n_point, &joint_abi, com, w, v, open_engine_fn, t, accepted, failed_check, failed_level));
    *joint_eval_out = joint_abi;
    // the closing claim after an accepted proof only: the reference leaves through `?` on a rejection (schemes.rs:541-549)
    if (*accepted) return jolt_host_opening_claim_absorb(t, point, n_point, joint_eval_out);
    return JOLT_OK;
}

extern "C" int32_t jolt_host_hyperkzg_prove_batch(jolt_ctx* ctx, const jolt_srs* srs, const jolt_onehot* const* sources, size_t n_sources, jolt_table* const* dense,
                                                  size_t n_dense, uint32_t log_k, const jolt_fr_t* evaluations, size_t n_claims, const jolt_fr_t* point, size_t n_point,
                                                  const jolt_grid_hint* hint, uint32_t levels, jolt_host_transcript* t, jolt_g1_t* com, jolt_g1_t* w, jolt_fr_t* v,
                                                  jolt_fr_t* challenges_out, jolt_fr_t* joint_eval_out) {
    if (!ctx || !srs || !evaluations || !point || !t || !t->t.inner || !w || !v || !joint_eval_out || (n_sources && !sources) || (n_dense && !dense) || (n_point > 1 && !com))
        return JOLT_ERR_INVALID_ARG;
    // ---- every check of this entry and of the joint polynomial, before the transcript absorbs anything and before anything is enqueued ----
    JOLT_REQUIRE(ctx, srs->ctx == ctx && (!hint || hint->ctx == ctx), "the SRS or the hint belongs to another context");
    JOLT_REQUIRE(ctx, n_claims != 0, "an empty batch");  // HomomorphicBatchStatement::new refuses it
    if (n_sources > 4 || n_dense > 8 || log_k > 8) return JOLT_ERR_UNSUPPORTED;  // the limits of jolt_grid_joint_polynomial
    for (size_t s = 0; s < n_sources; ++s) JOLT_REQUIRE(ctx, sources[s] && sources[s]->ctx == ctx, "a source is null or of another context");
    for (size_t d = 0; d < n_dense; ++d) JOLT_REQUIRE(ctx, dense[d] && dense[d]->ctx == ctx && dense[d]->data(), "a dense column is null or of another context");
    JOLT_REQUIRE(ctx, n_sources + n_dense != 0, "a batch has at least one column");
    const size_t T = n_sources ? sources[0]->cycles : dense[0]->len;
    JOLT_REQUIRE(ctx, T != 0 && (T & (T - 1)) == 0, "the cycle count must be a power of two");
    size_t log_t = 0, n_onehot = 0;
    while (((size_t)1 << log_t) < T) ++log_t;
    for (size_t s = 0; s < n_sources; ++s) {
        if (sources[s]->cycles != T) return JOLT_ERR_SIZE_MISMATCH;
        JOLT_REQUIRE(ctx, sources[s]->k <= (1u << log_k), "a hot address outside the grid");
        n_onehot += sources[s]->n_polys;
    }
    for (size_t d = 0; d < n_dense; ++d)
        if (dense[d]->len != T) return JOLT_ERR_SIZE_MISMATCH;
    JOLT_REQUIRE(ctx, n_claims == n_onehot + n_dense, "one claim per column of the joint polynomial");
    JOLT_REQUIRE(ctx, n_point == (size_t)log_k + log_t, "the point has one coordinate per variable of the grid");
    if (n_point == 0) return JOLT_ERR_EMPTY_POINT;
    if (n_point > kMaxEll) return JOLT_ERR_UNSUPPORTED;
    if (((size_t)1 << n_point) > srs->n) {
        ctx->last_error = "the SRS holds fewer than 2^ell bases";
        return JOLT_ERR_SRS_TOO_SMALL;
    }
    JOLT_REQUIRE(ctx, all_canonical(evaluations, n_claims) && all_canonical(point, n_point), "an evaluation or a coordinate is not a canonical Fr");
    const bool by_hint = hint && levels && n_onehot;  // otherwise every level commitment is an MSM and the hint is not read
    if (by_hint) JOLT_REQUIRE(ctx, hint->k == (1u << log_k) && hint->cycles == T && hint->n_cols == n_onehot, "the hint was not made over these sources on this grid");
    // ---- the statement: gamma's powers dealt to the columns (claim i is column i: one-hot columns source by source, then dense) ----
    std::vector<jolt_fr_t> powers(n_claims);
    JOLT_TRY(jolt_host_opening_statement_absorb(t, evaluations, n_claims, powers.data()));
    Fr joint = Fr::zero();
    for (size_t i = 0; i < n_claims; ++i) joint = add(joint, mul(fr_from_abi(&powers[i]), fr_from_abi(&evaluations[i])));
    fr_to_abi(joint_eval_out, joint);
    const jolt_fr_t *onehot_scalars = powers.data(), *dense_scalars = powers.data() + n_onehot;
    jolt_table* poly = nullptr;
    JOLT_TRY(jolt_grid_joint_polynomial(ctx, sources, n_sources, onehot_scalars, dense, n_dense, dense_scalars, log_k, &poly));
    // ---- the opening under t; a statement that does not hold is JOLT_ERR_ROUND_CHECK before a level commitment is absorbed ----
    const int32_t rc = jolt_internal_hyperkzg_open_grid_checked(ctx, srs, poly, point, n_point, open_engine_fn, t, by_hint ? hint : nullptr, levels, onehot_scalars, dense, n_dense,
                                                                dense_scalars, &joint, com, w, v, challenges_out);
    (void)jolt_table_free(ctx, poly);
    JOLT_TRY(rc);
    return jolt_host_opening_claim_absorb(t, point, n_point, joint_eval_out);
}
