// jolt_amd/csrc/dory_scheme.hip -- a Dory evaluation proof as one library call: the setup object, a round's in-place update as one call, the prover's side of
// Eval-VMV-RE under the caller's transcript or one of the library's engines, and the byte forms a transcript absorbs.
//
// Everything T-scale below exists already: the state comes from jolt_dory_state_* and each message is one jolt_dory_products batch (dory_resident.hip).  What is new on
// the device is the launch structure of a round's two updates (jolt_dory_round_update):
//   beta    v1 += beta Gamma1 | v2 += (1/beta) Gamma2                       k_dory_scale_add<G1Ops> on the main stream, k_dory_scale_add<G2Ops> on side[0]
//   alpha   v1 <- alpha v1_L + v1_R, s1 <- alpha s1_L + s1_R | the same under 1/alpha for v2, s2     each group's k_dory_scale_add and then its k_dory_fold_field
// TWO launches, one per group, not one kernel holding both paths: a shared kernel would give the G1 blocks G2's register budget (docs/kernels.md 3.5m).  The chains are
// forked by ctx->ev_fork and joined by ctx->ev_join[0] (Fork of dory_host.hpp, as jolt_dory_products forks its chains); no further stream, no captured graph, no host
// synchronisation.  The launches are enqueue_scale_add / enqueue_fold_field of dory_kernels.hip.h, the launch sites of the separate calls, so the vectors hold what those write.
// The opening (open_impl) is host control flow over those entries: the protocol of jolt_amd/dory_open.py and dory_reduce.py, with the challenges drawn through a
// callback after each message.  Every exit drains the streams before the state vectors go back to the pool (OpenState's destructor).
// The batch opening of stage 8 (jolt_host_dory_prove_batch) is HomomorphicBatch::prove_batch around it: the statement's framing (host_mirror.hip), the eq tables of the
// point, the lazy row fold under gamma's powers (the trace in either placement, then the block-embedded tables on top of it), the check <v, R> == joint_eval, open_impl with the hints weighted by the same powers, the closing claim.
#include <vector>

#include "ctx.hpp"
#include "dory_host.hpp"
#include "dory_kernels.hip.h"
#include "dory_prepared.hip.h"
#include "onehot.hpp"

using namespace jolt;
using namespace jolt::dory_host;
using namespace jolt::dory_dev;

namespace {

template <class T>
T* at(const jolt_dory_vec* v, size_t first) { return (T*)v->data + first; }

bool table_ok(const jolt_ctx* ctx, const jolt_table* t, size_t len) { return t && t->ctx == ctx && t->data() && t->len == len; }

constexpr uint32_t kMaxSigma = 30;  // 2^30 elements: kMaxElements of the resident vectors

}  // namespace

// ------------------------------------------------------------------------------------------------------------------ the setup
extern "C" int32_t jolt_dory_setup_free(jolt_ctx* ctx, jolt_dory_setup* setup) {
    if (!ctx) return JOLT_ERR_INVALID_ARG;
    if (!setup) return JOLT_OK;
    JOLT_REQUIRE(ctx, setup->ctx == ctx, "the setup belongs to another context");
    if (setup->prepared) (void)jolt_g2_prepared_free(ctx, setup->prepared);
    for (jolt_dory_vec* v : {setup->gamma1, setup->gamma2, setup->h1_vec, setup->h2_vec}) (void)jolt_dory_vec_free(ctx, v);
    delete setup;
    return JOLT_OK;
}

extern "C" int32_t jolt_dory_setup_create(jolt_ctx* ctx, const jolt_g1_t* gamma1, const jolt_g2_t* gamma2, size_t n, const jolt_g1_t* h1, const jolt_g2_t* h2, jolt_dory_setup** out) {
    if (!ctx || !gamma1 || !gamma2 || !h1 || !h2 || !out) return JOLT_ERR_INVALID_ARG;
    JOLT_REQUIRE(ctx, n != 0 && (n & (n - 1)) == 0, "Gamma1 and Gamma2 have one length, a power of two");
    if (n > ((size_t)1 << kMaxSigma)) return JOLT_ERR_UNSUPPORTED;
    jolt_dory_setup* s = new (std::nothrow) jolt_dory_setup();
    if (!s) return JOLT_ERR_OOM;
    s->ctx = ctx;
    s->n = n;
    s->h1 = *h1;
    s->h2 = *h2;
    int32_t rc = jolt_dory_vec_upload(ctx, JOLT_DORY_KIND_G1, gamma1, n, &s->gamma1);
    if (rc == JOLT_OK) rc = jolt_dory_vec_upload(ctx, JOLT_DORY_KIND_G2, gamma2, n, &s->gamma2);
    if (rc == JOLT_OK) rc = jolt_dory_vec_upload(ctx, JOLT_DORY_KIND_G1, h1, 1, &s->h1_vec);
    if (rc == JOLT_OK) rc = jolt_dory_vec_upload(ctx, JOLT_DORY_KIND_G2, h2, 1, &s->h2_vec);
    if (rc == JOLT_OK) rc = jolt_dory_g2_prepare_vec(ctx, s->gamma2, 0, n, &s->prepared);
    if (rc != JOLT_OK) {
        (void)jolt_dory_setup_free(ctx, s);
        return rc;
    }
    *out = s;
    return JOLT_OK;
}

extern "C" int32_t jolt_dory_setup_size(const jolt_dory_setup* setup, size_t* n) {
    if (!setup || !n) return JOLT_ERR_INVALID_ARG;
    *n = setup->n;
    return JOLT_OK;
}

extern "C" int32_t jolt_dory_setup_tier2(jolt_ctx* ctx, const jolt_dory_setup* setup, const jolt_dory_vec* const* hints, const size_t* hint_first, const size_t* hint_rows, size_t n,
                                         jolt_gt_t* outs) {
    if (!ctx || !setup || (n && (!hints || !hint_first || !hint_rows || !outs))) return JOLT_ERR_INVALID_ARG;
    JOLT_REQUIRE(ctx, setup->ctx == ctx, "the setup belongs to another context");
    std::vector<jolt_dory_item> items(n);
    for (size_t k = 0; k < n; ++k) items[k] = jolt_dory_item{JOLT_DORY_PAIR, hints[k], hint_first[k], nullptr, 0, setup->prepared, 0, hint_rows[k]};
    std::vector<jolt_dory_result> res(n);
    JOLT_TRY(jolt_dory_products(ctx, items.data(), n, res.data()));  // refuses the whole batch before it enqueues anything
    for (size_t k = 0; k < n; ++k) std::memcpy(&outs[k], &res[k], sizeof(jolt_gt_t));
    return JOLT_OK;
}

// ------------------------------------------------------------------------------------------------------------------ a round's update
extern "C" int32_t jolt_dory_round_update(jolt_ctx* ctx, int32_t mode, jolt_dory_vec* v1, size_t v1_first, jolt_dory_vec* v2, size_t v2_first, jolt_dory_vec* a, size_t a_first,
                                          jolt_dory_vec* b, size_t b_first, size_t n, const jolt_fr_t* scalar, const jolt_fr_t* scalar_inv) {
    if (!ctx || !v1 || !v2 || !a || !b || !scalar || !scalar_inv) return JOLT_ERR_INVALID_ARG;
    JOLT_REQUIRE(ctx, mode == JOLT_DORY_UPDATE_BETA || mode == JOLT_DORY_UPDATE_ALPHA, "unknown update mode");
    const bool alpha = mode == JOLT_DORY_UPDATE_ALPHA;
    JOLT_REQUIRE(ctx, view_ok(ctx, v1, JOLT_DORY_KIND_G1, v1_first, n) && view_ok(ctx, v2, JOLT_DORY_KIND_G2, v2_first, n), "v1 / v2 is not a G1 / G2 view of this context");
    if (alpha) {
        JOLT_REQUIRE(ctx, n % 2 == 0, "the alpha fold halves its vectors: n is even");
        JOLT_REQUIRE(ctx, view_ok(ctx, a, JOLT_DORY_KIND_FR, a_first, n) && view_ok(ctx, b, JOLT_DORY_KIND_FR, b_first, n), "s1 / s2 is not an Fr view of this context");
        JOLT_REQUIRE(ctx, a != b, "s1 and s2 are one vector");
    } else {
        JOLT_REQUIRE(ctx, view_ok(ctx, a, JOLT_DORY_KIND_G1, a_first, n) && view_ok(ctx, b, JOLT_DORY_KIND_G2, b_first, n), "Gamma1 / Gamma2 is not a G1 / G2 view of this context");
        JOLT_REQUIRE(ctx, !views_overlap(v1, v1_first, a, a_first, n) && !views_overlap(v2, v2_first, b, b_first, n), "a vector's view overlaps its bases");
    }
    NafPlan plan, plan_inv;
    JOLT_REQUIRE(ctx, naf_plan(scalar, &plan) && naf_plan(scalar_inv, &plan_inv), "scalar is not a canonical Fr");
    const Fr s = fr_from_abi(scalar), s_inv = fr_from_abi(scalar_inv);
    JOLT_REQUIRE(ctx, mul(s, s_inv) == Fr::one(), "the scalar times its inverse is not one");
    const size_t h = n / 2, m = alpha ? h : n;
    if (m != 0) {
        Fork fork(ctx, 1);  // the G2 work beside the G1 work
        hipStream_t main_st = ctx->stream, g2_st = fork.st[0];
        hipError_t e = fork.e;
        G1Jac* p1 = at<G1Jac>(v1, v1_first);
        G2Jac* p2 = at<G2Jac>(v2, v2_first);
        if (alpha) {
            if (e == hipSuccess) e = enqueue_scale_add<G1Ops>(main_st, plan, p1, p1 + h, p1, h);
            if (e == hipSuccess) e = enqueue_fold_field(main_st, at<Fr>(a, a_first), at<Fr>(a, a_first) + h, s, h);
            if (e == hipSuccess) e = enqueue_scale_add<G2Ops>(g2_st, plan_inv, p2, p2 + h, p2, h);
            if (e == hipSuccess) e = enqueue_fold_field(g2_st, at<Fr>(b, b_first), at<Fr>(b, b_first) + h, s_inv, h);
        } else {
            if (e == hipSuccess) e = enqueue_scale_add<G1Ops>(main_st, plan, at<G1Jac>(a, a_first), p1, p1, n);
            if (e == hipSuccess) e = enqueue_scale_add<G2Ops>(g2_st, plan_inv, at<G2Jac>(b, b_first), p2, p2, n);
        }
        e = fork.join(e);
        if (e != hipSuccess) return hip_fail(ctx, "dory round update", e);
    }
    if (alpha) {
        v1->len = v1_first + h;
        v2->len = v2_first + h;
        a->len = a_first + h;
        b->len = b_first + h;
    }
    return JOLT_OK;
}

// ------------------------------------------------------------------------------------------------------------------ the byte forms
namespace {

void put_le32(uint8_t* out, const Fq& canonical) {
    for (int i = 0; i < 8; ++i)
        for (int j = 0; j < 4; ++j) out[4 * i + j] = (uint8_t)(canonical.l[i] >> (8 * j));
}
// a > b as canonical integers
int cmp_canonical(const Fq& a, const Fq& b) {
    for (int i = 7; i >= 0; --i)
        if (a.l[i] != b.l[i]) return a.l[i] > b.l[i] ? 1 : -1;
    return 0;
}
Fq2 fq2_inverse(const Fq2& a) {  // (c0 - c1 u) / (c0^2 + c1^2)
    const Fq d = inv(add(sqr(a.c0), sqr(a.c1)));
    Fq2 r;
    r.c0 = mul(a.c0, d);
    r.c1 = neg(mul(a.c1, d));
    return r;
}

}  // namespace

extern "C" int32_t jolt_host_g2_serialize_compressed(const jolt_g2_t* p, uint8_t out[64]) {
    if (!p || !out) return JOLT_ERR_INVALID_ARG;
    G2Jac a;
    std::memcpy(&a, p, sizeof(a));
    if (!fq2_is_canonical(a.x) || !fq2_is_canonical(a.y) || !fq2_is_canonical(a.z)) return JOLT_ERR_INVALID_ARG;
    std::memset(out, 0, 64);
    if (g2_is_identity(a)) {
        out[63] |= 0x40;
        return JOLT_OK;
    }
    const Fq2 zi = fq2_inverse(a.z), zi2 = sqr(zi);
    const Fq2 x = mul(a.x, zi2), y = mul(a.y, mul(zi2, zi));
    put_le32(out, from_mont(x.c0));
    put_le32(out + 32, from_mont(x.c1));
    const Fq2 ny = neg(y);
    int c = cmp_canonical(from_mont(y.c1), from_mont(ny.c1));  // Fp2's order: c1 first, then c0
    if (c == 0) c = cmp_canonical(from_mont(y.c0), from_mont(ny.c0));
    if (c > 0) out[63] |= 0x80;
    return JOLT_OK;
}

extern "C" int32_t jolt_host_gt_serialize(const jolt_gt_t* f, uint8_t out[384]) {
    if (!f || !out) return JOLT_ERR_INVALID_ARG;
    Fq c[12];
    std::memcpy(c, f, sizeof(c));
    for (int k = 0; k < 12; ++k) {
        Fq d;
        if (sub_p(d, c[k]) == 0) return JOLT_ERR_INVALID_ARG;
    }
    for (int k = 0; k < 12; ++k) put_le32(out + 32 * k, from_mont(c[k]));
    return JOLT_OK;
}

namespace {
constexpr const char* kDoryGroupLabel = "dory_group";  // crates/jolt-dory/src/transcript.rs:51
int32_t append_group(jolt_host_transcript* t, const uint8_t* bytes, size_t n) {
    JOLT_TRY(jolt_host_transcript_append_label(t, kDoryGroupLabel, 1, n));
    return jolt_host_transcript_append_bytes(t, bytes, n);
}
}  // namespace

extern "C" int32_t jolt_host_dory_transcript_append_gt(jolt_host_transcript* t, const jolt_gt_t* element) {
    if (!t || !element) return JOLT_ERR_INVALID_ARG;
    uint8_t bytes[384];
    JOLT_TRY(jolt_host_gt_serialize(element, bytes));
    return append_group(t, bytes, sizeof(bytes));
}
extern "C" int32_t jolt_host_dory_transcript_append_g1(jolt_host_transcript* t, const jolt_g1_t* element) {
    if (!t || !element) return JOLT_ERR_INVALID_ARG;
    uint8_t bytes[32];
    JOLT_TRY(jolt_host_g1_serialize_compressed(element, bytes));
    return append_group(t, bytes, sizeof(bytes));
}
extern "C" int32_t jolt_host_dory_transcript_append_g2(jolt_host_transcript* t, const jolt_g2_t* element) {
    if (!t || !element) return JOLT_ERR_INVALID_ARG;
    uint8_t bytes[64];
    JOLT_TRY(jolt_host_g2_serialize_compressed(element, bytes));
    return append_group(t, bytes, sizeof(bytes));
}

extern "C" int32_t jolt_host_dory_proof_counts(uint32_t sigma, size_t* n_gt, size_t* n_g1, size_t* n_g2, size_t* n_challenges) {
    if (sigma > kMaxSigma) return JOLT_ERR_INVALID_ARG;
    if (n_gt) *n_gt = 2 + 6 * (size_t)sigma;
    if (n_g1) *n_g1 = 2 + 3 * (size_t)sigma;
    if (n_g2) *n_g2 = 1 + 3 * (size_t)sigma;
    if (n_challenges) *n_challenges = 2 * (size_t)sigma + 1;
    return JOLT_OK;
}

// ------------------------------------------------------------------------------------------------------------------ the evaluation proof
namespace {

// the state vectors of one opening.  Work of this call may still be in flight on the main stream or on a side stream when an exit is taken (a transcript abort after a
// message, a failed enqueue between a fork and its join): the streams are drained BEFORE the blocks go back to the pool, which hands them out again unsynchronised.
struct OpenState {
    jolt_ctx* ctx;
    jolt_dory_vec *v1 = nullptr, *v2 = nullptr, *s1 = nullptr, *s2 = nullptr, *v = nullptr;
    explicit OpenState(jolt_ctx* c) : ctx(c) {}
    ~OpenState() {
        (void)hipStreamSynchronize(ctx->stream);
        for (hipStream_t st : ctx->side)
            if (st) (void)hipStreamSynchronize(st);
        for (jolt_dory_vec* x : {v1, v2, s1, s2, v}) (void)jolt_dory_vec_free(ctx, x);
    }
};

jolt_dory_item pair_item(const jolt_dory_vec* a, size_t a_first, const jolt_dory_vec* b, size_t b_first, size_t n) {
    return jolt_dory_item{JOLT_DORY_PAIR, a, a_first, b, b_first, nullptr, 0, n};
}
jolt_dory_item pair_prepared(const jolt_dory_vec* a, size_t a_first, const jolt_g2_prepared* prepared, size_t n) {
    return jolt_dory_item{JOLT_DORY_PAIR, a, a_first, nullptr, 0, prepared, 0, n};
}
jolt_dory_item msm_item(int32_t op, const jolt_dory_vec* pts, size_t pts_first, const jolt_dory_vec* scalars, size_t scalars_first, size_t n) {
    return jolt_dory_item{op, pts, pts_first, scalars, scalars_first, nullptr, 0, n};
}
void take_gt(jolt_gt_t* out, const jolt_dory_result& r) { std::memcpy(out, &r, sizeof(*out)); }
void take_g1(jolt_g1_t* out, const jolt_dory_result& r) { std::memcpy(out, &r, sizeof(*out)); }
void take_g2(jolt_g2_t* out, const jolt_dory_result& r) { std::memcpy(out, &r, sizeof(*out)); }

// the challenge a callback handed back: canonical, not zero; its inverse
int32_t challenge_pair(jolt_ctx* ctx, const jolt_fr_t* c, jolt_fr_t* c_inv) {
    const Fr x = fr_from_abi(c);
    JOLT_REQUIRE(ctx, fr_is_canonical(x), "the transcript returned a challenge that is not a canonical Fr");
    if (x.is_zero()) {
        ctx->last_error = "the transcript returned a zero challenge";
        return JOLT_ERR_NOT_INVERTIBLE;
    }
    fr_to_abi(c_inv, inv(x));
    return JOLT_OK;
}

int32_t open_impl(jolt_ctx* ctx, const jolt_dory_setup* setup, const jolt_dory_vec* const* hints, const size_t* hint_first, const size_t* hint_rows, size_t n_hints,
                  const jolt_fr_t* scalars, const jolt_table* v_table, const jolt_table* left, const jolt_table* right, uint32_t nu, uint32_t sigma, jolt_dory_transcript_fn fn,
                  void* user, jolt_gt_t* gts, jolt_g1_t* g1s, jolt_g2_t* g2s, jolt_fr_t* challenges_out) {
    if (!ctx || !setup || !hints || !hint_first || !hint_rows || !scalars || !v_table || !left || !right || !fn || !gts || !g1s || !g2s || !challenges_out) return JOLT_ERR_INVALID_ARG;
    // ---- every check before anything is enqueued ----
    JOLT_REQUIRE(ctx, setup->ctx == ctx, "the setup belongs to another context");
    JOLT_REQUIRE(ctx, nu <= sigma && sigma <= kMaxSigma, "the matrix of a Dory opening has at most as many rows as columns: nu <= sigma <= 30");
    const size_t rows = (size_t)1 << nu, n = (size_t)1 << sigma;
    if (n > setup->n) {
        ctx->last_error = "the setup holds fewer than 2^sigma bases";
        return JOLT_ERR_SRS_TOO_SMALL;
    }
    JOLT_REQUIRE(ctx, n_hints != 0, "an opening combines at least one hint");
    if (n_hints > (size_t)0x00FFFFFFu) return JOLT_ERR_UNSUPPORTED;
    for (size_t i = 0; i < n_hints; ++i)
        JOLT_REQUIRE(ctx, view_ok(ctx, hints[i], JOLT_DORY_KIND_G1, hint_first[i], hint_rows[i]) && hint_rows[i] <= rows, "a hint is a G1 view of this context of at most 2^nu rows");
    JOLT_REQUIRE(ctx, all_canonical(scalars, n_hints), "scalar is not a canonical Fr");
    JOLT_REQUIRE(ctx, table_ok(ctx, v_table, n) && table_ok(ctx, right, n) && table_ok(ctx, left, rows), "v and right have 2^sigma entries, left has 2^nu, on this context");

    // ---- the state: v1 = the combined hints padded with identities, v2[i] = v[i] H2, s1 = R, s2 = L padded with zeros ----
    OpenState st(ctx);
    JOLT_TRY(jolt_dory_state_alloc(ctx, JOLT_DORY_KIND_G1, n, &st.v1));
    JOLT_TRY(jolt_dory_state_combine_hints(ctx, hints, hint_first, hint_rows, n_hints, scalars, st.v1, 0));
    JOLT_TRY(jolt_dory_state_alloc(ctx, JOLT_DORY_KIND_FR, n, &st.s1));
    JOLT_TRY(jolt_dory_state_alloc(ctx, JOLT_DORY_KIND_FR, n, &st.s2));
    JOLT_TRY(jolt_dory_state_alloc(ctx, JOLT_DORY_KIND_FR, n, &st.v));
    JOLT_TRY(jolt_dory_state_from_table(ctx, right, 0, st.s1, 0, n));
    JOLT_TRY(jolt_dory_state_from_table(ctx, left, 0, st.s2, 0, rows));
    JOLT_TRY(jolt_dory_state_from_table(ctx, v_table, 0, st.v, 0, n));
    JOLT_TRY(jolt_dory_state_alloc(ctx, JOLT_DORY_KIND_G2, n, &st.v2));
    JOLT_TRY(jolt_dory_state_fixed_base_mul(ctx, JOLT_DORY_KIND_G2, &setup->h2, st.v, 0, st.v2, 0, n));

    jolt_dory_result res[6];
    jolt_fr_t ignored = {};
    size_t n_gt = 0, n_g1 = 0, n_g2 = 0;
    // ---- the VMV message: C = <v1, v2>, D2 = <Gamma1, v2>, E1 = <v1, s2> ----
    {
        const jolt_dory_item items[3] = {pair_item(st.v1, 0, st.v2, 0, n), pair_item(setup->gamma1, 0, st.v2, 0, n), msm_item(JOLT_DORY_MSM_G1, st.v1, 0, st.s2, 0, n)};
        JOLT_TRY(jolt_dory_products(ctx, items, 3, res));
        take_gt(&gts[0], res[0]);
        take_gt(&gts[1], res[1]);
        take_g1(&g1s[0], res[2]);
        JOLT_TRY(fn(user, JOLT_DORY_PHASE_VMV, 0, gts, 2, g1s, 1, g2s, 0, &ignored));
        n_gt = 2;
        n_g1 = 1;
    }
    // ---- sigma rounds of Dory-Reduce ----
    size_t m = n;
    for (uint32_t k = 0; k < sigma; ++k) {
        const size_t h = m / 2;
        jolt_fr_t beta, beta_inv, alpha, alpha_inv;
        {
            const jolt_dory_item items[6] = {pair_prepared(st.v1, 0, setup->prepared, h), pair_prepared(st.v1, h, setup->prepared, h),
                                             pair_item(setup->gamma1, 0, st.v2, 0, h),    pair_item(setup->gamma1, 0, st.v2, h, h),
                                             msm_item(JOLT_DORY_MSM_G1, setup->gamma1, 0, st.s2, 0, m), msm_item(JOLT_DORY_MSM_G2, setup->gamma2, 0, st.s1, 0, m)};
            JOLT_TRY(jolt_dory_products(ctx, items, 6, res));
            for (int j = 0; j < 4; ++j) take_gt(&gts[n_gt + j], res[j]);
            take_g1(&g1s[n_g1], res[4]);
            take_g2(&g2s[n_g2], res[5]);
            JOLT_TRY(fn(user, JOLT_DORY_PHASE_FIRST, k, gts + n_gt, 4, g1s + n_g1, 1, g2s + n_g2, 1, &beta));
            n_gt += 4;
            n_g1 += 1;
            n_g2 += 1;
        }
        JOLT_TRY(challenge_pair(ctx, &beta, &beta_inv));
        challenges_out[2 * k] = beta;
        JOLT_TRY(jolt_dory_round_update(ctx, JOLT_DORY_UPDATE_BETA, st.v1, 0, st.v2, 0, setup->gamma1, 0, setup->gamma2, 0, m, &beta, &beta_inv));
        {
            const jolt_dory_item items[6] = {pair_item(st.v1, 0, st.v2, h, h), pair_item(st.v1, h, st.v2, 0, h),
                                             msm_item(JOLT_DORY_MSM_G1, st.v1, 0, st.s2, h, h), msm_item(JOLT_DORY_MSM_G1, st.v1, h, st.s2, 0, h),
                                             msm_item(JOLT_DORY_MSM_G2, st.v2, h, st.s1, 0, h), msm_item(JOLT_DORY_MSM_G2, st.v2, 0, st.s1, h, h)};
            JOLT_TRY(jolt_dory_products(ctx, items, 6, res));
            take_gt(&gts[n_gt], res[0]);
            take_gt(&gts[n_gt + 1], res[1]);
            take_g1(&g1s[n_g1], res[2]);
            take_g1(&g1s[n_g1 + 1], res[3]);
            take_g2(&g2s[n_g2], res[4]);
            take_g2(&g2s[n_g2 + 1], res[5]);
            JOLT_TRY(fn(user, JOLT_DORY_PHASE_SECOND, k, gts + n_gt, 2, g1s + n_g1, 2, g2s + n_g2, 2, &alpha));
            n_gt += 2;
            n_g1 += 2;
            n_g2 += 2;
        }
        JOLT_TRY(challenge_pair(ctx, &alpha, &alpha_inv));
        challenges_out[2 * k + 1] = alpha;
        JOLT_TRY(jolt_dory_round_update(ctx, JOLT_DORY_UPDATE_ALPHA, st.v1, 0, st.v2, 0, st.s1, 0, st.s2, 0, m, &alpha, &alpha_inv));
        m = h;
    }
    // ---- fold-scalars under gamma, the final message: w1 = v1 + (gamma s1) H1, w2 = v2 + (s2 / gamma) H2 over the single remaining elements ----
    jolt_fr_t gamma, gamma_inv;
    JOLT_TRY(fn(user, JOLT_DORY_PHASE_GAMMA, sigma, gts + n_gt, 0, g1s + n_g1, 0, g2s + n_g2, 0, &gamma));
    JOLT_TRY(challenge_pair(ctx, &gamma, &gamma_inv));
    challenges_out[2 * (size_t)sigma] = gamma;
    jolt_fr_t s1, s2;
    JOLT_TRY(jolt_dory_vec_download(ctx, st.s1, 0, 1, &s1));
    JOLT_TRY(jolt_dory_vec_download(ctx, st.s2, 0, 1, &s2));
    jolt_fr_t k1, k2;
    fr_to_abi(&k1, mul(fr_from_abi(&gamma), fr_from_abi(&s1)));
    fr_to_abi(&k2, mul(fr_from_abi(&gamma_inv), fr_from_abi(&s2)));
    JOLT_TRY(jolt_dory_vec_scale_bases_add(ctx, setup->h1_vec, 0, st.v1, 0, 1, &k1));
    JOLT_TRY(jolt_dory_vec_scale_bases_add(ctx, setup->h2_vec, 0, st.v2, 0, 1, &k2));
    JOLT_TRY(jolt_dory_vec_download(ctx, st.v1, 0, 1, &g1s[n_g1]));
    JOLT_TRY(jolt_dory_vec_download(ctx, st.v2, 0, 1, &g2s[n_g2]));
    return fn(user, JOLT_DORY_PHASE_FINAL, sigma, gts + n_gt, 0, g1s + n_g1, 1, g2s + n_g2, 1, &ignored);
}

}  // namespace

// the library's engines behind the callback: every element as JoltToDoryTranscript::append_group, every challenge Transcript::challenge_scalar.  The verifier's d
// (JOLT_DORY_PHASE_D) comes from a COPY of the transcript: the caller's stays where the prover's is after the final message
int32_t jolt::dory_host::engine_fn(void* user, int32_t phase, size_t, const jolt_gt_t* gts, size_t n_gt, const jolt_g1_t* g1s, size_t n_g1, const jolt_g2_t* g2s, size_t n_g2, jolt_fr_t* challenge_out) {
    jolt_host_transcript* t = (jolt_host_transcript*)user;
    for (size_t i = 0; i < n_gt; ++i) JOLT_TRY(jolt_host_dory_transcript_append_gt(t, &gts[i]));
    for (size_t i = 0; i < n_g1; ++i) JOLT_TRY(jolt_host_dory_transcript_append_g1(t, &g1s[i]));
    for (size_t i = 0; i < n_g2; ++i) JOLT_TRY(jolt_host_dory_transcript_append_g2(t, &g2s[i]));
    if (phase == JOLT_DORY_PHASE_FIRST || phase == JOLT_DORY_PHASE_SECOND || phase == JOLT_DORY_PHASE_GAMMA) return jolt_host_transcript_challenge(t, 1, challenge_out);
    if (phase == JOLT_DORY_PHASE_D) {
        jolt_host_transcript* copy = nullptr;
        JOLT_TRY(jolt_host_transcript_clone(t, &copy));
        const int32_t rc = jolt_host_transcript_challenge(copy, 1, challenge_out);
        (void)jolt_host_transcript_destroy(copy);
        return rc;
    }
    return JOLT_OK;
}

extern "C" int32_t jolt_host_dory_open_with_transcript(jolt_ctx* ctx, const jolt_dory_setup* setup, const jolt_dory_vec* const* hints, const size_t* hint_first,
                                                       const size_t* hint_rows, size_t n_hints, const jolt_fr_t* scalars, const jolt_table* v_table, const jolt_table* left,
                                                       const jolt_table* right, uint32_t nu, uint32_t sigma, jolt_dory_transcript_fn fn, void* user, jolt_gt_t* gts,
                                                       jolt_g1_t* g1s, jolt_g2_t* g2s, jolt_fr_t* challenges_out) {
    return open_impl(ctx, setup, hints, hint_first, hint_rows, n_hints, scalars, v_table, left, right, nu, sigma, fn, user, gts, g1s, g2s, challenges_out);
}

extern "C" int32_t jolt_host_dory_open(jolt_ctx* ctx, const jolt_dory_setup* setup, const jolt_dory_vec* const* hints, const size_t* hint_first, const size_t* hint_rows,
                                       size_t n_hints, const jolt_fr_t* scalars, const jolt_table* v_table, const jolt_table* left, const jolt_table* right, uint32_t nu,
                                       uint32_t sigma, jolt_host_transcript* t, jolt_gt_t* gts, jolt_g1_t* g1s, jolt_g2_t* g2s, jolt_fr_t* challenges_out) {
    if (!t) return JOLT_ERR_INVALID_ARG;
    return open_impl(ctx, setup, hints, hint_first, hint_rows, n_hints, scalars, v_table, left, right, nu, sigma, engine_fn, t, gts, g1s, g2s, challenges_out);
}

// ------------------------------------------------------------------------------------------------------------------ the batch opening of stage 8
namespace {

// the tables one batch opening makes (L, R, the trace's fold under a batch with blocks, v).  As OpenState: the streams are drained before the blocks go back to the pool.
struct BatchTables {
    jolt_ctx* ctx;
    jolt_table *left = nullptr, *right = nullptr, *trace = nullptr, *v = nullptr;
    explicit BatchTables(jolt_ctx* c) : ctx(c) {}
    ~BatchTables() {
        (void)hipStreamSynchronize(ctx->stream);
        for (hipStream_t st : ctx->side)
            if (st) (void)hipStreamSynchronize(st);
        for (jolt_table* x : {left, right, trace, v})
            if (x) (void)jolt_table_free(ctx, x);
    }
};

// eq(r[0 .. n)) as a device table; n = 0 is the table (1)
int32_t eq_table(jolt_ctx* ctx, const jolt_fr_t* r, size_t n, jolt_table** out) {
    if (n) return jolt_eq_evals(ctx, r, n, nullptr, out);
    jolt_fr_t one;
    fr_to_abi(&one, Fr::one());
    return jolt_table_upload(ctx, &one, 1, out);
}

}  // namespace

// The one body of both entries.  n_blocks = 0 in the cycle-major placement is jolt_host_dory_prove_batch as it always was: the same checks in the same order, the
// same launches, the same bytes.
static int32_t prove_batch_impl(jolt_ctx* ctx, const jolt_dory_setup* setup, const jolt_dory_vec* const* hints, const size_t* hint_first, const size_t* hint_rows, size_t n_claims,
                                const jolt_fr_t* evaluations, const jolt_onehot* const* sources, size_t n_sources, jolt_table* const* dense, size_t n_dense,
                                jolt_table* const* blocks, const uint32_t* sigma_blocks, size_t n_blocks, uint32_t log_k, int32_t order, uint32_t log_extra,
                                const size_t* column_of_claim, const jolt_fr_t* point, size_t n_point, jolt_host_transcript* t, jolt_gt_t* gts, jolt_g1_t* g1s, jolt_g2_t* g2s,
                                jolt_fr_t* challenges_out, jolt_fr_t* scalars_out, jolt_fr_t* joint_eval_out) {
    if (!ctx || !setup || !hints || !hint_first || !hint_rows || !evaluations || !point || !t || !gts || !g1s || !g2s || !challenges_out || !scalars_out || !joint_eval_out ||
        (n_sources && !sources) || (n_dense && !dense) || (n_blocks && (!blocks || !sigma_blocks)))
        return JOLT_ERR_INVALID_ARG;
    // ---- every check of this entry, of the row folds and of the opening, before the transcript absorbs anything and before anything is enqueued ----
    JOLT_REQUIRE(ctx, setup->ctx == ctx, "the setup belongs to another context");
    JOLT_REQUIRE(ctx, n_claims != 0, "an empty batch");  // HomomorphicBatchStatement::new refuses it
    // the limits of jolt_dory_fold_rows_grid, of jolt_dory_fold_rows_blocks_many and of the hint combination
    if (n_sources > 4 || n_dense > 8 || n_blocks > 256 || log_k > 8 || n_claims > (size_t)0x00FFFFFFu) return JOLT_ERR_UNSUPPORTED;
    const bool address_major = order == JOLT_DORY_ORDER_ADDRESS_MAJOR;
    JOLT_REQUIRE(ctx, address_major || order == JOLT_DORY_ORDER_CYCLE_MAJOR, "the order is cycle-major or address-major");
    JOLT_REQUIRE(ctx, address_major ? log_extra <= 32 : log_extra == 0, "log_extra widens the address-major grid only");
    for (size_t s = 0; s < n_sources; ++s) JOLT_REQUIRE(ctx, sources[s] && sources[s]->ctx == ctx, "a source is null or of another context");
    for (size_t d = 0; d < n_dense; ++d) JOLT_REQUIRE(ctx, dense[d] && dense[d]->ctx == ctx && dense[d]->data(), "a dense column is null or of another context");
    for (size_t d = 0; d < n_blocks; ++d) JOLT_REQUIRE(ctx, blocks[d] && blocks[d]->ctx == ctx && blocks[d]->data(), "a block is null or of another context");
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
    const size_t n_trace = n_onehot + n_dense;
    JOLT_REQUIRE(ctx, n_claims == n_trace + n_blocks, "one claim per column of the joint polynomial");
    JOLT_REQUIRE(ctx, n_point == (size_t)log_k + log_extra + log_t, "the point has one coordinate per variable of the grid");
    const uint32_t sigma = (uint32_t)((n_point + 1) / 2), nu = (uint32_t)n_point - sigma;  // crates/jolt-dory/src/scheme.rs:242-243
    JOLT_REQUIRE(ctx, sigma <= kMaxSigma, "sigma <= 30");
    if (address_major && sigma < log_k + log_extra) return JOLT_ERR_UNSUPPORTED;  // a cycle's block wider than a matrix row (jolt_dory_fold_rows_grid_am)
    const size_t rows = (size_t)1 << nu, n = (size_t)1 << sigma;
    if (n > setup->n) {
        ctx->last_error = "the setup holds fewer than 2^sigma bases";
        return JOLT_ERR_SRS_TOO_SMALL;
    }
    for (size_t i = 0; i < n_claims; ++i)
        JOLT_REQUIRE(ctx, view_ok(ctx, hints[i], JOLT_DORY_KIND_G1, hint_first[i], hint_rows[i]) && hint_rows[i] <= rows, "a hint is a G1 view of this context of at most 2^nu rows");
    JOLT_REQUIRE(ctx, all_canonical(evaluations, n_claims) && all_canonical(point, n_point), "an evaluation or a coordinate is not a canonical Fr");
    std::vector<size_t> column(n_claims);
    {
        std::vector<uint8_t> seen(n_claims, 0);
        for (size_t i = 0; i < n_claims; ++i) {
            const size_t c = column_of_claim ? column_of_claim[i] : i;
            JOLT_REQUIRE(ctx, c < n_claims && !seen[c], "column_of_claim is not a permutation of the columns");
            seen[c] = 1;
            column[i] = c;
        }
    }
    {  // a block: 2^m_d entries as 2^(m_d - sigma_d) rows of 2^sigma_d columns inside the grid, its hint one row commitment per row (jolt_dory_fold_rows_blocks' codes)
        std::vector<size_t> block_rows(n_blocks);
        for (size_t d = 0; d < n_blocks; ++d) {
            const size_t len = blocks[d]->len;
            JOLT_REQUIRE(ctx, len != 0 && (len & (len - 1)) == 0, "a block's length must be a power of two");
            uint32_t m = 0;
            while (((size_t)1 << m) < len) ++m;
            JOLT_REQUIRE(ctx, sigma_blocks[d] <= m && sigma_blocks[d] <= sigma, "a block's columns exceed its variables or the grid's");
            block_rows[d] = (size_t)1 << (m - sigma_blocks[d]);
            if (block_rows[d] > rows) return JOLT_ERR_SIZE_MISMATCH;
        }
        for (size_t i = 0; i < n_claims; ++i)
            if (column[i] >= n_trace) JOLT_REQUIRE(ctx, hint_rows[i] == block_rows[column[i] - n_trace], "a block's hint has one row commitment per row of the block");
    }
    // ---- the statement: rlc_claims, the evaluations, gamma's powers; joint_eval = sum_i gamma^i y_i ----
    JOLT_TRY(jolt_host_opening_statement_absorb(t, evaluations, n_claims, scalars_out));
    Fr joint = Fr::zero();
    for (size_t i = 0; i < n_claims; ++i) joint = add(joint, mul(fr_from_abi(&scalars_out[i]), fr_from_abi(&evaluations[i])));
    fr_to_abi(joint_eval_out, joint);
    std::vector<jolt_fr_t> by_column(n_claims);  // the row folds take their scalars in column order
    for (size_t i = 0; i < n_claims; ++i) by_column[column[i]] = scalars_out[i];
    // ---- L = eq(point[:nu]), R = eq(point[nu:]), v = L^T M by the lazy row fold of the trace, then the blocks on top of it ----
    BatchTables tb(ctx);
    JOLT_TRY(eq_table(ctx, point, nu, &tb.left));
    JOLT_TRY(eq_table(ctx, point + nu, sigma, &tb.right));
    jolt_table** trace_out = n_blocks ? &tb.trace : &tb.v;
    if (address_major)
        JOLT_TRY(jolt_dory_fold_rows_grid_am(ctx, sources, n_sources, by_column.data(), dense, n_dense, by_column.data() + n_onehot, log_k + log_extra, log_extra, sigma, tb.left, trace_out));
    else
        JOLT_TRY(jolt_dory_fold_rows_grid(ctx, sources, n_sources, by_column.data(), dense, n_dense, by_column.data() + n_onehot, log_k, sigma, tb.left, trace_out));
    if (n_blocks) JOLT_TRY(jolt_dory_fold_rows_blocks_many(ctx, blocks, sigma_blocks, n_blocks, by_column.data() + n_trace, sigma, tb.left, tb.trace, &tb.v));
    // ---- <v, R> is the joint polynomial's evaluation at the point: a statement that does not hold is refused here, before any state vector is built ----
    jolt_fr_t y;
    JOLT_TRY(jolt_table_dot(ctx, tb.v, tb.right, 0, &y));
    if (!(fr_from_abi(&y) == joint)) {
        ctx->last_error = "the claimed evaluations do not combine to the joint polynomial's evaluation at the point";
        return JOLT_ERR_ROUND_CHECK;
    }
    JOLT_TRY(open_impl(ctx, setup, hints, hint_first, hint_rows, n_claims, scalars_out, tb.v, tb.left, tb.right, nu, sigma, engine_fn, t, gts, g1s, g2s, challenges_out));
    return jolt_host_opening_claim_absorb(t, point, n_point, joint_eval_out);
}

extern "C" int32_t jolt_host_dory_prove_batch_blocks(jolt_ctx* ctx, const jolt_dory_setup* setup, const jolt_dory_vec* const* hints, const size_t* hint_first,
                                                     const size_t* hint_rows, size_t n_claims, const jolt_fr_t* evaluations, const jolt_onehot* const* sources, size_t n_sources,
                                                     jolt_table* const* dense, size_t n_dense, jolt_table* const* blocks, const uint32_t* sigma_blocks, size_t n_blocks,
                                                     uint32_t log_k, int32_t order, uint32_t log_extra, const size_t* column_of_claim, const jolt_fr_t* point, size_t n_point,
                                                     jolt_host_transcript* t, jolt_gt_t* gts, jolt_g1_t* g1s, jolt_g2_t* g2s, jolt_fr_t* challenges_out, jolt_fr_t* scalars_out,
                                                     jolt_fr_t* joint_eval_out) {
    return prove_batch_impl(ctx, setup, hints, hint_first, hint_rows, n_claims, evaluations, sources, n_sources, dense, n_dense, blocks, sigma_blocks, n_blocks, log_k, order,
                            log_extra, column_of_claim, point, n_point, t, gts, g1s, g2s, challenges_out, scalars_out, joint_eval_out);
}

extern "C" int32_t jolt_host_dory_prove_batch(jolt_ctx* ctx, const jolt_dory_setup* setup, const jolt_dory_vec* const* hints, const size_t* hint_first, const size_t* hint_rows,
                                              size_t n_claims, const jolt_fr_t* evaluations, const jolt_onehot* const* sources, size_t n_sources, jolt_table* const* dense,
                                              size_t n_dense, uint32_t log_k, const size_t* column_of_claim, const jolt_fr_t* point, size_t n_point, jolt_host_transcript* t,
                                              jolt_gt_t* gts, jolt_g1_t* g1s, jolt_g2_t* g2s, jolt_fr_t* challenges_out, jolt_fr_t* scalars_out, jolt_fr_t* joint_eval_out) {
    return prove_batch_impl(ctx, setup, hints, hint_first, hint_rows, n_claims, evaluations, sources, n_sources, dense, n_dense, nullptr, nullptr, 0, log_k,
                            JOLT_DORY_ORDER_CYCLE_MAJOR, 0, column_of_claim, point, n_point, t, gts, g1s, g2s, challenges_out, scalars_out, joint_eval_out);
}
