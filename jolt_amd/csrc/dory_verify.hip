// jolt_amd/csrc/dory_verify.hip -- Dory verification: GT multi-exponentiation on the device, the verifier's precomputed GT values, and the verifier of an evaluation
// proof (and of the stage-8 batch) as one call.
//
// Replaces:
//   DoryScheme::combine (crates/jolt-dory/src/scheme.rs:313-323)                        -> jolt_dory_gt_multi_exp
//   DoryVerifierSetup (crates/jolt-dory/src/types.rs)                                   -> jolt_dory_verifier_setup_*
//   DoryScheme::verify (scheme.rs:277-308)                                              -> jolt_host_dory_verify, jolt_host_dory_verify_with_transcript
//   HomomorphicBatch::verify_batch (crates/jolt-openings/src/schemes.rs:526-551)        -> jolt_host_dory_verify_batch
//
// One new kernel, workgroups of one wavefront, one element per lane (the launch shape of every latency-bound Dory kernel, docs/kernels.md 3.5f):
//   k_gt_pow    gts[i]^scalars[i] by square-and-multiply over the canonical scalar.  Every lane runs the same 254 steps -- a squaring and a multiplication by
//               (bit ? base : one), so the loop is uniform over the wavefront and the accumulator is the only Fq12 that lives across a step: the base is
//               read from global memory again in every step, as k_tree_level reads its second operand.  GENERAL Fq12 sqr and mul (fq12.hip.h): a verifier's
//               inputs are not known to lie in the order-r subgroup, so no cyclotomic squaring and no Frobenius split of the exponent.
// The product of the powers is the halving tree of the multi-pairings (enqueue_tree<Fq12, MulFq12>).  Integer VALU work, no MFMA.
//
// The verifier (verify_impl) is host control flow: it replays the transcript over the proof's elements, folds s1 and s2, computes EVERY exponent of the final
// equation in Fr (jolt_host_dory_verify_exponents -- the right-hand side is then one multi-exponentiation), folds the group elements as one jolt_dory_products
// batch of MSM items, and takes both checks' left-hand sides from one batch of PAIR items.
#include <vector>

#include "ctx.hpp"
#include "dory_host.hpp"
#include "dory_kernels.hip.h"
#include "dory_prepared.hip.h"

using namespace jolt;
using namespace jolt::dory_host;
using namespace jolt::dory_dev;

static_assert(sizeof(jolt_gt_t) == sizeof(Fq12) && sizeof(Fq12) == 12 * sizeof(Fq), "GT ABI layout");

struct jolt_dory_verifier_setup {
    jolt_ctx* ctx = nullptr;
    size_t n = 0;
    uint32_t s = 0;                // n = 2^s
    std::vector<jolt_gt_t> values;  // 3 s + 4, the order of jolt_dory_verifier_setup_values
    jolt_g1_t gamma1_0;            // Gamma1[0], Gamma2[0]: the final check adds their multiples to w1 and w2
    jolt_g2_t gamma2_0;
    // jolt_dory_verifier_setup_timing: the phases of the last verification made with this object while timing was on
    mutable bool timing = false;
    mutable double ms[4] = {0.0, 0.0, 0.0, 0.0};
};

namespace jolt {
namespace dory_dev {

static __global__ __launch_bounds__(kLanes) void k_gt_pow(const Fq12* gts, const Fr* __restrict__ scalars, Fq12* __restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * kLanes + threadIdx.x;
    if (i >= n) return;
    Fr k = from_mont(scalars[i]);
    shl256<2>(k);  // r < 2^254: bit 253 to the top
    const Fq* base = (const Fq*)(gts + i);
    Fq12 acc = Fq12::one();
#pragma unroll 1
    for (int step = 0; step < 254; ++step) {
        acc = sqr(acc);
        const bool bit = (k.l[7] >> 31) != 0;
        shl256<1>(k);
        Fq12 b;  // bit ? base : one, coefficient by coefficient
        Fq* bc = (Fq*)&b;
#pragma unroll
        for (int j = 0; j < 12; ++j) {
            const Fq neutral = j == 0 ? Fq::one() : Fq::zero();
#pragma unroll
            for (int w = 0; w < 8; ++w) bc[j].l[w] = bit ? base[j].l[w] : neutral.l[w];
        }
        acc = mul(acc, b);
    }
    out[i] = acc;
}
inline hipError_t enqueue_gt_pow(hipStream_t st, const Fq12* d_gts, const Fr* d_scalars, Fq12* d_out, size_t n) {
    hipLaunchKernelGGL(k_gt_pow, dim3(dory_host::lanes_grid(n)), dim3(kLanes), 0, st, d_gts, d_scalars, d_out, n);
    return hipGetLastError();
}

}  // namespace dory_dev
}  // namespace jolt

namespace {

constexpr size_t kMaxPowers = (size_t)1 << 20;
constexpr uint32_t kMaxSigma = 30;
// The two entries over host pointers report into the clock of jolt_dory_pairing_timing: its phases are theirs (checks, host -> device, -, the kernel over the
// elements, the product tree, device -> host, -), with the power kernel in the Miller kernel's place
enum { kChecks = 0, kUpload = 1, kPowers = 3, kProduct = 4, kDownload = 5 };
// The phases of jolt_dory_verifier_setup_timing
enum { kReplay = 0, kFolds = 1, kPairings = 2, kMultiExp = 3 };

bool all_gt_canonical(const jolt_gt_t* gts, size_t n) {
    return parallel_all(n, [gts](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; ++i)
            if (!fq12_is_canonical(pt_from_abi<Fq12>(&gts[i]))) return false;
        return true;
    });
}

// the powers on the device in d_out (n > 0), after the checks
void enqueue_powers(HostCall& c, const jolt_gt_t* gts, const jolt_fr_t* scalars, size_t n, Fq12** d_out) {
    Fq12* d_gts = nullptr;
    Fr* d_scalars = nullptr;
    c.up(gts, n, &d_gts);
    c.up(scalars, n, &d_scalars);
    c.take(n, d_out);
    c.mark(kUpload);
    if (c.ok()) c.e = enqueue_gt_pow(c.st, d_gts, d_scalars, *d_out, n);
    c.mark(kPowers);
}

int32_t powers_checked(jolt_ctx* ctx, const jolt_gt_t* gts, const jolt_fr_t* scalars, size_t n) {
    JOLT_REQUIRE(ctx, all_gt_canonical(gts, n), "an Fq coordinate of a GT element is not canonical");
    JOLT_REQUIRE(ctx, all_canonical(scalars, n), "scalar is not a canonical Fr");
    return JOLT_OK;
}

}  // namespace

extern "C" int32_t jolt_dory_gt_pow_many(jolt_ctx* ctx, const jolt_gt_t* gts, const jolt_fr_t* scalars, size_t n, jolt_gt_t* outs) {
    if (!ctx || (n && (!gts || !scalars || !outs))) return JOLT_ERR_INVALID_ARG;
    if (n > kMaxPowers) return JOLT_ERR_UNSUPPORTED;
    if (n == 0) return JOLT_OK;
    HostCall c(ctx, ctx->pairing_ms, ctx->pairing_timing);
    JOLT_TRY(powers_checked(ctx, gts, scalars, n));
    c.mark(kChecks, false);
    Fq12* d_out = nullptr;
    enqueue_powers(c, gts, scalars, n, &d_out);
    c.down(outs, d_out, n);
    return c.finish("dory gt_pow_many", kDownload);
}

extern "C" int32_t jolt_dory_gt_multi_exp(jolt_ctx* ctx, const jolt_gt_t* gts, const jolt_fr_t* scalars, size_t n, jolt_gt_t* out) {
    if (!ctx || !out || (n && (!gts || !scalars))) return JOLT_ERR_INVALID_ARG;
    if (n > kMaxPowers) return JOLT_ERR_UNSUPPORTED;
    Fq12 r = Fq12::one();
    if (n) {
        HostCall c(ctx, ctx->pairing_ms, ctx->pairing_timing);
        JOLT_TRY(powers_checked(ctx, gts, scalars, n));
        c.mark(kChecks, false);
        Fq12* d_f = nullptr;
        enqueue_powers(c, gts, scalars, n, &d_f);
        if (c.ok()) c.e = enqueue_tree<Fq12, MulFq12>(c.st, d_f, n);
        c.mark(kProduct);
        c.down(&r, d_f, 1);
        JOLT_TRY(c.finish("dory gt_multi_exp", kDownload));
    }
    std::memcpy(out, &r, sizeof(r));
    return JOLT_OK;
}

// ------------------------------------------------------------------------------------------------------------------ the verifier's setup
extern "C" int32_t jolt_dory_verifier_setup_free(jolt_ctx* ctx, jolt_dory_verifier_setup* vs) {
    if (!ctx) return JOLT_ERR_INVALID_ARG;
    if (!vs) return JOLT_OK;
    JOLT_REQUIRE(ctx, vs->ctx == ctx, "the verifier setup belongs to another context");
    delete vs;
    return JOLT_OK;
}

extern "C" int32_t jolt_dory_verifier_setup_create(jolt_ctx* ctx, const jolt_dory_setup* setup, jolt_dory_verifier_setup** out) {
    if (!ctx || !setup || !out) return JOLT_ERR_INVALID_ARG;
    JOLT_REQUIRE(ctx, setup->ctx == ctx, "the setup belongs to another context");
    uint32_t s = 0;
    while (((size_t)1 << s) < setup->n) ++s;
    std::vector<jolt_dory_item> items;
    const auto prepared = [&](size_t a_first, size_t p_first, size_t n) { items.push_back(jolt_dory_item{JOLT_DORY_PAIR, setup->gamma1, a_first, nullptr, 0, setup->prepared, p_first, n}); };
    for (uint32_t k = 0; k <= s; ++k) prepared(0, 0, setup->n >> k);                           // chi_k
    for (uint32_t k = 0; k < s; ++k) prepared(setup->n >> (k + 1), 0, setup->n >> (k + 1));    // Delta1R_k
    for (uint32_t k = 0; k < s; ++k) prepared(0, setup->n >> (k + 1), setup->n >> (k + 1));    // Delta2R_k
    items.push_back(jolt_dory_item{JOLT_DORY_PAIR, setup->h1_vec, 0, setup->h2_vec, 0, nullptr, 0, 1});   // HT
    items.push_back(jolt_dory_item{JOLT_DORY_PAIR, setup->h1_vec, 0, nullptr, 0, setup->prepared, 0, 1});  // e(H1, Gamma2[0])
    items.push_back(jolt_dory_item{JOLT_DORY_PAIR, setup->gamma1, 0, setup->h2_vec, 0, nullptr, 0, 1});   // e(Gamma1[0], H2)
    std::vector<jolt_dory_result> res(items.size());
    JOLT_TRY(jolt_dory_products(ctx, items.data(), items.size(), res.data()));
    jolt_dory_verifier_setup* vs = new (std::nothrow) jolt_dory_verifier_setup();
    if (!vs) return JOLT_ERR_OOM;
    vs->ctx = ctx;
    vs->n = setup->n;
    vs->s = s;
    vs->values.resize(items.size());
    for (size_t k = 0; k < items.size(); ++k) std::memcpy(&vs->values[k], &res[k], sizeof(jolt_gt_t));
    int32_t rc = jolt_dory_vec_download(ctx, setup->gamma1, 0, 1, &vs->gamma1_0);
    if (rc == JOLT_OK) rc = jolt_dory_vec_download(ctx, setup->gamma2, 0, 1, &vs->gamma2_0);
    if (rc != JOLT_OK) {
        delete vs;
        return rc;
    }
    *out = vs;
    return JOLT_OK;
}

extern "C" int32_t jolt_dory_verifier_setup_values(const jolt_dory_verifier_setup* vs, jolt_gt_t* out) {
    if (!vs || !out) return JOLT_ERR_INVALID_ARG;
    std::memcpy(out, vs->values.data(), vs->values.size() * sizeof(jolt_gt_t));
    return JOLT_OK;
}

extern "C" int32_t jolt_dory_verifier_setup_timing(const jolt_dory_verifier_setup* vs, int32_t enable, double* out_ms) {
    if (!vs) return JOLT_ERR_INVALID_ARG;
    if (out_ms)
        for (int k = 0; k < 4; ++k) out_ms[k] = vs->ms[k];
    vs->timing = enable != 0;
    return JOLT_OK;
}

// ------------------------------------------------------------------------------------------------------------------ the exponents
extern "C" int32_t jolt_host_dory_verify_exponents(uint32_t sigma, const jolt_fr_t* challenges, const jolt_fr_t* d, const jolt_fr_t* s1, const jolt_fr_t* s2, const jolt_fr_t* y,
                                                   jolt_fr_t* exp_proof_gt, jolt_fr_t* exp_commitment, jolt_fr_t* exp_setup, jolt_fr_t* coef_g1, jolt_fr_t* coef_g2,
                                                   jolt_fr_t* coef_h2) {
    if (!challenges || !d || !s1 || !s2 || !y || !exp_proof_gt || !exp_commitment || !exp_setup || !coef_g1 || !coef_g2 || !coef_h2 || sigma > kMaxSigma) return JOLT_ERR_INVALID_ARG;
    const size_t n_ch = 2 * (size_t)sigma + 1;
    if (!all_canonical(challenges, n_ch) || !all_canonical(d, 1) || !all_canonical(s1, 1) || !all_canonical(s2, 1) || !all_canonical(y, 1)) return JOLT_ERR_INVALID_ARG;
    std::vector<Fr> ch(n_ch), ch_inv(n_ch);
    for (size_t i = 0; i < n_ch; ++i) {
        ch[i] = fr_from_abi(&challenges[i]);
        if (ch[i].is_zero()) return JOLT_ERR_NOT_INVERTIBLE;
        ch_inv[i] = inv(ch[i]);
    }
    const Fr dd = fr_from_abi(d);
    if (dd.is_zero()) return JOLT_ERR_NOT_INVERTIBLE;
    const Fr d_inv = inv(dd), one = Fr::one();
    const Fr gamma = ch[2 * sigma], gamma_inv = ch_inv[2 * sigma];
    // d1_k and d2_k enter the right-hand side through c_{k+1} alone (d1_{k+1} and d2_{k+1} are built from the round's messages and the setup): their exponents are
    // 1 / beta_k and beta_k for k < sigma, and 1 / d and d for k = sigma
    const auto a_of = [&](uint32_t k) { return k < sigma ? ch_inv[2 * k] : d_inv; };
    const auto b_of = [&](uint32_t k) { return k < sigma ? ch[2 * k] : dd; };
    std::vector<Fr> chi(sigma + 1, one), delta1(sigma), delta2(sigma);
    fr_to_abi(&exp_proof_gt[0], one);      // C
    fr_to_abi(&exp_proof_gt[1], b_of(0));  // D2 = d2_0
    fr_to_abi(exp_commitment, a_of(0));    // d1_0
    fr_to_abi(&coef_g1[0], one);           // E1
    fr_to_abi(coef_h2, fr_from_abi(y));    // E2 = y H2
    for (uint32_t k = 0; k < sigma; ++k) {
        const Fr beta = ch[2 * k], beta_inv = ch_inv[2 * k], alpha = ch[2 * k + 1], alpha_inv = ch_inv[2 * k + 1];
        const Fr a = a_of(k + 1), b = b_of(k + 1);
        jolt_fr_t* e = exp_proof_gt + 2 + 6 * (size_t)k;
        fr_to_abi(&e[0], mul(a, alpha));      // D1L
        fr_to_abi(&e[1], a);                  // D1R
        fr_to_abi(&e[2], mul(b, alpha_inv));  // D2L
        fr_to_abi(&e[3], b);                  // D2R
        fr_to_abi(&e[4], alpha);              // C+
        fr_to_abi(&e[5], alpha_inv);          // C-
        chi[k + 1] = add(chi[k + 1], add(mul(a, mul(alpha, beta)), mul(b, mul(alpha_inv, beta_inv))));  // Delta1L = Delta2L = chi_{k+1}
        delta1[k] = mul(a, beta);
        delta2[k] = mul(b, beta_inv);
        fr_to_abi(&coef_g1[1 + 3 * (size_t)k], beta);
        fr_to_abi(&coef_g1[2 + 3 * (size_t)k], alpha);
        fr_to_abi(&coef_g1[3 + 3 * (size_t)k], alpha_inv);
        fr_to_abi(&coef_g2[3 * (size_t)k], beta_inv);
        fr_to_abi(&coef_g2[1 + 3 * (size_t)k], alpha);
        fr_to_abi(&coef_g2[2 + 3 * (size_t)k], alpha_inv);
    }
    for (uint32_t k = 0; k <= sigma; ++k) fr_to_abi(&exp_setup[k], chi[k]);
    for (uint32_t k = 0; k < sigma; ++k) {
        fr_to_abi(&exp_setup[sigma + 1 + k], delta1[k]);
        fr_to_abi(&exp_setup[2 * (size_t)sigma + 1 + k], delta2[k]);
    }
    const Fr f1 = fr_from_abi(s1), f2 = fr_from_abi(s2);
    fr_to_abi(&exp_setup[3 * (size_t)sigma + 1], mul(f1, f2));                       // HT
    fr_to_abi(&exp_setup[3 * (size_t)sigma + 2], mul(mul(gamma, f1), d_inv));        // e(H1, Gamma2[0]): D1'' = D1 + gamma s1 e(H1, Gamma2[0]), under 1 / d
    fr_to_abi(&exp_setup[3 * (size_t)sigma + 3], mul(mul(gamma_inv, f2), dd));       // e(Gamma1[0], H2): D2'' = D2 + (s2 / gamma) e(Gamma1[0], H2), under d
    return JOLT_OK;
}

// ------------------------------------------------------------------------------------------------------------------ the verifier
namespace {

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

int32_t challenge_checked(jolt_ctx* ctx, const jolt_fr_t* c) {
    const Fr x = fr_from_abi(c);
    JOLT_REQUIRE(ctx, fr_is_canonical(x), "the transcript returned a challenge that is not a canonical Fr");
    if (x.is_zero()) {
        ctx->last_error = "the transcript returned a zero challenge";
        return JOLT_ERR_NOT_INVERTIBLE;
    }
    return JOLT_OK;
}

// commitments[i] enters the multi-exponentiation with exponent weights[i] * exp_commitment: one commitment under weight one is DoryScheme::verify, a batch's
// commitments under gamma's powers are verify after combine
int32_t verify_impl(jolt_ctx* ctx, const jolt_dory_verifier_setup* vs, const jolt_dory_setup* setup, const jolt_gt_t* commitments, const jolt_fr_t* weights, size_t n_commitments,
                    const jolt_fr_t* y, const jolt_fr_t* left, const jolt_fr_t* right, uint32_t nu, uint32_t sigma, const jolt_gt_t* gts, const jolt_g1_t* g1s, const jolt_g2_t* g2s,
                    jolt_dory_transcript_fn fn, void* user, int32_t* accepted, int32_t* failed_check) {
    if (!ctx || !vs || !setup || !commitments || !weights || !y || !left || !right || !gts || !g1s || !g2s || !fn || !accepted || !failed_check) return JOLT_ERR_INVALID_ARG;
    // ---- every check before the transcript absorbs anything and before anything is enqueued ----
    JOLT_REQUIRE(ctx, setup->ctx == ctx && vs->ctx == ctx, "the setup belongs to another context");
    JOLT_REQUIRE(ctx, vs->n == setup->n, "the verifier setup was made from a setup of another size");
    JOLT_REQUIRE(ctx, nu <= sigma && sigma <= kMaxSigma, "the matrix of a Dory opening has at most as many rows as columns: nu <= sigma <= 30");
    const size_t rows = (size_t)1 << nu, n = (size_t)1 << sigma;
    if (n > setup->n) {
        ctx->last_error = "the setup holds fewer than 2^sigma bases";
        return JOLT_ERR_SRS_TOO_SMALL;
    }
    if (n_commitments > kMaxPowers - 64) return JOLT_ERR_UNSUPPORTED;
    const size_t n_gt = 2 + 6 * (size_t)sigma, n_g1 = 2 + 3 * (size_t)sigma, n_g2 = 1 + 3 * (size_t)sigma, n_setup = 3 * (size_t)sigma + 4;
    JOLT_REQUIRE(ctx, all_gt_canonical(gts, n_gt) && all_gt_canonical(commitments, n_commitments), "an Fq coordinate of a GT element is not canonical");
    JOLT_REQUIRE(ctx, all_on_curve<G1Ops>(g1s, n_g1) && all_on_curve<G2Ops>(g2s, n_g2), "a point is not on its curve or not canonical");
    JOLT_REQUIRE(ctx, all_canonical(y, 1) && all_canonical(left, rows) && all_canonical(right, n) && all_canonical(weights, n_commitments), "a field element is not a canonical Fr");

    auto t0 = std::chrono::steady_clock::now();
    const auto stamp = [&](int phase) {  // closes `phase`; every device phase below ends synchronised (jolt_dory_products, jolt_dory_gt_multi_exp)
        if (!vs->timing) return;
        const auto t1 = std::chrono::steady_clock::now();
        vs->ms[phase] = std::chrono::duration<double, std::milli>(t1 - t0).count();
        t0 = t1;
    };
    // ---- 1. the replay: beta_k, alpha_k, gamma, then d ----
    std::vector<jolt_fr_t> ch(2 * (size_t)sigma + 1);
    jolt_fr_t ignored = {}, d;
    size_t at_gt = 2, at_g1 = 1, at_g2 = 0;
    JOLT_TRY(fn(user, JOLT_DORY_PHASE_VMV, 0, gts, 2, g1s, 1, g2s, 0, &ignored));
    for (uint32_t k = 0; k < sigma; ++k) {
        JOLT_TRY(fn(user, JOLT_DORY_PHASE_FIRST, k, gts + at_gt, 4, g1s + at_g1, 1, g2s + at_g2, 1, &ch[2 * k]));
        JOLT_TRY(challenge_checked(ctx, &ch[2 * k]));
        at_gt += 4, at_g1 += 1, at_g2 += 1;
        JOLT_TRY(fn(user, JOLT_DORY_PHASE_SECOND, k, gts + at_gt, 2, g1s + at_g1, 2, g2s + at_g2, 2, &ch[2 * k + 1]));
        JOLT_TRY(challenge_checked(ctx, &ch[2 * k + 1]));
        at_gt += 2, at_g1 += 2, at_g2 += 2;
    }
    JOLT_TRY(fn(user, JOLT_DORY_PHASE_GAMMA, sigma, gts + at_gt, 0, g1s + at_g1, 0, g2s + at_g2, 0, &ch[2 * (size_t)sigma]));
    JOLT_TRY(challenge_checked(ctx, &ch[2 * (size_t)sigma]));
    JOLT_TRY(fn(user, JOLT_DORY_PHASE_FINAL, sigma, gts + at_gt, 0, g1s + at_g1, 1, g2s + at_g2, 1, &ignored));
    JOLT_TRY(fn(user, JOLT_DORY_PHASE_D, sigma, gts + at_gt, 0, g1s + at_g1, 0, g2s + at_g2, 0, &d));
    JOLT_TRY(challenge_checked(ctx, &d));

    // ---- 2. s1 from R under alpha, s2 from L (padded with zeros) under 1 / alpha ----
    jolt_fr_t s1_abi, s2_abi;
    {
        std::vector<Fr> s1(n), s2(n, Fr::zero());
        for (size_t i = 0; i < n; ++i) s1[i] = fr_from_abi(&right[i]);
        for (size_t i = 0; i < rows; ++i) s2[i] = fr_from_abi(&left[i]);
        size_t m = n;
        for (uint32_t k = 0; k < sigma; ++k) {
            const Fr alpha = fr_from_abi(&ch[2 * k + 1]), alpha_inv = inv(alpha);
            const size_t h = m / 2;
            for (size_t i = 0; i < h; ++i) {
                s1[i] = add(mul(alpha, s1[i]), s1[h + i]);
                s2[i] = add(mul(alpha_inv, s2[i]), s2[h + i]);
            }
            m = h;
        }
        fr_to_abi(&s1_abi, s1[0]);
        fr_to_abi(&s2_abi, s2[0]);
    }

    // ---- 3. every exponent ----
    std::vector<jolt_fr_t> exp_gt(n_gt), exp_setup(n_setup), coef_g1(1 + 3 * (size_t)sigma), coef_g2(3 * (size_t)sigma + 1);
    jolt_fr_t exp_commitment, coef_h2;
    JOLT_TRY(jolt_host_dory_verify_exponents(sigma, ch.data(), &d, &s1_abi, &s2_abi, y, exp_gt.data(), &exp_commitment, exp_setup.data(), coef_g1.data(), coef_g2.data() + 1, &coef_h2));
    coef_g2[0] = coef_h2;  // E2' = y H2 + ...: H2 leads the G2 points below
    stamp(kReplay);

    // ---- 4. the folds of the group elements, one batch of MSM items ----
    const Fr gamma = fr_from_abi(&ch[2 * (size_t)sigma]), dd = fr_from_abi(&d);
    const Fr minus_gamma_inv = neg(inv(gamma));
    const size_t n_e = 1 + 3 * (size_t)sigma;  // the terms of E1' and of E2'
    // G1 points: E1 and the rounds' (n_e), w1, Gamma1[0], H1;  G2 points: H2 and the rounds' (n_e), w2, Gamma2[0]
    std::vector<jolt_g1_t> p1(g1s, g1s + n_e);
    p1.push_back(g1s[n_g1 - 1]);
    p1.push_back(vs->gamma1_0);
    p1.push_back(setup->h1);
    std::vector<jolt_g2_t> p2;
    p2.push_back(setup->h2);
    p2.insert(p2.end(), g2s, g2s + 3 * (size_t)sigma);
    p2.push_back(g2s[n_g2 - 1]);
    p2.push_back(vs->gamma2_0);
    // scalars: -coef_g1 / gamma (n_e) | 1, d | -gamma | coef_h2, coef_g2 (n_e) | 1, 1 / d
    std::vector<jolt_fr_t> sc(2 * n_e + 5);
    for (size_t i = 0; i < n_e; ++i) fr_to_abi(&sc[i], mul(fr_from_abi(&coef_g1[i]), minus_gamma_inv));
    fr_to_abi(&sc[n_e], Fr::one());
    sc[n_e + 1] = d;
    fr_to_abi(&sc[n_e + 2], neg(gamma));
    for (size_t i = 0; i < n_e; ++i) sc[n_e + 3 + i] = coef_g2[i];
    fr_to_abi(&sc[2 * n_e + 3], Fr::one());
    fr_to_abi(&sc[2 * n_e + 4], inv(dd));
    Resident res(ctx);
    jolt_dory_vec *v_p1 = nullptr, *v_p2 = nullptr, *v_sc = nullptr, *v_q1 = nullptr, *v_q2 = nullptr;
    JOLT_TRY(res.upload(JOLT_DORY_KIND_G1, p1.data(), p1.size(), &v_p1));
    JOLT_TRY(res.upload(JOLT_DORY_KIND_G2, p2.data(), p2.size(), &v_p2));
    JOLT_TRY(res.upload(JOLT_DORY_KIND_FR, sc.data(), sc.size(), &v_sc));
    jolt_dory_result folds[5];
    {
        const jolt_dory_item items[5] = {
            jolt_dory_item{JOLT_DORY_MSM_G1, v_p1, 0, v_sc, 0, nullptr, 0, n_e},                // -E1' / gamma
            jolt_dory_item{JOLT_DORY_MSM_G1, v_p1, n_e, v_sc, n_e, nullptr, 0, 2},              // w1 + d Gamma1[0]
            jolt_dory_item{JOLT_DORY_MSM_G1, v_p1, n_e + 2, v_sc, n_e + 2, nullptr, 0, 1},      // -gamma H1
            jolt_dory_item{JOLT_DORY_MSM_G2, v_p2, 0, v_sc, n_e + 3, nullptr, 0, n_e},          // E2'
            jolt_dory_item{JOLT_DORY_MSM_G2, v_p2, n_e, v_sc, 2 * n_e + 3, nullptr, 0, 2}};     // w2 + Gamma2[0] / d
        JOLT_TRY(jolt_dory_products(ctx, items, 5, folds));
    }
    stamp(kFolds);

    // ---- 5. the two checks: both left-hand sides from one batch of PAIR items, the right-hand side of the final one from ONE multi-exponentiation ----
    jolt_g1_t q1[4];
    jolt_g2_t q2[4];
    q1[0] = g1s[0];  // (VMV) e(E1, H2)
    q2[0] = setup->h2;
    std::memcpy(&q1[1], &folds[1], sizeof(jolt_g1_t));  // e(w1 + d Gamma1[0], w2 + Gamma2[0] / d)
    std::memcpy(&q2[1], &folds[4], sizeof(jolt_g2_t));
    std::memcpy(&q1[2], &folds[2], sizeof(jolt_g1_t));  // e(-gamma H1, E2')
    std::memcpy(&q2[2], &folds[3], sizeof(jolt_g2_t));
    std::memcpy(&q1[3], &folds[0], sizeof(jolt_g1_t));  // e(-E1' / gamma, H2)
    q2[3] = setup->h2;
    JOLT_TRY(res.upload(JOLT_DORY_KIND_G1, q1, 4, &v_q1));
    JOLT_TRY(res.upload(JOLT_DORY_KIND_G2, q2, 4, &v_q2));
    jolt_dory_result lhs[2];
    {
        const jolt_dory_item items[2] = {jolt_dory_item{JOLT_DORY_PAIR, v_q1, 0, v_q2, 0, nullptr, 0, 1}, jolt_dory_item{JOLT_DORY_PAIR, v_q1, 1, v_q2, 1, nullptr, 0, 3}};
        JOLT_TRY(jolt_dory_products(ctx, items, 2, lhs));
    }
    stamp(kPairings);
    // the proof's GT elements, the commitments, the setup's values of levels s - sigma ... s (the tables are prefixes)
    std::vector<jolt_gt_t> bases(gts, gts + n_gt);
    std::vector<jolt_fr_t> exps(exp_gt);
    bases.insert(bases.end(), commitments, commitments + n_commitments);
    for (size_t i = 0; i < n_commitments; ++i) {
        jolt_fr_t e;
        fr_to_abi(&e, mul(fr_from_abi(&weights[i]), fr_from_abi(&exp_commitment)));
        exps.push_back(e);
    }
    const size_t s = vs->s, o = s - sigma;
    for (size_t k = 0; k <= sigma; ++k) bases.push_back(vs->values[o + k]);
    for (size_t k = 0; k < sigma; ++k) bases.push_back(vs->values[s + 1 + o + k]);
    for (size_t k = 0; k < sigma; ++k) bases.push_back(vs->values[2 * s + 1 + o + k]);
    for (size_t k = 0; k < 3; ++k) bases.push_back(vs->values[3 * s + 1 + k]);
    exps.insert(exps.end(), exp_setup.begin(), exp_setup.end());
    jolt_gt_t rhs;
    JOLT_TRY(jolt_dory_gt_multi_exp(ctx, bases.data(), exps.data(), bases.size(), &rhs));
    stamp(kMultiExp);
    const bool vmv = std::memcmp(&lhs[0], &gts[1], sizeof(jolt_gt_t)) == 0;
    const bool fin = std::memcmp(&lhs[1], &rhs, sizeof(jolt_gt_t)) == 0;
    *accepted = vmv && fin ? 1 : 0;
    *failed_check = !vmv ? 1 : !fin ? 2 : 0;
    return JOLT_OK;
}

}  // namespace

extern "C" int32_t jolt_host_dory_verify_with_transcript(jolt_ctx* ctx, const jolt_dory_verifier_setup* vs, const jolt_dory_setup* setup, const jolt_gt_t* commitment,
                                                         const jolt_fr_t* y, const jolt_fr_t* left, const jolt_fr_t* right, uint32_t nu, uint32_t sigma, const jolt_gt_t* gts,
                                                         const jolt_g1_t* g1s, const jolt_g2_t* g2s, jolt_dory_transcript_fn fn, void* user, int32_t* accepted,
                                                         int32_t* failed_check) {
    jolt_fr_t one;
    fr_to_abi(&one, Fr::one());
    return verify_impl(ctx, vs, setup, commitment, &one, 1, y, left, right, nu, sigma, gts, g1s, g2s, fn, user, accepted, failed_check);
}

extern "C" int32_t jolt_host_dory_verify(jolt_ctx* ctx, const jolt_dory_verifier_setup* vs, const jolt_dory_setup* setup, const jolt_gt_t* commitment, const jolt_fr_t* y,
                                         const jolt_fr_t* left, const jolt_fr_t* right, uint32_t nu, uint32_t sigma, const jolt_gt_t* gts, const jolt_g1_t* g1s,
                                         const jolt_g2_t* g2s, jolt_host_transcript* t, int32_t* accepted, int32_t* failed_check) {
    if (!t) return JOLT_ERR_INVALID_ARG;
    jolt_fr_t one;
    fr_to_abi(&one, Fr::one());
    return verify_impl(ctx, vs, setup, commitment, &one, 1, y, left, right, nu, sigma, gts, g1s, g2s, engine_fn, t, accepted, failed_check);
}

extern "C" int32_t jolt_host_dory_verify_batch(jolt_ctx* ctx, const jolt_dory_verifier_setup* vs, const jolt_dory_setup* setup, const jolt_gt_t* commitments,
                                               const jolt_fr_t* evaluations, size_t n_claims, const jolt_fr_t* point, size_t n_point, const jolt_gt_t* gts,
                                               const jolt_g1_t* g1s, const jolt_g2_t* g2s, jolt_host_transcript* t, int32_t* accepted, int32_t* failed_check,
                                               jolt_fr_t* joint_eval_out) {
    if (!ctx || !vs || !setup || !commitments || !evaluations || !point || !gts || !g1s || !g2s || !t || !accepted || !failed_check || !joint_eval_out) return JOLT_ERR_INVALID_ARG;
    // ---- this entry's checks and the verifier's, before the transcript absorbs the statement ----
    JOLT_REQUIRE(ctx, setup->ctx == ctx && vs->ctx == ctx, "the setup belongs to another context");
    JOLT_REQUIRE(ctx, vs->n == setup->n, "the verifier setup was made from a setup of another size");
    JOLT_REQUIRE(ctx, n_claims != 0, "an empty batch");
    if (n_claims > kMaxPowers - 64) return JOLT_ERR_UNSUPPORTED;
    JOLT_REQUIRE(ctx, n_point <= 2 * (size_t)kMaxSigma, "sigma <= 30");
    const uint32_t sigma = (uint32_t)((n_point + 1) / 2), nu = (uint32_t)n_point - sigma;  // crates/jolt-dory/src/scheme.rs:242-243
    if (sigma > 20) return JOLT_ERR_UNSUPPORTED;  // jolt_host_eq_evals' limit
    if (((size_t)1 << sigma) > setup->n) {
        ctx->last_error = "the setup holds fewer than 2^sigma bases";
        return JOLT_ERR_SRS_TOO_SMALL;
    }
    JOLT_REQUIRE(ctx, all_canonical(evaluations, n_claims) && all_canonical(point, n_point), "an evaluation or a coordinate is not a canonical Fr");
    JOLT_REQUIRE(ctx, all_gt_canonical(gts, 2 + 6 * (size_t)sigma) && all_gt_canonical(commitments, n_claims), "an Fq coordinate of a GT element is not canonical");
    JOLT_REQUIRE(ctx, all_on_curve<G1Ops>(g1s, 2 + 3 * (size_t)sigma) && all_on_curve<G2Ops>(g2s, 1 + 3 * (size_t)sigma), "a point is not on its curve or not canonical");
    // ---- the statement: gamma's powers, joint_eval = sum_i gamma^i y_i; L and R of the point's halves ----
    std::vector<jolt_fr_t> powers(n_claims);
    JOLT_TRY(jolt_host_opening_statement_absorb(t, evaluations, n_claims, powers.data()));
    Fr joint = Fr::zero();
    for (size_t i = 0; i < n_claims; ++i) joint = add(joint, mul(fr_from_abi(&powers[i]), fr_from_abi(&evaluations[i])));
    fr_to_abi(joint_eval_out, joint);
    std::vector<jolt_fr_t> left((size_t)1 << nu), right((size_t)1 << sigma);
    JOLT_TRY(jolt_host_eq_evals(point, nu, nullptr, left.data()));
    JOLT_TRY(jolt_host_eq_evals(point + nu, sigma, nullptr, right.data()));
    JOLT_TRY(verify_impl(ctx, vs, setup, commitments, powers.data(), n_claims, joint_eval_out, left.data(), right.data(), nu, sigma, gts, g1s, g2s, engine_fn, t, accepted, failed_check));
    return jolt_host_opening_claim_absorb(t, point, n_point, joint_eval_out);
}
