// jolt_amd/csrc/dory_pairing.hip -- Dory's multi-pairings on the device: the tier-2 commitment and the multi-pairings of every reduce-and-fold round.
//
// Replaces, through pairing.hip.h:
//   PairingGroup::multi_pairing (crates/jolt-crypto/src/ec/bn254/mod.rs:274-284), dory's multi_pair   -> jolt_dory_multi_pair
//   multi_pair_g2_setup(row_commitments, srs_prefix(g2_vec))   (crates/jolt-dory/src/scheme.rs:543-552) -> jolt_dory_g2_prepare once, jolt_dory_multi_pair_g2_setup
//
// Three kernels (dory_prepared.hip.h, dory_kernels.hip.h, with their launch sites), workgroups of one wavefront, one element per lane:
//   k_pair_prepare_g2     one lane per G2 point: the 88 lines of its Miller loop into a step-major table, lines[step][point], so that the 64 lanes of a wavefront
//                         store (and k_pair_miller loads) neighbouring 192-byte lines
//   k_pair_miller         one lane per PAIR: its own f, 65 squarings and 88 sparse multiplications.  Lanes do not share an f over a chunk of pairs: sharing saves
//                         squarings (12 of ~25 Fq2 multiplications per step) but the kernel is a dependent chain, bound by latency, and 2^13 ... 2^15 pairs are
//                         128 ... 512 wavefronts on 1024 SIMDs -- a chunk of c pairs would leave 1/c of them busy for a chain that is (12 + 13 c) / 25 as long
//   k_tree_level<Fq12, MulFq12>   halving products of the Miller values, the kernel of the MSMs' addition tree under another operation
// Integer VALU work, no MFMA.  The final exponentiation runs once per call on the host.  Every entry is one HostCall (dory_host.hpp).
#include "ctx.hpp"
#include "dory_host.hpp"
#include "dory_kernels.hip.h"
#include "dory_prepared.hip.h"
#include "pairing.hip.h"

using namespace jolt;
using namespace jolt::dory_host;
using namespace jolt::dory_dev;

static_assert(sizeof(jolt_gt_t) == sizeof(Fq12) && sizeof(jolt_g1_t) == sizeof(G1Jac) && sizeof(jolt_g2_t) == sizeof(G2Jac), "pairing ABI layouts");
static_assert(JOLT_PAIRING_LINES == kPairingLines, "jolt_hip.h and pairing_constants.hip.h disagree on the line count");

namespace {

constexpr size_t kMaxPairs = (size_t)1 << 20;

// The phases of jolt_dory_pairing_timing, closed by HostCall::mark
enum { kChecks = 0, kUpload = 1, kPrepare = 2, kMiller = 3, kProduct = 4, kDownload = 5, kFinalExp = 6 };

// Miller values of (d_g1[i], table point i), i < n, their product into *raw; n > 0.  Ends the call's device work: synchronised on every path
int32_t miller_product(HostCall& c, const G1Jac* d_g1, const PairLine* d_lines, const uint8_t* d_skip, size_t stride, size_t n, Fq12* raw, const char* what) {
    Fq12* d_f = nullptr;
    c.take(n, &d_f);
    if (c.ok()) c.e = enqueue_miller(c.st, d_g1, d_lines, d_skip, stride, d_f, n);
    c.mark(kMiller);
    if (c.ok()) c.e = enqueue_tree<Fq12, MulFq12>(c.st, d_f, n);
    c.mark(kProduct);
    c.down(raw, d_f, 1);
    return c.finish(what, kDownload);
}

void write_gt(HostCall& c, const Fq12& raw, bool final_exp, jolt_gt_t* out) {
    const Fq12 r = final_exp ? final_exponentiation(raw) : raw;
    std::memcpy(out, &r, sizeof(r));
    c.mark(kFinalExp, false);
}

int32_t multi_pair(jolt_ctx* ctx, const jolt_g1_t* g1s, const jolt_g2_t* g2s, size_t n, jolt_gt_t* out, bool final_exp) {
    if (!ctx || !out || (n && (!g1s || !g2s))) return JOLT_ERR_INVALID_ARG;
    if (n > kMaxPairs) return JOLT_ERR_UNSUPPORTED;
    HostCall c(ctx, ctx->pairing_ms, ctx->pairing_timing);
    JOLT_REQUIRE(ctx, all_on_curve<G1Ops>(g1s, n) && all_on_curve<G2Ops>(g2s, n), "a point is not on its curve or not canonical");
    c.mark(kChecks, false);
    Fq12 raw = Fq12::one();
    if (n) {
        G1Jac* d_g1 = nullptr;
        G2Jac* d_g2 = nullptr;
        PairLine* d_lines = nullptr;
        uint8_t* d_skip = nullptr;
        c.up(g1s, n, &d_g1);
        c.up(g2s, n, &d_g2);
        c.take(n * kPairingLines, &d_lines);
        c.take(n, &d_skip);
        c.mark(kUpload);
        if (c.ok()) c.e = launch_prepare(c.st, d_g2, d_lines, d_skip, n);
        c.mark(kPrepare);
        JOLT_TRY(miller_product(c, d_g1, d_lines, d_skip, n, n, &raw, "dory multi_pair"));
    }
    write_gt(c, raw, final_exp, out);
    return JOLT_OK;
}

bool fq12_sparse_shape(const Fq12& b) { return b.c0.c1.is_zero() && b.c0.c2.is_zero() && b.c1.c2.is_zero(); }

}  // namespace

extern "C" int32_t jolt_dory_multi_pair(jolt_ctx* ctx, const jolt_g1_t* g1s, const jolt_g2_t* g2s, size_t n, jolt_gt_t* out) {
    return multi_pair(ctx, g1s, g2s, n, out, true);
}
extern "C" int32_t jolt_dory_multi_miller(jolt_ctx* ctx, const jolt_g1_t* g1s, const jolt_g2_t* g2s, size_t n, jolt_gt_t* out) {
    return multi_pair(ctx, g1s, g2s, n, out, false);
}

extern "C" int32_t jolt_dory_g2_prepare(jolt_ctx* ctx, const jolt_g2_t* g2s, size_t n, jolt_g2_prepared** out) {
    if (!ctx || !out || (n && !g2s)) return JOLT_ERR_INVALID_ARG;
    if (n > kMaxPairs) return JOLT_ERR_UNSUPPORTED;
    HostCall c(ctx, ctx->pairing_ms, ctx->pairing_timing);
    JOLT_REQUIRE(ctx, all_on_curve<G2Ops>(g2s, n), "a point is not on its curve or not canonical");
    c.mark(kChecks, false);
    jolt_g2_prepared* p = new (std::nothrow) jolt_g2_prepared();
    if (!p) return JOLT_ERR_OOM;
    p->ctx = ctx;
    p->n = n;
    int32_t rc = JOLT_OK;
    if (n) {
        rc = jolt_internal_dev_alloc(ctx, n * kPairingLines * sizeof(PairLine), (void**)&p->lines);  // the table outlives the call: not one of its blocks
        if (rc == JOLT_OK) rc = jolt_internal_dev_alloc(ctx, n, (void**)&p->skip);
        if (rc == JOLT_OK) {
            G2Jac* d_g2 = nullptr;
            c.up(g2s, n, &d_g2);
            c.mark(kUpload);
            if (c.ok()) c.e = launch_prepare(c.st, d_g2, p->lines, p->skip, n);
            rc = c.finish("dory g2 prepare", kPrepare);
        }
    }
    if (rc != JOLT_OK) {
        (void)jolt_g2_prepared_free(ctx, p);
        return rc;
    }
    *out = p;
    return JOLT_OK;
}

extern "C" int32_t jolt_g2_prepared_free(jolt_ctx* ctx, jolt_g2_prepared* prepared) {
    if (!ctx) return JOLT_ERR_INVALID_ARG;
    if (!prepared) return JOLT_OK;
    if (prepared->lines) jolt_internal_dev_free(ctx, prepared->lines);
    if (prepared->skip) jolt_internal_dev_free(ctx, prepared->skip);
    delete prepared;
    return JOLT_OK;
}

extern "C" int32_t jolt_dory_multi_pair_g2_setup(jolt_ctx* ctx, const jolt_g1_t* g1s, const jolt_g2_prepared* prepared, size_t n, jolt_gt_t* out) {
    if (!ctx || !prepared || !out || (n && !g1s)) return JOLT_ERR_INVALID_ARG;
    JOLT_REQUIRE(ctx, prepared->ctx == ctx, "the prepared table belongs to another context");
    JOLT_REQUIRE(ctx, n <= prepared->n, "more pairs than prepared points");
    HostCall c(ctx, ctx->pairing_ms, ctx->pairing_timing);
    JOLT_REQUIRE(ctx, all_on_curve<G1Ops>(g1s, n), "a point is not on its curve or not canonical");
    c.mark(kChecks, false);
    Fq12 raw = Fq12::one();
    if (n) {
        G1Jac* d_g1 = nullptr;
        c.up(g1s, n, &d_g1);
        c.mark(kUpload);  // no prepare phase: the table is there
        JOLT_TRY(miller_product(c, d_g1, prepared->lines, prepared->skip, prepared->n, n, &raw, "dory multi_pair_g2_setup"));
    }
    write_gt(c, raw, true, out);
    return JOLT_OK;
}

extern "C" int32_t jolt_dory_pairing_timing(jolt_ctx* ctx, int32_t enable, double* out_ms) {
    if (!ctx) return JOLT_ERR_INVALID_ARG;
    if (out_ms)
        for (int k = 0; k < 7; ++k) out_ms[k] = ctx->pairing_ms[k];
    ctx->pairing_timing = enable != 0;
    return JOLT_OK;
}

// ---- host functions for the CPU suite: the same JOLT_HD code ----
extern "C" int32_t jolt_host_fq12_op(int32_t op, const jolt_gt_t* a, const jolt_gt_t* b, jolt_gt_t* out) {
    const bool binary = op == JOLT_FQ12_MUL || op == JOLT_FQ12_MUL_SPARSE;
    if (!a || !out || (binary && !b)) return JOLT_ERR_INVALID_ARG;
    const Fq12 x = pt_from_abi<Fq12>(a);
    const Fq12 y = binary ? pt_from_abi<Fq12>(b) : Fq12::one();
    if (!fq12_is_canonical(x) || !fq12_is_canonical(y)) return JOLT_ERR_INVALID_ARG;
    Fq12 r;
    switch (op) {
        case JOLT_FQ12_MUL: r = mul(x, y); break;
        case JOLT_FQ12_SQR: r = sqr(x); break;
        case JOLT_FQ12_INV:
            if (x.is_zero()) return JOLT_ERR_NOT_INVERTIBLE;
            r = fq12_inv(x);
            break;
        case JOLT_FQ12_CONJ: r = conj(x); break;
        case JOLT_FQ12_FROBENIUS1: r = frobenius1(x); break;
        case JOLT_FQ12_FROBENIUS2: r = frobenius2(x); break;
        case JOLT_FQ12_FROBENIUS3: r = frobenius3(x); break;
        case JOLT_FQ12_MUL_SPARSE:
            if (!fq12_sparse_shape(y)) return JOLT_ERR_INVALID_ARG;
            r = mul_by_034(x, y.c0.c0, y.c1.c0, y.c1.c1);
            break;
        default: return JOLT_ERR_INVALID_ARG;
    }
    std::memcpy(out, &r, sizeof(r));
    return JOLT_OK;
}
extern "C" int32_t jolt_host_g2_prepare_one(const jolt_g2_t* g2, jolt_fq2_t* lines, int32_t* skip) {
    if (!g2 || !lines || !skip) return JOLT_ERR_INVALID_ARG;
    const G2Jac q = pt_from_abi<G2Jac>(g2);
    if (!g2_is_on_curve(q)) return JOLT_ERR_INVALID_ARG;
    PairLine table[kPairingLines];
    *skip = g2_prepare_walk(q, PairLineTable{table, 1}) ? 1 : 0;
    std::memcpy(lines, table, sizeof(table));
    return JOLT_OK;
}
extern "C" int32_t jolt_host_miller_loop(const jolt_g1_t* g1s, const jolt_g2_t* g2s, size_t n, jolt_gt_t* out) {
    if (!out || (n && (!g1s || !g2s))) return JOLT_ERR_INVALID_ARG;
    if (!all_on_curve<G1Ops>(g1s, n) || !all_on_curve<G2Ops>(g2s, n)) return JOLT_ERR_INVALID_ARG;
    Fq12 f = Fq12::one();
    PairLine table[kPairingLines];
    for (size_t i = 0; i < n; ++i) {
        const bool skip = g2_prepare_walk(pt_from_abi<G2Jac>(&g2s[i]), PairLineTable{table, 1});
        f = mul(f, miller_walk(pt_from_abi<G1Jac>(&g1s[i]), PairLineTable{table, 1}, skip));
    }
    std::memcpy(out, &f, sizeof(f));
    return JOLT_OK;
}
extern "C" int32_t jolt_host_final_exponentiation(const jolt_gt_t* f, jolt_gt_t* out) {
    if (!f || !out) return JOLT_ERR_INVALID_ARG;
    const Fq12 x = pt_from_abi<Fq12>(f);
    if (!fq12_is_canonical(x)) return JOLT_ERR_INVALID_ARG;
    if (x.is_zero()) return JOLT_ERR_NOT_INVERTIBLE;
    const Fq12 r = final_exponentiation(x);
    std::memcpy(out, &r, sizeof(r));
    return JOLT_OK;
}
extern "C" int32_t jolt_host_gt_pow(const jolt_gt_t* gt, const jolt_fr_t* scalar, jolt_gt_t* out) {
    if (!gt || !scalar || !out) return JOLT_ERR_INVALID_ARG;
    const Fq12 x = pt_from_abi<Fq12>(gt);
    const Fr s = fr_from_abi(scalar);
    if (!fq12_is_canonical(x) || !fr_is_canonical(s)) return JOLT_ERR_INVALID_ARG;
    const Fr k = from_mont(s);
    const Fq12 r = fq12_pow(x, k.l, 256);
    std::memcpy(out, &r, sizeof(r));
    return JOLT_OK;
}
