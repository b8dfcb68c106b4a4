// jolt_amd/csrc/dory_routines.hip -- the group and field routines dory::prove calls in every reduce-and-fold round, for G1 and G2.
//
// Replaces the two impls of dory's DoryRoutines seam in crates/jolt-dory/src/routines.rs (JoltG1Routines :60-97, JoltG2Routines :101-147;
// the field fold written out in crates/jolt-prover-legacy/src/poly/commitment/dory/jolt_dory_routines.rs:10-18):
//   msm(bases, scalars)                              -> jolt_dory_g{1,2}_msm            sum_i scalars[i] * bases[i]
//   fixed_base_vector_scalar_mul(base, scalars)      -> jolt_dory_g{1,2}_fixed_base_mul out[i] = scalars[i] * base
//   fixed_scalar_mul_bases_then_add(bases, vs, s)    -> jolt_dory_g{1,2}_scale_bases_add vs[i] += s * bases[i]
//   fixed_scalar_mul_vs_then_add(vs, addends, s)     -> jolt_dory_g{1,2}_scale_vs_add   vs[i] = s * vs[i] + addends[i]
//   fold_field_vectors(left, right, s)               -> jolt_dory_fold_field_vectors    left[i] = left[i] * s + right[i]
// The rounds' multi-pairings are dory_pairing.hip; GT scalings and the control flow of dory::prove stay with the caller.
//
// One lane per element.  In the two per-round vector operations every element is multiplied by the SAME scalar: the host recodes it once into
// non-adjacent form (digits in {-1, 0, 1}, no two adjacent non-zero), and every lane walks that one sequence of doublings and additions -- control
// flow is uniform over the wavefront, only the special cases of the group law (identity, P + P, P - P) diverge.  At most 255 doublings and 128
// additions per element (85 on average), no table.  The per-element-scalar routines cannot share a sequence: the fixed-base one takes k * base
// (k = 0..8, signed 4-bit windows) from one shared table by index, the MSM is one double-and-add per term followed by a tree of additions.
// Integer VALU work, no MFMA; the chains are ~254 dependent doublings long, so these kernels are latency bound (docs/kernels.md).
// The kernels and their launch sites (enqueue_*) are dory_kernels.hip.h; every entry here is one HostCall (dory_host.hpp): checks, up() per array, one enqueue_*, down(), finish().
#include <algorithm>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "ctx.hpp"
#include "dory_host.hpp"
#include "dory_kernels.hip.h"

using namespace jolt;
using namespace jolt::dory_host;
using namespace jolt::dory_dev;

namespace {

// The phases of jolt_dory_routines_timing, closed by HostCall::mark: checks, host -> device, kernels, device -> host
enum { kChecks = 0, kUpload = 1, kKernels = 2, kDownload = 3 };

// vs[i] = addend + s * scaled with (scaled, addend) = (other, vs) [bases_then_add] or (vs, other) [vs_then_add]
template <class O>
int32_t scale_add(jolt_ctx* ctx, typename O::Abi* vs, const typename O::Abi* other, size_t n, const jolt_fr_t* scalar, bool scale_vs, const char* what) {
    if (!ctx || !scalar || (n && (!vs || !other))) return JOLT_ERR_INVALID_ARG;
    if (n > kMaxElements) return JOLT_ERR_UNSUPPORTED;
    HostCall c(ctx, ctx->dory_ms, ctx->dory_timing);
    NafPlan plan;
    JOLT_REQUIRE(ctx, naf_plan(scalar, &plan), "scalar is not a canonical Fr");
    JOLT_REQUIRE(ctx, all_on_curve<O>(vs, n) && all_on_curve<O>(other, n), "a point is not on its curve or not canonical");
    if (n == 0) return JOLT_OK;
    c.mark(kChecks, false);
    typename O::Pt *d_vs = nullptr, *d_other = nullptr;
    c.up(vs, n, &d_vs);
    c.up(other, n, &d_other);
    c.mark(kUpload);
    if (c.ok()) c.e = enqueue_scale_add<O>(c.st, plan, scale_vs ? d_vs : d_other, scale_vs ? d_other : d_vs, d_vs, n);
    c.mark(kKernels);
    c.down(vs, d_vs, n);
    return c.finish(what, kDownload);
}

template <class O>
int32_t fixed_base(jolt_ctx* ctx, const typename O::Abi* base, const jolt_fr_t* scalars, size_t n, typename O::Abi* out, const char* what) {
    if (!ctx || !base || (n && (!scalars || !out))) return JOLT_ERR_INVALID_ARG;
    if (n > kMaxElements) return JOLT_ERR_UNSUPPORTED;
    HostCall c(ctx, ctx->dory_ms, ctx->dory_timing);
    using Pt = typename O::Pt;
    JOLT_REQUIRE(ctx, all_on_curve<O>(base, 1), "a point is not on its curve or not canonical");
    JOLT_REQUIRE(ctx, all_canonical(scalars, n), "scalar is not a canonical Fr");
    if (n == 0) return JOLT_OK;  // an empty input gives an empty output (routines.rs:67-69)
    Pt table[kFixedTable];       // read by its upload until finish()
    fixed_table_from_abi<O>(base, table);
    c.mark(kChecks, false);
    Pt *d_table = nullptr, *d_out = nullptr;
    Fr* d_scalars = nullptr;
    c.up(table, kFixedTable, &d_table);
    c.up(scalars, n, &d_scalars);
    c.take(n, &d_out);
    c.mark(kUpload);
    if (c.ok()) c.e = enqueue_fixed_base<O>(c.st, d_table, d_scalars, d_out, n);
    c.mark(kKernels);
    c.down(out, d_out, n);
    return c.finish(what, kDownload);
}

template <class O>
int32_t msm(jolt_ctx* ctx, const typename O::Abi* bases, const jolt_fr_t* scalars, size_t n, typename O::Abi* out, const char* what) {
    if (!ctx || !out || (n && (!bases || !scalars))) return JOLT_ERR_INVALID_ARG;
    if (n > kMaxElements) return JOLT_ERR_UNSUPPORTED;
    HostCall c(ctx, ctx->dory_ms, ctx->dory_timing);
    using Pt = typename O::Pt;
    JOLT_REQUIRE(ctx, all_canonical(scalars, n), "scalar is not a canonical Fr");
    JOLT_REQUIRE(ctx, all_on_curve<O>(bases, n), "a point is not on its curve or not canonical");
    Pt sum = O::identity();  // the empty sum
    if (n) {
        c.mark(kChecks, false);
        Pt *d_bases = nullptr, *d_terms = nullptr;
        Fr* d_scalars = nullptr;
        c.up(bases, n, &d_bases);
        c.up(scalars, n, &d_scalars);
        c.take(n, &d_terms);
        c.mark(kUpload);
        if (c.ok()) c.e = enqueue_msm<O>(c.st, d_bases, d_scalars, d_terms, n);
        c.mark(kKernels);
        c.down(&sum, d_terms, 1);
        JOLT_TRY(c.finish(what, kDownload));
        sum = normalised<O>(sum);
    }
    std::memcpy(out, &sum, sizeof(sum));
    return JOLT_OK;
}

template <class O>
int32_t host_scale_add_one(const typename O::Abi* scaled, const typename O::Abi* addend, const jolt_fr_t* scalar, typename O::Abi* out) {
    if (!scaled || !addend || !scalar || !out) return JOLT_ERR_INVALID_ARG;
    NafPlan plan;
    if (!naf_plan(scalar, &plan)) return JOLT_ERR_INVALID_ARG;
    const auto p = pt_from_abi<typename O::Pt>(scaled), a = pt_from_abi<typename O::Pt>(addend);
    if (!O::on_curve(p) || !O::on_curve(a)) return JOLT_ERR_INVALID_ARG;
    const typename O::Pt r = scale_add_one<O>(plan, p, a);
    std::memcpy(out, &r, sizeof(r));
    return JOLT_OK;
}
template <class O>
int32_t host_fixed_base_one(const typename O::Abi* base, const jolt_fr_t* scalar, typename O::Abi* out) {
    if (!base || !scalar || !out) return JOLT_ERR_INVALID_ARG;
    const Fr s = fr_from_abi(scalar);
    const auto b = pt_from_abi<typename O::Pt>(base);
    if (!fr_is_canonical(s) || !O::on_curve(b)) return JOLT_ERR_INVALID_ARG;
    typename O::Pt table[kFixedTable];
    fixed_table<O>(b, table);
    const typename O::Pt r = fixed_mul_one<O>(table, s);
    std::memcpy(out, &r, sizeof(r));
    return JOLT_OK;
}
template <class O>
int32_t host_msm_term(const typename O::Abi* base, const jolt_fr_t* scalar, typename O::Abi* out) {
    if (!base || !scalar || !out) return JOLT_ERR_INVALID_ARG;
    const Fr s = fr_from_abi(scalar);
    const auto b = pt_from_abi<typename O::Pt>(base);
    if (!fr_is_canonical(s) || !O::on_curve(b)) return JOLT_ERR_INVALID_ARG;
    const typename O::Pt r = normalised<O>(term_mul_one<O>(b, s));
    std::memcpy(out, &r, sizeof(r));
    return JOLT_OK;
}

}  // namespace

extern "C" int32_t jolt_dory_g1_msm(jolt_ctx* ctx, const jolt_g1_t* bases, const jolt_fr_t* scalars, size_t n, jolt_g1_t* out) {
    return msm<G1Ops>(ctx, bases, scalars, n, out, "dory g1 msm");
}
extern "C" int32_t jolt_dory_g1_fixed_base_mul(jolt_ctx* ctx, const jolt_g1_t* base, const jolt_fr_t* scalars, size_t n, jolt_g1_t* out) {
    return fixed_base<G1Ops>(ctx, base, scalars, n, out, "dory g1 fixed base");
}
extern "C" int32_t jolt_dory_g1_scale_bases_add(jolt_ctx* ctx, const jolt_g1_t* bases, jolt_g1_t* vs, size_t n, const jolt_fr_t* scalar) {
    return scale_add<G1Ops>(ctx, vs, bases, n, scalar, false, "dory g1 scale bases");
}
extern "C" int32_t jolt_dory_g1_scale_vs_add(jolt_ctx* ctx, jolt_g1_t* vs, const jolt_g1_t* addends, size_t n, const jolt_fr_t* scalar) {
    return scale_add<G1Ops>(ctx, vs, addends, n, scalar, true, "dory g1 scale vs");
}
extern "C" int32_t jolt_dory_g2_msm(jolt_ctx* ctx, const jolt_g2_t* bases, const jolt_fr_t* scalars, size_t n, jolt_g2_t* out) {
    return msm<G2Ops>(ctx, bases, scalars, n, out, "dory g2 msm");
}
extern "C" int32_t jolt_dory_g2_fixed_base_mul(jolt_ctx* ctx, const jolt_g2_t* base, const jolt_fr_t* scalars, size_t n, jolt_g2_t* out) {
    return fixed_base<G2Ops>(ctx, base, scalars, n, out, "dory g2 fixed base");
}
extern "C" int32_t jolt_dory_g2_scale_bases_add(jolt_ctx* ctx, const jolt_g2_t* bases, jolt_g2_t* vs, size_t n, const jolt_fr_t* scalar) {
    return scale_add<G2Ops>(ctx, vs, bases, n, scalar, false, "dory g2 scale bases");
}
extern "C" int32_t jolt_dory_g2_scale_vs_add(jolt_ctx* ctx, jolt_g2_t* vs, const jolt_g2_t* addends, size_t n, const jolt_fr_t* scalar) {
    return scale_add<G2Ops>(ctx, vs, addends, n, scalar, true, "dory g2 scale vs");
}

extern "C" int32_t jolt_dory_fold_field_vectors(jolt_ctx* ctx, jolt_fr_t* left, const jolt_fr_t* right, size_t n, const jolt_fr_t* scalar) {
    if (!ctx || !scalar || (n && (!left || !right))) return JOLT_ERR_INVALID_ARG;
    if (n > kMaxElements) return JOLT_ERR_UNSUPPORTED;
    HostCall c(ctx, ctx->dory_ms, ctx->dory_timing);
    const Fr s = fr_from_abi(scalar);
    JOLT_REQUIRE(ctx, fr_is_canonical(s) && all_canonical(left, n) && all_canonical(right, n), "scalar is not a canonical Fr");
    if (n == 0) return JOLT_OK;
    c.mark(kChecks, false);
    Fr *d_left = nullptr, *d_right = nullptr;
    c.up(left, n, &d_left);
    c.up(right, n, &d_right);
    c.mark(kUpload);
    if (c.ok()) c.e = enqueue_fold_field(c.st, d_left, d_right, s, n);
    c.mark(kKernels);
    c.down(left, d_left, n);
    return c.finish("dory field fold", kDownload);
}

extern "C" int32_t jolt_dory_routines_timing(jolt_ctx* ctx, int32_t enable, double* out_ms) {
    if (!ctx) return JOLT_ERR_INVALID_ARG;
    if (out_ms)
        for (int k = 0; k < 4; ++k) out_ms[k] = ctx->dory_ms[k];
    ctx->dory_timing = enable != 0;
    return JOLT_OK;
}

// ---- host functions for the CPU suite: Fq2 and G2 as the kernels compute them, and single elements of the routines through the lanes' code ----
extern "C" int32_t jolt_host_fq2_op(int32_t op, const jolt_fq2_t* a, const jolt_fq2_t* b, jolt_fq2_t* out) {
    if (!a || !out || (op <= JOLT_FQ2_MUL && !b)) return JOLT_ERR_INVALID_ARG;
    const Fq2 x = pt_from_abi<Fq2>(a);
    const Fq2 y = op <= JOLT_FQ2_MUL ? pt_from_abi<Fq2>(b) : Fq2::zero();
    if (!fq2_is_canonical(x) || !fq2_is_canonical(y)) return JOLT_ERR_INVALID_ARG;
    Fq2 r;
    switch (op) {
        case JOLT_FQ2_ADD: r = add(x, y); break;
        case JOLT_FQ2_SUB: r = sub(x, y); break;
        case JOLT_FQ2_MUL: r = mul(x, y); break;
        case JOLT_FQ2_SQR: r = sqr(x); break;
        case JOLT_FQ2_NEG: r = neg(x); break;
        default: return JOLT_ERR_INVALID_ARG;
    }
    std::memcpy(out, &r, sizeof(r));
    return JOLT_OK;
}
extern "C" int32_t jolt_host_g2_add(const jolt_g2_t* p, const jolt_g2_t* q, jolt_g2_t* out) {
    if (!p || !q || !out) return JOLT_ERR_INVALID_ARG;
    const G2Jac r = g2_add(pt_from_abi<G2Jac>(p), pt_from_abi<G2Jac>(q));
    std::memcpy(out, &r, sizeof(r));
    return JOLT_OK;
}
extern "C" int32_t jolt_host_g2_double(const jolt_g2_t* p, jolt_g2_t* out) {
    if (!p || !out) return JOLT_ERR_INVALID_ARG;
    const G2Jac r = g2_double(pt_from_abi<G2Jac>(p));
    std::memcpy(out, &r, sizeof(r));
    return JOLT_OK;
}
extern "C" int32_t jolt_host_g2_neg(const jolt_g2_t* p, jolt_g2_t* out) {
    if (!p || !out) return JOLT_ERR_INVALID_ARG;
    const G2Jac r = g2_neg(pt_from_abi<G2Jac>(p));
    std::memcpy(out, &r, sizeof(r));
    return JOLT_OK;
}
extern "C" int32_t jolt_host_g2_eq(const jolt_g2_t* p, const jolt_g2_t* q, int32_t* equal) {
    if (!p || !q || !equal) return JOLT_ERR_INVALID_ARG;
    *equal = g2_eq(pt_from_abi<G2Jac>(p), pt_from_abi<G2Jac>(q)) ? 1 : 0;
    return JOLT_OK;
}
extern "C" int32_t jolt_host_g2_is_on_curve(const jolt_g2_t* p, int32_t* on_curve) {
    if (!p || !on_curve) return JOLT_ERR_INVALID_ARG;
    *on_curve = g2_is_on_curve(pt_from_abi<G2Jac>(p)) ? 1 : 0;
    return JOLT_OK;
}
extern "C" int32_t jolt_host_g2_scalar_mul(const jolt_g2_t* p, const jolt_fr_t* scalar, jolt_g2_t* out) {
    if (!p || !scalar || !out) return JOLT_ERR_INVALID_ARG;
    const Fr s = fr_from_abi(scalar);
    if (!fr_is_canonical(s)) return JOLT_ERR_INVALID_ARG;
    const Fr k = from_mont(s);
    const G2Jac r = normalised<G2Ops>(g2_mul_canonical(pt_from_abi<G2Jac>(p), k.l));
    std::memcpy(out, &r, sizeof(r));
    return JOLT_OK;
}
extern "C" int32_t jolt_host_dory_g1_scale_add_one(const jolt_g1_t* scaled, const jolt_g1_t* addend, const jolt_fr_t* scalar, jolt_g1_t* out) {
    return host_scale_add_one<G1Ops>(scaled, addend, scalar, out);
}
extern "C" int32_t jolt_host_dory_g2_scale_add_one(const jolt_g2_t* scaled, const jolt_g2_t* addend, const jolt_fr_t* scalar, jolt_g2_t* out) {
    return host_scale_add_one<G2Ops>(scaled, addend, scalar, out);
}
extern "C" int32_t jolt_host_dory_g1_fixed_base_one(const jolt_g1_t* base, const jolt_fr_t* scalar, jolt_g1_t* out) {
    return host_fixed_base_one<G1Ops>(base, scalar, out);
}
extern "C" int32_t jolt_host_dory_g2_fixed_base_one(const jolt_g2_t* base, const jolt_fr_t* scalar, jolt_g2_t* out) {
    return host_fixed_base_one<G2Ops>(base, scalar, out);
}
extern "C" int32_t jolt_host_dory_g1_msm_term(const jolt_g1_t* base, const jolt_fr_t* scalar, jolt_g1_t* out) {
    return host_msm_term<G1Ops>(base, scalar, out);
}
extern "C" int32_t jolt_host_dory_g2_msm_term(const jolt_g2_t* base, const jolt_fr_t* scalar, jolt_g2_t* out) {
    return host_msm_term<G2Ops>(base, scalar, out);
}
