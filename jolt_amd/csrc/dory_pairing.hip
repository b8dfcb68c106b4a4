// jolt_amd/csrc/dory_pairing.hip -- Dory's multi-pairings on the device: the tier-2 commitment and the multi-pairings of every reduce-and-fold round.
//
// Replaces, through pairing.hip.h:
//   PairingGroup::multi_pairing (crates/jolt-crypto/src/ec/bn254/mod.rs:274-284), dory's multi_pair   -> jolt_dory_multi_pair
//   multi_pair_g2_setup(row_commitments, srs_prefix(g2_vec))   (crates/jolt-dory/src/scheme.rs:543-552) -> jolt_dory_g2_prepare once, jolt_dory_multi_pair_g2_setup
//
// Three kernels, workgroups of one wavefront, one element per lane:
//   k_pair_prepare_g2     one lane per G2 point: the 88 lines of its Miller loop into a step-major table, lines[step][point], so that the 64 lanes of a wavefront
//                         store (and k_pair_miller loads) neighbouring 192-byte lines
//   k_pair_miller         one lane per PAIR: its own f, 65 squarings and 88 sparse multiplications.  Lanes do not share an f over a chunk of pairs: sharing saves
//                         squarings (12 of ~25 Fq2 multiplications per step) but the kernel is a dependent chain, bound by latency, and 2^13 ... 2^15 pairs are
//                         128 ... 512 wavefronts on 1024 SIMDs -- a chunk of c pairs would leave 1/c of them busy for a chain that is (12 + 13 c) / 25 as long
//   k_pair_product_level  halving products of the Miller values, as k_dory_tree_level
// Integer VALU work, no MFMA.  The final exponentiation runs once per call on the host.
#include <chrono>

#include "ctx.hpp"
#include "dory_host.hpp"
#include "dory_prepared.hip.h"
#include "pairing.hip.h"

using namespace jolt;
using namespace jolt::dory_host;
using namespace jolt::dory_dev;

static_assert(sizeof(jolt_gt_t) == sizeof(Fq12) && sizeof(jolt_g1_t) == sizeof(G1Jac) && sizeof(jolt_g2_t) == sizeof(G2Jac), "pairing ABI layouts");
static_assert(JOLT_PAIRING_LINES == kPairingLines, "jolt_hip.h and pairing_constants.hip.h disagree on the line count");

namespace {

// lines: a table of `stride` >= n points, of which the first n are used
__global__ __launch_bounds__(kLanes) void k_pair_miller(const G1Jac* __restrict__ g1s, const PairLine* lines, const uint8_t* __restrict__ skip, size_t stride, Fq12* __restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * kLanes + threadIdx.x;
    if (i >= n) return;
    const PairLineTable table = {const_cast<PairLine*>(lines) + i, stride};
    out[i] = miller_walk(g1s[i], table, skip[i] != 0);
}
// one level of the product tree: f[i] *= f[i + half] for i + half < m
__global__ __launch_bounds__(kLanes) void k_pair_product_level(Fq12* f, size_t half, size_t m) {
    const size_t i = (size_t)blockIdx.x * kLanes + threadIdx.x;
    if (i >= half || i + half >= m) return;
    f[i] = mul(f[i], f[i + half]);
}

constexpr size_t kMaxPairs = (size_t)1 << 20;

bool g1_all_on_curve(const jolt_g1_t* pts, size_t n) {
    return parallel_all(n, [pts](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; ++i)
            if (!g1_is_on_curve(pt_from_abi<G1Jac>(&pts[i]))) return false;
        return true;
    });
}
bool g2_all_on_curve(const jolt_g2_t* pts, size_t n) {
    return parallel_all(n, [pts](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; ++i)
            if (!g2_is_on_curve(pt_from_abi<G2Jac>(&pts[i]))) return false;
        return true;
    });
}

// Phase clock of jolt_dory_pairing_timing: 0 checks, 1 host -> device, 2 prepare, 3 Miller, 4 product, 5 device -> host, 6 final exponentiation
struct Phases {
    jolt_ctx* ctx;
    std::chrono::steady_clock::time_point t0;
    explicit Phases(jolt_ctx* c) : ctx(c), t0(std::chrono::steady_clock::now()) {
        if (c->pairing_timing)
            for (double& v : c->pairing_ms) v = 0.0;
    }
    hipError_t mark(int phase) {
        if (!ctx->pairing_timing) return hipSuccess;
        const hipError_t e = (phase >= 1 && phase <= 5) ? hipStreamSynchronize(ctx->stream) : hipSuccess;
        const auto t1 = std::chrono::steady_clock::now();
        ctx->pairing_ms[phase] += std::chrono::duration<double, std::milli>(t1 - t0).count();
        t0 = t1;
        return e;
    }
};

// Miller values of (d_g1[i], table point i), i < n, their product into *raw; n > 0
int32_t miller_product(jolt_ctx* ctx, Phases& ph, DevBufs& bufs, const G1Jac* d_g1, const PairLine* d_lines, const uint8_t* d_skip, size_t stride, size_t n, Fq12* raw, const char* what) {
    hipStream_t st = ctx->stream;
    Fq12* d_f = nullptr;
    const int32_t rc = bufs.take(n, &d_f);
    if (rc != JOLT_OK) {
        (void)hipStreamSynchronize(st);  // the copies from the caller's arrays are in flight
        return rc;
    }
    hipLaunchKernelGGL(k_pair_miller, dim3(lanes_grid(n)), dim3(kLanes), 0, st, d_g1, d_lines, d_skip, stride, d_f, n);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = ph.mark(3);
    if (e == hipSuccess) {
        for (size_t m = n; m > 1;) {
            const size_t half = (m + 1) / 2;
            hipLaunchKernelGGL(k_pair_product_level, dim3(lanes_grid(half)), dim3(kLanes), 0, st, d_f, half, m);
            m = half;
        }
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = ph.mark(4);
    if (e == hipSuccess) e = hipMemcpyAsync(raw, d_f, sizeof(Fq12), hipMemcpyDeviceToHost, st);
    const hipError_t e2 = hipStreamSynchronize(st);  // the caller's arrays are read until here
    if (e == hipSuccess) e = e2;
    (void)ph.mark(5);
    if (e != hipSuccess) return hip_fail(ctx, what, e);
    return JOLT_OK;
}

void finish(Phases& ph, const Fq12& raw, bool final_exp, jolt_gt_t* out) {
    const Fq12 r = final_exp ? final_exponentiation(raw) : raw;
    std::memcpy(out, &r, sizeof(r));
    (void)ph.mark(6);
}

int32_t multi_pair(jolt_ctx* ctx, const jolt_g1_t* g1s, const jolt_g2_t* g2s, size_t n, jolt_gt_t* out, bool final_exp) {
    if (!ctx || !out || (n && (!g1s || !g2s))) return JOLT_ERR_INVALID_ARG;
    if (n > kMaxPairs) return JOLT_ERR_UNSUPPORTED;
    Phases ph(ctx);
    JOLT_REQUIRE(ctx, g1_all_on_curve(g1s, n) && g2_all_on_curve(g2s, n), "a point is not on its curve or not canonical");
    (void)ph.mark(0);
    Fq12 raw = Fq12::one();
    if (n) {
        hipStream_t st = ctx->stream;
        DevBufs bufs(ctx);
        G1Jac* d_g1 = nullptr;
        G2Jac* d_g2 = nullptr;
        PairLine* d_lines = nullptr;
        uint8_t* d_skip = nullptr;
        JOLT_TRY(bufs.take(n, &d_g1));
        JOLT_TRY(bufs.take(n, &d_g2));
        JOLT_TRY(bufs.take(n * kPairingLines, &d_lines));
        JOLT_TRY(bufs.take(n, &d_skip));
        hipError_t e = hipMemcpyAsync(d_g1, g1s, n * sizeof(G1Jac), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(d_g2, g2s, n * sizeof(G2Jac), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = ph.mark(1);
        if (e == hipSuccess) e = launch_prepare(st, d_g2, d_lines, d_skip, n);
        if (e == hipSuccess) e = ph.mark(2);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(st);  // the caller's arrays may still be read
            return hip_fail(ctx, "dory multi_pair", e);
        }
        JOLT_TRY(miller_product(ctx, ph, bufs, d_g1, d_lines, d_skip, n, n, &raw, "dory multi_pair"));
    }
    finish(ph, raw, final_exp, out);
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
    Phases ph(ctx);
    JOLT_REQUIRE(ctx, g2_all_on_curve(g2s, n), "a point is not on its curve or not canonical");
    (void)ph.mark(0);
    jolt_g2_prepared* p = new (std::nothrow) jolt_g2_prepared();
    if (!p) return JOLT_ERR_OOM;
    p->ctx = ctx;
    p->n = n;
    int32_t rc = JOLT_OK;
    if (n) {
        hipStream_t st = ctx->stream;
        DevBufs bufs(ctx);
        G2Jac* d_g2 = nullptr;
        rc = bufs.take(n, &d_g2);
        if (rc == JOLT_OK) rc = jolt_internal_dev_alloc(ctx, n * kPairingLines * sizeof(PairLine), (void**)&p->lines);
        if (rc == JOLT_OK) rc = jolt_internal_dev_alloc(ctx, n, (void**)&p->skip);
        if (rc == JOLT_OK) {
            hipError_t e = hipMemcpyAsync(d_g2, g2s, n * sizeof(G2Jac), hipMemcpyHostToDevice, st);
            if (e == hipSuccess) e = ph.mark(1);
            if (e == hipSuccess) e = launch_prepare(st, d_g2, p->lines, p->skip, n);
            const hipError_t e2 = hipStreamSynchronize(st);  // the caller's array is read until here
            if (e == hipSuccess) e = e2;
            (void)ph.mark(2);
            if (e != hipSuccess) rc = hip_fail(ctx, "dory g2 prepare", e);
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
    Phases ph(ctx);
    JOLT_REQUIRE(ctx, g1_all_on_curve(g1s, n), "a point is not on its curve or not canonical");
    (void)ph.mark(0);
    Fq12 raw = Fq12::one();
    if (n) {
        hipStream_t st = ctx->stream;
        DevBufs bufs(ctx);
        G1Jac* d_g1 = nullptr;
        JOLT_TRY(bufs.take(n, &d_g1));
        hipError_t e = hipMemcpyAsync(d_g1, g1s, n * sizeof(G1Jac), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = ph.mark(1);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(st);
            return hip_fail(ctx, "dory multi_pair_g2_setup", e);
        }
        JOLT_TRY(miller_product(ctx, ph, bufs, d_g1, prepared->lines, prepared->skip, prepared->n, n, &raw, "dory multi_pair_g2_setup"));
    }
    finish(ph, raw, true, out);
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
    if (!g1_all_on_curve(g1s, n) || !g2_all_on_curve(g2s, n)) return JOLT_ERR_INVALID_ARG;
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
