// jolt_amd/csrc/device_probe.hip -- TESTS ONLY: the device twins of the suite's host forms (jolt_probe_*), and the array host form of the field ops.
//
// The CPU suite holds every piece of arithmetic the kernels rely on to an independent reference at deliberately nasty operands, through a jolt_host_* entry that
// compiles the JOLT_HD function for the CPU.  The x86 build differs from the gfx950 build exactly where such code goes wrong (device_probe.hip.h lists how), so each
// entry here runs the same function on the device: host arrays of n operand tuples in, ONE launch with one lane per tuple, n results out.  No kernel of the
// product path is touched and nothing here is on it.
//
// Every entry refuses n > 2^20 (JOLT_ERR_UNSUPPORTED), a null pointer with n > 0, an unknown op, and the operands its host form refuses, with the host form's
// status; a refused call launches nothing and writes nothing.  n = 0 is JOLT_OK.  One kernel per family and op (templates): an Fq12 product alone takes most of a
// lane's registers, so nothing here switches over ops inside a kernel.  One wavefront per workgroup (the launch shape of the latency-bound Dory kernels).
#include <cstring>
#include <vector>

#include "ctx.hpp"
#include "device_probe.hip.h"
#include "dory_host.hpp"

using namespace jolt;
using namespace jolt::dory_host;

namespace {

constexpr size_t kProbeMax = (size_t)1 << 20;

template <class PR, int OP>
__global__ __launch_bounds__(kLanes) void k_probe_field(const Fp<PR>* __restrict__ a, const Fp<PR>* __restrict__ b, Fp<PR>* __restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * kLanes + threadIdx.x;
    if (i >= n) return;
    out[i] = probe::field_op<PR, OP>(a[i], b[i]);
}
template <int OP>
__global__ __launch_bounds__(kLanes) void k_probe_fq_limb(const Fq* __restrict__ a, const Fq* __restrict__ b, const Fq* __restrict__ c, const Fq* __restrict__ d,
                                                           Fq* __restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * kLanes + threadIdx.x;
    if (i >= n) return;
    out[i] = probe::fq_limb_op<OP>(a[i], b[i], c[i], d[i]);
}
__global__ __launch_bounds__(kLanes) void k_probe_add_paths(const G1XyzzL* __restrict__ acc, const FqL* __restrict__ q, const int32_t* __restrict__ negate,
                                                             probe::AddPaths* __restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * kLanes + threadIdx.x;
    if (i >= n) return;
    probe::AddPaths r;
    probe::g1xl_add_paths(acc[i], q[2 * i], q[2 * i + 1], negate[i] != 0, r);
    out[i] = r;
}
template <int OP>
__global__ __launch_bounds__(kLanes) void k_probe_fq2(const Fq2* __restrict__ a, const Fq2* __restrict__ b, Fq2* __restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * kLanes + threadIdx.x;
    if (i >= n) return;
    out[i] = probe::fq2_op<OP>(a[i], b[i]);
}
template <int OP>
__global__ __launch_bounds__(kLanes) void k_probe_fq12(const Fq12* __restrict__ a, const Fq12* __restrict__ b, Fq12* __restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * kLanes + threadIdx.x;
    if (i >= n) return;
    out[i] = probe::fq12_op<OP>(a[i], b[i]);
}
template <int OP>
__global__ __launch_bounds__(kLanes) void k_probe_g2(const G2Jac* __restrict__ p, const G2Jac* __restrict__ q, G2Jac* __restrict__ out, int32_t* __restrict__ equal,
                                                      size_t n) {
    const size_t i = (size_t)blockIdx.x * kLanes + threadIdx.x;
    if (i >= n) return;
    if (OP == probe::kG2Add) out[i] = g2_add(p[i], q[i]);
    else if (OP == probe::kG2Double) out[i] = g2_double(p[i]);
    else equal[i] = g2_eq(p[i], q[i]) ? 1 : 0;
}
__global__ __launch_bounds__(kLanes) void k_probe_suffix(const uint32_t* __restrict__ kind, const uint64_t* __restrict__ lo, const uint64_t* __restrict__ hi,
                                                          const uint32_t* __restrict__ len, uint64_t* __restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * kLanes + threadIdx.x;
    if (i >= n) return;
    out[i] = probe::suffix_masked(kind[i], lo[i], hi[i], len[i]);
}
__global__ __launch_bounds__(kLanes) void k_probe_dory_fr_digits(const Fr* __restrict__ scalars, int c, int W, uint32_t* __restrict__ digits, uint32_t* __restrict__ negative,
                                                                  size_t n) {
    const size_t i = (size_t)blockIdx.x * kLanes + threadIdx.x;
    if (i >= n) return;
    uint32_t neg;
    probe::dory_fr_digits(scalars[i], c, W, digits + i * (size_t)W, neg);
    negative[i] = neg;
}

__global__ __launch_bounds__(kLanes) void k_probe_small_scalar_dots(const Fr* __restrict__ values, const void* __restrict__ ints, int kind, const uint64_t* __restrict__ offsets,
                                                                     Fr* __restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * kLanes + threadIdx.x;
    if (i >= n) return;
    out[i] = probe::small_scalar_dot(values, ints, kind, (size_t)offsets[i], (size_t)offsets[i + 1]);
}

template <class K, class... Args>
hipError_t launch(K kernel, hipStream_t st, size_t n, Args... args) {
    hipLaunchKernelGGL(kernel, dim3(lanes_grid(n)), dim3(kLanes), 0, st, args..., n);
    return hipGetLastError();
}

template <class PR>
hipError_t enqueue_field(hipStream_t st, int op, const Fp<PR>* a, const Fp<PR>* b, Fp<PR>* out, size_t n) {
    switch (op) {
        case probe::kMul: return launch(k_probe_field<PR, probe::kMul>, st, n, a, b, out);
        case probe::kSqr: return launch(k_probe_field<PR, probe::kSqr>, st, n, a, b, out);
        case probe::kAdd: return launch(k_probe_field<PR, probe::kAdd>, st, n, a, b, out);
        case probe::kSub: return launch(k_probe_field<PR, probe::kSub>, st, n, a, b, out);
        case probe::kNeg: return launch(k_probe_field<PR, probe::kNeg>, st, n, a, b, out);
        case probe::kDbl: return launch(k_probe_field<PR, probe::kDbl>, st, n, a, b, out);
        case probe::kFromMont: return launch(k_probe_field<PR, probe::kFromMont>, st, n, a, b, out);
        case probe::kToMont: return launch(k_probe_field<PR, probe::kToMont>, st, n, a, b, out);
        default: return launch(k_probe_field<PR, probe::kMulShifted>, st, n, a, b, out);
    }
}
template <class PR>
void host_field(int op, const jolt_fr_t* a, const jolt_fr_t* b, jolt_fr_t* out, size_t n) {
    for (size_t i = 0; i < n; ++i) {
        const Fp<PR> x = pt_from_abi<Fp<PR>>(&a[i]), y = pt_from_abi<Fp<PR>>(&b[i]);  // the caller's arrays need not be aligned as Fp is
        Fp<PR> r;
        switch (op) {
            case probe::kMul: r = probe::field_op<PR, probe::kMul>(x, y); break;
            case probe::kSqr: r = probe::field_op<PR, probe::kSqr>(x, y); break;
            case probe::kAdd: r = probe::field_op<PR, probe::kAdd>(x, y); break;
            case probe::kSub: r = probe::field_op<PR, probe::kSub>(x, y); break;
            case probe::kNeg: r = probe::field_op<PR, probe::kNeg>(x, y); break;
            case probe::kDbl: r = probe::field_op<PR, probe::kDbl>(x, y); break;
            case probe::kFromMont: r = probe::field_op<PR, probe::kFromMont>(x, y); break;
            case probe::kToMont: r = probe::field_op<PR, probe::kToMont>(x, y); break;
            default: r = probe::field_op<PR, probe::kMulShifted>(x, y); break;
        }
        std::memcpy(&out[i], &r, sizeof(r));
    }
}

// the argument checks the field entries share: JOLT_OK, or the status to return
int32_t field_args(int32_t field, int32_t op, const jolt_fr_t* a, const jolt_fr_t* b, size_t n, const jolt_fr_t* out) {
    if ((field != 0 && field != 1) || op < 0 || op >= probe::kNumFieldOps || (op == probe::kMulShifted && field != 0)) return JOLT_ERR_INVALID_ARG;
    if (n > kProbeMax) return JOLT_ERR_UNSUPPORTED;
    if (n && (!a || !out || (probe::field_op_is_binary(op) && !b))) return JOLT_ERR_INVALID_ARG;
    if (op == probe::kMulShifted)
        for (size_t i = 0; i < n; ++i)
            if (!fr_low_limbs_zero(fr_from_abi(&b[i]))) return JOLT_ERR_INVALID_ARG;
    return JOLT_OK;
}

template <class T, class Ok>
bool all_of(const void* p, size_t n, Ok ok) {
    for (size_t i = 0; i < n; ++i)
        if (!ok(pt_from_abi<T>((const char*)p + i * sizeof(T)))) return false;
    return true;
}

// dots[i] = the terms [offsets[i], offsets[i + 1]) of one column: offsets ascend from any start to the term count at most
int32_t small_dots_args(const jolt_fr_t* values, const void* ints, int32_t kind, const uint64_t* offsets, size_t n_terms, size_t n, const jolt_fr_t* out) {
    if (kind < kIntKindU64 || kind > kIntKindI128) return JOLT_ERR_INVALID_ARG;
    if (n > kProbeMax || n_terms > kProbeMax) return JOLT_ERR_UNSUPPORTED;
    if (n && (!offsets || !out || (n_terms && (!values || !ints)))) return JOLT_ERR_INVALID_ARG;
    for (size_t i = 0; i < n; ++i)
        if (offsets[i] > offsets[i + 1] || offsets[i + 1] > n_terms) return JOLT_ERR_INVALID_ARG;
    return JOLT_OK;
}

}  // namespace

// field 0 = Fr, 1 = Fq; op = JOLT_PROBE_*.  Unary ops ignore b.  Operands are taken as they are (the host forms of the field ops refuse nothing but a mul_shifted
// operand with non-zero low limbs).
extern "C" int32_t jolt_host_field_op(int32_t field, int32_t op, const jolt_fr_t* a, const jolt_fr_t* b, size_t n, jolt_fr_t* out) {
    JOLT_TRY(field_args(field, op, a, b, n, out));
    if (n == 0) return JOLT_OK;
    if (!probe::field_op_is_binary(op)) b = a;
    if (field == 0) host_field<FrParams>(op, a, b, out, n);
    else host_field<FqParams>(op, a, b, out, n);
    return JOLT_OK;
}
extern "C" int32_t jolt_probe_field_op(jolt_ctx* ctx, int32_t field, int32_t op, const jolt_fr_t* a, const jolt_fr_t* b, size_t n, jolt_fr_t* out) {
    if (!ctx) return JOLT_ERR_INVALID_ARG;
    JOLT_TRY(field_args(field, op, a, b, n, out));
    if (n == 0) return JOLT_OK;
    HostCall c(ctx);
    Fr *d_a = nullptr, *d_b = nullptr, *d_out = nullptr;  // Fr and Fq share a layout: eight words
    c.up(a, n, &d_a);
    if (probe::field_op_is_binary(op)) c.up(b, n, &d_b);
    else d_b = d_a;
    c.take(n, &d_out);
    if (c.ok()) c.e = field == 0 ? enqueue_field<FrParams>(c.st, op, d_a, d_b, d_out, n) : enqueue_field<FqParams>(c.st, op, (const Fq*)d_a, (const Fq*)d_b, (Fq*)d_out, n);
    c.down(out, d_out, n);
    return c.finish("probe field op");
}

extern "C" int32_t jolt_probe_fq_limb_op(jolt_ctx* ctx, int32_t op, const jolt_fr_t* a, const jolt_fr_t* b, const jolt_fr_t* c, const jolt_fr_t* d, size_t n, jolt_fr_t* out) {
    if (!ctx || op < 0 || op >= probe::kNumLimbOps) return JOLT_ERR_INVALID_ARG;
    if (n > kProbeMax) return JOLT_ERR_UNSUPPORTED;
    if (n && (!a || !out || (op != 1 && !b) || (op >= 2 && !c) || ((op == 2 || op == 4) && !d))) return JOLT_ERR_INVALID_ARG;
    if (n == 0) return JOLT_OK;
    HostCall call(ctx);
    Fq *d_a = nullptr, *d_b = nullptr, *d_c = nullptr, *d_d = nullptr, *d_out = nullptr;
    call.up(a, n, &d_a);
    d_b = d_c = d_d = d_a;  // an operand the op does not take: any valid address
    if (op != 1) call.up(b, n, &d_b);
    if (op >= 2) call.up(c, n, &d_c);
    if (op == 2 || op == 4) call.up(d, n, &d_d);
    call.take(n, &d_out);
    if (call.ok()) {
        switch (op) {
            case 0: call.e = launch(k_probe_fq_limb<0>, call.st, n, d_a, d_b, d_c, d_d, d_out); break;
            case 1: call.e = launch(k_probe_fq_limb<1>, call.st, n, d_a, d_b, d_c, d_d, d_out); break;
            case 2: call.e = launch(k_probe_fq_limb<2>, call.st, n, d_a, d_b, d_c, d_d, d_out); break;
            case 3: call.e = launch(k_probe_fq_limb<3>, call.st, n, d_a, d_b, d_c, d_d, d_out); break;
            default: call.e = launch(k_probe_fq_limb<4>, call.st, n, d_a, d_b, d_c, d_d, d_out); break;
        }
    }
    call.down(out, d_out, n);
    return call.finish("probe fq limb op");
}

// the twin of jolt_host_g1xl_add_paths over n tuples: acc n x 36 limbs, q n x 18, negate n; common / full / step n x 36 each, suspect n, canon n x 64 words
extern "C" int32_t jolt_probe_g1xl_add_paths(jolt_ctx* ctx, const uint32_t* acc, const uint32_t* q, const int32_t* negate, size_t n, uint32_t* common, uint32_t* full,
                                             uint32_t* step, int32_t* suspect, uint32_t* canon) {
    if (!ctx) return JOLT_ERR_INVALID_ARG;
    if (n > kProbeMax) return JOLT_ERR_UNSUPPORTED;
    if (n && (!acc || !q || !negate || !common || !full || !step || !suspect || !canon)) return JOLT_ERR_INVALID_ARG;
    if (n == 0) return JOLT_OK;
    HostCall c(ctx);
    G1XyzzL* d_acc = nullptr;
    FqL* d_q = nullptr;
    int32_t* d_neg = nullptr;
    probe::AddPaths* d_out = nullptr;
    c.up(acc, n, &d_acc);
    c.up(q, 2 * n, &d_q);
    c.up(negate, n, &d_neg);
    c.take(n, &d_out);
    if (c.ok()) c.e = launch(k_probe_add_paths, c.st, n, d_acc, d_q, d_neg, d_out);
    std::vector<probe::AddPaths> host(n);
    c.down(host.data(), d_out, n);
    JOLT_TRY(c.finish("probe g1xl add paths"));
    for (size_t i = 0; i < n; ++i) {
        std::memcpy(common + 36 * i, &host[i].common, sizeof(G1XyzzL));
        std::memcpy(full + 36 * i, &host[i].full, sizeof(G1XyzzL));
        std::memcpy(step + 36 * i, &host[i].step, sizeof(G1XyzzL));
        suspect[i] = host[i].suspect;
        std::memcpy(canon + 64 * i, host[i].canon, sizeof(host[i].canon));
    }
    return JOLT_OK;
}

extern "C" int32_t jolt_probe_fq2_op(jolt_ctx* ctx, int32_t op, const jolt_fq2_t* a, const jolt_fq2_t* b, size_t n, jolt_fq2_t* out) {
    if (!ctx || op < JOLT_FQ2_ADD || op > JOLT_FQ2_NEG) return JOLT_ERR_INVALID_ARG;
    const bool binary = op <= JOLT_FQ2_MUL;
    if (n > kProbeMax) return JOLT_ERR_UNSUPPORTED;
    if (n && (!a || !out || (binary && !b))) return JOLT_ERR_INVALID_ARG;
    if (!all_of<Fq2>(a, n, [](const Fq2& v) { return fq2_is_canonical(v); }) || (binary && !all_of<Fq2>(b, n, [](const Fq2& v) { return fq2_is_canonical(v); }))) return JOLT_ERR_INVALID_ARG;
    if (n == 0) return JOLT_OK;
    HostCall c(ctx);
    Fq2 *d_a = nullptr, *d_b = nullptr, *d_out = nullptr;
    c.up(a, n, &d_a);
    if (binary) c.up(b, n, &d_b);
    else d_b = d_a;
    c.take(n, &d_out);
    if (c.ok()) {
        switch (op) {
            case JOLT_FQ2_ADD: c.e = launch(k_probe_fq2<JOLT_FQ2_ADD>, c.st, n, d_a, d_b, d_out); break;
            case JOLT_FQ2_SUB: c.e = launch(k_probe_fq2<JOLT_FQ2_SUB>, c.st, n, d_a, d_b, d_out); break;
            case JOLT_FQ2_MUL: c.e = launch(k_probe_fq2<JOLT_FQ2_MUL>, c.st, n, d_a, d_b, d_out); break;
            case JOLT_FQ2_SQR: c.e = launch(k_probe_fq2<JOLT_FQ2_SQR>, c.st, n, d_a, d_b, d_out); break;
            default: c.e = launch(k_probe_fq2<JOLT_FQ2_NEG>, c.st, n, d_a, d_b, d_out); break;
        }
    }
    c.down(out, d_out, n);
    return c.finish("probe fq2 op");
}

// add, double and equality as jolt_host_g2_add / _double / _eq take them: any coordinates, no on-curve check.  out: n points (add, double); equal: n flags (eq)
extern "C" int32_t jolt_probe_g2_op(jolt_ctx* ctx, int32_t op, const jolt_g2_t* p, const jolt_g2_t* q, size_t n, jolt_g2_t* out, int32_t* equal) {
    if (!ctx || op < probe::kG2Add || op > probe::kG2Eq) return JOLT_ERR_INVALID_ARG;
    if (n > kProbeMax) return JOLT_ERR_UNSUPPORTED;
    if (n && (!p || (op != probe::kG2Double && !q) || (op == probe::kG2Eq ? !equal : !out))) return JOLT_ERR_INVALID_ARG;
    if (n == 0) return JOLT_OK;
    HostCall c(ctx);
    G2Jac *d_p = nullptr, *d_q = nullptr, *d_out = nullptr;
    int32_t* d_eq = nullptr;
    c.up(p, n, &d_p);
    if (op != probe::kG2Double) c.up(q, n, &d_q);
    else d_q = d_p;
    c.take(n, &d_out);
    c.take(n, &d_eq);
    if (c.ok()) {
        if (op == probe::kG2Add) c.e = launch(k_probe_g2<probe::kG2Add>, c.st, n, d_p, d_q, d_out, d_eq);
        else if (op == probe::kG2Double) c.e = launch(k_probe_g2<probe::kG2Double>, c.st, n, d_p, d_q, d_out, d_eq);
        else c.e = launch(k_probe_g2<probe::kG2Eq>, c.st, n, d_p, d_q, d_out, d_eq);
    }
    if (op == probe::kG2Eq) c.down(equal, d_eq, n);
    else c.down(out, d_out, n);
    return c.finish("probe g2 op");
}

// MUL, SQR, CONJ, MUL_SPARSE of JOLT_FQ12_*.  INV and the Frobenius maps are host-only functions (the final exponentiation runs on the host and no kernel calls
// them): JOLT_ERR_UNSUPPORTED
extern "C" int32_t jolt_probe_fq12_op(jolt_ctx* ctx, int32_t op, const jolt_gt_t* a, const jolt_gt_t* b, size_t n, jolt_gt_t* out) {
    if (!ctx || op < JOLT_FQ12_MUL || op > JOLT_FQ12_MUL_SPARSE) return JOLT_ERR_INVALID_ARG;
    if (op == JOLT_FQ12_INV || op == JOLT_FQ12_FROBENIUS1 || op == JOLT_FQ12_FROBENIUS2 || op == JOLT_FQ12_FROBENIUS3) return JOLT_ERR_UNSUPPORTED;
    const bool binary = op == JOLT_FQ12_MUL || op == JOLT_FQ12_MUL_SPARSE;
    if (n > kProbeMax) return JOLT_ERR_UNSUPPORTED;
    if (n && (!a || !out || (binary && !b))) return JOLT_ERR_INVALID_ARG;
    if (!all_of<Fq12>(a, n, [](const Fq12& v) { return fq12_is_canonical(v); }) || (binary && !all_of<Fq12>(b, n, [](const Fq12& v) { return fq12_is_canonical(v); }))) return JOLT_ERR_INVALID_ARG;
    if (op == JOLT_FQ12_MUL_SPARSE && !all_of<Fq12>(b, n, [](const Fq12& v) { return probe::fq12_sparse_shape(v); })) return JOLT_ERR_INVALID_ARG;
    if (n == 0) return JOLT_OK;
    HostCall c(ctx);
    Fq12 *d_a = nullptr, *d_b = nullptr, *d_out = nullptr;
    c.up(a, n, &d_a);
    if (binary) c.up(b, n, &d_b);
    else d_b = d_a;
    c.take(n, &d_out);
    if (c.ok()) {
        switch (op) {
            case JOLT_FQ12_MUL: c.e = launch(k_probe_fq12<probe::kFq12Mul>, c.st, n, d_a, d_b, d_out); break;
            case JOLT_FQ12_SQR: c.e = launch(k_probe_fq12<probe::kFq12Sqr>, c.st, n, d_a, d_b, d_out); break;
            case JOLT_FQ12_CONJ: c.e = launch(k_probe_fq12<probe::kFq12Conj>, c.st, n, d_a, d_b, d_out); break;
            default: c.e = launch(k_probe_fq12<probe::kFq12MulSparse>, c.st, n, d_a, d_b, d_out); break;
        }
    }
    c.down(out, d_out, n);
    return c.finish("probe fq12 op");
}

extern "C" int32_t jolt_probe_suffix_mle(jolt_ctx* ctx, const uint32_t* kind, const uint64_t* lo, const uint64_t* hi, const uint32_t* len, size_t n, uint64_t* out) {
    if (!ctx) return JOLT_ERR_INVALID_ARG;
    if (n > kProbeMax) return JOLT_ERR_UNSUPPORTED;
    if (n && (!kind || !lo || !hi || !len || !out)) return JOLT_ERR_INVALID_ARG;
    for (size_t i = 0; i < n; ++i)
        if (kind[i] >= (uint32_t)kNumSuffixKinds || len[i] > 128) return JOLT_ERR_INVALID_ARG;
    if (n == 0) return JOLT_OK;
    HostCall c(ctx);
    uint32_t *d_kind = nullptr, *d_len = nullptr;
    uint64_t *d_lo = nullptr, *d_hi = nullptr, *d_out = nullptr;
    c.up(kind, n, &d_kind);
    c.up(lo, n, &d_lo);
    c.up(hi, n, &d_hi);
    c.up(len, n, &d_len);
    c.take(n, &d_out);
    if (c.ok()) c.e = launch(k_probe_suffix, c.st, n, d_kind, d_lo, d_hi, d_len, d_out);
    c.down(out, d_out, n);
    return c.finish("probe suffix mle");
}

// digits_out: n rows of W words, negative_out: n words; c, W and the scalars as jolt_host_dory_fr_digits takes them
extern "C" int32_t jolt_probe_dory_fr_digits(jolt_ctx* ctx, const jolt_fr_t* scalars, size_t n, int32_t c, int32_t W, uint32_t* digits_out, uint32_t* negative_out) {
    if (!ctx || c < 3 || c > 13 || W < 1 || W > dory_fr::kMaxHostWindows) return JOLT_ERR_INVALID_ARG;
    if (n > kProbeMax) return JOLT_ERR_UNSUPPORTED;
    if (n && (!scalars || !digits_out || !negative_out)) return JOLT_ERR_INVALID_ARG;
    if (!all_of<Fr>(scalars, n, [](const Fr& v) { return fr_is_canonical(v); })) return JOLT_ERR_INVALID_ARG;
    if (n == 0) return JOLT_OK;
    HostCall call(ctx);
    Fr* d_s = nullptr;
    uint32_t *d_digits = nullptr, *d_neg = nullptr;
    call.up(scalars, n, &d_s);
    call.take(n * (size_t)W, &d_digits);
    call.take(n, &d_neg);
    if (call.ok()) call.e = launch(k_probe_dory_fr_digits, call.st, n, d_s, (int)c, (int)W, d_digits, d_neg);
    call.down(digits_out, d_digits, n * (size_t)W);
    call.down(negative_out, d_neg, n);
    return call.finish("probe dory fr digits");
}

// n dot products over slices of one column of n_terms machine integers of `kind` (JOLT_INT_*: 8 bytes per term, 16 for I128) against n_terms field elements:
// out[i] = sum of values[k] * ints[k] over offsets[i] <= k < offsets[i + 1] (offsets: n + 1 ascending entries, the last at most n_terms), through small_fmadd<2> /
// <4> and small_redc.  With kind I128 and one slice this is jolt_host_small_scalar_dot.
extern "C" int32_t jolt_host_small_scalar_dots(const jolt_fr_t* values, const void* ints, int32_t kind, const uint64_t* offsets, size_t n_terms, size_t n, jolt_fr_t* out) {
    JOLT_TRY(small_dots_args(values, ints, kind, offsets, n_terms, n, out));
    std::vector<Fr> v(n_terms);
    std::vector<uint64_t> z((kind == kIntKindI128 ? 2 : 1) * n_terms);  // copies: the caller's arrays need not be aligned as Fr and uint64_t are
    if (n_terms) {
        std::memcpy(v.data(), values, n_terms * sizeof(Fr));
        std::memcpy(z.data(), ints, z.size() * sizeof(uint64_t));
    }
    for (size_t i = 0; i < n; ++i) fr_to_abi(&out[i], probe::small_scalar_dot(v.data(), z.data(), kind, (size_t)offsets[i], (size_t)offsets[i + 1]));
    return JOLT_OK;
}
extern "C" int32_t jolt_probe_small_scalar_dots(jolt_ctx* ctx, const jolt_fr_t* values, const void* ints, int32_t kind, const uint64_t* offsets, size_t n_terms, size_t n,
                                                jolt_fr_t* out) {
    if (!ctx) return JOLT_ERR_INVALID_ARG;
    JOLT_TRY(small_dots_args(values, ints, kind, offsets, n_terms, n, out));
    if (n == 0) return JOLT_OK;
    HostCall c(ctx);
    Fr *d_values = nullptr, *d_out = nullptr;
    uint64_t *d_ints = nullptr, *d_offsets = nullptr;
    const size_t n_words = (kind == kIntKindI128 ? 2 : 1) * n_terms;
    c.take(n_terms, &d_values);  // (an empty column still gets a block: no lane reads it, nothing is copied into it)
    c.take(n_words, &d_ints);
    if (n_terms) {
        c.h2d(d_values, values, n_terms);
        c.h2d(d_ints, ints, n_words);
    }
    c.up(offsets, n + 1, &d_offsets);
    c.take(n, &d_out);
    if (c.ok()) c.e = launch(k_probe_small_scalar_dots, c.st, n, (const Fr*)d_values, (const void*)d_ints, (int)kind, (const uint64_t*)d_offsets, d_out);
    c.down(out, d_out, n);
    return c.finish("probe small scalar dots");
}
