// jolt_amd/csrc/dory_kernels.hip.h -- what the Dory round entry points share: the two groups behind one interface, the shared scalar's non-adjacent form and its
// walk, the fixed-base table and its signed-nibble walk, one MSM term, the kernels over them and their launch layer (enqueue_*: one launch site per kernel).
// dory_routines.hip runs them on the caller's host arrays, dory_resident.hip and dory_scheme.hip on vectors that stay in HBM.
#pragma once
#include <cstring>

#include "ctx.hpp"
#include "dory_host.hpp"
#include "g1.hip.h"
#include "g2.hip.h"
#include "poly_kernels.hip.h"

namespace jolt {
namespace dory_dev {

using dory_host::kLanes;
using dory_host::parallel_all;

// The two groups behind one set of kernels: G1 through the functions of g1.hip.h as they stand, G2 through g2.hip.h.
struct G1Ops {
    using Pt = G1Jac;
    using Abi = jolt_g1_t;
    static JOLT_HD Pt identity() { return g1_identity(); }
    static JOLT_HD bool is_identity(const Pt& p) { return g1_is_identity(p); }
    static JOLT_HD Pt dbl(const Pt& p) { return g1_double(p); }
    static JOLT_HD Pt add(const Pt& p, const Pt& q) { return g1_add(p, q); }
    static JOLT_HD Pt neg(const Pt& p) { return g1_neg(p); }
    static JOLT_HD bool on_curve(const Pt& p) { return g1_is_on_curve(p); }
};
struct G2Ops {
    using Pt = G2Jac;
    using Abi = jolt_g2_t;
    static JOLT_HD Pt identity() { return g2_identity(); }
    static JOLT_HD bool is_identity(const Pt& p) { return g2_is_identity(p); }
    static JOLT_HD Pt dbl(const Pt& p) { return g2_double(p); }
    static JOLT_HD Pt add(const Pt& p, const Pt& q) { return g2_add(p, q); }
    static JOLT_HD Pt neg(const Pt& p) { return g2_neg(p); }
    static JOLT_HD bool on_curve(const Pt& p) { return g2_is_on_curve(p); }
};
static_assert(sizeof(jolt_g2_t) == sizeof(G2Jac) && sizeof(jolt_fq2_t) == sizeof(Fq2), "G2 ABI layouts");

template <class O>
JOLT_HD typename O::Pt normalised(const typename O::Pt& p) { return O::is_identity(p) ? O::identity() : p; }

// ---- the shared scalar: non-adjacent form, two bits per digit (0: zero, 1: +1, 3: -1), digit i at bits 2 * (i & 15) of w[i >> 4] ----
constexpr int kNafMax = 256;  // s < r < 2^254: the form has at most 255 digits
struct NafPlan {
    uint32_t w[kNafMax / 16];
    int32_t len;  // digits in use; the top one is non-zero (0 for s = 0)
};
JOLT_HD int naf_digit(const NafPlan& plan, int i) {
    const uint32_t d = (plan.w[i >> 4] >> (2 * (i & 15))) & 3u;
    return d == 3u ? -1 : (int)d;
}
// scalar in Montgomery form; false: not canonical
inline bool naf_plan(const jolt_fr_t* scalar, NafPlan* plan) {
    const Fr m = fr_from_abi(scalar);
    if (!fr_is_canonical(m)) return false;
    Fr k = from_mont(m);
    std::memset(plan, 0, sizeof(*plan));
    int i = 0, len = 0;
    while (!k.is_zero()) {
        uint32_t d = 0;
        if (k.l[0] & 1u) {
            if ((k.l[0] & 3u) == 1u) {  // digit +1: clear the low bit
                d = 1u;
                k.l[0] &= ~1u;
            } else {  // digit -1: k + 1 (k < 2^254, no carry out of the top limb)
                d = 3u;
                uint32_t c = 1;
                for (int j = 0; j < 8 && c; ++j) {
                    k.l[j] += c;
                    c = k.l[j] == 0 ? 1u : 0u;
                }
            }
            plan->w[i >> 4] |= d << (2 * (i & 15));
            len = i + 1;
        }
        for (int j = 0; j < 8; ++j) k.l[j] = (k.l[j] >> 1) | (j + 1 < 8 ? k.l[j + 1] << 31 : 0u);
        ++i;
    }
    plan->len = len;
    return true;
}

// s * p along the plan: what every lane of k_dory_scale_add runs, and the host functions of the CPU suite
template <class O>
JOLT_HD typename O::Pt naf_mul(const NafPlan& plan, const typename O::Pt& p) {
    typename O::Pt acc = O::identity();
#pragma unroll 1
    for (int i = plan.len - 1; i >= 0; --i) {
        acc = O::dbl(acc);
        const int d = naf_digit(plan, i);
        if (d != 0) {
            typename O::Pt q = p;
            if (d < 0) q.y = neg(p.y);
            acc = O::add(acc, q);
        }
    }
    return acc;
}
// one element of both shared-scalar routines: addend + s * scaled, the identity as (1, 1, 0)
template <class O>
JOLT_HD typename O::Pt scale_add_one(const NafPlan& plan, const typename O::Pt& scaled, const typename O::Pt& addend) {
    return normalised<O>(O::add(naf_mul<O>(plan, scaled), addend));
}

// k << S over the eight limbs (S < 32): the scalar walks are MSB-first shifts of the whole integer, so no limb is ever indexed by a loop variable
template <int S>
JOLT_HD void shl256(Fr& k) {
#pragma unroll
    for (int j = 7; j >= 1; --j) k.l[j] = (k.l[j] << S) | (k.l[j - 1] >> (32 - S));
    k.l[0] <<= S;
}

// one term of the MSM: plain MSB-first double-and-add over the canonical scalar (the digits differ from lane to lane)
template <class O>
JOLT_HD typename O::Pt term_mul_one(const typename O::Pt& p, const Fr& scalar_mont) {
    Fr k = from_mont(scalar_mont);
    shl256<2>(k);  // r < 2^254: bit 253 to the top
    typename O::Pt acc = O::identity();
#pragma unroll 1
    for (int i = 253; i >= 0; --i) {
        acc = O::dbl(acc);
        const bool bit = (k.l[7] >> 31) != 0;
        shl256<1>(k);
        if (bit) acc = O::add(acc, p);
    }
    return acc;
}

// ---- per-element scalars over one base: signed 4-bit windows, table[k] = k * base for k = 0..8 ----
constexpr int kFixedWindow = 4;
constexpr int kFixedWindows = 64;  // 256 bits; digits in [-8, 7] (fixed_mul_one)
constexpr int kFixedTable = (1 << (kFixedWindow - 1)) + 1;
template <class O>
void fixed_table(const typename O::Pt& base, typename O::Pt* table) {
    table[0] = O::identity();
    table[1] = base;
    for (int k = 2; k < kFixedTable; ++k) table[k] = (k & 1) ? O::add(table[k - 1], base) : O::dbl(table[k / 2]);
}
// from a base point of the ABI (checked by the caller).  The table stays in the caller's frame: its upload reads it until the caller's synchronise
template <class O>
void fixed_table_from_abi(const void* base, typename O::Pt (&table)[kFixedTable]) {
    fixed_table<O>(dory_host::pt_from_abi<typename O::Pt>(base), table);
}
// scalar * base.  Signed digits without a carry chain: k' = k + 0x88..8 (8 in each of the 64 nibbles; k < 2^254, so k' < 2^256), digit w = nibble w of k' - 8 in [-8, 7],
// since sum_w 8 * 16^w is exactly what was added.  The table entry is taken by index (digits differ from lane to lane), its sign by a select on y.
template <class O>
JOLT_HD typename O::Pt fixed_mul_one(const typename O::Pt* __restrict__ table, const Fr& scalar_mont) {
    Fr k = from_mont(scalar_mont);
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) k.l[j] = __builtin_addc(k.l[j], 0x88888888u, c, &c);
    typename O::Pt acc = O::identity();
#pragma unroll 1
    for (int w = kFixedWindows - 1; w >= 0; --w) {
#pragma unroll 1
        for (int j = 0; j < kFixedWindow; ++j) acc = O::dbl(acc);
        const uint32_t nib = k.l[7] >> 28;
        shl256<kFixedWindow>(k);
        const bool negative = nib < 8u;
        const uint32_t mag = negative ? 8u - nib : nib - 8u;
        typename O::Pt t = table[mag];
        if (negative) t = O::neg(t);
        acc = O::add(acc, t);
    }
    return normalised<O>(acc);
}

// ---- kernels: one wavefront per workgroup (kLanes), one wavefront per SIMD (a G2 addition holds two 48-register points and its temporaries) ----
// out[i] = addend[i] + s * scaled[i], as scale_add_one; out may alias either input (each lane reads its own element before it writes it)
template <class O>
__global__ __launch_bounds__(kLanes) void k_dory_scale_add(NafPlan plan, const typename O::Pt* scaled, const typename O::Pt* addend, typename O::Pt* out, size_t n) {
    const size_t i = (size_t)blockIdx.x * kLanes + threadIdx.x;
    if (i >= n) return;
    const typename O::Pt acc = naf_mul<O>(plan, scaled[i]);
    out[i] = normalised<O>(O::add(acc, addend[i]));  // the addend is loaded after the walk: 48 registers of a G2 point that the loop does not have to carry
}
template <class O>
__global__ __launch_bounds__(kLanes) void k_dory_msm_terms(const typename O::Pt* __restrict__ bases, const Fr* __restrict__ scalars, typename O::Pt* __restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * kLanes + threadIdx.x;
    if (i >= n) return;
    out[i] = term_mul_one<O>(bases[i], scalars[i]);
}
template <class O>
__global__ __launch_bounds__(kLanes) void k_dory_fixed_base(const typename O::Pt* __restrict__ table, const Fr* __restrict__ scalars, typename O::Pt* __restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * kLanes + threadIdx.x;
    if (i >= n) return;
    out[i] = fixed_mul_one<O>(table, scalars[i]);
}
// one level of a halving tree: v[i] = v[i] (x) v[i + half] for i + half < m.  Op: AddPt<O> for the sums of an MSM, MulFq12 (dory_prepared.hip.h) for the product of
// the Miller values; k_batch_tree_level of dory_resident.hip takes the same step inside every item's segment
template <class O>
struct AddPt {
    static JOLT_HD typename O::Pt combine(const typename O::Pt& a, const typename O::Pt& b) { return O::add(a, b); }
};
template <class T, class Op>
__global__ __launch_bounds__(kLanes) void k_tree_level(T* v, size_t half, size_t m) {
    const size_t i = (size_t)blockIdx.x * kLanes + threadIdx.x;
    if (i >= half || i + half >= m) return;
    v[i] = Op::combine(v[i], v[i + half]);
}
static __global__ __launch_bounds__(256) void k_dory_fold_field(Fr* __restrict__ left, const Fr* __restrict__ right, Fr s, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    st_fr(left + i, add(mul(ld_fr(left + i), s), ld_fr(right + i)));
}

// ---- the launch layer: THE launch site of each kernel above, over device pointers, n > 0.  These only enqueue on `st` and return hipGetLastError(); the host-pointer
// entries (dory_routines.hip, dory_pairing.hip), the resident ones (dory_resident.hip) and a round's update (dory_scheme.hip) all go through them ----
template <class O>
hipError_t enqueue_scale_add(hipStream_t st, const NafPlan& plan, const typename O::Pt* scaled, const typename O::Pt* addend, typename O::Pt* out, size_t n) {
    hipLaunchKernelGGL(k_dory_scale_add<O>, dim3(dory_host::lanes_grid(n)), dim3(kLanes), 0, st, plan, scaled, addend, out, n);
    return hipGetLastError();
}
inline hipError_t enqueue_fold_field(hipStream_t st, Fr* left, const Fr* right, const Fr& s, size_t n) {
    hipLaunchKernelGGL(k_dory_fold_field, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, left, right, s, n);
    return hipGetLastError();
}
// d_table: fixed_table's kFixedTable points on the device
template <class O>
hipError_t enqueue_fixed_base(hipStream_t st, const typename O::Pt* d_table, const Fr* d_scalars, typename O::Pt* d_out, size_t n) {
    hipLaunchKernelGGL(k_dory_fixed_base<O>, dim3(dory_host::lanes_grid(n)), dim3(kLanes), 0, st, d_table, d_scalars, d_out, n);
    return hipGetLastError();
}
// the halving loop: the result in d_v[0], NOT normalised
template <class T, class Op>
hipError_t enqueue_tree(hipStream_t st, T* d_v, size_t n) {
    for (size_t m = n; m > 1;) {
        const size_t half = (m + 1) / 2;
        hipLaunchKernelGGL((k_tree_level<T, Op>), dim3(dory_host::lanes_grid(half)), dim3(kLanes), 0, st, d_v, half, m);
        m = half;
    }
    return hipGetLastError();
}
// sum_i scalars[i] * bases[i] into d_terms[0] (n terms of scratch): the term launch and the addition tree
template <class O>
hipError_t enqueue_msm(hipStream_t st, const typename O::Pt* d_bases, const Fr* d_scalars, typename O::Pt* d_terms, size_t n) {
    hipLaunchKernelGGL(k_dory_msm_terms<O>, dim3(dory_host::lanes_grid(n)), dim3(kLanes), 0, st, d_bases, d_scalars, d_terms, n);
    return enqueue_tree<typename O::Pt, AddPt<O>>(st, d_terms, n);
}

// ---- the argument checks of the entry points ----
template <class O>
bool all_on_curve(const typename O::Abi* pts, size_t n) {
    return parallel_all(n, [pts](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; ++i) {
            typename O::Pt p;
            std::memcpy(&p, &pts[i], sizeof(p));
            if (!O::on_curve(p)) return false;
        }
        return true;
    });
}
inline bool all_canonical(const jolt_fr_t* s, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (!fr_is_canonical(fr_from_abi(&s[i]))) return false;
    return true;
}

constexpr size_t kMaxElements = (size_t)1 << 30;  // keeps every grid below 2^31 workgroups; a Dory round holds 2^nu <= 2^20 points

}  // namespace dory_dev
}  // namespace jolt
