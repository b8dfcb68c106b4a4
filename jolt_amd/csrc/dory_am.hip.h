// jolt_amd/csrc/dory_am.hip.h -- Dory tier 1 and the opening's row fold in the ADDRESS-MAJOR trace placement (docs/kernels.md 3.5k).
//
// TracePolynomialOrder::AddressMajor (crates/jolt-claims/src/protocols/jolt/geometry/dimensions.rs:20-59; placed by TracePlacement,
// crates/jolt-kernels/src/optimized/opening.rs:340-373): the coefficient of (cycle t, address k) sits at grid index
//   (t << log_block) + (k << log_stride),   log_block = log2 cycle_stride(), log_stride = log2 one_hot_stride(),
// dense columns at k = 0.  With 2^sigma matrix columns and sigma >= log_block a row holds C = 2^(sigma - log_block) WHOLE cycles: row r is
// the cycles [r C, (r + 1) C), every column has T / C rows, and a row's cycles are contiguous in the hot-index array and already in order.
// So the row commitments need no keys, no scan and no scatter: one lane owns one (column, row) and walks its C cycles,
//   hint[r] = sum_{j < C, hot(r C + j) not cold} Gamma1[(j << log_block) + (hot(r C + j) << log_stride)],
// in lockstep with its wavefront -- at step j all 64 lanes gather inside the one block Gamma1[(j << log_block) ...] of 2^log_block points.
// The running sum is the limb-form XYZZ accumulator of fq_limb.hip.h (g1xl_accumulate: the rare cases of the mixed addition out of line,
// behind one wave-uniform branch), over an L-form copy of the first 2^sigma bases made once per call.
// Integer VALU work, no MFMA, no scratch; workgroups of one wavefront.
#pragma once
#include "fq_limb.hip.h"
#include "g1.hip.h"

namespace jolt {
namespace dory_am {

constexpr int kLanes = 64;

// TracePlacement's formula (address_cycle_to_index for an unwidened grid, where it is cycle * num_addresses + address)
JOLT_HD size_t place(uint32_t log_block, uint32_t log_stride, size_t cycle, size_t address) { return (cycle << log_block) + (address << log_stride); }

struct Consts {
    Fq one_l;  // L-form of 1 = the standard Montgomery form of 32
    Fq r256;   // 2^256 mod p = the words of Fq::one()
};
inline Consts consts() {
    Fq thirty_two = Fq::zero();
    thirty_two.l[0] = 32;
    Consts c;
    c.one_l = to_mont(thirty_two);
    c.r256 = Fq::one();
    return c;
}
// a base in the standard Montgomery form -> L-form: every coordinate times 32; (0, 0) stays (0, 0)
JOLT_HD G1Affine to_lform(const G1Affine& p, const Fq& mont32) {
    G1Affine r;
    r.x = mul(p.x, mont32);
    r.y = mul(p.y, mont32);
    return r;
}

// The sum of one row.  hot(j): the hot address of the row's cycle j, j = 0, 1, ... in order, anything >= K for a cold cycle; table: the L-form bases;
// load(p): the point at p.  The next cycle's index and base are in flight while the current addition runs.  Every exceptional case of the addition goes through
// g1xl_accumulate: an identity accumulator (the start, or after P - P in the middle of a row) and a doubling both show as ZZ3 = 0 and take the rare path.
template <class Hot, class Load>
JOLT_HD G1Jac row_sum(uint32_t C, uint32_t K, uint32_t log_block, uint32_t log_stride, Hot&& hot, const G1Affine* __restrict__ table, Load&& load, const Consts& lc) {
    const FqL one = fql_from_words(lc.one_l);
    G1XyzzL acc = g1xl_identity();
    bool ident = true;
    uint32_t h = hot(0u);
    const G1Affine* src = table + place(log_block, log_stride, 0, h < K ? h : 0u);
    G1Affine p = load(src);
    for (uint32_t j = 0; j < C; ++j) {
        uint32_t hn = K;
        const G1Affine* srcn = src;
        G1Affine pn = p;
        if (j + 1 < C) {
            hn = hot(j + 1);
            srcn = table + place(log_block, log_stride, j + 1, hn < K ? hn : 0u);  // a cold cycle reads the block's first base and adds nothing
            pn = load(srcn);
        }
        if (h < K) g1xl_accumulate(acc, ident, p, src, 0u, one);
        h = hn;
        src = srcn;
        p = pn;
    }
    if (ident) return g1_identity();
    const FqL r256 = fql_from_words(lc.r256);
    G1Jac out;  // (X, Y, ZZ, ZZZ) ~ Jacobian (X ZZ^2, Y ZZZ^2, ZZZ)
    out.x = fql_to_std(fql_mul(acc.x, fql_sqr(acc.zz)), r256);
    out.y = fql_to_std(fql_mul(acc.y, fql_sqr(acc.zzz)), r256);
    out.z = fql_to_std(acc.zzz, r256);
    return out;
}

#if defined(__HIPCC__)
// out[i] = srs[i << shift], in L-form when mont32 is given (lform != 0): the one-hot kernel's table (shift 0) and the C strided bases of the dense rows
__global__ __launch_bounds__(256) void k_dory_am_bases(const G1Affine* __restrict__ srs, size_t n, uint32_t shift, uint32_t lform, Fq mont32, G1Affine* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const G1Affine p = srs[i << shift];
    out[i] = lform ? to_lform(p, mont32) : p;
}

// A row's index bytes, 8 at a time: lanes of a wavefront read rows that are C entries apart, so a lane fetches the 8 bytes of its next 8 (4 for 16-bit indices) cycles
// with one load and shifts them out; rows shorter than 8 bytes (or an unaligned array) load entry by entry.
struct HotWords {
    const uint8_t* __restrict__ row;
    uint32_t wide, words;
    uint64_t w;
    __device__ __forceinline__ uint32_t operator()(uint32_t j) {
        uint32_t v;
        if (words) {
            const uint32_t per = 8u >> wide, sub = j & (per - 1);
            if (sub == 0) w = *reinterpret_cast<const uint64_t*>(row + ((size_t)j << wide));
            v = wide ? (uint32_t)(w >> (16 * sub)) & 0xFFFFu : (uint32_t)(w >> (8 * sub)) & 0xFFu;
        } else {
            v = wide ? (uint32_t) reinterpret_cast<const uint16_t*>(row)[j] : (uint32_t)row[j];
        }
        return v == (wide ? 0xFFFFu : 0xFFu) ? 0xFFFFFFFFu : v;
    }
};
__device__ __forceinline__ G1Affine ld_base(const G1Affine* p) {
    const uint4* q = reinterpret_cast<const uint4*>(p);
    const uint4 a = q[0], b = q[1], c = q[2], d = q[3];
    G1Affine r;
    r.x.l[0] = a.x; r.x.l[1] = a.y; r.x.l[2] = a.z; r.x.l[3] = a.w; r.x.l[4] = b.x; r.x.l[5] = b.y; r.x.l[6] = b.z; r.x.l[7] = b.w;
    r.y.l[0] = c.x; r.y.l[1] = c.y; r.y.l[2] = c.z; r.y.l[3] = c.w; r.y.l[4] = d.x; r.y.l[5] = d.y; r.y.l[6] = d.z; r.y.l[7] = d.w;
    return r;
}

// Lane = item = (column, row) of a launch set: idx points at the first item's first cycle, and item i's C cycles follow at entry i * C (a column's cycles are its
// rows back to back and the columns of a source are contiguous, so a launch set may start and end inside a column).  out[i]: the row's sum, Jacobian.
__global__ __launch_bounds__(kLanes) void k_dory_am_onehot_rows(const uint8_t* __restrict__ idx, uint32_t wide, uint32_t words, size_t n_items, uint32_t C, uint32_t K,
                                                                uint32_t log_block, uint32_t log_stride, const G1Affine* __restrict__ table, Consts lc,
                                                                G1Jac* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * kLanes + threadIdx.x;
    if (i >= n_items) return;
    HotWords hot{idx + ((i * C) << wide), wide, words, 0ull};
    out[i] = row_sum(C, K, log_block, log_stride, hot, table, [](const G1Affine* p) { return ld_base(p); }, lc);
}
#endif

}  // namespace dory_am
}  // namespace jolt
