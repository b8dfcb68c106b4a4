// jolt_amd/csrc/r1cs_rows.hip.h -- one cycle of the uni-skip first round over a constraint system given as ROWS (jolt_r1cs_rows):
// the row values a_i(t), b_i(t) as exact integers, their integer Lagrange extension Az(node), Bz(node) and the exact product.
//
// The reference's optimized tier evaluates the row values of a cycle once and extends them with D-term integer dot products
// (crates/jolt-kernels/src/optimized/spartan_outer.rs:183-340: RowGroupValues, extension_coefficients, extended_products); here the
// same arithmetic for any system of the row object: A rows as signed 128-bit integers, B rows as signed 192-bit integers (row 8 of the
// reference's system carries the constant -2^64, :243-247), Bz in 256 bits, |Az * Bz| < 2^254 by the range contract of include/jolt_hip.h.
// JOLT_HD throughout: k_rows_uniskip (small_r1cs.hip) and jolt_host_r1cs_rows_cycle (r1cs_rows.hip, the CPU suite's hook) compile this text.
#pragma once
#include "small_scalar.hip.h"

namespace jolt {

// What the kernel reads of a jolt_r1cs_rows: slot = stream * D + domain position (an unoccupied slot is an empty row: value 0).  Every
// index below is the same for all lanes of a wavefront.
struct RowsView {
    const uint32_t* a_off;  // [slots + 1] into a_col / a_cf
    const uint32_t* a_col;  // input index (0-based)
    const int64_t* a_cf;
    const int64_t* a_c0;    // [slots]
    const uint32_t* b_off;
    const uint32_t* b_col;
    const int64_t* b_cf;
    const uint64_t* b_c0;   // [slots][2]: signed 128-bit constant (lo, hi), two's complement
    const int64_t* ext;     // [2D - 1][D]: L_i(node), node = position in the extended centred domain
    const uint32_t* nodes;  // [n_eval]: the extended-domain positions to evaluate (all of them, or those outside the domain)
    uint32_t D, n_eval;
};

struct I192 {
    uint64_t w[3];  // two's complement, little-endian
};
struct I256 {
    uint64_t w[4];
};

JOLT_HD unsigned __int128 small_mag128(const SmallInt& z) {
    return ((unsigned __int128)(((uint64_t)z.m[3] << 32) | z.m[2]) << 64) | (((uint64_t)z.m[1] << 32) | z.m[0]);
}

// a[i], b[i] for the D rows of stream s at one cycle; load(c) -> SmallInt of input c at that cycle
template <int DCAP, class Load>
JOLT_HD void rows_cycle_values(const RowsView& rv, uint32_t s, Load&& load, unsigned __int128 (&a)[DCAP], I192 (&b)[DCAP]) {
#pragma unroll
    for (int i = 0; i < DCAP; ++i) {
        a[i] = 0;
        b[i].w[0] = b[i].w[1] = b[i].w[2] = 0;
        if ((uint32_t)i >= rv.D) continue;
        const uint32_t slot = s * rv.D + (uint32_t)i;
        unsigned __int128 av = (unsigned __int128)(__int128)rv.a_c0[slot];
        for (uint32_t k = rv.a_off[slot]; k < rv.a_off[slot + 1]; ++k) {
            const SmallInt z = load(rv.a_col[k]);
            const unsigned __int128 mag = small_mag128(z);
            av += (unsigned __int128)(__int128)rv.a_cf[k] * (z.neg ? (unsigned __int128)0 - mag : mag);  // mod 2^128: exact below 2^127
        }
        a[i] = av;
        const uint64_t c_lo = rv.b_c0[2 * slot], c_hi = rv.b_c0[2 * slot + 1];
        uint64_t w0 = c_lo, w1 = c_hi, w2 = (c_hi >> 63) ? ~(uint64_t)0 : 0;
        for (uint32_t k = rv.b_off[slot]; k < rv.b_off[slot + 1]; ++k) {
            const SmallInt z = load(rv.b_col[k]);
            const int64_t cf = rv.b_cf[k];
            const uint64_t wm = cf < 0 ? (uint64_t)0 - (uint64_t)cf : (uint64_t)cf;
            const uint64_t lo = ((uint64_t)z.m[1] << 32) | z.m[0], hi = ((uint64_t)z.m[3] << 32) | z.m[2];
            const unsigned __int128 p0 = (unsigned __int128)wm * lo, p1 = (unsigned __int128)wm * hi;
            const unsigned __int128 mid = (p0 >> 64) + (uint64_t)p1;
            const uint64_t m0 = (uint64_t)p0, m1 = (uint64_t)mid, m2 = (uint64_t)(p1 >> 64) + (uint64_t)(mid >> 64);
            unsigned long long c = 0;
            if ((cf < 0) != (z.neg != 0)) {
                w0 = __builtin_subcll(w0, m0, c, &c);
                w1 = __builtin_subcll(w1, m1, c, &c);
                w2 = __builtin_subcll(w2, m2, c, &c);
            } else {
                w0 = __builtin_addcll(w0, m0, c, &c);
                w1 = __builtin_addcll(w1, m1, c, &c);
                w2 = __builtin_addcll(w2, m2, c, &c);
            }
        }
        b[i].w[0] = w0;
        b[i].w[1] = w1;
        b[i].w[2] = w2;
    }
}

// Az = sum_i L[i] a[i] (mod 2^128), Bz = sum_i L[i] b[i] (mod 2^256): the integer extension to one node
template <int DCAP>
JOLT_HD void rows_extend(const int64_t* __restrict__ L, uint32_t D, const unsigned __int128 (&a)[DCAP], const I192 (&b)[DCAP], unsigned __int128* az_out, I256* bz_out) {
    unsigned __int128 az = 0;
    I256 bz = {{0, 0, 0, 0}};
#pragma unroll
    for (int i = 0; i < DCAP; ++i) {
        if ((uint32_t)i >= D) continue;
        const int64_t l = L[i];
        if (l == 0) continue;  // wave-uniform
        az += (unsigned __int128)(__int128)l * a[i];
        const uint64_t lm = l < 0 ? (uint64_t)0 - (uint64_t)l : (uint64_t)l;
        const uint64_t bw[4] = {b[i].w[0], b[i].w[1], b[i].w[2], (b[i].w[2] >> 63) ? ~(uint64_t)0 : 0};
        uint64_t p[4], carry = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned __int128 v = (unsigned __int128)bw[j] * lm + carry;
            p[j] = (uint64_t)v;
            carry = (uint64_t)(v >> 64);
        }
        unsigned long long c = 0;
        if (l < 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) bz.w[j] = __builtin_subcll(bz.w[j], p[j], c, &c);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) bz.w[j] = __builtin_addcll(bz.w[j], p[j], c, &c);
        }
    }
    *az_out = az;
    *bz_out = bz;
}

// |Az * Bz| as 8 x 32-bit limbs (< 2^254 by contract) and its sign
JOLT_HD bool rows_product(unsigned __int128 az, const I256& bz, uint32_t (&mag)[8]) {
    const bool a_neg = (uint64_t)(az >> 127) != 0, b_neg = (bz.w[3] >> 63) != 0;
    const unsigned __int128 am = a_neg ? (unsigned __int128)0 - az : az;
    uint64_t bm[4] = {bz.w[0], bz.w[1], bz.w[2], bz.w[3]};
    if (b_neg) {
        unsigned long long c = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) bm[j] = __builtin_subcll(0ull, bm[j], c, &c);
    }
    const uint64_t aw[2] = {(uint64_t)am, (uint64_t)(am >> 64)};
    uint64_t r[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        uint64_t carry = 0;
#pragma unroll
        for (int j = 0; i + j < 4; ++j) {
            const unsigned __int128 v = (unsigned __int128)aw[i] * bm[j] + r[i + j] + carry;
            r[i + j] = (uint64_t)v;
            carry = (uint64_t)(v >> 64);
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        mag[2 * j] = (uint32_t)r[j];
        mag[2 * j + 1] = (uint32_t)(r[j] >> 32);
    }
    return a_neg != b_neg;
}

}  // namespace jolt
