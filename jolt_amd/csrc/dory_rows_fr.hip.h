// jolt_amd/csrc/dory_rows_fr.hip.h -- what the row commitments of a field table (jolt_dory_commit_rows_fr / jolt_dory_hints_rows_fr, dory.hip) add to the integer
// rows: the signed magnitude of a field element, its packed form, the signed window digits of a magnitude of any word count, and the window plan.  JOLT_HD
// throughout: the kernels and the host forms of the suite (jolt_host_dory_fr_digits, jolt_host_dory_rows_fr_plan) run the same code.
//
// A scalar s of StreamingCommitment::feed(&[Fr]) (crates/jolt-dory/src/streaming.rs:53-70) is multiplied as its magnitude min(s, r - s) < 2^253 with the sign folded
// into the point, as the integer rows treat a negative value: small negatives (r - 1, ...) then need as few windows as their absolute value.
#pragma once
#include "field.hip.h"

namespace jolt {
namespace dory_fr {

constexpr int kWords = 8;             // magnitude words of a field element
constexpr int kMaxWindows = 48;       // kMaxRowWindows of dory.hip: the LDS window sums of the row fold
constexpr int kMaxHostWindows = 85;   // ceil(255 / 3): what the host form of the digits takes, which holds no window sums
constexpr size_t kMaxBatchSlots = (size_t)1 << 23;  // bucket slots of one batch of rows: 768 MiB of bucket sums
constexpr uint32_t kSignBit = 1u << 31;  // of word 7 of a packed magnitude: the magnitude ends below bit 253

// canonical value of a Montgomery-form element -> magnitude min(s, r - s) and whether r - s was taken
JOLT_HD void magnitude(const Fr& mont, uint32_t m[kWords], uint32_t& negative) {
    const Fr s = from_mont(mont);
    Fr p, d, t;
#pragma unroll
    for (int i = 0; i < kWords; ++i) p.l[i] = (uint32_t)FrParams::P[i];
    (void)sub256(d, p, s);               // r - s, in [1, r]
    negative = sub256(t, d, s);          // borrow: r - s < s
#pragma unroll
    for (int i = 0; i < kWords; ++i) m[i] = negative ? d.l[i] : s.l[i];
}

JOLT_HD void pack(const uint32_t m[kWords], uint32_t negative, uint4* out) {
    out[0] = make_uint4(m[0], m[1], m[2], m[3]);
    out[1] = make_uint4(m[4], m[5], m[6], m[7] | (negative ? kSignBit : 0u));
}
JOLT_HD void unpack(const uint4* in, uint32_t* m, uint32_t& negative) {
    const uint4 a = in[0], b = in[1];
    m[0] = a.x; m[1] = a.y; m[2] = a.z; m[3] = a.w;
    m[4] = b.x; m[5] = b.y; m[6] = b.z; m[7] = b.w & ~kSignBit;
    negative = b.w >> 31;
}

// The signed digit of window w of a magnitude of NW words, digits in [-2^(c-1), 2^(c-1)] (the carry chain is replayed from window 0: W <= 48 cheap steps)
template <int NW>
JOLT_HD void digit_at(const uint32_t* m, int c, int w, uint32_t& mag, uint32_t& negf) {
    const uint32_t B = 1u << (c - 1);
    uint32_t carry = 0;
    mag = 0;
    negf = 0;
    for (int v = 0; v <= w; ++v) {
        int bit = v * c;
        uint32_t raw = 0;
        if (bit < 32 * NW) {
            int limb = bit >> 5, off = bit & 31;
            uint64_t two = (uint64_t)m[limb] | (limb + 1 < NW ? (uint64_t)m[limb + 1] << 32 : 0ull);
            raw = (uint32_t)(two >> off) & ((1u << c) - 1);
        }
        raw += carry;
        if (raw > B) { mag = (1u << c) - raw; negf = 1; carry = 1; }
        else { mag = raw; negf = 0; carry = 0; }
    }
}

// Window width and count for magnitudes of `bits` bits in rows of 2^wl values.  The integer rows' rule, c = wl - 4 in [3, 13] (~16 points per bucket, never below
// `min_window`) and W = ceil((bits + 1) / c) with one spare bit for the signed-digit carry, needs up to 85 windows at 254 bits; the row fold holds kMaxWindows window
// sums, so c grows until W fits (c = 6 serves 254 bits: 43 windows).  For bits <= 128 nothing grows (c = 3 gives 43) and the plan is the integer rows'.
inline void plan(int bits, int wl, int min_window, int* c_out, int* w_out) {
    int c = wl - 4 < 13 ? wl - 4 : 13;
    if (c < 3) c = 3;
    if (c < min_window) c = min_window;
    while ((bits + c) / c > kMaxWindows) ++c;
    *c_out = c;
    *w_out = (bits + c) / c;
}

}  // namespace dory_fr
}  // namespace jolt
