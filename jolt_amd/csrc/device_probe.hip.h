// jolt_amd/csrc/device_probe.hip.h -- the per-tuple bodies of the device twins (jolt_probe_*, device_probe.hip) of the suite's host forms (jolt_host_*).
//
// Every body is ONE JOLT_HD function over the functions the kernels call (field.hip.h, fq_limb.hip.h, fq2.hip.h, g2.hip.h, fq12.hip.h, suffix_mle.hip.h,
// dory_rows_fr.hip.h, small_scalar.hip.h); the probe kernel runs it in one lane per tuple.  The host forms that live in host_mirror.hip (jolt_host_fq_limb_op,
// jolt_host_g1xl_add_paths) and here (jolt_host_field_op, jolt_host_small_scalar_dots) compile these very bodies for the CPU.  The older host forms of the other
// families stay where their kernels are and spell the same few calls out themselves: jolt_host_suffix_mle (read_raf.hip) beside suffix_masked,
// jolt_host_dory_fr_digits (dory.hip) beside dory_fr_digits, jolt_host_small_scalar_dot (small_r1cs.hip) beside small_scalar_dot, the switches of
// jolt_host_fq2_op / jolt_host_g2_* (dory_routines.hip) and jolt_host_fq12_op (dory_pairing.hip) beside fq2_op / fq12_op; tests/test_gpu_device_probe.py compares
// every twin with its host form bit for bit, which is also what holds the two spellings together.  What differs between the two builds is what the probe is for:
// `mul` is mul_limbs29 on the device and host_mul64 on the host, the limb-form multiply-accumulate is inline assembly on the device, the suffixes' bit counts are
// intrinsics, and carry chains and funnel shifts go through another backend.
#pragma once
#include "dory_rows_fr.hip.h"
#include "field.hip.h"
#include "fq12.hip.h"
#include "fq2.hip.h"
#include "fq_limb.hip.h"
#include "g1.hip.h"
#include "g2.hip.h"
#include "small_scalar.hip.h"
#include "suffix_mle.hip.h"

namespace jolt {
namespace probe {

// = JOLT_PROBE_* of include/jolt_hip.h
enum { kMul = 0, kSqr = 1, kAdd = 2, kSub = 3, kNeg = 4, kDbl = 5, kFromMont = 6, kToMont = 7, kMulShifted = 8, kNumFieldOps = 9 };
constexpr bool field_op_is_binary(int op) { return op == kMul || op == kAdd || op == kSub || op == kMulShifted; }

// The multiplication the kernels use.  On the device that is `mul` itself; the host form spells the device algorithm out (on the host `mul` is host_mul64).
template <class PR>
JOLT_HD Fp<PR> device_mul(const Fp<PR>& a, const Fp<PR>& b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return mul(a, b);
#else
    return mul_limbs29(a, b);
#endif
}
template <class PR, int OP>
JOLT_HD Fp<PR> field_op(const Fp<PR>& a, const Fp<PR>& b) {
    if (OP == kMul) return device_mul(a, b);
    if (OP == kSqr) {
#if defined(__HIP_DEVICE_COMPILE__)
        return sqr(a);
#else
        return mul_limbs29(a, a);
#endif
    }
    if (OP == kAdd) return add(a, b);
    if (OP == kSub) return sub(a, b);
    if (OP == kNeg) return neg(a);
    if (OP == kDbl) return dbl(a);
    if (OP == kFromMont) {
#if defined(__HIP_DEVICE_COMPILE__)
        return from_mont(a);
#else
        Fp<PR> one_int = Fp<PR>::zero();
        one_int.l[0] = 1;
        return mul_limbs29(a, one_int);
#endif
    }
    if (OP == kToMont) {
#if defined(__HIP_DEVICE_COMPILE__)
        return to_mont(a);
#else
        return mul_limbs29(a, Fp<PR>::r2());
#endif
    }
    const uint32_t chi[4] = {b.l[4], b.l[5], b.l[6], b.l[7]};  // kMulShifted: b's four low limbs are zero (the entries check)
    return mul_shifted(a, chi);
}

// ---- limb-form Fq (fq_limb.hip.h).  Operands are canonical Fq in STANDARD Montgomery form; they are taken to L-form (x * 2^261: a product with the Montgomery form
// of 32), combined there, and the result is brought back.  op 0: a * b   1: a^2   2: a * b + c * d (one reduction)   3: (a - b) * c through the lazily reduced
// difference a + 8p - b   4: (a - b - 2c) * d through a + 6p - b - 2c.
constexpr int kNumLimbOps = 5;
JOLT_HD Fq mont_thirty_two() {
    Fq thirty_two = Fq::zero();
    thirty_two.l[0] = 32;
    return to_mont(thirty_two);
}
template <int OP>
JOLT_HD Fq fq_limb_op(const Fq& a, const Fq& b, const Fq& c, const Fq& d) {
    const Fq m32 = mont_thirty_two();
    const FqL la = fql_from_words(mul(a, m32)), lb = fql_from_words(mul(b, m32)), lc = fql_from_words(mul(c, m32)), ld = fql_from_words(mul(d, m32));
    const FqL r256 = fql_from_words(Fq::one());
    FqL r;
    if (OP == 0) r = fql_mul(la, lb);
    else if (OP == 1) r = fql_sqr(la);
    else if (OP == 2) r = fql_mul2(la, lb, lc, ld);
    else if (OP == 3) r = fql_mul(fql_diff<8, false>(la, lb, la), lc);
    else r = fql_mul(fql_diff<6, true>(la, lb, lc), ld);
    return fql_to_std(r, r256);
}

// ONE mixed addition on raw limbs through both paths of fq_limb.hip.h: `common` = g1xl_add_mixed_common, `full` = the unchanged g1xl_add_mixed on (qx, +-qy),
// `step` = what a loop iteration leaves (common, then g1xl_add_mixed_rare when suspect), canon = common and full as canonical field elements (X, Y, ZZ, ZZZ each).
struct AddPaths {
    G1XyzzL common, full, step;
    int32_t suspect;
    Fq canon[8];
};
JOLT_HD void g1xl_add_paths(const G1XyzzL& p, const FqL& qx, const FqL& qy, bool negate, AddPaths& out) {
    const FqL one = fql_from_words(mont_thirty_two()), r256 = fql_from_words(Fq::one());
    const uint32_t neg_mask = negate ? ~0u : 0u;
    bool sus = false;
    out.common = g1xl_add_mixed_common(p, qx, qy, neg_mask, sus);
    out.full = g1xl_add_mixed(p, qx, fql_signed_y(qy, neg_mask), one);
    bool ident = g1xl_is_identity(p);  // the bit a loop carries beside its accumulator
    out.step = out.common;
    if (sus) out.step = g1xl_add_mixed_rare(out.common, ident, qx, qy, neg_mask, one);
    out.suspect = sus ? 1 : 0;
    out.canon[0] = fql_to_std(out.common.x, r256);
    out.canon[1] = fql_to_std(out.common.y, r256);
    out.canon[2] = fql_to_std(out.common.zz, r256);
    out.canon[3] = fql_to_std(out.common.zzz, r256);
    out.canon[4] = fql_to_std(out.full.x, r256);
    out.canon[5] = fql_to_std(out.full.y, r256);
    out.canon[6] = fql_to_std(out.full.zz, r256);
    out.canon[7] = fql_to_std(out.full.zzz, r256);
}

// ---- Fq2, G2, Fq12: op = JOLT_FQ2_* / JOLT_PROBE_G2_* / JOLT_FQ12_* of include/jolt_hip.h
template <int OP>
JOLT_HD Fq2 fq2_op(const Fq2& a, const Fq2& b) {
    if (OP == 0) return add(a, b);
    if (OP == 1) return sub(a, b);
    if (OP == 2) return mul(a, b);
    if (OP == 3) return sqr(a);
    return neg(a);
}
enum { kG2Add = 0, kG2Double = 1, kG2Eq = 2 };
enum { kFq12Mul = 0, kFq12Sqr = 1, kFq12Conj = 3, kFq12MulSparse = 7 };
JOLT_HD bool fq12_sparse_shape(const Fq12& b) { return b.c0.c1.is_zero() && b.c0.c2.is_zero() && b.c1.c2.is_zero(); }
template <int OP>
JOLT_HD Fq12 fq12_op(const Fq12& a, const Fq12& b) {
    if (OP == kFq12Mul) return mul(a, b);
    if (OP == kFq12Sqr) return sqr(a);
    if (OP == kFq12Conj) return conj(a);
    return mul_by_034(a, b.c0.c0, b.c1.c0, b.c1.c1);
}

// ---- suffixes: bits masked to `len` (LookupBits::new), then suffix_mle
JOLT_HD uint64_t suffix_masked(uint32_t kind, uint64_t lo, uint64_t hi, uint32_t len) {
    if (len < 128) {
        if (len >= 64) hi &= len == 64 ? 0ull : ((1ull << (len - 64)) - 1);
        else { hi = 0; lo &= len == 0 ? 0ull : ((1ull << len) - 1); }
    }
    return suffix_mle(kind, lo, hi, len);
}

// ---- Dory field rows: digits_out[w] = magnitude | negative << 31 of the signed digit of window w of min(s, r - s), through the packed form the kernels keep
JOLT_HD void dory_fr_digits(const Fr& s, int c, int W, uint32_t* digits_out, uint32_t& negative_out) {
    uint32_t m[dory_fr::kWords], negv, packed_neg;
    dory_fr::magnitude(s, m, negv);
    uint4 packed[2];
    dory_fr::pack(m, negv, packed);
    dory_fr::unpack(packed, m, packed_neg);
    for (int w = 0; w < W; ++w) {
        uint32_t mag, negf;
        dory_fr::digit_at<dory_fr::kWords>(m, c, w, mag, negf);
        digits_out[w] = mag | (negf << 31);
    }
    negative_out = packed_neg;
}

// ---- small-scalar accumulator (small_scalar.hip.h): sum_{first <= k < last} values[k] * ints[k] for a column of machine integers of `kind` (JOLT_INT_*), summed
// unreduced by sign in 13 limbs (two limbs of a 64-bit magnitude, four of a 128-bit one), ONE REDC each, brought back to Montgomery form
JOLT_HD Fr small_scalar_dot(const Fr* __restrict__ values, const void* __restrict__ ints, int kind, size_t first, size_t last) {
    SmallAcc pos = small_zero(), neg_acc = small_zero();
    for (size_t k = first; k < last; ++k) {
        const SmallInt s = load_small(ints, kind, k);
        const Fr v = values[k];
        if (kind == kIntKindI128) {
            if (s.neg) small_fmadd<4>(neg_acc, v, s.m);
            else small_fmadd<4>(pos, v, s.m);
        } else {
            if (s.neg) small_fmadd<2>(neg_acc, v, s.m);
            else small_fmadd<2>(pos, v, s.m);
        }
    }
    return mul(sub(small_redc<FrParams>(pos), small_redc<FrParams>(neg_acc)), Fr::r2());
}

}  // namespace probe
}  // namespace jolt
