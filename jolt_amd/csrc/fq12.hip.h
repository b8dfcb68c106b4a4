// jolt_amd/csrc/fq12.hip.h -- the tower Fq6 = Fq2[v] / (v^3 - xi), Fq12 = Fq6[w] / (w^2 - v) with xi = 9 + u, over fq2.hip.h, for device and host.
//
// Layout = ark_bn254::Fq12 (QuadExtField over CubicExtField: c0, c1, each c0, c1, c2), which Bn254GT wraps (crates/jolt-crypto/src/ec/bn254/gt.rs:30-32):
// twelve Montgomery Fq in the order c0.c0.c0, c0.c0.c1, c0.c1.c0, ..., c1.c2.c1.  The Fq2 coefficient c_h.c_j multiplies w^(2 j + h) (v = w^2).
// The Frobenius constants gamma_{e,k} = xi^(k (p^e - 1) / 6) come from pairing_constants.hip.h (tools/gen_pairing_constants.py); the Frobenius maps and the
// inverse of Fq12 are used by the final exponentiation only, which runs on the host.  Inversion in Fq is Fermat's, walked MSB-first by shifting the whole
// exponent: no limb array is ever indexed by a loop variable (docs/kernels.md 3.5f).
#pragma once
#include "fq2.hip.h"
#include "pairing_constants.hip.h"

namespace jolt {

struct PairingConsts {
    static constexpr uint32_t FROB1[6][2][8] = PAIRING_FROB1_LIMBS;
    static constexpr uint32_t FROB2[6][2][8] = PAIRING_FROB2_LIMBS;
    static constexpr uint32_t FROB3[6][2][8] = PAIRING_FROB3_LIMBS;
    static constexpr uint32_t TWIST_3B[2][8] = PAIRING_TWIST_3B_LIMBS;
};
// an Fq2 constant out of a [2][8] limb table; the indices are compile-time constants once unrolled
#define JOLT_FQ2_CONST(dst, TABLE)                      \
    do {                                                \
        _Pragma("unroll") for (int i_ = 0; i_ < 8; ++i_) { \
            (dst).c0.l[i_] = TABLE[0][i_];              \
            (dst).c1.l[i_] = TABLE[1][i_];              \
        }                                               \
    } while (0)

// ---- Fq and Fq2 inversion ----
// a^(p - 2); zero maps to zero.  254 squarings and the multiplications of the set bits, the same sequence in every lane
JOLT_HD Fq fq_inv_fermat(const Fq& a) {
    Fq k;  // p - 2, then shifted so that bit 253 is the top bit (p < 2^254, and p's lowest limb is above 2)
#pragma unroll
    for (int j = 0; j < 8; ++j) k.l[j] = FqParams::P[j];
    k.l[0] -= 2u;
#pragma unroll
    for (int j = 7; j >= 1; --j) k.l[j] = (k.l[j] << 2) | (k.l[j - 1] >> 30);
    k.l[0] <<= 2;
    Fq acc = Fq::one();
#pragma unroll 1
    for (int i = 0; i < 254; ++i) {
        acc = sqr(acc);
        const bool bit = (k.l[7] >> 31) != 0;
#pragma unroll
        for (int j = 7; j >= 1; --j) k.l[j] = (k.l[j] << 1) | (k.l[j - 1] >> 31);
        k.l[0] <<= 1;
        if (bit) acc = mul(acc, a);
    }
    return acc;
}
JOLT_HD Fq2 conj(const Fq2& a) {
    Fq2 r;
    r.c0 = a.c0;
    r.c1 = neg(a.c1);
    return r;
}
JOLT_HD Fq2 mul_fq(const Fq2& a, const Fq& s) {
    Fq2 r;
    r.c0 = mul(a.c0, s);
    r.c1 = mul(a.c1, s);
    return r;
}
// conj(a) / (a0^2 + a1^2); zero maps to zero
JOLT_HD Fq2 fq2_inv(const Fq2& a) {
    const Fq n = fq_inv_fermat(add(sqr(a.c0), sqr(a.c1)));
    return mul_fq(conj(a), n);
}

// ---- Fq6 ----
struct Fq6 {
    Fq2 c0, c1, c2;
    static JOLT_HD Fq6 zero() {
        Fq6 r;
        r.c0 = r.c1 = r.c2 = Fq2::zero();
        return r;
    }
    static JOLT_HD Fq6 one() {
        Fq6 r = zero();
        r.c0 = Fq2::one();
        return r;
    }
    JOLT_HD bool is_zero() const { return c0.is_zero() && c1.is_zero() && c2.is_zero(); }
    JOLT_HD bool operator==(const Fq6& o) const { return c0 == o.c0 && c1 == o.c1 && c2 == o.c2; }
};
JOLT_HD Fq6 add(const Fq6& a, const Fq6& b) {
    Fq6 r;
    r.c0 = add(a.c0, b.c0);
    r.c1 = add(a.c1, b.c1);
    r.c2 = add(a.c2, b.c2);
    return r;
}
JOLT_HD Fq6 sub(const Fq6& a, const Fq6& b) {
    Fq6 r;
    r.c0 = sub(a.c0, b.c0);
    r.c1 = sub(a.c1, b.c1);
    r.c2 = sub(a.c2, b.c2);
    return r;
}
JOLT_HD Fq6 neg(const Fq6& a) {
    Fq6 r;
    r.c0 = neg(a.c0);
    r.c1 = neg(a.c1);
    r.c2 = neg(a.c2);
    return r;
}
JOLT_HD Fq6 dbl(const Fq6& a) {
    Fq6 r;
    r.c0 = dbl(a.c0);
    r.c1 = dbl(a.c1);
    r.c2 = dbl(a.c2);
    return r;
}
// a * v: (xi a2, a0, a1)
JOLT_HD Fq6 mul_by_v(const Fq6& a) {
    Fq6 r;
    r.c0 = mul_by_xi(a.c2);
    r.c1 = a.c0;
    r.c2 = a.c1;
    return r;
}
// Karatsuba over Fq2, six multiplications
JOLT_HD Fq6 mul(const Fq6& a, const Fq6& b) {
    const Fq2 v0 = mul(a.c0, b.c0), v1 = mul(a.c1, b.c1), v2 = mul(a.c2, b.c2);
    Fq6 r;
    r.c0 = add(v0, mul_by_xi(sub(sub(mul(add(a.c1, a.c2), add(b.c1, b.c2)), v1), v2)));
    r.c1 = add(sub(sub(mul(add(a.c0, a.c1), add(b.c0, b.c1)), v0), v1), mul_by_xi(v2));
    r.c2 = add(sub(sub(mul(add(a.c0, a.c2), add(b.c0, b.c2)), v0), v2), v1);
    return r;
}
// a * (b0 + b1 v), five multiplications
JOLT_HD Fq6 mul_by_01(const Fq6& a, const Fq2& b0, const Fq2& b1) {
    const Fq2 v0 = mul(a.c0, b0), v1 = mul(a.c1, b1);
    Fq6 r;
    r.c0 = add(v0, mul_by_xi(sub(mul(add(a.c1, a.c2), b1), v1)));
    r.c1 = sub(sub(mul(add(a.c0, a.c1), add(b0, b1)), v0), v1);
    r.c2 = add(sub(mul(add(a.c0, a.c2), b0), v0), v1);
    return r;
}
JOLT_HD Fq6 mul_fq2(const Fq6& a, const Fq2& s) {
    Fq6 r;
    r.c0 = mul(a.c0, s);
    r.c1 = mul(a.c1, s);
    r.c2 = mul(a.c2, s);
    return r;
}
// Chung-Hasan SQR2: three squarings and two multiplications
JOLT_HD Fq6 sqr(const Fq6& a) {
    const Fq2 s0 = sqr(a.c0), s1 = dbl(mul(a.c0, a.c1)), s2 = sqr(add(sub(a.c0, a.c1), a.c2)), s3 = dbl(mul(a.c1, a.c2)), s4 = sqr(a.c2);
    Fq6 r;
    r.c0 = add(s0, mul_by_xi(s3));
    r.c1 = add(s1, mul_by_xi(s4));
    r.c2 = sub(sub(add(add(s1, s2), s3), s0), s4);
    return r;
}
// zero maps to zero
JOLT_HD Fq6 fq6_inv(const Fq6& a) {
    const Fq2 t0 = sub(sqr(a.c0), mul_by_xi(mul(a.c1, a.c2)));
    const Fq2 t1 = sub(mul_by_xi(sqr(a.c2)), mul(a.c0, a.c1));
    const Fq2 t2 = sub(sqr(a.c1), mul(a.c0, a.c2));
    const Fq2 d = fq2_inv(add(mul(a.c0, t0), mul_by_xi(add(mul(a.c2, t1), mul(a.c1, t2)))));
    Fq6 r;
    r.c0 = mul(t0, d);
    r.c1 = mul(t1, d);
    r.c2 = mul(t2, d);
    return r;
}

// ---- Fq12 ----
struct Fq12 {
    Fq6 c0, c1;
    static JOLT_HD Fq12 one() {
        Fq12 r;
        r.c0 = Fq6::one();
        r.c1 = Fq6::zero();
        return r;
    }
    JOLT_HD bool is_zero() const { return c0.is_zero() && c1.is_zero(); }
    JOLT_HD bool operator==(const Fq12& o) const { return c0 == o.c0 && c1 == o.c1; }
};
static_assert(sizeof(Fq12) == 384, "Fq12 layout");

JOLT_HD bool fq12_is_canonical(const Fq12& a) {
    return fq2_is_canonical(a.c0.c0) && fq2_is_canonical(a.c0.c1) && fq2_is_canonical(a.c0.c2) && fq2_is_canonical(a.c1.c0) && fq2_is_canonical(a.c1.c1) &&
           fq2_is_canonical(a.c1.c2);
}
// Karatsuba over Fq6: 18 multiplications in Fq2
JOLT_HD Fq12 mul(const Fq12& a, const Fq12& b) {
    const Fq6 v0 = mul(a.c0, b.c0), v1 = mul(a.c1, b.c1);
    Fq12 r;
    r.c1 = sub(sub(mul(add(a.c0, a.c1), add(b.c0, b.c1)), v0), v1);
    r.c0 = add(v0, mul_by_v(v1));
    return r;
}
// complex squaring: (a0 + a1)(a0 + v a1) - a0 a1 - v a0 a1, 2 a0 a1 -- 12 multiplications in Fq2
JOLT_HD Fq12 sqr(const Fq12& a) {
    const Fq6 ab = mul(a.c0, a.c1);
    Fq12 r;
    r.c0 = sub(sub(mul(add(a.c0, a.c1), add(a.c0, mul_by_v(a.c1))), ab), mul_by_v(ab));
    r.c1 = dbl(ab);
    return r;
}
// The sparse element of a Miller line: s0 + s3 w + s4 w^3, i.e. c0.c0 = s0, c1.c0 = s3, c1.c1 = s4 (arkworks' mul_by_034).  13 multiplications in Fq2.
JOLT_HD Fq12 mul_by_034(const Fq12& a, const Fq2& s0, const Fq2& s3, const Fq2& s4) {
    const Fq6 v0 = mul_fq2(a.c0, s0);
    const Fq6 v1 = mul_by_01(a.c1, s3, s4);
    Fq12 r;
    r.c1 = sub(sub(mul_by_01(add(a.c0, a.c1), add(s0, s3), s4), v0), v1);
    r.c0 = add(v0, mul_by_v(v1));
    return r;
}
// the p^6-th power
JOLT_HD Fq12 conj(const Fq12& a) {
    Fq12 r;
    r.c0 = a.c0;
    r.c1 = neg(a.c1);
    return r;
}
// zero maps to zero
JOLT_HD Fq12 fq12_inv(const Fq12& a) {
    const Fq6 d = fq6_inv(sub(sqr(a.c0), mul_by_v(sqr(a.c1))));
    Fq12 r;
    r.c0 = mul(a.c0, d);
    r.c1 = neg(mul(a.c1, d));
    return r;
}

// a^(p^E), E = 1, 2, 3: the coefficient g_k of w^k becomes g_k^(p^E) gamma_{E,k}, and g^(p^E) is the conjugate for odd E.  Host only (the final exponentiation).
inline Fq2 fq2_from_limbs(const uint32_t (&t)[2][8]) {
    Fq2 r;
    JOLT_FQ2_CONST(r, t);
    return r;
}
template <bool Conj>
inline Fq12 frobenius_with(const Fq12& a, const uint32_t (&gamma)[6][2][8]) {
    auto term = [&gamma](const Fq2& g, int k) { return mul(Conj ? conj(g) : g, fq2_from_limbs(gamma[k])); };
    Fq12 r;
    r.c0.c0 = Conj ? conj(a.c0.c0) : a.c0.c0;
    r.c1.c0 = term(a.c1.c0, 1);
    r.c0.c1 = term(a.c0.c1, 2);
    r.c1.c1 = term(a.c1.c1, 3);
    r.c0.c2 = term(a.c0.c2, 4);
    r.c1.c2 = term(a.c1.c2, 5);
    return r;
}
inline Fq12 frobenius1(const Fq12& a) { return frobenius_with<true>(a, PairingConsts::FROB1); }
inline Fq12 frobenius2(const Fq12& a) { return frobenius_with<false>(a, PairingConsts::FROB2); }
inline Fq12 frobenius3(const Fq12& a) { return frobenius_with<true>(a, PairingConsts::FROB3); }

}  // namespace jolt
