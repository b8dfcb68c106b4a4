// jolt_amd/csrc/fq2.hip.h -- Fq2 = Fq[u] / (u^2 + 1) over the Montgomery Fq of field.hip.h, for device and host.
//
// Layout = ark_bn254::Fq2 (QuadExtField: c0, c1), the coordinate field of G2 (g2.hip.h).  Every operation is built from the Fq
// operations of field.hip.h and keeps both components canonical.  No constant is stored here: the non-residue is -1 and the twist's
// xi = 9 + u is applied with doublings (mul_by_xi).
#pragma once
#include "field.hip.h"

namespace jolt {

struct Fq2 {
    Fq c0, c1;

    static JOLT_HD Fq2 zero() {
        Fq2 r;
        r.c0 = Fq::zero();
        r.c1 = Fq::zero();
        return r;
    }
    static JOLT_HD Fq2 one() {
        Fq2 r;
        r.c0 = Fq::one();
        r.c1 = Fq::zero();
        return r;
    }
    JOLT_HD bool is_zero() const { return c0.is_zero() && c1.is_zero(); }
    JOLT_HD bool operator==(const Fq2& o) const { return c0 == o.c0 && c1 == o.c1; }
    JOLT_HD bool operator!=(const Fq2& o) const { return !(*this == o); }
};
static_assert(sizeof(Fq2) == 64, "Fq2 layout");

// both components below q
JOLT_HD bool fq2_is_canonical(const Fq2& a) {
    Fq d;
    return sub_p(d, a.c0) != 0 && sub_p(d, a.c1) != 0;
}

JOLT_HD Fq2 add(const Fq2& a, const Fq2& b) {
    Fq2 r;
    r.c0 = add(a.c0, b.c0);
    r.c1 = add(a.c1, b.c1);
    return r;
}
JOLT_HD Fq2 sub(const Fq2& a, const Fq2& b) {
    Fq2 r;
    r.c0 = sub(a.c0, b.c0);
    r.c1 = sub(a.c1, b.c1);
    return r;
}
JOLT_HD Fq2 neg(const Fq2& a) {
    Fq2 r;
    r.c0 = neg(a.c0);
    r.c1 = neg(a.c1);
    return r;
}
JOLT_HD Fq2 dbl(const Fq2& a) {
    Fq2 r;
    r.c0 = dbl(a.c0);
    r.c1 = dbl(a.c1);
    return r;
}
// Karatsuba, three base multiplications: (a0 b0 - a1 b1) + ((a0 + a1)(b0 + b1) - a0 b0 - a1 b1) u
JOLT_HD Fq2 mul(const Fq2& a, const Fq2& b) {
    const Fq v0 = mul(a.c0, b.c0), v1 = mul(a.c1, b.c1);
    const Fq m = mul(add(a.c0, a.c1), add(b.c0, b.c1));
    Fq2 r;
    r.c0 = sub(v0, v1);
    r.c1 = sub(sub(m, v0), v1);
    return r;
}
// complex squaring, two base multiplications: (a0 + a1)(a0 - a1) + 2 a0 a1 u
JOLT_HD Fq2 sqr(const Fq2& a) {
    const Fq p = mul(a.c0, a.c1);
    Fq2 r;
    r.c0 = mul(add(a.c0, a.c1), sub(a.c0, a.c1));
    r.c1 = dbl(p);
    return r;
}
// a * (9 + u) = (9 a0 - a1) + (9 a1 + a0) u
JOLT_HD Fq2 mul_by_xi(const Fq2& a) {
    const Fq n0 = add(dbl(dbl(dbl(a.c0))), a.c0), n1 = add(dbl(dbl(dbl(a.c1))), a.c1);
    Fq2 r;
    r.c0 = sub(n0, a.c1);
    r.c1 = add(n1, a.c0);
    return r;
}

}  // namespace jolt
