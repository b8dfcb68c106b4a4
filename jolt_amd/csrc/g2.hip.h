// jolt_amd/csrc/g2.hip.h -- BN254 G2 group law for device and host: the twist y^2 = x^3 + 3 / (9 + u) over Fq2 (a = 0).
//
// Jacobian (X, Y, Z), identity <=> Z == 0; layout = ark_bn254::G2Projective, six Montgomery Fq in the order x.c0, x.c1, y.c0, y.c1,
// z.c0, z.c1 (dory's ArkG2 wraps it transparently).  The formulas are those of g1.hip.h (dbl-2009-l, add-2007-bl) written once over
// the coordinate field, with the same explicit special cases (identity, P + P, P - P); g1.hip.h itself is not touched, the bucket-sum
// kernels are built from it.  The curve equation is checked as (Y^2 - X^3)(9 + u) = 3 Z^6, so no twist constant is stored.
// On the curve is NOT in the group here: the twist has cofactor 2q - r and nothing in this file checks the subgroup.
#pragma once
#include "fq2.hip.h"

namespace jolt {

template <class F>
struct EcJac {
    F x, y, z;
};
using G2Jac = EcJac<Fq2>;
static_assert(sizeof(G2Jac) == 192, "G2 layout");

template <class F>
JOLT_HD bool ec_is_identity(const EcJac<F>& p) { return p.z.is_zero(); }
template <class F>
JOLT_HD EcJac<F> ec_identity() {
    EcJac<F> r;
    r.x = F::one();
    r.y = F::one();
    r.z = F::zero();
    return r;
}
template <class F>
JOLT_HD EcJac<F> ec_neg(const EcJac<F>& p) {
    EcJac<F> r = p;
    r.y = neg(p.y);
    return r;
}

// dbl-2009-l (a = 0)
template <class F>
JOLT_HD EcJac<F> ec_double(const EcJac<F>& p) {
    if (ec_is_identity(p)) return p;
    const F A = sqr(p.x), B = sqr(p.y), C = sqr(B);
    const F D = dbl(sub(sub(sqr(add(p.x, B)), A), C));
    const F E = add(dbl(A), A);
    const F Fv = sqr(E);
    EcJac<F> r;
    r.x = sub(Fv, dbl(D));
    r.z = dbl(mul(p.y, p.z));
    r.y = sub(mul(E, sub(D, r.x)), dbl(dbl(dbl(C))));
    return r;
}

// add-2007-bl: Jacobian + Jacobian
template <class F>
JOLT_HD EcJac<F> ec_add(const EcJac<F>& p, const EcJac<F>& q) {
    if (ec_is_identity(p)) return q;
    if (ec_is_identity(q)) return p;
    const F Z1Z1 = sqr(p.z), Z2Z2 = sqr(q.z);
    const F U1 = mul(p.x, Z2Z2), U2 = mul(q.x, Z1Z1);
    const F S1 = mul(mul(p.y, q.z), Z2Z2), S2 = mul(mul(q.y, p.z), Z1Z1);
    if (U1 == U2) {
        if (S1 == S2) return ec_double(p);
        return ec_identity<F>();
    }
    const F H = sub(U2, U1);
    const F I = sqr(dbl(H));
    const F J = mul(H, I);
    const F rr = dbl(sub(S2, S1));
    const F V = mul(U1, I);
    EcJac<F> r;
    r.x = sub(sub(sqr(rr), J), dbl(V));
    r.y = sub(mul(rr, sub(V, r.x)), dbl(mul(S1, J)));
    r.z = mul(sub(sub(sqr(add(p.z, q.z)), Z1Z1), Z2Z2), H);
    return r;
}

// equality as group elements
template <class F>
JOLT_HD bool ec_eq(const EcJac<F>& p, const EcJac<F>& q) {
    const bool pi = ec_is_identity(p), qi = ec_is_identity(q);
    if (pi || qi) return pi && qi;
    const F Z1Z1 = sqr(p.z), Z2Z2 = sqr(q.z);
    if (mul(p.x, Z2Z2) != mul(q.x, Z1Z1)) return false;
    return mul(p.y, mul(Z2Z2, q.z)) == mul(q.y, mul(Z1Z1, p.z));
}

JOLT_HD bool g2_is_identity(const G2Jac& p) { return ec_is_identity(p); }
JOLT_HD G2Jac g2_identity() { return ec_identity<Fq2>(); }
JOLT_HD G2Jac g2_neg(const G2Jac& p) { return ec_neg(p); }
JOLT_HD G2Jac g2_double(const G2Jac& p) { return ec_double(p); }
JOLT_HD G2Jac g2_add(const G2Jac& p, const G2Jac& q) { return ec_add(p, q); }
JOLT_HD bool g2_eq(const G2Jac& p, const G2Jac& q) { return ec_eq(p, q); }

// canonical coordinates and (Y^2 - X^3)(9 + u) = 3 Z^6, or the identity Z = 0: the twist equation only, no subgroup check
JOLT_HD bool g2_is_on_curve(const G2Jac& p) {
    if (!fq2_is_canonical(p.x) || !fq2_is_canonical(p.y) || !fq2_is_canonical(p.z)) return false;
    if (g2_is_identity(p)) return true;
    const Fq2 z2 = sqr(p.z), z6 = mul(sqr(z2), z2);
    const Fq2 lhs = mul_by_xi(sub(sqr(p.y), mul(sqr(p.x), p.x)));
    return lhs == add(dbl(z6), z6);
}

// scalar * p, scalar a canonical 256-bit integer (8 x u32), MSB-first double-and-add: the plain reference of the host suite
JOLT_HD G2Jac g2_mul_canonical(const G2Jac& p, const uint32_t k[8]) {
    G2Jac acc = g2_identity();
    for (int i = 255; i >= 0; --i) {
        acc = g2_double(acc);
        if ((k[i / 32] >> (i % 32)) & 1) acc = g2_add(acc, p);
    }
    return acc;
}

}  // namespace jolt
