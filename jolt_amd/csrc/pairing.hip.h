// jolt_amd/csrc/pairing.hip.h -- the BN254 optimal ate pairing over fq12.hip.h: line tables of G2 points, the Miller loop, the final exponentiation.
//
// Replaces ark_bn254's pairing behind PairingGroup::multi_pairing (crates/jolt-crypto/src/ec/bn254/mod.rs:274-284) and dory's multi_pair /
// multi_pair_g2_setup (crates/jolt-dory/src/scheme.rs:543-552).  One definition for the kernels of dory_pairing.hip and the host functions of the CPU suite.
//
// e(P, Q) = (f_{6z+2,Q}(P) l_{[6z+2]Q, pi(Q)}(P) l_{[6z+2]Q + pi(Q), -pi^2(Q)}(P))^((p^12 - 1) / r * h),  z = 4965661367192848881.
//
// Prepared G2 (g2_prepare_walk).  Q is brought to affine coordinates on the twist once (one Fermat inversion), then T = Q walks 6z + 2 in non-adjacent form
// (PAIRING_NAF_LEN digits; 65 doublings, 21 additions) in homogeneous projective coordinates, without inversions, followed by the additions of pi(Q) and
// -pi^2(Q): PAIRING_LINES = 88 lines.  A line is three Fq2 coefficients (a, b, c) of  a y_P + b x_P w + c w^3  -- the untwisted Q is (x w^2, y w^3), w^6 = xi,
// so the chord or tangent of slope lambda through T evaluates at P to  y_P - lambda x_P w + (lambda x_T - y_T) w^3;  every line here is that times an
// element of Fq2 (the cleared denominators), which the final exponentiation sends to one.  The representative of Q does not matter: lines are a function
// of the affine point.  A point outside the order-r subgroup meets no trap (nothing is inverted in the walk, and an addition of equal points only gives
// a meaningless line); its result is unspecified.  The identity gives a meaningless table and the flag "skip this pair".
//
// Miller accumulation (miller_walk).  f = 1; per doubling f = f^2 (complex squaring, 12 Fq2 multiplications), per line one sparse multiplication
// (mul_by_034, 13 Fq2 multiplications, after a and b were scaled by y_P and x_P: 4 Fq multiplications).
//
// Final exponentiation (host only).  Easy part f^((p^6 - 1)(p^2 + 1)) by conjugation, one inversion and the p^2 Frobenius.  Hard part: plain square-and-multiply
// by 2 z (6 z^2 + 3 z + 1) (p^4 - p^2 + 1) / r, the power ark-ec's BN model is recalled to compute -- a convention NOT pinned by a reference vector
// (docs/parity.md): any multiple of (p^4 - p^2 + 1) / r coprime to r is a pairing, but GT bytes in commitments and proofs only agree under the same multiple.
#pragma once
#include "fq12.hip.h"
#include "g1.hip.h"
#include "g2.hip.h"

namespace jolt {

constexpr int kPairingLines = PAIRING_LINES;

struct PairLine {
    Fq2 a, b, c;  // a y_P + b x_P w + c w^3
};
static_assert(sizeof(PairLine) == 192, "line layout");

// element `step` of a line table whose steps lie `stride` lines apart: stride = number of points for the step-major device table, 1 for a single point's table
struct PairLineTable {
    PairLine* base;
    size_t stride;
    JOLT_HD void put(int step, const PairLine& l) const { base[(size_t)step * stride] = l; }
    JOLT_HD PairLine get(int step) const { return base[(size_t)step * stride]; }
};

// digit i of 6z + 2 in non-adjacent form, i < PAIRING_NAF_LEN
JOLT_HD int pairing_naf_digit(int i) {
    const uint64_t nz = i < 64 ? PAIRING_NAF_NZ_LO >> i : PAIRING_NAF_NZ_HI >> (i - 64);
    const uint64_t ng = i < 64 ? PAIRING_NAF_NEG_LO >> i : PAIRING_NAF_NEG_HI >> (i - 64);
    return (nz & 1) ? ((ng & 1) ? -1 : 1) : 0;
}

// line `step` of a table is a tangent: the Miller accumulator is squared before it
JOLT_HD bool pairing_line_is_tangent(int step) { return ((step < 64 ? PAIRING_TANGENT_LO >> step : PAIRING_TANGENT_HI >> (step - 64)) & 1) != 0; }

struct G2Homog {
    Fq2 x, y, z;  // (x / z, y / z) on the twist
};

// T = 2 T and the tangent at T: (2 Y Z, -3 X^2, Y^2 - 3 b' Z^2)
JOLT_HD PairLine pair_double_step(G2Homog& t) {
    Fq2 b3;
    JOLT_FQ2_CONST(b3, PairingConsts::TWIST_3B);
    const Fq2 A = mul(t.x, t.y), B = sqr(t.y), C = sqr(t.z);
    const Fq2 E = mul(b3, C);                  // 3 b' Z^2
    const Fq2 F = add(dbl(E), E);              // 9 b' Z^2
    const Fq2 H = sub(sqr(add(t.y, t.z)), add(B, C));  // 2 Y Z
    const Fq2 J = sqr(t.x);
    const Fq2 E2 = sqr(dbl(E));                // 4 E^2
    PairLine l;
    l.a = H;
    l.b = neg(add(dbl(J), J));
    l.c = sub(B, E);
    // four times the textbook point (X Y (B - F) / 2, ((B + F) / 2)^2 - 3 E^2, B H): no halving
    t.x = dbl(mul(A, sub(B, F)));
    t.y = sub(sqr(add(B, F)), add(dbl(E2), E2));
    t.z = dbl(dbl(mul(B, H)));
    return l;
}
// T = T + Q (Q affine) and the chord through them: (lambda, -theta, theta x_Q - lambda y_Q) with theta = Y - y_Q Z, lambda = X - x_Q Z
JOLT_HD PairLine pair_add_step(G2Homog& t, const Fq2& qx, const Fq2& qy) {
    const Fq2 theta = sub(t.y, mul(qy, t.z)), lambda = sub(t.x, mul(qx, t.z));
    const Fq2 C = sqr(theta), D = sqr(lambda);
    const Fq2 E = mul(lambda, D), F = mul(t.z, C), G = mul(t.x, D);
    const Fq2 H = sub(add(E, F), dbl(G));
    PairLine l;
    l.a = lambda;
    l.b = neg(theta);
    l.c = sub(mul(theta, qx), mul(lambda, qy));
    t.x = mul(lambda, H);
    t.y = sub(mul(theta, sub(G, H)), mul(E, t.y));
    t.z = mul(t.z, E);
    return l;
}

// The kPairingLines lines of q into `out`; returns true when q is the identity ("skip this pair": the table then holds nothing of use)
JOLT_HD bool g2_prepare_walk(const G2Jac& q, const PairLineTable& out) {
    const Fq2 zi = fq2_inv(q.z), zi2 = sqr(zi);
    const Fq2 qx = mul(q.x, zi2), qy = mul(q.y, mul(zi2, zi)), nqy = neg(qy);
    G2Homog t;
    t.x = qx;
    t.y = qy;
    t.z = Fq2::one();
    int step = 0;
#pragma unroll 1
    for (int i = PAIRING_NAF_LEN - 2; i >= 0; --i) {
        out.put(step++, pair_double_step(t));
        const int d = pairing_naf_digit(i);
        if (d != 0) out.put(step++, pair_add_step(t, qx, d < 0 ? nqy : qy));
    }
    Fq2 g;
    JOLT_FQ2_CONST(g, PairingConsts::FROB1[2]);
    const Fq2 q1x = mul(conj(qx), g);
    JOLT_FQ2_CONST(g, PairingConsts::FROB1[3]);
    const Fq2 q1y = mul(conj(qy), g);
    out.put(step++, pair_add_step(t, q1x, q1y));
    JOLT_FQ2_CONST(g, PairingConsts::FROB2[2]);
    const Fq2 q2x = mul(qx, g);
    JOLT_FQ2_CONST(g, PairingConsts::FROB2[3]);
    const Fq2 q2y = neg(mul(qy, g));
    out.put(step++, pair_add_step(t, q2x, q2y));
    return g2_is_identity(q);
}

// squaring and line multiplication as separately scoped steps: each ends with f as its only live Fq12
JOLT_HD void miller_square(Fq12& f) { f = sqr(f); }
JOLT_HD void miller_line(Fq12& f, const PairLine& l, const Fq& xp, const Fq& yp) { f = mul_by_034(f, mul_fq(l.a, yp), mul_fq(l.b, xp), l.c); }

// The Miller value of one pair over a prepared table; p in any Jacobian representative.  One for the identity on either side.
JOLT_HD Fq12 miller_walk(const G1Jac& p, const PairLineTable& lines, bool skip) {
    const Fq zi = fq_inv_fermat(p.z), zi2 = sqr(zi);
    const Fq xp = mul(p.x, zi2), yp = mul(p.y, mul(zi2, zi));
    Fq12 f = Fq12::one();
    // one loop over the lines, so that the kernel holds ONE copy of the squaring and one of the line multiplication; the branch is uniform over the wavefront
#pragma unroll 1
    for (int step = 0; step < kPairingLines; ++step) {
        if (pairing_line_is_tangent(step)) miller_square(f);
        miller_line(f, lines.get(step), xp, yp);
    }
    return (skip || g1_is_identity(p)) ? Fq12::one() : f;
}

// ---- host only ----
// a^e, e a little-endian array of 32-bit limbs
inline Fq12 fq12_pow(const Fq12& a, const uint32_t* e, int bits) {
    Fq12 acc = Fq12::one();
    for (int i = bits - 1; i >= 0; --i) {
        acc = sqr(acc);
        if ((e[i / 32] >> (i % 32)) & 1) acc = mul(acc, a);
    }
    return acc;
}
// f^((p^12 - 1) / r * 2 z (6 z^2 + 3 z + 1)); zero maps to zero
inline Fq12 final_exponentiation(const Fq12& f) {
    static constexpr uint32_t kHard[] = PAIRING_HARD_EXP_LIMBS;
    const Fq12 t = mul(conj(f), fq12_inv(f));  // f^(p^6 - 1)
    const Fq12 easy = mul(frobenius2(t), t);   // ^(p^2 + 1)
    return fq12_pow(easy, kHard, PAIRING_HARD_EXP_BITS);
}

}  // namespace jolt
