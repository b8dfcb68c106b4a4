// jolt_amd/csrc/grid_pairs.hip.h -- the entries of the commitment grid's pair tables (grid_pairs.hip builds them, pcs.hip reads them).
//
// On the K x T grid a one-hot column contributes one of K bases per cycle, G[hot * D + j'] on the domain of length D = T >> shift, so two
// consecutive cycles contribute one of K^2 sums.  PT_D[m][a][b] = G[a * D + 2m] + G[b * D + 2m + 1] depends on the SRS, K and D alone: with it
// resident a sum of bases costs one mixed addition per PAIR of hot cycles.  Entries are affine points in L-form (fq_limb.hip.h) like window 0
// of the fixed-base tables, (0, 0) = infinity.  Every function also compiles for the host (jolt_host_grid_pair_*), where the CPU suite pins it.
#pragma once
#include "g1.hip.h"

namespace jolt {

// entry (m, a, b) of the table of a K-row grid: a lane's K^2 candidates for pair m are one contiguous block (16 KiB at K = 16)
JOLT_HD size_t grid_pair_index(size_t m, uint32_t k, uint32_t a, uint32_t b) { return (m * k + a) * k + b; }

// What the affine sum p + q divides by: x_q - x_p, or 2 y for a doubling; one where the sum needs no division (an operand at infinity, q = -p, and a y of
// zero, which no point of the curve has) -- never zero, so that a lane's entries can share one inversion of their product.
JOLT_HD Fq grid_pair_denominator(const G1Affine& p, const G1Affine& q) {
    if (g1_aff_is_inf(p) || g1_aff_is_inf(q)) return Fq::one();
    if (p.x == q.x) return (p.y == q.y && !p.y.is_zero()) ? dbl(p.y) : Fq::one();
    return sub(q.x, p.x);
}
// p + q as the table stores it, given inv_d = 1 / grid_pair_denominator(p, q); operands in standard Montgomery form, mont32 = the Montgomery form of 32
// (the factor between a standard coordinate and its L-form).  inf + q = q, p + inf = p, p + p by the tangent, p + (-p) = inf + inf = (0, 0).
JOLT_HD G1Affine grid_pair_entry(const G1Affine& p, const G1Affine& q, const Fq& inv_d, const Fq& mont32) {
    G1Affine r;
    if (g1_aff_is_inf(p)) {
        r = q;
    } else if (g1_aff_is_inf(q)) {
        r = p;
    } else {
        Fq lambda;
        if (p.x == q.x) {
            if (p.y != q.y || p.y.is_zero()) {
                r.x = Fq::zero();
                r.y = Fq::zero();
                return r;
            }
            const Fq xx = sqr(p.x);
            lambda = mul(add(dbl(xx), xx), inv_d);
        } else {
            lambda = mul(sub(q.y, p.y), inv_d);
        }
        r.x = sub(sub(sqr(lambda), p.x), q.x);
        r.y = sub(mul(lambda, sub(p.x, r.x)), p.y);
    }
    r.x = mul(r.x, mont32);  // (0, 0) stays (0, 0)
    r.y = mul(r.y, mont32);
    return r;
}

}  // namespace jolt
