// jolt_amd/csrc/precommitted_kernels.hip.h -- kernels of the precommitted claim reductions (precommitted.hip): the fused round kernel and the table builders.
//
// The reduction's state (crates/jolt-kernels/src/precommitted_reduction.rs:76-85) is `value`, `eq` and n_aux passenger tables of one length, bound LowToHigh together;
// only value and eq enter the round sums (:96-133)
//     e0 = sum_j value[2j] eq[2j],     e2 = sum_j (2 value[2j+1] - value[2j]) (2 eq[2j+1] - eq[2j]).
// An active round that follows an active round applies the pending challenge to every table AND needs the two sums over the freshly bound value / eq: one launch
// (k_precommitted_bind_sums) instead of a bind launch plus a round-sum launch over the member machinery.  A work item reads FOUR consecutive old entries of a table
// and writes the TWO bound ones, so that the bound pair a round term is made of never leaves registers.  Traffic per old entry: 32 B read, 16 B written -- what
// k_bind_low_to_high moves (poly_kernels.hip.h), the sums ride along.
//
// The tables are addressed through two pointer arrays in device memory (the ping and the pong side of every table, written once when the operator is made): the
// table index is blockIdx.y as in k_bind_low_to_high, and any number of passengers is one launch.
#pragma once
#include "poly_kernels.hip.h"

namespace jolt {

// out[2j], out[2j+1] from in[4j .. 4j+3]: two steps of Polynomial::bind_low_to_high (crates/jolt-poly/src/dense.rs:223-303)
template <bool SHIFTED>
__device__ __forceinline__ void bind_quad(const Fr* __restrict__ in, Fr* __restrict__ out, size_t j, const Fr& r, Fr& lo, Fr& hi) {
    const Fr a = ld_fr(in + 4 * j), b = ld_fr(in + 4 * j + 1), c = ld_fr(in + 4 * j + 2), d = ld_fr(in + 4 * j + 3);
    lo = bind_pair<SHIFTED>(a, b, r);
    hi = bind_pair<SHIFTED>(c, d, r);
    st_fr(out + 2 * j, lo);
    st_fr(out + 2 * j + 1, hi);
}
// one term of each round sum (precommitted_reduction.rs:103-112)
__device__ __forceinline__ void precommitted_term(const Fr& v0, const Fr& v1, const Fr& e0, const Fr& e1, Fr (&acc)[2]) {
    acc[0] = add(acc[0], mul(v0, e0));
    acc[1] = add(acc[1], mul(sub(dbl(v1), v0), sub(dbl(e1), e0)));
}

// Bind + sums.  quads = old length / 4 (old length >= 4).  blockIdx.y = 0: the value / eq pair (tables 0 and 1), partial sums to partials[2 blockIdx.x ..], and
// the last of these workgroups to finish adds the partials up and publishes the two sums to the host (finish_member, poly_kernels.hip.h: the completion path of the
// batch rounds -- no second launch, no copy, no stream synchronisation per round); blockIdx.y = k >= 1: passenger table k + 1, the same path without the products.
template <bool SHIFTED>
static __global__ __launch_bounds__(kBlock) void k_precommitted_bind_sums(const Fr* const* __restrict__ in, Fr* const* __restrict__ out, size_t quads, Fr r,
                                                                          Fr* __restrict__ partials, RoundDone rd) {
    const size_t stride = (size_t)gridDim.x * kBlock, first = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (blockIdx.y == 0) {
        const Fr* __restrict__ vin = in[0];
        const Fr* __restrict__ ein = in[1];
        Fr* __restrict__ vout = out[0];
        Fr* __restrict__ eout = out[1];
        Fr acc[2] = {Fr::zero(), Fr::zero()};
        for (size_t j = first; j < quads; j += stride) {
            Fr v0, v1, e0, e1;
            bind_quad<SHIFTED>(vin, vout, j, r, v0, v1);
            bind_quad<SHIFTED>(ein, eout, j, r, e0, e1);
            precommitted_term(v0, v1, e0, e1, acc);
        }
        block_reduce_store<2>(acc, partials);
        finish_member(partials, 2, 0u, 0u, rd);
    } else {
        const Fr* __restrict__ tin = in[blockIdx.y + 1];
        Fr* __restrict__ tout = out[blockIdx.y + 1];
        for (size_t j = first; j < quads; j += stride) {
            Fr lo, hi;
            bind_quad<SHIFTED>(tin, tout, j, r, lo, hi);
        }
    }
}

// Bind only (finish_rounds, or an inactive round follows): blockIdx.y = table, half = the new length (>= 1); a work item writes out[2j] and, if it exists, out[2j+1].
template <bool SHIFTED>
static __global__ __launch_bounds__(kBlock) void k_precommitted_bind(const Fr* const* __restrict__ in, Fr* const* __restrict__ out, size_t half, Fr r) {
    const Fr* __restrict__ tin = in[blockIdx.y];
    Fr* __restrict__ tout = out[blockIdx.y];
    const size_t stride = (size_t)gridDim.x * kBlock, items = (half + 1) / 2;
    for (size_t j = (size_t)blockIdx.x * kBlock + threadIdx.x; j < items; j += stride) {
        const size_t y = 2 * j;
        st_fr(tout + y, bind_pair<SHIFTED>(ld_fr(tin + 2 * y), ld_fr(tin + 2 * y + 1), r));
        if (y + 1 < half) st_fr(tout + y + 1, bind_pair<SHIFTED>(ld_fr(tin + 2 * y + 2), ld_fr(tin + 2 * y + 3), r));
    }
}

// Sums only (round 0, or the pending challenge belonged to an inactive round): pairs = length / 2 (>= 1), nothing is written but the partial sums.
static __global__ __launch_bounds__(kBlock) void k_precommitted_sums(const Fr* const* __restrict__ in, size_t pairs, Fr* __restrict__ partials, RoundDone rd) {
    const Fr* __restrict__ v = in[0];
    const Fr* __restrict__ e = in[1];
    const size_t stride = (size_t)gridDim.x * kBlock;
    Fr acc[2] = {Fr::zero(), Fr::zero()};
    for (size_t j = (size_t)blockIdx.x * kBlock + threadIdx.x; j < pairs; j += stride)
        precommitted_term(ld_fr(v + 2 * j), ld_fr(v + 2 * j + 1), ld_fr(e + 2 * j), ld_fr(e + 2 * j + 1), acc);
    block_reduce_store<2>(acc, partials);
    finish_member(partials, 2, 0u, 0u, rd);
}

// The fully bound coefficients (final_claim / final_aux_claims, precommitted_reduction.rs:204-218): out[i] = in[i][0].
static __global__ __launch_bounds__(kBlock) void k_precommitted_first_entries(const Fr* const* __restrict__ in, size_t n, Fr* __restrict__ out) {
    for (size_t i = threadIdx.x; i < n; i += kBlock) st_fr(out + i, ld_fr(in[i]));
}

// permute_coefficients (precommitted_reduction.rs:615-636): out[new] = in[old], bit b of `new` moved to position new_to_old[b] of `old`.  A pure gather.
struct BitPermutation {
    uint8_t new_to_old[48];
    uint32_t n;
};
static __global__ __launch_bounds__(kBlock) void k_permute_bits(const Fr* __restrict__ in, Fr* __restrict__ out, size_t len, BitPermutation p) {
    const size_t stride = (size_t)gridDim.x * kBlock;
    for (size_t x = (size_t)blockIdx.x * kBlock + threadIdx.x; x < len; x += stride) {
        size_t old = 0;
        for (uint32_t b = 0; b < p.n; ++b) old |= ((x >> b) & 1) << p.new_to_old[b];
        st_fr(out + x, ld_fr(in + old));
    }
}

// The bytecode reduction's eq template (optimized/precommitted_reduction.rs:419-425): out[index] = lane_weights[lane] * cycle_table[cycle] with
// (lane, cycle) = TracePolynomialOrder::index_to_address_cycle (crates/jolt-claims/src/protocols/jolt/geometry/dimensions.rs:48-58):
// cycle-major (index / cycles, index % cycles), address-major (index % lanes, index / lanes).
static __global__ __launch_bounds__(kBlock) void k_table_outer(const Fr* __restrict__ lane_weights, size_t lanes, const Fr* __restrict__ cycle_table, size_t cycles,
                                                               int address_major, Fr* __restrict__ out) {
    const size_t stride = (size_t)gridDim.x * kBlock, len = lanes * cycles;
    for (size_t x = (size_t)blockIdx.x * kBlock + threadIdx.x; x < len; x += stride) {
        const size_t lane = address_major ? x % lanes : x / cycles, cycle = address_major ? x / lanes : x % cycles;
        st_fr(out + x, mul(ld_fr(lane_weights + lane), ld_fr(cycle_table + cycle)));
    }
}

}  // namespace jolt
