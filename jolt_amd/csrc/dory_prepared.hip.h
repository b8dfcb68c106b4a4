// jolt_amd/csrc/dory_prepared.hip.h -- the prepared G2 line table behind jolt_g2_prepared, the kernel that fills one and the Miller kernel that reads one, with their
// launch sites (launch_prepare, enqueue_miller): shared by the entry points over host points (dory_pairing.hip) and over resident vectors (dory_resident.hip).
#pragma once
#include "ctx.hpp"
#include "dory_host.hpp"
#include "pairing.hip.h"

struct jolt_g2_prepared {
    jolt_ctx* ctx = nullptr;
    size_t n = 0;
    jolt::PairLine* lines = nullptr;  // device, [kPairingLines][n]
    uint8_t* skip = nullptr;    // device, [n]: the point is the identity
};

namespace jolt {
namespace dory_dev {

using dory_host::kLanes;

static __global__ __launch_bounds__(kLanes) void k_pair_prepare_g2(const G2Jac* __restrict__ pts, PairLine* __restrict__ lines, uint8_t* __restrict__ skip, size_t n) {
    const size_t i = (size_t)blockIdx.x * kLanes + threadIdx.x;
    if (i >= n) return;
    const PairLineTable table = {lines + i, n};
    skip[i] = g2_prepare_walk(pts[i], table) ? 1 : 0;
}
inline hipError_t launch_prepare(hipStream_t st, const G2Jac* d_g2, PairLine* d_lines, uint8_t* d_skip, size_t n) {
    hipLaunchKernelGGL(k_pair_prepare_g2, dim3(dory_host::lanes_grid(n)), dim3(kLanes), 0, st, d_g2, d_lines, d_skip, n);
    return hipGetLastError();
}

// one lane per PAIR against a table of `stride` >= n points, of which the first n are used: its own f, 65 squarings and 88 sparse multiplications
static __global__ __launch_bounds__(kLanes) void k_pair_miller(const G1Jac* __restrict__ g1s, const PairLine* lines, const uint8_t* __restrict__ skip, size_t stride, Fq12* __restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * kLanes + threadIdx.x;
    if (i >= n) return;
    const PairLineTable table = {const_cast<PairLine*>(lines) + i, stride};
    out[i] = miller_walk(g1s[i], table, skip[i] != 0);
}
inline hipError_t enqueue_miller(hipStream_t st, const G1Jac* d_g1, const PairLine* d_lines, const uint8_t* d_skip, size_t stride, Fq12* d_f, size_t n) {
    hipLaunchKernelGGL(k_pair_miller, dim3(dory_host::lanes_grid(n)), dim3(kLanes), 0, st, d_g1, d_lines, d_skip, stride, d_f, n);
    return hipGetLastError();
}
// the product of the Miller values: the Op of k_tree_level / k_batch_tree_level (AddPt<O> of dory_kernels.hip.h is the one of the sums)
struct MulFq12 {
    static JOLT_HD Fq12 combine(const Fq12& a, const Fq12& b) { return mul(a, b); }
};

}  // namespace dory_dev
}  // namespace jolt
