// jolt_amd/csrc/dory_prepared.hip.h -- the prepared G2 line table behind jolt_g2_prepared and the kernel that fills one, shared by the entry points that build a
// table from host points (dory_pairing.hip) and from a resident vector (dory_resident.hip).
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

}  // namespace dory_dev
}  // namespace jolt
