// jolt_amd/csrc/dory_hints.hip.h -- row commitments leave the MSM workspace as opening hints: transposed into hint order, normalised, in one pass (docs/kernels.md 3.5j).
//
// The tier-1 commitments of dory.hip end as Jacobian points in the MSM workspace: the bucket sums of the one-hot chunks, the folded rows of the dense columns.  An opening
// wants them as resident G1 vectors in the order finish_one_hot_column_major_chunks (crates/jolt-dory/src/streaming.rs:318-362) gives a hint.  k_dory_hints_normalise reads
// element e of a batch through an index map, divides Z out and writes the point where the map says: (x / z^2, y / z^3, 1), the identity as (1, 1, 0).
// The inversions are batched by Montgomery's trick: a lane owns a run of points, keeps the running products of their Z in a pool of one Fq per point (global memory, not a
// per-lane array), inverts the last product once (Fermat) and walks back.  A point with z = 0 enters the product as one.
// Workgroups of one wavefront; a lane's points are interleaved with its neighbours' (point j of lane l is block base + l + 64 j), so that the 64 lanes of a step touch 64
// consecutive points.  Integer VALU work, no MFMA, no scratch.
#pragma once
#include "g1.hip.h"

namespace jolt {
namespace dory_hints {

constexpr int kLanes = 64;
constexpr uint32_t kRun = 16;  // points per lane: the 380 multiplications of the inversion spread over 16 points, against 7 per point for the trick and the division

// The dense columns: row r of the fold kernels' output is hint element r.
struct RowsMap {
    JOLT_HD void at(size_t e, size_t& src, size_t& dst) const { src = dst = e; }
};
// The one-hot columns.  A batch holds the windows [window0, window0 + V) of the key stream of a range of columns, window = column * chunks + chunk, with K + 1 buckets each
// (bucket 0 = cold cycles).  Element e = (window - window0) * K + row reads bucket (window - window0) * (K + 1) + row + 1 and is hint element
// column * K * chunks + row * chunks + chunk of the destination view: the transposition of streaming.rs:318-362.
struct OneHotMap {
    uint32_t K;
    size_t chunks, window0;
    JOLT_HD void at(size_t e, size_t& src, size_t& dst) const {
        const size_t local = e / K, row = e % K, window = window0 + local;
        const size_t column = window / chunks, chunk = window % chunks;
        src = local * ((size_t)K + 1) + row + 1;
        dst = (column * K + row) * chunks + chunk;
    }
};

// One lane's run.  a.z(j): Z of the run's point j; a.point(j): the point; a.put(j, v) / a.get(j): the pool cell of point j; a.store(j, p): the normalised point.
template <class Access>
JOLT_HD void normalise_run(uint32_t count, Access&& a) {
    if (count == 0) return;
    Fq acc = Fq::one();
    for (uint32_t j = 0; j < count; ++j) {
        const Fq z = a.z(j);
        if (!z.is_zero()) acc = mul(acc, z);
        a.put(j, acc);
    }
    Fq inv_rest = inv(acc);  // 1 / (z_0 ... z_j) on the way down
    for (uint32_t j = count; j-- > 0;) {
        const G1Jac p = a.point(j);
        if (g1_is_identity(p)) {
            a.store(j, g1_identity());
            continue;
        }
        const Fq zi = j ? mul(inv_rest, a.get(j - 1)) : inv_rest;
        inv_rest = mul(inv_rest, p.z);
        const Fq zi2 = sqr(zi);
        G1Jac r;
        r.x = mul(p.x, zi2);
        r.y = mul(p.y, mul(zi2, zi));
        r.z = Fq::one();
        a.store(j, r);
    }
}

template <class Map>
struct LaneAccess {
    const G1Jac* __restrict__ src;
    G1Jac* __restrict__ dst;
    Fq* __restrict__ pool;
    Map map;
    size_t first;  // the lane's point j is element first + 64 j
    __device__ __forceinline__ size_t elem(uint32_t j) const { return first + (size_t)j * kLanes; }
    __device__ __forceinline__ Fq z(uint32_t j) const {
        size_t s, d;
        map.at(elem(j), s, d);
        return src[s].z;
    }
    __device__ __forceinline__ G1Jac point(uint32_t j) const {
        size_t s, d;
        map.at(elem(j), s, d);
        return src[s];
    }
    __device__ __forceinline__ void put(uint32_t j, const Fq& v) const { pool[elem(j)] = v; }
    __device__ __forceinline__ Fq get(uint32_t j) const { return pool[elem(j)]; }
    __device__ __forceinline__ void store(uint32_t j, const G1Jac& p) const {
        size_t s, d;
        map.at(elem(j), s, d);
        dst[d] = p;
    }
};

// n elements; workgroup b owns the elements [b * 64 * run, (b + 1) * 64 * run); pool: n cells
template <class Map>
__global__ __launch_bounds__(kLanes) void k_dory_hints_normalise(const G1Jac* __restrict__ src, Map map, size_t n, uint32_t run, Fq* __restrict__ pool, G1Jac* __restrict__ dst) {
    const size_t first = (size_t)blockIdx.x * kLanes * run + threadIdx.x;
    if (first >= n) return;
    const size_t left = (n - first + kLanes - 1) / kLanes;
    normalise_run(left < run ? (uint32_t)left : run, LaneAccess<Map>{src, dst, pool, map, first});
}

__global__ __launch_bounds__(kLanes) void k_dory_hints_identity(G1Jac* __restrict__ dst, size_t n) {
    const size_t i = (size_t)blockIdx.x * kLanes + threadIdx.x;
    if (i < n) dst[i] = g1_identity();
}

template <class Map>
inline hipError_t launch_normalise(hipStream_t st, const G1Jac* src, const Map& map, size_t n, Fq* pool, G1Jac* dst) {
    if (n == 0) return hipSuccess;
    const size_t per = (size_t)kLanes * kRun;
    hipLaunchKernelGGL(k_dory_hints_normalise<Map>, dim3((unsigned)((n + per - 1) / per)), dim3(kLanes), 0, st, src, map, n, kRun, pool, dst);
    return hipGetLastError();
}
}  // namespace dory_hints
}  // namespace jolt
