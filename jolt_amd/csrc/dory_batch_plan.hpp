// jolt_amd/csrc/dory_batch_plan.hpp -- the launch plan of one chain of a Dory product batch (dory_resident.hip): plain host code, no HIP.
//
// A chain is a list of items (inner products) of ragged lengths that run as ONE launch set.  Every item is padded to whole wavefronts, so a workgroup (one
// wavefront) belongs to exactly one item and no lane branches on the item: the kernels read (item, first) for their workgroup from a small table and the item's
// pointers and length from a second one.  The reduction is a halving tree per item, one launch per level over all items: `levels` is that of the longest item,
// shorter ones have finished by then and their workgroups leave at once.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace jolt {
namespace dory_plan {

constexpr size_t kPlanLanes = 64;
constexpr size_t kMaxPacked = (size_t)1 << 24;  // slots of one chain: keeps workgroup counts and `first` far inside 32 bits

struct BatchPlan {
    std::vector<uint32_t> wg_item;   // per workgroup: its item ...
    std::vector<uint32_t> wg_first;  // ... and the item-relative index of its lane 0 (a multiple of kPlanLanes)
    std::vector<size_t> item_base;   // per item: its first slot in the packed array
    size_t packed = 0;               // slots in all
    uint32_t levels = 0;             // ceil(log2(longest item)), 0 when no item is longer than 1
};

// halvings m -> ceil(m / 2) until one element is left
inline uint32_t tree_levels(size_t m) {
    uint32_t l = 0;
    for (; m > 1; m = (m + 1) / 2) ++l;
    return l;
}

// false: the padded total would pass kMaxPacked (nothing is kept then)
inline bool batch_plan(const size_t* lens, size_t n_items, BatchPlan* out) {
    BatchPlan p;
    p.item_base.reserve(n_items);
    for (size_t k = 0; k < n_items; ++k) {
        if (lens[k] > kMaxPacked || p.packed > kMaxPacked - lens[k]) return false;  // before any rounding up: nothing here can wrap
        const size_t wgs = (lens[k] + kPlanLanes - 1) / kPlanLanes;
        p.item_base.push_back(p.packed);
        for (size_t w = 0; w < wgs; ++w) {
            p.wg_item.push_back((uint32_t)k);
            p.wg_first.push_back((uint32_t)(w * kPlanLanes));
        }
        p.packed += wgs * kPlanLanes;
        const uint32_t l = tree_levels(lens[k]);
        if (l > p.levels) p.levels = l;
    }
    if (p.packed > kMaxPacked) return false;
    *out = std::move(p);
    return true;
}

}  // namespace dory_plan
}  // namespace jolt
