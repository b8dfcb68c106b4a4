// jolt_amd/csrc/dory_batches.hip.h -- the batch pipeline under every tier-1 entry of dory.hip: the bucket method of msm.hip over many bucket sets at once.
//
// An entry is a SOURCE (where the keys of a batch come from and what follows its bucket sums: the integer rows, the field rows, the one-hot columns) and a SINK
// (where a batch's result goes: the caller's host array, or normalised into a resident view); bucket_batches runs the launch set of one batch after the other
// between the two.  Host code only: the kernels are msm_kernels.hip.h's and the caller's.
#pragma once
#include <algorithm>
#include <string>

#include "ctx.hpp"
#include "msm_kernels.hip.h"

namespace jolt {
namespace dory_batches {
using namespace jolt::msmk;

constexpr size_t kMaxBatchKeys = (size_t)1 << 26;  // keys (points) of one batch: 256 MiB of keys and as much of sorted keys

inline int32_t hip_fail(jolt_ctx* ctx, const char* what, hipError_t e) {
    ctx->last_error = std::string(what) + ": " + hipGetErrorString(e);
    return e == hipErrorOutOfMemory ? JOLT_ERR_OOM : JOLT_ERR_HIP;
}

struct BucketPlan {
    int L;
    uint32_t heavy_threshold, heavy_cap;
};
// V bucket sets of B buckets over n points each
inline BucketPlan plan_buckets(size_t V, uint32_t B, size_t n) {
    BucketPlan p;
    p.L = 1;
    while (p.L < 64 && V * B * (size_t)(2 * p.L) <= 524288) p.L *= 2;  // enough lanes to fill the chip when there are few buckets
    size_t avg = (n + B - 1) / B;
    p.heavy_threshold = (uint32_t)std::min<size_t>((size_t)p.L * std::max<size_t>(kLaneCap, 2 * avg), 0x7FFFFFFFu);
    size_t pts = V * n;
    p.heavy_cap = (uint32_t)std::min<size_t>(pts / kHeavySeg + pts / p.heavy_threshold + 16, 0x7FFFFFFFu);
    return p;  // sources keep V * (B + 1) < 2^32 (bucket slots are u32) by batching at kMaxBatchKeys points
}

struct Workspace {
    uint32_t *keys, *sorted, *hist, *offs, *cur, *heavy, *hcnt;
    G1Jac *buckets, *seg, *out;
    Fq* pool;
};
// Carve lane 0's grow-only MSM workspace for V windows of n points, B buckets each, `outs` result points and `pool` Fq cells (the running products of
// k_dory_hints_normalise; none: the layout the host-pointer entries have always had).  Growing it waits for the stream first: what an earlier carve handed out
// is read back before the next one.
inline int32_t carve(jolt_ctx* ctx, size_t V, size_t n, uint32_t B, uint32_t heavy_cap, size_t outs, Workspace* w, size_t pool = 0) {
    const size_t VB = V * (B + 1);
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    size_t o_keys = take(V * n * 4), o_sorted = take(V * n * 4), o_hist = take(VB * 4), o_offs = take(VB * 4), o_cur = take(VB * 4),
           o_heavy = take((size_t)heavy_cap * 8), o_hcnt = take(256), o_buckets = take(VB * sizeof(G1Jac)),
           o_seg = take((size_t)heavy_cap * sizeof(G1Jac)), o_out = take(outs * sizeof(G1Jac)), o_pool = take(pool * sizeof(Fq));
    ctx->msm_ws_gen[0]++;
    if (off > ctx->msm_ws_cap[0]) {
        if (ctx->msm_ws[0]) {
            JOLT_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            JOLT_HIP_TRY(ctx, hipFree(ctx->msm_ws[0]));
            ctx->msm_ws[0] = nullptr;
            ctx->msm_ws_cap[0] = 0;
        }
        JOLT_HIP_TRY(ctx, hipMalloc(&ctx->msm_ws[0], off));
        ctx->msm_ws_cap[0] = off;
    }
    char* ws = (char*)ctx->msm_ws[0];
    w->keys = (uint32_t*)(ws + o_keys);
    w->sorted = (uint32_t*)(ws + o_sorted);
    w->hist = (uint32_t*)(ws + o_hist);
    w->offs = (uint32_t*)(ws + o_offs);
    w->cur = (uint32_t*)(ws + o_cur);
    w->heavy = (uint32_t*)(ws + o_heavy);
    w->hcnt = (uint32_t*)(ws + o_hcnt);
    w->buckets = (G1Jac*)(ws + o_buckets);
    w->seg = (G1Jac*)(ws + o_seg);
    w->out = (G1Jac*)(ws + o_out);
    w->pool = (Fq*)(ws + o_pool);
    return JOLT_OK;
}

// scan -> scatter -> light / heavy bucket sums for V windows whose keys and histogram are in place (already_sorted: hist / offsets /
// sorted / heavy list were produced by the source's own sort)
inline void launch_bucket_sums(jolt_ctx* ctx, const Workspace& w, const G1Affine* bases, size_t V, size_t n, uint32_t B, const BucketPlan& p, bool already_sorted) {
    hipStream_t st = ctx->stream;
    const unsigned gn = (unsigned)((n + kBlock - 1) / kBlock);
    const unsigned gy = (unsigned)std::min<size_t>(V, 32768), gz = (unsigned)((V + gy - 1) / gy);
    const unsigned gh = std::min<uint32_t>((p.heavy_cap + 3) / 4, 4096);
    if (!already_sorted) {
        hipLaunchKernelGGL(k_msm_scan, dim3((unsigned)V), dim3(kBlock), 0, st, (const uint32_t*)w.hist, w.offs, w.cur, B, p.heavy_threshold, w.heavy, w.hcnt,
                           p.heavy_cap);
        hipLaunchKernelGGL(k_msm_scatter, dim3(gn, gy, gz), dim3(kBlock), 0, st, (const uint32_t*)w.keys, n, B, w.cur, w.sorted, V);
    }
    hipLaunchKernelGGL(k_msm_buckets_light<false>, dim3((unsigned)(((size_t)B * p.L + kBlock - 1) / kBlock), gy, gz), dim3(kBlock), 0, st, (const uint32_t*)w.hist,
                       (const uint32_t*)w.offs, (const uint32_t*)w.sorted, bases, n, B, p.L, p.heavy_threshold, w.buckets, V);
    hipLaunchKernelGGL(k_msm_buckets_heavy<false>, dim3(gh), dim3(kBlock), 0, st, (const uint32_t*)w.heavy, (const uint32_t*)w.hcnt, (const uint32_t*)w.hist,
                       (const uint32_t*)w.offs, (const uint32_t*)w.sorted, bases, n, B, w.seg, LformConsts{});
    hipLaunchKernelGGL(k_msm_heavy_combine, dim3(gh), dim3(kBlock), 0, st, (const uint32_t*)w.heavy, (const uint32_t*)w.hcnt, (const uint32_t*)w.hist,
                       (const G1Jac*)w.seg, w.buckets);
}

// What a source states of its batches: `items` in all (rows, or one-hot chunks), at most `batch` of them per launch set -- the source's own bound, docs/kernels.md
// "Tier-1 batches" -- and per item `windows` bucket sets of `buckets` buckets over `points` points each
struct BatchShape {
    size_t items, batch, windows, points;
    uint32_t buckets;
};

// One launch set per batch, `what` in front of a failure's text.  Beside its `shape` a source has
//   keys(ctx, i0, n, plan, w)   enqueues the keys and histogram of items [i0, i0 + n), or their own sort: true when hist / offsets / sorted / heavy list are in place
//   reduce(ctx, w, n)           enqueues what turns the bucket sums into w.out (the row fold; nothing for one-hot chunks)
// and releases what it holds in its destructor, so every return here is a whole exit.  A sink states the result points and pool cells of n items (outs, pool_cells)
// and takes a batch with emit(ctx, w, i0, n).  Nothing here waits for the device: a sink that hands results to the host does.
template <class Source, class Sink>
int32_t bucket_batches(jolt_ctx* ctx, const G1Affine* bases, const char* what, const Source& source, const Sink& sink) {
    hipStream_t st = ctx->stream;
    const BatchShape& s = source.shape;
    for (size_t i0 = 0; i0 < s.items; i0 += s.batch) {
        const size_t ni = std::min(s.batch, s.items - i0), V = ni * s.windows;
        const BucketPlan p = plan_buckets(V, s.buckets, s.points);
        Workspace w;
        JOLT_TRY(carve(ctx, V, s.points, s.buckets, p.heavy_cap, sink.outs(ni), &w, sink.pool_cells(ni)));
        const size_t VB = V * ((size_t)s.buckets + 1);
        hipError_t e = hipMemsetAsync(w.hist, 0, VB * 4, st);
        if (e == hipSuccess) e = hipMemsetAsync(w.hcnt, 0, 256, st);
        if (e == hipSuccess) e = hipMemsetAsync(w.buckets, 0, VB * sizeof(G1Jac), st);  // z = 0: identity
        if (e != hipSuccess) return hip_fail(ctx, what, e);
        const bool sorted = source.keys(ctx, i0, ni, p, w);
        launch_bucket_sums(ctx, w, bases, V, s.points, s.buckets, p, sorted);
        source.reduce(ctx, w, ni);
        e = sink.emit(ctx, w, i0, ni);
        if (e != hipSuccess) return hip_fail(ctx, what, e);
    }
    return JOLT_OK;
}

}  // namespace dory_batches
}  // namespace jolt
