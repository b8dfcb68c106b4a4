// jolt_amd/csrc/dory.hip -- Dory tier-1 (G1) streaming commitments on gfx950: SURVEY.md section 8(f) row 2.
//
// Replaces the row-commitment work of DoryScheme's streaming interface (crates/jolt-dory/src/streaming.rs):
//   feed_u64 / feed_i128 / feed_i128_rows_with (:115-205)  -> jolt_dory_commit_rows: one G1 MSM per row_width window of
//       small integers, every row over the same first row_width bases (ark msm_u64 / msm_i128: sum_j v_j * G_j, negative
//       values as v = -|v|);
//   process_one_hot_chunk(s_with) (:230-275) -> one_hot_chunk_commitments (:366-419) -> jolt_dory_commit_onehot:
//       commitment[k] = sum of the bases of the columns whose hot row is k (no scalar multiplications at all).
//   feed(&[Fr]) (:53-70), commit_rows_dense (scheme.rs:455-472), commit_advice -> jolt_dory_commit_rows_fr / jolt_dory_hints_rows_fr: the rows of a device field
//       table, the integer rows' kernels instantiated with an eight-word magnitude (dory_rows_fr.hip.h).
// Tier 2 (pairings into GT, commit_rows_tier_2) is outside SURVEY.md section 8.
//
// Both are the bucket method of msm.hip with more bucket sets: a "window" is (row, digit window) for the integer rows and
// one chunk for the one-hot columns, so a whole batch is ONE pass of digits -> scan -> scatter -> bucket sums, followed by
// one workgroup per row that folds its windows (running-sum reduction + Horner).  Only the windows the batch's largest
// magnitude needs are processed (an OR-reduction over the batch decides).  Integer VALU work, no MFMA.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

#include "ctx.hpp"
#include "dory_am.hip.h"
#include "dory_batches.hip.h"
#include "dory_hints.hip.h"
#include "dory_host.hpp"
#include "dory_rows_fr.hip.h"
#include "msm_kernels.hip.h"
#include "onehot.hpp"
#include "srs.hpp"

using namespace jolt;
using namespace jolt::msmk;
using namespace jolt::dory_batches;

#include "ints.hpp"

namespace {

constexpr int kMaxRowWindows = 48;  // LDS window sums of the row fold: 129 bits / c with c >= 3

__host__ __device__ inline size_t int_bytes(int kind) { return kind == JOLT_INT_I128 ? 16 : 8; }

// A fourth kind beside JOLT_INT_U64 / _I64 / _I128, internal to this file: the packed magnitudes k_fr_magnitudes writes for a stretch of a field table
// (dory_rows_fr.hip.h).  The integer kinds carry four magnitude words through the row kernels, this one eight.
constexpr int kKindFrMag = 3;
template <int KIND>
struct MagWords { static constexpr int value = 4; };
template <>
struct MagWords<kKindFrMag> { static constexpr int value = dory_fr::kWords; };

// |v| as a 128-bit magnitude in four u32 (LE) and the sign; a field element's 254-bit magnitude in eight
template <int KIND>
__device__ __forceinline__ void load_magnitude(const void* __restrict__ data, size_t i, uint32_t* m, uint32_t& negative) {
    if constexpr (KIND == kKindFrMag) {
        dory_fr::unpack(reinterpret_cast<const uint4*>(data) + 2 * i, m, negative);
        return;
    }
    uint64_t lo, hi;
    if (KIND == JOLT_INT_I128) {
        const uint64_t* p = reinterpret_cast<const uint64_t*>(data) + 2 * i;
        lo = p[0];
        hi = p[1];
        negative = (uint32_t)(hi >> 63);
        if (negative) {  // two's complement negate; |i128::MIN| = 2^127 still fits
            lo = ~lo + 1;
            hi = ~hi + (lo == 0 ? 1 : 0);
        }
    } else {
        lo = reinterpret_cast<const uint64_t*>(data)[i];
        hi = 0;
        negative = KIND == JOLT_INT_I64 ? (uint32_t)(lo >> 63) : 0u;
        if (negative) lo = ~lo + 1;
    }
    m[0] = (uint32_t)lo; m[1] = (uint32_t)(lo >> 32); m[2] = (uint32_t)hi; m[3] = (uint32_t)(hi >> 32);
}

// OR of all magnitudes of the batch -> its bit length bounds the windows worth processing
template <int KIND>
__global__ __launch_bounds__(kBlock) void k_ints_or(const void* __restrict__ data, size_t n, uint32_t* __restrict__ out4) {
    uint32_t acc[4] = {0, 0, 0, 0};
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) {
        uint32_t m[4], negf;
        load_magnitude<KIND>(data, i, m, negf);
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] |= m[k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        for (int off = 32; off >= 1; off >>= 1) acc[k] |= (uint32_t)__shfl_xor((int)acc[k], off, 64);
        if ((threadIdx.x & 63) == 0 && acc[k]) atomicOr(&out4[k], acc[k]);
    }
}

// Signed c-bit digits of the values of rows [row0, row0 + rows): window (r, w) = r * W + w, keys[window * width + col].
template <int KIND>
__global__ __launch_bounds__(kBlock) void k_rows_digits(const void* __restrict__ data, size_t first, size_t n, uint32_t width_log, int c, int W,
                                                       uint32_t* __restrict__ keys, uint32_t* __restrict__ hist) {
    size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = i < n;
    constexpr int NW = MagWords<KIND>::value;
    uint32_t m[NW] = {}, negv = 0;
    if (live) load_magnitude<KIND>(data, first + i, m, negv);
    const size_t row = i >> width_log, col = i & (((size_t)1 << width_log) - 1);
    const uint32_t B = 1u << (c - 1);
    uint32_t carry = 0;
    for (int w = 0; w < W; ++w) {
        int bit = w * c;
        uint32_t raw = 0;
        if (bit < 32 * NW) {
            int limb = bit >> 5, off = bit & 31;
            uint64_t two = (uint64_t)m[limb] | (limb + 1 < NW ? (uint64_t)m[limb + 1] << 32 : 0ull);
            raw = (uint32_t)(two >> off) & ((1u << c) - 1);
        }
        raw += carry;
        uint32_t mag, negf;
        if (raw > B) { mag = (1u << c) - raw; negf = 1; carry = 1; }
        else { mag = raw; negf = 0; carry = 0; }
        const size_t win = row * (size_t)W + w;
        if (live) keys[(win << width_log) + col] = mag | ((negf ^ negv) << 31);
        const uint32_t slot = (uint32_t)(win * (B + 1) + mag);  // < 2^32 (checked by the host); also the aggregation key, rows may share a wavefront
        WaveAgg ag = wave_aggregate(slot, live && mag != 0);
        if (ag.do_atomic) atomicAdd(&hist[slot], ag.count);
    }
}

using dory_fr::digit_at;  // the signed digit of window w of a magnitude of NW words (dory_rows_fr.hip.h: the host form runs it too)

// Counting sort of one row's digits, window after window, entirely in LDS: blockIdx.x = row.  Replaces digits -> scan -> scatter
// with their two global atomics per key (device-scope atomics cost ~90 ps each on this part: 1.7 of the 11 ms of a
// 2048 x 2048 u64 batch); writes hist / offsets / sorted for the row's W windows and lists the over-full buckets.
template <int KIND>
__global__ __launch_bounds__(kBlock) void k_rows_sort_lds(const void* __restrict__ data, size_t first, uint32_t width_log, int c, int W,
                                                         uint32_t* __restrict__ hist, uint32_t* __restrict__ offsets, uint32_t* __restrict__ sorted,
                                                         uint32_t heavy_threshold, uint32_t* __restrict__ heavy_list, uint32_t* __restrict__ heavy_count,
                                                         uint32_t heavy_cap) {
    extern __shared__ uint32_t rows_sh[];  // B + 1 counters, then kBlock scan cells
    const uint32_t B = 1u << (c - 1), width = 1u << width_log;
    uint32_t* cnt = rows_sh;
    uint32_t* cell = rows_sh + B + 1;
    const size_t row = blockIdx.x;
    const size_t base = first + (row << width_log);
    const uint32_t per = (B + kBlock) / kBlock;  // bins per thread in the scan, bins 0..B
    for (int w = 0; w < W; ++w) {
        for (uint32_t b = threadIdx.x; b <= B; b += kBlock) cnt[b] = 0;
        __syncthreads();
        for (uint32_t col0 = 0; col0 < width; col0 += kBlock) {  // whole wavefronts walk the loop together (ballots inside)
            const uint32_t col = col0 + threadIdx.x;
            uint32_t mag = 0, negf = 0;
            if (col < width) {
                uint32_t m[MagWords<KIND>::value], negv;
                load_magnitude<KIND>(data, base + col, m, negv);
                digit_at<MagWords<KIND>::value>(m, c, w, mag, negf);
            }
            WaveAgg ag = wave_aggregate(mag, mag != 0);
            if (ag.do_atomic) atomicAdd(&cnt[mag], ag.count);
        }
        __syncthreads();
        // exclusive scan of the counters (bin 0 stays empty) -> global hist / offsets; the counters become the scatter cursors
        const uint32_t lo = threadIdx.x * per, hi = min(lo + per, B + 1);
        uint32_t local = 0;
        for (uint32_t k = lo; k < hi; ++k) local += cnt[k];
        cell[threadIdx.x] = local;
        __syncthreads();
        for (int off = 1; off < kBlock; off <<= 1) {
            uint32_t v = (int)threadIdx.x >= off ? cell[threadIdx.x - off] : 0;
            __syncthreads();
            cell[threadIdx.x] += v;
            __syncthreads();
        }
        uint32_t run = cell[threadIdx.x] - local;
        const size_t win = row * (size_t)W + w;
        for (uint32_t k = lo; k < hi; ++k) {
            const uint32_t n_k = cnt[k];
            const uint32_t slot = (uint32_t)(win * (B + 1) + k);
            hist[slot] = n_k;
            offsets[slot] = run;
            cnt[k] = run;
            if (n_k > heavy_threshold) {
                uint32_t nseg = (n_k + kHeavySeg - 1) / kHeavySeg;
                uint32_t f0 = atomicAdd(heavy_count, nseg);
                for (uint32_t sgi = 0; sgi < nseg && f0 + sgi < heavy_cap; ++sgi) {
                    heavy_list[2 * (f0 + sgi)] = slot;
                    heavy_list[2 * (f0 + sgi) + 1] = sgi;
                }
            }
            run += n_k;
        }
        __syncthreads();
        for (uint32_t col0 = 0; col0 < width; col0 += kBlock) {
            const uint32_t col = col0 + threadIdx.x;
            uint32_t mag = 0, negf = 0, negv = 0;
            if (col < width) {
                uint32_t m[MagWords<KIND>::value];
                load_magnitude<KIND>(data, base + col, m, negv);
                digit_at<MagWords<KIND>::value>(m, c, w, mag, negf);
            }
            WaveAgg ag = wave_aggregate(mag, mag != 0);
            uint32_t f0 = 0;
            if (ag.do_atomic) f0 = atomicAdd(&cnt[mag], ag.count);
            uint32_t pos = (uint32_t)__shfl((int)f0, ag.src, 64) + ag.rank;
            if (mag) sorted[(win << width_log) + pos] = col | ((negf ^ negv) << 31);
        }
        __syncthreads();
    }
}

// One workgroup per row: each wavefront folds whole windows (running sums over its lanes' bucket ranges, butterfly over the
// lanes), then one lane runs the Horner recombination acc = 2^c acc + S_w over the row's W window sums.
__global__ __launch_bounds__(kBlock) void k_rows_fold(const G1Jac* __restrict__ buckets, uint32_t B, int c, int W, G1Jac* __restrict__ out) {
    __shared__ G1Jac sm[kMaxRowWindows];
    const size_t row = blockIdx.x;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t G = (B + 63) / 64;
    for (int w = (int)wave; w < W; w += kBlock / 64) {
        const G1Jac* bk = buckets + (row * (size_t)W + w) * (B + 1);
        uint32_t lo = lane * G + 1, hi = min(lo + G - 1, B);
        G1Jac contrib = g1_identity();
        if (lo <= B) {
            G1Jac running = g1_identity(), acc = g1_identity();
            for (uint32_t b = hi; b >= lo; --b) {
                running = g1_add(running, bk[b]);
                acc = g1_add(acc, running);
            }
            contrib = g1_add(acc, g1_mul_small(running, lo - 1));  // sum_b b B_b over the lane's range
        }
        contrib = wave_sum_g1(contrib, 64);
        if (lane == 0) sm[w] = contrib;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        G1Jac acc = g1_identity();
        for (int w = W - 1; w >= 0; --w) {
            for (int k = 0; k < c; ++k) acc = g1_double(acc);
            acc = g1_add(acc, sm[w]);
        }
        out[row] = g1_is_identity(acc) ? g1_identity() : acc;
    }
}

// The same fold for small bucket sets (B <= 128, row widths up to 4096): sum_w 2^(cw) sum_b b B_(w,b) = sum_b b H_b with
// H_b = sum_w 2^(cw) B_(w,b).  Lane b runs the Horner recombination over the windows for ITS bucket -- all lanes in
// lockstep, so the W*c doublings cost one wavefront pass instead of one idle-lane pass per row on top of W butterfly
// reductions -- then a single weighted reduction over the lanes.  Measured 5.3 -> see DESIGN.md on 2048 rows x 2048 u64.
__global__ __launch_bounds__(128) void k_rows_fold_lanes(const G1Jac* __restrict__ buckets, uint32_t B, int c, int W, G1Jac* __restrict__ out) {
    __shared__ G1Jac sm[2];
    const size_t row = blockIdx.x;
    const uint32_t b = threadIdx.x + 1;
    G1Jac h = g1_identity();
    if (b <= B) {
        const G1Jac* bk = buckets + row * (size_t)W * (B + 1) + b;
        for (int w = W - 1; w >= 0; --w) {
            for (int k = 0; k < c; ++k) h = g1_double(h);
            h = g1_add(h, bk[(size_t)w * (B + 1)]);
        }
        h = g1_mul_small(h, b);
    }
    h = wave_sum_g1(h, 64);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = h;
    __syncthreads();
    if (threadIdx.x == 0) {
        G1Jac acc = blockDim.x > 64 ? g1_add(sm[0], sm[1]) : sm[0];
        out[row] = g1_is_identity(acc) ? g1_identity() : acc;
    }
}

// One-hot chunks: window = chunk, key = hot row + 1 (0 = cold cycle, skipped), no signs.
__global__ __launch_bounds__(kBlock) void k_onehot_keys(const uint8_t* __restrict__ idx, uint32_t wide, size_t n, uint32_t width_log, uint32_t K,
                                                       uint32_t* __restrict__ keys, uint32_t* __restrict__ hist) {
    size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = i < n;
    const uint32_t v = live ? hot_load(idx, i, wide) : kColdIdx;
    uint32_t mag = v == kColdIdx ? 0u : v + 1;
    if (live) keys[i] = mag;
    const uint32_t slot = (uint32_t)((i >> width_log) * (K + 1) + mag);
    WaveAgg ag = wave_aggregate(slot, mag != 0);
    if (ag.do_atomic) atomicAdd(&hist[slot], ag.count);
}
__global__ __launch_bounds__(kBlock) void k_onehot_emit(const G1Jac* __restrict__ buckets, uint32_t K, size_t total, G1Jac* __restrict__ out) {
    size_t t = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= total) return;
    G1Jac b = buckets[(t / K) * (K + 1) + (t % K) + 1];
    out[t] = g1_is_identity(b) ? g1_identity() : b;
}

int log2_exact(size_t v) {
    if (v == 0 || (v & (v - 1))) return -1;
    int l = 0;
    while (((size_t)1 << l) < v) ++l;
    return l;
}

}  // namespace

extern "C" int32_t jolt_ints_upload(jolt_ctx* ctx, const void* host, int32_t kind, size_t count, jolt_ints** out) {
    if (!ctx || !out || (!host && count)) return JOLT_ERR_INVALID_ARG;
    if (kind != JOLT_INT_U64 && kind != JOLT_INT_I64 && kind != JOLT_INT_I128) return JOLT_ERR_INVALID_ARG;
    jolt_ints* v = new (std::nothrow) jolt_ints();
    if (!v) return JOLT_ERR_OOM;
    v->ctx = ctx;
    v->count = count;
    v->kind = kind;
    hipError_t e = hipMalloc(&v->data, std::max<size_t>(count, 1) * int_bytes(kind));
    if (e == hipSuccess && count) e = hipMemcpyAsync(v->data, host, count * int_bytes(kind), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        if (v->data) (void)hipFree(v->data);
        delete v;
        return hip_fail(ctx, "ints upload", e);
    }
    *out = v;
    return JOLT_OK;
}

extern "C" int32_t jolt_ints_free(jolt_ctx* ctx, jolt_ints* v) {
    if (!v) return JOLT_OK;
    jolt_ctx* c = v->ctx ? v->ctx : ctx;
    const bool pooled = c && v->data && c->pool_live.count(v->data);  // jolt_ints_from_rows: back to the pool, reused in stream order; uploads: the runtime's block
    if (c && !pooled) (void)hipStreamSynchronize(c->stream);
    if (v->data) { if (c) jolt_internal_dev_free(c, v->data); else (void)hipFree(v->data); }
    delete v;
    return JOLT_OK;
}

// =====================================================================================================================
// The sinks and sources of bucket_batches (dory_batches.hip.h), the one launch loop under every tier-1 entry below.
// =====================================================================================================================
namespace {

// Where a batch of row commitments goes once the fold kernels have left it in the workspace: to the caller's host array, as jolt_dory_commit_rows always has ...
struct RowsToHost {
    jolt_g1_t* out;
    size_t outs(size_t nr) const { return nr; }
    size_t pool_cells(size_t) const { return 0; }
    hipError_t zeros(jolt_ctx*, size_t rows) const {  // all-zero batch: every row commitment is the identity (Bn254G1::default())
        G1Jac id = g1_identity();
        for (size_t r = 0; r < rows; ++r) std::memcpy(&out[r], &id, sizeof(id));
        return hipSuccess;
    }
    hipError_t emit(jolt_ctx* ctx, const Workspace& w, size_t r0, size_t nr) const {
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(out + r0, w.out, nr * sizeof(G1Jac), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        return e;
    }
};
// ... or normalised into a resident G1 view (jolt_dory_hints_rows): enqueued only
struct RowsToView {
    G1Jac* out;
    size_t outs(size_t nr) const { return nr; }
    size_t pool_cells(size_t nr) const { return nr; }
    hipError_t zeros(jolt_ctx* ctx, size_t rows) const {
        hipLaunchKernelGGL(dory_hints::k_dory_hints_identity, dim3((unsigned)((rows + dory_hints::kLanes - 1) / dory_hints::kLanes)), dim3(dory_hints::kLanes), 0, ctx->stream, out, rows);
        return hipGetLastError();
    }
    hipError_t emit(jolt_ctx* ctx, const Workspace& w, size_t r0, size_t nr) const {
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = dory_hints::launch_normalise(ctx->stream, (const G1Jac*)w.out, dory_hints::RowsMap{}, nr, w.pool, out + r0);
        return e;
    }
};
// The one-hot chunks' two: the K bucket sums of every chunk, as they are, to the caller's host array (jolt_dory_commit_onehot) ...
struct OneHotToHost {
    jolt_g1_t* out;
    uint32_t K;
    size_t outs(size_t V) const { return V * K; }
    size_t pool_cells(size_t) const { return 0; }
    hipError_t emit(jolt_ctx* ctx, const Workspace& w, size_t c0, size_t V) const {
        hipLaunchKernelGGL(k_onehot_emit, dim3((unsigned)((V * K + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->stream, (const G1Jac*)w.buckets, K, V * K, w.out);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(out + c0 * K, w.out, V * K * sizeof(G1Jac), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        return e;
    }
};
// ... or normalised straight from the buckets to where OneHotMap places window v0 + i of the column range (jolt_dory_hints_onehot): enqueued only
struct OneHotToView {
    G1Jac* out;
    uint32_t K;
    size_t chunks;
    size_t outs(size_t) const { return 0; }
    size_t pool_cells(size_t V) const { return V * K; }
    hipError_t emit(jolt_ctx* ctx, const Workspace& w, size_t v0, size_t V) const {
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = dory_hints::launch_normalise(ctx->stream, (const G1Jac*)w.buckets, dory_hints::OneHotMap{K, chunks, v0}, V * K, w.pool, out);
        return e;
    }
};

// values->kind as a compile-time constant: f(std::integral_constant<int, KIND>)
template <class F>
void with_int_kind(int kind, F&& f) {
    if (kind == JOLT_INT_U64) f(std::integral_constant<int, JOLT_INT_U64>{});
    else if (kind == JOLT_INT_I64) f(std::integral_constant<int, JOLT_INT_I64>{});
    else f(std::integral_constant<int, JOLT_INT_I128>{});
}

// The integer rows' magnitudes: read in place by the row kernels of the values' kind
struct IntMagnitudes {
    const jolt_ints* values;
    static constexpr int kWords = 4;
    size_t batch_slots() const { return ~(size_t)0; }  // a batch is bounded by its keys alone
    int32_t reserve(size_t) { return JOLT_OK; }  // nothing of its own per batch
    void enqueue_or(hipStream_t st, uint32_t* out) const {
        const unsigned g = (unsigned)std::min<size_t>((values->count + kBlock - 1) / kBlock, 4096);
        with_int_kind(values->kind, [&](auto kind) {
            hipLaunchKernelGGL(k_ints_or<decltype(kind)::value>, dim3(g), dim3(kBlock), 0, st, (const void*)values->data, values->count, out);
        });
    }
    // f(kind, data, first): the magnitudes of values [first, first + n) are data[first ...] for the row kernels of `kind`
    template <class F>
    void stage(hipStream_t, size_t first, size_t, F&& f) const {
        with_int_kind(values->kind, [&](auto kind) { f(kind, (const void*)values->data, first); });
    }
};

// Rows of 2^wl values over the first 2^wl bases: an item is a row, W windows of c bits (2^(c-1) buckets) each
template <class Magnitudes>
struct RowSource {
    const Magnitudes& mags;
    int wl, c, W;
    BatchShape shape;
    bool keys(jolt_ctx* ctx, size_t r0, size_t nr, const BucketPlan& p, const Workspace& w) const {
        hipStream_t st = ctx->stream;
        const size_t nvals = nr << wl;
        const size_t sort_lds = ((size_t)shape.buckets + 1 + kBlock) * sizeof(uint32_t);
        const bool lds_sort = ctx->msm_lds_sort && sort_lds <= 64 * 1024;
        mags.stage(st, r0 << wl, nvals, [&](auto kind, const void* data, size_t first) {
            constexpr int KIND = decltype(kind)::value;
            if (lds_sort)  // one workgroup per row sorts its W windows in LDS
                hipLaunchKernelGGL(k_rows_sort_lds<KIND>, dim3((unsigned)nr), dim3(kBlock), sort_lds, st, data, first, (uint32_t)wl, c, W, w.hist, w.offs, w.sorted,
                                   p.heavy_threshold, w.heavy, w.hcnt, p.heavy_cap);
            else
                hipLaunchKernelGGL(k_rows_digits<KIND>, dim3((unsigned)((nvals + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, data, first, nvals, (uint32_t)wl, c, W, w.keys,
                                   w.hist);
        });
        return lds_sort;
    }
    void reduce(jolt_ctx* ctx, const Workspace& w, size_t nr) const {
        const uint32_t B = shape.buckets;
        if (B <= 128)
            hipLaunchKernelGGL(k_rows_fold_lanes, dim3((unsigned)nr), dim3(B <= 64 ? 64 : 128), 0, ctx->stream, (const G1Jac*)w.buckets, B, c, W, w.out);
        else
            hipLaunchKernelGGL(k_rows_fold, dim3((unsigned)nr), dim3(kBlock), 0, ctx->stream, (const G1Jac*)w.buckets, B, c, W, w.out);
    }
};

// The row commitments of `rows` rows of 2^wl magnitudes (checked by the caller: rows > 0), batch by batch into `sink`: the OR of all magnitudes bounds the windows
// worth processing, an all-zero column never reaches the pipeline.
// (min_window: the narrow rows of the address-major entry ask for wider digits than the ~16 points per bucket rule gives them; 0: the rule alone)
template <class Magnitudes, class Sink>
int32_t commit_rows_into(jolt_ctx* ctx, const G1Affine* bases, const char* what, Magnitudes& mags, int wl, size_t rows, const Sink& sink, int min_window = 0) {
    hipStream_t st = ctx->stream;
    // ---- bit length of the largest magnitude (pinned scratch: the lane-0 MSM result buffer).  The probe's words are read back before the first batch carves:
    // that may move the workspace.
    if (!ctx->msm_host[0]) JOLT_HIP_TRY(ctx, hipHostMalloc(&ctx->msm_host[0], 128 * sizeof(G1Jac), hipHostMallocDefault));
    Workspace probe;
    JOLT_TRY(carve(ctx, 1, 1, 1, 16, 1, &probe));
    JOLT_HIP_TRY(ctx, hipMemsetAsync(probe.hcnt, 0, 256, st));
    mags.enqueue_or(st, probe.hcnt);
    uint32_t* h_or = (uint32_t*)ctx->msm_host[0];
    JOLT_HIP_TRY(ctx, hipMemcpyAsync(h_or, probe.hcnt, 4 * Magnitudes::kWords, hipMemcpyDeviceToHost, st));
    JOLT_HIP_TRY(ctx, hipStreamSynchronize(st));
    int bits = 0;
    for (int k = Magnitudes::kWords - 1; k >= 0 && !bits; --k)
        if (h_or[k]) bits = 32 * k + 32 - __builtin_clz(h_or[k]);
    if (bits == 0) {
        const hipError_t e = sink.zeros(ctx, rows);
        return e == hipSuccess ? JOLT_OK : hip_fail(ctx, what, e);
    }
    // ---- plan: ~16 points per bucket, the top window keeps one spare bit for the signed-digit carry, at most kMaxRowWindows windows (dory_fr::plan)
    int c, W;
    dory_fr::plan(bits, wl, min_window, &c, &W);
    const size_t width = (size_t)1 << wl, B = (size_t)1 << (c - 1);
    const size_t by_keys = kMaxBatchKeys / ((size_t)W * width), by_slots = mags.batch_slots() / ((size_t)W * (B + 1));
    const size_t batch_rows = std::max<size_t>(1, std::min(rows, std::min(by_keys, by_slots)));
    JOLT_TRY(mags.reserve(batch_rows * width));
    return bucket_batches(ctx, bases, what, RowSource<Magnitudes>{mags, wl, c, W, {rows, batch_rows, (size_t)W, width, (uint32_t)B}}, sink);
}

// the argument checks the two row entries share, with the reference's codes; rows = 0: nothing to do
int32_t rows_shape(jolt_ctx* ctx, const jolt_srs* srs, const jolt_ints* values, size_t row_width, int* wl, size_t* rows) {
    *wl = log2_exact(row_width);
    JOLT_REQUIRE(ctx, *wl >= 0, "streaming: row width must be a power of two");  // streaming.rs:99-102
    if (row_width > srs->n) return JOLT_ERR_SRS_TOO_SMALL;                         // :103-108
    if (values->count % row_width) return JOLT_ERR_SIZE_MISMATCH;                  // :192-195
    *rows = values->count / row_width;
    return JOLT_OK;
}

}  // namespace

extern "C" int32_t jolt_dory_commit_rows(jolt_ctx* ctx, const jolt_srs* srs, const jolt_ints* values, size_t row_width, jolt_g1_t* out) {
    if (!ctx || !srs || !values || (!out && values->count)) return JOLT_ERR_INVALID_ARG;
    int wl;
    size_t rows;
    JOLT_TRY(rows_shape(ctx, srs, values, row_width, &wl, &rows));
    if (rows == 0) return JOLT_OK;
    IntMagnitudes mags{values};
    return commit_rows_into(ctx, srs->pts, "dory rows", mags, wl, rows, RowsToHost{out});
}

extern "C" int32_t jolt_dory_hints_rows(jolt_ctx* ctx, const jolt_srs* srs, const jolt_ints* values, size_t row_width, jolt_dory_vec* out, size_t out_first) {
    if (!ctx || !srs || !values || !out) return JOLT_ERR_INVALID_ARG;
    int wl;
    size_t rows;
    JOLT_TRY(rows_shape(ctx, srs, values, row_width, &wl, &rows));
    G1Jac* dst = (G1Jac*)dory_host::g1_view(ctx, out, out_first, rows);
    JOLT_REQUIRE(ctx, dst, "out is not a G1 view of this context that holds the row commitments");
    if (rows == 0) return JOLT_OK;
    IntMagnitudes mags{values};
    return commit_rows_into(ctx, srs->pts, "dory rows", mags, wl, rows, RowsToView{dst});
}

// =====================================================================================================================
// Row commitments of a device field table: StreamingCommitment::feed(&[Fr]) per row (crates/jolt-dory/src/streaming.rs:53-70), the dense arm of DoryScheme::commit
// (commit_rows_dense, scheme.rs:455-472), commit_advice.  The pipeline of the integer rows with an eight-word magnitude (dory_rows_fr.hip.h): one pass over the
// stretch for the OR of the magnitudes, then per batch of rows the packed magnitudes (32 bytes per value, from the pool) and the kKindFrMag instantiations of the
// digit / LDS sort kernels; bucket sums, heavy buckets, the row fold and the sinks are the integer rows' own.
// =====================================================================================================================
namespace {

static_assert(kMaxRowWindows == dory_fr::kMaxWindows, "the window plan of dory_rows_fr.hip.h is cut to the LDS window sums of k_rows_fold");

__global__ __launch_bounds__(kBlock) void k_fr_or(const Fr* __restrict__ table, size_t n, uint32_t* __restrict__ out8) {
    uint32_t acc[dory_fr::kWords] = {};
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) {
        uint32_t m[dory_fr::kWords], negf;
        dory_fr::magnitude(ld_fr(table + i), m, negf);
#pragma unroll
        for (int k = 0; k < dory_fr::kWords; ++k) acc[k] |= m[k];
    }
#pragma unroll
    for (int k = 0; k < dory_fr::kWords; ++k) {
        for (int off = 32; off >= 1; off >>= 1) acc[k] |= (uint32_t)__shfl_xor((int)acc[k], off, 64);
        if ((threadIdx.x & 63) == 0 && acc[k]) atomicOr(&out8[k], acc[k]);
    }
}
__global__ __launch_bounds__(kBlock) void k_fr_magnitudes(const Fr* __restrict__ table, size_t n, uint4* __restrict__ packed) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    uint32_t m[dory_fr::kWords], negf;
    dory_fr::magnitude(ld_fr(table + i), m, negf);
    dory_fr::pack(m, negf, packed + 2 * i);
}

// The field rows' magnitudes of table[0, count): packed per batch into a pool buffer, which goes back to the pool (reuse is stream-ordered) whichever way the entry ends
struct FrMagnitudes {
    jolt_ctx* ctx;
    const Fr* values;
    size_t count;
    uint4* packed = nullptr;
    static constexpr int kWords = dory_fr::kWords;
    FrMagnitudes(jolt_ctx* c, const Fr* v, size_t n) : ctx(c), values(v), count(n) {}
    FrMagnitudes(const FrMagnitudes&) = delete;
    ~FrMagnitudes() { if (packed) jolt_internal_dev_free(ctx, packed); }
    // a batch is bounded by its bucket slots too: the widened digits give narrow rows 33 slots per window where c = 3 gives 5
    size_t batch_slots() const { return dory_fr::kMaxBatchSlots; }
    int32_t reserve(size_t batch_values) { return jolt_internal_dev_alloc(ctx, batch_values * 2 * sizeof(uint4), (void**)&packed); }
    void enqueue_or(hipStream_t st, uint32_t* out) const {
        hipLaunchKernelGGL(k_fr_or, dim3((unsigned)std::min<size_t>((count + kBlock - 1) / kBlock, 4096)), dim3(kBlock), 0, st, values, count, out);
    }
    // the batch's values are packed first: the row kernels read them from the buffer's start
    template <class F>
    void stage(hipStream_t st, size_t first, size_t n, F&& f) const {
        hipLaunchKernelGGL(k_fr_magnitudes, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, values + first, n, packed);
        f(std::integral_constant<int, kKindFrMag>{}, (const void*)packed, (size_t)0);
    }
};

// the argument checks the two field-row entries share: jolt_dory_commit_rows' codes, and the stretch inside the table
int32_t rows_fr_shape(jolt_ctx* ctx, const jolt_srs* srs, const jolt_table* table, size_t first, size_t count, size_t row_width, int* wl, size_t* rows) {
    *wl = log2_exact(row_width);
    JOLT_REQUIRE(ctx, *wl >= 0, "streaming: row width must be a power of two");
    if (row_width > srs->n) return JOLT_ERR_SRS_TOO_SMALL;
    JOLT_REQUIRE(ctx, table->data() && first <= table->len && count <= table->len - first, "the stretch leaves the table");
    if (count % row_width) return JOLT_ERR_SIZE_MISMATCH;
    *rows = count / row_width;
    return JOLT_OK;
}

}  // namespace

extern "C" int32_t jolt_dory_commit_rows_fr(jolt_ctx* ctx, const jolt_srs* srs, const jolt_table* table, size_t first, size_t count, size_t row_width, jolt_g1_t* out) {
    if (!ctx || !srs || !table || (!out && count)) return JOLT_ERR_INVALID_ARG;
    int wl;
    size_t rows;
    JOLT_TRY(rows_fr_shape(ctx, srs, table, first, count, row_width, &wl, &rows));
    if (rows == 0) return JOLT_OK;
    FrMagnitudes mags(ctx, (const Fr*)table->data() + first, count);
    return commit_rows_into(ctx, srs->pts, "dory field rows", mags, wl, rows, RowsToHost{out});
}

extern "C" int32_t jolt_dory_hints_rows_fr(jolt_ctx* ctx, const jolt_srs* srs, const jolt_table* table, size_t first, size_t count, size_t row_width, jolt_dory_vec* out,
                                           size_t out_first) {
    if (!ctx || !srs || !table || !out) return JOLT_ERR_INVALID_ARG;
    int wl;
    size_t rows;
    JOLT_TRY(rows_fr_shape(ctx, srs, table, first, count, row_width, &wl, &rows));
    G1Jac* dst = (G1Jac*)dory_host::g1_view(ctx, out, out_first, rows);
    JOLT_REQUIRE(ctx, dst, "out is not a G1 view of this context that holds the row commitments");
    if (rows == 0) return JOLT_OK;
    FrMagnitudes mags(ctx, (const Fr*)table->data() + first, count);
    return commit_rows_into(ctx, srs->pts, "dory field rows", mags, wl, rows, RowsToView{dst});
}

// The digits the kKindFrMag kernels give one scalar, on the host through the same routines: digits_out[w] = magnitude | negative << 31 of the signed digit of window w
// of min(s, r - s), *negative_out = whether r - s was taken (the kernels fold it into each key's sign).  A plain loop with no window sums to hold: W goes up to the
// ceil(255 / 3) = 85 windows of a full-width magnitude at c = 3, past the cap dory_fr::plan keeps for the device.
extern "C" int32_t jolt_host_dory_fr_digits(const jolt_fr_t* scalar, int32_t c, int32_t W, uint32_t* digits_out, uint32_t* negative_out) {
    if (!scalar || !digits_out || !negative_out || c < 3 || c > 13 || W < 1 || W > dory_fr::kMaxHostWindows) return JOLT_ERR_INVALID_ARG;
    const Fr s = fr_from_abi(scalar);
    if (!fr_is_canonical(s)) return JOLT_ERR_INVALID_ARG;
    uint32_t m[dory_fr::kWords], negv, packed_neg;
    dory_fr::magnitude(s, m, negv);
    uint4 packed[2];
    dory_fr::pack(m, negv, packed);
    dory_fr::unpack(packed, m, packed_neg);
    for (int w = 0; w < W; ++w) {
        uint32_t mag, negf;
        dory_fr::digit_at<dory_fr::kWords>(m, c, w, mag, negf);
        digits_out[w] = mag | (negf << 31);
    }
    *negative_out = packed_neg;
    return JOLT_OK;
}
extern "C" int32_t jolt_host_dory_rows_fr_plan(uint32_t bit_length, size_t row_width, int32_t* c, int32_t* W) {
    const int wl = log2_exact(row_width);
    if (!c || !W || wl < 0 || bit_length == 0 || bit_length > 254) return JOLT_ERR_INVALID_ARG;
    int cc, ww;
    dory_fr::plan((int)bit_length, wl, 0, &cc, &ww);
    *c = cc;
    *W = ww;
    return JOLT_OK;
}

namespace {

// One-hot columns from `first_poly` on as one key stream (the index array is [poly][cycle] contiguous): items = chunks of 2^wl cycles, each ONE window of K buckets whose
// sums are the result as they stand
struct OneHotSource {
    const jolt_onehot* source;
    size_t first_poly;
    int wl;
    BatchShape shape;
    OneHotSource(const jolt_onehot* s, size_t poly, int log_width, size_t windows, size_t batch)
        : source(s), first_poly(poly), wl(log_width), shape{windows, batch, 1, (size_t)1 << log_width, s->k} {}
    bool keys(jolt_ctx* ctx, size_t v0, size_t V, const BucketPlan&, const Workspace& w) const {
        const size_t nvals = V << wl;
        const uint8_t* idx = source->idx + ((first_poly * source->cycles + (v0 << wl)) << source->wide);
        hipLaunchKernelGGL(k_onehot_keys, dim3((unsigned)((nvals + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->stream, idx, source->wide, nvals, (uint32_t)wl, source->k, w.keys,
                           w.hist);
        return false;
    }
    void reduce(jolt_ctx*, const Workspace&, size_t) const {}
};

}  // namespace

extern "C" int32_t jolt_dory_commit_onehot(jolt_ctx* ctx, const jolt_srs* srs, const jolt_onehot* source, size_t poly, size_t chunk_width, jolt_g1_t* out) {
    if (!ctx || !srs || !source || !out) return JOLT_ERR_INVALID_ARG;
    if (poly >= source->n_polys) return JOLT_ERR_INVALID_ARG;
    const int wl = log2_exact(chunk_width);
    JOLT_REQUIRE(ctx, wl >= 0, "streaming one-hot: chunk length must be a power of two");  // streaming.rs:376-380
    if (chunk_width > srs->n) return JOLT_ERR_SRS_TOO_SMALL;                                 // :381-392
    if (source->cycles % chunk_width) return JOLT_ERR_SIZE_MISMATCH;
    const size_t chunks = source->cycles / chunk_width;
    if (chunks == 0) return JOLT_OK;
    const size_t batch = std::max<size_t>(1, std::min(chunks, kMaxBatchKeys / chunk_width));
    return bucket_batches(ctx, srs->pts, "dory one-hot", OneHotSource{source, poly, wl, chunks, batch}, OneHotToHost{out, source->k});
}

// The hints of columns [first_poly, first_poly + n_polys) at once.  The index array is [poly][cycle] contiguous and chunk_width divides the cycle count, so the range is
// ONE key stream whose window i >> log2(chunk_width) runs over (column, chunk): k_onehot_keys and launch_bucket_sums serve a batch of those windows wherever it starts and
// ends, inside a column or across several, and k_dory_hints_normalise writes each bucket where OneHotMap places its window.  Enqueued only: nothing comes back.
extern "C" int32_t jolt_dory_hints_onehot(jolt_ctx* ctx, const jolt_srs* srs, const jolt_onehot* source, size_t first_poly, size_t n_polys, size_t chunk_width,
                                          jolt_dory_vec* out, size_t out_first, size_t batch_points) {
    if (!ctx || !srs || !source || !out) return JOLT_ERR_INVALID_ARG;
    JOLT_REQUIRE(ctx, !(first_poly > source->n_polys || n_polys > source->n_polys - first_poly), "the columns are past the source");
    const int wl = log2_exact(chunk_width);
    JOLT_REQUIRE(ctx, wl >= 0, "streaming one-hot: chunk length must be a power of two");  // streaming.rs:376-380
    if (chunk_width > srs->n) return JOLT_ERR_SRS_TOO_SMALL;                                 // :381-392
    if (source->cycles % chunk_width) return JOLT_ERR_SIZE_MISMATCH;
    JOLT_REQUIRE(ctx, batch_points == 0 || (batch_points >= chunk_width && batch_points % chunk_width == 0), "batch_points is a whole number of chunks");
    const size_t chunks = source->cycles / chunk_width;
    const uint32_t K = source->k;
    size_t per_column = 0, total = 0, windows = 0;
    if (__builtin_mul_overflow((size_t)K, chunks, &per_column) || __builtin_mul_overflow(per_column, n_polys, &total) || __builtin_mul_overflow(n_polys, chunks, &windows))
        return JOLT_ERR_UNSUPPORTED;
    G1Jac* dst = (G1Jac*)dory_host::g1_view(ctx, out, out_first, total);
    JOLT_REQUIRE(ctx, dst, "out is not a G1 view of this context that holds the hints");
    if (total == 0) return JOLT_OK;
    size_t batch = batch_points ? batch_points / chunk_width : std::max<size_t>(1, kMaxBatchKeys / chunk_width);
    batch = std::min(std::min(batch, windows), (size_t)0xFFFFFFFFu / ((size_t)K + 1));  // bucket slots are u32
    if (batch == 0) return JOLT_ERR_UNSUPPORTED;
    return bucket_batches(ctx, srs->pts, "dory one-hot hints", OneHotSource{source, first_poly, wl, windows, batch}, OneHotToView{dst, K, chunks});
}

// k_dory_hints_normalise on the host, for the suite: lane r owns the points [r * run, (r + 1) * run) (on the device a lane's points are interleaved with its neighbours';
// the routine is the same), the pool is a host array
extern "C" int32_t jolt_host_dory_g1_normalise(const jolt_g1_t* points, size_t n, size_t run, jolt_g1_t* out) {
    if (n == 0) return JOLT_OK;
    if (!points || !out || run == 0) return JOLT_ERR_INVALID_ARG;
    std::vector<Fq> pool(n);
    struct Access {
        const jolt_g1_t* points;
        jolt_g1_t* out;
        Fq* pool;
        size_t first;
        G1Jac point(uint32_t j) const {
            G1Jac p;
            std::memcpy(&p, &points[first + j], sizeof(p));
            return p;
        }
        Fq z(uint32_t j) const { return point(j).z; }
        void put(uint32_t j, const Fq& v) const { pool[first + j] = v; }
        Fq get(uint32_t j) const { return pool[first + j]; }
        void store(uint32_t j, const G1Jac& p) const { std::memcpy(&out[first + j], &p, sizeof(p)); }
    };
    const size_t lane_run = std::min<size_t>(run, 0xFFFFFFFFu);
    for (size_t first = 0; first < n; first += lane_run) dory_hints::normalise_run((uint32_t)std::min(lane_run, n - first), Access{points, out, pool.data(), first});
    return JOLT_OK;
}
// OneHotMap on the host: element e of a batch that starts at window0 reads workspace bucket *src and is hint element *dst
extern "C" int32_t jolt_host_dory_hint_map(uint32_t k, size_t chunks, size_t window0, size_t e, size_t* src, size_t* dst) {
    if (!src || !dst || k == 0 || chunks == 0) return JOLT_ERR_INVALID_ARG;
    dory_hints::OneHotMap{k, chunks, window0}.at(e, *src, *dst);
    return JOLT_OK;
}

// =====================================================================================================================
// Address-major placement (dory_am.hip.h): the hints of one-hot and dense columns.  Row r of every column is the cycles [r C, (r + 1) C), C = 2^(sigma - log_block).
// =====================================================================================================================
namespace {

// the shape checks the address-major entries share; *C = cycles per row
int32_t am_shape(jolt_ctx* ctx, uint32_t sigma, uint32_t log_block, uint32_t log_stride, size_t* C) {
    JOLT_REQUIRE(ctx, log_stride <= log_block, "address-major: the one-hot stride exceeds the cycle stride");
    if (sigma < log_block) return JOLT_ERR_UNSUPPORTED;  // a cycle's block wider than a row
    JOLT_REQUIRE(ctx, sigma < 48, "address-major: sigma out of range");
    *C = (size_t)1 << (sigma - log_block);
    return JOLT_OK;
}

size_t am_batch_rows() {  // rows per launch set: 2^20 (128 MiB of sums and pool cells), or the cap the suite sets to force a cut inside a column
    if (const char* e = std::getenv("JOLT_DORY_AM_BATCH_ROWS"))
        if (std::atoll(e) > 0) return (size_t)std::atoll(e);
    return (size_t)1 << 20;
}

}  // namespace

extern "C" int32_t jolt_dory_hints_onehot_am(jolt_ctx* ctx, const jolt_srs* srs, const jolt_onehot* source, size_t first_poly, size_t n_polys, uint32_t sigma,
                                             uint32_t log_block, uint32_t log_stride, jolt_dory_vec* out, size_t out_first) {
    if (!ctx || !srs || !source || !out) return JOLT_ERR_INVALID_ARG;
    JOLT_REQUIRE(ctx, !(first_poly > source->n_polys || n_polys > source->n_polys - first_poly), "the columns are past the source");
    size_t C;
    JOLT_TRY(am_shape(ctx, sigma, log_block, log_stride, &C));
    if (((size_t)1 << sigma) > srs->n) return JOLT_ERR_SRS_TOO_SMALL;
    const uint32_t K = source->k;
    JOLT_REQUIRE(ctx, (log_block - log_stride >= 32 || K <= (1u << (log_block - log_stride))), "address-major: a hot address outside the cycle's block");
    JOLT_REQUIRE(ctx, source->cycles % C == 0, "address-major: the cycles per row do not divide the cycle count");
    const size_t rows = source->cycles / C;
    size_t total = 0;
    if (__builtin_mul_overflow(rows, n_polys, &total)) return JOLT_ERR_UNSUPPORTED;
    G1Jac* dst = (G1Jac*)dory_host::g1_view(ctx, out, out_first, total);
    JOLT_REQUIRE(ctx, dst, "out is not a G1 view of this context that holds the hints");
    if (total == 0) return JOLT_OK;
    if (C > 0xFFFFFFFFull) return JOLT_ERR_UNSUPPORTED;
    hipStream_t st = ctx->stream;
    const size_t width = (size_t)1 << sigma, batch = std::min(am_batch_rows(), total);
    // workspace: the sums of a launch set, their pool cells for the normalisation, then the L-form table (two Fq per base)
    Workspace w;
    JOLT_TRY(carve(ctx, 1, 1, 1, 16, batch, &w, batch + 2 * width));
    G1Affine* table = reinterpret_cast<G1Affine*>(w.pool + batch);
    const dory_am::Consts lc = dory_am::consts();
    hipLaunchKernelGGL(dory_am::k_dory_am_bases, dim3((unsigned)((width + 255) / 256)), dim3(256), 0, st, (const G1Affine*)srs->pts, width, 0u, 1u, lc.one_l, table);
    const uint8_t* idx = source->idx + ((first_poly * source->cycles) << source->wide);
    const uint32_t words = (((C << source->wide) & 7) == 0 && ((uintptr_t)idx & 7) == 0) ? 1u : 0u;
    for (size_t i0 = 0; i0 < total; i0 += batch) {
        const size_t n = std::min(batch, total - i0);
        hipLaunchKernelGGL(dory_am::k_dory_am_onehot_rows, dim3((unsigned)((n + dory_am::kLanes - 1) / dory_am::kLanes)), dim3(dory_am::kLanes), 0, st,
                           idx + ((i0 * C) << source->wide), source->wide, words, n, (uint32_t)C, K, log_block, log_stride, (const G1Affine*)table, lc, w.out);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = dory_hints::launch_normalise(st, (const G1Jac*)w.out, dory_hints::RowsMap{}, n, w.pool, dst + i0);
        if (e != hipSuccess) return hip_fail(ctx, "dory address-major one-hot hints", e);
    }
    return JOLT_OK;
}

// jolt_dory_hints_rows with row width C over the C strided bases srs[j << log_block]: they are gathered into a compact array (at most 2^sigma * 64 bytes, from the
// pool) and the row kernels and the sink of the cycle-major entry run over it, with wider digits than their rule gives short rows.
extern "C" int32_t jolt_dory_hints_rows_am(jolt_ctx* ctx, const jolt_srs* srs, const jolt_ints* values, uint32_t sigma, uint32_t log_block, jolt_dory_vec* out,
                                           size_t out_first) {
    if (!ctx || !srs || !values || !out) return JOLT_ERR_INVALID_ARG;
    size_t C;
    JOLT_TRY(am_shape(ctx, sigma, log_block, 0, &C));
    if (((size_t)1 << sigma) > srs->n) return JOLT_ERR_SRS_TOO_SMALL;
    JOLT_REQUIRE(ctx, values->count % C == 0, "address-major: the cycles per row do not divide the column's length");
    const size_t rows = values->count / C;
    G1Jac* dst = (G1Jac*)dory_host::g1_view(ctx, out, out_first, rows);
    JOLT_REQUIRE(ctx, dst, "out is not a G1 view of this context that holds the row commitments");
    if (rows == 0) return JOLT_OK;
    G1Affine* compact = nullptr;
    JOLT_TRY(jolt_internal_dev_alloc(ctx, C * sizeof(G1Affine), (void**)&compact));
    hipLaunchKernelGGL(dory_am::k_dory_am_bases, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, ctx->stream, (const G1Affine*)srs->pts, C, log_block, 0u, Fq::one(), compact);
    hipError_t e = hipGetLastError();
    int32_t rc = e == hipSuccess ? JOLT_OK : hip_fail(ctx, "dory address-major rows", e);
    if (rc == JOLT_OK) {
        // Rows of C = 2^8 or 2^9 values would get 8 or 16 buckets per window: one bucket per lane leaves most of a wavefront idle in the bucket sums and the row fold
        // (measured 25 ms per column at T = 2^20).  Digits of up to 7 bits fill the 64 lanes; rows shorter than 2^4 keep the rule.
        const int wl = (int)(sigma - log_block);
        IntMagnitudes mags{values};
        rc = commit_rows_into(ctx, compact, "dory address-major rows", mags, wl, rows, RowsToView{dst}, std::min(7, wl - 1));
    }
    jolt_internal_dev_free(ctx, compact);  // back to the pool: reuse is stream-ordered
    return rc;
}

extern "C" int32_t jolt_host_dory_am_place(uint32_t log_block, uint32_t log_stride, uint32_t sigma, size_t cycle, size_t address, size_t* row, size_t* col) {
    if (!row || !col || log_stride > log_block || sigma >= 64 || log_block >= 64) return JOLT_ERR_INVALID_ARG;
    if ((cycle << log_block) >> log_block != cycle || (address << log_stride) >> log_stride != address) return JOLT_ERR_INVALID_ARG;
    const size_t index = dory_am::place(log_block, log_stride, cycle, address);
    if (index < (cycle << log_block)) return JOLT_ERR_INVALID_ARG;
    *row = index >> sigma;
    *col = index & (((size_t)1 << sigma) - 1);
    return JOLT_OK;
}

// dory_am::row_sum -- the routine every lane of k_dory_am_onehot_rows runs -- over one row on the host, then the normalisation; bases in the ABI's form with z = 1
// (z = 0: the point at infinity), cold = 0xFFFF.  One lane sums a whole row, so there is no partition to pass.
extern "C" int32_t jolt_host_dory_am_row(const jolt_g1_t* bases, size_t n_bases, const uint16_t* hot, size_t cycles_in_row, uint32_t k, uint32_t log_block,
                                         uint32_t log_stride, jolt_g1_t* out) {
    if (!bases || !out || (!hot && cycles_in_row) || k == 0 || log_stride > log_block || log_block >= 32 || cycles_in_row > 0xFFFFFFFFull) return JOLT_ERR_INVALID_ARG;
    if (k > (1u << (log_block - log_stride))) return JOLT_ERR_INVALID_ARG;
    if (cycles_in_row && dory_am::place(log_block, log_stride, cycles_in_row - 1, k - 1) >= n_bases) return JOLT_ERR_INVALID_ARG;
    const dory_am::Consts lc = dory_am::consts();
    std::vector<G1Affine> table(n_bases);
    for (size_t i = 0; i < n_bases; ++i) {
        G1Jac p;
        std::memcpy(&p, &bases[i], sizeof(p));
        G1Affine a;
        a.x = p.z.is_zero() ? Fq::zero() : p.x;
        a.y = p.z.is_zero() ? Fq::zero() : p.y;
        table[i] = dory_am::to_lform(a, lc.one_l);
    }
    G1Jac sum = g1_identity();
    if (cycles_in_row)
        sum = dory_am::row_sum((uint32_t)cycles_in_row, k, log_block, log_stride, [&](uint32_t j) { return hot[j] == 0xFFFFu ? 0xFFFFFFFFu : (uint32_t)hot[j]; },
                               table.data(), [](const G1Affine* p) { return *p; }, lc);
    jolt_g1_t raw;
    std::memcpy(&raw, &sum, sizeof(sum));
    return jolt_host_dory_g1_normalise(&raw, 1, 1, out);
}

// =====================================================================================================================
// The opening's G1 and Fr work ahead of the pairing rounds (crates/jolt-dory/src/scheme.rs): the vector-matrix product
// of dory::prove, answered lazily from the per-cycle columns (RlcSource::fold_rows over TraceOpeningPoly,
// crates/jolt-kernels/src/optimized/opening.rs:439-511, crates/jolt-poly/src/multilinear.rs:447-462), and
// DoryScheme::combine_hints (scheme.rs:325-360).  Tier 2 (G2 / GT) and the reduce-and-fold rounds stay on the host.
// =====================================================================================================================
namespace {

constexpr int kFoldMaxSources = 4;   // the limits of jolt_grid_joint_polynomial (pcs.hip)
constexpr int kFoldMaxDense = 8;
constexpr uint32_t kAmFoldSlice = 128;  // matrix rows per thread of k_dory_am_fold: 2^sigma * rows / 128 threads, partial sums of 2^sigma * rows / 128 entries
constexpr uint32_t kFoldSlice = 32;  // matrix rows per address block that one workgroup stages in LDS and one thread walks
struct FoldArgs {
    const uint8_t* idx[kFoldMaxSources];  // [polys of the source][cycles]
    uint32_t wide[kFoldMaxSources];
    uint32_t n_polys[kFoldMaxSources];
    uint32_t first[kFoldMaxSources];      // offset of the source's first polynomial in `scalars`
    int n_sources;
    const Fr* dense[kFoldMaxDense];
    Fr dense_scalar[kFoldMaxDense];
    int n_dense;
};

// sigma <= log_t: the column of grid entry (k, j) is j & (2^sigma - 1) whatever k, so output column c OWNS the cycles c, c + 2^sigma, ... -- a gather, no atomics.
// The M = T / 2^sigma cycles of a column are cut into slices of `slice`; thread = (column, slice): lane <-> column, so the index bytes of a wavefront are 64
// consecutive bytes.  Per polynomial the inner sum is additions only (left[(hot << log_m) + m] picked by the hot address), one multiplication by the polynomial's
// scalar per (polynomial, column, slice).  The K * slice entries of `left` a workgroup can touch sit in LDS (pitch slice + 1: lanes with different hot
// addresses fall on different banks); use_lds = 0 (K too large for LDS) gathers them from global memory, where the 2^nu-entry vector lives in L2.
// partial[s * 2^sigma + c] = the share of slice s; k_dory_fold_sum adds the slices.
__global__ __launch_bounds__(kBlock) void k_dory_fold_cols(FoldArgs a, const Fr* __restrict__ scalars, const Fr* __restrict__ left, uint32_t log_t, uint32_t sigma,
                                                           uint32_t K, uint32_t slice, uint32_t col_groups, uint32_t use_lds, Fr* __restrict__ partial) {
    extern __shared__ __align__(16) unsigned char fold_raw[];
    Fr* sh = reinterpret_cast<Fr*>(fold_raw);
    const uint32_t log_m = log_t - sigma, pitch = slice + 1;
    const size_t cols = (size_t)1 << sigma;
    const uint32_t sl = blockIdx.x / col_groups;
    const size_t c = (size_t)(blockIdx.x % col_groups) * kBlock + threadIdx.x;
    const size_t m0 = (size_t)sl * slice;
    if (use_lds) {
        for (uint32_t e = threadIdx.x; e < K * slice; e += kBlock) {
            const uint32_t h = e / slice, mm = e % slice;
            sh[h * pitch + mm] = ld_fr(left + ((size_t)h << log_m) + m0 + mm);
        }
        __syncthreads();
    }
    if (c >= cols) return;
    Fr acc = Fr::zero();
    for (int s = 0; s < a.n_sources; ++s) {
        for (uint32_t p = 0; p < a.n_polys[s]; ++p) {
            const uint8_t* col = hot_col(a.idx[s], (size_t)p << log_t, a.wide[s]);
            Fr sum = Fr::zero();
            bool any = false;
#pragma unroll 8
            for (uint32_t mm = 0; mm < slice; ++mm) {
                const uint32_t h = hot_load(col, ((m0 + mm) << sigma) + c, a.wide[s]);
                if (h < K) {  // cold cycles (the sentinel) select no row
                    sum = add(sum, use_lds ? sh[h * pitch + mm] : ld_fr(left + ((size_t)h << log_m) + m0 + mm));
                    any = true;
                }
            }
            if (any) acc = add(acc, mul(sum, scalars[a.first[s] + p]));
        }
    }
    for (int d = 0; d < a.n_dense; ++d) {  // dense columns live on address 0: matrix row m, the deferred-reduction accumulator over the slice's products
        Fr sum = Fr::zero();
        WideAcc<FrParams> w = wide_zero<FrParams>();
        int pending = 0;
        for (uint32_t mm = 0; mm < slice; ++mm) {
            const Fr l = use_lds ? sh[mm] : ld_fr(left + m0 + mm);
            wide_fmadd(w, l, ld_fr(a.dense[d] + ((m0 + mm) << sigma) + c));
            if (++pending == kWideMaxProducts) {
                sum = add(sum, wide_reduce(w));
                w = wide_zero<FrParams>();
                pending = 0;
            }
        }
        if (pending) sum = add(sum, wide_reduce(w));
        acc = add(acc, mul(sum, a.dense_scalar[d]));
    }
    st_fr(partial + (size_t)sl * cols + c, acc);
}
__global__ __launch_bounds__(kBlock) void k_dory_fold_sum(const Fr* __restrict__ partial, size_t cols, uint32_t slices, Fr* __restrict__ out) {
    const size_t c = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (c >= cols) return;
    Fr acc = ld_fr(partial + c);
    for (uint32_t s = 1; s < slices; ++s) acc = add(acc, ld_fr(partial + (size_t)s * cols + c));
    st_fr(out + c, acc);
}
// The same product in the address-major placement: output column c = (j << log_block) + (k << log_stride) takes the cycles r C + j of every matrix row r whose hot
// address is k -- a gather, no atomics, and no bins: thread = (column, row slice) compares each index byte with ITS address, so log_k = 8 costs compares, not registers.
// The 2^log_block lanes that share j read the same byte (a broadcast), left[r] is uniform per step; additions only inside, one multiplication by the polynomial's
// scalar per (polynomial, column, slice).  Columns no (j, k) maps to (widened grids) get zero.  Dense columns live on k = 0.  partial[s * 2^sigma + c].
__global__ __launch_bounds__(kBlock) void k_dory_am_fold(FoldArgs a, const Fr* __restrict__ scalars, const Fr* __restrict__ left, size_t T, size_t rows, uint32_t log_block,
                                                         uint32_t log_stride, uint32_t sigma, uint32_t slice, uint32_t col_groups, Fr* __restrict__ partial) {
    const size_t cols = (size_t)1 << sigma;
    const uint32_t sl = blockIdx.x / col_groups;
    const size_t c = (size_t)(blockIdx.x % col_groups) * kBlock + threadIdx.x;
    if (c >= cols) return;
    const size_t C = (size_t)1 << (sigma - log_block), j = c >> log_block;
    const uint32_t within = (uint32_t)(c & (((size_t)1 << log_block) - 1));
    const bool mapped = (within & ((1u << log_stride) - 1)) == 0;
    const uint32_t k = mapped ? within >> log_stride : kColdIdx;  // a cold cycle never equals an address: hot_load gives kColdIdx, an unmapped column asks for it
    const size_t r0 = (size_t)sl * slice, r1 = r0 + slice < rows ? r0 + slice : rows;
    Fr acc = Fr::zero();
    for (int s = 0; s < a.n_sources; ++s) {
        for (uint32_t p = 0; p < a.n_polys[s]; ++p) {
            const uint8_t* col = hot_col(a.idx[s], (size_t)p * T, a.wide[s]);
            Fr sum = Fr::zero();
            bool any = false;
#pragma unroll 4
            for (size_t r = r0; r < r1; ++r) {
                const uint32_t h = hot_load(col, r * C + j, a.wide[s]);
                if (mapped && h == k) {
                    sum = add(sum, ld_fr(left + r));
                    any = true;
                }
            }
            if (any) acc = add(acc, mul(sum, scalars[a.first[s] + p]));
        }
    }
    if (within == 0) {
        for (int d = 0; d < a.n_dense; ++d) {
            Fr sum = Fr::zero();
            WideAcc<FrParams> w = wide_zero<FrParams>();
            int pending = 0;
            for (size_t r = r0; r < r1; ++r) {
                wide_fmadd(w, ld_fr(left + r), ld_fr(a.dense[d] + r * C + j));
                if (++pending == kWideMaxProducts) {
                    sum = add(sum, wide_reduce(w));
                    w = wide_zero<FrParams>();
                    pending = 0;
                }
            }
            if (pending) sum = add(sum, wide_reduce(w));
            acc = add(acc, mul(sum, a.dense_scalar[d]));
        }
    }
    st_fr(partial + (size_t)sl * cols + c, acc);
}
// sigma > log_t: the column index takes in the low sigma - log_t address bits, c = ((hot & amask) << log_t) | j, and the row is hot >> (sigma - log_t).  Still a
// gather: one thread per output column walks the polynomials of its cycle.  The plain general path.
__global__ __launch_bounds__(kBlock) void k_dory_fold_wide(FoldArgs a, const Fr* __restrict__ scalars, const Fr* __restrict__ left, uint32_t log_t, uint32_t sigma,
                                                           uint32_t K, Fr* __restrict__ out) {
    const size_t c = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (c >= ((size_t)1 << sigma)) return;
    const uint32_t shift = sigma - log_t, amask = (1u << shift) - 1;
    const uint32_t lowaddr = (uint32_t)(c >> log_t);
    const size_t j = c & (((size_t)1 << log_t) - 1);
    Fr acc = Fr::zero();
    for (int s = 0; s < a.n_sources; ++s) {
        for (uint32_t p = 0; p < a.n_polys[s]; ++p) {
            const uint32_t h = hot_load(a.idx[s], ((size_t)p << log_t) + j, a.wide[s]);
            if (h < K && (h & amask) == lowaddr) acc = add(acc, mul(ld_fr(left + (h >> shift)), scalars[a.first[s] + p]));
        }
    }
    if (lowaddr == 0) {
        const Fr l0 = ld_fr(left);
        for (int d = 0; d < a.n_dense; ++d) acc = add(acc, mul(mul(l0, ld_fr(a.dense[d] + j)), a.dense_scalar[d]));
    }
    st_fr(out + c, acc);
}

// ---- combine_hints ----------------------------------------------------------------------------------------------------
// out[row] = sum_i s_i P_i[row]: every row multiplies by the SAME scalars, so the signed-digit decomposition is done once on the host and the bucket
// of term i in window w is the same for every row.  Per window the host lists the terms by DESCENDING digit magnitude; a row then needs no bucket array at
// all: walking the list with `running += +-P_i`, and `acc += running` once per magnitude level passed on the way down, gives sum_b b * (bucket b) with
// two accumulators (the running-sum reduction of the bucket method, with the buckets emitted in order).  Control flow depends on the plan alone -- uniform
// over the rows of a wavefront; only the special cases of the group law (identity, P + P, P - P) diverge.
// Group operations per row: windows * (n + 2^(c-1) + c + 1) at most = 51 * (n + 22) for c = 5, against 1.5 * 254 * n of double-and-add.
constexpr int kCombineWindow = 5;                                               // c: signed digits in [-16, 16]
constexpr int kCombineWindows = (254 + 1 + kCombineWindow - 1) / kCombineWindow;  // r < 2^254; one spare bit takes the last carry
constexpr uint32_t kCombineIdxMask = 0x00FFFFFFu;                               // plan entry: term | magnitude << 24 | negative << 31

}  // namespace

// scalars in Montgomery form; false: one of them is not canonical
bool jolt::dory_host::combine_plan(const jolt_fr_t* scalars, size_t n, CombinePlan* plan) {
    constexpr uint32_t B = 1u << (kCombineWindow - 1);
    std::vector<uint8_t> mag((size_t)kCombineWindows * n), sgn((size_t)kCombineWindows * n);
    for (size_t i = 0; i < n; ++i) {
        const Fr m = fr_from_abi(&scalars[i]);
        if (!fr_is_canonical(m)) return false;
        const Fr k = from_mont(m);
        uint32_t carry = 0;
        for (int w = 0; w < kCombineWindows; ++w) {
            const int bit = w * kCombineWindow, limb = bit >> 5, off = bit & 31;
            const uint64_t two = (uint64_t)k.l[limb] | (limb + 1 < 8 ? (uint64_t)k.l[limb + 1] << 32 : 0ull);
            uint32_t raw = ((uint32_t)(two >> off) & ((1u << kCombineWindow) - 1)) + carry;
            if (raw > B) { mag[w * n + i] = (uint8_t)((1u << kCombineWindow) - raw); sgn[w * n + i] = 1; carry = 1; }
            else { mag[w * n + i] = (uint8_t)raw; sgn[w * n + i] = 0; carry = 0; }
        }
    }
    plan->ent.clear();
    plan->start.assign(kCombineWindows + 1, 0);
    for (int w = 0; w < kCombineWindows; ++w) {
        plan->start[w] = (uint32_t)plan->ent.size();
        for (uint32_t b = B; b >= 1; --b)
            for (size_t i = 0; i < n; ++i)
                if (mag[w * n + i] == b) plan->ent.push_back((uint32_t)i | (b << 24) | ((uint32_t)sgn[w * n + i] << 31));
    }
    plan->start[kCombineWindows] = (uint32_t)plan->ent.size();
    return true;
}

namespace {
using jolt::dory_host::CombinePlan;
using jolt::dory_host::combine_plan;

// sum over the window's terms of digit_i * P_i; load(i) = term i's point of this row
template <class Load>
JOLT_HD G1Jac combine_window(const uint32_t* __restrict__ ent, uint32_t count, Load&& load) {
    G1Jac running = g1_identity(), acc = g1_identity();
    uint32_t level = count ? (ent[0] >> 24) & 0x7Fu : 0u;
    for (uint32_t k = 0; k < count; ++k) {
        const uint32_t e = ent[k], m = (e >> 24) & 0x7Fu;
        for (; level > m; --level) acc = g1_add(acc, running);
        G1Jac p = load(e & kCombineIdxMask);
        if (e >> 31) p.y = neg(p.y);
        running = g1_add(running, p);
    }
    for (; level > 0; --level) acc = g1_add(acc, running);
    return acc;
}
// sum_w 2^(c w) S_w, most significant window first; win(w) = S_w
template <class Win>
JOLT_HD G1Jac combine_horner(Win&& win) {
    G1Jac acc = g1_identity();
    for (int w = kCombineWindows - 1; w >= 0; --w) {
        for (int k = 0; k < kCombineWindow; ++k) acc = g1_double(acc);
        acc = g1_add(acc, win(w));
    }
    return acc;
}

// thread = (row, window): blockIdx.y = window, so the plan entries are uniform over the workgroup.  points = the hints back to back, hint i at offset[i] with
// hint_rows[i] rows; a hint shorter than the widest contributes the identity to the rows it lacks.  wsum[w * rows + r], r counted from row0.
__global__ __launch_bounds__(kBlock) void k_dory_combine_windows(const G1Jac* __restrict__ points, const uint64_t* __restrict__ offset, const uint64_t* __restrict__ hint_rows,
                                                                 const uint32_t* __restrict__ ent, const uint32_t* __restrict__ start, size_t row0, size_t rows,
                                                                 G1Jac* __restrict__ wsum) {
    const size_t r = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= rows) return;
    const uint32_t w = blockIdx.y;
    const size_t row = row0 + r;
    const uint32_t lo = start[w], hi = start[w + 1];
    wsum[(size_t)w * rows + r] = combine_window(ent + lo, hi - lo, [&](uint32_t i) { return row < hint_rows[i] ? points[offset[i] + row] : g1_identity(); });
}
__global__ __launch_bounds__(kBlock) void k_dory_combine_horner(const G1Jac* __restrict__ wsum, size_t rows, G1Jac* __restrict__ out) {
    const size_t r = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= rows) return;
    const G1Jac acc = combine_horner([&](int w) { return wsum[(size_t)w * rows + r]; });
    out[r] = g1_is_identity(acc) ? g1_identity() : acc;
}

}  // namespace

namespace {

// What the two grid folds share ahead of their kernels.  The limits, the sources and the dense tables into `a` (*T cycles each, *total one-hot polynomials), the
// canonical-scalar checks, in the order the refusal tests pin; shape(T, &left_len) is the entry's own derivation, run once T is known: it refuses what its placement
// cannot take and states the length `left` has to have.  The grid has 2^log_k addresses per cycle.
template <class Shape>
int32_t fold_gather(jolt_ctx* ctx, const jolt_onehot* const* sources, size_t n_sources, const jolt_fr_t* onehot_scalars, jolt_table* const* dense, size_t n_dense,
                    const jolt_fr_t* dense_scalars, uint32_t log_k, const jolt_table* left, Shape&& shape, FoldArgs* a, size_t* T, size_t* total) {
    if (n_sources > (size_t)kFoldMaxSources || n_dense > (size_t)kFoldMaxDense || log_k > 8 || n_sources + n_dense == 0) return JOLT_ERR_UNSUPPORTED;
    const uint32_t K = 1u << log_k;
    std::memset(a, 0, sizeof(*a));
    for (size_t s = 0; s < n_sources; ++s) if (!sources[s]) return JOLT_ERR_INVALID_ARG;
    for (size_t d = 0; d < n_dense; ++d) if (!dense[d]) return JOLT_ERR_INVALID_ARG;
    *T = n_sources ? sources[0]->cycles : dense[0]->len;
    size_t left_len = 0;
    JOLT_TRY(shape(*T, &left_len));
    *total = 0;
    for (size_t s = 0; s < n_sources; ++s) {
        if (sources[s]->cycles != *T) return JOLT_ERR_SIZE_MISMATCH;
        JOLT_REQUIRE(ctx, sources[s]->k <= K, "fold_rows: a hot address outside the grid");
        a->idx[s] = sources[s]->idx;
        a->wide[s] = sources[s]->wide;
        a->n_polys[s] = (uint32_t)sources[s]->n_polys;
        a->first[s] = (uint32_t)*total;
        *total += sources[s]->n_polys;
    }
    a->n_sources = (int)n_sources;
    for (size_t d = 0; d < n_dense; ++d) {
        if (dense[d]->len != *T) return JOLT_ERR_SIZE_MISMATCH;
        a->dense[d] = dense[d]->data();
        a->dense_scalar[d] = fr_from_abi(&dense_scalars[d]);
        JOLT_REQUIRE(ctx, fr_is_canonical(a->dense_scalar[d]), "scalar is not a canonical Fr");
    }
    a->n_dense = (int)n_dense;
    if (left->len != left_len) return JOLT_ERR_SIZE_MISMATCH;
    for (size_t p = 0; p < *total; ++p) JOLT_REQUIRE(ctx, fr_is_canonical(fr_from_abi(&onehot_scalars[p])), "scalar is not a canonical Fr");
    return JOLT_OK;
}

// ... and behind them: the result table of 2^sigma columns, the one-hot scalars on the device, then launch(scalars, dst, groups) -- the entry's kernel over `groups`
// column groups, writing `slices` partial tables into dst, which k_dory_fold_sum adds when there is more than one.  Everything is released in one place and *out is
// written only on success.
template <class Launch>
int32_t fold_finish(jolt_ctx* ctx, const jolt_fr_t* onehot_scalars, size_t total, uint32_t sigma, size_t slices, Launch&& launch, jolt_table** out) {
    const size_t cols = (size_t)1 << sigma, groups = (cols + kBlock - 1) / kBlock;
    jolt_table *r = nullptr, *ds = nullptr;
    Fr* partial = nullptr;
    JOLT_TRY(jolt_internal_table_new(ctx, cols, &r));
    int32_t st = total ? jolt_table_upload(ctx, onehot_scalars, total, &ds) : JOLT_OK;  // synchronises: the caller's array may be short-lived
    if (st == JOLT_OK && slices * groups > 0x7FFFFFFFull) st = JOLT_ERR_UNSUPPORTED;
    if (st == JOLT_OK && slices > 1) st = jolt_internal_dev_alloc(ctx, slices * cols * sizeof(Fr), (void**)&partial);
    if (st == JOLT_OK) {
        launch(ds ? (const Fr*)ds->data() : (const Fr*)nullptr, partial ? partial : r->data(), groups);
        if (slices > 1) hipLaunchKernelGGL(k_dory_fold_sum, dim3((unsigned)groups), dim3(kBlock), 0, ctx->stream, (const Fr*)partial, cols, (uint32_t)slices, r->data());
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) {
            ctx->last_error = hipGetErrorString(e);
            st = JOLT_ERR_HIP;
        }
    }
    if (partial) jolt_internal_dev_free(ctx, partial);  // back to the pool: reuse is stream-ordered
    if (ds) jolt_table_free(ctx, ds);
    if (st != JOLT_OK) {
        jolt_table_free(ctx, r);
        return st;
    }
    *out = r;
    return JOLT_OK;
}

}  // namespace

extern "C" int32_t jolt_dory_fold_rows_grid(jolt_ctx* ctx, const jolt_onehot* const* sources, size_t n_sources, const jolt_fr_t* onehot_scalars,
                                            jolt_table* const* dense, size_t n_dense, const jolt_fr_t* dense_scalars, uint32_t log_k, uint32_t sigma,
                                            const jolt_table* left, jolt_table** out) {
    if (!ctx || !out || !left || (n_sources && (!sources || !onehot_scalars)) || (n_dense && (!dense || !dense_scalars))) return JOLT_ERR_INVALID_ARG;
    FoldArgs a;
    size_t T, total;
    int log_t = 0;
    auto shape = [&](size_t cycles, size_t* left_len) -> int32_t {
        log_t = log2_exact(cycles);
        JOLT_REQUIRE(ctx, log_t >= 0, "fold_rows: the cycle count must be a power of two");
        JOLT_REQUIRE(ctx, sigma <= log_k + (uint32_t)log_t, "fold_rows: sigma exceeds the grid's variables");
        *left_len = (size_t)1 << (log_k + (uint32_t)log_t - sigma);  // 2^nu matrix rows
        return JOLT_OK;
    };
    JOLT_TRY(fold_gather(ctx, sources, n_sources, onehot_scalars, dense, n_dense, dense_scalars, log_k, left, shape, &a, &T, &total));
    const uint32_t K = 1u << log_k;
    const Fr* lv = (const Fr*)left->data();
    if (sigma > (uint32_t)log_t)
        return fold_finish(ctx, onehot_scalars, total, sigma, 1, [&](const Fr* scalars, Fr* dst, size_t groups) {
            hipLaunchKernelGGL(k_dory_fold_wide, dim3((unsigned)groups), dim3(kBlock), 0, ctx->stream, a, scalars, lv, (uint32_t)log_t, sigma, K, dst);
        }, out);
    const size_t M = T >> sigma;
    const uint32_t slice = (uint32_t)std::min<size_t>(M, kFoldSlice);
    const size_t slices = M / slice, lds = (size_t)K * (slice + 1) * sizeof(Fr);
    const uint32_t use_lds = lds <= 48 * 1024 ? 1u : 0u;
    return fold_finish(ctx, onehot_scalars, total, sigma, slices, [&](const Fr* scalars, Fr* dst, size_t groups) {
        hipLaunchKernelGGL(k_dory_fold_cols, dim3((unsigned)(slices * groups)), dim3(kBlock), use_lds ? lds : 0, ctx->stream, a, scalars, lv, (uint32_t)log_t, sigma, K, slice,
                           (uint32_t)groups, use_lds, dst);
    }, out);
}

extern "C" int32_t jolt_dory_fold_rows_grid_am(jolt_ctx* ctx, const jolt_onehot* const* sources, size_t n_sources, const jolt_fr_t* onehot_scalars,
                                               jolt_table* const* dense, size_t n_dense, const jolt_fr_t* dense_scalars, uint32_t log_block, uint32_t log_stride,
                                               uint32_t sigma, const jolt_table* left, jolt_table** out) {
    if (!ctx || !out || !left || (n_sources && (!sources || !onehot_scalars)) || (n_dense && (!dense || !dense_scalars))) return JOLT_ERR_INVALID_ARG;
    size_t C;
    JOLT_TRY(am_shape(ctx, sigma, log_block, log_stride, &C));
    FoldArgs a;
    size_t T, total, rows = 0;
    auto shape = [&](size_t cycles, size_t* left_len) -> int32_t {
        JOLT_REQUIRE(ctx, cycles % C == 0, "address-major: the cycles per row do not divide the cycle count");
        *left_len = rows = cycles / C;
        return JOLT_OK;
    };
    JOLT_TRY(fold_gather(ctx, sources, n_sources, onehot_scalars, dense, n_dense, dense_scalars, log_block - log_stride, left, shape, &a, &T, &total));
    if (rows == 0) return JOLT_ERR_SIZE_MISMATCH;
    const uint32_t slice = (uint32_t)std::min<size_t>(rows, kAmFoldSlice);
    const size_t slices = (rows + slice - 1) / slice;
    return fold_finish(ctx, onehot_scalars, total, sigma, slices, [&](const Fr* scalars, Fr* dst, size_t groups) {
        hipLaunchKernelGGL(k_dory_am_fold, dim3((unsigned)(slices * groups)), dim3(kBlock), 0, ctx->stream, a, scalars, (const Fr*)left->data(), T, rows, log_block, log_stride,
                           sigma, slice, (uint32_t)groups, dst);
    }, out);
}

// ---- fold_rows of dense field tables, whole or block-embedded ----------------------------------------------------------------
// BlockOpeningPoly::fold_rows (crates/jolt-kernels/src/optimized/opening.rs:594-611): table d is a 2^(m_d - sigma_d) x 2^sigma_d matrix placed top-left in the
// 2^nu x 2^sigma grid, coefficient r * 2^sigma_d + c at grid index r * 2^sigma + c.  Lane = column: a wavefront reads 64 consecutive field elements of a table row
// and one (uniform) entry of `left`; the rows are cut into slices of kBlockFoldSlice, thread = (column, slice), products through the deferred-reduction accumulator
// of the dense columns of k_dory_fold_cols.  partial[s * 2^sigma + c]; k_dory_fold_blocks_sum adds the slices and `base`.  No zero test per entry.
namespace {

constexpr uint32_t kBlockFoldSlice = 64;  // matrix rows per thread: DORY_BLOCK_FOLD_SLICE of jolt_amd/ffi.py
struct BlockFoldArgs {
    const Fr* table[kFoldMaxDense];
    Fr scalar[kFoldMaxDense];
    uint32_t sigma_d[kFoldMaxDense];
    uint32_t log_rows[kFoldMaxDense];
    int n;
};

__global__ __launch_bounds__(kBlock) void k_dory_fold_blocks(BlockFoldArgs a, const Fr* __restrict__ left, uint32_t sigma, uint32_t col_groups, Fr* __restrict__ partial) {
    const size_t cols = (size_t)1 << sigma;
    const uint32_t sl = blockIdx.x / col_groups;
    const size_t c = (size_t)(blockIdx.x % col_groups) * kBlock + threadIdx.x;
    if (c >= cols) return;
    const size_t r0 = (size_t)sl * kBlockFoldSlice;
    Fr acc = Fr::zero();
    for (int d = 0; d < a.n; ++d) {
        const size_t rows = (size_t)1 << a.log_rows[d], r1 = r0 + kBlockFoldSlice < rows ? r0 + kBlockFoldSlice : rows;
        if ((c >> a.sigma_d[d]) != 0 || r0 >= r1) continue;  // outside the block
        const Fr* col = a.table[d] + c;
        Fr sum = Fr::zero();
        WideAcc<FrParams> w = wide_zero<FrParams>();
        int pending = 0;
        for (size_t r = r0; r < r1; ++r) {
            wide_fmadd(w, ld_fr(left + r), ld_fr(col + (r << a.sigma_d[d])));
            if (++pending == kWideMaxProducts) {
                sum = add(sum, wide_reduce(w));
                w = wide_zero<FrParams>();
                pending = 0;
            }
        }
        if (pending) sum = add(sum, wide_reduce(w));
        acc = add(acc, mul(sum, a.scalar[d]));
    }
    st_fr(partial + (size_t)sl * cols + c, acc);
}
__global__ __launch_bounds__(kBlock) void k_dory_fold_blocks_sum(const Fr* __restrict__ partial, const Fr* __restrict__ base, size_t cols, uint32_t slices,
                                                                 Fr* __restrict__ out) {
    const size_t c = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (c >= cols) return;
    Fr acc = base ? ld_fr(base + c) : Fr::zero();
    for (uint32_t s = 0; s < slices; ++s) acc = add(acc, ld_fr(partial + (size_t)s * cols + c));
    st_fr(out + c, acc);
}

// ---- the claims of block-embedded tables: claims[d] = sum_r L[r] * sum_c R[c] * table_d[(r << sigma_d) + c] ----
// The statement's (already scaled) claim of a BlockOpeningPoly at the grid-order opening point, L = eq(point[:nu]), R = eq(point[nu:]).  ONE launch over all tables:
// blockIdx.y names the table, its descriptor is read from device memory (256 of them do not fit kernel arguments).  A table is cut into UNITS of consecutive entries
// that one wavefront serves, lane <-> entry, so a wavefront reads 64 consecutive field elements: at 2^sigma_d >= 64 columns a unit is min(2^sigma_d, 64 *
// kEvalBlockRun) entries of ONE row -- a lane's products R[c] * entry go through the deferred-reduction accumulator (at most kEvalBlockRun <= kWideMaxProducts of
// them) and are multiplied by L[r] once; below 64 columns a unit is 64 entries of 64 / 2^sigma_d rows, one product per lane and its own L[r].  Waves stride over the
// units, so the launch may be capped.  No atomics: a workgroup's sum goes to partials[table * gridDim.x + block] and k_dory_eval_blocks_sum adds them, so the claims
// are the same field elements for every grid.
constexpr size_t kBlocksMax = 256;       // tables per call of jolt_dory_evaluate_blocks and jolt_dory_fold_rows_blocks_many
constexpr uint32_t kEvalBlockLogRun = 3;
constexpr uint32_t kEvalBlockRun = 1u << kEvalBlockLogRun;  // products per lane and unit
static_assert(kEvalBlockRun <= (uint32_t)kWideMaxProducts, "a unit's products fit one deferred reduction");
struct BlockDesc {
    const Fr* table;
    uint32_t sigma_d, log_len;
};
__host__ __device__ inline uint32_t eval_block_log_unit(uint32_t sigma_d) { return sigma_d < 6 ? 6 : (sigma_d < 6 + kEvalBlockLogRun ? sigma_d : 6 + kEvalBlockLogRun); }

__global__ __launch_bounds__(kBlock) void k_dory_eval_blocks(const BlockDesc* __restrict__ descs, const Fr* __restrict__ left, const Fr* __restrict__ right,
                                                             Fr* __restrict__ partials) {
    const BlockDesc d = descs[blockIdx.y];  // uniform over the workgroup
    const size_t len = (size_t)1 << d.log_len, mask = ((size_t)1 << d.sigma_d) - 1;
    const uint32_t log_unit = eval_block_log_unit(d.sigma_d);
    const size_t units = (len + (((size_t)1 << log_unit) - 1)) >> log_unit;
    const uint32_t lane = threadIdx.x & 63;
    const size_t waves = (size_t)gridDim.x * (kBlock / 64);
    Fr acc[1] = {Fr::zero()};
    for (size_t u = (size_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); u < units; u += waves) {
        const size_t i0 = (u << log_unit) + lane;
        const size_t end = ((u + 1) << log_unit) < len ? ((u + 1) << log_unit) : len;
        if (i0 >= end) continue;  // a table of fewer than 64 entries
        WideAcc<FrParams> w = wide_zero<FrParams>();
        for (size_t i = i0; i < end; i += 64) wide_fmadd(w, ld_fr(right + (i & mask)), ld_fr(d.table + i));  // one row: 2^log_unit <= 2^sigma_d wherever a lane has two entries
        acc[0] = add(acc[0], mul(wide_reduce(w), ld_fr(left + (i0 >> d.sigma_d))));
    }
    block_reduce_store_at<1>(acc, partials + (size_t)blockIdx.y * gridDim.x + blockIdx.x);
}
// one workgroup per table: out[d] = the sum of its n_blocks partial sums
__global__ __launch_bounds__(kBlock) void k_dory_eval_blocks_sum(const Fr* __restrict__ partials, uint32_t n_blocks, Fr* __restrict__ out) {
    Fr acc[1] = {Fr::zero()};
    for (uint32_t b = threadIdx.x; b < n_blocks; b += kBlock) acc[0] = add(acc[0], ld_fr(partials + (size_t)blockIdx.x * n_blocks + b));
    block_reduce_store_at<1>(acc, out + blockIdx.x);
}

size_t eval_blocks_cap() {  // workgroups per table at most: unset, the launch stays near 2048 workgroups; the suite sets it to make waves stride at small sizes
    if (const char* e = std::getenv("JOLT_DORY_EVAL_BLOCKS_CAP"))
        if (std::atoll(e) > 0) return (size_t)std::atoll(e);
    return 0;
}

}  // namespace

// One launch set of at most kFoldMaxDense tables: out[c] = (base ? base[c] : 0) + the tables' fold.  Everything was checked by the caller; enqueue only.
static int32_t fold_blocks_enqueue(jolt_ctx* ctx, const BlockFoldArgs& a, size_t max_rows, uint32_t sigma, const Fr* left, const Fr* base, Fr* out) {
    const size_t cols = (size_t)1 << sigma;
    const size_t slices = (max_rows + kBlockFoldSlice - 1) / kBlockFoldSlice, groups = (cols + kBlock - 1) / kBlock;
    Fr* partial = nullptr;
    const bool direct = slices == 1 && !base;
    if (!direct) JOLT_TRY(jolt_internal_dev_alloc(ctx, slices * cols * sizeof(Fr), (void**)&partial));
    hipLaunchKernelGGL(k_dory_fold_blocks, dim3((unsigned)(slices * groups)), dim3(kBlock), 0, ctx->stream, a, left, sigma, (uint32_t)groups, direct ? out : partial);
    if (!direct) hipLaunchKernelGGL(k_dory_fold_blocks_sum, dim3((unsigned)groups), dim3(kBlock), 0, ctx->stream, (const Fr*)partial, base, cols, (uint32_t)slices, out);
    const hipError_t e = hipGetLastError();
    if (partial) jolt_internal_dev_free(ctx, partial);  // back to the pool: reuse is stream-ordered
    if (e != hipSuccess) { ctx->last_error = hipGetErrorString(e); return JOLT_ERR_HIP; }
    return JOLT_OK;
}

// The wide form: up to kBlocksMax tables as a CHAIN of launch sets of kFoldMaxDense, each taking the running output as its base (field addition is exact, so the
// grouping does not show in the output; at most eight tables are one set, the launches jolt_dory_fold_rows_blocks always made).  Two result tables alternate, so that
// no launch reads the table it writes.
extern "C" int32_t jolt_dory_fold_rows_blocks_many(jolt_ctx* ctx, jolt_table* const* tables, const uint32_t* sigma_tables, size_t n_tables, const jolt_fr_t* scalars,
                                                   uint32_t sigma, const jolt_table* left, const jolt_table* base, jolt_table** out) {
    if (!ctx || !out || !left || !tables || !sigma_tables || !scalars || n_tables == 0) return JOLT_ERR_INVALID_ARG;
    if (n_tables > kBlocksMax) return JOLT_ERR_UNSUPPORTED;
    JOLT_REQUIRE(ctx, sigma < 48 && left->data(), "fold_rows: sigma out of range");
    const size_t n_sets = (n_tables + kFoldMaxDense - 1) / kFoldMaxDense;
    std::vector<BlockFoldArgs> sets(n_sets);
    std::vector<size_t> set_rows(n_sets, 0);
    std::memset(sets.data(), 0, n_sets * sizeof(BlockFoldArgs));
    size_t max_rows = 0;
    for (size_t d = 0; d < n_tables; ++d) {
        if (!tables[d] || !tables[d]->data()) return JOLT_ERR_INVALID_ARG;
        const int m = log2_exact(tables[d]->len);
        JOLT_REQUIRE(ctx, m >= 0, "fold_rows: a block's length must be a power of two");
        JOLT_REQUIRE(ctx, sigma_tables[d] <= (uint32_t)m && sigma_tables[d] <= sigma, "fold_rows: a block's columns exceed its variables or the grid's");
        BlockFoldArgs& a = sets[d / kFoldMaxDense];
        const size_t k = d % kFoldMaxDense;
        a.table[k] = tables[d]->data();
        a.sigma_d[k] = sigma_tables[d];
        a.log_rows[k] = (uint32_t)m - sigma_tables[d];
        a.scalar[k] = fr_from_abi(&scalars[d]);
        JOLT_REQUIRE(ctx, fr_is_canonical(a.scalar[k]), "scalar is not a canonical Fr");
        a.n = (int)k + 1;
        set_rows[d / kFoldMaxDense] = std::max(set_rows[d / kFoldMaxDense], (size_t)1 << a.log_rows[k]);
        max_rows = std::max(max_rows, (size_t)1 << a.log_rows[k]);
    }
    if (max_rows > left->len) return JOLT_ERR_SIZE_MISMATCH;
    const size_t cols = (size_t)1 << sigma;
    if (base && (!base->data() || base->len != cols)) return JOLT_ERR_SIZE_MISMATCH;
    if ((max_rows + kBlockFoldSlice - 1) / kBlockFoldSlice * ((cols + kBlock - 1) / kBlock) > 0x7FFFFFFFull) return JOLT_ERR_UNSUPPORTED;
    jolt_table* r[2] = {nullptr, nullptr};
    JOLT_TRY(jolt_internal_table_new(ctx, cols, &r[0]));
    int32_t st = n_sets > 1 ? jolt_internal_table_new(ctx, cols, &r[1]) : JOLT_OK;
    const Fr* running = base ? (const Fr*)base->data() : (const Fr*)nullptr;
    size_t at = (n_sets - 1) & 1;  // the last set writes r[0]
    for (size_t g = 0; g < n_sets && st == JOLT_OK; ++g, at ^= 1) {
        st = fold_blocks_enqueue(ctx, sets[g], set_rows[g], sigma, (const Fr*)left->data(), running, r[at]->data());
        running = r[at]->data();
    }
    if (r[1]) jolt_table_free(ctx, r[1]);  // back to the pool: reuse is stream-ordered
    if (st != JOLT_OK) { jolt_table_free(ctx, r[0]); return st; }
    *out = r[0];
    return JOLT_OK;
}

extern "C" int32_t jolt_dory_fold_rows_blocks(jolt_ctx* ctx, jolt_table* const* tables, const uint32_t* sigma_tables, size_t n_tables, const jolt_fr_t* scalars,
                                              uint32_t sigma, const jolt_table* left, const jolt_table* base, jolt_table** out) {
    if (!ctx || !out || !left || !tables || !sigma_tables || !scalars || n_tables == 0) return JOLT_ERR_INVALID_ARG;
    if (n_tables > (size_t)kFoldMaxDense) return JOLT_ERR_UNSUPPORTED;  // this entry keeps its limit; the wide form is the entry above
    return jolt_dory_fold_rows_blocks_many(ctx, tables, sigma_tables, n_tables, scalars, sigma, left, base, out);
}

// The claims a stage-8 statement holds for its block-embedded polynomials (crates/jolt-prover/src/dory/stages/stage8.rs:148-162, opening_claim * entry.scale: the
// Lagrange factors of the grid's high row and column coordinates sit inside L[r] and R[c] for the small r and c a block reaches).  Two launches (k_dory_eval_blocks,
// k_dory_eval_blocks_sum), one upload of the descriptors and one download, which synchronises the stream.
extern "C" int32_t jolt_dory_evaluate_blocks(jolt_ctx* ctx, jolt_table* const* tables, const uint32_t* sigma_tables, size_t n_tables, const jolt_fr_t* point, size_t n_point,
                                             uint32_t nu, uint32_t sigma, jolt_fr_t* claims_out) {
    if (!ctx || !tables || !sigma_tables || !point || !claims_out || n_tables == 0) return JOLT_ERR_INVALID_ARG;
    if (n_tables > kBlocksMax) return JOLT_ERR_UNSUPPORTED;
    // ---- every check before anything is enqueued ----
    JOLT_REQUIRE(ctx, sigma < 48 && nu < 48, "evaluate_blocks: sigma or nu out of range");
    JOLT_REQUIRE(ctx, n_point == (size_t)nu + sigma, "evaluate_blocks: the point has nu + sigma coordinates");
    std::vector<BlockDesc> descs(n_tables);
    size_t max_rows = 0, max_units = 1;
    for (size_t d = 0; d < n_tables; ++d) {
        if (!tables[d] || tables[d]->ctx != ctx || !tables[d]->data()) return JOLT_ERR_INVALID_ARG;
        const int m = log2_exact(tables[d]->len);
        JOLT_REQUIRE(ctx, m >= 0, "evaluate_blocks: a block's length must be a power of two");
        JOLT_REQUIRE(ctx, sigma_tables[d] <= (uint32_t)m && sigma_tables[d] <= sigma, "evaluate_blocks: a block's columns exceed its variables or the grid's");
        descs[d] = BlockDesc{tables[d]->data(), sigma_tables[d], (uint32_t)m};
        max_rows = std::max(max_rows, (size_t)1 << ((uint32_t)m - sigma_tables[d]));
        const uint32_t log_unit = eval_block_log_unit(sigma_tables[d]);
        max_units = std::max(max_units, (tables[d]->len + (((size_t)1 << log_unit) - 1)) >> log_unit);
    }
    if (max_rows > (size_t)1 << nu) return JOLT_ERR_SIZE_MISMATCH;
    for (size_t i = 0; i < n_point; ++i) JOLT_REQUIRE(ctx, fr_is_canonical(fr_from_abi(&point[i])), "evaluate_blocks: a coordinate is not a canonical Fr");
    // a workgroup per four units of the largest table, capped so that the launch stays near 2048 workgroups; the waves stride over the rest
    const size_t forced = eval_blocks_cap(), cap = forced ? forced : std::max<size_t>(1, 2048 / n_tables);
    const size_t n_blocks = std::max<size_t>(1, std::min<size_t>((max_units + kBlock / 64 - 1) / (kBlock / 64), std::min<size_t>(cap, 65535)));

    jolt_table *left = nullptr, *right = nullptr, *out = nullptr;
    Fr* partials = nullptr;
    BlockDesc* d_descs = nullptr;
    const jolt_fr_t one = [] { jolt_fr_t o; fr_to_abi(&o, Fr::one()); return o; }();
    int32_t st = nu ? jolt_eq_evals(ctx, point, nu, nullptr, &left) : jolt_table_upload(ctx, &one, 1, &left);
    if (st == JOLT_OK) st = sigma ? jolt_eq_evals(ctx, point + nu, sigma, nullptr, &right) : jolt_table_upload(ctx, &one, 1, &right);
    if (st == JOLT_OK) st = jolt_internal_table_new(ctx, n_tables, &out);
    if (st == JOLT_OK) st = jolt_internal_dev_alloc(ctx, n_tables * n_blocks * sizeof(Fr), (void**)&partials);
    if (st == JOLT_OK) st = jolt_internal_dev_alloc(ctx, n_tables * sizeof(BlockDesc), (void**)&d_descs);
    if (st == JOLT_OK) {
        hipError_t e = hipMemcpyAsync(d_descs, descs.data(), n_tables * sizeof(BlockDesc), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_dory_eval_blocks, dim3((unsigned)n_blocks, (unsigned)n_tables), dim3(kBlock), 0, ctx->stream, (const BlockDesc*)d_descs, (const Fr*)left->data(),
                               (const Fr*)right->data(), partials);
            hipLaunchKernelGGL(k_dory_eval_blocks_sum, dim3((unsigned)n_tables), dim3(kBlock), 0, ctx->stream, (const Fr*)partials, (uint32_t)n_blocks, out->data());
            e = hipGetLastError();
        }
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(ctx->stream);  // `descs` is read by the copy until here
            ctx->last_error = std::string("evaluate_blocks: ") + hipGetErrorString(e);
            st = JOLT_ERR_HIP;
        } else {
            st = jolt_table_download(ctx, out, 0, n_tables, claims_out);  // synchronises the stream
        }
    }
    if (partials) jolt_internal_dev_free(ctx, partials);  // back to the pool: reuse is stream-ordered
    if (d_descs) jolt_internal_dev_free(ctx, d_descs);
    for (jolt_table* t : {left, right, out})
        if (t) jolt_table_free(ctx, t);
    return st;
}

// grid index of coefficient i of a block of 2^sigma_table columns embedded top-left in a grid of 2^sigma_grid columns
extern "C" int32_t jolt_host_dory_block_index(uint32_t sigma_table, uint32_t sigma_grid, size_t i, size_t* index) {
    if (!index || sigma_table > sigma_grid || sigma_grid >= 64) return JOLT_ERR_INVALID_ARG;
    const size_t row = i >> sigma_table;
    if ((row << sigma_grid) >> sigma_grid != row) return JOLT_ERR_INVALID_ARG;
    *index = (row << sigma_grid) | (i & (((size_t)1 << sigma_table) - 1));
    return JOLT_OK;
}

// The window sums and the Horner recombination of `rows` combined rows over points that are on the device already: the plan's upload and, per pass of at most 8192
// rows, the two launches.  Enqueued on the context's stream; the temporaries go back to the pool at once (reuse is stream-ordered).  `meta` and `plan` are read by
// the copies enqueued here: the caller synchronises the stream before they go, on every path.
int32_t jolt::dory_host::combine_enqueue(jolt_ctx* ctx, const void* d_points, const std::vector<uint64_t>& meta, const CombinePlan& plan, size_t rows, void* d_out_rows) {
    const size_t n_hints = meta.size() / 2;
    const G1Jac* d_pts = (const G1Jac*)d_points;
    G1Jac* d_out = (G1Jac*)d_out_rows;
    hipStream_t st = ctx->stream;
    const size_t batch = std::min<size_t>(rows, 8192);  // window sums of one pass: 51 * 8192 points, 40 MB
    const size_t b_meta = meta.size() * 8, b_ent = std::max<size_t>(plan.ent.size(), 1) * 4, b_start = plan.start.size() * 4;
    G1Jac* d_wsum = nullptr;
    unsigned char* d_plan = nullptr;
    int32_t rc = jolt_internal_dev_alloc(ctx, (size_t)kCombineWindows * batch * sizeof(G1Jac), (void**)&d_wsum);
    if (rc == JOLT_OK) rc = jolt_internal_dev_alloc(ctx, b_meta + b_ent + b_start, (void**)&d_plan);
    hipError_t e = hipSuccess;
    if (rc == JOLT_OK) {
        e = hipMemcpyAsync(d_plan, meta.data(), b_meta, hipMemcpyHostToDevice, st);
        if (e == hipSuccess && !plan.ent.empty()) e = hipMemcpyAsync(d_plan + b_meta, plan.ent.data(), plan.ent.size() * 4, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(d_plan + b_meta + b_ent, plan.start.data(), b_start, hipMemcpyHostToDevice, st);
        const uint64_t* d_off = (const uint64_t*)d_plan;
        const uint32_t* d_ent = (const uint32_t*)(d_plan + b_meta);
        const uint32_t* d_start = (const uint32_t*)(d_plan + b_meta + b_ent);
        for (size_t r0 = 0; r0 < rows && e == hipSuccess; r0 += batch) {
            const size_t nr = std::min(batch, rows - r0);
            const unsigned g = (unsigned)((nr + kBlock - 1) / kBlock);
            hipLaunchKernelGGL(k_dory_combine_windows, dim3(g, kCombineWindows), dim3(kBlock), 0, st, d_pts, d_off, d_off + n_hints, d_ent, d_start, r0, nr, d_wsum);
            hipLaunchKernelGGL(k_dory_combine_horner, dim3(g), dim3(kBlock), 0, st, (const G1Jac*)d_wsum, nr, d_out + r0);
            e = hipGetLastError();
        }
    }
    jolt_internal_dev_free(ctx, d_wsum);
    jolt_internal_dev_free(ctx, d_plan);
    if (rc != JOLT_OK) return rc;
    if (e != hipSuccess) return hip_fail(ctx, "dory combine", e);
    return JOLT_OK;
}

extern "C" int32_t jolt_dory_combine_hints(jolt_ctx* ctx, const jolt_g1_t* const* hints, const size_t* hint_rows, size_t n_hints, const jolt_fr_t* scalars,
                                           jolt_g1_t* out) {
    if (!ctx) return JOLT_ERR_INVALID_ARG;
    JOLT_REQUIRE(ctx, n_hints != 0, "combine_hints: no hints");  // scheme.rs:326 assert
    if (!hints || !hint_rows || !scalars) return JOLT_ERR_INVALID_ARG;
    if (n_hints > (size_t)kCombineIdxMask) return JOLT_ERR_UNSUPPORTED;
    size_t rows = 0, total = 0;
    std::vector<uint64_t> meta(2 * n_hints);  // offsets, then row counts
    for (size_t i = 0; i < n_hints; ++i) {
        if (!hints[i] && hint_rows[i]) return JOLT_ERR_INVALID_ARG;
        meta[i] = total;
        meta[n_hints + i] = hint_rows[i];
        total += hint_rows[i];
        rows = std::max(rows, hint_rows[i]);
    }
    CombinePlan plan;
    JOLT_REQUIRE(ctx, combine_plan(scalars, n_hints, &plan), "scalar is not a canonical Fr");
    if (rows == 0) return JOLT_OK;
    if (!out) return JOLT_ERR_INVALID_ARG;
    dory_host::HostCall c(ctx);
    G1Jac *d_pts = nullptr, *d_out = nullptr;
    c.take(total, &d_pts);
    c.take(rows, &d_out);
    for (size_t i = 0; i < n_hints; ++i)
        if (hint_rows[i]) c.h2d(d_pts + meta[i], hints[i], hint_rows[i]);
    if (c.ok()) c.rc = dory_host::combine_enqueue(ctx, d_pts, meta, plan, rows, d_out);
    c.down(out, d_out, rows);
    return c.finish("dory combine");  // the plan and the caller's arrays are read until here
}

// The per-row routine of k_dory_combine_windows / k_dory_combine_horner on the host: out = sum_i scalars[i] * points[i], through the same plan, window walk and Horner
// recombination, so that the suite pins them against the oracle without a GPU.
extern "C" int32_t jolt_host_dory_combine_row(const jolt_g1_t* points, const jolt_fr_t* scalars, size_t n, jolt_g1_t* out) {
    if (!out || (n && (!points || !scalars)) || n > (size_t)kCombineIdxMask) return JOLT_ERR_INVALID_ARG;
    CombinePlan plan;
    if (!combine_plan(scalars, n, &plan)) return JOLT_ERR_INVALID_ARG;
    const G1Jac acc = combine_horner([&](int w) {
        return combine_window(plan.ent.data() + plan.start[w], plan.start[w + 1] - plan.start[w], [&](uint32_t i) {
            G1Jac p;
            std::memcpy(&p, &points[i], sizeof(p));
            return p;
        });
    });
    const G1Jac r = g1_is_identity(acc) ? g1_identity() : acc;
    std::memcpy(out, &r, sizeof(r));
    return JOLT_OK;
}
