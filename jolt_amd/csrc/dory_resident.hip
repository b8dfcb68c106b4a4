// jolt_amd/csrc/dory_resident.hip -- Dory's reduce-and-fold rounds on vectors that stay in HBM, the products of one prover message as one launch set.
//
// The host-pointer entry points (dory_routines.hip, dory_pairing.hip) run one routine per call: upload, one kernel chain alone on the chip, synchronise, download.
// Every one of those chains is latency bound -- ~254 dependent doublings per lane, or 88 dependent line steps -- and at one wavefront per workgroup 2^15 lanes do not
// even give each of the 1024 SIMDs a wavefront, so six products in a row cost six chain latencies on a nearly empty chip.  Here
//   jolt_dory_vec            a G1 / G2 / Fr array from the context's pool; its elements are checked once, at upload
//   jolt_dory_vec_scale_*    the shared-scalar routines and the field fold in place on views: k_dory_scale_add / k_dory_fold_field of dory_kernels.hip.h, enqueued only
//   jolt_dory_products       a batch of multi-pairings and MSMs over views.  Per chain (pairings, G1 sums, G2 sums) the items are packed by dory_batch_plan.hpp:
//     k_batch_prepare_g2     one launch over the distinct G2 views of the batch: g2_prepare_walk per lane into ONE step-major scratch table
//     k_batch_miller         one launch over all pairs of all PAIR items: miller_walk per lane against the scratch table or a range of a jolt_g2_prepared
//     k_batch_msm_terms      one launch per group over all MSM items of that group: term_mul_one per lane
//     k_batch_tree_level     one launch per LEVEL over all items of a chain: f[i] *= f[i + half] / terms[i] += terms[i + half] inside each item's segment, with that
//                            segment's own m -- the step of k_tree_level (dory_kernels.hip.h), under the same operations
//     k_batch_gather         each item's element 0 (or the neutral element of an empty item) into one result block: one read-back for the batch
//   jolt_dory_state_alloc / _from_table / _combine_hints / _fixed_base_mul   the state an opening's rounds start from, built where it is used: neutral vectors
//                            (k_dory_fill), entries of an Fr table (a device copy), the combined hints (the plan and the two kernels of dory.hip's combine_hints, on
//                            the hints gathered back to back by device copies), multiples of one base (k_dory_fixed_base of dory_kernels.hip.h)
//   The three chains are independent: they run on the context's side streams, forked from the main stream by one event and joined before the read-back (Fork of
//   dory_host.hpp).  Single launches go through the launch layer of dory_kernels.hip.h / dory_prepared.hip.h; an entry that reads host memory is one HostCall.
// Workgroups of one wavefront, one element per lane, integer VALU work, no MFMA, as the kernels these are made of; register figures in docs/kernels.md 3.5h.
#include <algorithm>
#include <thread>
#include <vector>

#include "ctx.hpp"
#include "dory_batch_plan.hpp"
#include "dory_host.hpp"
#include "dory_kernels.hip.h"
#include "dory_prepared.hip.h"
#include "pairing.hip.h"

using namespace jolt;
using namespace jolt::dory_host;
using namespace jolt::dory_dev;
using namespace jolt::dory_plan;

static_assert(kPlanLanes == (size_t)kLanes, "the plan pads to the kernels' wavefront");
static_assert(sizeof(jolt_dory_result) >= sizeof(Fq12) && sizeof(jolt_gt_t) == sizeof(Fq12), "result block");

namespace {

size_t kind_size(int32_t kind) { return kind == JOLT_DORY_KIND_G1 ? sizeof(G1Jac) : kind == JOLT_DORY_KIND_G2 ? sizeof(G2Jac) : sizeof(Fr); }

// two valid views of different lengths share an element
bool ranges_overlap(const jolt_dory_vec* a, size_t a_first, size_t a_n, const jolt_dory_vec* b, size_t b_first, size_t b_n) {
    if (a != b || a_n == 0 || b_n == 0) return false;
    return a_first < b_first ? b_first - a_first < a_n : a_first - b_first < b_n;
}
template <class T>
T* at(const jolt_dory_vec* v, size_t first) { return (T*)v->data + first; }

// a vector of n elements whose block is not written yet
int32_t vec_new(jolt_ctx* ctx, int32_t kind, size_t n, jolt_dory_vec** out) {
    jolt_dory_vec* v = new (std::nothrow) jolt_dory_vec();
    if (!v) return JOLT_ERR_OOM;
    v->ctx = ctx;
    v->kind = kind;
    v->len = n;
    const int32_t rc = jolt_internal_dev_alloc(ctx, std::max<size_t>(n * kind_size(kind), 16), &v->data);
    if (rc != JOLT_OK) {
        delete v;
        return rc;
    }
    *out = v;
    return JOLT_OK;
}

template <class T>
__global__ __launch_bounds__(kLanes) void k_dory_fill(T* __restrict__ out, size_t n, T value) {
    const size_t i = (size_t)blockIdx.x * kLanes + threadIdx.x;
    if (i < n) out[i] = value;
}
template <class T>
hipError_t fill(hipStream_t st, jolt_dory_vec* v, const T& value) {
    hipLaunchKernelGGL(k_dory_fill<T>, dim3(lanes_grid(v->len)), dim3(kLanes), 0, st, (T*)v->data, v->len, value);
    return hipGetLastError();
}

// ---- the tables of a batch: per workgroup (item, first), per item its pointers, its first slot in the chain's packed array and its length ----
struct WgDev {
    uint32_t item, first;
};
struct SegDev {
    size_t base, len;
};
struct PrepDev {
    const G2Jac* pts;
    size_t base, len;  // base: the range's first column of the scratch line table
};
struct PairDev {
    const G1Jac* g1;
    const PairLine* lines;  // column of the item's first pair
    const uint8_t* skip;
    size_t stride, base, len;
};
template <class Pt>
struct MsmDev {
    const Pt* pts;
    const Fr* scalars;
    size_t base, len;
};

__global__ __launch_bounds__(kLanes) void k_batch_prepare_g2(const WgDev* __restrict__ wgs, const PrepDev* __restrict__ ranges, PairLine* __restrict__ lines, uint8_t* __restrict__ skip, size_t stride) {
    const WgDev w = wgs[blockIdx.x];
    const PrepDev r = ranges[w.item];
    const size_t i = (size_t)w.first + threadIdx.x;
    if (i >= r.len) return;
    const size_t col = r.base + i;
    skip[col] = g2_prepare_walk(r.pts[i], PairLineTable{lines + col, stride}) ? 1 : 0;
}
__global__ __launch_bounds__(kLanes) void k_batch_miller(const WgDev* __restrict__ wgs, const PairDev* __restrict__ items, Fq12* __restrict__ f) {
    const WgDev w = wgs[blockIdx.x];
    const PairDev it = items[w.item];
    const size_t i = (size_t)w.first + threadIdx.x;
    if (i >= it.len) return;
    f[it.base + i] = miller_walk(it.g1[i], PairLineTable{const_cast<PairLine*>(it.lines) + i, it.stride}, it.skip[i] != 0);
}
template <class O>
__global__ __launch_bounds__(kLanes) void k_batch_msm_terms(const WgDev* __restrict__ wgs, const MsmDev<typename O::Pt>* __restrict__ items, typename O::Pt* __restrict__ terms) {
    const WgDev w = wgs[blockIdx.x];
    const MsmDev<typename O::Pt> it = items[w.item];
    const size_t i = (size_t)w.first + threadIdx.x;
    if (i >= it.len) return;
    terms[it.base + i] = term_mul_one<O>(it.pts[i], it.scalars[i]);
}
// level `level` of every item's tree at once: the segment holds m = len halved `level` times elements, v[i] = v[i] (x) v[i + half] for i + half < m -- the step of
// k_tree_level, under the same Op (MulFq12, AddPt<O>)
template <class T, class Op>
__global__ __launch_bounds__(kLanes) void k_batch_tree_level(const WgDev* __restrict__ wgs, const SegDev* __restrict__ segs, T* v, uint32_t level) {
    const WgDev w = wgs[blockIdx.x];
    const SegDev s = segs[w.item];
    size_t m = s.len;
    for (uint32_t l = 0; l < level; ++l) m = (m + 1) / 2;
    const size_t half = (m + 1) / 2;
    const size_t i = (size_t)w.first + threadIdx.x;
    if (m <= 1 || i >= half || i + half >= m) return;
    T* seg = v + s.base;
    seg[i] = Op::combine(seg[i], seg[i + half]);
}
template <class T>
__global__ __launch_bounds__(kLanes) void k_batch_gather(const SegDev* __restrict__ segs, const T* __restrict__ v, T* __restrict__ out, size_t n_items, T empty) {
    const size_t k = (size_t)blockIdx.x * kLanes + threadIdx.x;
    if (k >= n_items) return;
    out[k] = segs[k].len ? v[segs[k].base] : empty;
}

// one host block for every table of a batch: one upload
struct Blob {
    std::vector<uint8_t> bytes;
    template <class T>
    size_t put(const std::vector<T>& a) {
        const size_t off = (bytes.size() + 15) / 16 * 16;
        bytes.resize(off + a.size() * sizeof(T));
        if (!a.empty()) std::memcpy(bytes.data() + off, a.data(), a.size() * sizeof(T));
        return off;
    }
};
std::vector<WgDev> wg_table(const BatchPlan& p) {
    std::vector<WgDev> t(p.wg_item.size());
    for (size_t w = 0; w < t.size(); ++w) t[w] = WgDev{p.wg_item[w], p.wg_first[w]};
    return t;
}

// one chain's reduction and its result block, on `st`
template <class T, class Op>
hipError_t reduce_chain(hipStream_t st, const BatchPlan& plan, const WgDev* d_wgs, const SegDev* d_segs, T* d_v, T* d_out, const T& empty) {
    const size_t n_items = plan.item_base.size();
    if (!plan.wg_item.empty())
        for (uint32_t level = 0; level < plan.levels; ++level) hipLaunchKernelGGL((k_batch_tree_level<T, Op>), dim3((unsigned)plan.wg_item.size()), dim3(kLanes), 0, st, d_wgs, d_segs, d_v, level);
    hipLaunchKernelGGL(k_batch_gather<T>, dim3(lanes_grid(n_items)), dim3(kLanes), 0, st, d_segs, (const T*)d_v, d_out, n_items, empty);
    return hipGetLastError();
}

template <class O>
int32_t scale_add_views(jolt_ctx* ctx, jolt_dory_vec* vs, size_t vs_first, const jolt_dory_vec* other, size_t other_first, size_t n, const NafPlan& plan, bool scale_vs, const char* what) {
    using Pt = typename O::Pt;
    if (n == 0) return JOLT_OK;
    Pt* d_vs = at<Pt>(vs, vs_first);
    const Pt* d_other = at<Pt>(other, other_first);
    const hipError_t e = enqueue_scale_add<O>(ctx->stream, plan, scale_vs ? d_vs : d_other, scale_vs ? d_other : d_vs, d_vs, n);
    return e == hipSuccess ? JOLT_OK : hip_fail(ctx, what, e);
}
int32_t scale_add_entry(jolt_ctx* ctx, jolt_dory_vec* vs, size_t vs_first, const jolt_dory_vec* other, size_t other_first, size_t n, const jolt_fr_t* scalar, bool scale_vs, const char* what) {
    if (!ctx || !vs || !other || !scalar) return JOLT_ERR_INVALID_ARG;
    JOLT_REQUIRE(ctx, vs->kind == JOLT_DORY_KIND_G1 || vs->kind == JOLT_DORY_KIND_G2, "the vectors of a shared-scalar routine hold points");
    JOLT_REQUIRE(ctx, view_ok(ctx, vs, vs->kind, vs_first, n) && view_ok(ctx, other, vs->kind, other_first, n), "a view is outside its vector, or of another kind or context");
    JOLT_REQUIRE(ctx, !views_overlap(vs, vs_first, other, other_first, n), "the two views overlap");
    NafPlan plan;
    JOLT_REQUIRE(ctx, naf_plan(scalar, &plan), "scalar is not a canonical Fr");
    return vs->kind == JOLT_DORY_KIND_G1 ? scale_add_views<G1Ops>(ctx, vs, vs_first, other, other_first, n, plan, scale_vs, what)
                                         : scale_add_views<G2Ops>(ctx, vs, vs_first, other, other_first, n, plan, scale_vs, what);
}

constexpr size_t kMaxItems = 4096;

}  // namespace

void* jolt::dory_host::g1_view(const jolt_ctx* ctx, const jolt_dory_vec* vec, size_t first, size_t n) {
    return view_ok(ctx, vec, JOLT_DORY_KIND_G1, first, n) ? (void*)at<G1Jac>(vec, first) : nullptr;
}

extern "C" int32_t jolt_dory_vec_upload(jolt_ctx* ctx, int32_t kind, const void* host, size_t n, jolt_dory_vec** out) {
    if (!ctx || !out || (n && !host)) return JOLT_ERR_INVALID_ARG;
    JOLT_REQUIRE(ctx, kind == JOLT_DORY_KIND_G1 || kind == JOLT_DORY_KIND_G2 || kind == JOLT_DORY_KIND_FR, "unknown vector kind");
    if (n > kMaxElements) return JOLT_ERR_UNSUPPORTED;
    if (kind == JOLT_DORY_KIND_FR) {
        const jolt_fr_t* s = (const jolt_fr_t*)host;
        JOLT_REQUIRE(ctx, parallel_all(n, [s](size_t lo, size_t hi) { return all_canonical(s + lo, hi - lo); }), "scalar is not a canonical Fr");
    } else {
        const bool ok = kind == JOLT_DORY_KIND_G1 ? all_on_curve<G1Ops>((const jolt_g1_t*)host, n) : all_on_curve<G2Ops>((const jolt_g2_t*)host, n);
        JOLT_REQUIRE(ctx, ok, "a point is not on its curve or not canonical");
    }
    jolt_dory_vec* v = nullptr;
    JOLT_TRY(vec_new(ctx, kind, n, &v));
    int32_t rc = JOLT_OK;
    if (n) {
        HostCall c(ctx);
        c.h2d((uint8_t*)v->data, host, n * kind_size(kind));
        rc = c.finish("dory vec upload");
    }
    if (rc != JOLT_OK) {
        (void)jolt_dory_vec_free(ctx, v);
        return rc;
    }
    *out = v;
    return JOLT_OK;
}

extern "C" int32_t jolt_dory_vec_download(jolt_ctx* ctx, const jolt_dory_vec* vec, size_t first, size_t n, void* host) {
    if (!ctx || !vec || (n && !host)) return JOLT_ERR_INVALID_ARG;
    JOLT_REQUIRE(ctx, view_ok(ctx, vec, vec->kind, first, n), "the view is outside its vector, or the vector belongs to another context");
    if (n == 0) return JOLT_OK;
    const size_t sz = kind_size(vec->kind);
    HostCall c(ctx);
    c.down(host, (const uint8_t*)vec->data + first * sz, n * sz);
    return c.finish("dory vec download");
}

extern "C" int32_t jolt_dory_vec_len(const jolt_dory_vec* vec, size_t* len) {
    if (!vec || !len) return JOLT_ERR_INVALID_ARG;
    *len = vec->len;
    return JOLT_OK;
}
extern "C" int32_t jolt_dory_vec_kind(const jolt_dory_vec* vec, int32_t* kind) {
    if (!vec || !kind) return JOLT_ERR_INVALID_ARG;
    *kind = vec->kind;
    return JOLT_OK;
}
extern "C" int32_t jolt_dory_vec_free(jolt_ctx* ctx, jolt_dory_vec* vec) {
    if (!ctx) return JOLT_ERR_INVALID_ARG;
    if (!vec) return JOLT_OK;
    if (vec->data) jolt_internal_dev_free(ctx, vec->data);  // reuse of the block is ordered by the main stream, which every chain of a batch joins
    delete vec;
    return JOLT_OK;
}
extern "C" int32_t jolt_dory_vec_truncate(jolt_dory_vec* vec, size_t n) {
    if (!vec || n > vec->len) return JOLT_ERR_INVALID_ARG;
    vec->len = n;
    return JOLT_OK;
}

extern "C" int32_t jolt_dory_g2_prepare_vec(jolt_ctx* ctx, const jolt_dory_vec* vec, size_t first, size_t n, jolt_g2_prepared** out) {
    if (!ctx || !vec || !out) return JOLT_ERR_INVALID_ARG;
    JOLT_REQUIRE(ctx, view_ok(ctx, vec, JOLT_DORY_KIND_G2, first, n), "the view is outside its vector, or not a G2 vector of this context");
    if (n > kMaxPacked) return JOLT_ERR_UNSUPPORTED;
    jolt_g2_prepared* p = new (std::nothrow) jolt_g2_prepared();
    if (!p) return JOLT_ERR_OOM;
    p->ctx = ctx;
    p->n = n;
    int32_t rc = JOLT_OK;
    if (n) {
        rc = jolt_internal_dev_alloc(ctx, n * kPairingLines * sizeof(PairLine), (void**)&p->lines);
        if (rc == JOLT_OK) rc = jolt_internal_dev_alloc(ctx, n, (void**)&p->skip);
        if (rc == JOLT_OK) {
            const hipError_t e = launch_prepare(ctx->stream, at<G2Jac>(vec, first), p->lines, p->skip, n);
            if (e != hipSuccess) rc = hip_fail(ctx, "dory g2 prepare vec", e);
        }
    }
    if (rc != JOLT_OK) {
        (void)jolt_g2_prepared_free(ctx, p);
        return rc;
    }
    *out = p;
    return JOLT_OK;
}

extern "C" int32_t jolt_dory_vec_scale_bases_add(jolt_ctx* ctx, const jolt_dory_vec* bases, size_t bases_first, jolt_dory_vec* vs, size_t vs_first, size_t n, const jolt_fr_t* scalar) {
    return scale_add_entry(ctx, vs, vs_first, bases, bases_first, n, scalar, false, "dory vec scale bases");
}
extern "C" int32_t jolt_dory_vec_scale_vs_add(jolt_ctx* ctx, jolt_dory_vec* vs, size_t vs_first, const jolt_dory_vec* addends, size_t addends_first, size_t n, const jolt_fr_t* scalar) {
    return scale_add_entry(ctx, vs, vs_first, addends, addends_first, n, scalar, true, "dory vec scale vs");
}
extern "C" int32_t jolt_dory_vec_fold_field(jolt_ctx* ctx, jolt_dory_vec* left, size_t left_first, const jolt_dory_vec* right, size_t right_first, size_t n, const jolt_fr_t* scalar) {
    if (!ctx || !left || !right || !scalar) return JOLT_ERR_INVALID_ARG;
    JOLT_REQUIRE(ctx, view_ok(ctx, left, JOLT_DORY_KIND_FR, left_first, n) && view_ok(ctx, right, JOLT_DORY_KIND_FR, right_first, n), "a view is outside its vector, or not an Fr vector of this context");
    JOLT_REQUIRE(ctx, !views_overlap(left, left_first, right, right_first, n), "the two views overlap");
    const Fr s = fr_from_abi(scalar);
    JOLT_REQUIRE(ctx, fr_is_canonical(s), "scalar is not a canonical Fr");
    if (n == 0) return JOLT_OK;
    const hipError_t e = enqueue_fold_field(ctx->stream, at<Fr>(left, left_first), at<Fr>(right, right_first), s, n);
    return e == hipSuccess ? JOLT_OK : hip_fail(ctx, "dory vec field fold", e);
}

extern "C" int32_t jolt_dory_state_alloc(jolt_ctx* ctx, int32_t kind, size_t n, jolt_dory_vec** out) {
    if (!ctx || !out) return JOLT_ERR_INVALID_ARG;
    JOLT_REQUIRE(ctx, kind == JOLT_DORY_KIND_G1 || kind == JOLT_DORY_KIND_G2 || kind == JOLT_DORY_KIND_FR, "unknown vector kind");
    if (n > kMaxElements) return JOLT_ERR_UNSUPPORTED;
    jolt_dory_vec* v = nullptr;
    JOLT_TRY(vec_new(ctx, kind, n, &v));
    if (n) {
        const hipError_t e = kind == JOLT_DORY_KIND_G1 ? fill(ctx->stream, v, G1Ops::identity()) : kind == JOLT_DORY_KIND_G2 ? fill(ctx->stream, v, G2Ops::identity()) : fill(ctx->stream, v, Fr::zero());
        if (e != hipSuccess) {
            (void)jolt_dory_vec_free(ctx, v);
            return hip_fail(ctx, "dory state alloc", e);
        }
    }
    *out = v;
    return JOLT_OK;
}

extern "C" int32_t jolt_dory_state_from_table(jolt_ctx* ctx, const jolt_table* table, size_t table_first, jolt_dory_vec* dst, size_t dst_first, size_t n) {
    if (!ctx || !table || !dst) return JOLT_ERR_INVALID_ARG;
    JOLT_REQUIRE(ctx, table->ctx == ctx && table->data() && !(table_first > table->len || n > table->len - table_first), "the range is outside the table, or the table belongs to another context");
    JOLT_REQUIRE(ctx, view_ok(ctx, dst, JOLT_DORY_KIND_FR, dst_first, n), "the view is outside its vector, or not an Fr vector of this context");
    if (n == 0) return JOLT_OK;
    const hipError_t e = hipMemcpyAsync(at<Fr>(dst, dst_first), table->data() + table_first, n * sizeof(Fr), hipMemcpyDeviceToDevice, ctx->stream);
    return e == hipSuccess ? JOLT_OK : hip_fail(ctx, "dory state from table", e);
}

extern "C" int32_t jolt_dory_state_combine_hints(jolt_ctx* ctx, const jolt_dory_vec* const* hints, const size_t* hint_first, const size_t* hint_rows, size_t n_hints, const jolt_fr_t* scalars,
                                               jolt_dory_vec* out, size_t out_first) {
    if (!ctx) return JOLT_ERR_INVALID_ARG;
    JOLT_REQUIRE(ctx, n_hints != 0, "combine_hints: no hints");  // scheme.rs:326 assert
    if (!hints || !hint_first || !hint_rows || !scalars || !out) return JOLT_ERR_INVALID_ARG;
    if (n_hints > (size_t)0x00FFFFFFu) return JOLT_ERR_UNSUPPORTED;  // a plan entry holds the term in 24 bits
    size_t rows = 0, total = 0;
    std::vector<uint64_t> meta(2 * n_hints);  // offsets into the gathered points, then row counts
    for (size_t i = 0; i < n_hints; ++i) {
        JOLT_REQUIRE(ctx, view_ok(ctx, hints[i], JOLT_DORY_KIND_G1, hint_first[i], hint_rows[i]), "a hint is not a G1 view of this context");
        meta[i] = total;
        meta[n_hints + i] = hint_rows[i];
        total += hint_rows[i];
        rows = std::max(rows, hint_rows[i]);
    }
    JOLT_REQUIRE(ctx, view_ok(ctx, out, JOLT_DORY_KIND_G1, out_first, rows), "out is not a G1 view of this context that holds the combined rows");
    for (size_t i = 0; i < n_hints; ++i) JOLT_REQUIRE(ctx, !ranges_overlap(out, out_first, rows, hints[i], hint_first[i], hint_rows[i]), "out overlaps a hint");
    CombinePlan plan;
    JOLT_REQUIRE(ctx, combine_plan(scalars, n_hints, &plan), "scalar is not a canonical Fr");
    if (rows == 0) return JOLT_OK;
    HostCall c(ctx);
    G1Jac* d_pts = nullptr;
    c.take(total, &d_pts);
    for (size_t i = 0; i < n_hints && c.ok(); ++i)  // back to back, the layout k_dory_combine_windows indexes
        if (hint_rows[i]) c.e = hipMemcpyAsync(d_pts + meta[i], at<G1Jac>(hints[i], hint_first[i]), hint_rows[i] * sizeof(G1Jac), hipMemcpyDeviceToDevice, c.st);
    if (c.ok()) c.rc = combine_enqueue(ctx, d_pts, meta, plan, rows, at<G1Jac>(out, out_first));
    return c.finish("dory state combine");  // the plan (host memory of this call) is read until here
}

namespace {
template <class O>
int32_t fixed_base_views(jolt_ctx* ctx, const void* base, const jolt_dory_vec* scalars, size_t scalars_first, jolt_dory_vec* out, size_t out_first, size_t n) {
    using Pt = typename O::Pt;
    JOLT_REQUIRE(ctx, all_on_curve<O>((const typename O::Abi*)base, 1), "a point is not on its curve or not canonical");
    if (n == 0) return JOLT_OK;
    Pt table[kFixedTable];  // read by its upload until finish()
    fixed_table_from_abi<O>(base, table);
    HostCall c(ctx);
    Pt* d_table = nullptr;
    c.up(table, kFixedTable, &d_table);
    if (c.ok()) c.e = enqueue_fixed_base<O>(c.st, d_table, at<Fr>(scalars, scalars_first), at<Pt>(out, out_first), n);
    return c.finish("dory state fixed base");
}
}  // namespace

extern "C" int32_t jolt_dory_state_fixed_base_mul(jolt_ctx* ctx, int32_t kind, const void* base, const jolt_dory_vec* scalars, size_t scalars_first, jolt_dory_vec* out, size_t out_first, size_t n) {
    if (!ctx || !base || !scalars || !out) return JOLT_ERR_INVALID_ARG;
    JOLT_REQUIRE(ctx, kind == JOLT_DORY_KIND_G1 || kind == JOLT_DORY_KIND_G2, "a fixed-base multiplication gives points");
    JOLT_REQUIRE(ctx, view_ok(ctx, scalars, JOLT_DORY_KIND_FR, scalars_first, n) && view_ok(ctx, out, kind, out_first, n), "a view is outside its vector, or of another kind or context");
    return kind == JOLT_DORY_KIND_G1 ? fixed_base_views<G1Ops>(ctx, base, scalars, scalars_first, out, out_first, n) : fixed_base_views<G2Ops>(ctx, base, scalars, scalars_first, out, out_first, n);
}

extern "C" int32_t jolt_dory_products(jolt_ctx* ctx, const jolt_dory_item* items, size_t n_items, jolt_dory_result* outs) {
    if (!ctx || (n_items && (!items || !outs))) return JOLT_ERR_INVALID_ARG;
    if (n_items > kMaxItems) return JOLT_ERR_UNSUPPORTED;
    // ---- every check before anything is enqueued ----
    std::vector<size_t> pair_ids, g1_ids, g2_ids;
    for (size_t k = 0; k < n_items; ++k) {
        const jolt_dory_item& it = items[k];
        switch (it.op) {
            case JOLT_DORY_PAIR:
                JOLT_REQUIRE(ctx, view_ok(ctx, it.a, JOLT_DORY_KIND_G1, it.a_first, it.n), "PAIR: a is not a G1 view of this context");
                if (it.b) {
                    JOLT_REQUIRE(ctx, !it.prepared, "PAIR: both a G2 view and a prepared table");
                    JOLT_REQUIRE(ctx, view_ok(ctx, it.b, JOLT_DORY_KIND_G2, it.b_first, it.n), "PAIR: b is not a G2 view of this context");
                } else {
                    JOLT_REQUIRE(ctx, it.prepared && it.prepared->ctx == ctx, "PAIR: neither a G2 view nor a prepared table of this context");
                    JOLT_REQUIRE(ctx, !(it.prepared_first > it.prepared->n || it.n > it.prepared->n - it.prepared_first), "PAIR: the range is past the prepared table");
                }
                pair_ids.push_back(k);
                break;
            case JOLT_DORY_MSM_G1:
            case JOLT_DORY_MSM_G2:
                JOLT_REQUIRE(ctx, !it.prepared, "MSM: a prepared table");
                JOLT_REQUIRE(ctx, view_ok(ctx, it.a, it.op == JOLT_DORY_MSM_G1 ? JOLT_DORY_KIND_G1 : JOLT_DORY_KIND_G2, it.a_first, it.n), "MSM: a is not a point view of the item's group");
                JOLT_REQUIRE(ctx, view_ok(ctx, it.b, JOLT_DORY_KIND_FR, it.b_first, it.n), "MSM: b is not an Fr view of this context");
                (it.op == JOLT_DORY_MSM_G1 ? g1_ids : g2_ids).push_back(k);
                break;
            default:
                JOLT_REQUIRE(ctx, false, "unknown item op");
        }
    }
    if (n_items == 0) return JOLT_OK;

    // ---- the plans: distinct G2 views (a range shared by items is prepared once), then the three chains ----
    struct Range {
        const jolt_dory_vec* vec;
        size_t first, n;
    };
    std::vector<Range> ranges;
    std::vector<size_t> pair_range(pair_ids.size(), 0);
    for (size_t j = 0; j < pair_ids.size(); ++j) {
        const jolt_dory_item& it = items[pair_ids[j]];
        if (!it.b || it.n == 0) continue;
        size_t u = 0;
        while (u < ranges.size() && !(ranges[u].vec == it.b && ranges[u].first == it.b_first && ranges[u].n == it.n)) ++u;
        if (u == ranges.size()) ranges.push_back(Range{it.b, it.b_first, it.n});
        pair_range[j] = u;
    }
    auto lens_of = [items](const std::vector<size_t>& ids) {
        std::vector<size_t> lens(ids.size());
        for (size_t j = 0; j < ids.size(); ++j) lens[j] = items[ids[j]].n;
        return lens;
    };
    std::vector<size_t> range_lens(ranges.size());
    for (size_t u = 0; u < ranges.size(); ++u) range_lens[u] = ranges[u].n;
    const std::vector<size_t> pair_lens = lens_of(pair_ids), g1_lens = lens_of(g1_ids), g2_lens = lens_of(g2_ids);
    BatchPlan prep_plan, pair_plan, g1_plan, g2_plan;
    if (!batch_plan(range_lens.data(), range_lens.size(), &prep_plan) || !batch_plan(pair_lens.data(), pair_lens.size(), &pair_plan) ||
        !batch_plan(g1_lens.data(), g1_lens.size(), &g1_plan) || !batch_plan(g2_lens.data(), g2_lens.size(), &g2_plan))
        return JOLT_ERR_UNSUPPORTED;

    HostCall c(ctx);
    PairLine* d_lines = nullptr;
    uint8_t *d_skip = nullptr, *d_blob = nullptr, *d_res = nullptr;
    Fq12* d_f = nullptr;
    G1Jac* d_t1 = nullptr;
    G2Jac* d_t2 = nullptr;
    const size_t stride = prep_plan.packed;
    JOLT_TRY(c.bufs.take(stride * kPairingLines, &d_lines));
    JOLT_TRY(c.bufs.take(stride, &d_skip));
    JOLT_TRY(c.bufs.take(pair_plan.packed, &d_f));
    JOLT_TRY(c.bufs.take(g1_plan.packed, &d_t1));
    JOLT_TRY(c.bufs.take(g2_plan.packed, &d_t2));
    const size_t res_gt = 0, res_g1 = res_gt + pair_ids.size() * sizeof(Fq12), res_g2 = res_g1 + g1_ids.size() * sizeof(G1Jac), res_bytes = res_g2 + g2_ids.size() * sizeof(G2Jac);
    JOLT_TRY(c.bufs.take(res_bytes, &d_res));

    // ---- the tables, one block ----
    std::vector<PrepDev> prep_items(ranges.size());
    for (size_t u = 0; u < ranges.size(); ++u) prep_items[u] = PrepDev{at<G2Jac>(ranges[u].vec, ranges[u].first), prep_plan.item_base[u], ranges[u].n};
    std::vector<PairDev> pair_items(pair_ids.size());
    std::vector<SegDev> pair_segs(pair_ids.size()), g1_segs(g1_ids.size()), g2_segs(g2_ids.size());
    for (size_t j = 0; j < pair_ids.size(); ++j) {
        const jolt_dory_item& it = items[pair_ids[j]];
        PairDev d = {at<G1Jac>(it.a, it.a_first), nullptr, nullptr, 0, pair_plan.item_base[j], it.n};
        if (it.b) {
            const size_t col = it.n ? prep_plan.item_base[pair_range[j]] : 0;
            d.lines = d_lines + col;
            d.skip = d_skip + col;
            d.stride = stride;
        } else {
            d.lines = it.prepared->lines + it.prepared_first;
            d.skip = it.prepared->skip + it.prepared_first;
            d.stride = it.prepared->n;
        }
        pair_items[j] = d;
        pair_segs[j] = SegDev{d.base, d.len};
    }
    std::vector<MsmDev<G1Jac>> g1_items(g1_ids.size());
    for (size_t j = 0; j < g1_ids.size(); ++j) {
        const jolt_dory_item& it = items[g1_ids[j]];
        g1_items[j] = MsmDev<G1Jac>{at<G1Jac>(it.a, it.a_first), at<Fr>(it.b, it.b_first), g1_plan.item_base[j], it.n};
        g1_segs[j] = SegDev{g1_plan.item_base[j], it.n};
    }
    std::vector<MsmDev<G2Jac>> g2_items(g2_ids.size());
    for (size_t j = 0; j < g2_ids.size(); ++j) {
        const jolt_dory_item& it = items[g2_ids[j]];
        g2_items[j] = MsmDev<G2Jac>{at<G2Jac>(it.a, it.a_first), at<Fr>(it.b, it.b_first), g2_plan.item_base[j], it.n};
        g2_segs[j] = SegDev{g2_plan.item_base[j], it.n};
    }
    Blob blob;
    const size_t o_prep_wg = blob.put(wg_table(prep_plan)), o_pair_wg = blob.put(wg_table(pair_plan)), o_g1_wg = blob.put(wg_table(g1_plan)), o_g2_wg = blob.put(wg_table(g2_plan));
    const size_t o_prep = blob.put(prep_items), o_pair = blob.put(pair_items), o_g1 = blob.put(g1_items), o_g2 = blob.put(g2_items);
    const size_t o_pair_seg = blob.put(pair_segs), o_g1_seg = blob.put(g1_segs), o_g2_seg = blob.put(g2_segs);
    JOLT_TRY(c.bufs.take(blob.bytes.size(), &d_blob));

    // ---- enqueue: tables on the main stream, fork, the three chains, join, one read-back ----
    std::vector<uint8_t> res(res_bytes);
    c.h2d(d_blob, blob.bytes.data(), blob.bytes.size());
    Fork fork(ctx, 3);
    hipError_t e = c.ok() ? fork.e : c.e;
    if (e == hipSuccess && !pair_ids.empty()) {
        hipStream_t st = fork.st[0];
        const WgDev* wgs = (const WgDev*)(d_blob + o_pair_wg);
        if (!prep_plan.wg_item.empty())
            hipLaunchKernelGGL(k_batch_prepare_g2, dim3((unsigned)prep_plan.wg_item.size()), dim3(kLanes), 0, st, (const WgDev*)(d_blob + o_prep_wg), (const PrepDev*)(d_blob + o_prep), d_lines, d_skip, stride);
        if (!pair_plan.wg_item.empty())
            hipLaunchKernelGGL(k_batch_miller, dim3((unsigned)pair_plan.wg_item.size()), dim3(kLanes), 0, st, wgs, (const PairDev*)(d_blob + o_pair), d_f);
        e = reduce_chain<Fq12, MulFq12>(st, pair_plan, wgs, (const SegDev*)(d_blob + o_pair_seg), d_f, (Fq12*)(d_res + res_gt), Fq12::one());
    }
    if (e == hipSuccess && !g1_ids.empty()) {
        hipStream_t st = fork.st[1];
        const WgDev* wgs = (const WgDev*)(d_blob + o_g1_wg);
        if (!g1_plan.wg_item.empty())
            hipLaunchKernelGGL(k_batch_msm_terms<G1Ops>, dim3((unsigned)g1_plan.wg_item.size()), dim3(kLanes), 0, st, wgs, (const MsmDev<G1Jac>*)(d_blob + o_g1), d_t1);
        e = reduce_chain<G1Jac, AddPt<G1Ops>>(st, g1_plan, wgs, (const SegDev*)(d_blob + o_g1_seg), d_t1, (G1Jac*)(d_res + res_g1), G1Ops::identity());
    }
    if (e == hipSuccess && !g2_ids.empty()) {
        hipStream_t st = fork.st[2];
        const WgDev* wgs = (const WgDev*)(d_blob + o_g2_wg);
        if (!g2_plan.wg_item.empty())
            hipLaunchKernelGGL(k_batch_msm_terms<G2Ops>, dim3((unsigned)g2_plan.wg_item.size()), dim3(kLanes), 0, st, wgs, (const MsmDev<G2Jac>*)(d_blob + o_g2), d_t2);
        e = reduce_chain<G2Jac, AddPt<G2Ops>>(st, g2_plan, wgs, (const SegDev*)(d_blob + o_g2_seg), d_t2, (G2Jac*)(d_res + res_g2), G2Ops::identity());
    }
    c.e = fork.join(e);
    c.down(res.data(), d_res, res_bytes);
    JOLT_TRY(c.finish("dory products"));  // the tables of this call are read until here

    // ---- one final exponentiation per PAIR item, beside each other on the host ----
    std::vector<Fq12> gt(pair_ids.size());
    auto finish_range = [&](size_t lo, size_t hi) {
        for (size_t j = lo; j < hi; ++j) {
            Fq12 raw;
            std::memcpy(&raw, res.data() + res_gt + j * sizeof(Fq12), sizeof(raw));
            gt[j] = final_exponentiation(raw);
        }
    };
    {
        const size_t parts = std::min<size_t>(pair_ids.size(), 16);
        std::vector<std::thread> workers;
        size_t started = 0;
        try {
            for (; started + 1 < parts; ++started) workers.emplace_back(finish_range, pair_ids.size() * started / parts, pair_ids.size() * (started + 1) / parts);
        } catch (...) {  // no more threads to be had: the calling thread takes the rest
        }
        if (parts) finish_range(pair_ids.size() * started / parts, pair_ids.size());
        for (std::thread& w : workers) w.join();
    }
    for (size_t j = 0; j < pair_ids.size(); ++j) std::memcpy(&outs[pair_ids[j]], &gt[j], sizeof(Fq12));
    for (size_t j = 0; j < g1_ids.size(); ++j) {
        G1Jac p;
        std::memcpy(&p, res.data() + res_g1 + j * sizeof(G1Jac), sizeof(p));
        p = normalised<G1Ops>(p);
        std::memcpy(&outs[g1_ids[j]], &p, sizeof(p));
    }
    for (size_t j = 0; j < g2_ids.size(); ++j) {
        G2Jac p;
        std::memcpy(&p, res.data() + res_g2 + j * sizeof(G2Jac), sizeof(p));
        p = normalised<G2Ops>(p);
        std::memcpy(&outs[g2_ids[j]], &p, sizeof(p));
    }
    return JOLT_OK;
}

extern "C" int32_t jolt_host_dory_batch_plan(const size_t* lens, size_t n_items, size_t wg_cap, uint32_t* wg_item, uint32_t* wg_first, size_t* item_base, size_t* n_wgs, uint32_t* levels) {
    if ((n_items && (!lens || !item_base)) || !n_wgs || !levels || (wg_cap && (!wg_item || !wg_first))) return JOLT_ERR_INVALID_ARG;
    BatchPlan p;
    if (!batch_plan(lens, n_items, &p)) return JOLT_ERR_UNSUPPORTED;
    *n_wgs = p.wg_item.size();
    *levels = p.levels;
    for (size_t k = 0; k < n_items; ++k) item_base[k] = p.item_base[k];
    if (wg_cap == 0) return JOLT_OK;
    if (p.wg_item.size() > wg_cap) return JOLT_ERR_SIZE_MISMATCH;
    for (size_t w = 0; w < p.wg_item.size(); ++w) {
        wg_item[w] = p.wg_item[w];
        wg_first[w] = p.wg_first[w];
    }
    return JOLT_OK;
}
