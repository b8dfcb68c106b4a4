// jolt_amd/csrc/dory_host.hpp -- host-side helpers shared by the Dory entry points (dory.hip, dory_routines.hip, dory_pairing.hip, dory_resident.hip,
// dory_scheme.hip): the views of resident vectors, the argument checks' thread pool, and the two scopes every entry's body is written on -- HostCall (pool blocks,
// copies, phase clock, running error, the synchronise before return) and Fork (side chains forked from and joined to the main stream).
#pragma once
#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "ctx.hpp"

// the object behind jolt_dory_vec (dory_resident.hip makes and frees them; dory_scheme.hip reads them too)
struct jolt_dory_vec {
    jolt_ctx* ctx = nullptr;
    int32_t kind = 0;
    size_t len = 0;
    void* data = nullptr;  // device, from the context's pool
};

// the object behind jolt_dory_setup (dory_scheme.hip makes and frees them; dory_verify.hip reads them too)
struct jolt_dory_setup {
    jolt_ctx* ctx = nullptr;
    size_t n = 0;
    jolt_dory_vec *gamma1 = nullptr, *gamma2 = nullptr, *h1_vec = nullptr, *h2_vec = nullptr;
    jolt_g2_prepared* prepared = nullptr;
    jolt_g1_t h1;
    jolt_g2_t h2;
};

namespace jolt {
namespace dory_host {

// (vec, first, n) lies inside a vector of this context and kind.  Never first + n: that sum can wrap.
inline bool view_ok(const jolt_ctx* ctx, const jolt_dory_vec* v, int32_t kind, size_t first, size_t n) {
    return v && v->ctx == ctx && v->kind == kind && !(first > v->len || n > v->len - first);
}
// two valid views of n elements share an element
inline bool views_overlap(const jolt_dory_vec* a, size_t a_first, const jolt_dory_vec* b, size_t b_first, size_t n) {
    if (a != b || n == 0) return false;
    return a_first < b_first ? b_first - a_first < n : a_first - b_first < n;
}

// one wavefront per workgroup, one element per lane: the launch shape of every latency-bound Dory kernel (docs/kernels.md 3.5f)
constexpr int kLanes = 64;
inline unsigned lanes_grid(size_t n) { return (unsigned)((n + kLanes - 1) / kLanes); }

inline int32_t hip_fail(jolt_ctx* ctx, const char* what, hipError_t e) {
    ctx->last_error = std::string(what) + ": " + hipGetErrorString(e);
    return e == hipErrorOutOfMemory ? JOLT_ERR_OOM : JOLT_ERR_HIP;
}

// The argument checks run on the host before anything is enqueued (a refused call enqueues nothing).  A G2 on-curve check costs ~2 us of host time and a round holds
// 2^14 ... 2^16 points, which is more than the kernels take: long vectors are checked by up to 16 host threads.
template <class Ok>
bool parallel_all(size_t n, Ok&& ok_range) {
    const size_t hw = std::min<size_t>(16, std::max(1u, std::thread::hardware_concurrency()));
    const size_t parts = std::min(hw, n / 1024);
    if (parts <= 1) return ok_range((size_t)0, n);
    std::vector<char> ok(parts, 1);
    std::vector<std::thread> workers;
    size_t started = 0;
    try {
        for (; started + 1 < parts; ++started) workers.emplace_back([&ok, &ok_range, started, n, parts] { ok[started] = ok_range(n * started / parts, n * (started + 1) / parts) ? 1 : 0; });
    } catch (...) {  // no more threads to be had: the calling thread takes the rest
    }
    bool all = ok_range(n * started / parts, n);
    for (std::thread& w : workers) w.join();
    for (size_t t = 0; t < started; ++t) all = all && ok[t];
    return all;
}

struct DevBufs {  // pool blocks of one call, returned on every path
    jolt_ctx* ctx;
    std::vector<void*> blocks;
    explicit DevBufs(jolt_ctx* c) : ctx(c) {}
    ~DevBufs() {
        for (void* b : blocks) jolt_internal_dev_free(ctx, b);
    }
    template <class T>
    int32_t take(size_t count, T** out) {
        void* p = nullptr;
        const int32_t rc = jolt_internal_dev_alloc(ctx, std::max<size_t>(count, 1) * sizeof(T), &p);
        if (rc == JOLT_OK) blocks.push_back(p);
        *out = (T*)p;
        return rc;
    }
};

// One call of an entry point that copies from or to the caller's host arrays: its pool blocks, its phase clock (`ms` and `timing` of jolt_dory_routines_timing or
// jolt_dory_pairing_timing; none for an entry without a clock) and its running error.  After the first failure every member but finish() does nothing, so a body
// reads straight down: up() per array, `if (c.ok()) c.e = enqueue_...`, down(), finish().  finish() synchronises the stream on EVERY path: host memory of the call
// (the caller's arrays, tables on the entry's stack) is read and written until there.
struct HostCall {
    jolt_ctx* ctx;
    hipStream_t st;
    DevBufs bufs;
    hipError_t e = hipSuccess;
    int32_t rc = JOLT_OK;  // a pool allocation that failed; it outranks `e`
    double* ms = nullptr;
    bool timing = false;
    std::chrono::steady_clock::time_point t0;
    explicit HostCall(jolt_ctx* c) : ctx(c), st(c->stream), bufs(c) {}
    template <size_t P>
    HostCall(jolt_ctx* c, double (&phase_ms)[P], bool timing_on) : ctx(c), st(c->stream), bufs(c), ms(phase_ms), timing(timing_on), t0(std::chrono::steady_clock::now()) {
        if (timing) std::fill(ms, ms + P, 0.0);
    }
    bool ok() const { return e == hipSuccess && rc == JOLT_OK; }
    template <class T>
    void take(size_t n, T** dev) {
        if (ok()) rc = bufs.take(n, dev);
    }
    template <class T>
    void h2d(T* dev, const void* host, size_t n) {
        if (ok()) e = hipMemcpyAsync(dev, host, n * sizeof(T), hipMemcpyHostToDevice, st);
    }
    template <class T>
    void up(const void* host, size_t n, T** dev) {
        take(n, dev);
        h2d(*dev, host, n);
    }
    template <class T>
    void down(void* host, const T* dev, size_t n) {
        if (ok()) e = hipMemcpyAsync(host, dev, n * sizeof(T), hipMemcpyDeviceToHost, st);
    }
    // closes `phase`.  With timing on, the stream is drained first so that the phase gets its own wall time -- not for host-only phases (`drain` false); with
    // timing off, neither the stream nor the array is touched
    void mark(int phase, bool drain = true) {
        if (!timing || !ok()) return;
        if (drain) e = hipStreamSynchronize(st);
        stamp(phase);
    }
    // the call's last phase ends with its synchronise
    int32_t finish(const char* what, int last_phase = 0) {
        const hipError_t e_sync = hipStreamSynchronize(st);
        if (rc != JOLT_OK) return rc;
        if (e == hipSuccess) e = e_sync;
        if (timing) stamp(last_phase);
        return e == hipSuccess ? JOLT_OK : hip_fail(ctx, what, e);
    }

private:
    void stamp(int phase) {
        const auto t1 = std::chrono::steady_clock::now();
        ms[phase] += std::chrono::duration<double, std::milli>(t1 - t0).count();
        t0 = t1;
    }
};

// Side chains beside the context's main stream: forked from it by ev_fork when made, joined by ev_join[c].  A chain runs on the main stream itself when the
// context serialises its streams or has no side stream c.
struct Fork {
    jolt_ctx* ctx;
    int chains;
    hipStream_t st[3];
    hipError_t e;  // of the fork
    Fork(jolt_ctx* c, int n_chains) : ctx(c), chains(n_chains) {
        for (int k = 0; k < chains; ++k) st[k] = (c->serial_streams || !c->side[k]) ? c->stream : c->side[k];
        e = hipEventRecord(c->ev_fork, c->stream);
        for (int k = 0; k < chains && e == hipSuccess; ++k)
            if (st[k] != c->stream) e = hipStreamWaitEvent(st[k], c->ev_fork, 0);
    }
    // enqueued on every path: the main stream must not run ahead of a chain that was started.  A chain whose join cannot be enqueued is synchronised instead.
    // Returns `err`, or the first error of the joins when `err` is none.
    hipError_t join(hipError_t err) {
        for (int k = 0; k < chains; ++k) {
            if (st[k] == ctx->stream) continue;
            hipError_t ej = hipEventRecord(ctx->ev_join[k], st[k]);
            if (ej == hipSuccess) ej = hipStreamWaitEvent(ctx->stream, ctx->ev_join[k], 0);
            if (ej != hipSuccess) {
                (void)hipStreamSynchronize(st[k]);
                if (err == hipSuccess) err = ej;
            }
        }
        return err;
    }
};

template <class Pt>
Pt pt_from_abi(const void* p) {
    Pt r;
    std::memcpy(&r, p, sizeof(r));
    return r;
}

// ---- combine_hints (dory.hip): the shared-scalar digit plan and the launches over points on the device, for the host-pointer entry and the resident one ----
struct CombinePlan {
    std::vector<uint32_t> ent;    // per window, the terms with a non-zero digit, by descending magnitude
    std::vector<uint32_t> start;  // one offset into ent per window, and the end
};
bool combine_plan(const jolt_fr_t* scalars, size_t n, CombinePlan* plan);
// d_points: G1Jac, the hints back to back; meta: the hints' offsets into d_points, then their row counts; d_out: G1Jac, `rows` of them
int32_t combine_enqueue(jolt_ctx* ctx, const void* d_points, const std::vector<uint64_t>& meta, const CombinePlan& plan, size_t rows, void* d_out);

// elements [first, first + n) of a resident G1 vector of this context (dory_resident.hip, where jolt_dory_vec is defined): the device address (G1Jac), or null when the
// vector is of another kind or context or the view leaves it -- for the entries of dory.hip that write their results into resident vectors
void* g1_view(const jolt_ctx* ctx, const jolt_dory_vec* vec, size_t first, size_t n);

// the transcript callback of the library's engines (dory_scheme.hip): `user` is a jolt_host_transcript
int32_t engine_fn(void* user, int32_t phase, size_t round, const jolt_gt_t* gts, size_t n_gt, const jolt_g1_t* g1s, size_t n_g1, const jolt_g2_t* g2s, size_t n_g2, jolt_fr_t* challenge_out);

}  // namespace dory_host
}  // namespace jolt
