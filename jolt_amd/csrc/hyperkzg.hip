// jolt_amd/csrc/hyperkzg.hip -- HyperKZG prover pieces on gfx950 and the host-side mirror of commit/open.
//
// Device kernels replace the rayon / sequential loops of crates/jolt-hyperkzg/src/{scheme.rs,kzg.rs}:
//   fold_polynomials            scheme.rs:88-114   -> out-of-place LowToHigh bind (same kernel as the sumcheck bind)
//   eval_univariate x 3 points  kzg.rs:51-59,84-85 -> blocked Horner with per-block weights, one pass for the 3 points
//   B = sum_j q^j P_j           kzg.rs:95-105      -> one fused pass over all levels
//   compute_witness_polynomial  kzg.rs:34-46       -> the sequential recurrence h[i-1] = f[i] + h[i]*u as a blocked suffix
//                                                     scan (exact: the recurrence is linear, chunks compose by mu^C)
// All are HBM-bound streaming passes (<= 2 multiplies per element); the MSMs they feed dominate (msm.hip).
#include <algorithm>
#include <cstdlib>
#include <system_error>
#include <thread>

#include "ctx.hpp"
#include "g1.hip.h"
#include "grid_hint.hpp"
#include "host_mirror.hpp"
#include "hyperkzg_transcript.hpp"
#include "poly_kernels.hip.h"
#include "srs.hpp"
#include "term_map.hip.h"

using namespace jolt;

int32_t jolt_internal_msm(jolt_ctx* ctx, const jolt_srs* srs, const Fr* d_scalars, size_t n, G1Jac* out);
int32_t jolt_internal_msm_shifted(jolt_ctx* ctx, const jolt_srs* srs, const Fr* d_scalars, size_t n, const size_t* shifts, int n_shifts, G1Jac* out);
int32_t jolt_internal_msm_many(jolt_ctx* ctx, const jolt_srs* srs, const Fr* const* d_scalars, const size_t* n, size_t count, G1Jac* out,
                               const size_t* base_offsets = nullptr);

namespace {

constexpr int kHornerChunk = 16;

struct Fr3 {
    Fr v[3];
};

// table[t * 256 + i] = base_t^i for i < 256 (one workgroup): the per-thread weights (u^16)^tid of k_horner3, computed ONCE per evaluation
// point instead of by every thread of every level (which cost 2.5x the Horner steps themselves: 12.8 ms of a 2^26-coefficient opening)
static __global__ __launch_bounds__(kBlock) void k_power_table3(Fr3 base, Fr* __restrict__ table) {
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        Fr w = Fr::one(), b = base.v[t];
        for (unsigned e = threadIdx.x; e; e >>= 1) {
            if (e & 1) w = mul(w, b);
            b = sqr(b);
        }
        st_fr(table + t * kBlock + threadIdx.x, w);
    }
}
// u^e by square-and-multiply
__device__ __forceinline__ Fr fr_pow_u64(Fr b, uint64_t e) {
    Fr w = Fr::one();
    for (; e; e >>= 1) {
        if (e & 1) w = mul(w, b);
        b = sqr(b);
    }
    return w;
}
// partials[block*3 + t] = sum over this block's coefficients c[i] * u_t^i
// SUBTREE: c is a rank's COMPACT array (term_map.hip.h, kSubtree) and the exponent of slot i is term_global(map, i).  Chunks of 16 slots
// from slot 16 on and workgroups of 4096 slots from slot 4096 on lie inside one segment [2^L, 2^(L+1)) of the compact array, where the
// index is affine in the slot: only the workgroup weight changes (u^index(4096 b) instead of (u^4096)^b); workgroup 0 weighs its chunks
// one by one and its first chunk slot by slot.
template <bool SUBTREE>
static __global__ __launch_bounds__(kBlock) void k_horner3(const Fr* __restrict__ c, size_t n, Fr3 u, const Fr* __restrict__ chunk_weights /* (u^16)^tid */,
                                                           Fr3 u_block /* u^4096 */, Fr* __restrict__ partials, TermMap map) {
    __shared__ Fr block_weight[3];
    if (threadIdx.x < 3) {  // (u^4096)^blockIdx, once per workgroup
        if (SUBTREE) block_weight[threadIdx.x] = blockIdx.x ? fr_pow_u64(u.v[threadIdx.x], term_global(map, (size_t)blockIdx.x * kBlock * kHornerChunk)) : Fr::one();
        else block_weight[threadIdx.x] = fr_pow_u64(u_block.v[threadIdx.x], blockIdx.x);
    }
    size_t base = ((size_t)blockIdx.x * kBlock + threadIdx.x) * kHornerChunk;
    Fr acc[3] = {Fr::zero(), Fr::zero(), Fr::zero()};
    if (base < n) {
        size_t end = base + kHornerChunk < n ? base + kHornerChunk : n;
        if (SUBTREE && base == 0) {  // slots 0 .. 15: five segments and the crown slot, weighed one by one
            for (size_t i = base; i < end; ++i) {
                Fr ci = ld_fr(c + i);
                const uint64_t e = term_global(map, i);
#pragma unroll
                for (int t = 0; t < 3; ++t) acc[t] = add(acc[t], mul(ci, fr_pow_u64(u.v[t], e)));
            }
        } else {
            for (size_t i = end; i-- > base;) {
                Fr ci = ld_fr(c + i);
#pragma unroll
                for (int t = 0; t < 3; ++t) acc[t] = add(mul(acc[t], u.v[t]), ci);
            }
        }
    }
    __syncthreads();
    if (base < n) {
        if (SUBTREE && blockIdx.x == 0) {
            if (base) {
                const uint64_t e = term_global(map, base);
#pragma unroll
                for (int t = 0; t < 3; ++t) acc[t] = mul(acc[t], fr_pow_u64(u.v[t], e));
            }
        } else {
#pragma unroll
            for (int t = 0; t < 3; ++t) acc[t] = mul(mul(acc[t], ld_fr(chunk_weights + t * kBlock + threadIdx.x)), block_weight[t]);
        }
    }
    block_reduce_store<3>(acc, partials);
}

// The same sums with coalesced loads (the plain, non-subtree case): thread t of a workgroup takes the coefficients base + 256 e + t, e < 16 -- adjacent lanes on
// adjacent coefficients in every load -- as a polynomial in x^256, weighs it with u^t (lane_weights: u^tid) and the workgroup with (u^4096)^blockIdx.
// The kernel is bound by its field multiplications (75 G/s measured at three per coefficient), not by the loads, so what pays is PLUS_MINUS: for u_1 = -u_0 (the points
// r and -r of an opening, kzg.rs:84-85) the polynomial in x^256 takes the same value at both, and the second point costs a sign per lane instead of a multiplication per
// coefficient: two multiplications per coefficient instead of three.
template <bool PLUS_MINUS>
static __global__ __launch_bounds__(kBlock) void k_horner3_strided(const Fr* __restrict__ c, size_t n, Fr3 u256, const Fr* __restrict__ lane_weights /* u^tid */,
                                                                   Fr3 u_block /* u^4096 */, Fr* __restrict__ partials) {
    __shared__ Fr block_weight[3];
    if (threadIdx.x < 3) block_weight[threadIdx.x] = fr_pow_u64(u_block.v[threadIdx.x], blockIdx.x);
    const size_t base = (size_t)blockIdx.x * kBlock * kHornerChunk + threadIdx.x;
    Fr ci[kHornerChunk];
#pragma unroll
    for (int e = 0; e < kHornerChunk; ++e) {
        const size_t i = base + (size_t)e * kBlock;
        ci[e] = i < n ? ld_fr(c + i) : Fr::zero();
    }
    Fr acc[3] = {ci[kHornerChunk - 1], ci[kHornerChunk - 1], ci[kHornerChunk - 1]};
#pragma unroll
    for (int e = kHornerChunk - 2; e >= 0; --e) {
#pragma unroll
        for (int t = 0; t < 3; ++t)
            if (!(PLUS_MINUS && t == 1)) acc[t] = add(mul(acc[t], u256.v[t]), ci[e]);
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 3; ++t)
        if (!(PLUS_MINUS && t == 1)) acc[t] = mul(mul(acc[t], ld_fr(lane_weights + t * kBlock + threadIdx.x)), block_weight[t]);
    if (PLUS_MINUS) acc[1] = (threadIdx.x & 1) ? neg(acc[0]) : acc[0];  // (-u)^(4096 b + 256 e + t) = (-1)^t u^(...)
    block_reduce_store<3>(acc, partials);
}

struct RlcArgs {
    const Fr* level[40];
    size_t len[40];
    int ell;
};
// out[i] = sum_j q^j P_j[i] over the levels that still cover index i (qpow resident in device memory)
static __global__ __launch_bounds__(kBlock) void k_rlc(RlcArgs a, const Fr* __restrict__ qpow, Fr* __restrict__ out, size_t n) {
    size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    Fr acc = ld_fr(a.level[0] + i);  // q^0 = 1
    for (int j = 1; j < a.ell; ++j) {
        if (i >= a.len[j]) break;  // lengths halve: no later level covers i either
        acc = add(acc, mul(ld_fr(a.level[j] + i), ld_fr(qpow + j)));
    }
    st_fr(out + i, acc);
}

// log2 of the elements per thread of the blocked suffix scan: 64.  8 / 16 / 32 / 64 measure the same (141 ms of suffix + Horner kernel time over three
// 2^26-coefficient openings each)
constexpr int kScanChunkLog = 6;
// A thread of a scan walks a chunk of its own, 2 or 4 KiB from its neighbours'.  It reads the kLineFr coefficients of a 128-byte line together and then steps through
// them, instead of coming back to the line four times with every other thread's line in between (chunks start on a line boundary).
constexpr int kLineFr = 4;
__device__ __forceinline__ void ld_line(const Fr* p, Fr (&x)[kLineFr]) {
#pragma unroll
    for (int i = 0; i < kLineFr; ++i) x[i] = ld_fr(p + i);
}
// LANES interleaved chains: s[k] = a[k] + mu s[k + LANES].  LANES = 1 is the suffix Horner of a witness polynomial (kzg.rs:39-44); LANES = 2 runs the even and the odd
// coefficients as two chains, which divides by (X^2 - mu) in ONE pass -- the pair of witness polynomials at r and -r of an opening share that quotient
// (hyperkzg_open_impl).  A chunk is kScanChunk positions of EVERY chain (kScanChunk * LANES consecutive coefficients); heads / S hold LANES values per chunk.
// A version through LDS tiles (coalesced loads and stores, chains of 8) needed 3.1 multiplications per coefficient for its in-tile scan and measured no faster
// (profiles/r04_open_tiled_scan_ab.txt).
// heads[c * LANES + l] = Horner of chunk c of chain l with zero carry-in
template <int LANES>
static __global__ __launch_bounds__(kBlock) void k_suffix_heads(const Fr* __restrict__ a, size_t m /* positions per chain */, Fr mu, Fr* __restrict__ heads, size_t nchunks, size_t kScanChunk) {
    size_t c = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (c >= nchunks) return;
    size_t lo = c * kScanChunk, hi = lo + kScanChunk < m ? lo + kScanChunk : m;
    Fr acc[LANES];
#pragma unroll
    for (int l = 0; l < LANES; ++l) acc[l] = Fr::zero();
    size_t k = hi;
    for (; k > lo && (k * LANES) % kLineFr; --k) {  // down to a line boundary (a short last chunk only)
#pragma unroll
        for (int l = 0; l < LANES; ++l) acc[l] = add(mul(acc[l], mu), ld_fr(a + (k - 1) * LANES + l));
    }
    for (; k > lo; k -= kLineFr / LANES) {  // a line at a time, as k_suffix_apply
        Fr x[kLineFr];
        ld_line(a + (k * LANES - kLineFr), x);
#pragma unroll
        for (int i = kLineFr - 1; i >= 0; --i) acc[i % LANES] = add(mul(acc[i % LANES], mu), x[i]);
    }
#pragma unroll
    for (int l = 0; l < LANES; ++l) st_fr(heads + c * LANES + l, acc[l]);
}
// s inside chunk c, starting from the true carry-in S[(c + 1) * LANES + l] (the last chunk: `carry`, the value entering the array from above -- zero for a whole
// polynomial, the suffix evaluation of the segments above for one segment of a sharded one; LANES = 1 only); writes s[k] to out[k - shift] (k >= shift, in coefficients)
template <int LANES>
static __global__ __launch_bounds__(kBlock) void k_suffix_apply(const Fr* __restrict__ a, size_t m, Fr mu, const Fr* __restrict__ S, size_t nchunks,
                                                                Fr* __restrict__ out, size_t shift, size_t kScanChunk, Fr carry) {
    size_t c = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (c >= nchunks) return;
    size_t lo = c * kScanChunk, hi = lo + kScanChunk < m ? lo + kScanChunk : m;
    Fr acc[LANES];
#pragma unroll
    for (int l = 0; l < LANES; ++l) acc[l] = (S != nullptr && c + 1 < nchunks) ? ld_fr(S + (c + 1) * LANES + l) : carry;
    static_assert(kLineFr % LANES == 0, "a line holds whole positions");
    size_t k = hi;
    for (; k > lo && (k * LANES) % kLineFr; --k) {  // down to a line boundary (a short last chunk only: chunks start on one)
#pragma unroll
        for (int l = LANES - 1; l >= 0; --l) {
            const size_t g = (k - 1) * LANES + l;
            acc[l] = add(mul(acc[l], mu), ld_fr(a + g));
            if (g >= shift) st_fr(out + (g - shift), acc[l]);
        }
    }
    for (; k > lo; k -= kLineFr / LANES) {  // (k - lo) * LANES is a multiple of kLineFr from here on
        const size_t g0 = k * LANES - kLineFr;
        Fr x[kLineFr];
        ld_line(a + g0, x);
#pragma unroll
        for (int i = kLineFr - 1; i >= 0; --i) {
            acc[i % LANES] = add(mul(acc[i % LANES], mu), x[i]);
            if (g0 + i >= shift) st_fr(out + (g0 + i - shift), acc[i % LANES]);
        }
    }
}

// s[k] = a[k] + mu s[k + LANES] over the m coefficients of a (m a multiple of LANES), written to out[k - shift].  `given_heads`: the chunk heads of a where the caller
// has them already (nchunks * LANES values in this function's chunk geometry; the opening gets them by linearity from the heads of its levels); nullptr: a heads pass
// over the array computes them.
template <int LANES>
int32_t suffix_scan(jolt_ctx* ctx, const Fr* a, size_t m, const Fr& mu, Fr* out, size_t shift, const Fr& carry, const Fr* given_heads = nullptr) {
    if (m % LANES) return JOLT_ERR_UNSUPPORTED;
    if (LANES != 1 && !(carry == Fr::zero())) return JOLT_ERR_UNSUPPORTED;
    const size_t positions = m / LANES;  // per chain
    // a non-zero carry enters the chunk-level recurrence with the weight mu^chunk: the last chunk must be full (segments of a sharded
    // polynomial are powers of two long)
    if (!(carry == Fr::zero()) && (m & (m - 1)) != 0) return JOLT_ERR_UNSUPPORTED;
    const int chunk_log = kScanChunkLog;
    const size_t kScanChunk = (size_t)1 << chunk_log;
    size_t nchunks = (positions + kScanChunk - 1) / kScanChunk;
    unsigned grid = (unsigned)((nchunks + kBlock - 1) / kBlock);
    if (nchunks <= 1) {
        hipLaunchKernelGGL(k_suffix_apply<LANES>, dim3(1), dim3(kBlock), 0, ctx->stream, a, positions, mu, (const Fr*)nullptr, (size_t)1, out, shift, kScanChunk, carry);
        JOLT_HIP_TRY(ctx, hipGetLastError());
        return JOLT_OK;
    }
    Fr *heads = nullptr, *S = nullptr;
    if (given_heads == nullptr) {
        JOLT_TRY(jolt_internal_dev_alloc(ctx, nchunks * LANES * sizeof(Fr), (void**)&heads));
        hipLaunchKernelGGL(k_suffix_heads<LANES>, dim3(grid), dim3(kBlock), 0, ctx->stream, a, positions, mu, heads, nchunks, kScanChunk);
        given_heads = heads;
    }
    if (jolt_internal_dev_alloc(ctx, nchunks * LANES * sizeof(Fr), (void**)&S) != JOLT_OK) { if (heads) jolt_internal_dev_free(ctx, heads); return JOLT_ERR_OOM; }
    Fr mu_c = mu;
    for (int i = 0; i < chunk_log; ++i) mu_c = sqr(mu_c);  // mu^chunk
    int32_t s = suffix_scan<LANES>(ctx, given_heads, nchunks * LANES, mu_c, S, 0, carry);  // the chunk values form LANES chains again; the carry enters at the same place
    if (s == JOLT_OK) {
        hipLaunchKernelGGL(k_suffix_apply<LANES>, dim3(grid), dim3(kBlock), 0, ctx->stream, a, positions, mu, (const Fr*)S, nchunks, out, shift, kScanChunk, carry);
        if (hipGetLastError() != hipSuccess) s = JOLT_ERR_HIP;
    }
    if (heads) jolt_internal_dev_free(ctx, heads);  // pool blocks: reused in stream order, no synchronisation
    jolt_internal_dev_free(ctx, S);
    return s;
}
// s = suffix Horner of a (length m) with multiplier mu, written to out[k - shift]
int32_t suffix_horner(jolt_ctx* ctx, const Fr* a, size_t m, const Fr& mu, Fr* out, size_t shift, const Fr& carry = Fr::zero()) {
    return suffix_scan<1>(ctx, a, m, mu, out, shift, carry);
}

// ---- the opening's evaluations as the heads of its quotient scan (hyperkzg_open_impl, one GPU) ---------------------------------------------
// With mu = r^2 the chunk heads of suffix_scan<2> over level P_j are Horner values of the chunk's even and odd coefficients, so their chunk-level Horner sums are
// E_j(mu) and O_j(mu) for P_j(X) = E_j(X^2) + X O_j(X^2): P_j(r) = E_j + r O_j, P_j(-r) = E_j - r O_j, and, level j + 1 being the fold (1 - x) E_j + x O_j
// coefficient by coefficient, P_(j+1)(mu) = (1 - x) E_j(mu) + x O_j(mu).  Heads are linear in the input and every level starts at index 0, so the heads of
// B = sum_j q^j P_j are the same combination of the levels' heads (k_rlc over arrays 64 times shorter): ONE pass over the levels before q exists gives every
// evaluation of the proof and the heads of the scan that divides B, at one multiplication per coefficient (two on level 0, whose value at mu needs a third chain).
struct LevelHeadsArgs {
    const Fr* level[40];
    Fr* heads[40];             // 2 * nchunks_j values: (even, odd) per chunk of 2 * 64 coefficients
    size_t len[40];
    unsigned first_block[41];  // level j owns the workgroups [first_block[j], first_block[j + 1]): 256 chunks each
    int ell;
};
// partials[block * 3 + t]: the block's chunk values weighed with lane_weights[t][tid] = w_t^tid (w_0 = w_1 = mu^64, a chunk of one chain; w_2 = mu^128: a chunk of
// the plain Horner sum of level 0, zero on the other levels)
static __global__ __launch_bounds__(kBlock) void k_level_heads(LevelHeadsArgs a, Fr mu, const Fr* __restrict__ lane_weights, Fr* __restrict__ partials) {
    int j = 0;
    while (j + 1 < a.ell && blockIdx.x >= a.first_block[j + 1]) ++j;
    const Fr* __restrict__ p = a.level[j];
    const size_t chunk = (size_t)1 << kScanChunkLog, positions = a.len[j] / 2, nchunks = (positions + chunk - 1) >> kScanChunkLog;
    const size_t c = (size_t)(blockIdx.x - a.first_block[j]) * kBlock + threadIdx.x;
    Fr acc[3] = {Fr::zero(), Fr::zero(), Fr::zero()};
    if (c < nchunks) {
        const size_t lo = c * chunk, hi = lo + chunk < positions ? lo + chunk : positions;
        const bool plain = j == 0;  // (the same for the whole workgroup)
        auto step = [&](const Fr& e, const Fr& o) {
            acc[0] = add(mul(acc[0], mu), e);
            acc[1] = add(mul(acc[1], mu), o);
            if (plain) acc[2] = add(mul(add(mul(acc[2], mu), o), mu), e);
        };
        size_t k = hi;
        if (k & 1) {  // (a level of two coefficients)
            --k;
            step(ld_fr(p + 2 * k), ld_fr(p + 2 * k + 1));
        }
        for (; k > lo; k -= 2) {  // two positions: one 128-byte line
            Fr x[kLineFr];
            ld_line(p + (2 * k - kLineFr), x);
            step(x[2], x[3]);
            step(x[0], x[1]);
        }
        Fr* __restrict__ h = a.heads[j];
        st_fr(h + 2 * c, acc[0]);
        st_fr(h + 2 * c + 1, acc[1]);
#pragma unroll
        for (int t = 0; t < 3; ++t)
            if (t < 2 || j == 0) acc[t] = mul(acc[t], ld_fr(lane_weights + t * kBlock + threadIdx.x));
    }
    block_reduce_store<3>(acc, partials);
}
// results[3 j + t] = sum over level j's workgroups b of partials[b][t] (w_t^256)^b: workgroup = level; thread tid takes the workgroups tid, tid + 256, ... by Horner
// in (w_t^256)^256 and weighs the sum with (w_t^256)^tid
static __global__ __launch_bounds__(kBlock) void k_level_totals(LevelHeadsArgs a, const Fr* __restrict__ partials, Fr3 wb /* w_t^256 */, Fr3 wb256, Fr* __restrict__ results) {
    const unsigned b0 = a.first_block[blockIdx.x], nb = a.first_block[blockIdx.x + 1] - b0;
    Fr acc[3] = {Fr::zero(), Fr::zero(), Fr::zero()};
    if (threadIdx.x < nb) {
        for (unsigned b = threadIdx.x + (nb - 1 - threadIdx.x) / kBlock * kBlock;; b -= kBlock) {
#pragma unroll
            for (int t = 0; t < 3; ++t) acc[t] = add(mul(acc[t], wb256.v[t]), ld_fr(partials + (size_t)(b0 + b) * 3 + t));
            if (b < (unsigned)kBlock) break;
        }
#pragma unroll
        for (int t = 0; t < 3; ++t) acc[t] = mul(acc[t], fr_pow_u64(wb.v[t], threadIdx.x));
    }
    block_reduce_store_at<3>(acc, results + 3 * (size_t)blockIdx.x);
}

struct OpenLevelHeads {
    LevelHeadsArgs args;
    Fr* heads = nullptr;  // one pool block behind args.heads[]
};
// The first pass of an opening behind r: the heads of every level and, from their sums, v[t][j] = P_j(u_t) for u = (r, -r, r^2), row-major as jolt_hyperkzg_eval3 returns them.
// Level lengths are 2^(ell - j); x: the opening point (fold j uses x[ell - j], jolt_hyperkzg_fold).  One download, one synchronisation.
int32_t open_level_heads(jolt_ctx* ctx, jolt_table* const* levels, size_t ell, const Fr& r, const jolt_fr_t* x, jolt_fr_t* v_out, OpenLevelHeads* out) {
    LevelHeadsArgs& a = out->args;
    const size_t chunk = (size_t)1 << kScanChunkLog;
    size_t total = 0, off[40];
    a.ell = (int)ell;
    a.first_block[0] = 0;
    for (size_t j = 0; j < 40; ++j) { a.level[j] = nullptr; a.heads[j] = nullptr; a.len[j] = 0; }
    for (size_t j = 0; j < ell; ++j) {
        if (!levels[j] || levels[j]->len < 2 || levels[j]->len % 2) return JOLT_ERR_INVALID_ARG;
        const size_t nchunks = (levels[j]->len / 2 + chunk - 1) / chunk;
        a.level[j] = levels[j]->data();
        a.len[j] = levels[j]->len;
        a.first_block[j + 1] = a.first_block[j] + (unsigned)((nchunks + kBlock - 1) / kBlock);
        off[j] = total;
        total += 2 * nchunks;
    }
    const unsigned nblocks = a.first_block[ell];
    const Fr mu = mul(r, r);
    Fr3 w, wb, wb256;
    w.v[0] = mu;
    for (int i = 0; i < kScanChunkLog; ++i) w.v[0] = sqr(w.v[0]);
    w.v[1] = w.v[0];
    w.v[2] = sqr(w.v[0]);
    for (int t = 0; t < 3; ++t) {
        wb.v[t] = w.v[t];
        for (int i = 0; i < 8; ++i) wb.v[t] = sqr(wb.v[t]);  // kBlock = 2^8 chunks per workgroup
        wb256.v[t] = wb.v[t];
        for (int i = 0; i < 8; ++i) wb256.v[t] = sqr(wb256.v[t]);
    }
    static_assert(kBlock == 256, "the chunk weights of k_level_heads / k_level_totals are powers by eight squarings");
    JOLT_TRY(jolt_internal_ensure_scratch(ctx, (size_t)nblocks * 3, 3 * ell + 8));
    Fr* lane_weights = nullptr;
    JOLT_TRY(jolt_internal_dev_alloc(ctx, 3 * kBlock * sizeof(Fr), (void**)&lane_weights));
    if (jolt_internal_dev_alloc(ctx, total * sizeof(Fr), (void**)&out->heads) != JOLT_OK) { jolt_internal_dev_free(ctx, lane_weights); return JOLT_ERR_OOM; }
    for (size_t j = 0; j < ell; ++j) a.heads[j] = out->heads + off[j];
    hipLaunchKernelGGL(k_power_table3, dim3(1), dim3(kBlock), 0, ctx->stream, w, lane_weights);
    hipLaunchKernelGGL(k_level_heads, dim3(nblocks), dim3(kBlock), 0, ctx->stream, a, mu, (const Fr*)lane_weights, ctx->d_partials);
    hipLaunchKernelGGL(k_level_totals, dim3((unsigned)ell), dim3(kBlock), 0, ctx->stream, a, (const Fr*)ctx->d_partials, wb, wb256, ctx->d_results);
    hipError_t e = hipGetLastError();
    jolt_internal_dev_free(ctx, lane_weights);  // stream-ordered: safe right after the last launch
    if (e == hipSuccess) e = hipMemcpyAsync(ctx->h_results, ctx->d_results, 3 * ell * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        ctx->last_error = std::string("hyperkzg open (level heads): ") + hipGetErrorString(e);
        jolt_internal_dev_free(ctx, out->heads);
        out->heads = nullptr;
        return JOLT_ERR_HIP;
    }
    const Fr* tot = ctx->h_results;  // (E_j, O_j, P_0(mu) on level 0) at mu
    for (size_t j = 0; j < ell; ++j) {
        const Fr ro = mul(r, tot[3 * j + 1]);
        Fr at_mu = tot[2];
        if (j) {
            const Fr xj = fr_from_abi(&x[ell - j]);
            at_mu = add(tot[3 * (j - 1)], mul(xj, sub(tot[3 * (j - 1) + 1], tot[3 * (j - 1)])));
        }
        fr_to_abi(&v_out[j], add(tot[3 * j], ro));
        fr_to_abi(&v_out[ell + j], sub(tot[3 * j], ro));
        fr_to_abi(&v_out[2 * ell + j], at_mu);
    }
    return JOLT_OK;
}
// q = B div (X^2 - mu) for B = sum_j q^j P_j (length len_0, qp: len_0 - 2 coefficients): the heads of the scan are the same combination of the levels' heads,
// over arrays 64 times shorter than the levels, and the heads pass over B is not run
int32_t open_quotient(jolt_ctx* ctx, const OpenLevelHeads& lh, const Fr& q, const Fr& mu, const Fr* B, Fr* qp) {
    const LevelHeadsArgs& a = lh.args;
    const size_t ell = (size_t)a.ell, chunk = (size_t)1 << kScanChunkLog;
    RlcArgs hd;
    hd.ell = a.ell;
    std::vector<Fr> qpow(ell);
    Fr cur = Fr::one();
    for (size_t j = 0; j < 40; ++j) {
        hd.level[j] = a.heads[j];
        hd.len[j] = j < ell ? 2 * ((a.len[j] / 2 + chunk - 1) / chunk) : 0;
    }
    for (size_t j = 0; j < ell; ++j) { qpow[j] = cur; cur = mul(cur, q); }  // challenge_powers (kzg.rs:213-221)
    jolt_table* dq = nullptr;
    JOLT_TRY(jolt_table_upload(ctx, reinterpret_cast<const jolt_fr_t*>(qpow.data()), ell, &dq));
    Fr* heads_b = nullptr;
    int32_t s = jolt_internal_dev_alloc(ctx, hd.len[0] * sizeof(Fr), (void**)&heads_b);
    if (s == JOLT_OK) {
        hipLaunchKernelGGL(k_rlc, dim3((unsigned)((hd.len[0] + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->stream, hd, (const Fr*)dq->data(), heads_b, hd.len[0]);
        if (hipGetLastError() != hipSuccess) s = JOLT_ERR_HIP;
    }
    if (s == JOLT_OK) s = suffix_scan<2>(ctx, B, a.len[0], mu, qp, 2, Fr::zero(), heads_b);
    if (heads_b) jolt_internal_dev_free(ctx, heads_b);
    jolt_table_free(ctx, dq);  // back to the pool; reused in stream order
    return s;
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------------
// device entry points
// ------------------------------------------------------------------------------------------------------------------
extern "C" int32_t jolt_hyperkzg_fold(jolt_ctx* ctx, const jolt_table* evals, const jolt_fr_t* point, size_t ell, jolt_table** levels_out) {
    if (!ctx || !evals || !point || !levels_out) return JOLT_ERR_INVALID_ARG;
    if (ell == 0) return JOLT_ERR_EMPTY_POINT;
    if (evals->len != ((size_t)1 << ell)) return JOLT_ERR_SIZE_MISMATCH;  // scheme.rs:133 assert
    JOLT_TRY(jolt_table_clone(ctx, evals, &levels_out[0]));
    for (size_t i = 1; i < ell; ++i) {  // fold i uses point[ell - i] (scheme.rs:97-98)
        Fr x = fr_from_abi(&point[ell - i]);
        JOLT_REQUIRE(ctx, fr_is_canonical(x), "point coordinate is not a canonical Fr");
        const jolt_table* prev = levels_out[i - 1];
        size_t half = prev->len / 2;
        jolt_table* nxt = nullptr;
        JOLT_TRY(jolt_internal_table_new(ctx, half, &nxt));
        BindBatch b;
        b.in[0] = prev->data();
        b.out[0] = nxt->data();
        b.half[0] = half;
        dim3 grid((unsigned)((half + kBlock - 1) / kBlock), 1);
        if (fr_low_limbs_zero(x)) hipLaunchKernelGGL(k_bind_low_to_high<true>, grid, dim3(kBlock), 0, ctx->stream, b, x);
        else hipLaunchKernelGGL(k_bind_low_to_high<false>, grid, dim3(kBlock), 0, ctx->stream, b, x);
        JOLT_HIP_TRY(ctx, hipGetLastError());
        levels_out[i] = nxt;
    }
    return JOLT_OK;
}

extern "C" int32_t jolt_hyperkzg_eval3(jolt_ctx* ctx, jolt_table* const* levels, size_t ell, const jolt_fr_t u[3], jolt_fr_t* v_out) {
    if (!ctx || !levels || !u || !v_out || ell == 0 || ell > 40) return JOLT_ERR_INVALID_ARG;
    Fr3 uu, u256, u4096;
    for (int t = 0; t < 3; ++t) {
        uu.v[t] = fr_from_abi(&u[t]);
        JOLT_REQUIRE(ctx, fr_is_canonical(uu.v[t]), "evaluation point is not a canonical Fr");
        Fr p = uu.v[t];
        for (int i = 0; i < 8; ++i) p = sqr(p);
        u256.v[t] = p;
        for (int i = 0; i < 4; ++i) p = sqr(p);
        u4096.v[t] = p;
    }
    const bool plus_minus = uu.v[1] == neg(uu.v[0]);
    JOLT_TRY(jolt_internal_ensure_scratch(ctx, 1, 3 * ell + 8));
    Fr* chunk_weights = nullptr;
    JOLT_TRY(jolt_internal_dev_alloc(ctx, 3 * kBlock * sizeof(Fr), (void**)&chunk_weights));
    hipLaunchKernelGGL(k_power_table3, dim3(1), dim3(kBlock), 0, ctx->stream, uu, chunk_weights);  // u^tid
    struct FreeWeights { jolt_ctx* c; Fr* p; ~FreeWeights() { jolt_internal_dev_free(c, p); } } free_weights{ctx, chunk_weights};  // stream-ordered: safe right after the last launch
    for (size_t j = 0; j < ell; ++j) {
        const jolt_table* t = levels[j];
        if (!t) return JOLT_ERR_INVALID_ARG;
        size_t per_block = (size_t)kBlock * kHornerChunk;
        int grid = (int)std::max<size_t>(1, (t->len + per_block - 1) / per_block);
        JOLT_TRY(jolt_internal_ensure_scratch(ctx, (size_t)grid * 3, 3 * ell + 8));
        if (plus_minus)
            hipLaunchKernelGGL(k_horner3_strided<true>, dim3(grid), dim3(kBlock), 0, ctx->stream, (const Fr*)t->data(), t->len, u256, (const Fr*)chunk_weights, u4096, ctx->d_partials);
        else
            hipLaunchKernelGGL(k_horner3_strided<false>, dim3(grid), dim3(kBlock), 0, ctx->stream, (const Fr*)t->data(), t->len, u256, (const Fr*)chunk_weights, u4096, ctx->d_partials);
        JOLT_HIP_TRY(ctx, hipGetLastError());
        hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(kBlock), 0, ctx->stream, (const Fr*)ctx->d_partials, grid, 3, ctx->d_results + 3 * j);
        JOLT_HIP_TRY(ctx, hipGetLastError());
    }
    JOLT_HIP_TRY(ctx, hipMemcpyAsync(ctx->h_results, ctx->d_results, 3 * ell * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
    JOLT_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t j = 0; j < ell; ++j)
        for (int t = 0; t < 3; ++t) fr_to_abi(&v_out[(size_t)t * ell + j], ctx->h_results[3 * j + t]);  // v[t][j], row-major
    return JOLT_OK;
}

extern "C" int32_t jolt_hyperkzg_rlc(jolt_ctx* ctx, jolt_table* const* levels, size_t ell, const jolt_fr_t* q, jolt_table** out) {
    if (!ctx || !levels || !q || !out || ell == 0 || ell > 40) return JOLT_ERR_INVALID_ARG;
    Fr qq = fr_from_abi(q);
    JOLT_REQUIRE(ctx, fr_is_canonical(qq), "q is not a canonical Fr");
    RlcArgs a;
    a.ell = (int)ell;
    std::vector<Fr> qpow(ell);
    Fr cur = Fr::one();
    for (size_t j = 0; j < 40; ++j) { a.level[j] = nullptr; a.len[j] = 0; }
    for (size_t j = 0; j < ell; ++j) {  // challenge_powers (kzg.rs:213-221)
        if (!levels[j]) return JOLT_ERR_INVALID_ARG;
        if (j && levels[j]->len > levels[j - 1]->len) return JOLT_ERR_SIZE_MISMATCH;
        a.level[j] = levels[j]->data();
        a.len[j] = levels[j]->len;
        qpow[j] = cur;
        cur = mul(cur, qq);
    }
    size_t n = levels[0]->len;
    jolt_table *res = nullptr, *dq = nullptr;
    JOLT_TRY(jolt_internal_table_new(ctx, n, &res));
    int32_t s = jolt_table_upload(ctx, reinterpret_cast<const jolt_fr_t*>(qpow.data()), ell, &dq);
    if (s != JOLT_OK) { jolt_table_free(ctx, res); return s; }
    hipLaunchKernelGGL(k_rlc, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->stream, a, (const Fr*)dq->data(), res->data(), n);
    hipError_t e = hipGetLastError();
    jolt_table_free(ctx, dq);  // back to the pool; reused in stream order
    if (e != hipSuccess) { jolt_table_free(ctx, res); ctx->last_error = hipGetErrorString(e); return JOLT_ERR_HIP; }
    *out = res;
    return JOLT_OK;
}

extern "C" int32_t jolt_hyperkzg_witness_poly(jolt_ctx* ctx, const jolt_table* f, const jolt_fr_t* u, jolt_table** out) {
    if (!ctx || !f || !u || !out) return JOLT_ERR_INVALID_ARG;
    Fr uu = fr_from_abi(u);
    JOLT_REQUIRE(ctx, fr_is_canonical(uu), "u is not a canonical Fr");
    size_t d = f->len;
    jolt_table* h = nullptr;
    JOLT_TRY(jolt_internal_table_new(ctx, d > 1 ? d - 1 : 0, &h));
    if (d > 1) {
        // h[k] = s[k+1] with s[k] = f[k] + u*s[k+1]  (kzg.rs:39-44)
        int32_t s = suffix_horner(ctx, f->data(), d, uu, h->data(), 1);
        if (s != JOLT_OK) { jolt_table_free(ctx, h); return s; }
    }
    *out = h;
    return JOLT_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// host mirror: HyperKZGScheme::{commit, open}
// ------------------------------------------------------------------------------------------------------------------
using namespace jolt_host;

using namespace jolt::hyperkzg_host;  // append_g1, OpenTranscript: shared with the verifier (hyperkzg_transcript.hpp)

// CommitmentScheme::commit -> kzg_commit (scheme.rs:302-312, kzg.rs:15-27)
extern "C" int32_t jolt_host_hyperkzg_commit(jolt_ctx* ctx, const jolt_srs* srs, const jolt_table* evals, jolt_g1_t* out) {
    if (!ctx || !srs || !evals || !out) return JOLT_ERR_INVALID_ARG;
    G1Jac r;
    JOLT_TRY(jolt_internal_msm(ctx, srs, evals->data(), evals->len, &r));  // SrsTooSmall when len > srs length
    std::memcpy(out, &r, sizeof(r));
    return JOLT_OK;
}

// The MSMs of an opening over `world` ranks: rank g multiplies terms [n*g/world, n*(g+1)/world) of every MSM
// against the same range of the bases, the partial points are all-gathered (96 bytes each) and added in rank order on every rank,
// so all ranks absorb identical commitments and draw identical challenges.  world = 1: the plain opening.
//
// block > 0: the BLOCK-CYCLIC assignment instead -- term i belongs to rank (i / block) % world and `srs` is the rank's compact SRS
// (its own terms' bases in index order, msm.hip), so the rank's terms of every level are a prefix of its SRS and the window tables
// built over it (51 GB for 2^26 points, whatever the world size) serve all of them; the rank's scalars are gathered into one
// compact buffer first (32 B read + written per owned term).
int32_t jolt_internal_gather_owned_terms(jolt_ctx* ctx, const Fr* src, size_t n, const TermMap& map, Fr* dst);
namespace {
int32_t gather_with_status(jolt_ctx* ctx, jolt_gather_fn gather, void* user, int32_t local_status, const jolt_fr_t* payload, size_t count, int world, std::vector<jolt_fr_t>* all);
}
static int32_t sharded_msm_many(jolt_ctx* ctx, const jolt_srs* srs, const std::vector<const Fr*>& ptrs, const std::vector<size_t>& lens, int rank, int world,
                                size_t block, jolt_gather_fn gather, void* user, G1Jac* out) {
    const size_t count = ptrs.size();
    if (count == 0) return JOLT_OK;
    if (world <= 1) return jolt_internal_msm_many(ctx, srs, ptrs.data(), lens.data(), count, out);
    std::vector<const Fr*> p(count);
    std::vector<size_t> n(count), off(count);
    std::vector<G1Jac> partial(count), all((size_t)world * count);
    int32_t ls = JOLT_OK;  // this rank's local status (see gather_with_status)
    if (block) {
        TermMap map;
        if (!make_block_map(block, rank, world, &map)) return JOLT_ERR_INVALID_ARG;  // the same arguments on every rank: all of them return here
        size_t total = 0;
        for (size_t i = 0; i < count; ++i) {
            n[i] = term_owned(map, lens[i]);
            if (n[i] > srs->n && ls == JOLT_OK) ls = JOLT_ERR_SRS_TOO_SMALL;  // a rank-local condition (its compact SRS): reported through the exchange
            off[i] = total;
            total += n[i];
        }
        Fr* compact = nullptr;
        int32_t s = ls;
        if (s == JOLT_OK) s = jolt_internal_dev_alloc(ctx, std::max<size_t>(total, 1) * sizeof(Fr), (void**)&compact);
        for (size_t i = 0; i < count && s == JOLT_OK; ++i) {
            s = jolt_internal_gather_owned_terms(ctx, ptrs[i], lens[i], map, compact + off[i]);
            p[i] = compact + off[i];
        }
        if (s == JOLT_OK) s = jolt_internal_msm_many(ctx, srs, p.data(), n.data(), count, partial.data());  // every MSM multiplies a prefix of the compact SRS
        if (compact) jolt_internal_dev_free(ctx, compact);
        ls = s;
    } else {
        for (size_t i = 0; i < count; ++i) {
            const size_t lo = lens[i] * (size_t)rank / (size_t)world, hi = lens[i] * (size_t)(rank + 1) / (size_t)world;
            p[i] = ptrs[i] + lo;
            n[i] = hi - lo;
            off[i] = lo;
        }
        ls = jolt_internal_msm_many(ctx, srs, p.data(), n.data(), count, partial.data(), off.data());
    }
    static_assert(sizeof(G1Jac) == 3 * sizeof(jolt_fr_t), "a Jacobian point travels as three 32-byte words");
    // the partial points travel with this rank's status: a rank whose MSMs failed still enters the exchange and every rank returns its error
    std::vector<jolt_fr_t> raw;
    JOLT_TRY(gather_with_status(ctx, gather, user, ls, reinterpret_cast<const jolt_fr_t*>(partial.data()), 3 * count, world, &raw));
    std::memcpy(all.data(), raw.data(), raw.size() * sizeof(jolt_fr_t));
    for (size_t i = 0; i < count; ++i) {
        G1Jac acc = all[i];
        for (int r = 1; r < world; ++r) acc = g1_add(acc, all[(size_t)r * count + i]);
        out[i] = acc;
    }
    return JOLT_OK;
}

// The three witness commitments of kzg_open_batch (kzg.rs:108-116) from the commitments of ONE polynomial against shifted bases.  With u = r^2,
// B = q (X^2 - u) + alpha X + beta and q = Q3 (X - u) + a (a = q(u)), the witness polynomials are
//   h_r    = q (X + r) + alpha = Q3 (X - u)(X + r) + a (X + r) + alpha
//   h_(-r) = q (X - r) + alpha = Q3 (X - u)(X - r) + a (X - r) + alpha
//   h_u    = Q3 (X^2 - u) + a (X + u) + alpha                                  (B - B(u) = q (X^2 - u) - a (u^2 - u) + alpha (X - u))
// so with C_k = commit(X^k Q3), E = C2 + a G1 + alpha G0 and O = r C1 - (u r) C0 + (a r) G0:
//   w_r = E - u C1 + O,   w_(-r) = E - u C1 - O,   w_u = E - u C0 + (a u) G0
// The scalars are folded in Fr first, which leaves eight scalar multiplications that do not depend on one another.  Each takes a few tenths of a millisecond of host time and the
// opening waits for them behind its last reduction, so they run side by side on threads of their own (inline, should the process not get the threads): 0.24 ms in all.
// Built for the host as well (jolt_host_hyperkzg_witness_triple): the CPU suite holds it to the oracle's three commitments.
static void witness_triple_combine(const G1Jac c[3], const G1Jac& g0, const G1Jac& g1, const Fr& r, const Fr& a, const Fr& alpha, G1Jac w[3]) {
    const Fr u = mul(r, r);
    enum { R_C1, U_C1, UR_C0, U_C0, A_G1, AR_G0, AU_G0, ALPHA_G0, N_MUL };
    const G1Jac* const base[N_MUL] = {&c[1], &c[1], &c[0], &c[0], &g1, &g0, &g0, &g0};
    const Fr scalar[N_MUL] = {from_mont(r), from_mont(u), from_mont(mul(u, r)), from_mont(u), from_mont(a), from_mont(mul(a, r)), from_mont(mul(a, u)), from_mont(alpha)};
    G1Jac m[N_MUL];
    std::thread workers[N_MUL];
    for (int i = 0; i < N_MUL; ++i) {
        auto one = [&m, &base, &scalar, i]() { m[i] = g1_mul_canonical(*base[i], scalar[i].l); };
        try {
            if (i + 1 < N_MUL) workers[i] = std::thread(one);
        } catch (const std::system_error&) {
        }
        if (!workers[i].joinable()) one();
    }
    for (std::thread& t : workers) if (t.joinable()) t.join();
    const G1Jac e = g1_add(g1_add(c[2], m[A_G1]), m[ALPHA_G0]);
    const G1Jac o = g1_add(g1_add(m[R_C1], g1_neg(m[UR_C0])), m[AR_G0]);
    const G1Jac even = g1_add(e, g1_neg(m[U_C1]));
    w[0] = g1_add(even, o);
    w[1] = g1_add(even, g1_neg(o));
    w[2] = g1_add(g1_add(e, g1_neg(m[U_C0])), m[AU_G0]);
}
extern "C" int32_t jolt_host_hyperkzg_witness_triple(const jolt_g1_t* c, const jolt_g1_t* g0, const jolt_g1_t* g1, const jolt_fr_t* r, const jolt_fr_t* a,
                                                     const jolt_fr_t* alpha, jolt_g1_t* w) {
    if (!c || !g0 || !g1 || !r || !a || !alpha || !w) return JOLT_ERR_INVALID_ARG;
    G1Jac pts[5], out[3];
    std::memcpy(&pts[0], c, 3 * sizeof(G1Jac));
    std::memcpy(&pts[3], g0, sizeof(G1Jac));
    std::memcpy(&pts[4], g1, sizeof(G1Jac));
    for (const G1Jac& p : pts) if (!g1_is_on_curve(p)) return JOLT_ERR_INVALID_ARG;
    const Fr rr = fr_from_abi(r), aa = fr_from_abi(a), al = fr_from_abi(alpha);
    if (!fr_is_canonical(rr) || !fr_is_canonical(aa) || !fr_is_canonical(al)) return JOLT_ERR_INVALID_ARG;
    witness_triple_combine(pts, pts[3], pts[4], rr, aa, al, out);
    for (G1Jac& p : out) if (g1_is_identity(p)) p = g1_identity();
    std::memcpy(w, out, sizeof(out));
    return JOLT_OK;
}

// The first level commitments of an opening of the commitment grid's joint polynomial by LINEARITY (docs/kernels.md section 3.7b): the one-hot part from the hint's
// class sums (grid_hint.hpp; the combination runs on the hint's stream beside the level MSMs), the dense part as MSMs over the dense columns' folds (T >> s terms, in
// the same pipeline as the other levels' MSMs) -- no host round trip, nothing allocated outside the pool.
namespace {
struct GridLinear {
    const jolt_grid_hint* hint;
    const jolt_fr_t* onehot_scalars;  // n_cols
    jolt_table* const* dense;
    size_t n_dense;
    const jolt_fr_t* dense_scalars;
    uint32_t levels;
};
}  // namespace

// HyperKZGScheme::open (scheme.rs:122-158) + kzg_open_batch (kzg.rs:69-126)
static int32_t hyperkzg_open_impl(jolt_ctx* ctx, const jolt_srs* srs, const jolt_table* evals, const jolt_fr_t* point, size_t ell, uint64_t transcript_label,
                                  int rank, int world, size_t block, jolt_gather_fn gather, void* user, jolt_g1_t* com, jolt_g1_t* w, jolt_fr_t* v, jolt_fr_t* challenges_out,
                                  jolt_open_transcript_fn transcript_fn = nullptr, void* transcript_user = nullptr, const jolt_g1_t* known_levels = nullptr, size_t n_known = 0,
                                  const GridLinear* lin = nullptr, const Fr* expected_eval = nullptr) {
    if (!ctx || !srs || !evals || !point || !w || !v || (ell > 1 && !com)) return JOLT_ERR_INVALID_ARG;
    if (world < 1 || rank < 0 || rank >= world || (world > 1 && !gather)) return JOLT_ERR_INVALID_ARG;
    if (ell == 0) return JOLT_ERR_EMPTY_POINT;
    if (ell > 40) return JOLT_ERR_UNSUPPORTED;
    OpenTranscript tr{LabelledTranscript(transcript_label), transcript_fn, transcript_user};
    std::vector<jolt_table*> polys(ell, nullptr);
    auto cleanup = [&](jolt_table* extra1 = nullptr, jolt_table* extra2 = nullptr) {
        for (jolt_table* t : polys) if (t) jolt_table_free(ctx, t);
        if (extra1) jolt_table_free(ctx, extra1);
        if (extra2) jolt_table_free(ctx, extra2);
    };
    int32_t s = jolt_hyperkzg_fold(ctx, evals, point, ell, polys.data());  // phase 1
    if (s != JOLT_OK) { cleanup(); return s; }
    if (expected_eval) {
        // a batch's statement (jolt_host_hyperkzg_prove_batch): the last level's two entries give the polynomial's value at the point, p[0] + point[0] (p[1] - p[0]).
        // A statement that does not hold is refused here, before a level is committed and before the transcript absorbs one.
        Fr last[2];
        hipError_t e = hipMemcpyAsync(last, polys[ell - 1]->data(), sizeof(last), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) { (void)hipGetLastError(); ctx->last_error = std::string("hyperkzg open (statement check): ") + hipGetErrorString(e); cleanup(); return JOLT_ERR_HIP; }
        const Fr x0 = fr_from_abi(&point[0]);
        if (!fr_is_canonical(x0)) { ctx->last_error = "point coordinate is not a canonical Fr"; cleanup(); return JOLT_ERR_INVALID_ARG; }
        if (!(add(last[0], mul(x0, sub(last[1], last[0]))) == *expected_eval)) {
            ctx->last_error = "the claimed evaluations do not combine to the joint polynomial's evaluation at the point";
            cleanup();
            return JOLT_ERR_ROUND_CHECK;
        }
    }
    std::vector<G1Jac> coms(ell > 1 ? ell - 1 : 0);
    {  // scheme.rs:141-145: the ell-1 level commitments are independent MSMs -> pipelined over the MSM lanes
        // the first n_known level commitments come from the caller (computed by linearity from the structure of the polynomial: jolt_grid_commit_onehot_classes)
        if (n_known > coms.size() || (n_known && !known_levels) || (n_known && world != 1)) { cleanup(); return JOLT_ERR_INVALID_ARG; }
        for (size_t i = 0; i < n_known; ++i) {
            std::memcpy(&coms[i], &known_levels[i], sizeof(G1Jac));
            if (!g1_is_on_curve(coms[i])) {  // caller-supplied points are absorbed into the transcript and returned in the proof: at least they are points
                ctx->last_error = "a supplied level commitment is not a point of BN254 G1 (coordinates not canonical or off the curve)";
                cleanup();
                return JOLT_ERR_INVALID_ARG;
            }
        }
        // levels by linearity: the one-hot part's combination goes on the hint's stream now, the dense folds' MSMs join the other levels' below
        size_t n_lin = 0;
        G1Jac* d_small = nullptr;
        void* d_temp = nullptr;
        std::vector<jolt_table*> dense_levels;
        jolt_table* dense_rlc = nullptr;
        auto lin_cleanup = [&]() {
            // the combination runs on the hint's stream and the pool hands freed blocks to main-stream work at once: on every exit the buffers go back only after
            // that stream has drained (a no-op after the download below, which has waited for it already)
            if ((d_small || d_temp) && lin && lin->hint && lin->hint->stream != ctx->stream) (void)hipStreamSynchronize(lin->hint->stream);
            if (d_small) jolt_internal_dev_free(ctx, d_small);
            if (d_temp) jolt_internal_dev_free(ctx, d_temp);
            for (jolt_table* t : dense_levels) if (t) jolt_table_free(ctx, t);
            if (dense_rlc) jolt_table_free(ctx, dense_rlc);
            d_small = nullptr;
            d_temp = nullptr;
            dense_levels.clear();
            dense_rlc = nullptr;
        };
        if (lin && lin->hint && world == 1 && n_known == 0) {
            const jolt_grid_hint* h = lin->hint;
            size_t log_t = 0;
            while (((size_t)1 << log_t) < h->cycles) ++log_t;
            n_lin = std::min<size_t>({(size_t)lin->levels, (size_t)h->levels, coms.size(), log_t ? log_t - 1 : 0});  // (the dense folds exist down to 2 coefficients)
            if ((size_t)h->k * h->cycles != evals->len || (lin->n_dense && (!lin->dense || !lin->dense_scalars)) || !lin->onehot_scalars) { cleanup(); return JOLT_ERR_INVALID_ARG; }
            if (n_lin) {
                std::vector<Fr> sc(h->n_cols), xs(n_lin);
                for (size_t p = 0; p < h->n_cols; ++p) sc[p] = fr_from_abi(&lin->onehot_scalars[p]);
                for (size_t b = 0; b < n_lin; ++b) xs[b] = fr_from_abi(&point[ell - 1 - b]);  // fold i uses point[ell - i] (scheme.rs:97-98)
                s = jolt_internal_grid_hint_combine(ctx, h, (uint32_t)n_lin, sc.data(), xs.data(), &d_small, &d_temp);
                if (s == JOLT_OK && lin->n_dense) {
                    for (size_t dd = 0; dd < lin->n_dense && s == JOLT_OK; ++dd)
                        if (!lin->dense[dd] || lin->dense[dd]->len != h->cycles) s = JOLT_ERR_SIZE_MISMATCH;
                    if (s == JOLT_OK) s = jolt_rlc(ctx, lin->dense, lin->n_dense, lin->dense_scalars, &dense_rlc);  // the dense part of row 0: T coefficients
                    if (s == JOLT_OK) {
                        dense_levels.assign(log_t, nullptr);
                        s = jolt_hyperkzg_fold(ctx, dense_rlc, point + (ell - log_t), log_t, dense_levels.data());  // its folds by the same low variables
                    }
                }
                if (s != JOLT_OK) { lin_cleanup(); cleanup(); return s; }
            }
        }
        const size_t first_msm = std::max(n_known, n_lin);
        std::vector<const Fr*> ptrs;
        std::vector<size_t> lens;
        for (size_t i = 1 + first_msm; i < ell; ++i) { ptrs.push_back(polys[i]->data()); lens.push_back(polys[i]->len); }
        const size_t n_level_msms = ptrs.size();
        if (n_lin && dense_rlc)
            for (size_t s_ = 1; s_ <= n_lin; ++s_) { ptrs.push_back(dense_levels[s_]->data()); lens.push_back(dense_levels[s_]->len); }
        std::vector<G1Jac> msm_out(ptrs.size());
        ctx->msm_full_width_scalars = true;  // folds by challenges: uniform field elements whatever the committed polynomial held
        s = ptrs.empty() ? JOLT_OK : sharded_msm_many(ctx, srs, ptrs, lens, rank, world, block, gather, user, msm_out.data());
        ctx->msm_full_width_scalars = false;
        if (s == JOLT_OK && n_lin) {
            std::vector<G1Jac> small(n_lin);
            hipError_t e = hipMemcpyAsync(small.data(), d_small, n_lin * sizeof(G1Jac), hipMemcpyDeviceToHost, lin->hint->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(lin->hint->stream);
            if (e != hipSuccess) { (void)hipGetLastError(); ctx->last_error = std::string("hyperkzg open (levels by linearity): ") + hipGetErrorString(e); s = JOLT_ERR_HIP; }
            for (size_t i = 0; i < n_lin && s == JOLT_OK; ++i) coms[i] = dense_rlc ? g1_add(small[i], msm_out[n_level_msms + i]) : small[i];
        } else if (n_lin) {
            (void)hipStreamSynchronize(lin->hint->stream);  // the combination still reads d_temp
        }
        for (size_t i = 0; i < n_level_msms && s == JOLT_OK; ++i) coms[first_msm + i] = msm_out[i];
        lin_cleanup();
        if (s != JOLT_OK) { cleanup(); return s; }
    }
    Fr r;  // phase 2 (scheme.rs:148-152)
    s = tr.after_points(0, coms.data(), coms.size(), &r);
    if (s != JOLT_OK) { cleanup(); return s; }
    Fr u[3] = {r, neg(r), mul(r, r)};
    jolt_fr_t u_abi[3];
    for (int t = 0; t < 3; ++t) fr_to_abi(&u_abi[t], u[t]);
    // One GPU, at least two variables (an even length >= 4): the evaluations come out of the heads pass of the quotient scan below (open_level_heads), run on the
    // levels before q exists.
    const bool from_heads = world == 1 && ell >= 2;
    OpenLevelHeads level_heads;
    struct FreeHeads { jolt_ctx* c; OpenLevelHeads* h; ~FreeHeads() { if (h->heads) jolt_internal_dev_free(c, h->heads); } } free_heads{ctx, &level_heads};
    if (from_heads) s = open_level_heads(ctx, polys.data(), ell, r, point, v, &level_heads);
    else s = jolt_hyperkzg_eval3(ctx, polys.data(), ell, u_abi, v);  // kzg.rs:84-85
    if (s != JOLT_OK) { cleanup(); return s; }
    Fr q;  // kzg.rs:88-95: every v[t][j], row-major
    s = tr.after_values(1, v, 3 * ell, &q);
    if (s != JOLT_OK) { cleanup(); return s; }
    jolt_fr_t q_abi;
    fr_to_abi(&q_abi, q);
    jolt_table* b_poly = nullptr;
    s = jolt_hyperkzg_rlc(ctx, polys.data(), ell, &q_abi, &b_poly);  // kzg.rs:95-105
    if (s != JOLT_OK) { cleanup(); return s; }
    G1Jac ws[3];
    bool paired = false;
    if (world == 1 && b_poly->len >= 4) {
        // ALL THREE witness commitments from ONE sorted scalar vector.  B = q (X^2 - r^2) + alpha X + beta, and one more linear division q = Q3 (X - r^2) + a: the three
        // witness polynomials are Q3 times a monic quadratic plus a linear remainder each (witness_triple_combine above), so with C_k = commit(X^k Q3) -- the same scalars
        // against the bases shifted by k = 0, 1, 2: three bucket passes over one digit sort (jolt_internal_msm_fixed_enqueue with base shifts) -- the host combines the
        // same group elements kzg.rs:108-116 commits to.  h_(r^2) is never built, and the second lane sorts nothing.
        // q in ONE pass over B when its length is even (every opening of >= 2 variables): q[k] = B[k + 2] + r^2 q[k + 2], two interleaved chains (suffix_scan<2>), and
        // alpha = B[1] + r^2 q[1] (the X^1 coefficient of B = q (X^2 - r^2) + alpha X + beta); otherwise two divisions, by (X - r) and then by (X + r), whose second
        // remainder h_r[0] + q[0] (-r) is alpha.  Q3[k] = q[k + 1] + r^2 Q3[k + 1] (len - 3 coefficients), a = q[0] + r^2 Q3[0].
        // The scan's heads are there since the evaluations (open_level_heads, open_quotient).
        jolt_table *h0 = nullptr, *qp = nullptr, *q3 = nullptr;
        bool direct = false;
        const size_t q3_len = b_poly->len - 3;
        if (srs->n < 2 || q3_len > srs->n - 2) s = JOLT_ERR_SRS_TOO_SMALL;  // (what the three commitments of len - 1 coefficients need)
        if (s == JOLT_OK && from_heads) {
            s = jolt_internal_table_new(ctx, b_poly->len - 2, &qp);
            if (s == JOLT_OK) {
                const int32_t qs = open_quotient(ctx, level_heads, q, u[2], b_poly->data(), qp->data());
                if (qs == JOLT_OK) direct = true;
                else if (qs == JOLT_ERR_UNSUPPORTED) { jolt_table_free(ctx, qp); qp = nullptr; }
                else s = qs;
            }
        }
        if (s == JOLT_OK && !direct) {
            s = jolt_hyperkzg_witness_poly(ctx, b_poly, &u_abi[0], &h0);
            if (s == JOLT_OK) s = jolt_hyperkzg_witness_poly(ctx, h0, &u_abi[1], &qp);
        }
        if (s == JOLT_OK) s = jolt_hyperkzg_witness_poly(ctx, qp, &u_abi[2], &q3);
        // the five words and two points the combination needs go to the pinned result buffer BEHIND the scans and AHEAD of the MSMs on the main stream: the collect
        // step's synchronisation is the only one.  [0], [1]: direct: B[1], q[1]; else h_r[0], q[0];  [2]: q[0];  [3]: Q3[0];  [4..8): G_0, G_1
        static_assert(2 * sizeof(G1Affine) == 4 * sizeof(Fr), "two affine points take four result slots");
        if (s == JOLT_OK) s = jolt_internal_ensure_scratch(ctx, 1, 8);
        if (s == JOLT_OK) {
            Fr* hr = ctx->h_results;
            hipError_t e = hipMemcpyAsync(&hr[0], direct ? b_poly->data() + 1 : h0->data(), sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(&hr[1], direct ? qp->data() + 1 : qp->data(), sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(&hr[2], qp->data(), sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(&hr[3], q3->data(), sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(&hr[4], srs->pts, 2 * sizeof(G1Affine), hipMemcpyDeviceToHost, ctx->stream);
            if (e != hipSuccess) { (void)hipStreamSynchronize(ctx->stream); ctx->last_error = std::string("hyperkzg open: ") + hipGetErrorString(e); s = JOLT_ERR_HIP; }
        }
        if (s == JOLT_OK) {
            G1Jac three[3];
            const size_t shifts[3] = {0, 1, 2};
            ctx->msm_full_width_scalars = ctx->msm_uniform_scalars = true;  // quotients of the random linear combination: uniform field elements (lets the sort use capacity regions, msm_fixed.hip 2d)
            const int32_t ts = jolt_internal_msm_shifted(ctx, srs, q3->data(), q3->len, shifts, 3, three);  // lane 0 = the main stream: ordered behind Q3's producer
            ctx->msm_full_width_scalars = ctx->msm_uniform_scalars = false;
            if (ts == JOLT_OK) {
                const Fr* hr = ctx->h_results;
                G1Affine g01[2];
                std::memcpy(g01, &hr[4], sizeof(g01));
                const Fr alpha = add(hr[0], mul(hr[1], direct ? u[2] : u[1])), a = add(hr[2], mul(hr[3], u[2]));
                witness_triple_combine(three, g1_from_affine(g01[0]), g1_from_affine(g01[1]), r, a, alpha, ws);
                paired = true;
            } else if (ts != JOLT_ERR_UNSUPPORTED) {
                s = ts;
            }
        }
        for (jolt_table* t : {h0, qp, q3}) if (t) jolt_table_free(ctx, t);
        if (s != JOLT_OK) { cleanup(b_poly); return s; }
    }
    if (!paired) {  // kzg.rs:108-116: three witness polynomials, then their three independent MSMs on the MSM lanes
        jolt_table* h[3] = {nullptr, nullptr, nullptr};
        std::vector<const Fr*> ptrs;
        std::vector<size_t> lens;
        for (int t = 0; t < 3 && s == JOLT_OK; ++t) {
            s = jolt_hyperkzg_witness_poly(ctx, b_poly, &u_abi[t], &h[t]);
            if (s == JOLT_OK) { ptrs.push_back(h[t]->data()); lens.push_back(h[t]->len); }
        }
        if (s == JOLT_OK) s = sharded_msm_many(ctx, srs, ptrs, lens, rank, world, block, gather, user, ws);
        for (int t = 0; t < 3; ++t) if (h[t]) jolt_table_free(ctx, h[t]);
        if (s != JOLT_OK) { cleanup(b_poly); return s; }
    }
    Fr d0;  // kzg.rs:118-124
    s = tr.after_points(2, ws, 3, &d0);
    if (s != JOLT_OK) { cleanup(b_poly); return s; }
    for (size_t i = 0; i + 1 < ell; ++i) std::memcpy(&com[i], &coms[i], sizeof(G1Jac));
    for (int t = 0; t < 3; ++t) std::memcpy(&w[t], &ws[t], sizeof(G1Jac));
    if (challenges_out) { fr_to_abi(&challenges_out[0], r); fr_to_abi(&challenges_out[1], q); fr_to_abi(&challenges_out[2], d0); }
    cleanup(b_poly);
    return JOLT_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// HyperKZGScheme::open with the POLYNOMIAL sharded over the ranks (subtree assignment, term_map.hip.h; tests/subtree_model.py is the
// executable specification this follows step by step).  Rank g holds the 2^(ell - gamma) coefficients it owns as a compact array
// and its compact SRS; folds, RLC, Horner passes, quotient scans and MSMs all run on 1 / world of the data.  What crosses ranks, through
// `gather` (32-byte words): ell - gamma + 1 words after the folds (subtree roots + crown), 3 (ell - 1) + 9 words of partial points,
// 3 (ell - gamma) words of partial evaluations, 3 (ell - gamma) + 1 words of segment sums before the quotient scans.
// ------------------------------------------------------------------------------------------------------------------
namespace {
int32_t read_slot(jolt_ctx* ctx, const jolt_table* t, size_t slot, Fr* out) {
    JOLT_HIP_TRY(ctx, hipMemcpyAsync(out, t->data() + slot, sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
    return JOLT_OK;
}
int32_t write_slot(jolt_ctx* ctx, Fr* dst, const Fr& v) {  // pageable source: the copy is staged before the call returns
    JOLT_HIP_TRY(ctx, hipMemcpyAsync(dst, &v, sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
    return JOLT_OK;
}
// Every exchange of the sharded opening carries the sender's status in one extra 32-byte word.  A rank whose LOCAL work failed (an allocation, a
// launch) still takes part in the next exchange -- with a zero payload -- and every rank leaves with the first failing rank's status, instead of
// the healthy ranks blocking in a collective the failing rank never enters (the shared-memory exchange would time out, RCCL would hang).
int32_t gather_with_status(jolt_ctx* ctx, jolt_gather_fn gather, void* user, int32_t local_status, const jolt_fr_t* payload, size_t count, int world, std::vector<jolt_fr_t>* all) {
    std::vector<jolt_fr_t> send(count + 1), recv((count + 1) * (size_t)world);
    std::memset(send.data(), 0, send.size() * sizeof(jolt_fr_t));
    send[0].l[0] = (uint64_t)(uint32_t)local_status;
    if (local_status == JOLT_OK && count) std::memcpy(&send[1], payload, count * sizeof(jolt_fr_t));
    ctx->d_round_count = 0;  // these words are not the round sums of the context's last batch round (jolt_comm_gather_round_sums' shortcut)
    const int32_t gs = gather(user, send.data(), count + 1, recv.data());
    if (gs != JOLT_OK) return gs;  // the collective itself failed: nothing left to agree on
    all->resize(count * (size_t)world);
    int32_t first = JOLT_OK;
    for (int r = 0; r < world; ++r) {
        const int32_t st = (int32_t)(uint32_t)recv[(size_t)r * (count + 1)].l[0];
        if (st != JOLT_OK && first == JOLT_OK) first = st;
        if (count) std::memcpy(all->data() + (size_t)r * count, &recv[(size_t)r * (count + 1) + 1], count * sizeof(jolt_fr_t));
    }
    return local_status != JOLT_OK ? local_status : first;
}
int32_t gather_words(jolt_ctx* ctx, jolt_gather_fn gather, void* user, int32_t local_status, const std::vector<Fr>& local, int world, std::vector<Fr>* all) {
    std::vector<jolt_fr_t> raw;
    JOLT_TRY(gather_with_status(ctx, gather, user, local_status, reinterpret_cast<const jolt_fr_t*>(local.data()), local.size(), world, &raw));
    all->resize(raw.size());
    if (!raw.empty()) std::memcpy(all->data(), raw.data(), raw.size() * sizeof(jolt_fr_t));
    return JOLT_OK;
}
// partial points of `count` MSMs -> the sums over the ranks, in rank order on every rank
int32_t gather_points(jolt_ctx* ctx, jolt_gather_fn gather, void* user, int32_t local_status, const std::vector<G1Jac>& partial, int world, G1Jac* out) {
    const size_t count = partial.size();
    std::vector<jolt_fr_t> raw;
    JOLT_TRY(gather_with_status(ctx, gather, user, local_status, reinterpret_cast<const jolt_fr_t*>(partial.data()), 3 * count, world, &raw));
    const G1Jac* all = reinterpret_cast<const G1Jac*>(raw.data());
    for (size_t i = 0; i < count; ++i) {
        G1Jac acc = all[i];
        for (int r = 1; r < world; ++r) acc = g1_add(acc, all[(size_t)r * count + i]);
        out[i] = acc;
    }
    return JOLT_OK;
}
}  // namespace

extern "C" int32_t jolt_host_hyperkzg_open_subtree(jolt_ctx* ctx, const jolt_srs* srs, const jolt_table* evals, const jolt_fr_t* point, size_t ell,
                                                   uint64_t transcript_label, int32_t rank, int32_t world, jolt_gather_fn gather, void* user, jolt_g1_t* com,
                                                   jolt_g1_t* w, jolt_fr_t* v, jolt_fr_t* challenges_out) {
    if (!ctx || !srs || !evals || !point || !w || !v || !gather || (ell > 1 && !com)) return JOLT_ERR_INVALID_ARG;
    TermMap map;
    if (world < 2 || !make_subtree_map(rank, world, &map)) return JOLT_ERR_INVALID_ARG;  // one rank: jolt_host_hyperkzg_open
    if (ell > 40) return JOLT_ERR_UNSUPPORTED;
    const size_t gamma = map.gamma, G = (size_t)world;
    if (ell <= gamma) return JOLT_ERR_UNSUPPORTED;  // every rank owns at least two coefficients
    const size_t lam = ell - gamma;
    if (evals->len != ((size_t)1 << lam)) return JOLT_ERR_SIZE_MISMATCH;
    if (srs->n < evals->len) return JOLT_ERR_SRS_TOO_SMALL;
    LabelledTranscript tr(transcript_label);
    std::vector<Fr> x(ell);
    for (size_t i = 0; i < ell; ++i) {
        x[i] = fr_from_abi(&point[i]);
        JOLT_REQUIRE(ctx, fr_is_canonical(x[i]), "point coordinate is not a canonical Fr");
    }
    std::vector<jolt_table*> polys(ell, nullptr);
    jolt_table* b_poly = nullptr;
    jolt_table* h[3] = {nullptr, nullptr, nullptr};
    auto cleanup = [&]() {
        for (jolt_table* t : polys) if (t) jolt_table_free(ctx, t);
        if (b_poly) jolt_table_free(ctx, b_poly);
        for (jolt_table* t : h) if (t) jolt_table_free(ctx, t);
    };
    // local work: SUB_TRY records the first failure and skips what follows; the next exchange (gather_* with the status word) makes every rank leave together
    int32_t ls = JOLT_OK;
#define SUB_TRY(expr) do { if (ls == JOLT_OK) ls = (expr); } while (0)
#define SUB_EXCHANGE(expr) do { const int32_t s_ = (expr); if (s_ != JOLT_OK) { cleanup(); return s_; } } while (0)
    // phase 1a: the local folds -- fold i uses point[ell - i]; the compact arrays of levels 0 .. lam-1 have >= 2 slots
    SUB_TRY(jolt_hyperkzg_fold(ctx, evals, point + gamma, lam, polys.data()));
    // phase 1b: every rank publishes slot 1 of each of those levels (its subtree's root, index G + g) and slot 0 of level 0; the
    // crowns (indices below G) of all levels follow from these on every rank
    std::vector<Fr> local(lam + 1), all;
    for (size_t k = 0; k < lam && ls == JOLT_OK; ++k) ls = read_slot(ctx, polys[k], 1, &local[k]);
    if (ls == JOLT_OK) ls = read_slot(ctx, polys[0], 0, &local[lam]);
    if (ls == JOLT_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) ls = JOLT_ERR_HIP;
    SUB_EXCHANGE(gather_words(ctx, gather, user, ls, local, world, &all));
    std::vector<std::vector<Fr>> crowns(ell);
    crowns[0].resize(G);
    for (size_t g = 0; g < G; ++g) crowns[0][g] = all[g * (lam + 1) + lam];
    for (size_t k = 1; k < ell; ++k) {
        std::vector<Fr> prev = crowns[k - 1];
        if (k - 1 < lam)
            for (size_t g = 0; g < G; ++g) prev.push_back(all[g * (lam + 1) + (k - 1)]);  // indices [G, 2G) of level k-1
        const Fr xk = x[ell - k];
        crowns[k].resize(prev.size() / 2);
        for (size_t y = 0; y < crowns[k].size(); ++y) crowns[k][y] = add(prev[2 * y], mul(xk, sub(prev[2 * y + 1], prev[2 * y])));
    }
    for (size_t k = 1; k < ell && ls == JOLT_OK; ++k) {
        if (k < lam) {
            ls = write_slot(ctx, polys[k]->data(), crowns[k][(size_t)rank]);
        } else {  // levels of at most G coefficients: the crown alone
            const size_t len = (size_t)rank < crowns[k].size() ? 1 : 0;
            ls = jolt_internal_table_new(ctx, len, &polys[k]);
            if (ls == JOLT_OK && len) ls = write_slot(ctx, polys[k]->data(), crowns[k][(size_t)rank]);
        }
    }
    // phase 1c: level commitments over the compact SRS (every level is a prefix of it)
    std::vector<G1Jac> coms(ell > 1 ? ell - 1 : 0);
    if (ell > 1) {
        std::vector<const Fr*> ptrs;
        std::vector<size_t> lens;
        std::vector<G1Jac> partial(ell - 1);
        if (ls == JOLT_OK) {
            for (size_t i = 1; i < ell; ++i) { ptrs.push_back(polys[i]->data()); lens.push_back(polys[i]->len); }
            ls = jolt_internal_msm_many(ctx, srs, ptrs.data(), lens.data(), ell - 1, partial.data());
        }
        SUB_EXCHANGE(gather_points(ctx, gather, user, ls, partial, world, coms.data()));
    }
    for (const G1Jac& c : coms) append_g1(tr, c);  // phase 2 (scheme.rs:148-152)
    const Fr r = tr.challenge();
    const Fr u[3] = {r, neg(r), mul(r, r)};
    // evaluations (kzg.rs:84-85): levels with a compact array on the device (slot i weighs u^index(i)), crown-only levels on the host
    std::vector<Fr> vals(3 * ell, Fr::zero());
    {
        Fr3 uu, u16, u4096;
        for (int t = 0; t < 3; ++t) {
            uu.v[t] = u[t];
            Fr p = u[t];
            for (int i = 0; i < 4; ++i) p = sqr(p);
            u16.v[t] = p;
            for (int i = 0; i < 8; ++i) p = sqr(p);
            u4096.v[t] = p;
        }
        SUB_TRY(jolt_internal_ensure_scratch(ctx, 1, 3 * ell + 8));
        Fr* chunk_weights = nullptr;
        SUB_TRY(jolt_internal_dev_alloc(ctx, 3 * kBlock * sizeof(Fr), (void**)&chunk_weights));
        if (ls == JOLT_OK) hipLaunchKernelGGL(k_power_table3, dim3(1), dim3(kBlock), 0, ctx->stream, u16, chunk_weights);
        int32_t es = ls;
        for (size_t j = 0; j < lam && es == JOLT_OK; ++j) {
            const jolt_table* t = polys[j];
            const size_t per_block = (size_t)kBlock * kHornerChunk;
            const int grid = (int)std::max<size_t>(1, (t->len + per_block - 1) / per_block);
            es = jolt_internal_ensure_scratch(ctx, (size_t)grid * 3, 3 * ell + 8);
            if (es != JOLT_OK) break;
            hipLaunchKernelGGL(k_horner3<true>, dim3(grid), dim3(kBlock), 0, ctx->stream, (const Fr*)t->data(), t->len, uu, (const Fr*)chunk_weights, u4096, ctx->d_partials, map);
            hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(kBlock), 0, ctx->stream, (const Fr*)ctx->d_partials, grid, 3, ctx->d_results + 3 * j);
            if (hipGetLastError() != hipSuccess) es = JOLT_ERR_HIP;
        }
        if (chunk_weights) jolt_internal_dev_free(ctx, chunk_weights);  // stream-ordered
        SUB_TRY(es);
        std::vector<Fr> part(3 * lam, Fr::zero());
        if (ls == JOLT_OK && (hipMemcpyAsync(part.data(), ctx->d_results, 3 * lam * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
                              hipStreamSynchronize(ctx->stream) != hipSuccess)) ls = JOLT_ERR_HIP;
        SUB_EXCHANGE(gather_words(ctx, gather, user, ls, part, world, &all));
        for (size_t j = 0; j < lam; ++j)
            for (int t = 0; t < 3; ++t) {
                Fr acc = Fr::zero();
                for (size_t g = 0; g < G; ++g) acc = add(acc, all[g * 3 * lam + 3 * j + t]);
                vals[(size_t)t * ell + j] = acc;
            }
        for (size_t j = lam; j < ell; ++j)
            for (int t = 0; t < 3; ++t) {
                Fr acc = Fr::zero();
                for (size_t y = crowns[j].size(); y-- > 0;) acc = add(mul(acc, u[t]), crowns[j][y]);
                vals[(size_t)t * ell + j] = acc;
            }
    }
    for (size_t i = 0; i < 3 * ell; ++i) fr_to_abi(&v[i], vals[i]);
    for (int t = 0; t < 3; ++t)
        for (size_t j = 0; j < ell; ++j) tr.append_fr(vals[(size_t)t * ell + j]);  // kzg.rs:88-92
    const Fr q = tr.challenge();
    jolt_fr_t q_abi;
    fr_to_abi(&q_abi, q);
    SUB_TRY(jolt_hyperkzg_rlc(ctx, polys.data(), ell, &q_abi, &b_poly));  // kzg.rs:95-105: slot-wise on the compact arrays
    // witness polynomials (kzg.rs:34-46, 108-116).  A rank's segments [2^L, 2^(L+1)) are contiguous index ranges; the quotient scan of a
    // segment [a, b) starts from the carry E(b) = sum_{i >= b} B[i] u^(i - b).  Every rank publishes the Horner sum of each of its
    // segments (three points) and its crown value; the chain of carries is evaluated identically on every rank.
    {
        Fr3 uu, u16, u4096;
        for (int t = 0; t < 3; ++t) {
            uu.v[t] = u[t];
            Fr p = u[t];
            for (int i = 0; i < 4; ++i) p = sqr(p);
            u16.v[t] = p;
            for (int i = 0; i < 8; ++i) p = sqr(p);
            u4096.v[t] = p;
        }
        SUB_TRY(jolt_internal_ensure_scratch(ctx, 1, 3 * ell + 8));
        Fr* chunk_weights = nullptr;
        SUB_TRY(jolt_internal_dev_alloc(ctx, 3 * kBlock * sizeof(Fr), (void**)&chunk_weights));
        if (ls == JOLT_OK) hipLaunchKernelGGL(k_power_table3, dim3(1), dim3(kBlock), 0, ctx->stream, u16, chunk_weights);
        int32_t es = ls;
        for (size_t L = 0; L < lam && es == JOLT_OK; ++L) {  // segment L = slots [2^L, 2^(L+1)): a plain Horner sum from its first slot
            const size_t len = (size_t)1 << L, per_block = (size_t)kBlock * kHornerChunk;
            const int grid = (int)std::max<size_t>(1, (len + per_block - 1) / per_block);
            es = jolt_internal_ensure_scratch(ctx, (size_t)grid * 3, 3 * ell + 8);
            if (es != JOLT_OK) break;
            hipLaunchKernelGGL(k_horner3<false>, dim3(grid), dim3(kBlock), 0, ctx->stream, (const Fr*)(b_poly->data() + len), len, uu, (const Fr*)chunk_weights, u4096, ctx->d_partials,
                               TermMap{});
            hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(kBlock), 0, ctx->stream, (const Fr*)ctx->d_partials, grid, 3, ctx->d_results + 3 * L);
            if (hipGetLastError() != hipSuccess) es = JOLT_ERR_HIP;
        }
        if (chunk_weights) jolt_internal_dev_free(ctx, chunk_weights);
        SUB_TRY(es);
        std::vector<Fr> sums(3 * lam + 1, Fr::zero());
        if (ls == JOLT_OK && hipMemcpyAsync(sums.data(), ctx->d_results, 3 * lam * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) ls = JOLT_ERR_HIP;
        SUB_TRY(read_slot(ctx, b_poly, 0, &sums[3 * lam]));
        if (ls == JOLT_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) ls = JOLT_ERR_HIP;
        SUB_EXCHANGE(gather_words(ctx, gather, user, ls, sums, world, &all));
        const size_t stride = 3 * lam + 1;
        const size_t n_h = ((size_t)1 << lam) - ((size_t)rank + 1 == G ? 1 : 0);  // the quotient has 2^ell - 1 coefficients: the owner of the last index holds one less
        std::vector<Fr> carries[3];  // kept until the MSMs below have synchronised: sources of small host-to-device copies
        for (int t = 0; t < 3; ++t) {
            // carries, from the top index down: layers L = lam-1 .. 0 (ranks G-1 .. 0 inside a layer), then the crown G-1 .. 0
            std::vector<Fr>& carry = carries[t];  // this rank's: carry[L] enters segment L, carry[lam] enters the crown slot
            carry.assign(lam + 1, Fr::zero());
            Fr e = Fr::zero(), upow = u[t];
            std::vector<Fr> u_len(lam);  // u^(2^L)
            for (size_t L = 0; L < lam; ++L) { u_len[L] = upow; upow = sqr(upow); }
            for (size_t L = lam; L-- > 0;)
                for (size_t g = G; g-- > 0;) {
                    if (g == (size_t)rank) carry[L] = e;
                    e = add(all[g * stride + 3 * L + t], mul(u_len[L], e));
                }
            for (size_t g = G; g-- > 0;) {
                if (g == (size_t)rank) carry[lam] = e;
                e = add(all[g * stride + 3 * lam], mul(u[t], e));
            }
            SUB_TRY(jolt_internal_table_new(ctx, (size_t)1 << lam, &h[t]));
            if (ls != JOLT_OK) break;
            Fr* hd = h[t]->data();
            SUB_TRY(write_slot(ctx, hd, carry[lam]));  // h[g] = s[g + 1] = E(g + 1)
            for (size_t L = 0; L < lam; ++L) {
                const size_t lo = (size_t)1 << L, len = lo;
                SUB_TRY(write_slot(ctx, hd + lo + len - 1, carry[L]));  // the segment's top entry is the carry itself
                if (len > 1) SUB_TRY(suffix_horner(ctx, b_poly->data() + lo, len, u[t], hd + lo, 1, carry[L]));
            }
            h[t]->len = n_h;
        }
        if (ls == JOLT_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) ls = JOLT_ERR_HIP;
    }
    G1Jac ws[3];
    {
        std::vector<G1Jac> partial(3);
        if (ls == JOLT_OK) {
            const Fr* ptrs[3] = {h[0]->data(), h[1]->data(), h[2]->data()};
            const size_t lens[3] = {h[0]->len, h[1]->len, h[2]->len};
            ls = jolt_internal_msm_many(ctx, srs, ptrs, lens, 3, partial.data());
        }
        SUB_EXCHANGE(gather_points(ctx, gather, user, ls, partial, world, ws));
    }
#undef SUB_TRY
#undef SUB_EXCHANGE
    for (int t = 0; t < 3; ++t) append_g1(tr, ws[t]);  // kzg.rs:118-124
    const Fr d0 = tr.challenge();
    for (size_t i = 0; i + 1 < ell; ++i) std::memcpy(&com[i], &coms[i], sizeof(G1Jac));
    for (int t = 0; t < 3; ++t) std::memcpy(&w[t], &ws[t], sizeof(G1Jac));
    if (challenges_out) { fr_to_abi(&challenges_out[0], r); fr_to_abi(&challenges_out[1], q); fr_to_abi(&challenges_out[2], d0); }
    cleanup();
    return JOLT_OK;
}

extern "C" int32_t jolt_host_hyperkzg_open(jolt_ctx* ctx, const jolt_srs* srs, const jolt_table* evals, const jolt_fr_t* point, size_t ell,
                                           uint64_t transcript_label, jolt_g1_t* com, jolt_g1_t* w, jolt_fr_t* v, jolt_fr_t* challenges_out) {
    return hyperkzg_open_impl(ctx, srs, evals, point, ell, transcript_label, 0, 1, 0, nullptr, nullptr, com, w, v, challenges_out);
}
// The same opening under the CALLER's transcript (CommitmentScheme::open takes `transcript: &mut impl Transcript`, crates/jolt-openings/src/schemes.rs:66-72): `fn`
// absorbs what the prover sends at each of the three steps and returns the challenge drawn after it.
extern "C" int32_t jolt_host_hyperkzg_open_with_transcript(jolt_ctx* ctx, const jolt_srs* srs, const jolt_table* evals, const jolt_fr_t* point, size_t ell,
                                                           jolt_open_transcript_fn fn, void* user, jolt_g1_t* com, jolt_g1_t* w, jolt_fr_t* v, jolt_fr_t* challenges_out) {
    if (!fn) return JOLT_ERR_INVALID_ARG;
    return hyperkzg_open_impl(ctx, srs, evals, point, ell, 0, 0, 1, 0, nullptr, nullptr, com, w, v, challenges_out, fn, user);
}


// The same opening with its first n_known level commitments SUPPLIED by the caller -- computed by linearity from the structure of the polynomial (the joint polynomial
// of one-hot and dense columns: jolt_grid_commit_onehot_classes) instead of by MSM over the folded coefficients.  They are absorbed and returned like the computed ones:
// a wrong one yields a proof the verifier rejects, nothing else.  fn == NULL: the library's test transcript with `transcript_label`.
extern "C" int32_t jolt_host_hyperkzg_open_with_levels(jolt_ctx* ctx, const jolt_srs* srs, const jolt_table* evals, const jolt_fr_t* point, size_t ell,
                                                       uint64_t transcript_label, jolt_open_transcript_fn fn, void* user, const jolt_g1_t* known_levels, size_t n_known,
                                                       jolt_g1_t* com, jolt_g1_t* w, jolt_fr_t* v, jolt_fr_t* challenges_out) {
    return hyperkzg_open_impl(ctx, srs, evals, point, ell, transcript_label, 0, 1, 0, nullptr, nullptr, com, w, v, challenges_out, fn, user, known_levels, n_known);
}

// The opening of the commitment grid's joint polynomial (jolt_grid_joint_polynomial: `evals`, 2^ell = K * T coefficients) with its first `levels` level commitments
// by linearity from the commit-time hint (jolt_grid_hint_begin over the same one-hot sources, onehot_scalars in their column order) and the dense columns
// (`dense` of T entries each with dense_scalars: the same arguments jolt_grid_joint_polynomial took).  The same proof as jolt_host_hyperkzg_open of `evals`.
extern "C" int32_t jolt_host_hyperkzg_open_grid(jolt_ctx* ctx, const jolt_srs* srs, const jolt_table* evals, const jolt_fr_t* point, size_t ell, uint64_t transcript_label,
                                                jolt_open_transcript_fn fn, void* user, const jolt_grid_hint* hint, uint32_t levels, const jolt_fr_t* onehot_scalars,
                                                jolt_table* const* dense, size_t n_dense, const jolt_fr_t* dense_scalars, jolt_g1_t* com, jolt_g1_t* w, jolt_fr_t* v,
                                                jolt_fr_t* challenges_out) {
    if (!hint || !onehot_scalars || hint->ctx != ctx) return JOLT_ERR_INVALID_ARG;
    const GridLinear lin{hint, onehot_scalars, dense, n_dense, dense_scalars, levels};
    return hyperkzg_open_impl(ctx, srs, evals, point, ell, transcript_label, 0, 1, 0, nullptr, nullptr, com, w, v, challenges_out, fn, user, nullptr, 0, &lin);
}

// jolt_host_hyperkzg_open_grid for the batch framing (hyperkzg_verify.hip): always under a callback, the hint optional, the statement's check inside.
int32_t jolt_internal_hyperkzg_open_grid_checked(jolt_ctx* ctx, const jolt_srs* srs, const jolt_table* evals, const jolt_fr_t* point, size_t ell, jolt_open_transcript_fn fn,
                                                 void* user, const jolt_grid_hint* hint, uint32_t levels, const jolt_fr_t* onehot_scalars, jolt_table* const* dense,
                                                 size_t n_dense, const jolt_fr_t* dense_scalars, const Fr* expected_eval, jolt_g1_t* com, jolt_g1_t* w, jolt_fr_t* v,
                                                 jolt_fr_t* challenges_out) {
    if (!fn || (hint && hint->ctx != ctx)) return JOLT_ERR_INVALID_ARG;
    if (!hint || levels == 0) return hyperkzg_open_impl(ctx, srs, evals, point, ell, 0, 0, 1, 0, nullptr, nullptr, com, w, v, challenges_out, fn, user, nullptr, 0, nullptr, expected_eval);
    if (!onehot_scalars) return JOLT_ERR_INVALID_ARG;
    const GridLinear lin{hint, onehot_scalars, dense, n_dense, dense_scalars, levels};
    return hyperkzg_open_impl(ctx, srs, evals, point, ell, 0, 0, 1, 0, nullptr, nullptr, com, w, v, challenges_out, fn, user, nullptr, 0, &lin, expected_eval);
}

// The same opening with its MSMs sharded over `world` ranks by term range (every rank holds the polynomial and the SRS; `gather` is a
// jolt_gather_fn moving world x count 32-byte words -- jolt_comm_gather_round_sums / jolt_shm_gather_round_sums fit).  Every rank
// returns the same proof.
extern "C" int32_t jolt_host_hyperkzg_open_sharded(jolt_ctx* ctx, const jolt_srs* srs, const jolt_table* evals, const jolt_fr_t* point, size_t ell,
                                                   uint64_t transcript_label, int32_t rank, int32_t world, jolt_gather_fn gather, void* user, jolt_g1_t* com,
                                                   jolt_g1_t* w, jolt_fr_t* v, jolt_fr_t* challenges_out) {
    return hyperkzg_open_impl(ctx, srs, evals, point, ell, transcript_label, rank, world, 0, gather, user, com, w, v, challenges_out);
}
// The same with the block-cyclic term assignment: `srs` is the rank's COMPACT SRS (the bases of the terms i with (i / block) % world ==
// rank, in index order -- jolt_srs_setup_from_secret_blocks or an upload of those points), optionally with window tables.
extern "C" int32_t jolt_host_hyperkzg_open_sharded_blocks(jolt_ctx* ctx, const jolt_srs* srs, const jolt_table* evals, const jolt_fr_t* point, size_t ell,
                                                          uint64_t transcript_label, int32_t rank, int32_t world, size_t block, jolt_gather_fn gather, void* user,
                                                          jolt_g1_t* com, jolt_g1_t* w, jolt_fr_t* v, jolt_fr_t* challenges_out) {
    if (block == 0) return JOLT_ERR_INVALID_ARG;
    return hyperkzg_open_impl(ctx, srs, evals, point, ell, transcript_label, rank, world, block, gather, user, com, w, v, challenges_out);
}
