// jolt_amd/csrc/grid_pairs.hip -- the pair tables of the commitment grid (grid_pairs.hip.h): built once per SRS beside its window tables, read by the one-hot
// sums of bases (pcs.hip: k_grid_onehot_sum_pairs).  A function of the SRS, K and the domain length alone, like the window tables: the same for every column,
// residue class and proof.
#include <cstring>

#include "grid_pairs.hip.h"
#include "msm_kernels.hip.h"
#include "srs.hpp"

using namespace jolt;
using namespace jolt::msmk;

namespace {

// One lane per (pair m, row a): its k entries out[(m * k + a) * k + b] = pts[a * D + 2m] + pts[b * D + 2m + 1] share ONE inversion (Montgomery's trick).  The
// running products of the denominators are parked in the entries' own x words on the way up and replaced by the entries on the way down, so the trick needs no
// array in registers; a lane only ever reads back what it wrote itself.
__global__ __launch_bounds__(kBlock) void k_grid_pairs_build(const G1Affine* __restrict__ pts, size_t domain, uint32_t k, size_t count, Fq mont32, G1Affine* out) {
    const size_t t = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= count) return;
    const size_t m = t / k;
    const uint32_t a = (uint32_t)(t % k);
    const G1Affine p = ld_aff(pts + (size_t)a * domain + 2 * m);
    const G1Affine* qs = pts + 2 * m + 1;
    G1Affine* o = out + grid_pair_index(m, k, a, 0);
    Fq run = Fq::one();
    for (uint32_t b = 0; b < k; ++b) {
        run = mul(run, grid_pair_denominator(p, ld_aff(qs + (size_t)b * domain)));
        o[b].x = run;
    }
    Fq inv_run = inv(run);  // no denominator is zero
    for (uint32_t b = k; b-- > 0;) {
        const G1Affine q = ld_aff(qs + (size_t)b * domain);
        const Fq before = b ? o[b - 1].x : Fq::one();
        const Fq inv_d = mul(inv_run, before);
        inv_run = mul(inv_run, grid_pair_denominator(p, q));
        o[b] = grid_pair_entry(p, q, inv_d, mont32);
    }
}

Fq mont_of_32() {
    Fq thirty_two = Fq::zero();
    thirty_two.l[0] = 32;
    return to_mont(thirty_two);
}

}  // namespace

extern "C" int32_t jolt_srs_precompute_grid_pairs(jolt_ctx* ctx, jolt_srs* srs, uint32_t k, size_t cycles, uint32_t shift_mask) {
    if (!ctx || !srs) return JOLT_ERR_INVALID_ARG;
    // The tables are an optimisation next to window tables that are already built and usable, as the mid set is (msm_fixed.hip): ANY failure building one
    // (unsupported shape, out of memory, a HIP error) leaves the SRS as it was and the sums on the single bases.
    if (!srs->pre || srs->pre_stride != srs->n || k == 0 || k > 16 || cycles == 0 || (cycles & (cycles - 1)) != 0 || (size_t)k * cycles > srs->n) return JOLT_OK;
    const Fq mont32 = mont_of_32();
    for (uint32_t s = 0; s <= 4; ++s) {  // shift 0 first: the commitment itself, then the opening hint's levels
        if (!((shift_mask >> s) & 1u) || cycles < ((size_t)2 << s)) continue;
        const size_t domain = cycles >> s;
        if (jolt_srs_grid_pairs(srs, k, domain) || srs->n_pairs == jolt_srs::kMaxGridPairs) continue;
        const size_t count = domain / 2 * k, bytes = count * k * sizeof(G1Affine);
        G1Affine* table = nullptr;
        hipError_t e = hipMalloc((void**)&table, bytes);
        if (e != hipSuccess) { (void)hipGetLastError(); continue; }
        hipLaunchKernelGGL(k_grid_pairs_build, dim3((unsigned)((count + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->stream, (const G1Affine*)srs->pts, domain, k, count, mont32,
                           table);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) { (void)hipGetLastError(); (void)hipFree(table); continue; }
        srs->pairs[srs->n_pairs].k = k;
        srs->pairs[srs->n_pairs].domain = domain;
        srs->pairs[srs->n_pairs].table = table;
        srs->n_pairs++;
        if (srs->ctx) srs->ctx->grid_pairs_bytes += bytes;
    }
    return JOLT_OK;
}

extern "C" int32_t jolt_srs_grid_pairs_bytes(const jolt_srs* srs, uint32_t k, size_t domain, size_t* bytes) {
    if (!srs || !bytes) return JOLT_ERR_INVALID_ARG;
    *bytes = jolt_srs_grid_pairs(srs, k, domain) ? 32 * (size_t)k * k * domain : 0;
    return JOLT_OK;
}

// ---- host twins (the CPU suite pins the entry arithmetic and the index map) -------------------------------------------------------------------------------------
extern "C" int32_t jolt_host_grid_pair_entry(const jolt_g1_t* p, const jolt_g1_t* q, uint64_t* out_words) {
    if (!p || !q || !out_words) return JOLT_ERR_INVALID_ARG;
    G1Jac pj, qj;
    std::memcpy(&pj, p, sizeof(pj));
    std::memcpy(&qj, q, sizeof(qj));
    const G1Affine pa = g1_to_affine(pj), qa = g1_to_affine(qj);
    const G1Affine r = grid_pair_entry(pa, qa, inv(grid_pair_denominator(pa, qa)), mont_of_32());
    std::memcpy(out_words, &r, sizeof(r));
    return JOLT_OK;
}
extern "C" int32_t jolt_host_grid_pair_index(size_t m, uint32_t k, uint32_t a, uint32_t b, size_t* out) {
    if (!out) return JOLT_ERR_INVALID_ARG;
    *out = grid_pair_index(m, k, a, b);
    return JOLT_OK;
}
