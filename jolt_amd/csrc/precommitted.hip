// jolt_amd/csrc/precommitted.hip -- the precommitted claim reductions as stage operators, and their table builders.
//
// Reference: crates/jolt-kernels/src/precommitted_reduction.rs (the two phase kernels over one PrecommittedTables state, the 6b -> 7 carry, lsb_permutation /
// permute_coefficients / permute_challenges) and crates/jolt-kernels/src/optimized/precommitted_reduction.rs (the prepare side: advice, program image, bytecode).
// The four kinds (trusted advice, untrusted advice, committed bytecode, program image) differ in how their tables are BUILT and in how their output claims are
// named on the wire; the rounds are one algebra.  Here that algebra is ONE operator class over a table state that lives either on the device (the product) or on the
// host (jolt_stage_host_precommitted_create: what the CPU suite checks against the definition before any device code is trusted).  The round schedule and the
// variable permutation are inputs: PrecommittedClaimReduction's geometry is not restated.
//
//   entry                                         reference
//   jolt_stage_precommitted_cycle_create          CycleReductionKernel::new + ProveRounds (:308-407), output_claims (:455-534)
//   jolt_stage_precommitted_address_create        park_carry / AddressReductionKernel::new (:367-379, :418-453), output_claims (:536-590)
//   jolt_stage_host_precommitted_create, _address_create   the same over host tables
//   jolt_host_precommitted_lsb_permutation        lsb_permutation (:595-609)
//   jolt_host_precommitted_permute_challenges     permute_challenges (:641-652)
//   jolt_table_permute_bits                       permute_coefficients (:615-636)
//   jolt_eq_evals_shifted                         shifted_eq_slice (optimized/precommitted_reduction.rs:337-360)
//   jolt_table_outer                              the bytecode eq template (optimized/precommitted_reduction.rs:419-425)
#include <algorithm>
#include <memory>

#include "precommitted_kernels.hip.h"
#include "stage_op.hpp"

using namespace jolt;
using namespace jolt_host;

namespace {

constexpr size_t kMaxAux = 256;
constexpr const char* kMissingCarry = "stage 6b parked no precommitted reduction state for the scheduled address phase";

// PrecommittedTables (:76-85) behind the two operations a round needs.  `step` applies `bind` (if any) to every table and, if asked, returns the two round sums over
// the value / eq tables as they are AFTER that bind.
struct PrecommittedState {
    Fr scale = Fr::one(), scale_inv = Fr::one();
    size_t len = 0, n_aux = 0;
    virtual ~PrecommittedState() = default;
    virtual int32_t step(const Fr* bind, bool want_sums, Fr* e0, Fr* e2) = 0;
    virtual int32_t dot(Fr* out) = 0;                      // sum value eq (unscaled)
    virtual int32_t finals(std::vector<Fr>* out) = 0;      // value[0], aux[i][0]; len == 1
};

struct HostTables final : PrecommittedState {
    std::vector<std::vector<Fr>> t;  // value, eq, aux...

    int32_t step(const Fr* bind, bool want_sums, Fr* e0, Fr* e2) override {
        if (bind) {
            if (len < 2) return JOLT_ERR_INVALID_ARG;
            for (std::vector<Fr>& v : t) {
                for (size_t y = 0; y < len / 2; ++y) v[y] = add(v[2 * y], mul(*bind, sub(v[2 * y + 1], v[2 * y])));  // dense.rs:223-303
                v.resize(len / 2);
            }
            len /= 2;
        }
        if (!want_sums) return JOLT_OK;
        if (len < 2) return JOLT_ERR_INVALID_ARG;
        Fr a = Fr::zero(), b = Fr::zero();
        const std::vector<Fr>&v = t[0], &e = t[1];
        for (size_t j = 0; j < len / 2; ++j) {  // :103-112
            a = add(a, mul(v[2 * j], e[2 * j]));
            b = add(b, mul(sub(dbl(v[2 * j + 1]), v[2 * j]), sub(dbl(e[2 * j + 1]), e[2 * j])));
        }
        *e0 = a;
        *e2 = b;
        return JOLT_OK;
    }
    int32_t dot(Fr* out) override {
        Fr a = Fr::zero();
        for (size_t j = 0; j < len; ++j) a = add(a, mul(t[0][j], t[1][j]));
        *out = a;
        return JOLT_OK;
    }
    int32_t finals(std::vector<Fr>* out) override {
        out->clear();
        out->push_back(t[0][0]);
        for (size_t i = 0; i < n_aux; ++i) out->push_back(t[2 + i][0]);
        return JOLT_OK;
    }
};

// The device state: every table has a ping buffer (the copy of the caller's table) and a pong buffer of half that length; the two pointer arrays the kernels
// index with blockIdx.y are written once.
struct DeviceTables final : PrecommittedState {
    jolt_ctx* ctx = nullptr;
    std::vector<Fr*> buf[2];
    std::vector<const Fr*> h_ptrs;  // 2 x n_tables: what d_ptrs holds
    Fr** d_ptrs = nullptr;          // [side * n_tables + table]
    int cur = 0;

    size_t n_tables() const { return 2 + n_aux; }
    ~DeviceTables() override {
        (void)jolt_internal_join_side_writers(ctx);
        for (int s = 0; s < 2; ++s)
            for (Fr* p : buf[s])
                if (p) jolt_internal_dev_free(ctx, p);
        if (d_ptrs) jolt_internal_dev_free(ctx, d_ptrs);
    }
    const Fr* const* side(int s) const { return (const Fr* const*)(d_ptrs + (size_t)s * n_tables()); }
    unsigned grid_x(size_t items) const {
        const size_t need = (items + kBlock - 1) / kBlock;
        return (unsigned)std::max<size_t>(1, std::min<size_t>(need, (size_t)ctx->num_cus * 8));
    }
    int32_t fetch(int nblocks, int ne, const Fr* partials, Fr* out) {
        hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(kBlock), 0, ctx->stream, partials, nblocks, ne, ctx->d_results);
        JOLT_HIP_TRY(ctx, hipGetLastError());
        return read_results((size_t)ne, out);
    }
    int32_t read_results(size_t count, Fr* out) {
        JOLT_HIP_TRY(ctx, hipMemcpyAsync(ctx->h_results, ctx->d_results, count * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
        JOLT_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        std::memcpy(out, ctx->h_results, count * sizeof(Fr));
        return JOLT_OK;
    }

    int32_t step(const Fr* bind, bool want_sums, Fr* e0, Fr* e2) override {
        if (!bind && !want_sums) return JOLT_OK;
        if (len < 2 || (bind && want_sums && len < 4)) return JOLT_ERR_INVALID_ARG;
        JOLT_HIP_TRY(ctx, hipSetDevice(ctx->device));
        JOLT_TRY(jolt_internal_join_side_writers(ctx));
        const Fr* const* in = side(cur);
        Fr* const* out = (Fr* const*)side(1 - cur);
        // the round sums come back the way a batch round's do: the last workgroup publishes them to host-mapped memory and the host spins on the flag
        RoundDone rd;
        rd.counters = ctx->d_counters;
        rd.results = ctx->h_round;
        rd.results_dev = nullptr;
        rd.flag = ctx->h_flag;
        rd.seq = 0;
        rd.group_total = 1;
        if (want_sums) rd.seq = ++ctx->seq;
        if (bind && want_sums) {  // ONE launch: the pending challenge on every table, the sums over the bound value / eq
            const size_t quads = len / 4;
            const unsigned gx = grid_x(quads);
            JOLT_TRY(jolt_internal_ensure_scratch(ctx, (size_t)gx * 2, 2));
            const dim3 grid(gx, (unsigned)(1 + n_aux));
            if (fr_low_limbs_zero(*bind)) hipLaunchKernelGGL(k_precommitted_bind_sums<true>, grid, dim3(kBlock), 0, ctx->stream, in, out, quads, *bind, ctx->d_partials, rd);
            else hipLaunchKernelGGL(k_precommitted_bind_sums<false>, grid, dim3(kBlock), 0, ctx->stream, in, out, quads, *bind, ctx->d_partials, rd);
        } else if (bind) {
            const size_t half = len / 2;
            const dim3 grid(grid_x((half + 1) / 2), (unsigned)n_tables());
            if (fr_low_limbs_zero(*bind)) hipLaunchKernelGGL(k_precommitted_bind<true>, grid, dim3(kBlock), 0, ctx->stream, in, out, half, *bind);
            else hipLaunchKernelGGL(k_precommitted_bind<false>, grid, dim3(kBlock), 0, ctx->stream, in, out, half, *bind);
        } else {
            const size_t pairs = len / 2;
            const unsigned gx = grid_x(pairs);
            JOLT_TRY(jolt_internal_ensure_scratch(ctx, (size_t)gx * 2, 2));
            hipLaunchKernelGGL(k_precommitted_sums, dim3(gx), dim3(kBlock), 0, ctx->stream, in, pairs, ctx->d_partials, rd);
        }
        JOLT_HIP_TRY(ctx, hipGetLastError());
        if (bind) {
            cur = 1 - cur;
            len /= 2;
        }
        if (!want_sums) return JOLT_OK;
        Fr s[2];
        JOLT_TRY(wait_round(rd.seq, s));
        *e0 = s[0];
        *e2 = s[1];
        return JOLT_OK;
    }
    // spin on the host-mapped flag (as the batch rounds do); if the stream has drained without the flag, say so instead of waiting for ever
    int32_t wait_round(uint64_t want, Fr* sums) {
        volatile uint64_t* flag = ctx->h_flag;
        uint64_t spins = 0;
        while (*flag != want) {
            if (++spins > (1ull << 22)) {
                spins = 0;
                const hipError_t q = hipStreamQuery(ctx->stream);
                if (q == hipSuccess) {
                    if (*flag == want) break;
                    ctx->last_error = "precommitted round finished without publishing its completion flag";
                    return JOLT_ERR_HIP;
                }
                if (q != hipErrorNotReady) {
                    ctx->last_error = std::string("precommitted round: ") + hipGetErrorString(q);
                    return JOLT_ERR_HIP;
                }
            }
        }
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
        std::memcpy(sums, ctx->h_round, 2 * sizeof(Fr));
        return JOLT_OK;
    }
    int32_t dot(Fr* out) override {
        JOLT_HIP_TRY(ctx, hipSetDevice(ctx->device));
        JOLT_TRY(jolt_internal_join_side_writers(ctx));
        const unsigned gx = grid_x(len);
        JOLT_TRY(jolt_internal_ensure_scratch(ctx, gx, 2));
        hipLaunchKernelGGL(k_sum_or_dot<true>, dim3(gx), dim3(kBlock), 0, ctx->stream, (const Fr*)buf[cur][0], (const Fr*)buf[cur][1], len, ctx->d_partials);
        JOLT_HIP_TRY(ctx, hipGetLastError());
        return fetch((int)gx, 1, ctx->d_partials, out);
    }
    int32_t finals(std::vector<Fr>* out) override {
        JOLT_HIP_TRY(ctx, hipSetDevice(ctx->device));
        JOLT_TRY(jolt_internal_join_side_writers(ctx));
        const size_t n = n_tables();
        JOLT_TRY(jolt_internal_ensure_scratch(ctx, 1, n));
        hipLaunchKernelGGL(k_precommitted_first_entries, dim3(1), dim3(kBlock), 0, ctx->stream, side(cur), n, ctx->d_results);
        JOLT_HIP_TRY(ctx, hipGetLastError());
        std::vector<Fr> all(n);
        JOLT_TRY(read_results(n, all.data()));
        out->clear();
        out->push_back(all[0]);
        for (size_t i = 0; i < n_aux; ++i) out->push_back(all[2 + i]);
        return JOLT_OK;
    }
};

bool is_active(const std::vector<size_t>& active, size_t round) { return std::binary_search(active.begin(), active.end(), round); }  // :221-223

// Both phase kernels (CycleReductionKernel :269-407, AddressReductionKernel :412-453): one schedule walk over a state.
struct PrecommittedOp final : jolt_stage_op {
    std::unique_ptr<PrecommittedState> st;  // null once the carry has been reclaimed
    std::vector<size_t> active;             // this phase's active rounds
    std::vector<size_t> address_active;     // a cycle operator: the schedule its carry resumes under
    size_t address_total = 0;
    bool is_address = false, finished = false, device = false;
    size_t next_round = 0;                  // the rounds come in order, each once
    Fr two_inv = inv(fr_from_u64(2));

    bool has_address_phase() const { return !is_address && !address_active.empty(); }  // :349-351

    // bind_round (:160-172) of round `round`, then -- if `message` -- round_message (:96-133) of the round after it
    int32_t ingest(const Fr* bind, size_t bound_round, bool want_sums, Fr* e0, Fr* e2) {
        const bool bind_tables = bind && is_active(active, bound_round);
        if (bind && !bind_tables) {
            st->scale = mul(st->scale, two_inv);
            st->scale_inv = dbl(st->scale_inv);
        }
        return st->step(bind_tables ? bind : nullptr, want_sums, e0, e2);
    }
    int32_t prove_round(const Fr* bind, size_t round, const Fr& claim, UnivariatePoly* out) override {
        if (!st || finished || round >= rounds) return JOLT_ERR_INVALID_ARG;
        // head-aligned and consulted every round of its window: `bind` is Some exactly when round >= 1 (:136-139), and the rounds come in order
        if (round != next_round || (bind != nullptr) != (round > 0)) return fail(JOLT_ERR_INVALID_ARG, "rounds out of order");
        const bool act = is_active(active, round);
        Fr e0 = Fr::zero(), e2 = Fr::zero();
        JOLT_TRY(ingest(bind, round - 1, act, &e0, &e2));
        if (bind) binds.push_back(*bind);
        ++next_round;
        out->coefficients.clear();
        if (!act) {
            out->coefficients.push_back(mul(claim, two_inv));  // :97-99
            return JOLT_OK;
        }
        const Fr e1 = sub(mul(claim, st->scale_inv), e0);  // the hint: from the (possibly padded) claim, not from the tables (:129)
        const Fr c2 = mul(add(sub(sub(e0, e1), e1), e2), two_inv);
        const Fr c1 = sub(sub(e1, e0), c2);
        out->coefficients = {mul(e0, st->scale), mul(c1, st->scale), mul(c2, st->scale)};
        return JOLT_OK;
    }
    int32_t finish_rounds(const Fr& bind) override {
        if (!st || finished || next_round != rounds) return fail(JOLT_ERR_INVALID_ARG, "finish_rounds before the last round");
        JOLT_TRY(ingest(&bind, rounds - 1, false, nullptr, nullptr));  // :154-156
        binds.push_back(bind);
        finished = true;
        return JOLT_OK;
    }
    int32_t intermediate(Fr* out) {  // :176-192
        Fr d;
        JOLT_TRY(st->dot(&d));
        *out = mul(d, st->scale);
        return JOLT_OK;
    }
    int32_t input_claim(Fr* out) override {
        if (!st || next_round != 0) return JOLT_ERR_INVALID_ARG;
        return intermediate(out);
    }
    int32_t output_claims(std::vector<Fr>* out) override {
        if (has_address_phase()) {  // scalar_claim (:359-365) / the chunked counterpart (:496-509)
            const auto it = kept.find("intermediate");
            if (it != kept.end()) {
                *out = it->second;
                return JOLT_OK;
            }
            if (!st) return JOLT_ERR_INVALID_ARG;
            Fr c;
            JOLT_TRY(intermediate(&c));
            *out = {c};
            if (finished) kept["intermediate"] = *out;
            return JOLT_OK;
        }
        if (!st) return JOLT_ERR_INVALID_ARG;
        if (st->len != 1) return fail(JOLT_ERR_NOT_FULLY_BOUND, "precommitted reduction final claim requested before the polynomial is fully bound");  // :194-202
        return st->finals(out);
    }
};

bool ascending_below(const size_t* v, size_t n, size_t total) {
    for (size_t i = 0; i < n; ++i)
        if (v[i] >= total || (i && v[i] <= v[i - 1])) return false;
    return true;
}

// the checks both constructors share; *n_vars = log2 len
int32_t check_shape(size_t len, size_t n_aux, const size_t* cycle_active, size_t n_cycle_active, size_t cycle_total, const size_t* address_active, size_t n_address_active,
                    size_t address_total, size_t* n_vars) {
    if (n_aux > kMaxAux || (!cycle_active && n_cycle_active) || (!address_active && n_address_active) || cycle_total == 0) return JOLT_ERR_INVALID_ARG;
    if (len == 0 || (len & (len - 1)) != 0) return JOLT_ERR_INVALID_ARG;
    if (!ascending_below(cycle_active, n_cycle_active, cycle_total) || !ascending_below(address_active, n_address_active, address_total)) return JOLT_ERR_INVALID_ARG;
    size_t n = 0;
    while (((size_t)1 << n) < len) ++n;
    if (n_cycle_active + n_address_active != n) return JOLT_ERR_SIZE_MISMATCH;  // the tables are 2^(permutation length) long (:317-329)
    *n_vars = n;
    return JOLT_OK;
}

PrecommittedOp* new_cycle_op(jolt_ctx* ctx, bool device, const size_t* cycle_active, size_t n_cycle_active, size_t cycle_total, const size_t* address_active,
                             size_t n_address_active, size_t address_total) {
    PrecommittedOp* op = new (std::nothrow) PrecommittedOp();
    if (!op) return nullptr;
    op->ctx = ctx;
    op->name = "precommitted_cycle";
    op->device = device;
    op->rounds = cycle_total;
    op->degree = 2;
    op->active.assign(cycle_active, cycle_active + n_cycle_active);
    op->address_active.assign(address_active, address_active + n_address_active);
    op->address_total = address_total;
    return op;
}

int32_t reclaim(jolt_ctx* ctx, jolt_stage_op* cycle_op, bool device, jolt_stage_op** out) {
    PrecommittedOp* cyc = dynamic_cast<PrecommittedOp*>(cycle_op);
    if (!cyc || !out) return JOLT_ERR_INVALID_ARG;
    if (cyc->device != device || (device && cyc->ctx != ctx) || !cyc->has_address_phase() || !cyc->finished || !cyc->st) {
        jolt_ctx* c = ctx ? ctx : cyc->ctx;
        if (c) c->last_error = kMissingCarry;
        return JOLT_ERR_INVALID_ARG;
    }
    std::vector<Fr> claim;
    JOLT_TRY(cyc->output_claims(&claim));  // the cycle operator keeps its intermediate claim
    PrecommittedOp* op = new (std::nothrow) PrecommittedOp();
    if (!op) return JOLT_ERR_OOM;
    op->ctx = cyc->ctx;
    op->name = "precommitted_address";
    op->device = device;
    op->is_address = true;
    op->rounds = cyc->address_total;
    op->degree = 2;
    op->active = cyc->address_active;
    op->st = std::move(cyc->st);  // PrecommittedReductionCarry (:225-234): the bound tables and the running scale, moved
    *out = op;
    return JOLT_OK;
}

}  // namespace

extern "C" int32_t jolt_stage_precommitted_cycle_create(jolt_ctx* ctx, const jolt_table* value, const jolt_table* eq, const jolt_table* const* aux, size_t n_aux,
                                                        const size_t* cycle_active, size_t n_cycle_active, size_t cycle_total, const size_t* address_active,
                                                        size_t n_address_active, size_t address_total, jolt_stage_op** out) {
    if (!ctx || !value || !eq || !out || (!aux && n_aux) || n_aux > kMaxAux) return JOLT_ERR_INVALID_ARG;
    std::vector<const jolt_table*> src = {value, eq};
    for (size_t i = 0; i < n_aux; ++i) src.push_back(aux[i]);
    for (const jolt_table* t : src) {
        if (!t || (t->ctx && t->ctx != ctx) || t->ints) return JOLT_ERR_INVALID_ARG;
        if (t->len != value->len) return JOLT_ERR_SIZE_MISMATCH;
    }
    size_t n = 0;
    JOLT_TRY(check_shape(value->len, n_aux, cycle_active, n_cycle_active, cycle_total, address_active, n_address_active, address_total, &n));
    std::unique_ptr<PrecommittedOp> op(new_cycle_op(ctx, true, cycle_active, n_cycle_active, cycle_total, address_active, n_address_active, address_total));
    if (!op) return JOLT_ERR_OOM;
    std::unique_ptr<DeviceTables> st(new (std::nothrow) DeviceTables());
    if (!st) return JOLT_ERR_OOM;
    JOLT_HIP_TRY(ctx, hipSetDevice(ctx->device));
    JOLT_TRY(jolt_internal_join_side_writers(ctx));
    st->ctx = ctx;
    st->len = value->len;
    st->n_aux = n_aux;
    const size_t nt = src.size(), len = value->len;
    st->buf[0].assign(nt, nullptr);
    st->buf[1].assign(nt, nullptr);
    for (size_t i = 0; i < nt; ++i) {
        JOLT_TRY(jolt_internal_dev_alloc(ctx, len * sizeof(Fr), (void**)&st->buf[0][i]));
        JOLT_TRY(jolt_internal_dev_alloc(ctx, std::max<size_t>(len / 2, 1) * sizeof(Fr), (void**)&st->buf[1][i]));
        JOLT_HIP_TRY(ctx, hipMemcpyAsync(st->buf[0][i], src[i]->data(), len * sizeof(Fr), hipMemcpyDeviceToDevice, ctx->stream));
    }
    st->h_ptrs.resize(2 * nt);
    for (int s = 0; s < 2; ++s)
        for (size_t i = 0; i < nt; ++i) st->h_ptrs[(size_t)s * nt + i] = st->buf[s][i];
    JOLT_TRY(jolt_internal_dev_alloc(ctx, 2 * nt * sizeof(Fr*), (void**)&st->d_ptrs));
    JOLT_HIP_TRY(ctx, hipMemcpyAsync(st->d_ptrs, st->h_ptrs.data(), 2 * nt * sizeof(Fr*), hipMemcpyHostToDevice, ctx->stream));
    JOLT_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // the pointer arrays are in place; the caller's tables may go
    op->st = std::move(st);
    *out = op.release();
    return JOLT_OK;
}

extern "C" int32_t jolt_stage_precommitted_address_create(jolt_ctx* ctx, jolt_stage_op* cycle_op, jolt_stage_op** out) {
    if (!ctx) return JOLT_ERR_INVALID_ARG;
    return reclaim(ctx, cycle_op, true, out);
}

extern "C" int32_t jolt_stage_host_precommitted_create(const jolt_fr_t* value, const jolt_fr_t* eq, const jolt_fr_t* const* aux, size_t n_aux, size_t len,
                                                       const size_t* cycle_active, size_t n_cycle_active, size_t cycle_total, const size_t* address_active,
                                                       size_t n_address_active, size_t address_total, jolt_stage_op** out) {
    if (!value || !eq || !out || (!aux && n_aux) || n_aux > kMaxAux) return JOLT_ERR_INVALID_ARG;
    size_t n = 0;
    JOLT_TRY(check_shape(len, n_aux, cycle_active, n_cycle_active, cycle_total, address_active, n_address_active, address_total, &n));
    std::unique_ptr<PrecommittedOp> op(new_cycle_op(nullptr, false, cycle_active, n_cycle_active, cycle_total, address_active, n_address_active, address_total));
    if (!op) return JOLT_ERR_OOM;
    std::unique_ptr<HostTables> st(new (std::nothrow) HostTables());
    if (!st) return JOLT_ERR_OOM;
    st->len = len;
    st->n_aux = n_aux;
    std::vector<const jolt_fr_t*> src = {value, eq};
    for (size_t i = 0; i < n_aux; ++i) src.push_back(aux[i]);
    for (const jolt_fr_t* p : src) {
        if (!p) return JOLT_ERR_INVALID_ARG;
        std::vector<Fr> v(len);
        for (size_t j = 0; j < len; ++j) {
            v[j] = fr_from_abi(&p[j]);
            if (!fr_is_canonical(v[j])) return JOLT_ERR_INVALID_ARG;
        }
        st->t.push_back(std::move(v));
    }
    op->st = std::move(st);
    *out = op.release();
    return JOLT_OK;
}

extern "C" int32_t jolt_stage_host_precommitted_address_create(jolt_stage_op* cycle_op, jolt_stage_op** out) { return reclaim(nullptr, cycle_op, false, out); }

// ------------------------------------------------------------------------------------------------------------------
// the prepare side
// ------------------------------------------------------------------------------------------------------------------
extern "C" int32_t jolt_host_precommitted_lsb_permutation(const size_t* perm_be, size_t n, size_t* old_lsb_to_new_lsb, int32_t* is_identity) {
    if ((!perm_be && n) || (!old_lsb_to_new_lsb && n) || !is_identity || n > 40) return JOLT_ERR_INVALID_ARG;
    std::vector<size_t> be_var_by_round(n);
    for (size_t i = 0; i < n; ++i) be_var_by_round[i] = i;
    std::sort(be_var_by_round.begin(), be_var_by_round.end(), [&](size_t a, size_t b) { return perm_be[a] < perm_be[b]; });
    for (size_t i = 1; i < n; ++i)
        if (perm_be[be_var_by_round[i]] == perm_be[be_var_by_round[i - 1]]) return JOLT_ERR_INVALID_ARG;  // two variables in one opening round
    int32_t same = 1;
    for (size_t new_lsb = 0; new_lsb < n; ++new_lsb) {
        const size_t old_lsb = n - 1 - be_var_by_round[new_lsb];
        old_lsb_to_new_lsb[old_lsb] = new_lsb;
        if (old_lsb != new_lsb) same = 0;
    }
    *is_identity = same;
    return JOLT_OK;
}

static bool is_bit_permutation(const size_t* map, size_t n) {
    uint64_t seen = 0;
    for (size_t i = 0; i < n; ++i) {
        if (map[i] >= n || ((seen >> map[i]) & 1)) return false;
        seen |= (uint64_t)1 << map[i];
    }
    return true;
}

extern "C" int32_t jolt_host_precommitted_permute_challenges(const jolt_fr_t* challenges_be, size_t n, const size_t* map, jolt_fr_t* out) {
    if (n > 40 || (n && (!challenges_be || !map || !out)) || !is_bit_permutation(map, n)) return JOLT_ERR_INVALID_ARG;
    for (size_t old_be = 0; old_be < n; ++old_be) out[n - 1 - map[n - 1 - old_be]] = challenges_be[old_be];
    return JOLT_OK;
}

extern "C" int32_t jolt_table_permute_bits(jolt_ctx* ctx, const jolt_table* table, const size_t* old_lsb_to_new_lsb, size_t n, jolt_table** out) {
    if (!ctx || !table || !out || table->ints || n > 40 || (n && !old_lsb_to_new_lsb) || !is_bit_permutation(old_lsb_to_new_lsb, n)) return JOLT_ERR_INVALID_ARG;
    if (table->len != ((size_t)1 << n)) return JOLT_ERR_SIZE_MISMATCH;
    JOLT_HIP_TRY(ctx, hipSetDevice(ctx->device));
    JOLT_TRY(jolt_internal_join_side_writers(ctx));
    BitPermutation p;
    std::memset(&p, 0, sizeof(p));
    p.n = (uint32_t)n;
    for (size_t old_lsb = 0; old_lsb < n; ++old_lsb) p.new_to_old[old_lsb_to_new_lsb[old_lsb]] = (uint8_t)old_lsb;
    jolt_table* t = nullptr;
    JOLT_TRY(jolt_internal_table_new(ctx, table->len, &t));
    const unsigned gx = (unsigned)std::max<size_t>(1, std::min<size_t>((table->len + kBlock - 1) / kBlock, (size_t)ctx->num_cus * 8));
    hipLaunchKernelGGL(k_permute_bits, dim3(gx), dim3(kBlock), 0, ctx->stream, (const Fr*)table->data(), t->buf[0], table->len, p);
    if (hipGetLastError() != hipSuccess) {
        jolt_table_free(ctx, t);
        ctx->last_error = "k_permute_bits: launch failed";
        return JOLT_ERR_HIP;
    }
    *out = t;
    return JOLT_OK;
}

extern "C" int32_t jolt_eq_evals_shifted(jolt_ctx* ctx, const jolt_fr_t* r, size_t n, size_t start_index, size_t len, jolt_table** out) {
    if (!ctx || !out || (!r && n) || n > 40 || len == 0 || len > ((size_t)1 << n)) return JOLT_ERR_INVALID_ARG;
    const size_t domain = (size_t)1 << n;
    jolt_table* t = nullptr;
    JOLT_TRY(jolt_internal_table_new(ctx, len, &t));
    size_t index = start_index & (domain - 1), remaining = len, pos = 0;
    int32_t st = JOLT_OK;
    while (remaining > 0 && st == JOLT_OK) {
        // the largest power-of-two block that starts at `index`, is aligned there and neither passes the domain top nor the slice's end
        // (EqPolynomial::evals_for_max_aligned_block; a wrapped continuation restarts at 0, aligned to everything)
        const size_t span = std::min(remaining, domain - index);
        size_t block = 1;
        while (block * 2 <= span && index % (block * 2) == 0) block *= 2;
        jolt_table* b = nullptr;
        st = jolt_eq_evals_aligned_block(ctx, r, n, index, block, &b);
        if (st != JOLT_OK) break;
        if (hipMemcpyAsync(t->buf[0] + pos, b->data(), block * sizeof(Fr), hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess) {
            ctx->last_error = "jolt_eq_evals_shifted: block copy failed";
            st = JOLT_ERR_HIP;
        }
        jolt_table_free(ctx, b);  // back to the pool: reuse is stream-ordered behind the copy
        index = (index + block) & (domain - 1);
        pos += block;
        remaining -= block;
    }
    if (st != JOLT_OK) {
        jolt_table_free(ctx, t);
        return st;
    }
    *out = t;
    return JOLT_OK;
}

extern "C" int32_t jolt_table_outer(jolt_ctx* ctx, const jolt_fr_t* lane_weights, size_t n_lanes, const jolt_table* cycle_table, int32_t order, jolt_table** out) {
    if (!ctx || !lane_weights || !n_lanes || !cycle_table || !out || cycle_table->ints || cycle_table->len == 0 ||
        (order != JOLT_TRACE_CYCLE_MAJOR && order != JOLT_TRACE_ADDRESS_MAJOR))
        return JOLT_ERR_INVALID_ARG;
    for (size_t i = 0; i < n_lanes; ++i)
        if (!fr_is_canonical(fr_from_abi(&lane_weights[i]))) return JOLT_ERR_INVALID_ARG;
    if (n_lanes > ((size_t)1 << 40) / cycle_table->len) return JOLT_ERR_UNSUPPORTED;
    jolt_table *w = nullptr, *t = nullptr;
    JOLT_TRY(jolt_table_upload(ctx, lane_weights, n_lanes, &w));
    const size_t len = n_lanes * cycle_table->len;
    int32_t st = jolt_internal_table_new(ctx, len, &t);
    if (st == JOLT_OK) {
        const unsigned gx = (unsigned)std::max<size_t>(1, std::min<size_t>((len + kBlock - 1) / kBlock, (size_t)ctx->num_cus * 8));
        hipLaunchKernelGGL(k_table_outer, dim3(gx), dim3(kBlock), 0, ctx->stream, (const Fr*)w->data(), n_lanes, (const Fr*)cycle_table->data(), cycle_table->len,
                           order == JOLT_TRACE_ADDRESS_MAJOR ? 1 : 0, t->buf[0]);
        if (hipGetLastError() != hipSuccess) {
            ctx->last_error = "k_table_outer: launch failed";
            st = JOLT_ERR_HIP;
        }
    }
    jolt_table_free(ctx, w);
    if (st != JOLT_OK) {
        if (t) jolt_table_free(ctx, t);
        return st;
    }
    *out = t;
    return JOLT_OK;
}
