// jolt_amd/csrc/r1cs_rows.hip -- HOST code: a constraint system as rows (jolt_r1cs_rows) and the uni-skip first round above it.
//
//   jolt_r1cs_rows_create / _destroy / _extension / _fold_small   the row object and its integer extension coefficients L_i(node)
//   jolt_host_centered_lagrange_evals / _kernel                   crates/jolt-poly/src/lagrange.rs:20-104
//   jolt_host_interpolate_to_coeffs                               :567-608
//   jolt_host_uniskip_first_round_poly                            s1 = LK(tau_high, .) x t1 (crates/jolt-kernels/src/reference/spartan_outer.rs:217-225)
//   jolt_host_prove_uniskip                                       prove_uniskip_clear (crates/jolt-sumcheck/src/prover.rs:415-440)
//   jolt_host_r1cs_rows_cycle                                     r1cs_rows.hip.h built for the host (what k_rows_uniskip runs per cycle and node)
//   jolt_host_r1cs_rows_remainder_weights                         spartan_outer_row_weights + weighted_columns + public_column_contributions
//                                                                 (crates/jolt-r1cs/src/constraints/jolt.rs:141-170, reference/spartan_outer.rs:239-262)
#include <cstring>
#include <new>

#include "host_mirror.hpp"
#include "r1cs_rows.hpp"

using namespace jolt;
using namespace jolt_host;

namespace jolt_r1cs_rows_host {

int64_t centered_start(size_t n) { return -(int64_t)((n - 1) / 2); }

Fr fr_from_i64(int64_t v) {
    const Fr m = fr_from_u64(v < 0 ? (uint64_t)0 - (uint64_t)v : (uint64_t)v);
    return v < 0 ? neg(m) : m;
}
Fr fr_from_i128(uint64_t lo, uint64_t hi) {
    const Fr two32 = fr_from_u64((uint64_t)1 << 32);
    return add(fr_from_u64(lo), mul(fr_from_i64((int64_t)hi), mul(two32, two32)));
}

std::vector<Fr> centered_lagrange_evals(size_t D, const Fr& r) {
    const int64_t start = centered_start(D);
    std::vector<Fr> nodes(D), out(D, Fr::zero());
    for (size_t k = 0; k < D; ++k) nodes[k] = fr_from_i64(start + (int64_t)k);
    for (size_t k = 0; k < D; ++k)
        if (r == nodes[k]) {  // a grid point: the unit vector (:28-34)
            out[k] = Fr::one();
            return out;
        }
    Fr full = Fr::one();
    std::vector<Fr> diffs(D);
    for (size_t k = 0; k < D; ++k) {
        diffs[k] = sub(r, nodes[k]);
        full = mul(full, diffs[k]);
    }
    for (size_t i = 0; i < D; ++i) {
        Fr w = Fr::one();
        for (size_t j = 0; j < D; ++j)
            if (i != j) w = mul(w, fr_from_i64((int64_t)i - (int64_t)j));
        out[i] = mul(mul(full, inv(w)), inv(diffs[i]));
    }
    return out;
}

Fr centered_lagrange_kernel(size_t D, const Fr& x, const Fr& y) {
    const std::vector<Fr> lx = centered_lagrange_evals(D, x), ly = centered_lagrange_evals(D, y);
    Fr s = Fr::zero();
    for (size_t i = 0; i < D; ++i) s = add(s, mul(lx[i], ly[i]));
    return s;
}

std::vector<Fr> interpolate_to_coeffs(int64_t start, const std::vector<Fr>& values) {
    const size_t n = values.size();
    std::vector<Fr> dd = values;  // Newton's divided differences over consecutive integers: the denominator is `step`
    for (size_t step = 1; step < n; ++step) {
        const Fr d = inv(fr_from_i64((int64_t)step));
        for (size_t i = n - 1; i >= step; --i) dd[i] = mul(sub(dd[i], dd[i - 1]), d);
    }
    std::vector<Fr> coeffs(n, Fr::zero()), basis(n, Fr::zero());
    basis[0] = Fr::one();
    for (size_t k = 0; k < n; ++k) {
        for (size_t i = 0; i <= k; ++i) coeffs[i] = add(coeffs[i], mul(dd[k], basis[i]));
        if (k + 1 < n) {  // basis *= (x - (start + k))
            const Fr shift = fr_from_i64(-(start + (int64_t)k));
            for (size_t i = k + 1; i >= 1; --i) basis[i] = add(basis[i - 1], mul(basis[i], shift));
            basis[0] = mul(basis[0], shift);
        }
    }
    return coeffs;
}

void remainder_weights(const jolt_r1cs_rows& rows, const Fr& r0, const Fr& tau_high, std::vector<Fr>* fa, std::vector<Fr>* fb, Fr* scale) {
    const size_t per = 1 + rows.n_inputs;
    const std::vector<Fr> L = centered_lagrange_evals(rows.D, r0);
    fa->assign(rows.n_streams * per, Fr::zero());
    fb->assign(rows.n_streams * per, Fr::zero());
    for (uint32_t s = 0; s < rows.n_streams; ++s)
        for (uint32_t i = 0; i < rows.D; ++i) {
            const uint32_t slot = s * rows.D + i;
            Fr* a = fa->data() + s * per;
            Fr* b = fb->data() + s * per;
            a[0] = add(a[0], mul(L[i], fr_from_i64(rows.a_c0[slot])));
            b[0] = add(b[0], mul(L[i], fr_from_i128(rows.b_c0[2 * slot], rows.b_c0[2 * slot + 1])));
            for (uint32_t k = rows.a_off[slot]; k < rows.a_off[slot + 1]; ++k) a[1 + rows.a_col[k]] = add(a[1 + rows.a_col[k]], mul(L[i], fr_from_i64(rows.a_cf[k])));
            for (uint32_t k = rows.b_off[slot]; k < rows.b_off[slot + 1]; ++k) b[1 + rows.b_col[k]] = add(b[1 + rows.b_col[k]], mul(L[i], fr_from_i64(rows.b_cf[k])));
        }
    *scale = centered_lagrange_kernel(rows.D, tau_high, r0);
}

}  // namespace jolt_r1cs_rows_host

using namespace jolt_r1cs_rows_host;

namespace {

// L_i(x) over the nodes start .. start + D - 1 at an integer x, exactly: prod_{j != i} (x - x_j) / (x_i - x_j)
bool integer_lagrange(int64_t start, uint32_t D, uint32_t i, int64_t x, int64_t* out) {
    __int128 num = 1, den = 1;
    for (uint32_t j = 0; j < D; ++j) {
        if (j == i) continue;
        if (__builtin_mul_overflow(num, (__int128)(x - (start + (int64_t)j)), &num)) return false;
        den *= (__int128)((int64_t)i - (int64_t)j);  // |den| <= 15!
    }
    const __int128 q = num / den;  // exact: the value is an integer at an integer x
    if (q > (__int128)INT64_MAX || q < -(__int128)INT64_MAX) return false;
    *out = (int64_t)q;
    return true;
}

bool canonical(const jolt_fr_t* p, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (!fr_is_canonical(fr_from_abi(&p[i]))) return false;
    return true;
}

}  // namespace

extern "C" int32_t jolt_r1cs_rows_create(uint32_t n_streams, uint32_t domain_size, const uint32_t* rows_per_stream, uint32_t n_inputs, const uint32_t* a_offsets,
                                         const uint32_t* a_columns, const int64_t* a_coefficients, const int64_t* a_constants, const uint32_t* b_offsets,
                                         const uint32_t* b_columns, const int64_t* b_coefficients, const uint64_t* b_constants, int32_t zero_on_domain, jolt_r1cs_rows** out) {
    if (!out || !rows_per_stream || !a_offsets || !b_offsets || !a_constants || !b_constants) return JOLT_ERR_INVALID_ARG;
    if ((n_streams != 1 && n_streams != 2) || domain_size < 2 || domain_size > 16 || n_inputs == 0 || n_inputs > 64) return JOLT_ERR_INVALID_ARG;
    const uint32_t D = domain_size;
    uint32_t total = 0;
    for (uint32_t s = 0; s < n_streams; ++s) {
        if (rows_per_stream[s] > D) return JOLT_ERR_INVALID_ARG;
        total += rows_per_stream[s];
    }
    if (a_offsets[0] != 0 || b_offsets[0] != 0) return JOLT_ERR_INVALID_ARG;
    for (uint32_t r = 0; r < total; ++r)
        if (a_offsets[r + 1] < a_offsets[r] || b_offsets[r + 1] < b_offsets[r]) return JOLT_ERR_INVALID_ARG;
    if ((a_offsets[total] && (!a_columns || !a_coefficients)) || (b_offsets[total] && (!b_columns || !b_coefficients))) return JOLT_ERR_INVALID_ARG;
    for (uint32_t k = 0; k < a_offsets[total]; ++k)
        if (a_columns[k] >= n_inputs || a_coefficients[k] == INT64_MIN) return JOLT_ERR_INVALID_ARG;
    for (uint32_t k = 0; k < b_offsets[total]; ++k)
        if (b_columns[k] >= n_inputs || b_coefficients[k] == INT64_MIN) return JOLT_ERR_INVALID_ARG;
    for (uint32_t r = 0; r < total; ++r)
        if (a_constants[r] == INT64_MIN) return JOLT_ERR_INVALID_ARG;
    jolt_r1cs_rows* h = new (std::nothrow) jolt_r1cs_rows();
    if (!h) return JOLT_ERR_OOM;
    h->n_streams = n_streams;
    h->D = D;
    h->n_inputs = n_inputs;
    h->zero_on_domain = zero_on_domain != 0;
    const uint32_t slots = n_streams * D;
    h->a_off.assign(slots + 1, 0);
    h->b_off.assign(slots + 1, 0);
    h->a_c0.assign(slots, 0);
    h->b_c0.assign(2 * slots, 0);
    uint32_t row = 0;
    for (uint32_t s = 0; s < n_streams; ++s) {
        h->n_rows[s] = rows_per_stream[s];
        for (uint32_t i = 0; i < D; ++i) {
            const uint32_t slot = s * D + i;
            if (i < rows_per_stream[s]) {
                h->a_col.insert(h->a_col.end(), a_columns + a_offsets[row], a_columns + a_offsets[row + 1]);
                h->a_cf.insert(h->a_cf.end(), a_coefficients + a_offsets[row], a_coefficients + a_offsets[row + 1]);
                h->b_col.insert(h->b_col.end(), b_columns + b_offsets[row], b_columns + b_offsets[row + 1]);
                h->b_cf.insert(h->b_cf.end(), b_coefficients + b_offsets[row], b_coefficients + b_offsets[row + 1]);
                h->a_c0[slot] = a_constants[row];
                h->b_c0[2 * slot] = b_constants[2 * row];
                h->b_c0[2 * slot + 1] = b_constants[2 * row + 1];
                ++row;
            }
            h->a_off[slot + 1] = (uint32_t)h->a_col.size();
            h->b_off[slot + 1] = (uint32_t)h->b_col.size();
        }
    }
    // the 2D - 1 centred extended nodes (extended_start = -(D - 1)) against the domain's D nodes, as integers
    const int64_t start = centered_start(D), ext_start = centered_start(2 * D - 1);
    h->ext.assign((size_t)(2 * D - 1) * D, 0);
    for (uint32_t p = 0; p < 2 * D - 1; ++p) {
        const int64_t node = ext_start + (int64_t)p;
        const bool inside = node >= start && node < start + (int64_t)D;
        if (!(inside && h->zero_on_domain)) h->nodes.push_back(p);
        for (uint32_t i = 0; i < D; ++i)
            if (!integer_lagrange(start, D, i, node, &h->ext[(size_t)p * D + i])) {
                delete h;
                return JOLT_ERR_UNSUPPORTED;
            }
    }
    *out = h;
    return JOLT_OK;
}

extern "C" int32_t jolt_r1cs_rows_destroy(jolt_r1cs_rows* rows) {
    delete rows;
    return JOLT_OK;
}

extern "C" int32_t jolt_r1cs_rows_extension(const jolt_r1cs_rows* rows, int64_t* out) {
    if (!rows || !out) return JOLT_ERR_INVALID_ARG;
    std::memcpy(out, rows->ext.data(), rows->ext.size() * sizeof(int64_t));
    return JOLT_OK;
}

// the column form of the same system: wa / wb [node][stream][1 + n_inputs] = sum_i L_i(node) * row i, for the nodes the first round evaluates, when every entry has an int64
extern "C" int32_t jolt_r1cs_rows_fold_small(const jolt_r1cs_rows* rows, int64_t* a_weights, int64_t* b_weights, size_t* n_nodes) {
    if (!rows || !n_nodes) return JOLT_ERR_INVALID_ARG;
    *n_nodes = rows->nodes.size();
    if (!a_weights && !b_weights) return JOLT_OK;
    if (!a_weights || !b_weights) return JOLT_ERR_INVALID_ARG;
    const size_t per = 1 + rows->n_inputs;
    std::vector<__int128> wa(per), wb(per);
    for (size_t k = 0; k < rows->nodes.size(); ++k)
        for (uint32_t s = 0; s < rows->n_streams; ++s) {
            std::fill(wa.begin(), wa.end(), (__int128)0);
            std::fill(wb.begin(), wb.end(), (__int128)0);
            for (uint32_t i = 0; i < rows->D; ++i) {
                const __int128 l = rows->ext[(size_t)rows->nodes[k] * rows->D + i];
                const uint32_t slot = s * rows->D + i;
                const uint64_t lo = rows->b_c0[2 * slot], hi = rows->b_c0[2 * slot + 1];
                if (hi != ((lo >> 63) ? ~(uint64_t)0 : 0)) return JOLT_ERR_UNSUPPORTED;  // the constant alone has no int64
                wa[0] += l * rows->a_c0[slot];
                wb[0] += l * (int64_t)lo;
                for (uint32_t j = rows->a_off[slot]; j < rows->a_off[slot + 1]; ++j) wa[1 + rows->a_col[j]] += l * rows->a_cf[j];
                for (uint32_t j = rows->b_off[slot]; j < rows->b_off[slot + 1]; ++j) wb[1 + rows->b_col[j]] += l * rows->b_cf[j];
            }
            for (size_t v = 0; v < per; ++v) {
                if (wa[v] > INT64_MAX || wa[v] < -(__int128)INT64_MAX || wb[v] > INT64_MAX || wb[v] < -(__int128)INT64_MAX) return JOLT_ERR_UNSUPPORTED;
                a_weights[(k * rows->n_streams + s) * per + v] = (int64_t)wa[v];
                b_weights[(k * rows->n_streams + s) * per + v] = (int64_t)wb[v];
            }
        }
    return JOLT_OK;
}

extern "C" int32_t jolt_host_centered_lagrange_evals(size_t domain_size, const jolt_fr_t* r, jolt_fr_t* out) {
    if (!r || !out || domain_size == 0 || domain_size > 64 || !canonical(r, 1)) return JOLT_ERR_INVALID_ARG;
    const std::vector<Fr> v = centered_lagrange_evals(domain_size, fr_from_abi(r));
    for (size_t i = 0; i < domain_size; ++i) fr_to_abi(&out[i], v[i]);
    return JOLT_OK;
}

extern "C" int32_t jolt_host_centered_lagrange_kernel(size_t domain_size, const jolt_fr_t* x, const jolt_fr_t* y, jolt_fr_t* out) {
    if (!x || !y || !out || domain_size == 0 || domain_size > 64 || !canonical(x, 1) || !canonical(y, 1)) return JOLT_ERR_INVALID_ARG;
    fr_to_abi(out, centered_lagrange_kernel(domain_size, fr_from_abi(x), fr_from_abi(y)));
    return JOLT_OK;
}

extern "C" int32_t jolt_host_interpolate_to_coeffs(int64_t domain_start, const jolt_fr_t* values, size_t n, jolt_fr_t* out) {
    if (!values || !out || n == 0 || n > 256 || !canonical(values, n)) return JOLT_ERR_INVALID_ARG;
    std::vector<Fr> v(n);
    for (size_t i = 0; i < n; ++i) v[i] = fr_from_abi(&values[i]);
    const std::vector<Fr> c = interpolate_to_coeffs(domain_start, v);
    for (size_t i = 0; i < n; ++i) fr_to_abi(&out[i], c[i]);
    return JOLT_OK;
}

extern "C" int32_t jolt_host_uniskip_first_round_poly(size_t domain_size, const jolt_fr_t* tau_high, const jolt_fr_t* t1, jolt_fr_t* coeffs_out) {
    if (!tau_high || !t1 || !coeffs_out || domain_size < 2 || domain_size > 16 || !canonical(tau_high, 1) || !canonical(t1, 2 * domain_size - 1)) return JOLT_ERR_INVALID_ARG;
    const size_t D = domain_size, E = 2 * D - 1;
    const std::vector<Fr> kernel = interpolate_to_coeffs(centered_start(D), centered_lagrange_evals(D, fr_from_abi(tau_high)));
    std::vector<Fr> values(E);
    for (size_t i = 0; i < E; ++i) values[i] = fr_from_abi(&t1[i]);
    const std::vector<Fr> t1c = interpolate_to_coeffs(centered_start(E), values);
    std::vector<Fr> prod(D + E - 1, Fr::zero());  // poly_mul (lagrange.rs:540-556)
    for (size_t i = 0; i < D; ++i)
        for (size_t j = 0; j < E; ++j) prod[i + j] = add(prod[i + j], mul(kernel[i], t1c[j]));
    for (size_t i = 0; i < prod.size(); ++i) fr_to_abi(&coeffs_out[i], prod[i]);
    return JOLT_OK;
}

// prove_uniskip_clear (prover.rs:415-440) on any engine of the header
extern "C" int32_t jolt_host_prove_uniskip(jolt_host_transcript* transcript, const jolt_fr_t* coeffs, size_t n, size_t domain_size, const jolt_fr_t* input_claim,
                                           jolt_fr_t* r0_out, jolt_fr_t* output_claim_out) {
    if (!transcript || !coeffs || !input_claim || !r0_out || !output_claim_out || n == 0 || domain_size < 2 || domain_size > 16) return JOLT_ERR_INVALID_ARG;
    if (!canonical(coeffs, n) || !canonical(input_claim, 1)) return JOLT_ERR_INVALID_ARG;
    if (n - 1 > 3 * domain_size - 3) return JOLT_ERR_UNSUPPORTED;  // DegreeBoundExceeded (check_uniskip_round :395-400), as prove_batch reports it
    UnivariatePoly poly;
    poly.coefficients.resize(n);
    for (size_t i = 0; i < n; ++i) poly.coefficients[i] = fr_from_abi(&coeffs[i]);
    // CenteredIntegerDomain::check_round_sum (domain.rs:11-41, 107-118): sum_k c_k S_k with the i128 power sums S_k = sum_{t in domain} t^k (lagrange.rs:499-534);
    // a power sum that leaves i128 is the reference's InvalidIntegerDomain
    const int64_t start = centered_start(domain_size);
    std::vector<__int128> sums(n, 0);
    for (size_t o = 0; o < domain_size; ++o) {
        const __int128 t = start + (int64_t)o;
        __int128 pw = 1;
        for (size_t k = 0; k < n; ++k) {
            if (__builtin_add_overflow(sums[k], pw, &sums[k])) return JOLT_ERR_UNSUPPORTED;
            if (k + 1 < n && __builtin_mul_overflow(pw, t, &pw)) return JOLT_ERR_UNSUPPORTED;
        }
    }
    Fr actual = Fr::zero();
    for (size_t k = 0; k < n; ++k) {
        const bool negative = sums[k] < 0;
        const unsigned __int128 mag = negative ? (unsigned __int128)0 - (unsigned __int128)sums[k] : (unsigned __int128)sums[k];
        const Fr m = fr_from_i128((uint64_t)mag, (uint64_t)(mag >> 64) & ~((uint64_t)1 << 63));
        // (|S_k| < 2^127: the high word's sign bit is clear)
        actual = add(actual, mul(poly.coefficients[k], negative ? neg(m) : m));
    }
    if (actual != fr_from_abi(input_claim)) return JOLT_ERR_ROUND_CHECK;
    Transcript& tr = transcript->t;
    tr.append_label_with_count(kUniskipRoundLabel, (uint64_t)n);  // LabeledRoundPoly::uniskip (round_proof.rs:70-86): every coefficient
    for (size_t k = 0; k < n; ++k) tr.append_fr(poly.coefficients[k]);
    const Fr challenge = tr.challenge();
    const Fr claim = poly.evaluate(challenge);
    tr.append_label("opening_claim");  // OPENING_CLAIM_TRANSCRIPT_LABEL (crates/jolt-sumcheck/src/lib.rs:111), append_labeled (legacy.rs:51-54)
    tr.append_fr(claim);
    fr_to_abi(r0_out, challenge);
    fr_to_abi(output_claim_out, claim);
    return JOLT_OK;
}

// one cycle through r1cs_rows.hip.h on the host: values = the inputs of the cycle as the column kinds store them (2 words each; a U64 / I64 column uses the first)
extern "C" int32_t jolt_host_r1cs_rows_cycle(const jolt_r1cs_rows* rows, const uint64_t* values, const int32_t* kinds, uint32_t stream, uint32_t node, uint64_t* az_out /* 2 */,
                                             uint64_t* bz_out /* 4 */, uint64_t* product_out /* 4 */, int32_t* negative_out) {
    if (!rows || !values || !kinds || !az_out || !bz_out || !product_out || !negative_out || stream >= rows->n_streams || node >= 2 * rows->D - 1) return JOLT_ERR_INVALID_ARG;
    for (uint32_t c = 0; c < rows->n_inputs; ++c)
        if (kinds[c] != JOLT_INT_U64 && kinds[c] != JOLT_INT_I64 && kinds[c] != JOLT_INT_I128) return JOLT_ERR_INVALID_ARG;
    const RowsView rv = rows->host_view();
    unsigned __int128 a[16];
    I192 b[16];
    rows_cycle_values<16>(rv, stream, [&](uint32_t c) { return load_small(values + 2 * c, kinds[c], 0); }, a, b);
    unsigned __int128 az;
    I256 bz;
    rows_extend<16>(rv.ext + (size_t)node * rv.D, rv.D, a, b, &az, &bz);
    uint32_t mag[8];
    *negative_out = rows_product(az, bz, mag) ? 1 : 0;
    az_out[0] = (uint64_t)az;
    az_out[1] = (uint64_t)(az >> 64);
    for (int j = 0; j < 4; ++j) {
        bz_out[j] = bz.w[j];
        product_out[j] = ((uint64_t)mag[2 * j + 1] << 32) | mag[2 * j];
    }
    return JOLT_OK;
}

extern "C" int32_t jolt_host_r1cs_rows_remainder_weights(const jolt_r1cs_rows* rows, const jolt_fr_t* r0, const jolt_fr_t* tau_high, jolt_fr_t* a_weights, jolt_fr_t* b_weights,
                                                         jolt_fr_t* scale) {
    if (!rows || !r0 || !tau_high || !a_weights || !b_weights || !scale || !canonical(r0, 1) || !canonical(tau_high, 1)) return JOLT_ERR_INVALID_ARG;
    std::vector<Fr> fa, fb;
    Fr k;
    remainder_weights(*rows, fr_from_abi(r0), fr_from_abi(tau_high), &fa, &fb, &k);
    for (size_t i = 0; i < fa.size(); ++i) {
        fr_to_abi(&a_weights[i], fa[i]);
        fr_to_abi(&b_weights[i], fb[i]);
    }
    fr_to_abi(scale, k);
    return JOLT_OK;
}
