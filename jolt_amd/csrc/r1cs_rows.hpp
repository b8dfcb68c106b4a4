// jolt_amd/csrc/r1cs_rows.hpp -- the object behind jolt_r1cs_rows: a constraint system as rows over a centred uni-skip domain (r1cs_rows.hip).
#pragma once
#include <vector>

#include "ctx.hpp"
#include "r1cs_rows.hip.h"

struct jolt_r1cs_rows {
    uint32_t n_streams = 0, D = 0, n_inputs = 0;
    uint32_t n_rows[2] = {0, 0};
    bool zero_on_domain = false;
    // slot = stream * D + domain position; an unoccupied slot is an empty row
    std::vector<uint32_t> a_off, a_col, b_off, b_col;
    std::vector<int64_t> a_cf, a_c0, b_cf;
    std::vector<uint64_t> b_c0;    // 2 per slot
    std::vector<int64_t> ext;      // (2D - 1) x D integer extension coefficients L_i(node)
    std::vector<uint32_t> nodes;   // extended-domain positions the first round evaluates

    jolt::RowsView host_view() const {
        return jolt::RowsView{a_off.data(), a_col.data(), a_cf.data(), a_c0.data(), b_off.data(), b_col.data(), b_cf.data(), b_c0.data(), ext.data(), nodes.data(), D, (uint32_t)nodes.size()};
    }
};

namespace jolt_r1cs_rows_host {
using jolt::Fr;
int64_t centered_start(size_t n);                                        // lagrange.rs:484-492
Fr fr_from_i64(int64_t v);
Fr fr_from_i128(uint64_t lo, uint64_t hi);                               // two's complement
std::vector<Fr> centered_lagrange_evals(size_t D, const Fr& r);          // lagrange.rs:20-77
Fr centered_lagrange_kernel(size_t D, const Fr& x, const Fr& y);         // :92-104
std::vector<Fr> interpolate_to_coeffs(int64_t start, const std::vector<Fr>& values);  // :567-608
// fa / fb: [stream][1 + n_inputs] column weights of the remainder at the uni-skip challenge r0, scale = LK(tau_high, r0)
void remainder_weights(const jolt_r1cs_rows& rows, const Fr& r0, const Fr& tau_high, std::vector<Fr>* fa, std::vector<Fr>* fb, Fr* scale);
}  // namespace jolt_r1cs_rows_host
