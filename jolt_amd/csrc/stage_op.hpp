// jolt_amd/csrc/stage_op.hpp -- the object behind a jolt_stage_op handle (stage_ops.hip, precommitted.hip): one stage operator as a ProveRounds with output claims.
#pragma once
#include <map>
#include <string>
#include <vector>

#include "host_mirror.hpp"

struct jolt_stage_op : jolt_host::ProveRounds {
    jolt_ctx* ctx = nullptr;
    size_t rounds = 0, degree = 0;  // degree: the largest degree a round message can have
    std::vector<Fr> binds;          // the challenges received so far, in round order
    std::map<std::string, std::vector<Fr>> kept;  // intermediate values the parity tests compare (scan sums, pushforward masses, ...): host copies, O(K)
    Fr carry = Fr::zero();          // a window's last challenge, waiting for the next window's first round (jolt_stage_op_window)
    bool has_carry = false;
    const char* name = "";

    size_t num_rounds() const override { return rounds; }
    virtual int32_t output_claims(std::vector<Fr>* out) = 0;
    virtual int32_t input_claim(Fr* /*out*/) { return JOLT_ERR_UNSUPPORTED; }

    int32_t fail(int32_t st, const std::string& what) const {
        if (ctx && st != JOLT_OK && ctx->last_error.empty()) ctx->last_error = std::string(name) + ": " + what;
        return st;
    }
};
