// jolt_amd/csrc/hyperkzg_transcript.hpp -- the Fiat-Shamir steps of a HyperKZG opening, shared by the prover (hyperkzg.hip) and the verifier (hyperkzg_verify.hip):
// the verifier replays a proof through the absorb code the prover ran.
//
// Three absorb-then-challenge steps: the level commitments -> r (scheme.rs:148-152, :188-192), the 3 ell evaluations -> q (kzg.rs:88-95, :152-159), the three witness
// commitments -> d_0 (kzg.rs:118-124, :162-166).
#pragma once
#include <cstring>

#include "ctx.hpp"
#include "g1.hip.h"
#include "host_mirror.hpp"

namespace jolt {
namespace hyperkzg_host {

using jolt_host::LabelledTranscript;
using jolt_host::Transcript;

inline void append_g1(Transcript& tr, const G1Jac& p) {
    uint8_t b[32];
    jolt_g1_t abi;
    std::memcpy(&abi, &p, sizeof(abi));
    jolt_host_g1_serialize_compressed(&abi, b);
    tr.append_bytes(b, 32);
}

// The opening's Fiat-Shamir: the library's test transcript, or the CALLER's (jolt_open_transcript_fn: the reference's Blake2b / Keccak transcript stays in Rust).
struct OpenTranscript {
    LabelledTranscript mock;
    jolt_open_transcript_fn fn;
    void* user;
    int32_t after_points(int32_t phase, const G1Jac* pts, size_t n, Fr* out) {
        if (!fn) {
            for (size_t i = 0; i < n; ++i) append_g1(mock, pts[i]);
            *out = mock.challenge();
            return JOLT_OK;
        }
        static_assert(sizeof(G1Jac) == sizeof(jolt_g1_t), "a Jacobian point crosses the ABI as it lies in memory");
        jolt_fr_t ch;
        JOLT_TRY(fn(user, phase, reinterpret_cast<const jolt_g1_t*>(pts), n, nullptr, 0, &ch));
        *out = fr_from_abi(&ch);
        return fr_is_canonical(*out) ? JOLT_OK : JOLT_ERR_INVALID_ARG;
    }
    int32_t after_values(int32_t phase, const jolt_fr_t* vals, size_t n, Fr* out) {
        if (!fn) {
            for (size_t i = 0; i < n; ++i) mock.append_fr(fr_from_abi(&vals[i]));
            *out = mock.challenge();
            return JOLT_OK;
        }
        jolt_fr_t ch;
        JOLT_TRY(fn(user, phase, nullptr, 0, vals, n, &ch));
        *out = fr_from_abi(&ch);
        return fr_is_canonical(*out) ? JOLT_OK : JOLT_ERR_INVALID_ARG;
    }
};

// A jolt_open_transcript_fn over one of the library's engines: `user` is a jolt_host_transcript.  It absorbs and draws as OpenTranscript does on its own engine,
// so an opening and a verification under it stand where jolt_host_hyperkzg_open(label) stands on a fresh jolt_host_transcript_create(label).
inline int32_t open_engine_fn(void* user, int32_t, const jolt_g1_t* points, size_t n_points, const jolt_fr_t* values, size_t n_values, jolt_fr_t* challenge_out) {
    jolt_host_transcript* t = (jolt_host_transcript*)user;
    if (!t || !t->t.inner || !challenge_out) return JOLT_ERR_INVALID_ARG;
    for (size_t i = 0; i < n_points; ++i) {
        G1Jac p;
        std::memcpy(&p, &points[i], sizeof(p));
        append_g1(t->t, p);
    }
    for (size_t i = 0; i < n_values; ++i) t->t.append_fr(fr_from_abi(&values[i]));
    fr_to_abi(challenge_out, t->t.challenge());
    return JOLT_OK;
}

}  // namespace hyperkzg_host
}  // namespace jolt

// jolt_host_hyperkzg_open_grid under a caller's callback, with the statement's check (hyperkzg.hip): when `expected_eval` is given, the last folded level (two entries)
// is read back after the folds and evaluated at point[0]; a value other than *expected_eval is JOLT_ERR_ROUND_CHECK before the callback has been called.
// hint == NULL or levels == 0: every level commitment by MSM.
int32_t jolt_internal_hyperkzg_open_grid_checked(jolt_ctx* ctx, const jolt_srs* srs, const jolt_table* evals, const jolt_fr_t* point, size_t ell, jolt_open_transcript_fn fn,
                                                 void* user, const jolt_grid_hint* hint, uint32_t levels, const jolt_fr_t* onehot_scalars, jolt_table* const* dense,
                                                 size_t n_dense, const jolt_fr_t* dense_scalars, const jolt::Fr* expected_eval, jolt_g1_t* com, jolt_g1_t* w, jolt_fr_t* v,
                                                 jolt_fr_t* challenges_out);
