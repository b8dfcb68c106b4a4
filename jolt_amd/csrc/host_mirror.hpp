// jolt_amd/csrc/host_mirror.hpp -- host-side mirror of the reference interfaces that CALL the hot path.
//
// The reference's host code is Rust and stays Rust in a real deployment; this image has no Rust
// toolchain, so the callers are restated in C++ ABOVE the C ABI of include/jolt_hip.h, with the reference's names,
// argument meaning and error behaviour, so that the parity tests read like the reference's own:
//   ProveRounds / RoundScheduler / SequentialRounds / prove_batch   crates/jolt-sumcheck/src/prover.rs:52-362
//   BatchMember / BatchPrelude                                       crates/jolt-sumcheck/src/batch.rs:23-72
//   UnivariatePoly::{from_evals, evaluate, compress}                 crates/jolt-poly/src/univariate.rs
//   GruenSplitEqPolynomial::gruen_poly_deg_3                         crates/jolt-poly/src/split_eq.rs:383-417
//   Transcript                                                       crates/jolt-transcript/src/legacy.rs:55-100
#pragma once
#include <functional>
#include <memory>
#include <vector>

#include "ctx.hpp"

// jolt_round_group_prove with a host callback that runs after the round has been enqueued and before its sums are awaited
// (capi.hip): work that does not depend on the sums overlaps with the device.
int32_t jolt_internal_round_group_prove(jolt_ctx* ctx, jolt_member* const* members, size_t n, const jolt_fr_t* const* binds, jolt_fr_t* evals_out,
                                        size_t cap, const std::function<void()>* overlap);

namespace jolt_host {

using jolt::Fr;

struct UnivariatePoly {
    std::vector<Fr> coefficients;
    static UnivariatePoly from_evals(const Fr* evals, size_t n);  // univariate.rs:198-202
    Fr evaluate(const Fr& x) const;
    size_t degree() const;  // index of the last stored coefficient (univariate.rs `degree`)
};

// SumcheckError (crates/jolt-sumcheck/src/error.rs) as status codes of include/jolt_hip.h
struct SumcheckError {
    int32_t status = JOLT_OK;
    size_t round = 0;
};

// Fiat-Shamir surface the path needs (crates/jolt-transcript/src/legacy.rs:32-100): absorb bytes, squeeze a challenge, and the reference's encodings of what the path
// absorbs -- a field element as 32 BIG-endian bytes (legacy.rs:116-123), the 32-byte label words (legacy.rs:146-209), a compressed labelled round polynomial
// (crates/jolt-sumcheck/src/round_proof.rs:129-143).
struct Transcript {
    virtual ~Transcript() = default;
    virtual void append_bytes(const uint8_t* b, size_t n) = 0;
    virtual void draw16(uint8_t out[16]) = 0;  // the 16 squeezed bytes behind either challenge shape
    virtual void state(uint8_t out[32]) const = 0;  // Transcript::state
    virtual Transcript* clone() const = 0;          // an independent copy in the same state (the Dory verifier draws its last challenge from one)
    Fr challenge();         // Transcript::challenge: 16 bytes -> from_challenge_bytes (125-bit shape)
    Fr challenge_scalar();  // Transcript::challenge_scalar: 16 bytes -> from_scalar_challenge_bytes
    void append_fr(const Fr& v);
    void append_label(const char* label);                             // Label
    void append_label_with_count(const char* label, uint64_t count);  // LabelWithCount
    void append_u64_word(uint64_t v);                                 // U64Word
    void append_round_poly(const char* label, const Fr* coefficients, size_t n);  // CompressedLabeledRoundPoly::append_to_transcript
};
constexpr const char* kSumcheckRoundLabel = "sumcheck_poly";  // crates/jolt-sumcheck/src/lib.rs:105
constexpr const char* kUniskipRoundLabel = "uniskip_poly";    // :107

// Deterministic test transcript; re-implemented from the SPEC comment in oracle/mock_transcript.h.
struct MockTranscript final : Transcript {
    uint64_t s[4];
    explicit MockTranscript(uint64_t label);
    void append_bytes(const uint8_t* b, size_t n) override;
    void draw16(uint8_t out[16]) override;
    void state(uint8_t out[32]) const override;
    Transcript* clone() const override { return new MockTranscript(*this); }

   private:
    void absorb_word(uint64_t w);
};

// jolt_transcript::LegacyBlake2bTranscript = DigestTranscript<Blake2b<U32>> (crates/jolt-transcript/src/digest.rs:84-189, lib.rs:70-75): the transcript of the
// reference's benchmark profile (crates/jolt-prover/src/profile.rs:69).  Chained digests: state' = H(state || 28 zero bytes || n_rounds u32 BE || payload).
struct LegacyBlake2bTranscript final : Transcript {
    uint8_t chain[32];
    uint32_t n_rounds = 0;
    LegacyBlake2bTranscript(const uint8_t* label, size_t n);  // n <= 32 (MAX_LABEL_LEN, legacy.rs:17)
    void append_bytes(const uint8_t* b, size_t n) override;
    void draw16(uint8_t out[16]) override;
    void state(uint8_t out[32]) const override;
    Transcript* clone() const override { return new LegacyBlake2bTranscript(*this); }

   private:
    void step(const uint8_t* payload, size_t n);
};

// jolt_transcript::KeccakTranscript = SpongeTranscript<spongefish::instantiations::Keccak> (legacy.rs:211-305): spongefish's duplex sponge over Keccak-f[1600]
// (overwrite mode, rate 136, zero initial state; spongefish rev d2d190b1 is a Cargo dependency, restated from its published construction) behind the facade's framing.
struct KeccakSpongeTranscript final : Transcript {
    uint8_t lanes[200];
    unsigned absorb_pos = 0, squeeze_pos = 136;
    KeccakSpongeTranscript(const uint8_t* label, size_t n);
    void append_bytes(const uint8_t* b, size_t n) override;
    void draw16(uint8_t out[16]) override;
    void state(uint8_t out[32]) const override;
    Transcript* clone() const override { return new KeccakSpongeTranscript(*this); }

   private:
    void absorb(const uint8_t* b, size_t n);
    void squeeze(uint8_t* out, size_t n);
};

// jolt_transcript::Blake2bTranscript = SpongeTranscript<spongefish::instantiations::Blake2b512> (lib.rs:63-66): the facade's framing over spongefish's hash-to-duplex
// bridge.  The reference's known-answer vector (tests/blake2b_tests.rs:13-37) pins it through the FIRST challenge; how a squeeze is closed before the next absorb is
// restated from the crate's published source without a vector -- unpinned there, used by no parity claim and not by the bench.
struct Blake2bSpongeTranscript final : Transcript {
    struct Bridge;
    std::shared_ptr<Bridge> bridge;  // shared_ptr only for the incomplete type; copied deeply by state()
    Blake2bSpongeTranscript(const uint8_t* label, size_t n);
    void append_bytes(const uint8_t* b, size_t n) override;
    void draw16(uint8_t out[16]) override;
    void state(uint8_t out[32]) const override;
    Transcript* clone() const override;
};

// What a 64-bit transcript label of the C ABI selects: the two top bits name the engine (0 the test transcript, 1 LegacyBlake2b, 2 Keccak sponge, 3 Blake2b512 sponge; for 1 - 3 the session
// label is the ASCII string "jolt-amd/<label mod 2^62>"), or an engine with a byte label as the reference writes it (`Transcript::new(b"Jolt")`).
struct LabelledTranscript final : Transcript {
    std::unique_ptr<Transcript> inner;
    explicit LabelledTranscript(uint64_t label);
    LabelledTranscript(int kind, const uint8_t* label, size_t n);  // inner stays null for an unknown kind / a label over 32 bytes
    void append_bytes(const uint8_t* b, size_t n) override { inner->append_bytes(b, n); }
    void draw16(uint8_t out[16]) override { inner->draw16(out); }
    void state(uint8_t out[32]) const override { inner->state(out); }
    Transcript* clone() const override {
        LabelledTranscript* c = new LabelledTranscript();
        if (inner) c->inner.reset(inner->clone());
        return c;
    }

   private:
    LabelledTranscript() = default;
};
void blake2b_digest(const uint8_t* in, size_t n, size_t outlen, uint8_t* out);  // RFC 7693, unkeyed
void keccak_f1600(uint8_t lanes[200]);                                             // FIPS 202

// prover.rs:52-72
struct ProveRounds {
    virtual ~ProveRounds() = default;
    virtual size_t num_rounds() const = 0;
    virtual int32_t prove_round(const Fr* bind, size_t round, const Fr& previous_claim, UnivariatePoly* out) = 0;
    virtual int32_t finish_rounds(const Fr& bind) = 0;
    // the device member whose rounds ARE this object's rounds (its round sums may be fetched together with other members', MemberGroupedRounds); NULL: none
    virtual jolt_member* group_member() const { return nullptr; }
};

// A batch member whose tables live on the GPU: calls jolt_member_prove_round / jolt_member_finish and assembles the
// round message exactly as the reference kernels do (from_evals + round check, naive.rs:298-309; gruen_poly_deg_3 for
// the split-eq member, ram_hamming_booleanity.rs:128-135).
struct DeviceMember final : ProveRounds {
    jolt_member* m;
    explicit DeviceMember(jolt_member* member) : m(member) {}
    size_t num_rounds() const override;
    int32_t prove_round(const Fr* bind, size_t round, const Fr& previous_claim, UnivariatePoly* out) override;
    int32_t finish_rounds(const Fr& bind) override;
    // message assembly from the device sums (shared with the grouped scheduler)
    int32_t assemble(const Fr* evals, const Fr& previous_claim, UnivariatePoly* out, const Fr* inv_l1 = nullptr) const;
    // l(1) = scalar * w_i of the NEXT round message, given the bind that the round applies first (split-eq members)
    bool next_l1(bool has_bind, const Fr& bind, Fr* l1) const;
    size_t n_evals() const;
    jolt_member* group_member() const override { return m; }
};

// prover.rs:74-107
struct MemberRound {
    size_t index, local_round;
    bool has_bind;
    Fr bind;
    Fr claim;
    ProveRounds* member;
    bool has_message;
    UnivariatePoly message;
};
struct MemberFinish {
    Fr bind;
    ProveRounds* member;
};
// prover.rs:110-120
struct RoundScheduler {
    virtual ~RoundScheduler() = default;
    virtual int32_t batch_prove_round(std::vector<MemberRound>& work) = 0;
    virtual int32_t batch_finish_rounds(std::vector<MemberFinish>& finishes) = 0;
};
struct SequentialRounds final : RoundScheduler {  // prover.rs:124-146
    int32_t batch_prove_round(std::vector<MemberRound>& work) override;
    int32_t batch_finish_rounds(std::vector<MemberFinish>& finishes) override;
};
// What BuildRoundScheduler (crates/jolt-kernels/src/backend.rs:68-70) would return for this backend: all device members
// of a round are enqueued back to back and fetched with ONE copy + ONE sync (jolt_round_group_prove).
struct DeviceGroupedRounds final : RoundScheduler {
    jolt_ctx* ctx;
    explicit DeviceGroupedRounds(jolt_ctx* c) : ctx(c) {}
    int32_t batch_prove_round(std::vector<MemberRound>& work) override;
    int32_t batch_finish_rounds(std::vector<MemberFinish>& finishes) override;
};
// BuildRoundScheduler for a batch that MIXES device members with other ProveRounds objects (a protocol stage: catalogue relations beside stage operators): per round
// the members that name a device member (ProveRounds::group_member) go into ONE jolt_round_group_prove per context, the final binds into ONE jolt_round_group_finish;
// everything else runs as under SequentialRounds, after the group.  The messages are SequentialRounds' messages: the grouping changes launches, not values.
struct MemberGroupedRounds final : RoundScheduler {
    int32_t batch_prove_round(std::vector<MemberRound>& work) override;
    int32_t batch_finish_rounds(std::vector<MemberFinish>& finishes) override;
};

// batch.rs:23-72
struct BatchMember {
    Fr input_claim, coefficient;
    size_t rounds, offset;
};
struct BatchPrelude {
    std::vector<BatchMember> members;
    Fr claimed_sum;
    size_t max_num_vars, max_degree;
    static BatchPrelude make(std::vector<BatchMember> members, size_t max_num_vars, size_t max_degree);
};
struct ProvedBatch {  // prover.rs:152-157
    std::vector<Fr> challenges;
    Fr final_claim;
    std::vector<Fr> member_claims;
    std::vector<UnivariatePoly> round_polys;  // what ClearSumcheckRecorder keeps (recorder.rs:126)
};

// prover.rs:193-362.  `full_width_challenges` selects challenge_scalar() (test hook for the non-shifted bind path).
int32_t prove_batch(const BatchPrelude& prelude, std::vector<ProveRounds*>& members, RoundScheduler& scheduler, Transcript& transcript,
                    bool full_width_challenges, ProvedBatch* out, SumcheckError* err);

Fr fr_mul_pow_2(Fr a, size_t k);
// `inv_l1` (optional): 1 / (current_scalar * point_i), computed by the caller while the device was busy with the round
// (the one field inversion of the message assembly; it does not depend on the round sums).  Verified before use.
int32_t gruen_poly_deg_3(const Fr& current_scalar, const Fr& point_i, const Fr& q_constant, const Fr& q_quadratic, const Fr& s0_plus_s1,
                         UnivariatePoly* out, const Fr* inv_l1 = nullptr);
int32_t gruen_poly_from_q(const Fr& current_scalar, const Fr& point_i, const Fr* q_evals, size_t dq, const Fr& s0_plus_s1, UnivariatePoly* out,
                          const Fr* inv_l1 = nullptr);
Fr inverse_or_given(const Fr& x, const Fr* given);
void fr_to_bytes_le(const Fr& a, uint8_t out[32]);
Fr fr_from_challenge_bytes(const uint8_t* b, size_t n);
Fr fr_from_scalar_challenge_bytes(const uint8_t* b, size_t n);

}  // namespace jolt_host

// the object behind jolt_host_transcript_* (host_mirror.hip); the drivers that prove on a transcript the caller holds reach the engine through it
struct jolt_host_transcript {
    jolt_host::LabelledTranscript t;
    explicit jolt_host_transcript(uint64_t label) : t(label) {}
    jolt_host_transcript(int kind, const uint8_t* label, size_t n) : t(kind, label, n) {}
    jolt_host_transcript(const jolt_host_transcript& other) : t(0) { t.inner.reset(other.t.inner ? other.t.inner->clone() : nullptr); }
};
