"""A Dory evaluation proof as ONE call of the library: jolt_host_dory_open / jolt_host_dory_open_with_transcript (dory_scheme.hip) behind prove(), and the proof
with its messages by name.

dory_open.DoryOpening and dory_reduce.DoryReduce drive the same protocol message by message from here, with every challenge handed in; they stay, as the second
implementation the tests compare this one against.  Here the library runs the whole prover's side -- state, VMV message, sigma rounds, fold-scalars, final message --
and draws each challenge from a transcript after the message that precedes it:

    transcript=HostTranscript   one of the library's engines; every element goes in as the reference's adapter absorbs a group element
                                (LabelWithCount(b"dory_group", len) and the compressed bytes), every challenge is challenge_scalar
    callback=f                  the caller's own transcript: f(phase, round, gts, g1s, g2s) absorbs the message and returns the challenge after it
                                (beta for DORY_PHASE_FIRST, alpha for _SECOND, gamma for _GAMMA, None for _VMV and _FINAL), or an int status that aborts

The order of the appends is the message order above; dory-pcs's own order is pinned by nothing in the reference checkout (docs/parity.md), which is what the
callback form is for.  Transparent mode only.
"""
import numpy as np

from . import ffi

DoryProofSetup = ffi.DoryLibSetup  # jolt_dory_setup: DoryProofSetup(ctx, gamma1, gamma2, h1, h2), .n, .tier2(hints), .verifier(), .combine(commitments, scalars), .close()


class DoryProof:
    """vmv = (C, D2, E1); rounds[k] = (first, second) with first = (D1L, D1R, D2L, D2R, E1beta, E2beta) and second = (C+, C-, E1+, E1-, E2+, E2-);
    final = (w1, w2); challenges[k] = (beta_k, alpha_k); gamma.  GT elements are (48,), G1 points (12,), G2 points (24,), challenges (4,) uint64 arrays."""

    def __init__(self, sigma, gts, g1s, g2s, challenges):
        if (gts.shape[0], g1s.shape[0], g2s.shape[0], challenges.shape[0]) != ffi.host_dory_proof_counts(sigma):
            raise ValueError("the arrays are not those of an opening of 2^sigma columns")
        self.sigma, self.gts, self.g1s, self.g2s = sigma, gts, g1s, g2s
        self.vmv = (gts[0], gts[1], g1s[0])
        self.rounds = []
        for k in range(sigma):
            t, a, b = gts[2 + 6 * k:8 + 6 * k], g1s[1 + 3 * k:4 + 3 * k], g2s[3 * k:3 * k + 3]
            self.rounds.append(((t[0], t[1], t[2], t[3], a[0], b[0]), (t[4], t[5], a[1], a[2], b[1], b[2])))
        self.final = (g1s[1 + 3 * sigma], g2s[3 * sigma])
        self.challenges = [(challenges[2 * k], challenges[2 * k + 1]) for k in range(sigma)]
        self.gamma = challenges[2 * sigma]

    def elements(self):
        """every element in the order a transcript absorbs them"""
        out = list(self.vmv)
        for first, second in self.rounds:
            out += list(first) + list(second)
        return out + list(self.final)


def prove(setup, hints, scalars, v_table, left, right, nu, sigma, transcript=None, callback=None):
    """The inputs of dory_open.DoryOpening over a DoryProofSetup: resident G1 hints (DoryVec or views) of at most 2^nu rows with one scalar each, the device tables
    v = L^T M (2^sigma entries), L (2^nu) and R (2^sigma).  The library checks everything before it enqueues anything and refuses with a JoltError."""
    out = setup.ctx.dory_open(setup, hints, scalars, v_table, left, right, nu, sigma, transcript=transcript, callback=callback)
    return DoryProof(sigma, out["gts"], out["g1s"], out["g2s"], out["challenges"])


def verify(setup, commitment, y, left, right, nu, sigma, proof, transcript=None, callback=None):
    """DoryScheme::verify as one call over a DoryProofSetup: proof a DoryProof (or a dict(gts, g1s, g2s)), left / right host arrays of 2^nu / 2^sigma field elements.
    The callback form is prove()'s, asked once more for d with DORY_PHASE_D.  -> (accepted, failed_check)"""
    p = proof if isinstance(proof, dict) else dict(gts=proof.gts, g1s=proof.g1s, g2s=proof.g2s)
    return setup.ctx.dory_verify(setup.verifier(), commitment, y, left, right, nu, sigma, p, transcript=transcript, callback=callback)


def absorb(transcript, elements):
    """what jolt_host_dory_open appends for a message: each element through jolt_host_dory_transcript_append_*"""
    for e in elements:
        ffi.host_dory_transcript_append(transcript, np.asarray(e))
