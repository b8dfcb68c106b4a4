"""Replay checker for multi-operator stage batches (TEST INFRASTRUCTURE).

A member whose window ends with the batch (offset = max_num_vars - rounds) is handed, inside prove_batch (crates/jolt-sumcheck/src/prover.rs:193-362), exactly what it is
handed alone: its own input claim (the 2^(max - rounds) padding is halved away by the inactive rounds in front of it) and the challenges of its own rounds,
challenges[offset:].  So every member's messages can be computed by its oracle twin fed those challenges (`ReplayTranscript`, `replay_member`), and `check_batch`
restates the driver (oracle/sumcheck.c orc_prove_batch) in Python over the oracle's field operations and transcript: it batches the twins' messages, compares the
batched polynomial with the one under test coefficient for coefficient, and draws the challenge ITSELF.  Round r's challenge depends only on the batched polynomials
of rounds <= r, which are the oracle's given the challenges of rounds < r -- so equality of every polynomial and every challenge, by induction over the rounds, is
equality with the oracle's batch.  Nothing on the checking side comes from the library under test except `got`.

A window that does not end with the batch would hand the member a scaled claim (prover.rs:241-245): no twin computes that without a scaled kernel, so it is refused."""
import numpy as np

import oracle_lib as O


class ReplayTranscript:
    """A transcript whose challenges are prescribed: `challenge()` hands them out in order and raises when they run out, `append` / `append_fr` record what was
    absorbed.  Fits the `Tr` objects of tests/workload_oracle.py (append, challenge) and the places that take an O.MockTranscript (append_fr, challenge)."""

    def __init__(self, challenges):
        self.challenges = np.ascontiguousarray(challenges, dtype=np.uint64).reshape(-1, 4).copy()
        self.drawn, self.absorbed = 0, []

    def append(self, values):
        self.absorbed.append(np.array(values, dtype=np.uint64).reshape(-1, 4))

    append_fr = append

    def challenge(self):
        if self.drawn >= self.challenges.shape[0]:
            raise IndexError(f"ReplayTranscript: challenge {self.drawn} asked for, {self.challenges.shape[0]} prescribed")
        self.drawn += 1
        return self.challenges[self.drawn - 1].copy()


def replay_member(member, claim, challenges):
    """An O.Member driven through the ProveRounds contract under prescribed challenges (the loop of tests/test_gpu_sumcheck.py lockstep): per round
    prove_round(bind, claim), the claim becomes the message at the challenge; finish_rounds with the last one.
    -> dict(polys = per round the (degree + 1, 4) coefficients, challenges, final_claim, final_values)"""
    challenges = np.ascontiguousarray(challenges, dtype=np.uint64).reshape(-1, 4)
    rounds = member.num_rounds()
    if challenges.shape[0] != rounds:
        raise ValueError(f"replay_member: {challenges.shape[0]} challenges for a member of {rounds} rounds")
    polys, bind, claim = [], None, np.asarray(claim, dtype=np.uint64).reshape(4)
    for rnd in range(rounds):
        poly = member.prove_round(bind, claim)
        bind = challenges[rnd]
        claim = O.univariate_evaluate(poly, bind)
        polys.append(poly)
    if bind is not None:
        member.finish_rounds(bind)
    return dict(polys=polys, challenges=challenges.copy(), final_claim=claim, final_values=member.final_values())


def _v(a):
    return np.ascontiguousarray(a, dtype=np.uint64).reshape(1, 4)


def check_batch(got, member_polys, input_claims, coefficients, offsets, rounds_per_member, max_num_vars, max_degree, label=0, challenge_mode=0):
    """`got`: what a prove_batch under test returned (polys (max_num_vars, max_degree + 1, 4), challenges, member_claims, final_claim).  member_polys[i]: member i's
    replayed messages, one coefficient array per round of its window.  Raises AssertionError at the first difference, naming the round and the coefficient."""
    n = len(member_polys)
    assert len(input_claims) == n and len(coefficients) == n and len(offsets) == n and len(rounds_per_member) == n
    zero, one = np.zeros(4, dtype=np.uint64), O.to_mont([1])[0]
    two_inv = O.fr_inv(O.to_mont([2]))[0]
    mul = lambda a, b: O.fr_mul(_v(a), _v(b))[0]
    add = lambda a, b: O.fr_add(_v(a), _v(b))[0]
    stride = max_degree + 1
    got_polys = np.asarray(got["polys"], dtype=np.uint64).reshape(max_num_vars, stride, 4)
    got_challenges = np.asarray(got["challenges"], dtype=np.uint64).reshape(max_num_vars, 4)
    member_claims, running = [], zero
    for i in range(n):
        rounds = rounds_per_member[i]
        assert rounds <= max_num_vars and offsets[i] == max_num_vars - rounds, \
            f"member {i}: offset {offsets[i]} with {rounds} of {max_num_vars} rounds is not a tail-aligned window (the member would see a scaled claim)"
        assert len(member_polys[i]) == rounds, f"member {i}: {len(member_polys[i])} replayed messages for {rounds} rounds"
        member_claims.append(O.fr_mul_pow_2(np.asarray(input_claims[i], dtype=np.uint64).reshape(4), max_num_vars - rounds))  # prover.rs:244-249
        running = add(running, mul(coefficients[i], member_claims[i]))
    tr = O.MockTranscript(label)
    for rnd in range(max_num_vars):
        batched = np.zeros((stride, 4), dtype=np.uint64)
        active = []
        for i in range(n):
            if rnd < offsets[i]:  # prover.rs:273-282: the constant claim / 2
                member_claims[i] = mul(member_claims[i], two_inv)
                batched[0] = add(batched[0], mul(coefficients[i], member_claims[i]))
                continue
            poly = np.asarray(member_polys[i][rnd - offsets[i]], dtype=np.uint64).reshape(-1, 4)
            assert poly.shape[0] <= stride, f"member {i}, round {rnd}: degree {poly.shape[0] - 1} above max_degree {max_degree}"
            batched[:poly.shape[0]] = O.fr_add(batched[:poly.shape[0]], O.fr_mul(np.repeat(_v(coefficients[i]), poly.shape[0], axis=0), poly))
            active.append((i, poly))
        s1 = zero
        for k in range(stride):
            s1 = add(s1, batched[k])
        assert np.array_equal(add(batched[0], s1), running), f"round {rnd}: s(0) + s(1) of the replayed batch is not the running claim"  # prover.rs:316-324
        for k in range(stride):
            assert np.array_equal(batched[k], got_polys[rnd, k]), f"round {rnd}, coefficient {k}: the batch under test differs from the replayed members' " \
                f"(active members: {[i for i, _ in active]})"
        ncoef = stride
        while ncoef > 2 and not batched[ncoef - 1].any():
            ncoef -= 1
        tr.append_round_poly(batched[:ncoef])
        challenge = tr.challenge_scalar() if challenge_mode else tr.challenge()
        assert np.array_equal(challenge, got_challenges[rnd]), f"round {rnd}: the challenge drawn from the replayed messages is not the batch's"
        running = O.univariate_evaluate(batched, challenge)
        for i, poly in active:
            member_claims[i] = O.univariate_evaluate(poly, challenge)
    for i in range(n):
        assert np.array_equal(member_claims[i], np.asarray(got["member_claims"])[i]), f"member {i}: claim after the last round"
    assert np.array_equal(running, np.asarray(got["final_claim"]).reshape(4)), "final claim"
    return dict(member_claims=np.stack(member_claims) if n else np.zeros((0, 4), dtype=np.uint64), final_claim=running)
