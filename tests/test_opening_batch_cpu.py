"""The framing of a homomorphic batch opening (HomomorphicBatch::prove_batch, crates/jolt-openings/src/schemes.rs:487-524) on the host:
jolt_host_opening_statement_absorb and jolt_host_opening_claim_absorb, and the G2 generator constant of jolt_amd/dory_setup.py.

Pins, in order of strength:
  * LegacyBlake2bTranscript: the bytes the two entries absorb, against a restatement over hashlib alone of claims.rs:23-35,79-88 and legacy.rs:82-91,116-123 on top
    of digest.rs -- 32-byte padded labels, the count big-endian in bytes 24..32, field elements as 32 big-endian bytes, one digest per append, one for the challenge;
  * all four engines: state and challenges against the oracle's transcript driven with the same appends (a separately written implementation);
  * the G2 generator against the big-integer model's derivation."""
import hashlib

import numpy as np
import pytest

import oracle_lib as O
from jolt_amd import dory_setup, ffi
from test_transcript_cpu import DigestModel, R_MOD, fr_int
from util import rand_fr

ENGINES = [0, 1, 2, 3]


def mont(v):
    return O.to_mont([v % R_MOD])[0]


def powers_of(gamma, n):
    """1, gamma, ..., gamma^(n - 1) as canonical integers"""
    out, p = [], 1
    for _ in range(n):
        out.append(p)
        p = p * gamma % R_MOD
    return out


def oracle_statement(t, evaluations):
    """VerifierRlcClaims::append_to_transcript, then challenge_scalar_powers's ONE challenge, on the oracle's transcript -> gamma"""
    t.append_label_with_count(b"rlc_claims", len(evaluations))
    for v in evaluations:
        t.append_fr(v)
    return t.challenge_scalar()


def oracle_claim(t, point, value):
    """EvaluationClaim::append_to_transcript on the oracle's transcript"""
    t.append_label_with_count(b"opening_point", len(point))
    for c in point:
        t.append_fr(c)
    t.append_label(b"opening_eval")
    t.append_fr(value)


@pytest.mark.parametrize("n", [1, 2, 38])
def test_blake2b_absorbed_bytes_against_hashlib(n):
    evaluations, point, value = rand_fr(n, 3100 + n), rand_fr(2 * n + 1, 3200 + n), rand_fr(1, 3300 + n)[0]
    model, mine = DigestModel(b"Jolt"), ffi.HostTranscript(b"Jolt", kind=1)
    # ---- the statement
    model.append_bytes(b"rlc_claims".ljust(24, b"\0") + n.to_bytes(8, "big"))
    for v in evaluations:
        model.append_bytes(fr_int(v).to_bytes(32, "big"))
    scalars = ffi.host_opening_statement_absorb(mine, evaluations)
    # challenge_scalar (digest.rs:184-188, bn254/mod.rs:189-193): 16 bytes of the next digest, reversed, as a little-endian integer reduced modulo r
    gamma = int.from_bytes(model.challenge_bytes16(), "big") % R_MOD
    assert mine.state() == model.state
    assert [fr_int(s) for s in scalars] == powers_of(gamma, n)
    # ---- the closing claim
    model.append_bytes(b"opening_point".ljust(24, b"\0") + len(point).to_bytes(8, "big"))
    for c in point:
        model.append_bytes(fr_int(c).to_bytes(32, "big"))
    model.append_bytes(b"opening_eval".ljust(32, b"\0"))
    model.append_bytes(fr_int(value).to_bytes(32, "big"))
    ffi.host_opening_claim_absorb(mine, point, value)
    assert mine.state() == model.state
    assert model.n_rounds == (1 + n + 1) + (1 + len(point) + 1 + 1)  # one digest per append and one for the challenge: nothing else went in
    mine.close()


@pytest.mark.parametrize("kind", ENGINES)
@pytest.mark.parametrize("n", [1, 2, 38])
def test_framing_against_the_oracle_transcript(kind, n):
    label = (kind << 62) | (5000 + n)
    evaluations, point, value = rand_fr(n, 3400 + n), rand_fr(n + 3, 3500 + n), rand_fr(1, 3600 + n)[0]
    orc, mine = O.MockTranscript(label), ffi.HostTranscript(label)
    prefix = rand_fr(2, 3700)  # the statement is absorbed into a transcript that already holds the proof so far
    for v in prefix:
        orc.append_fr(v)
    mine.append(prefix)
    gamma = oracle_statement(orc, evaluations)
    scalars = ffi.host_opening_statement_absorb(mine, evaluations)
    assert scalars.shape == (n, 4)
    assert np.array_equal(scalars[0], mont(1))
    assert [fr_int(s) for s in scalars] == powers_of(fr_int(gamma), n)
    assert orc.state() == mine.state()
    oracle_claim(orc, point, value)
    ffi.host_opening_claim_absorb(mine, point, value)
    assert orc.state() == mine.state()
    assert np.array_equal(orc.challenge_scalar(), mine.challenge(full_width=True))
    assert np.array_equal(orc.challenge(), mine.challenge())
    mine.close()


@pytest.mark.parametrize("kind", ENGINES)
def test_every_absorbed_value_binds(kind):
    label = (kind << 62) | 5100
    n = 5
    evaluations, point, value = rand_fr(n, 3800), rand_fr(7, 3801), rand_fr(1, 3802)[0]

    def run(evs, pt, val):
        t = ffi.HostTranscript(label)
        scalars = ffi.host_opening_statement_absorb(t, evs)
        mid = t.state()
        ffi.host_opening_claim_absorb(t, pt, val)
        end = t.state()
        t.close()
        return scalars, mid, end

    base_scalars, base_mid, base_end = run(evaluations, point, value)
    again = run(evaluations, point, value)
    assert np.array_equal(again[0], base_scalars) and again[1:] == (base_mid, base_end)
    for i in range(n):  # one evaluation altered: another gamma
        evs = evaluations.copy()
        evs[i] = O.fr_add(evs[i:i + 1], mont(1).reshape(1, 4))[0]
        scalars, _, _ = run(evs, point, value)
        assert not np.array_equal(scalars[1], base_scalars[1]), i
    swapped = evaluations.copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    assert not np.array_equal(run(swapped, point, value)[0][1], base_scalars[1])  # the order binds too
    for i in range(len(point)):  # one coordinate altered: the statement's part is the same, the state after the claim is not
        pt = point.copy()
        pt[i] = O.fr_add(pt[i:i + 1], mont(1).reshape(1, 4))[0]
        _, mid, end = run(evaluations, pt, value)
        assert mid == base_mid and end != base_end, i
    _, mid, end = run(evaluations, point, O.fr_add(value.reshape(1, 4), mont(1).reshape(1, 4))[0])
    assert mid == base_mid and end != base_end
    _, mid, end = run(evaluations, point[:-1], value)  # the count is absorbed
    assert end != base_end


def test_refusals_absorb_nothing():
    t = ffi.HostTranscript(ffi.TRANSCRIPT_BLAKE2B | 5200)
    before = t.state()
    with pytest.raises(ffi.JoltError) as e:  # an empty batch: the reference refuses it (HomomorphicBatchStatement::new)
        ffi.host_opening_statement_absorb(t, np.zeros((0, 4), dtype=np.uint64))
    assert e.value.status == 1  # JOLT_ERR_INVALID_ARG
    bad = rand_fr(3, 3900)
    bad[2] = np.full(4, 2**64 - 1, dtype=np.uint64)  # not canonical
    with pytest.raises(ffi.JoltError):
        ffi.host_opening_statement_absorb(t, bad)
    with pytest.raises(ffi.JoltError):
        ffi.host_opening_claim_absorb(t, bad, bad[0])
    with pytest.raises(ffi.JoltError):
        ffi.host_opening_claim_absorb(t, bad[:2], bad[2])
    assert t.state() == before
    ffi.host_opening_claim_absorb(t, np.zeros((0, 4), dtype=np.uint64), bad[0])  # a point of no coordinates is a claim about a constant
    assert t.state() != before
    t.close()


def test_g2_generator_constant_is_the_models():
    import g2_model as M
    x, y = dory_setup.G2_GENERATOR
    assert (x, y) == M.GENERATOR
    assert M.on_curve((x, y))                       # on the twist y^2 = x^3 + 3 / (9 + u)
    assert M.mul((x, y), M.R) is None               # of order r (r is prime and the point is not the identity)
    assert M.from_abi(dory_setup.g2_generator()) == M.GENERATOR
    assert np.array_equal(dory_setup.g2_generator(), M.to_abi(M.GENERATOR))
    assert np.array_equal(dory_setup.g1_generator(), O.g1_generator())
    assert dory_setup.Q == M.Q


def test_setup_base_arrays_are_checked():
    g1, g2 = np.zeros((4, 12), dtype=np.uint64), np.zeros((4, 24), dtype=np.uint64)
    ok = dory_setup.check(dict(gamma1=g1, gamma2=g2, h1=g1[0], h2=g2[0]))
    assert ok["gamma1"].shape == (4, 12) and ok["h2"].shape == (24,)
    with pytest.raises(ValueError):
        dory_setup.check(dict(gamma1=g1, gamma2=g2, h1=g1[0]))
    with pytest.raises(ValueError):
        dory_setup.check(dict(gamma1=g1[:3], gamma2=g2[:3], h1=g1[0], h2=g2[0]))
    with pytest.raises(ValueError):
        dory_setup.check(dict(gamma1=g1, gamma2=g2[:2], h1=g1[0], h2=g2[0]))


def test_the_new_entry_points_are_exported():
    for name in ("jolt_host_opening_statement_absorb", "jolt_host_opening_claim_absorb", "jolt_host_dory_prove_batch", "jolt_grid_evaluate_columns"):
        assert hasattr(ffi.lib(), name), name
    assert hashlib.blake2b(b"", digest_size=32).digest() == ffi.host_blake2b(b"", 32)  # the restatement above and the library share nothing but the specification
