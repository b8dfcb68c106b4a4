"""The precommitted claim reductions without a device: the host operator (jolt_stage_host_precommitted_create / _address_create) and the two host permutation
helpers against the definition restated in tests/precommitted_model.py -- every coefficient, the coefficient COUNT (3 in an active round, 1 in an inactive one),
intermediate and final claims; alone under the four transcript engines; as the offset-0 member of a padded batch beside a tail-aligned dense member; and every
refusal of the contract.  All comparisons are bit for bit: the arithmetic is exact."""
import numpy as np
import pytest

import oracle_lib as O
import precommitted_model as M
from precommitted_model import SCHEDULES, schedule
from jolt_amd import ffi
from util import rand_fr

ENGINES = [0, ffi.TRANSCRIPT_BLAKE2B, ffi.TRANSCRIPT_KECCAK, ffi.TRANSCRIPT_BLAKE2B_SPONGE]
INVALID_ARG, SIZE_MISMATCH, NOT_FULLY_BOUND = 1, 5, 7


def tables(n, n_aux, seed):
    t = [rand_fr(1 << n, 100 * seed + k) for k in range(2 + n_aux)]
    return t, [M.ints(x) for x in t]


def same_message(got, want, where):
    assert got.shape[0] == len(want), f"{where}: {got.shape[0]} coefficients, the definition has {len(want)}"
    assert M.ints(got) == want, where


def drive_against_model(op, phase, claim, seed, where):
    """the operator under test and the model's phase round by round under the same challenges -> the claim after the last round"""
    challenges = M.ints(rand_fr(max(phase.num_rounds(), 1), seed))
    assert op.rounds == phase.num_rounds() and op.degree == 2
    bind = None
    for rnd in range(phase.num_rounds()):
        got = op.prove_round(None if bind is None else M.limbs([bind])[0], rnd, M.limbs([claim])[0])
        want = phase.prove_round(bind, rnd, claim)
        same_message(got, want, f"{where}, round {rnd}")
        bind = challenges[rnd]
        claim = M.evaluate(want, bind)
    op.finish_rounds(M.limbs([bind])[0])
    phase.finish_rounds(bind)
    return claim


@pytest.mark.parametrize("kind", SCHEDULES)
@pytest.mark.parametrize("n_aux", [0, 1, 3])
@pytest.mark.parametrize("n", [1, 2, 3, 6])
def test_host_operator_is_the_definition(n, n_aux, kind):
    ca, ct, aa, at = schedule(kind, n)
    t, ti = tables(n, n_aux, 7 * n + n_aux)
    red = M.Reduction(ti[0], ti[1], ti[2:], ca, ct, aa, at)
    op = ffi.stage_host_precommitted(t[0], t[1], t[2:], ca, ct, aa, at)
    claim = red.input_claim()
    assert M.ints(op.input_claim()) == [claim]
    claim = drive_against_model(op, red.cycle, claim, 31 + n, f"{kind} cycle")
    assert M.ints(op.output_claims()) == red.cycle.output_claims()
    if not aa:
        assert len(op.output_claims()) == 1 + n_aux
        # the running claim is the bound summand at the accumulated scale
        assert claim == red.tables.value[0] * red.tables.eq[0] * red.tables.scale % M.R
        return
    assert red.cycle.output_claims() == [claim]  # the intermediate claim IS the running claim (nothing was padded here)
    adr = ffi.stage_host_precommitted_address(op)
    assert M.ints(op.output_claims()) == [claim]  # the cycle operator keeps answering after the reclaim
    assert M.ints(adr.input_claim()) == [claim]
    phase = red.address()
    claim = drive_against_model(adr, phase, claim, 57 + n, f"{kind} address")
    assert M.ints(adr.output_claims()) == phase.output_claims() and len(adr.output_claims()) == 1 + n_aux
    assert claim == red.tables.value[0] * red.tables.eq[0] * red.tables.scale % M.R


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("kind", ["middle", "two_phase"])
def test_alone_under_every_transcript_engine(kind, engine):
    n, n_aux = 3, 2
    ca, ct, aa, at = schedule(kind, n)
    t, ti = tables(n, n_aux, 91)
    red = M.Reduction(ti[0], ti[1], ti[2:], ca, ct, aa, at)
    op = ffi.stage_host_precommitted(t[0], t[1], t[2:], ca, ct, aa, at)
    phases = [(op, red.cycle)]
    claim = red.input_claim()
    for which in range(2 if aa else 1):
        if which:
            phases.append((ffi.stage_host_precommitted_address(op), red.address()))
        o, phase = phases[which]
        label = engine | (20 + which)
        mine, theirs = ffi.HostTranscript(label), O.MockTranscript(label)
        got = o.prove_alone(mine, M.limbs([claim])[0])
        bind = None
        for rnd in range(phase.num_rounds()):
            want = phase.prove_round(bind, rnd, claim)
            same_message(got["polys"][rnd], want, f"{kind}, phase {which}, round {rnd}")
            for c in M.limbs(want):
                theirs.append_fr(c)
            bind = M.ints(theirs.challenge())[0]
            assert M.ints(got["challenges"][rnd]) == [bind]
            claim = M.evaluate(want, bind)
        phase.finish_rounds(bind)
        assert M.ints(got["final_claim"]) == [claim]
        assert M.ints(o.output_claims()) == phase.output_claims()
        mine.close()


def windowed(op, cuts):
    return [op.window(a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]


def test_round_windows_carry_the_challenge_across():
    """jolt_stage_op_window over the operator: the phases of one schedule under two drivers see the same messages"""
    n, n_aux = 4, 1
    ca, ct, aa, at = schedule("middle", n)
    t, ti = tables(n, n_aux, 17)
    red = M.Reduction(ti[0], ti[1], ti[2:], ca, ct, aa, at)
    op = ffi.stage_host_precommitted(t[0], t[1], t[2:], ca, ct, aa, at)
    claim, bind, rnd = red.input_claim(), None, 0
    challenges = M.ints(rand_fr(ct, 18))
    for w in windowed(op, [0, 2, ct]):
        for local in range(w.rounds):
            got = w.prove_round(None if local == 0 else M.limbs([bind])[0], local, M.limbs([claim])[0])
            want = red.cycle.prove_round(bind, rnd, claim)
            same_message(got, want, f"window round {rnd}")
            bind = challenges[rnd]
            claim = M.evaluate(want, bind)
            rnd += 1
        w.finish_rounds(M.limbs([bind])[0])
    red.cycle.finish_rounds(bind)
    assert M.ints(op.output_claims()) == red.cycle.output_claims()


@pytest.mark.parametrize("challenge_mode", [0, 1])
@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("kind", ["all", "head", "middle", "two_phase"])
def test_offset_zero_member_of_a_padded_batch(kind, grouped, challenge_mode):
    """max_num_vars = rounds + 3: the member's claim enters the batch times 2^3 and the hint carries that factor into the emitted quadratic (the padded-claim path)"""
    n, n_aux = 3, 2
    ca, ct, aa, at = schedule(kind, n)
    t, ti = tables(n, n_aux, 23)
    max_num_vars = ct + 3
    dense_rounds = ct + 1  # a tail-aligned dense member that starts two rounds in: it overlaps the reduction's window and outlives it
    dt = [rand_fr(1 << dense_rounds, 300 + k) for k in range(3)]
    terms = [(rand_fr(1, 310)[0], [0, 1, 2]), (rand_fr(1, 311)[0], [2])]

    def model_members():
        red = M.Reduction(ti[0], ti[1], ti[2:], ca, ct, aa, at)
        return red, [red.cycle, M.OracleExpr(dt, terms, 3)]

    red, members = model_members()
    claims = [red.input_claim(), members[1].input_claim()]
    coeffs = M.ints(rand_fr(2, 320))
    offsets = [0, max_num_vars - dense_rounds]
    label = 77 + challenge_mode
    want = M.prove_batch(members, claims, coeffs, offsets, max_num_vars, 3, label=label, challenge_mode=challenge_mode)
    ops = [ffi.stage_host_precommitted(t[0], t[1], t[2:], ca, ct, aa, at), ffi.stage_host_expr(dt, terms, 3)]
    fn = ffi.prove_batch_ops_grouped if grouped else ffi.prove_batch_ops
    got = fn(ops, list(M.limbs(claims)), list(M.limbs(coeffs)), offsets, max_num_vars, 3, label=label, challenge_mode=challenge_mode)
    for rnd in range(max_num_vars):
        assert M.ints(got["polys"][rnd]) == want["polys"][rnd], f"round {rnd}"
    assert M.ints(got["challenges"]) == want["challenges"]
    assert M.ints(got["member_claims"]) == want["member_claims"] and M.ints(got["final_claim"]) == [want["final_claim"]]
    assert M.ints(ops[0].output_claims()) == red.cycle.output_claims()
    # the padding is IN the messages: the same reduction alone, under the same challenges, emits other quadratics in its active rounds
    alone, _ = M.drive(model_members()[0].cycle, claims[0], want["challenges"][:ct])
    padded, _ = M.drive(model_members()[0].cycle, claims[0] * 8 % M.R, want["challenges"][:ct])
    first_active = ca[0] if ca else None
    if first_active is not None:
        assert alone[first_active][0] == padded[first_active][0] and alone[first_active][2] != padded[first_active][2]


def test_batch_on_a_held_transcript():
    n, n_aux = 2, 1
    ca, ct, aa, at = schedule("tail", n)
    t, ti = tables(n, n_aux, 29)
    red = M.Reduction(ti[0], ti[1], ti[2:], ca, ct, aa, at)
    claims, coeffs = [red.input_claim()], M.ints(rand_fr(1, 30))
    want = M.prove_batch([red.cycle], claims, coeffs, [0], ct + 3, 2, label=5)
    op = ffi.stage_host_precommitted(t[0], t[1], t[2:], ca, ct, aa, at)
    tr = ffi.HostTranscript(5)
    got = ffi.prove_batch_ops_on([op], list(M.limbs(claims)), list(M.limbs(coeffs)), [0], ct + 3, 2, tr)
    assert [M.ints(p) for p in got["polys"]] == want["polys"] and M.ints(got["final_claim"]) == [want["final_claim"]]
    assert M.ints(op.output_claims()) == red.cycle.output_claims()
    tr.close()


# ---- the permutation helpers ------------------------------------------------------------------------------------------------------------------------------
def permutations(n):
    rng = np.random.default_rng(n)
    out = [list(range(n)), list(range(n))[::-1], [int(x) for x in rng.permutation(n)]]
    out.append([3 * x + 5 for x in out[2]])  # opening rounds are global indices: only their order matters
    return out


@pytest.mark.parametrize("n", [1, 2, 5, 9])
def test_lsb_permutation_and_challenge_permute(n):
    for perm_be in permutations(n):
        want, same = M.lsb_permutation(perm_be)
        got, got_same = ffi.host_precommitted_lsb_permutation(perm_be)
        assert got == want and got_same == same
        c = rand_fr(n, 40 + n)
        assert M.ints(ffi.host_precommitted_permute_challenges(c, got)) == M.permute_challenges(M.ints(c), want)
    # the big-endian identity round order is the REVERSAL of the LSB order, and an ascending one is the identity of neither: pin one by hand
    assert ffi.host_precommitted_lsb_permutation([2, 1, 0]) == ([0, 1, 2], True)
    if n >= 2:
        assert not ffi.host_precommitted_lsb_permutation(list(range(n)))[1]
    # the two permutes are ONE relabeling: eq of the permuted challenges is the permuted eq table
    perm_be = permutations(n)[2]
    m, _ = M.lsb_permutation(perm_be)
    r = M.ints(rand_fr(n, 50 + n))
    assert M.eq_table(M.permute_challenges(r, m)) == M.permute_coefficients(M.eq_table(r), m)


def test_permutation_helpers_refuse():
    with pytest.raises(ffi.JoltError) as e:
        ffi.host_precommitted_lsb_permutation([4, 1, 4])
    assert e.value.status == INVALID_ARG
    with pytest.raises(ValueError):
        M.lsb_permutation([4, 1, 4])
    for bad in ([0, 0, 1], [0, 1, 3]):
        with pytest.raises(ffi.JoltError) as e:
            ffi.host_precommitted_permute_challenges(rand_fr(3, 1), bad)
        assert e.value.status == INVALID_ARG


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------------------
def refused(status, *args, **kw):
    with pytest.raises(ffi.JoltError) as e:
        ffi.stage_host_precommitted(*args, **kw)
    assert e.value.status == status, e.value


def test_constructor_refusals():
    v, e, a = rand_fr(8, 1), rand_fr(8, 2), rand_fr(8, 3)
    ffi.stage_host_precommitted(v, e, [a], [0, 1, 2], 3).destroy()  # the control
    refused(SIZE_MISMATCH, v, e, [a], [0, 1], 3)                      # n_cycle_active + n_address_active != n
    refused(SIZE_MISMATCH, v, e, [a], [0, 1, 2], 3, [0], 1)
    refused(INVALID_ARG, v[:6], e[:6], [], [0, 1, 2], 3)              # a length that is not a power of two
    refused(INVALID_ARG, v, e, [a], [0, 2, 1], 3)                     # unsorted
    refused(INVALID_ARG, v, e, [a], [0, 1, 1], 3)                     # a round twice
    refused(INVALID_ARG, v, e, [a], [0, 1, 3], 3)                     # out of range
    refused(INVALID_ARG, v, e, [a], [0, 1], 2, [1], 1)                # address round out of range
    refused(INVALID_ARG, v, e, [a], [0], 1, [1, 0], 2)                # address rounds unsorted
    refused(INVALID_ARG, v[:1], e[:1], [], [], 0)                     # a cycle phase has at least one round
    bad = v.copy()
    bad[3] = np.array([2**64 - 1] * 4, dtype=np.uint64)               # not a canonical field element
    refused(INVALID_ARG, bad, e, [a], [0, 1, 2], 3)
    # 257 passengers
    refused(INVALID_ARG, v, e, [a] * 257, [0, 1, 2], 3)
    ffi.stage_host_precommitted(v[:2], e[:2], [a[:2]] * 256, [0], 1).destroy()


def test_device_constructor_refuses_tables_of_unequal_length_without_a_device():
    """the length comparison of the device constructor needs tables, hence a device; the host constructor takes ONE length for all its tables, so a short table cannot
    be expressed there.  What can be checked here: both null tables and a null context are refused before anything is touched."""
    import ctypes as C
    h = C.c_void_p()
    st = ffi.lib().jolt_stage_precommitted_cycle_create(None, None, None, None, C.c_size_t(0), None, C.c_size_t(0), C.c_size_t(1), None, C.c_size_t(0), C.c_size_t(0), C.byref(h))
    assert st == INVALID_ARG and not h
    st = ffi.lib().jolt_stage_precommitted_address_create(None, None, C.byref(h))
    assert st == INVALID_ARG and not h


def test_claims_before_full_binding_and_round_order():
    t, ti = tables(2, 1, 5)
    op = ffi.stage_host_precommitted(t[0], t[1], t[2:], [0, 1], 2)
    with pytest.raises(ffi.JoltError) as e:
        op.output_claims()
    assert e.value.status == NOT_FULLY_BOUND
    claim = op.input_claim()
    r = rand_fr(1, 6)[0]
    with pytest.raises(ffi.JoltError) as e:  # round 1 before round 0
        op.prove_round(r, 1, claim)
    assert e.value.status == INVALID_ARG
    with pytest.raises(ffi.JoltError):  # a bind in round 0
        op.prove_round(r, 0, claim)
    msg = op.prove_round(None, 0, claim)
    with pytest.raises(ffi.JoltError) as e:  # one variable is still free
        op.output_claims()
    assert e.value.status == NOT_FULLY_BOUND
    with pytest.raises(ffi.JoltError):  # finish before the last round
        op.finish_rounds(r)
    with pytest.raises(ffi.JoltError):  # round 0 again
        op.prove_round(None, 0, claim)
    op.prove_round(r, 1, O.univariate_evaluate(msg, r))
    with pytest.raises(ffi.JoltError) as e:
        op.output_claims()
    assert e.value.status == NOT_FULLY_BOUND
    op.finish_rounds(r)
    assert len(op.output_claims()) == 2
    with pytest.raises(ffi.JoltError):  # and nothing after the end
        op.finish_rounds(r)


def test_the_carry_is_reclaimed_once_from_a_finished_operator():
    t, ti = tables(2, 1, 8)
    r = rand_fr(1, 9)[0]
    cycle_only = ffi.stage_host_precommitted(t[0], t[1], t[2:], [0, 1], 2)
    with pytest.raises(ffi.JoltError) as e:  # no address phase scheduled
        ffi.stage_host_precommitted_address(cycle_only)
    assert e.value.status == INVALID_ARG
    op = ffi.stage_host_precommitted(t[0], t[1], t[2:], [0], 1, [0], 1)
    assert len(op.output_claims()) == 1  # the intermediate claim exists before any round: it is the input claim
    assert np.array_equal(op.output_claims()[0], op.input_claim())
    with pytest.raises(ffi.JoltError) as e:  # not finished
        ffi.stage_host_precommitted_address(op)
    assert e.value.status == INVALID_ARG
    op.prove_round(None, 0, op.input_claim())
    with pytest.raises(ffi.JoltError):
        ffi.stage_host_precommitted_address(op)
    op.finish_rounds(r)
    adr = ffi.stage_host_precommitted_address(op)
    with pytest.raises(ffi.JoltError) as e:  # a second reclaim of one carry
        ffi.stage_host_precommitted_address(op)
    assert e.value.status == INVALID_ARG
    with pytest.raises(ffi.JoltError):  # an address operator parks nothing
        ffi.stage_host_precommitted_address(adr)
    with pytest.raises(ffi.JoltError):  # nor does any other operator
        ffi.stage_host_precommitted_address(ffi.stage_host_expr([t[0]], [(rand_fr(1, 1)[0], [0])], 1))
    with pytest.raises(ffi.JoltError) as e:
        adr.output_claims()
    assert e.value.status == NOT_FULLY_BOUND
