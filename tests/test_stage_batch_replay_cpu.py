"""The replay checker of tests/stage_batch_replay.py on the CPU (no device): `check_batch` over members replayed under a batch's challenges accepts exactly what the C
oracle's prove_batch (oracle/sumcheck.c) and the library's prove_batch over host-only operators (jolt_host_prove_batch_ops over jolt_stage_host_expr_create) produce --
2 to 5 members, degrees 1 to 4, different round counts in tail-aligned windows, both challenge modes, the test transcript and the three reference engines -- and refuses
a batch in which one coefficient of one message, one challenge, one batching coefficient or one offset is off.  The replay paths of the oracle twins
(tests/workload_oracle.py) reproduce the twins' own transcripts when fed their own challenges."""
import numpy as np
import pytest

import oracle_lib as O
from jolt_amd import ffi
from stage_batch_replay import ReplayTranscript, check_batch, replay_member
import util
from util import rand_fr
from workload_oracle import OracleExtended

ENGINES = [0, ffi.TRANSCRIPT_BLAKE2B, ffi.TRANSCRIPT_KECCAK, ffi.TRANSCRIPT_BLAKE2B_SPONGE]


def random_batch(seed, with_gruen=True):
    """A description of a batch: per member (tables, terms, degree) or ("gruen", a, b, w); rounds 1 .. max in tail-aligned windows, at least one member over all rounds"""
    rng = np.random.default_rng([seed, 0xBA7C])
    n = int(rng.integers(2, 6))
    max_num_vars = int(rng.integers(3, 7))
    rounds = [int(rng.integers(1, max_num_vars + 1)) for _ in range(n)]
    rounds[int(rng.integers(0, n))] = max_num_vars
    descs = []
    for i, r in enumerate(rounds):
        s = 1000 * seed + 50 * i
        if with_gruen and rng.random() < 0.2:
            descs.append(("gruen", rand_fr(1 << r, s), rand_fr(1 << r, s + 1), rand_fr(r, s + 2)))
            continue
        degree = int(rng.integers(1, 5))
        n_tables = degree + int(rng.integers(0, 2))
        shape = [list(rng.permutation(n_tables)[:degree])]  # one term of full degree ...
        for _ in range(int(rng.integers(0, 3))):  # ... and up to two more of any degree <= it, a table possibly repeated
            shape.append(list(rng.integers(0, n_tables, size=int(rng.integers(1, degree + 1)))))
        tabs = [rand_fr(1 << r, s + k) for k in range(n_tables)]
        terms = [(rand_fr(1, s + 20 + k)[0], [int(t) for t in term]) for k, term in enumerate(shape)]
        descs.append((tabs, terms, degree))
    degrees = [3 if d[0] == "gruen" else d[2] for d in descs]
    return dict(descs=descs, rounds=rounds, offsets=[max_num_vars - r for r in rounds], max_num_vars=max_num_vars, max_degree=max(degrees), coeffs=list(rand_fr(n, 7 * seed + 1)))


def oracle_members(b):
    return [O.Member.gruen_product(*d[1:]) if d[0] == "gruen" else O.Member.expr(*d) for d in b["descs"]]


def replayed(b, claims, challenges):
    """every member of the batch alone, under the challenges of its own window"""
    return [replay_member(m, c, challenges[off:])["polys"] for m, c, off in zip(oracle_members(b), claims, b["offsets"])]


@pytest.mark.parametrize("challenge_mode", [0, 1])
@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5, 6])
def test_the_checker_accepts_the_oracle_batch(seed, engine, challenge_mode):
    b = random_batch(seed)
    ms = oracle_members(b)
    claims = [m.input_claim() for m in ms]
    label = engine | (40 + seed)
    got = O.prove_batch(ms, claims, b["coeffs"], b["offsets"], b["max_num_vars"], b["max_degree"], label=label, challenge_mode=challenge_mode)
    out = check_batch(got, replayed(b, claims, got["challenges"]), claims, b["coeffs"], b["offsets"], b["rounds"], b["max_num_vars"], b["max_degree"], label, challenge_mode)
    assert np.array_equal(out["final_claim"], got["final_claim"])
    # the replayed members end where the batch's members ended
    for m, again, c, off in zip(ms, oracle_members(b), claims, b["offsets"]):
        assert np.array_equal(replay_member(again, c, got["challenges"][off:])["final_values"], m.final_values())


@pytest.mark.parametrize("challenge_mode", [0, 1])
@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5, 6])
def test_the_checker_accepts_the_batch_over_host_operators(seed, engine, challenge_mode):
    """the same batches (dense members only: the host-only operator is one) through jolt_host_prove_batch_ops; the claims and the replayed messages are the oracle's"""
    b = random_batch(seed, with_gruen=False)
    ops = [ffi.stage_host_expr(*d) for d in b["descs"]]
    claims = [m.input_claim() for m in oracle_members(b)]
    assert all(np.array_equal(op.input_claim(), c) for op, c in zip(ops, claims))
    assert [op.rounds for op in ops] == b["rounds"]
    label = engine | (60 + seed)
    got = ffi.prove_batch_ops(ops, claims, b["coeffs"], b["offsets"], b["max_num_vars"], b["max_degree"], label=label, challenge_mode=challenge_mode)
    check_batch(got, replayed(b, claims, got["challenges"]), claims, b["coeffs"], b["offsets"], b["rounds"], b["max_num_vars"], b["max_degree"], label, challenge_mode)
    for op, m, c, off in zip(ops, oracle_members(b), claims, b["offsets"]):
        assert np.array_equal(np.stack(op.output_claims()), replay_member(m, c, got["challenges"][off:])["final_values"])
        op.destroy()


def control():
    """one fixed batch that passes: -> (got, kwargs of check_batch)"""
    b = random_batch(3, with_gruen=False)
    ms = oracle_members(b)
    claims = [m.input_claim() for m in ms]
    got = O.prove_batch(ms, claims, b["coeffs"], b["offsets"], b["max_num_vars"], b["max_degree"], label=9)
    args = dict(member_polys=replayed(b, claims, got["challenges"]), input_claims=claims, coefficients=b["coeffs"], offsets=list(b["offsets"]), rounds_per_member=b["rounds"],
                max_num_vars=b["max_num_vars"], max_degree=b["max_degree"], label=9, challenge_mode=0)
    check_batch(got, **args)
    return got, args


ONE = O.to_mont([1])[0]


def test_the_checker_refuses_a_changed_message_coefficient():
    got, args = control()
    for member in range(len(args["member_polys"])):  # the last round's top coefficient of every member in turn: each alone must be noticed
        polys = [[p.copy() for p in ps] for ps in args["member_polys"]]
        polys[member][-1][-1] = O.fr_add(polys[member][-1][-1].reshape(1, 4), ONE.reshape(1, 4))[0]
        with pytest.raises(AssertionError):
            check_batch(got, **{**args, "member_polys": polys})
    polys = [[p.copy() for p in ps] for ps in args["member_polys"]]
    polys[0][0][0] = O.fr_add(polys[0][0][0].reshape(1, 4), ONE.reshape(1, 4))[0]  # the first round's constant term
    with pytest.raises(AssertionError):
        check_batch(got, **{**args, "member_polys": polys})


def test_the_checker_refuses_a_changed_challenge():
    got, args = control()
    for rnd in (0, args["max_num_vars"] - 1):
        bad = {k: np.array(v, copy=True) for k, v in got.items()}
        bad["challenges"][rnd] = O.fr_add(bad["challenges"][rnd].reshape(1, 4), ONE.reshape(1, 4))[0]
        with pytest.raises(AssertionError):
            check_batch(bad, **args)


def test_the_checker_refuses_a_changed_batching_coefficient():
    got, args = control()
    coeffs = [c.copy() for c in args["coefficients"]]
    coeffs[1] = O.fr_add(coeffs[1].reshape(1, 4), ONE.reshape(1, 4))[0]
    with pytest.raises(AssertionError):
        check_batch(got, **{**args, "coefficients": coeffs})


def test_the_checker_refuses_a_window_that_does_not_end_with_the_batch():
    got, args = control()
    short = next(i for i, off in enumerate(args["offsets"]) if off > 0)
    offsets = list(args["offsets"])
    offsets[short] -= 1
    with pytest.raises(AssertionError, match="tail-aligned"):
        check_batch(got, **{**args, "offsets": offsets})


def test_the_checker_refuses_changed_end_claims():
    got, args = control()
    for key in ("member_claims", "final_claim"):
        bad = {k: np.array(v, copy=True) for k, v in got.items()}
        bad[key].reshape(-1, 4)[0] = O.fr_add(bad[key].reshape(-1, 4)[:1], ONE.reshape(1, 4))[0]
        with pytest.raises(AssertionError):
            check_batch(bad, **args)


def test_a_replay_transcript_runs_out():
    tr = ReplayTranscript(rand_fr(2, 5))
    tr.append(rand_fr(3, 6))
    assert np.array_equal(tr.challenge(), rand_fr(2, 5)[0]) and np.array_equal(tr.challenge(), rand_fr(2, 5)[1])
    with pytest.raises(IndexError):
        tr.challenge()
    assert tr.absorbed[0].shape == (3, 4)


def same(a, b, path=""):
    """util.same both ways round: the same keys on both sides, at every level"""
    util.same(a, b, path)
    util.same(b, a, path)


def test_every_twin_replayed_under_its_own_challenges_is_the_twin():
    """the replay paths of OracleExtended (a prescribed transcript / prescribed challenges) against its default paths (the oracle's own transcript, one-member prove_batch):
    the same messages, claims, final values, output claims and kept intermediates -- so what a GPU batch is checked against is what the operators driven alone are"""
    n_vars, label = 6, 17
    kw = dict(n_tables=6, log_k=4)
    orc = lambda: OracleExtended(n_vars, seed=29, **kw)
    for name in ("ram_read_write", "registers_read_write", "booleanity_address", "hamming_weight"):
        want = getattr(orc(), name)(label)
        tr = ReplayTranscript(want["challenges"])
        got = getattr(orc(), name)(label, transcript=tr)
        same(want, got, name)
        assert tr.drawn == len(want["polys"]) and np.array_equal(np.concatenate(tr.absorbed), np.concatenate(want["polys"])), name
    for name in ("spartan_outer", "spartan_product"):
        want = getattr(orc(), name)(label)
        same(want, getattr(orc(), name)(label, challenges=want["challenges"]), name)
    address = orc().booleanity_address(label)
    want = orc().booleanity_cycle(label, address["challenges"][::-1])
    same(want, orc().booleanity_cycle(label, address["challenges"][::-1], challenges=want["challenges"]), "booleanity_cycle")
    want = orc().instruction_read_raf(label)
    tr = ReplayTranscript(want["address_challenges"])
    same(want, orc().instruction_read_raf(label, transcript=tr, cycle_challenges=want["challenges"]), "instruction_read_raf")
    assert tr.drawn == 128
    want = orc().address_domain(label)
    replay = {label: want["bytecode_read_raf"]["address"]["challenges"], label + 1: want["bytecode_read_raf"]["cycle"]["challenges"],
              label + 10: want["ram_raf_evaluation"]["challenges"], label + 20: want["ram_output_check"]["challenges"]}
    same(want, orc().address_domain(label, replay=replay), "address_domain")
    same({"ram_output_check": want["ram_output_check"]}, orc().address_domain(label, replay=replay, only=["ram_output_check"]), "only")
