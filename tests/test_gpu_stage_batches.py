"""Device stage operators batched the way a stage driver batches them -- several jolt_stage_op objects on ONE context under ONE transcript, random batching
coefficients, different round counts and degrees in tail-aligned windows (jolt_host_prove_batch_ops; prove_batch, crates/jolt-sumcheck/src/prover.rs:193-362) --
against the CPU oracle: every member's oracle twin (tests/workload_oracle.py) is replayed under the challenges of its window and tests/stage_batch_replay.py
check_batch rebuilds the batch from the twins' messages, polynomial for polynomial and challenge for challenge.  The batches are the reference's stage membership
restricted to what exists as a stage operator.  Beside the transcript: every operator's output claims and kept intermediates are its twin's, a second batch over the
same resident inputs is the same bytes, and an operator of the batch driven alone on the same context afterwards still proves what its twin proves alone."""
import numpy as np
import pytest

from jolt_amd import ffi
from jolt_amd.stages import ADDRESS_BITS, CHUNK, PHASES, DeviceExtended, build_extended
from stage_batch_replay import ReplayTranscript, check_batch
from util import rand_fr, same
from workload_oracle import OracleExtended

pytestmark = pytest.mark.gpu

SEED = 733
SIZES = {6: dict(n_tables=6, log_k=4), 10: dict(n_tables=5, log_k=6, log_kb=5), 16: dict(log_k=14)}  # 2^16 x 2^14: many columns per merged group, many workgroups per scan


class Bed:
    """one context, the resident inputs of one description, and fresh oracle twins over the same description"""

    def __init__(self, n_vars):
        self.n_vars = n_vars
        self.d = build_extended(n_vars, SEED + n_vars, **SIZES[n_vars])
        self.ctx = ffi.Context(0)
        self.dev = DeviceExtended(self.ctx, n_vars, description=self.d)

    def orc(self):
        return OracleExtended(self.n_vars, description=self.d)

    def batch(self, make, coeffs, offsets, max_num_vars, max_degree, label, challenge_mode=0):
        """make() -> (operators, input claims, collect, release): one prove_batch_ops over fresh operators; collect() reads the operators' outputs after the batch"""
        ops, claims, collect, release = make()
        got = self.ctx.prove_batch_ops(ops, claims, coeffs, offsets, max_num_vars, max_degree, label=label, challenge_mode=challenge_mode)
        out = collect()
        release()
        return got, [np.array(c, copy=True) for c in claims], out

    def twice(self, *args, **kw):
        """the batch, and the same batch again over the same resident inputs: the same bytes"""
        first, again = self.batch(*args, **kw), self.batch(*args, **kw)
        same(first, again, "second batch")
        same(again, first, "second batch")
        return first

    def close(self):
        self.dev.close()
        self.ctx.close()


def check(got, twins, coeffs, offsets, rounds, max_num_vars, max_degree, label, challenge_mode=0):
    """twins: per member (replayed messages, the twin's input claim)"""
    check_batch(got, [t[0] for t in twins], [t[1] for t in twins], coeffs, offsets, rounds, max_num_vars, max_degree, label, challenge_mode)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# stage 2: RAM read / write (log T + log K rounds), the Spartan product remainder (log T), RAM RAF evaluation and the RAM output check (log K each)
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_vars,engine,challenge_mode", [(6, 0, 0), (10, 0, 0), (16, 0, 0), (10, ffi.TRANSCRIPT_BLAKE2B, 0), (10, 0, 1)])
def test_stage_2_batch(n_vars, engine, challenge_mode):
    bed = Bed(n_vars)
    dev, d = bed.dev, bed.d
    log_t, log_k = n_vars, d["ram"]["log_k"]
    total, label = log_t + log_k, engine | 81
    rounds = [total, log_t, log_k, log_k]
    offsets = [total - r for r in rounds]
    coeffs = list(rand_fr(4, 5 + n_vars))

    def make():
        index = dev.ram_index()
        given = {"ram_read_write": {}, "spartan_product": {}, "ram_raf_evaluation": dict(index=index), "ram_output_check": dict(index=index)}
        ops = [dev.operator(name, **kw) for name, kw in given.items()]
        assert [op.rounds for op in ops] == rounds
        claims = [dev.input_claim(name, op) for name, op in zip(given, ops)]

        def release():
            for op in ops:
                op.destroy()
            index.free()
        return ops, claims, lambda: [op.output_claims() for op in ops], release

    got, claims, outputs = bed.twice(make, coeffs, offsets, total, 3, label, challenge_mode)
    ch = got["challenges"]
    rw = bed.orc().ram_read_write(0, transcript=ReplayTranscript(ch))
    product = bed.orc().spartan_product(0, challenges=ch[offsets[1]:])
    adr = bed.orc().address_domain(0, replay={10: ch[log_t:], 20: ch[log_t:]}, only=["ram_raf_evaluation", "ram_output_check"])
    twins = [(rw["polys"], rw["claim"]), (product["polys"], product["claim"]), (adr["ram_raf_evaluation"]["polys"], adr["ram_raf_evaluation"]["claim"]),
             (adr["ram_output_check"]["polys"], adr["ram_output_check"]["claim"])]
    same(claims, [t[1] for t in twins], "input claims")
    check(got, twins, coeffs, offsets, rounds, total, 3, label, challenge_mode)
    same(outputs[0], rw["final_values"], "ram_read_write output claims")
    same(outputs[1], product["values"], "spartan_product output claims")
    same(outputs[2][0], adr["ram_raf_evaluation"]["ra_claim"], "ram_raf_evaluation output claim (the bound ra_folded; the bound unmap table follows it)")
    assert len(outputs[2]) == 2 and len(outputs[3]) == 1
    same(outputs[3][0], adr["ram_output_check"]["val_final_claim"], "ram_output_check output claim")
    # the context after the batch: the RAM read / write operator alone, as tests/test_gpu_extended.py drives it
    alone, want = dev.ram_read_write(300), bed.orc().ram_read_write(300)
    same(alone, want, "ram_read_write alone after the batch")
    assert np.array_equal(want["claim"], claims[0])
    bed.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# stages 4 / 7: registers read / write (log T + 7 rounds) and the Hamming-weight reduction (log K_chunk rounds, the last window of the batch)
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_vars", [6, 10, 16])
def test_stage_4_and_7_batch(n_vars):
    bed = Bed(n_vars)
    dev, d = bed.dev, bed.d
    bo, reg = d["booleanity"], d["registers"]
    total, label = n_vars + reg["log_k"], 82
    rounds = [total, bo["log_k"]]
    offsets = [0, total - bo["log_k"]]
    coeffs = list(rand_fr(2, 15 + n_vars))

    def make():
        names = ["registers_read_write", "hamming_weight"]
        ops = [dev.operator(name) for name in names]
        assert [op.rounds for op in ops] == rounds

        def release():
            for op in ops:
                op.destroy()
        return ops, [dev.input_claim(name, op) for name, op in zip(names, ops)], lambda: dict(registers=ops[0].output_claims(), g_claims=ops[1].output_claims(), masses=ops[1].kept("masses")), release

    got, claims, outputs = bed.twice(make, coeffs, offsets, total, 3, label)
    ch = got["challenges"]
    registers = bed.orc().registers_read_write(0, transcript=ReplayTranscript(ch))
    hamming = bed.orc().hamming_weight(0, transcript=ReplayTranscript(ch[offsets[1]:]))
    twins = [(registers["polys"], registers["claim"]), (hamming["polys"], hamming["claim"])]
    same(claims, [t[1] for t in twins], "input claims")
    check(got, twins, coeffs, offsets, rounds, total, 3, label)
    same(outputs["registers"][:5], registers["final_values"], "registers final values")
    same(outputs["registers"][5:7], registers["operand_claims"], "registers operand claims")
    assert len(outputs["registers"]) == 7
    same(outputs["g_claims"], hamming["g_claims"], "hamming_weight output claims")
    same(outputs["masses"].reshape(hamming["masses"].shape), hamming["masses"], "hamming_weight masses")
    same(dev.hamming_weight(470), bed.orc().hamming_weight(470), "hamming_weight alone after the batch")
    bed.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# stage 5: instruction read + RAF as ONE member of 128 + log T rounds beside the Spartan outer remainder (log T + 1 rounds); T <= 2^10, where the twin computes all
# 128 address rounds from the definition
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_vars", [6, 10])
def test_stage_5_batch(n_vars):
    assert n_vars <= OracleExtended.DIRECT_ADDRESS_ROUNDS_MAX_LOG_T
    bed = Bed(n_vars)
    dev, d = bed.dev, bed.d
    lk = d["lookup"]
    total, label = ADDRESS_BITS + n_vars, 83
    rounds = [total, n_vars + 1]
    offsets = [0, total - (n_vars + 1)]
    max_degree = d["ra_count"] + 2
    coeffs = list(rand_fr(2, 25 + n_vars))
    n_present = int(dev.lookup_present.sum())

    def make():
        names = ["instruction_read_raf", "spartan_outer"]
        ops = [dev.operator(name) for name in names]
        assert [op.rounds for op in ops] == rounds and ops[0].degree == max_degree

        def collect():
            op, claims = ops[0], ops[0].output_claims()
            raf_scans, suf_scans = op.kept("scan_raf").reshape(PHASES, 6, CHUNK, 4), op.kept("scan_suffix").reshape(PHASES, -1, CHUNK, 4)
            return dict(lookup=dict(lookup_table_flags=claims[:n_present], instruction_raf_flag=claims[n_present], instruction_ra=claims[n_present + 1:],
                                    scans=[(raf_scans[ph], suf_scans[ph]) for ph in range(PHASES)], v_tables=op.kept("v_tables").reshape(PHASES, CHUNK, 4),
                                    table_values=op.kept("table_values")[lk["present"]], raf_values=op.kept("raf_values"), cycle_claim=op.kept("cycle_claim")[0]),
                        outer=ops[1].output_claims())

        def release():
            for op in ops:
                op.destroy()
        return ops, [dev.input_claim(name, op) for name, op in zip(names, ops)], collect, release

    got, claims, outputs = bed.twice(make, coeffs, offsets, total, max_degree, label)
    ch = got["challenges"]
    orc = bed.orc()
    lookup = orc.instruction_read_raf(0, transcript=ReplayTranscript(ch[:ADDRESS_BITS]), cycle_challenges=ch[ADDRESS_BITS:])
    assert orc.direct_checked == list(range(ADDRESS_BITS))
    outer = bed.orc().spartan_outer(0, challenges=ch[offsets[1]:])
    twins = [(list(lookup["address_polys"]) + list(lookup["polys"]), lookup["claim"]), (outer["polys"], outer["claim"])]
    same(claims, [t[1] for t in twins], "input claims")
    check(got, twins, coeffs, offsets, rounds, total, max_degree, label)
    same(outputs["lookup"], lookup, "instruction_read_raf outputs")
    same(outputs["outer"], outer["values"], "spartan_outer output claims")
    alone = dev.spartan(dev.outer_ints, d["outer_iwa"], d["outer_iwb"], d["outer_wa"], d["outer_wb"], d["outer_tau"], d["outer_kernel"], dev.claims["outer"], 2, 100)
    same(alone, bed.orc().spartan_outer(100), "spartan_outer alone after the batch")
    bed.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# stage 6a: bytecode read + RAF, address phase (log K_bytecode rounds) and booleanity, address phase (log K_chunk rounds, a later window);
# stage 6b: their cycle phases (log T rounds each), created from what 6a left: the bound address operator, the booleanity window's challenges and its intermediate claim
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def stage_6(n_vars, with_cycle):
    bed = Bed(n_vars)
    ctx, dev, d = bed.ctx, bed.dev, bed.d
    bc, bo = d["bytecode"], d["booleanity"]
    log_kb, log_kc = bc["log_k"], bo["log_k"]
    n_chunks = (log_kb + bc["chunk_bits"] - 1) // bc["chunk_bits"]
    rounds_a, offsets_a = [log_kb, log_kc], [0, log_kb - log_kc]
    rounds_b, offsets_b, degree_b = [n_vars, n_vars], [0, 0], max(3, 1 + n_chunks)
    coeffs_a, coeffs_b = list(rand_fr(2, 35 + n_vars)), list(rand_fr(2, 45 + n_vars))
    label_a, label_b = 84, 85
    n_cols = bo["cols"].shape[0]

    def chain():
        """6a, then (with_cycle) 6b over what 6a left"""
        pc_index = dev.pc_index()
        a_ops = [dev.operator("bytecode_read_raf_address", index=pc_index), dev.operator("booleanity_address")]
        assert [op.rounds for op in a_ops] == rounds_a
        claims_a = [dev.input_claim("bytecode_read_raf_address", a_ops[0]), dev.input_claim("booleanity_address", a_ops[1])]
        got_a = ctx.prove_batch_ops(a_ops, claims_a, coeffs_a, offsets_a, log_kb, 3, label=label_a)
        fin = a_ops[0].output_claims()
        out = dict(a=got_a, claims_a=claims_a, fin=fin, intermediate=a_ops[1].output_claims()[0], masses=a_ops[1].kept("masses").reshape(n_cols, 1 << log_kc, 4))
        if with_cycle:
            r_address = got_a["challenges"][offsets_a[1]:][::-1]
            b_ops = [dev.operator("bytecode_read_raf_cycle", address=a_ops[0]), dev.operator("booleanity_cycle", r_address=r_address)]
            assert [op.rounds for op in b_ops] == rounds_b and max(op.degree for op in b_ops) == degree_b
            claims_b = [dev.input_claim("bytecode_read_raf_cycle", b_ops[0]), dev.input_claim("booleanity_cycle", b_ops[1], out["intermediate"])]
            got_b = ctx.prove_batch_ops(b_ops, claims_b, coeffs_b, offsets_b, n_vars, degree_b, label=label_b)
            out.update(b=got_b, claims_b=claims_b, ra_claims=b_ops[0].output_claims(), bool_ra_claims=b_ops[1].output_claims(), eq_scalar=b_ops[1].kept("eq_scalar")[0])
            for op in b_ops:
                op.destroy()
        for op in a_ops:
            op.destroy()
        pc_index.free()
        return out

    out, again = chain(), chain()
    same(out, again, "second batch")
    ch_a = out["a"]["challenges"]
    replay = {0: ch_a}
    if with_cycle:
        replay[1] = out["b"]["challenges"]
    bytecode = bed.orc().address_domain(0, replay=replay, only=["bytecode_read_raf"])["bytecode_read_raf"]
    address = bed.orc().booleanity_address(0, transcript=ReplayTranscript(ch_a[offsets_a[1]:]))
    twins = [(bytecode["address"]["polys"], bytecode["claim_address"]), (address["polys"], address["claim"])]
    same(out["claims_a"], [t[1] for t in twins], "6a input claims")
    check(out["a"], twins, coeffs_a, offsets_a, rounds_a, log_kb, 3, label_a)
    assert len(out["fin"]) == 14
    same(out["fin"][13], bytecode["intermediate"], "bytecode intermediate claim")
    same(out["fin"][5:10], bytecode["val_stages"], "bytecode stage values")
    same(out["intermediate"], address["intermediate"], "booleanity intermediate claim")
    same(out["masses"], address["masses"], "booleanity masses")
    r_address = ch_a[offsets_a[1]:][::-1]
    if with_cycle:
        cycle = bed.orc().booleanity_cycle(0, r_address, challenges=out["b"]["challenges"])
        twins = [(bytecode["cycle"]["polys"], bytecode["claim_cycle"]), (cycle["polys"], cycle["claim"])]
        same(out["claims_b"], [t[1] for t in twins], "6b input claims")
        check(out["b"], twins, coeffs_b, offsets_b, rounds_b, n_vars, degree_b, label_b)
        same(out["ra_claims"], bytecode["ra_claims"], "bytecode ra claims")
        same(out["bool_ra_claims"], cycle["ra_claims"], "booleanity ra claims")
        same(out["eq_scalar"], cycle["eq_scalar"], "booleanity eq scalar")
        same(dev.booleanity_cycle(460, r_address, out["intermediate"]), bed.orc().booleanity_cycle(460, r_address), "booleanity_cycle alone after the batch")
    else:
        same(dev.booleanity_address(450), bed.orc().booleanity_address(450), "booleanity_address alone after the batch")
    bed.close()


@pytest.mark.parametrize("n_vars", [6, 10, 16])
def test_stage_6a_batch(n_vars):
    stage_6(n_vars, with_cycle=False)


@pytest.mark.parametrize("n_vars", [6, 10, 16])
def test_stage_6b_batch(n_vars):
    stage_6(n_vars, with_cycle=True)


def test_the_alone_driver_checks_what_the_operator_does_not():
    """jolt_host_stage_op_prove_alone checks s(0) + s(1) against the running claim every round, as prove_batch does.  Booleanity's address phase samples all four points of
    its message and never reads the claim, so under a claim that is not its sum (zero) nothing in the operator objects: the DRIVER must report JOLT_ERR_ROUND_CHECK.  A
    fresh operator under the right claim then proves what the twin proves."""
    bed = Bed(6)
    op = bed.dev.operator("booleanity_address")
    tr = ffi.HostTranscript(450)
    with pytest.raises(ffi.JoltError) as e:
        op.prove_alone(tr, ffi.host_fr_from_u64(1))
    assert e.value.status == 8  # JOLT_ERR_ROUND_CHECK
    tr.close()
    op.destroy()
    same(bed.dev.booleanity_address(450), bed.orc().booleanity_address(450), "booleanity_address after the refusal")
    bed.close()
