"""Whole protocol stages as ONE batched sumcheck on ONE context under ONE transcript (DeviceWorkload.prove_stage_batches): the reference's stage memberships
(crates/jolt-verifier/src/stages/stage{2,3,4,5,6a,6b,7}/outputs.rs) with the stage operators (jolt_stage_*_create) AND the catalogue's relations (device members wrapped
by jolt_stage_member_create) in the same prove_batch (crates/jolt-sumcheck/src/prover.rs:193-362), through jolt_host_prove_batch_ops_grouped -- against the CPU oracle.

How a batch is checked (tests/stage_batch_replay.py): every window ends with its batch (instance_point_offset, crates/jolt-verifier/src/stages/relations.rs:202-213 and
stage2/mod.rs:25-49), so every relation's oracle twin replayed under challenges[offset:] sends what the relation must send.  A catalogue relation's twin is the O.Member
OracleWorkload.member builds (the naive flat-Expr member over dense tables), replayed with replay_member; an operator's twin is the OracleExtended method under prescribed
challenges.  check_batch rebuilds the batch from the twins' messages, compares every coefficient of every round polynomial and draws every challenge itself.  Nothing on
the checking side comes from the library under test except `got` -- with the one exception the suite already has: above T = 2^16 the read-RAF twin takes 111 of its 128
address-round polynomials from the library's HOST state machine fed with the oracle's scan sums and verifies them from the definition at 17 rounds and at the ends
(OracleExtended.instruction_read_raf); at T <= 2^16 all 128 are from the definition.

Beside check_batch: input claims are the twins'; every operator's output claims are its twin's values and a wrapped member's are the twin's final values (in the device
member's table order, the bound eq scalar last); a second batch over the same resident inputs is the same bytes; and afterwards DeviceWorkload.prove() on the same object
still equals OracleWorkload.prove() (the operators only borrowed the members).  The comparison of the grouped driver with jolt_host_prove_batch_ops is a RACE CHECK of
the scheduler (one launch set per round against one launch per member), device against device: it is not the parity claim -- check_batch is.

Status: written without a GPU at hand; no figure of this file has been observed on a device yet (the oracle side -- every twin, window, round count and degree -- was
dry-run on the CPU under random challenges)."""
import os

import numpy as np
import pytest

import oracle_lib as O
from jolt_amd import ffi
from jolt_amd import workload as W
from jolt_amd.stages import ADDRESS_BITS, N_LOOKUP_TABLES
from jolt_amd.workload import DeviceWorkload
from stage_batch_replay import ReplayTranscript, check_batch, replay_member
from util import same
from workload_oracle import OracleExtended, OracleWorkload

pytestmark = pytest.mark.gpu

SEED, LABEL, PROVE_LABEL = 4100, 900, 700
KEYS = ("polys", "challenges", "member_claims", "final_claim")
ORDER = (2, 3, 4, 5, "6a", "6b", 7)


class EveryRoundDirect(OracleExtended):  # all 128 read-RAF address rounds from the definition up to T = 2^16 (tests/test_gpu_extended.py does the same at that size)
    DIRECT_ADDRESS_ROUNDS_MAX_LOG_T = 16


class Bed:
    """one context, one DeviceWorkload with both descriptions resident (extended=True), and the oracle's side of the same descriptions"""

    def __init__(self, n_vars, only_stages=None):
        O.baseline_set_threads(min(16, os.cpu_count() or 1))
        self.n_vars, seed = n_vars, SEED + n_vars
        self.ctx = ffi.Context(0)
        self.wl = DeviceWorkload(self.ctx, n_vars, seed=seed, extended=True)
        self.d = self.wl.ext.d  # the description (numpy): what OracleExtended is built over
        self.ow = OracleWorkload(n_vars, seed=seed, only_stages=only_stages)
        self.by_name = {ms.name: i for i, ms in enumerate(self.ow.members_spec)}
        names = [n for key in ORDER for n in DeviceWorkload.STAGE_BATCHES[key]]
        self.coeffs = dict(zip(names, W.rand_fr(len(names), np.random.default_rng(seed + 5))))  # random field elements, one per relation
        self.want_prove = None

    def orc(self):
        return EveryRoundDirect(self.n_vars, description=self.d)

    def catalogue_twin(self, name, challenges):
        """-> (messages, input claim, final values in the device member's table order)"""
        i = self.by_name[name]
        ms, m = self.ow.members_spec[i], self.ow.member(i)
        claim = m.input_claim()
        out = replay_member(m, claim, challenges)
        fv = out["final_values"]
        if ms.uniform is not None or ms.eq_inner is not None:  # the eq weight is factored out on the device: its bound scalar comes last
            fv = np.concatenate([fv[1:], fv[:1]])
        elif ms.fused is not None:  # linear-leaf fusion: the device binds A = sum_i s_i leaf_i as one table
            parts, names, _ = ms.fused
            fused = {}
            for fname, entries in parts:
                acc = np.zeros((1, 4), dtype=np.uint64)
                for c, ti in entries:
                    acc = O.fr_add(acc, O.fr_mul(np.asarray(self.ow.res.coeff(c)).reshape(1, 4), fv[ti].reshape(1, 4)))
                fused[fname] = acc[0]
            fv = np.stack([fused[t] if t in fused else fv[ms.tables.index(t)] for t in names])
        m.close()
        return out["polys"], claim, fv

    def close(self):
        self.wl.close()
        self.ctx.close()


BEDS = {}


def bed_for(n_vars):
    """one bed at a time: the cases below are ordered by size"""
    if n_vars not in BEDS:
        for bed in BEDS.values():
            bed.close()
        BEDS.clear()
        BEDS[n_vars] = Bed(n_vars, only_stages={4, 5} if n_vars >= 20 else None)
    return BEDS[n_vars]


@pytest.fixture(scope="module", autouse=True)
def _close_beds():
    yield
    for bed in BEDS.values():
        bed.close()
    BEDS.clear()


def twins_for(bed, key, got, all_got):
    """-> [(name, messages, input claim, expected output claims or None, how many leading output claims to compare)], max_degree"""
    d, n = bed.d, bed.n_vars
    ch = np.asarray(got["challenges"])
    cat = lambda name, window: (name,) + bed.catalogue_twin(name, window)
    if key == 2:
        log_k = d["ram"]["log_k"]
        rw = bed.orc().ram_read_write(0, transcript=ReplayTranscript(ch))
        product = bed.orc().spartan_product(0, challenges=ch[log_k:])
        adr = bed.orc().address_domain(0, replay={10: ch[n:], 20: ch[n:]}, only=["ram_raf_evaluation", "ram_output_check"])
        raf, oc = adr["ram_raf_evaluation"], adr["ram_output_check"]
        return [("ram_read_write", rw["polys"], rw["claim"], rw["final_values"]), ("spartan_product", product["polys"], product["claim"], product["values"]),
                cat("instruction_claim_reduction", ch[log_k:]), ("ram_raf_evaluation", raf["polys"], raf["claim"], [raf["ra_claim"]]),
                ("ram_output_check", oc["polys"], oc["claim"], [oc["val_final_claim"]])], 3
    if key == 3:
        return [cat(name, ch) for name in DeviceWorkload.STAGE_BATCHES[3]], 3
    if key == 4:
        reg = bed.orc().registers_read_write(0, transcript=ReplayTranscript(ch))
        return [("registers_read_write", reg["polys"], reg["claim"], list(reg["final_values"]) + list(reg["operand_claims"])), cat("ram_val_check", ch[d["registers"]["log_k"]:])], 3
    if key == 5:
        orc = bed.orc()
        lk = orc.instruction_read_raf(0, transcript=ReplayTranscript(ch[:ADDRESS_BITS]), cycle_challenges=ch[ADDRESS_BITS:])
        assert orc.direct_checked == sorted(OracleExtended.sampled_direct_rounds(n) if n > 16 else range(ADDRESS_BITS))
        claims = list(lk["lookup_table_flags"]) + [lk["instruction_raf_flag"]] + list(lk["instruction_ra"])
        return [("instruction_read_raf", list(lk["address_polys"]) + list(lk["polys"]), lk["claim"], claims), cat("ram_ra_claim_reduction", ch[ADDRESS_BITS:]),
                cat("registers_val_evaluation", ch[ADDRESS_BITS:])], d["ra_count"] + 2
    if key in ("6a", "6b"):
        a, b = all_got["6a"], all_got["6b"]
        ch_a, ch_b = np.asarray(a["challenges"]), np.asarray(b["challenges"])
        log_kb, log_kc = d["bytecode"]["log_k"], d["booleanity"]["log_k"]
        total_a = max(log_kb, log_kc)
        bytecode = bed.orc().address_domain(0, replay={0: ch_a[total_a - log_kb:], 1: ch_b}, only=["bytecode_read_raf"])["bytecode_read_raf"]
        r_address = ch_a[total_a - log_kc:][::-1]
        if key == "6a":
            address = bed.orc().booleanity_address(0, transcript=ReplayTranscript(ch_a[total_a - log_kc:]))
            fin = [None] * 5 + list(bytecode["val_stages"]) + [None] * 3 + [bytecode["intermediate"]]
            return [("bytecode_read_raf_address", bytecode["address"]["polys"], bytecode["claim_address"], fin), ("booleanity_address", address["polys"], address["claim"], [address["intermediate"]])], 3
        cycle = bed.orc().booleanity_cycle(0, r_address, challenges=ch_b)
        assert np.array_equal(b["eq_scalar"], cycle["eq_scalar"]), "booleanity eq scalar"
        n_chunks = (log_kb + d["bytecode"]["chunk_bits"] - 1) // d["bytecode"]["chunk_bits"]
        return [("bytecode_read_raf_cycle", bytecode["cycle"]["polys"], bytecode["claim_cycle"], list(bytecode["ra_claims"])),
                ("booleanity_cycle", cycle["polys"], cycle["claim"], list(cycle["ra_claims"]))] + [cat(name, ch_b) for name in DeviceWorkload.STAGE_BATCHES["6b"][2:]], max(3, 1 + n_chunks, 5)
    if key == 7:
        hamming = bed.orc().hamming_weight(0, transcript=ReplayTranscript(ch))
        return [("hamming_weight", hamming["polys"], hamming["claim"], list(hamming["g_claims"]))], 2
    raise ValueError(key)


def run_case(n_vars, stage, engine=0, challenge_mode=0):
    bed = bed_for(n_vars)
    wl, base = bed.wl, engine | LABEL
    got = wl.prove_stage_batches(base, stages=(stage,), challenge_mode=challenge_mode)
    again = wl.prove_stage_batches(base, stages=(stage,), challenge_mode=challenge_mode)
    same(got, again, "a second batch over the same resident inputs")
    same(again, got, "a second batch over the same resident inputs")
    # RACE CHECK, not the parity claim (device against device): one launch set per round must give what one launch per member gives
    sequential = wl.prove_stage_batches(base, stages=(stage,), challenge_mode=challenge_mode, grouped=False)
    same(got, sequential, "grouped against sequential rounds (race check)")
    keys = ("6a", "6b") if stage == 6 else (stage,)
    assert tuple(got) == keys
    for key in keys:
        g = got[key]
        twins, max_degree = twins_for(bed, key, g, got)
        names = [t[0] for t in twins]
        assert tuple(names) == DeviceWorkload.STAGE_BATCHES[key] and g["names"] == names
        rounds = [len(t[1]) for t in twins]
        total = max(rounds)
        offsets = [total - r for r in rounds]  # instance_point_offset: every window of these stages ends with the batch
        coeffs = [bed.coeffs[name] for name in names]
        label = base + DeviceWorkload.STAGE_BATCH_LABELS[key]
        assert g["rounds"] == rounds and g["offsets"] == offsets and g["max_num_vars"] == total and g["max_degree"] == max_degree, (key, g["rounds"], rounds, g["max_degree"], max_degree)
        same(g["coefficients"], coeffs, f"stage {key} batching coefficients")
        same(g["input_claims"], [t[2] for t in twins], f"stage {key} input claims")
        check_batch({k: g[k] for k in KEYS}, [t[1] for t in twins], [t[2] for t in twins], coeffs, offsets, rounds, total, max_degree, label, challenge_mode)
        for (name, _, _, want), out in zip(twins, g["output_claims"]):
            if name == "ram_raf_evaluation":  # (the bound unmap table follows the bound ra_folded)
                assert len(out) == 2
                out = out[:1]
            assert len(out) == len(want), (key, name, len(out), len(want))
            for k, (x, y) in enumerate(zip(out, want)):
                if y is not None:  # (bytecode address: the twin reports the stage values and the intermediate claim of the 14)
                    assert np.array_equal(x, y), f"stage {key}, {name}: output claim {k}"
    # the borrowed members after the batches: the catalogue's own proof is still the oracle's
    if bed.want_prove is None:
        bed.want_prove = bed.ow.prove(label=PROVE_LABEL)
    after = wl.prove(label=PROVE_LABEL)
    for st, want in bed.want_prove.items():
        for k in ("polys", "challenges", "final_claim"):
            assert np.array_equal(after[st][k], want[k]), f"DeviceWorkload.prove() after the stage {stage} batch: stage {st} {k}"


STAGES = [2, 3, 4, 5, 6, 7]


@pytest.mark.parametrize("n_vars,stage", [(n_vars, stage) for n_vars in (6, 10, 16) for stage in STAGES])
def test_full_stage_batch(n_vars, stage):
    run_case(n_vars, stage)


@pytest.mark.parametrize("stage", STAGES)
def test_full_stage_batch_under_the_reference_transcript(stage):
    run_case(10, stage, engine=ffi.TRANSCRIPT_BLAKE2B)


@pytest.mark.parametrize("stage", STAGES)
def test_full_stage_batch_with_full_width_challenges(stage):
    run_case(10, stage, challenge_mode=1)


@pytest.mark.parametrize("stage", [4, 5])
def test_full_stage_batch_at_trace_scale(stage):
    """T = 2^20 under LegacyBlake2bTranscript: registers read / write beside the RAM value check, instruction read + RAF beside the two stage-5 reductions"""
    run_case(20, stage, engine=ffi.TRANSCRIPT_BLAKE2B)


def test_one_member_cannot_be_two_operators_of_a_batch_nor_cross_contexts():
    bed = bed_for(6)
    ctx, wl = bed.ctx, bed.wl
    i = wl.stages[3][0]
    m = wl.members[i]
    ops = [ctx.stage_member(m), ctx.stage_member(m)]
    n = wl.n_vars
    for prove in (ctx.prove_batch_ops_grouped, ctx.prove_batch_ops):
        with pytest.raises(ffi.JoltError) as e:
            prove(ops, [wl.claims[i]] * 2, [bed.coeffs["spartan_shift"]] * 2, [0, 0], n, ops[0].degree, label=5)
        assert e.value.status == 1  # JOLT_ERR_INVALID_ARG, before any round ran
    for op in ops:
        op.destroy()
    other = ffi.Context(0)
    with pytest.raises(ffi.JoltError) as e:
        other.stage_member(m)
    assert e.value.status == 1
    other.close()
    m.reset()
    after = wl.prove(label=PROVE_LABEL)
    if bed.want_prove is None:
        bed.want_prove = bed.ow.prove(label=PROVE_LABEL)
    for st, want in bed.want_prove.items():
        assert np.array_equal(after[st]["polys"], want["polys"]), st
