"""The Spartan uni-skip round from constraint rows on the device: t1 off the rows (jolt_r1cs_uniskip_sums_rows), and the whole stage on one transcript
(jolt_host_prove_spartan_stage) -- against tests/uniskip_twin.py: the oracle's restatement of the reference's loop, Python big integers, the oracle's transcript and hashlib."""
import functools

import numpy as np
import pytest

import oracle_lib as O
import uniskip_twin as TW
from jolt_amd import ffi
from jolt_amd import stages as S
from test_uniskip_rows_cpu import extreme_cycles, extreme_system
from util import rand_challenge

pytestmark = pytest.mark.gpu
R = O.R_MOD
SHAPES = {(2, 10): dict(second=None, zero_on_domain=True), (1, 3): dict(second=None, zero_on_domain=False), (2, 2): dict(second=1, zero_on_domain=True)}


@pytest.fixture(scope="module")
def ctx():
    c = ffi.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def system_of(shape):
    return S.random_row_system(*shape, second_stream_rows=SHAPES[shape]["second"])


@functools.lru_cache(maxsize=None)
def block_of(shape, log_t, broken):
    return S.satisfied_rows_block({}, log_t, 0, system=system_of(shape), broken_cycle=(1 << log_t) // 3 if broken else None)


def tau_of(shape, log_t, seed=40):
    return np.stack([rand_challenge(seed + 7 * k + log_t) for k in range(log_t + shape[0])])  # log T cycle coordinates, the stream's, tau_high


def rows_of(shape):
    system = system_of(shape)
    return ffi.R1csRows(system["streams"], system["domain_size"], system["n_inputs"], SHAPES[shape]["zero_on_domain"])


def upload(ctx, block):
    return [ctx.ints(c) for c in block["cols"]]


@functools.lru_cache(maxsize=None)
def twin_t1(shape, log_t, broken):
    system, block = system_of(shape), block_of(shape, log_t, broken)
    tau_low = tau_of(shape, log_t)[:-1]
    eq = O.eq_evals(tau_low) if len(tau_low) else O.to_mont([1])
    zod = SHAPES[shape]["zero_on_domain"]
    if shape[0] == 2:
        return TW.ints(TW.t1_oracle(system, TW.promote(block["ints"]), eq, zod))
    return TW.t1_bigint(system, block["ints"], eq, zod)


@pytest.mark.parametrize("broken", [False, True], ids=["satisfied", "unsatisfied"])
@pytest.mark.parametrize("log_t", [0, 1, 7, 8, 9, 12])  # one cycle; under a block; exactly one; two blocks (with padded idle workgroups); several slices
@pytest.mark.parametrize("shape", list(SHAPES), ids=lambda s: f"S{s[0]}D{s[1]}")
def test_sums_off_the_rows_match_the_twin(ctx, shape, log_t, broken):
    block = block_of(shape, log_t, broken)
    rows, cols = rows_of(shape), upload(ctx, block)
    tau_low = tau_of(shape, log_t)[:-1]
    eq = ctx.eq_evals(tau_low) if len(tau_low) else ctx.upload(O.to_mont([1]))
    got = TW.ints(ctx.r1cs_uniskip_sums_rows(rows, cols, eq))
    assert got == twin_t1(shape, log_t, broken)
    if SHAPES[shape]["zero_on_domain"]:
        D = shape[1]
        inside = [p for p in range(2 * D - 1) if p not in TW.evaluated_nodes(D, True)]
        assert len(inside) == D and all(got[p] == 0 for p in inside)
    elif not broken:  # a satisfied witness: t1 vanishes on the domain although every node was evaluated
        D = shape[1]
        assert all(got[p] == 0 for p in range(2 * D - 1) if p not in TW.evaluated_nodes(D, True)) and any(got)
    eq.free()
    for c in cols:
        c.free()
    rows.destroy()


def test_extreme_column_values_and_the_2_pow_64_constant(ctx):
    system = extreme_system()
    log_t = 9
    ints = extreme_cycles(system, 1 << log_t, 11)
    rows = ffi.R1csRows(system["streams"], 4, system["n_inputs"], False)
    cols = [ctx.ints(S._int_column(v, k)) for v, k in zip(ints, system["kinds"])]
    tau_low = np.stack([rand_challenge(60 + k) for k in range(log_t + 1)])
    eq = ctx.eq_evals(tau_low)
    assert TW.ints(ctx.r1cs_uniskip_sums_rows(rows, cols, eq)) == TW.t1_bigint(system, ints, O.eq_evals(tau_low), zero_on_domain=False)
    eq.free()
    for c in cols:
        c.free()


def test_a_lane_that_takes_more_than_one_cycle(ctx):
    """T = 2^19: the launch code caps the grid at 4 workgroups per compute unit (256 x 4 x 256 = 2^18 lanes), so a lane takes two cycles.  The trace is a 2^6-cycle block
    repeated 2^13 times; since sum_k eq(tau_hi, k) = 1, t1 of the repeated trace is t1 of the block against eq over the LAST 6 cycle coordinates and the stream's --
    which the twin computes at the small size."""
    shape, log_t, log_b = (2, 10), 19, 6
    system, block = system_of(shape), block_of(shape, log_b, True)
    rows = rows_of(shape)
    cols = [ctx.ints(np.tile(c, (1 << (log_t - log_b),) + (1,) * (c.ndim - 1))) for c in block["cols"]]
    tau_low = np.stack([rand_challenge(90 + k) for k in range(log_t + 1)])
    eq = ctx.eq_evals(tau_low)
    want = TW.ints(TW.t1_oracle(system, TW.promote(block["ints"]), O.eq_evals(tau_low[log_t - log_b:]), True))
    assert TW.ints(ctx.r1cs_uniskip_sums_rows(rows, cols, eq)) == want and any(want)
    eq.free()
    for c in cols:
        c.free()


def test_rows_against_the_column_form(ctx):
    """device against device -- a cross-check, not parity: on a system whose folded weights have an int64 the row kernel and k_small_uniskip agree"""
    system = S.random_row_system(2, 10, seed=5, foldable=True)
    block = S.satisfied_rows_block({}, 9, 0, system=system, broken_cycle=17)
    h = ffi.R1csRows(system["streams"], 10, system["n_inputs"], True)
    wa, wb = h.fold_small()
    cols = upload(ctx, block)
    tau_low = np.stack([rand_challenge(120 + k) for k in range(10)])
    eq = ctx.eq_evals(tau_low)
    by_rows = ctx.r1cs_uniskip_sums_rows(h, cols, eq)
    by_cols = ctx.r1cs_uniskip_sums_small(cols, eq, wa, wb, streams=2)
    assert np.array_equal(by_rows[TW.evaluated_nodes(10, True)], by_cols) and by_cols.any()
    eq.free()
    for c in cols:
        c.free()


STAGE_CASES = [((2, 10), 0, 11), ((2, 10), 3, 12), ((2, 10), 10, 13), ((2, 10), 10, ffi.TRANSCRIPT_BLAKE2B | 14),
               ((1, 3), 0, 15), ((1, 3), 3, 16), ((1, 3), 10, 17), ((1, 3), 10, ffi.TRANSCRIPT_BLAKE2B | 18)]


@pytest.mark.parametrize("shape,log_t,label", STAGE_CASES, ids=[f"S{s[0]}D{s[1]}-T{t}-{'blake2b' if l >> 62 else 'test'}" for s, t, l in STAGE_CASES])
def test_whole_stage_on_one_transcript(ctx, shape, log_t, label):
    system, block = system_of(shape), block_of(shape, log_t, False)
    rows, cols = rows_of(shape), upload(ctx, block)
    tau = tau_of(shape, log_t, seed=70)
    zero = np.zeros(4, dtype=np.uint64)
    one = O.to_mont([1])[0]

    def prove():
        tr = ffi.HostTranscript(label)
        out = ctx.prove_spartan_stage(rows, cols, tau, zero, one, tr)
        out["state"], out["next"] = tr.state(), tr.challenge()
        tr.close()
        return out

    got = prove()
    # the twin proves the stage on a transcript of its own (the oracle's for the stand-in engine, hashlib for LegacyBlake2bTranscript) and draws every challenge itself:
    # the uni-skip round, then the remainder's compressed rounds
    vtr = TW.HashlibBlake2bTranscript(b"jolt-amd/%d" % (label & ((1 << 62) - 1))) if label >> 62 else O.MockTranscript(label)
    want = TW.stage(system, block["ints"], tau, 0, vtr, zero_on_domain=SHAPES[shape]["zero_on_domain"])
    assert np.array_equal(got["uniskip_coeffs"], want["uniskip_coeffs"])
    assert np.array_equal(got["r0"], want["r0"]) and np.array_equal(got["uniskip_claim"], want["uniskip_claim"])
    n = tau.shape[0] - 1
    assert got["polys"].shape[0] == n == len(want["polys"])
    for rnd in range(n):
        assert np.array_equal(got["polys"][rnd], want["polys"][rnd]), f"round {rnd}"
    assert np.array_equal(got["challenges"], want["challenges"]) and np.array_equal(got["final_claim"], want["final_claim"])
    assert np.array_equal(got["values"], want["values"])
    assert got["state"] == vtr.state() and np.array_equal(got["next"], vtr.challenge())
    if n:
        # the same messages by replay under the device's challenges, and the remainder's input claim IS the uni-skip output claim
        rep = TW.stage(system, block["ints"], tau, 0, O.MockTranscript(label) if not label >> 62 else TW.HashlibBlake2bTranscript(b"jolt-amd/%d" % (label & ((1 << 62) - 1))),
                       challenges=got["challenges"], zero_on_domain=SHAPES[shape]["zero_on_domain"])
        assert all(np.array_equal(a, b) for a, b in zip(rep["polys"], got["polys"])) and np.array_equal(rep["remainder_input_claim"], got["uniskip_claim"])
    again = prove()
    for key in got:
        assert np.array_equal(np.asarray(got[key]), np.asarray(again[key])) if not isinstance(got[key], bytes) else got[key] == again[key], key
    for c in cols:
        c.free()
    rows.destroy()


def test_device_method_runs_the_stage(ctx):
    """DeviceExtended.spartan_stage is the stage under a transcript label (the method needs only the context and the library of its object)"""
    shape, log_t = (2, 10), 3
    block, rows = block_of(shape, log_t, False), rows_of(shape)
    cols = upload(ctx, block)
    dev = S.DeviceExtended.__new__(S.DeviceExtended)
    dev.ffi, dev._home_ctx, dev._tls, dev.one = ffi, ctx, type("T", (), {})(), O.to_mont([1])[0]
    tau = tau_of(shape, log_t, seed=70)
    got = dev.spartan_stage(rows, cols, tau, np.zeros(4, dtype=np.uint64), 12)
    tr = ffi.HostTranscript(12)
    want = ctx.prove_spartan_stage(rows, cols, tau, np.zeros(4, dtype=np.uint64), dev.one, tr)
    tr.close()
    assert all(np.array_equal(got[k], want[k]) for k in want)
    assert "spartan_stage" not in S.DeviceExtended.OPERATORS
    for c in cols:
        c.free()


@pytest.mark.parametrize("shape", [(2, 10), (1, 3)], ids=lambda s: f"S{s[0]}D{s[1]}")
def test_an_unsatisfied_witness_is_a_round_check_failure(ctx, shape):
    """One broken cycle.  A system that is taken to vanish on the domain ((2, 10)) passes the uni-skip round -- its first-round polynomial is interpolated through zeros
    there -- and fails the REMAINDER's first round: the uni-skip output claim is not the sum of the remainder.  A system whose domain nodes are evaluated ((1, 3)) already
    fails the centred-domain check of the uni-skip round.  Either way JOLT_ERR_ROUND_CHECK, nothing stays allocated, and the context proves correctly afterwards."""
    log_t = 6
    system = system_of(shape)
    rows = rows_of(shape)
    tau = tau_of(shape, log_t, seed=150)
    zero, one = np.zeros(4, dtype=np.uint64), O.to_mont([1])[0]
    good, bad = upload(ctx, block_of(shape, log_t, False)), upload(ctx, block_of(shape, log_t, True))
    ctx.synchronize()
    tr = ffi.HostTranscript(21)
    ctx.prove_spartan_stage(rows, good, tau, zero, one, tr)  # (warms the context's pools: what is live afterwards is the baseline)
    tr.close()
    before = ctx.memory_stats()["live_bytes"]
    tr = ffi.HostTranscript(21)
    with pytest.raises(ffi.JoltError) as e:
        ctx.prove_spartan_stage(rows, bad, tau, zero, one, tr)
    tr.close()
    assert e.value.status == 8  # JOLT_ERR_ROUND_CHECK
    assert ctx.memory_stats()["live_bytes"] == before  # the operator, its tables and the row tables were released
    tr = ffi.HostTranscript(21)
    got = ctx.prove_spartan_stage(rows, good, tau, zero, one, tr)
    tr.close()
    want = TW.stage(system, block_of(shape, log_t, False)["ints"], tau, 0, O.MockTranscript(21), zero_on_domain=SHAPES[shape]["zero_on_domain"])
    assert np.array_equal(got["challenges"], want["challenges"]) and np.array_equal(got["final_claim"], want["final_claim"]) and np.array_equal(got["values"], want["values"])
    for c in good + bad:
        c.free()
    rows.destroy()
