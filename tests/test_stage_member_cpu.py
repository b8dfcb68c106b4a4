"""The member-backed stage operator and the grouped driver on the CPU (no device): the library exports jolt_stage_member_create and
jolt_host_prove_batch_ops_grouped and jolt_amd/ffi.py binds them; host-only operators (jolt_stage_host_expr_create: 2 to 5 members, degrees 1 to 4, unequal round counts in
tail-aligned windows, the four transcript engines, both challenge modes) through the grouped driver -- MemberGroupedRounds with no member to group: everything runs as under
SequentialRounds -- return the bytes jolt_host_prove_batch_ops returns, and both pass tests/stage_batch_replay.py check_batch over the oracle's members; the negative
controls return error statuses.  Device members through the same driver: tests/test_gpu_full_stage_batches.py."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from jolt_amd import ffi
from stage_batch_replay import check_batch, replay_member
from test_stage_batch_replay_cpu import ENGINES, oracle_members, random_batch, replayed

KEYS = ("polys", "challenges", "member_claims", "final_claim")
INVALID_ARG = 1


def test_the_library_exports_the_new_entry_points_and_ffi_binds_them():
    lib = ffi.lib()
    for name in ("jolt_stage_member_create", "jolt_host_prove_batch_ops_grouped"):
        assert hasattr(lib, name), name
    assert callable(ffi.Context.stage_member) and callable(ffi.Context.prove_batch_ops_grouped) and callable(ffi.prove_batch_ops_grouped)
    assert ffi.STAGE_MEMBER_OWN == 1


@pytest.mark.parametrize("challenge_mode", [0, 1])
@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5, 6])
def test_the_grouped_driver_returns_the_sequential_driver_s_bytes(seed, engine, challenge_mode):
    b = random_batch(seed, with_gruen=False)
    assert 2 <= len(b["descs"]) <= 5 and 1 <= min(d[2] for d in b["descs"]) and max(d[2] for d in b["descs"]) <= 4
    claims = [m.input_claim() for m in oracle_members(b)]
    label = engine | (70 + seed)
    args = (claims, b["coeffs"], b["offsets"], b["max_num_vars"], b["max_degree"])
    outs = []
    for driver in (ffi.prove_batch_ops, ffi.prove_batch_ops_grouped):
        ops = [ffi.stage_host_expr(*d) for d in b["descs"]]
        got = driver(ops, *args, label=label, challenge_mode=challenge_mode)
        check_batch(got, replayed(b, claims, got["challenges"]), claims, b["coeffs"], b["offsets"], b["rounds"], b["max_num_vars"], b["max_degree"], label, challenge_mode)
        for op, m, c, off in zip(ops, oracle_members(b), claims, b["offsets"]):
            assert np.array_equal(np.stack(op.output_claims()), replay_member(m, c, got["challenges"][off:])["final_values"])
            op.destroy()
        outs.append(got)
    for key in KEYS:
        assert np.array_equal(outs[0][key], outs[1][key]), key


def test_a_null_member_is_refused():
    h = C.c_void_p()
    for ctx in (None, C.c_void_p(0)):
        assert ffi.lib().jolt_stage_member_create(ctx, None, C.c_uint32(0), C.byref(h)) == INVALID_ARG
        assert not h.value
    assert ffi.lib().jolt_stage_member_create(None, None, C.c_uint32(ffi.STAGE_MEMBER_OWN), None) == INVALID_ARG


def fixed_batch():
    b = random_batch(3, with_gruen=False)
    return b, [ffi.stage_host_expr(*d) for d in b["descs"]], [m.input_claim() for m in oracle_members(b)]


def test_an_operator_window_out_of_range_is_refused():
    b, ops, claims = fixed_batch()
    short = next(i for i, off in enumerate(b["offsets"]) if off > 0)
    for bad in (b["offsets"][short] + 1, b["max_num_vars"] + 1):
        offsets = list(b["offsets"])
        offsets[short] = bad
        with pytest.raises(ffi.JoltError) as e:
            ffi.prove_batch_ops_grouped(ops, claims, b["coeffs"], offsets, b["max_num_vars"], b["max_degree"], label=9)
        assert e.value.status == INVALID_ARG
    # nothing ran: the same operators still prove the batch
    got = ffi.prove_batch_ops_grouped(ops, claims, b["coeffs"], b["offsets"], b["max_num_vars"], b["max_degree"], label=9)
    check_batch(got, replayed(b, claims, got["challenges"]), claims, b["coeffs"], b["offsets"], b["rounds"], b["max_num_vars"], b["max_degree"], 9)
    for op in ops:
        op.destroy()


def test_a_batch_that_lists_one_borrowed_operator_twice_is_refused():
    """Without a device the borrowed object is the operator itself: the grouped driver refuses it before any round runs (both entries would bind the same tables).  The same
    control over ONE device member behind two operators is in tests/test_gpu_full_stage_batches.py."""
    b, ops, claims = fixed_batch()
    full = [i for i, off in enumerate(b["offsets"]) if off == 0][0]
    twice, cl = [ops[full], ops[full]], [claims[full], claims[full]]
    with pytest.raises(ffi.JoltError) as e:
        ffi.prove_batch_ops_grouped(twice, cl, b["coeffs"][:2], [0, 0], b["max_num_vars"], b["max_degree"], label=9)
    assert e.value.status == INVALID_ARG
    got = ffi.prove_batch_ops_grouped(ops, claims, b["coeffs"], b["offsets"], b["max_num_vars"], b["max_degree"], label=9)
    want = O.prove_batch(oracle_members(b), claims, b["coeffs"], b["offsets"], b["max_num_vars"], b["max_degree"], label=9)
    for key in KEYS:
        assert np.array_equal(got[key], want[key]), key
    for op in ops:
        op.destroy()
