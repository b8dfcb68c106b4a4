"""The precommitted claim reductions on the device against the definition (tests/precommitted_model.py, Python integers): the operator pair over resident tables --
the fused bind + sums kernel, its sums-only and bind-only variants, the passenger batching -- the table builders, and the three constructors of
jolt_amd/precommitted.py end to end from raw inputs.  Bit for bit throughout."""
import numpy as np
import pytest

import oracle_lib as O
import precommitted_model as M
from jolt_amd import ffi, precommitted as P
from precommitted_model import SCHEDULES, schedule
from util import rand_challenge, rand_fr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = ffi.Context(0)
    yield c
    c.close()


def same_message(got, want, where):
    assert got.shape[0] == len(want), f"{where}: {got.shape[0]} coefficients, the definition has {len(want)}"
    assert M.ints(got) == want, where


def host_tables(n, n_aux, seed):
    t = [rand_fr(1 << n, 1000 * seed + k) for k in range(2 + n_aux)]
    return t, [M.ints(x) for x in t]


def challenges(count, seed):
    """the reference's 125-bit challenge shape in the even rounds (the kernels' short multiply), full-width elements in the odd ones"""
    return [rand_challenge(seed + k, shifted=(k % 2 == 0)) for k in range(count)]


def drive(op, phase, claim, seed, where, also=None):
    """device operator, model phase (and optionally the host operator) round by round under the same challenges -> the claim after the last round"""
    ch = challenges(phase.num_rounds(), seed)
    assert op.rounds == phase.num_rounds() and op.degree == 2
    bind = None
    for rnd in range(phase.num_rounds()):
        b = None if bind is None else M.limbs([bind])[0]
        got = op.prove_round(b, rnd, M.limbs([claim])[0])
        want = phase.prove_round(bind, rnd, claim)
        same_message(got, want, f"{where}, round {rnd}")
        if also is not None:
            assert np.array_equal(also.prove_round(b, rnd, M.limbs([claim])[0]), got), f"{where}, round {rnd}: device against host operator"
        bind = M.ints(ch[rnd])[0]
        claim = M.evaluate(want, bind)
    op.finish_rounds(M.limbs([bind])[0])
    phase.finish_rounds(bind)
    if also is not None:
        also.finish_rounds(M.limbs([bind])[0])
    return claim


def run_reduction(ctx, n, n_aux, kind, seed, with_host=False):
    ca, ct, aa, at = schedule(kind, n)
    t, ti = host_tables(n, n_aux, seed)
    dev = [ctx.upload(x) for x in t]
    red = M.Reduction(ti[0], ti[1], ti[2:], ca, ct, aa, at)
    op = ctx.stage_precommitted_cycle(dev[0], dev[1], dev[2:], ca, ct, aa, at)
    host = ffi.stage_host_precommitted(t[0], t[1], t[2:], ca, ct, aa, at) if with_host else None
    claim = red.input_claim()
    assert M.ints(op.input_claim()) == [claim]
    claim = drive(op, red.cycle, claim, 10 * seed, f"{kind} cycle", host)
    assert M.ints(op.output_claims()) == red.cycle.output_claims()
    if aa:
        adr = ctx.stage_precommitted_address(op)
        assert M.ints(op.output_claims()) == [claim] and M.ints(adr.input_claim()) == [claim]
        phase = red.address()
        host_adr = ffi.stage_host_precommitted_address(host) if with_host else None
        claim = drive(adr, phase, claim, 10 * seed + 5, f"{kind} address", host_adr)
        assert M.ints(adr.output_claims()) == phase.output_claims() and len(adr.output_claims()) == 1 + n_aux
        if with_host:
            assert np.array_equal(adr.output_claims(), host_adr.output_claims())
        adr.destroy()
    else:
        assert len(op.output_claims()) == 1 + n_aux
    # the operator worked on its own copies
    for d, x in zip(dev, t):
        assert np.array_equal(d.download(), x)
    op.destroy()
    return claim


@pytest.mark.parametrize("kind", SCHEDULES)
@pytest.mark.parametrize("n", [1, 2, 7, 11])
def test_device_operator_is_the_definition(ctx, n, kind):
    """L = 2 and 4: one work item, with and without sums; 2^7: half a wavefront of pairs; 2^11: more than one workgroup"""
    run_reduction(ctx, n, 1, kind, seed=n, with_host=(n <= 7))


@pytest.mark.parametrize("n,n_aux", [(11, 0), (11, 1), (11, 5), (4, 65)])
def test_passenger_batching(ctx, n, n_aux):
    run_reduction(ctx, n, n_aux, "two_phase", seed=40 + n_aux)
    run_reduction(ctx, n, n_aux, "middle", seed=50 + n_aux)


def test_grid_rounds_then_tail_rounds(ctx):
    """L = 2^17 with two passengers: 2^16 pairs in round 0, above tail_pairs = 16384, down to one"""
    run_reduction(ctx, 17, 2, "middle", seed=3)


def test_a_second_run_gives_equal_bytes(ctx):
    n, n_aux = 12, 3
    ca, ct, aa, at = schedule("two_phase", n)
    t, _ = host_tables(n, n_aux, 9)
    dev = [ctx.upload(x) for x in t]
    runs = []
    for _ in range(2):
        op = ctx.stage_precommitted_cycle(dev[0], dev[1], dev[2:], ca, ct, aa, at)
        a = op.prove_alone(ffi.HostTranscript(11), op.input_claim())
        adr = ctx.stage_precommitted_address(op)
        b = adr.prove_alone(ffi.HostTranscript(12), a["final_claim"])
        runs.append(np.concatenate(a["polys"] + b["polys"] + [a["challenges"], b["challenges"], adr.output_claims()]))
    assert np.array_equal(runs[0], runs[1])


@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("kind", ["head", "two_phase"])
def test_offset_zero_member_of_a_padded_batch_beside_a_device_member(ctx, kind, grouped):
    n, n_aux = 9, 2
    ca, ct, aa, at = schedule(kind, n)
    t, ti = host_tables(n, n_aux, 13)
    max_num_vars = ct + 3
    dense_rounds = ct + 1
    dt = [rand_fr(1 << dense_rounds, 600 + k) for k in range(3)]
    terms = [(rand_fr(1, 610)[0], [0, 1, 2]), (rand_fr(1, 611)[0], [2])]
    red = M.Reduction(ti[0], ti[1], ti[2:], ca, ct, aa, at)
    members = [red.cycle, M.OracleExpr(dt, terms, 3)]
    claims = [red.input_claim(), members[1].input_claim()]
    coeffs = M.ints(rand_fr(2, 620))
    offsets = [0, max_num_vars - dense_rounds]
    want = M.prove_batch(members, claims, coeffs, offsets, max_num_vars, 3, label=33)
    dev = [ctx.upload(x) for x in t]
    member = ctx.member_expr([ctx.upload(x) for x in dt], terms, 3)
    ops = [ctx.stage_precommitted_cycle(dev[0], dev[1], dev[2:], ca, ct, aa, at), ctx.stage_member(member)]
    fn = ctx.prove_batch_ops_grouped if grouped else ctx.prove_batch_ops
    got = fn(ops, list(M.limbs(claims)), list(M.limbs(coeffs)), offsets, max_num_vars, 3, label=33)
    for rnd in range(max_num_vars):
        assert M.ints(got["polys"][rnd]) == want["polys"][rnd], f"round {rnd}"
    assert M.ints(got["challenges"]) == want["challenges"]
    assert M.ints(got["member_claims"]) == want["member_claims"] and M.ints(got["final_claim"]) == [want["final_claim"]]
    assert M.ints(ops[0].output_claims()) == red.cycle.output_claims()
    for o in ops:
        o.destroy()
    member.destroy()


def test_device_refusals(ctx):
    v, e, a, short = ctx.upload(rand_fr(8, 1)), ctx.upload(rand_fr(8, 2)), ctx.upload(rand_fr(8, 3)), ctx.upload(rand_fr(4, 4))
    for args, status in (((v, e, [short], [0, 1, 2], 3), 5), ((v, short, [], [0, 1, 2], 3), 5), ((v, e, [a], [0, 1], 3), 5), ((v, e, [a], [0, 2, 1], 3), 1),
                         ((v, e, [a], [0, 1, 3], 3), 1)):
        with pytest.raises(ffi.JoltError) as err:
            ctx.stage_precommitted_cycle(*args)
        assert err.value.status == status, args[3:]
    six = ctx.upload(rand_fr(6, 5))
    with pytest.raises(ffi.JoltError) as err:
        ctx.stage_precommitted_cycle(six, six, [], [0, 1, 2], 3)
    assert err.value.status == 1
    op = ctx.stage_precommitted_cycle(v, e, [a], [0, 1], 2, [0], 1)
    with pytest.raises(ffi.JoltError, match="stage 6b parked no"):  # not finished
        ctx.stage_precommitted_address(op)
    op.prove_alone(ffi.HostTranscript(1), op.input_claim())
    adr = ctx.stage_precommitted_address(op)
    with pytest.raises(ffi.JoltError, match="stage 6b parked no"):  # reclaimed
        ctx.stage_precommitted_address(op)
    with pytest.raises(ffi.JoltError) as err:
        adr.output_claims()
    assert err.value.status == 7
    host = ffi.stage_host_precommitted(rand_fr(2, 1), rand_fr(2, 2), [], [], 1, [0], 1)
    host.prove_alone(ffi.HostTranscript(1), host.input_claim())
    with pytest.raises(ffi.JoltError):  # a host operator's carry does not live on the device
        ctx.stage_precommitted_address(host)


# ---- the builders -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 4, 12])
def test_table_permute_bits(ctx, n):
    t = rand_fr(1 << n, 70 + n)
    rng = np.random.default_rng(n)
    for perm_be in ([int(x) for x in rng.permutation(n)], list(range(n)), list(range(n))[::-1]):
        m, _ = M.lsb_permutation(perm_be)
        src = ctx.upload(t)
        got = ctx.table_permute_bits(src, m).download()
        want = M.permute_coefficients(list(range(1 << n)), m)  # the index map, applied to the rows here
        assert np.array_equal(got, t[want])
        assert np.array_equal(src.download(), t)
    with pytest.raises(ffi.JoltError):
        ctx.table_permute_bits(ctx.upload(t), [0] * n if n > 1 else [1])
    with pytest.raises(ffi.JoltError) as err:
        ctx.table_permute_bits(ctx.upload(t), list(range(n + 1)))
    assert err.value.status == 5


def test_eq_evals_shifted(ctx):
    r = rand_fr(4, 91)
    full = M.eq_table(M.ints(r))
    assert M.limbs(full).tolist() == O.eq_evals(r).tolist()  # the model's eq table is the oracle's
    for start, length in [(0, 16), (3, 8), (13, 8), (5, 2), (15, 4), (6, 1)]:  # the reference's own list
        got = ctx.eq_evals_shifted(r, start, length)
        assert len(got) == length and M.ints(got.download()) == M.shifted_eq(M.ints(r), start, length), (start, length)
    r = rand_fr(12, 92)
    full = O.eq_evals(r)
    for start, length in [(4000, 256), (4095, 2), (1, 4095), (2048, 2048), (3000, 4096)]:  # wrapped tails, an odd start, a whole turn from the middle
        got = ctx.eq_evals_shifted(r, start, length).download()
        assert np.array_equal(got, full[(start + np.arange(length)) % 4096]), (start, length)
    for start, length in [(0, 0), (0, 4097)]:
        with pytest.raises(ffi.JoltError):
            ctx.eq_evals_shifted(r, start, length)


@pytest.mark.parametrize("lanes", [8, 512])
@pytest.mark.parametrize("order", [ffi.TRACE_CYCLE_MAJOR, ffi.TRACE_ADDRESS_MAJOR])
def test_table_outer(ctx, order, lanes):
    w, r = rand_fr(lanes, 5), rand_fr(3, 6)
    cyc = ctx.eq_evals(r)
    got = ctx.table_outer(w, cyc, order)
    assert len(got) == lanes * 8
    assert M.ints(got.download()) == M.outer(M.ints(w), M.eq_table(M.ints(r)), order)
    with pytest.raises(ffi.JoltError):
        ctx.table_outer(w, cyc, 2)


# ---- the constructors, end to end from raw inputs -----------------------------------------------------------------------------------------------------------
def finish_against(cycle_op, red, seed, n_aux):
    claim = red.input_claim()
    assert M.ints(cycle_op.input_claim()) == [claim]
    claim = drive(cycle_op, red.cycle, claim, seed, "cycle")
    assert M.ints(cycle_op.output_claims()) == red.cycle.output_claims()
    adr = P.address_phase(cycle_op)
    phase = red.address()
    drive(adr, phase, claim, seed + 50, "address")
    assert M.ints(adr.output_claims()) == phase.output_claims() and len(adr.output_claims()) == 1 + n_aux


def perm_and_schedule(n, seed):
    perm_be = [7 + 2 * int(x) for x in np.random.default_rng(seed).permutation(n)]
    return perm_be, P.Schedule(*schedule("two_phase", n))


@pytest.mark.parametrize("identity", [False, True])
def test_advice_constructor(ctx, identity):
    n = 6
    perm_be, sched = perm_and_schedule(n, 1)
    if identity:
        perm_be = list(range(n))[::-1]
    table, r_val = rand_fr(1 << n, 3), rand_fr(n, 4)
    value, eq = M.advice_tables(M.ints(table), M.ints(r_val), perm_be)
    dev = ctx.upload(table)
    finish_against(P.advice(dev, r_val, perm_be, sched), M.Reduction(value, eq, [], *sched), 200, 0)
    assert np.array_equal(dev.download(), table)


def test_program_image_constructor(ctx):
    n, ram_vars, start = 5, 8, 250  # the 32-word block wraps past the top of the 256-word RAM domain
    perm_be, sched = perm_and_schedule(n, 2)
    rng = np.random.default_rng(8)
    words = rng.integers(0, 2**64, size=1 << n, dtype=np.uint64)
    words[20:] = 0  # the padding
    r = rand_fr(ram_vars, 9)
    value, eq = M.program_image_tables([int(w) for w in words], M.ints(r), start, perm_be)
    finish_against(P.program_image(ffi.Ints(ctx, words), r, start, perm_be, sched), M.Reduction(value, eq, [], *sched), 300, 0)


@pytest.mark.parametrize("order", [ffi.TRACE_CYCLE_MAJOR, ffi.TRACE_ADDRESS_MAJOR])
@pytest.mark.parametrize("n_chunks", [3, 43])
def test_bytecode_constructor(ctx, n_chunks, order):
    lanes, cycle_vars = 8, 3  # 43 chunks: the value fold takes two jolt_rlc groups
    n = 3 + cycle_vars
    perm_be, sched = perm_and_schedule(n, 3)
    chunks = [rand_fr(1 << n, 400 + c) for c in range(n_chunks)]
    cw, lw, r_bc = rand_fr(n_chunks, 5), rand_fr(lanes, 6), rand_fr(cycle_vars, 7)
    value, eq, aux = M.bytecode_tables([M.ints(c) for c in chunks], M.ints(cw), M.ints(lw), M.ints(r_bc), order, perm_be)
    dev = [ctx.upload(c) for c in chunks]
    finish_against(P.bytecode(dev, cw, lw, r_bc, order, perm_be, sched), M.Reduction(value, eq, aux, *sched), 500, n_chunks)
    assert np.array_equal(dev[-1].download(), chunks[-1])


def test_advice_opening(ctx):
    table, point = rand_fr(1 << 7, 21), rand_fr(7, 22)
    want = np.zeros((1, 4), dtype=np.uint64)
    for row in O.fr_mul(table, O.eq_evals(point)):
        want = O.fr_add(want, row.reshape(1, 4))
    assert np.array_equal(P.advice_opening(ctx.upload(table), point), want[0])
