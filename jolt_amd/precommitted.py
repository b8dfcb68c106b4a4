"""The precommitted claim reductions over resident inputs: one constructor per kind, each returning the stage-6b cycle operator (ffi.StageOp).

The prepare side of crates/jolt-kernels/src/optimized/precommitted_reduction.rs composed from library entries: the tables are built on the device, permuted into
opening-round order when `perm_be` asks for it, and handed to jolt_stage_precommitted_cycle_create, which works on its own copies -- so everything built here is freed
before the constructor returns and the caller's tables stay as they were.

A `schedule` is the four round lists and totals, `Schedule(cycle_active, cycle_total, address_active, address_total)`; `perm_be[i]` is the opening round of big-endian
variable i.  Both are INPUTS (relation accessors in the reference: PrecommittedClaimReduction::cycle_phase_rounds / address_phase_rounds /
poly_opening_round_permutation_be); deriving them from the reduction's geometry is not done here."""
from collections import namedtuple

from . import ffi

Schedule = namedtuple("Schedule", "cycle_active cycle_total address_active address_total", defaults=((), 0))
RLC_GROUP = 40  # jolt_rlc combines at most this many tables in one call


def _cycle(ctx, value, eq, aux, schedule):
    s = Schedule(*schedule)
    return ctx.stage_precommitted_cycle(value, eq, aux, s.cycle_active, s.cycle_total, s.address_active, s.address_total)


def _permuted(ctx, tables, mapping, same):
    """-> (tables in opening-round order, the temporaries among them)"""
    if same:
        return list(tables), []
    out = [ctx.table_permute_bits(t, mapping) for t in tables]
    return out, list(out)


def _free(tables):
    for t in tables:
        t.free()


def advice(table, r_val, perm_be, schedule):
    """for_advice (:223-249): the advice polynomial against eq of the staged RAM value-check point; the eq table is built from the permuted challenges directly"""
    ctx = table.ctx
    mapping, same = ffi.host_precommitted_lsb_permutation(perm_be)
    eq = ctx.eq_evals(r_val if same else ffi.host_precommitted_permute_challenges(r_val, mapping))
    (value,), temps = _permuted(ctx, [table], mapping, same)
    try:
        return _cycle(ctx, value, eq, [], schedule)
    finally:
        _free(temps + [eq])


def program_image(words, r_addr_rw, start_index, perm_be, schedule):
    """for_program_image (:298-334): `words` = the padded word vector as resident u64 (ffi.Ints) against eq(r_addr_rw, start_index + .), the wrap included"""
    ctx = words.ctx
    mapping, same = ffi.host_precommitted_lsb_permutation(perm_be)
    raw = [ctx.table_from_ints(words), ctx.eq_evals_shifted(r_addr_rw, start_index, words.count)]
    (value, eq), temps = _permuted(ctx, raw, mapping, same)
    try:
        return _cycle(ctx, value, eq, [], schedule)
    finally:
        _free(temps + raw)


def _fold(ctx, chunks, weights):
    """sum_c w_c chunk_c: jolt_rlc, in groups when there are more chunks than one call takes"""
    w = ffi.fr(weights).reshape(-1, 4)
    if len(chunks) <= RLC_GROUP:
        return ctx.rlc(chunks, w)
    parts = [ctx.rlc(chunks[i:i + RLC_GROUP], w[i:i + RLC_GROUP]) for i in range(0, len(chunks), RLC_GROUP)]
    try:
        return ctx.rlc(parts, [ffi.host_fr_from_u64(1)] * len(parts))
    finally:
        _free(parts)


def bytecode(chunks, chunk_weights, lane_weights, r_bc, order, perm_be, schedule):
    """for_bytecode (:396-465): value = the chunk-weighted fold of the grids, eq = lane_weights x eq(r_bc) at index -> (lane, cycle) in the trace order
    (ffi.TRACE_CYCLE_MAJOR / TRACE_ADDRESS_MAJOR), the raw grids ride along as passengers: their bound coefficients are the per-chunk openings"""
    ctx = chunks[0].ctx
    mapping, same = ffi.host_precommitted_lsb_permutation(perm_be)
    eq_cycle = ctx.eq_evals(r_bc)
    raw = [_fold(ctx, chunks, chunk_weights), ctx.table_outer(lane_weights, eq_cycle, order)]
    tables, temps = _permuted(ctx, raw + list(chunks), mapping, same)
    try:
        return _cycle(ctx, tables[0], tables[1], tables[2:], schedule)
    finally:
        _free(temps + raw + [eq_cycle])


def address_phase(cycle_op):
    """the stage-7 operator from the carry of a finished cycle operator (the bound tables and the running scale move; a second call is refused)"""
    return cycle_op.ctx.stage_precommitted_address(cycle_op)


def advice_opening(table, point):
    """AdviceOpeningEvaluation::evaluate (:133-158): the advice polynomial at `point` (jolt_table_evaluate)"""
    return table.ctx.evaluate(table, point)
