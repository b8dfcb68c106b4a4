"""Instruction read+RAF checking (stage 5) scans on the device through the C ABI: every phase's condensation, RAF
sums and per-table suffix accumulators (all 48 suffix kinds), the cycle-phase columns, and the cycle rounds through the split-eq
uniform member -- against oracle/read_raf.c (tests/test_oracle_read_raf.py pins that restatement to a big-integer model)."""
import functools

import numpy as np
import pytest

import oracle_lib as O
from jolt_amd import ffi
from read_raf_fixture import KINDS, make_rows, suffix_lists
from util import rand_challenge, rand_fr

pytestmark = pytest.mark.gpu
ADDRESS_BITS, PHASES = 128, 16


@pytest.fixture(scope="module")
def ctx():
    c = ffi.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("log_t,n_tables,canonical", [(12, 8, False), (9, 3, True), (0, 2, False)])
def test_all_sixteen_phases_match_oracle(ctx, log_t, n_tables, canonical):
    """the loop of OptimizedInstructionReadRafKernel::init_phase over the 16 phases: condense with the previous phase's eq table, then
    scan; the per-cycle mass u, the RAF sums and every (table, suffix) accumulator equal the oracle's after every phase"""
    T = 1 << log_t
    idx, table, raf = make_rows(T, n_tables, 50 + log_t)
    lists = suffix_lists(n_tables, 51)
    assert sorted({k for l in lists for k in l}) == list(range(len(KINDS)))  # every suffix kind is exercised
    rr = ctx.read_raf(idx, table, raf, n_tables)
    u_host = rand_fr(T, 52)
    u = ctx.upload(u_host)
    for phase in range(PHASES):
        suffix_len = ADDRESS_BITS - 8 * (phase + 1)
        if phase:
            v = rand_fr(256, 60 + phase)  # the bound-challenge eq table of the previous phase (any 256 field elements here)
            rr.condense(u, v, suffix_len + 8)
            u_host = O.read_raf_condense(idx, u_host, v, suffix_len + 8)
            assert np.array_equal(u.download(), u_host), phase
        got_raf, got_suf = rr.phase_scan(u, suffix_len, ADDRESS_BITS, lists, canonical=canonical)
        want_raf, want_suf = O.read_raf_phase_scan(idx, table, raf, n_tables, u_host, suffix_len, ADDRESS_BITS, lists, canonical=canonical)
        assert np.array_equal(got_raf, want_raf), phase
        for t in range(n_tables):
            base = sum(len(l) for l in lists[:t])
            for s, kind in enumerate(lists[t]):
                assert np.array_equal(got_suf[base + s], want_suf[base + s]), (phase, t, KINDS[kind])
    rr.free()


def test_skewed_rows_one_table_one_chunk(ctx):
    """every row in the same (table, chunk) bin -- one wavefront sums 2^11 rows -- and a table nobody uses"""
    T, n_tables = 1 << 11, 3
    rng = np.random.default_rng(70)
    idx = np.zeros((T, 2), dtype=np.uint64)
    idx[:, 0] = rng.integers(0, 2**48, size=T, dtype=np.uint64)
    idx[:, 1] = np.uint64(0xAB) << np.uint64(56)  # the top chunk of every row is 0xAB
    table = np.full(T, 1, dtype=np.uint8)
    raf = (rng.random(T) < 0.5).astype(np.uint8)
    lists = [[0, 1], [0, 5, 12, 23, 44], [3]]
    u_host = rand_fr(T, 71)
    rr = ctx.read_raf(idx, table, raf, n_tables)
    got_raf, got_suf = rr.phase_scan(ctx.upload(u_host), 120, ADDRESS_BITS, lists)
    want_raf, want_suf = O.read_raf_phase_scan(idx, table, raf, n_tables, u_host, 120, ADDRESS_BITS, lists)
    assert np.array_equal(got_raf, want_raf) and np.array_equal(got_suf, want_suf)
    assert not np.any(got_suf[0]) and not np.any(got_suf[7])  # tables 0 and 2 are absent
    rr.free()


def test_cycle_columns_and_cycle_rounds(ctx):
    """pending_combined_base / pending_ra_base for every cycle, then eq(r_reduction, j) * combined(j) * prod_i ra_i(j) over the log T
    cycle rounds through the eq-weighted product member, lock step with the oracle's dense member"""
    log_t, n_tables, ra_count = 9, 6, 4
    T = 1 << log_t
    idx, table, raf = make_rows(T, n_tables, 80)
    rr = ctx.read_raf(idx, table, raf, n_tables)
    tv, ri, rid = rand_fr(n_tables, 81), rand_fr(1, 82)[0], rand_fr(1, 83)[0]
    vt = rand_fr(PHASES * 256, 84).reshape(PHASES, 256, 4)
    combined, ra = rr.cycle_tables(tv, ri, rid, vt, ADDRESS_BITS, ra_count)
    want_combined, want_ra = O.read_raf_cycle_tables(idx, table, raf, tv, ri, rid, vt, ADDRESS_BITS, ra_count)
    assert np.array_equal(combined.download(), want_combined)
    for i in range(ra_count):
        assert np.array_equal(ra[i].download(), want_ra[i]), i
    r_reduction = rand_fr(log_t, 85)
    one = O.to_mont([1])[0]
    # one product group of 1 + ra_count linear factors with the eq weight factored out (degree 2 + ra_count = 6 round messages)
    member = ctx.member_lc([combined] + ra, [[(None, [(one, i)]) for i in range(1 + ra_count)]], 1 + ra_count, eq_point=r_reduction)
    orc = O.Member.expr([O.eq_evals(r_reduction), want_combined] + [want_ra[i] for i in range(ra_count)], [(one, list(range(2 + ra_count)))], 2 + ra_count)
    claim = orc.input_claim()
    bind = None
    for rnd in range(log_t):
        want = orc.prove_round(bind, claim)
        evals, aux = member.prove_round(bind, want_aux=True)
        assert np.array_equal(ffi.host_gruen_poly_from_q(aux[0], aux[1], evals, claim), want), rnd
        bind = rand_challenge(90 + rnd)
        claim = O.univariate_evaluate(want, bind)
    rr.free()


def test_argument_checks(ctx):
    idx, table, raf = make_rows(16, 2, 95)
    with pytest.raises(ffi.JoltError):
        ctx.read_raf(idx, np.full(16, 2, dtype=np.uint8), raf, 2)  # table index out of range
    rr = ctx.read_raf(idx, table, raf, 2)
    u = ctx.upload(rand_fr(16, 96))
    with pytest.raises(ffi.JoltError) as e:
        rr.phase_scan(u, 120, ADDRESS_BITS, [[0], [200]])  # unknown suffix kind
    assert e.value.status == 6  # JOLT_ERR_UNSUPPORTED
    with pytest.raises(ffi.JoltError):
        rr.phase_scan(u, 124, ADDRESS_BITS, [[0], [1]])  # the chunk above the suffix must fit the address
    with pytest.raises(ffi.JoltError) as e:
        rr.phase_scan(ctx.upload(rand_fr(8, 97)), 120, ADDRESS_BITS, [[0], [1]])
    assert e.value.status == 5
    rr.free()


@pytest.mark.parametrize("log_t,seed,canonical,all_tables", [(4, 12345, False, False), (3, 67890, True, False), (10, 31, False, True)])
def test_address_rounds_with_device_scans_match_the_definition(ctx, log_t, seed, canonical, all_tables):
    """The kernel end to end on its address side: device condensation + scans over the 42 REAL tables feed the host state machine (jolt_host_read_raf_address_*),
    and every one of the 128 round polynomials equals the oracle's from-the-definition round (oracle/lookup_tables.c).  Rows, reduction point, gamma and
    challenges are the reference kernel's own parity recipe (instruction_read_raf.rs:1477-1522, 1579-1646); the third case has every table present.  Then the
    cycle columns built from the state machine's table values equal the oracle's built from evaluate_mle at r_address, and the running claim is their sum."""
    from lookup_table_fixture import all_table_rows, challenge, fixture_rows
    idx, tab, raf = all_table_rows(log_t, seed) if all_tables else fixture_rows(log_t, seed)
    T = 1 << log_t
    lists = ffi.lookup_suffix_lists()
    r_reduction = O.to_mont([1000 + 37 * i for i in range(log_t)])
    u_host = O.eq_evals(r_reduction)
    gamma = O.to_mont([0xACE157EF])[0]
    challenges = O.to_mont([challenge(i) for i in range(128)])
    present = np.zeros(42, dtype=np.uint8)
    present[[int(t) for t in set(tab.tolist()) if t != 0xFF]] = 1
    rr = ctx.read_raf(idx, tab, raf, 42)
    u = ctx.upload(u_host)
    state = ffi.HostReadRafAddress(gamma, present, canonical)
    direct = O.ReadRafAddressDirect(idx, tab, raf, u_host, gamma, canonical=canonical)
    claim = O.read_raf_input_claim(idx, tab, raf, u_host, gamma, canonical=canonical)
    v_tables = []
    for phase in range(PHASES):
        suffix_len = ADDRESS_BITS - 8 * (phase + 1)
        if phase:
            rr.condense(u, v_tables[-1], suffix_len + 8)
        raf_sums, suffix_sums = rr.phase_scan(u, suffix_len, ADDRESS_BITS, lists, canonical=canonical)
        state.init_phase(phase, raf_sums, suffix_sums)
        if phase == 0:
            first = state.message()  # s(1) summed from the tables: s(0) + s(1) is the first-principles input claim
            assert np.array_equal(ffi.host_fr_add(first[0], first[1]), claim)
        for rnd in range(8):
            i = 8 * phase + rnd
            got = state.message(claim)
            assert np.array_equal(got, direct.round()), i
            coeffs = O.univariate_from_evals(got)
            claim = O.univariate_evaluate(coeffs, challenges[i])
            direct.bind(challenges[i])
            assert state.bind(challenges[i]) == (rnd == 7)
        v_tables.append(state.v_table(phase))
        assert np.array_equal(v_tables[-1], O.eq_evals(challenges[8 * phase: 8 * phase + 8]))
    table_values, raf_interleaved, raf_identity = state.finish()
    want_values, (left, right, identity, upper) = direct.values()
    used = np.flatnonzero(present)
    assert np.array_equal(table_values[used], want_values[used])
    g2 = O.fr_mul(gamma.reshape(1, 4), gamma.reshape(1, 4))
    assert np.array_equal(raf_interleaved, O.fr_add(O.fr_mul(gamma.reshape(1, 4), left.reshape(1, 4)), O.fr_mul(g2, right.reshape(1, 4)))[0])
    want_identity = O.fr_mul(g2, identity.reshape(1, 4))
    if canonical:
        want_identity = O.fr_add(want_identity, O.fr_mul(O.fr_mul(g2, gamma.reshape(1, 4)), upper.reshape(1, 4)))
    assert np.array_equal(raf_identity, want_identity[0])
    ra_count = 8 if log_t != 3 else 4
    vt = np.stack(v_tables)
    combined, ra = rr.cycle_tables(table_values, raf_interleaved, raf_identity, vt, ADDRESS_BITS, ra_count)
    want_combined, want_ra = O.read_raf_cycle_tables(idx, tab, raf, want_values, raf_interleaved, raf_identity, vt, ADDRESS_BITS, ra_count)
    assert np.array_equal(combined.download(), want_combined)
    orc = O.Member.expr([O.eq_evals(r_reduction), want_combined] + [want_ra[i] for i in range(ra_count)], [(O.to_mont([1])[0], list(range(2 + ra_count)))], 2 + ra_count)
    assert np.array_equal(orc.input_claim(), claim)  # what 128 address rounds leave is what the log T cycle rounds sum
    for i in range(ra_count):
        assert np.array_equal(ra[i].download(), want_ra[i])
        ra[i].free()
    combined.free()
    u.free()
    state.close()
    rr.free()


FIXED_CORNERS = 13  # the head of interesting_bits: zero, all ones, one operand zero / all ones, single bits, all but the top / the lowest bit


@functools.lru_cache(maxsize=None)
def corner_rows(n_tables, seed):
    """rows built from the suffix corner grid instead of make_rows: for each of the 16 phases the grid at that phase's suffix length (tests/corner_grids.py:
    zero, all ones, one operand zero / all ones, single high bits, runs of leading ones) with the phase's own 8-bit chunk above it -- 0x00, 0xFF, 0x80, 0x01 and random
    ones -- and zeros, ones or random bits above the chunk.  A row is accumulated under the suffix kinds of ITS table only, so the thirteen fixed corners of every
    grid stand once in EVERY table; the grid's other 240 suffixes draw a table (or none) and every row a RAF flag as in make_rows.  16 x (13 n_tables + 240) rows,
    padded to the next power of two with rows that have no table.  Returns idx, table, raf and, per row, (phase, suffix bits)."""
    from corner_grids import interesting_bits
    rng = np.random.default_rng(seed)
    rows, tables, meta = [], [], []
    for phase in range(PHASES):
        suffix_len = ADDRESS_BITS - 8 * (phase + 1)
        for i, bits in enumerate(interesting_bits(rng, suffix_len)):
            bits %= 1 << suffix_len  # (the grid's `full ^ 1` is 1 at length 0; the evaluators mask, a row must not spill into its chunk)
            for t in (range(n_tables) if i < FIXED_CORNERS else [0xFF if rng.random() < 0.1 else int(rng.integers(0, n_tables))]):
                j = len(rows)
                chunk = (0x00, 0xFF, 0x80, 0x01)[j % 8] if j % 8 < 4 else int(rng.integers(0, 256))
                above = (0, (1 << 128) - 1, int.from_bytes(rng.bytes(16), "little"))[j % 3]
                rows.append((((above >> (suffix_len + 8)) << 8 | chunk) << suffix_len | bits) & ((1 << 128) - 1))
                tables.append(t)
                meta.append((phase, bits))
    n = len(rows)
    T = 1 << n.bit_length()
    idx = np.zeros((T, 2), dtype=np.uint64)
    idx[:n, 0] = [r & (2**64 - 1) for r in rows]
    idx[:n, 1] = [r >> 64 for r in rows]
    table = np.full(T, 0xFF, dtype=np.uint8)
    table[:n] = tables
    raf = (rng.random(T) < 0.3).astype(np.uint8)
    return idx, table, raf, meta


def corner_rows_hold_their_classes(idx, table, meta, lists):
    """on the model alone: at every phase whose suffix has 8 bits or more, every 0/1-valued suffix kind takes BOTH values among the phase's own rows whose table lists
    that kind -- the rows under which the scan accumulates it -- but the kinds that are constant by definition (One; OverflowBitsZero while the suffix has no bit
    above 64); the four fixed chunk values stand above every phase's suffixes; and operands that are zero, all ones and a single bit reach every table"""
    from read_raf_fixture import ZERO_ONE, suffix_model, uninterleave
    for phase in range(PHASES):
        suffix_len = ADDRESS_BITS - 8 * (phase + 1)
        own = [(j, bits) for j, (p, bits) in enumerate(meta) if p == phase]
        chunks = {((int(idx[j, 0]) | int(idx[j, 1]) << 64) >> suffix_len) & 255 for j, _ in own}
        assert chunks >= {0x00, 0xFF, 0x80, 0x01}, phase
        assert all(((int(idx[j, 0]) | int(idx[j, 1]) << 64) % (1 << suffix_len)) == bits for j, bits in own), phase
        if suffix_len < 8:
            continue
        for t, kinds in enumerate(lists):
            mine = [bits for j, bits in own if table[j] == t]
            ops = [uninterleave(bits, suffix_len) for bits in mine]
            assert any(y == 0 and x != 0 for x, _, y, _ in ops) and any(x == 0 and y == (1 << yl) - 1 for x, _, y, yl in ops), (phase, t)  # y = 0 with x != 0; y all ones, x = 0
            assert any(y and y & (y - 1) == 0 for _, _, y, _ in ops), (phase, t)
            for kind in kinds:
                if KINDS[kind] not in ZERO_ONE or KINDS[kind] == "One" or (KINDS[kind] == "OverflowBitsZero" and suffix_len <= 64):
                    continue
                assert {suffix_model(kind, bits, suffix_len) for bits in mine} == {0, 1}, (phase, t, KINDS[kind])


@pytest.mark.parametrize("canonical", [False, True])
def test_all_sixteen_phases_match_oracle_on_the_suffix_corner_grid(ctx, canonical):
    """test_all_sixteen_phases_match_oracle over corner_rows: the scan kernels' own chunk_of / mask_low at the 64-bit boundaries (a chunk that straddles bit 64, a suffix
    of exactly 64 bits, of none) and the bit-count intrinsics inside suffix_mle meet zero, all-ones and single-bit operands, which random indices give them only
    where the suffix is a few bits long.  Condensation, the RAF sums and every (table, suffix) accumulator after every phase against the oracle."""
    n_tables = 3  # sixteen suffix kinds per table
    idx, table, raf, meta = corner_rows(n_tables, 130)  # one row set for both cases (built and checked once)
    T = idx.shape[0]
    assert len(meta) == 16 * (FIXED_CORNERS * n_tables + 240) and T == 8192 and (table[len(meta):] == 0xFF).all()
    lists = suffix_lists(n_tables, 131)
    assert sorted({k for l in lists for k in l}) == list(range(len(KINDS)))  # every suffix kind is listed
    if not canonical:
        corner_rows_hold_their_classes(idx, table, meta, lists)
    rr = ctx.read_raf(idx, table, raf, n_tables)
    u_host = rand_fr(T, 132)
    u = ctx.upload(u_host)
    for phase in range(PHASES):
        suffix_len = ADDRESS_BITS - 8 * (phase + 1)
        if phase:
            v = rand_fr(256, 140 + phase)
            rr.condense(u, v, suffix_len + 8)
            u_host = O.read_raf_condense(idx, u_host, v, suffix_len + 8)
            assert np.array_equal(u.download(), u_host), phase
        got_raf, got_suf = rr.phase_scan(u, suffix_len, ADDRESS_BITS, lists, canonical=canonical)
        want_raf, want_suf = O.read_raf_phase_scan(idx, table, raf, n_tables, u_host, suffix_len, ADDRESS_BITS, lists, canonical=canonical)
        assert np.array_equal(got_raf, want_raf), phase
        for t in range(n_tables):
            base = sum(len(l) for l in lists[:t])
            for s, kind in enumerate(lists[t]):
                assert np.array_equal(got_suf[base + s], want_suf[base + s]), (phase, t, KINDS[kind])
    rr.free()
