"""GPU: the corner grids of the host forms on the DEVICE build (device_probe.hip, jolt_probe_*): one launch runs one lane per operand tuple through the function the
kernels call, and every result is held, bit for bit,
  (a) to the independent reference the CPU test of the same grid uses -- the oracle's field arithmetic, Python integers, the big-integer models of tests/g2_model.py,
      tests/pairing_model.py, tests/read_raf_fixture.py, the exact model of the limb-form addition in tests/corner_grids.py: the parity claim; and
  (b) to the host form of the same op on the same operands: the two builds of one source agree, which says where a failure of (a) comes from.
The x86 build is not the gfx950 build where such code goes wrong: `mul` is another algorithm per target, the limb-form multiply-accumulate is inline assembly on the
device only, the suffixes' bit counts are intrinsics there, carry chains and funnel shifts go through another backend.

Every test first asserts, on the reference alone, that its grid holds the classes it is there for; runs the whole grid and its first 63, 64, 65 and 100 tuples (one
lane short of a wavefront, a whole one, one over, a size that is no multiple of the 64-lane workgroup: the probe's own tail guard); and ends with the comparer's
negative control: one flipped bit in one result must be found, at its tuple."""
import numpy as np
import pytest

import g2_model as M
import oracle_lib as O
import pairing_model as PM
from corner_grids import (MASK, P0, Q, R, RL, add_paths_false_positive_cases, add_paths_random_cases, add_paths_special_cases, dory_fr_scalars, field_grid, fq12_grid,
                          fq2_grid, g2_grid, interesting_bits, limb_form_grid, limbs, limbs64, model_common, oracle_inv, saturated_operands, shifted_challenge_grid, small_scalar_columns, value)
from jolt_amd import ffi
from read_raf_fixture import KINDS, ZERO_ONE, leading_ones, suffix_model, uninterleave

pytestmark = pytest.mark.gpu
SIZES = (63, 64, 65, 100)
MIN_TUPLES = 130  # a grid with fewer tuples is repeated up to here, so that the prefixes above and more than two workgroups exist


@pytest.fixture(scope="module")
def ctx():
    c = ffi.Context(0)
    yield c
    c.close()


def tile(a, n=MIN_TUPLES):
    """the rows of `a`, repeated in order until there are at least n"""
    a = np.asarray(a)
    return a if a.shape[0] >= n else np.resize(a, (n,) + a.shape[1:])


def differing(got, want):
    """the tuples at which two result arrays differ in any bit"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    return np.flatnonzero((got != want).reshape(got.shape[0], -1).any(axis=1)).tolist()


def hold(name, launch, operands, want, host):
    """launch(*operands cut to n tuples) for the whole grid and the prefixes: equal to the reference `want` and to the host form's `host`; then the negative control"""
    assert differing(host, want) == [], (name, "the host form misses the reference")
    total = want.shape[0]
    assert total >= MIN_TUPLES
    for n in (total,) + SIZES:
        got = launch(*[None if o is None else o[:n] for o in operands])
        assert differing(got, want[:n]) == [], (name, n, "device result differs from the reference at these tuples")
        assert differing(got, host[:n]) == [], (name, n, "device build differs from the host build of the same source")
    flipped = got.copy()
    flat = flipped.reshape(flipped.shape[0], -1)
    flat[n - 1, flat.shape[1] - 1] ^= flat.dtype.type(1 << 7)
    assert differing(flipped, want[:n]) == [n - 1], (name, "the comparer did not see a flipped bit")


# ------------------------------------------------------------------------------------------------------ Fr / Fq
@pytest.mark.parametrize("field", [0, 1], ids=["fr", "fq"])
def test_field_ops_on_the_device_match_the_oracle_and_the_host_form(ctx, field):
    mod = (R, Q)[field]
    omul, oadd, osub = ((O.fr_mul, O.fr_add, O.fr_sub), (O.fq_mul, O.fq_add, O.fq_sub))[field]
    ints, vals, pairs = field_grid(field)
    # the grid: 0, 1, p - 1, p - 2, the all-ones patterns, and the saturated operands against themselves and each other
    sat = [ints.index(s) for s in saturated_operands(mod)]
    assert all(v in ints for v in (0, 1, mod - 1, mod - 2, (1 << 232) - 1, (1 << 253) - 1))
    assert all((s, t) in pairs for s in sat for t in sat) and (ints.index(mod - 1), ints.index(mod - 1)) in pairs and (0, 0) in pairs
    nine = lambda v: [(v >> (29 * k)) & 0x1FFFFFFF for k in range(9)]
    assert nine(ints[sat[0]])[:8] == [0x1FFFFFFF] * 8  # (and no larger top limb stays below p: saturated_operands)
    assert sum(l == 0x1FFFFFFF for l in nine(((1 << 253) - 1) << 5)) == 7  # as the second operand (taken << 5) this one saturates limbs 1 .. 7
    a, b = vals[[i for i, _ in pairs]], vals[[j for _, j in pairs]]
    a_int, zero = [ints[i] for i, _ in pairs], np.zeros_like(a)
    assert any(x < y for (x, y) in zip(a_int, [ints[j] for _, j in pairs])) and any(x + y >= mod for (x, y) in zip(a_int, [ints[j] for _, j in pairs]))  # sub borrows, add wraps
    want = {ffi.PROBE_MUL: omul(a, b), ffi.PROBE_SQR: omul(a, a), ffi.PROBE_ADD: oadd(a, b), ffi.PROBE_SUB: osub(a, b), ffi.PROBE_NEG: osub(zero, a),
            ffi.PROBE_DBL: oadd(a, a),
            ffi.PROBE_FROM_MONT: limbs64([x * pow(1 << 256, -1, mod) % mod for x in a_int]), ffi.PROBE_TO_MONT: limbs64([x * (1 << 256) % mod for x in a_int])}
    assert np.array_equal(want[ffi.PROBE_TO_MONT], O.to_mont(a_int, mod)) and O.from_mont(a, mod) == [x * pow(1 << 256, -1, mod) % mod for x in a_int]
    binary = (ffi.PROBE_MUL, ffi.PROBE_ADD, ffi.PROBE_SUB)
    for op, w in want.items():
        bb = b if op in binary else None
        hold(("field", field, op), lambda x, y, op=op: ffi.probe_field_op(ctx, field, op, x, y), (a, bb), w, ffi.host_field_op(field, op, a, bb))
    if field == 0:  # the four-row product of a challenge-shaped operand (mont_rows<4>)
        sa, sc = shifted_challenge_grid()
        assert not sc[:, :2].any() and (~sc.any(axis=1)).any() and ((sc[:, 2] == np.uint64(2**64 - 1)) & (sc[:, 3] == np.uint64((1 << 61) - 1))).any()  # low limbs zero; zero; all ones
        host = np.stack([ffi.host_fr_mul_shifted(x, y) for x, y in zip(sa, sc)])
        assert np.array_equal(host, ffi.host_field_op(0, ffi.PROBE_MUL_SHIFTED, sa, sc))
        hold(("field", 0, "mul_shifted"), lambda x, y: ffi.probe_field_op(ctx, 0, ffi.PROBE_MUL_SHIFTED, x, y), (sa, sc), O.fr_mul(sa, sc), host)


# ------------------------------------------------------------------------------------------------------ limb-form Fq
def test_limb_form_ops_on_the_device_match_the_oracle_and_the_host_form(ctx):
    vals, tuples = limb_form_grid()
    raw = [sum(int(w) << (64 * k) for k, w in enumerate(row)) for row in vals]
    assert all(v in raw for v in (0, 1, Q - 1, Q - 2, Q - 3, (1 << 232) - 1, (1 << 253) - 1))
    assert any(raw[a] < raw[b] for a, b, _, _ in tuples) and any(raw[a] < raw[b] + 2 * raw[c] for a, b, c, _ in tuples)  # the subtrahend LARGER than the minuend
    assert any(raw[a] == 0 and raw[b] for a, b, _, _ in tuples) and any(raw[a] == Q - 1 for a, _, _, _ in tuples)
    a, b, c, d = (tile(vals[[t[k] for t in tuples]]) for k in range(4))
    mul, add, sub = O.fq_mul, O.fq_add, O.fq_sub
    want = [mul(a, b), mul(a, a), add(mul(a, b), mul(c, d)), mul(sub(a, b), c), mul(sub(sub(a, b), add(c, c)), d)]
    takes = [(a, b, None, None), (a, None, None, None), (a, b, c, d), (a, b, c, None), (a, b, c, d)]
    for op in range(5):
        ops = takes[op]
        host = np.stack([ffi.host_fq_limb_op(op, *[None if o is None else o[i] for o in ops]) for i in range(len(tuples))])
        hold(("fq limb", op), lambda *xs, op=op: ffi.probe_fq_limb_op(ctx, op, *xs), ops, want[op], tile(host))


def test_limb_form_mixed_addition_paths_on_the_device(ctx):
    """the twin of jolt_host_g1xl_add_paths over every case of tests/test_limb_add_paths_cpu.py in ONE launch: the common path limb for limb against the integer
    model, the true special cases (identity accumulator, doubling, cancellation, P = 0 as an integer) against what the group law says, the planted false positives,
    and every output word against the host build"""
    cases = [("random", acc, q, neg, {}) for acc, q, neg in add_paths_random_cases()] + list(add_paths_special_cases()) + list(add_paths_false_positive_cases())
    kinds = [c[0] for c in cases]
    assert {k: kinds.count(k) for k in sorted(set(kinds))} == {"cancel": 36, "double": 36, "identity": 24, "incoming": 32, "p_zero": 6, "planted": 160, "random": 406}
    assert {c[4]["zz"] for c in cases if c[0] == "identity"} == {0, Q} and {c[3] for c in cases if c[0] == "double"} == {False, True}
    acc = np.array([[limbs(v) for v in c[1]] for c in cases], dtype=np.uint32).reshape(-1, 36)
    q = np.array([[limbs(v) for v in c[2]] for c in cases], dtype=np.uint32).reshape(-1, 18)
    neg = np.array([1 if c[3] else 0 for c in cases], dtype=np.int32)
    got = ffi.probe_g1xl_add_paths(ctx, acc, q, neg)
    keys = ("common", "full", "step", "suspect", "canon_common", "canon_full")
    host = [ffi.host_g1xl_add_paths(acc[i], q[i], bool(neg[i])) for i in range(len(cases))]
    for k in keys:  # (b) the two builds of one source
        assert differing(got[k], np.stack([np.asarray(h[k]) for h in host])) == [], k
    seen_rep, found = set(), 0
    for i, (kind, a_, q_, negate, info) in enumerate(cases):  # (a) the model and the group law, as the CPU test states them
        common, full, step = got["common"][i], got["full"][i], got["step"][i]
        assert (common[:, :8] <= MASK).all() and (full[:, :8] <= MASK).all() and (step[:, :8] <= MASK).all(), i
        zz3 = value(common[2])
        if kind in ("random", "planted", "incoming"):
            hit = zz3 & MASK in (0, P0)
            assert [value(r) for r in common] == model_common(*a_, *q_, negate), (kind, i)
            assert bool(got["suspect"][i]) == hit and np.array_equal(step, common), (kind, i)
            if negate:
                assert np.array_equal(got["canon_common"][i], got["canon_full"][i]) and all(value(x) % Q == value(y) % Q for x, y in zip(common, full))
            else:
                assert np.array_equal(common, full), (kind, i)
            if kind == "random":
                assert not hit
            if kind == "planted":
                assert zz3 in (info["t"], info["t"] + Q) and zz3 % Q != 0 and hit == (zz3 == info["t"] or info["lo"] == 0)
                found += hit
            continue
        assert got["suspect"][i] and np.array_equal(step, full), (kind, i)
        if kind == "identity":
            assert [value(r) for r in step] == [q_[0], (Q - q_[1]) if negate else q_[1], RL, RL]
            seen_rep.add(zz3)
        elif kind == "p_zero":
            assert zz3 == 0
        else:
            assert zz3 in (0, Q)
            seen_rep.add(zz3)
            if kind == "double":
                x, y = info["x"], info["y"]
                xs, _, zv = [value(r) % Q for r in step[:3]]
                lam = 3 * x * x * oracle_inv(2 * y % Q) % Q
                assert zv != 0 and xs * oracle_inv(zv) % Q == (lam * lam - 2 * x) % Q
            else:
                assert not step.any()
    assert seen_rep == {0, Q} and found >= 33
    for n in SIZES:  # the probe's tail guard
        part = ffi.probe_g1xl_add_paths(ctx, acc[:n], q[:n], neg[:n])
        for k in keys:
            assert differing(part[k], got[k][:n]) == [], (k, n)
    flipped = got["step"].copy()
    flipped[407, 3, 8] ^= np.uint32(1)
    assert differing(flipped, np.stack([h["step"] for h in host])) == [407]


# ------------------------------------------------------------------------------------------------------ Fq2, G2, Fq12
def test_fq2_ops_on_the_device_match_python_integers_and_the_host_form(ctx):
    corners, rand = fq2_grid()
    assert (0, 0) in corners and (Q - 1, Q - 1) in corners and (1, 0) in corners and (0, 1) in corners
    lefts, rights = corners + rand, corners + rand[:2]
    pairs = [(x, y) for x in lefts for y in rights]
    assert ((Q - 1, Q - 1), (Q - 1, Q - 1)) in pairs and ((0, 0), (Q - 1, Q - 1)) in pairs  # the largest operands against each other, and a borrow in both components
    to_abi = lambda xs: np.stack([M.fq2_to_abi(x) for x in xs])
    a2, b2, a1 = tile(to_abi([p[0] for p in pairs])), tile(to_abi([p[1] for p in pairs])), tile(to_abi(lefts))
    for op, model in ((ffi.FQ2_ADD, M.f2_add), (ffi.FQ2_SUB, M.f2_sub), (ffi.FQ2_MUL, M.f2_mul)):
        want = tile(to_abi([model(x, y) for x, y in pairs]))
        host = tile(np.stack([ffi.host_fq2_op(op, M.fq2_to_abi(x), M.fq2_to_abi(y)) for x, y in pairs]))
        hold(("fq2", op), lambda x, y, op=op: ffi.probe_fq2_op(ctx, op, x, y), (a2, b2), want, host)
    for op, model in ((ffi.FQ2_SQR, M.f2_sqr), (ffi.FQ2_NEG, M.f2_neg)):
        want = tile(to_abi([model(x) for x in lefts]))
        host = tile(np.stack([ffi.host_fq2_op(op, M.fq2_to_abi(x)) for x in lefts]))
        hold(("fq2", op), lambda x, op=op: ffi.probe_fq2_op(ctx, op, x), (a1,), want, host)


def test_g2_ops_on_the_device_match_the_model_and_the_host_form(ctx):
    grid = g2_grid()
    pa, pb, A, B, ident, garbage = grid["points"]
    adds, doubles, eqs = grid["add"], grid["double"], grid["eq"]
    # every exceptional case of the addition: doubling across representatives, cancellation, the identity on either side; the identity doubled
    assert [w for _, _, w in adds] == [M.add(pa, pb), M.double(pa), None, pb, pb] and not np.array_equal(adds[1][0], adds[1][1])
    assert not M.from_abi(adds[3][0]) and not M.from_abi(adds[4][1]) and [w for _, w in doubles] == [M.double(pb), None]
    assert [w for _, _, w in eqs] == [True, False, False, True, False]
    p, q = tile(np.stack([t[0] for t in adds])), tile(np.stack([t[1] for t in adds]))
    host = tile(np.stack([ffi.host_g2_add(t[0], t[1]) for t in adds]))
    assert [M.from_abi(h) for h in host[:5]] == [w for _, _, w in adds]  # the host form is the model's point; the device is then held to the host form's very words
    hold(("g2", "add"), lambda x, y: ffi.probe_g2_op(ctx, ffi.PROBE_G2_ADD, x, y), (p, q), host, host)
    p = tile(np.stack([t[0] for t in doubles]))
    host = tile(np.stack([ffi.host_g2_double(t[0]) for t in doubles]))
    assert [M.from_abi(h) for h in host[:2]] == [w for _, w in doubles]
    hold(("g2", "double"), lambda x: ffi.probe_g2_op(ctx, ffi.PROBE_G2_DOUBLE, x), (p,), host, host)
    p, q = tile(np.stack([t[0] for t in eqs])), tile(np.stack([t[1] for t in eqs]))
    want = tile(np.array([t[2] for t in eqs]))
    host = tile(np.array([ffi.host_g2_eq(t[0], t[1]) for t in eqs]))
    for n in (want.shape[0],) + SIZES:
        got = ffi.probe_g2_op(ctx, ffi.PROBE_G2_EQ, p[:n], q[:n])
        assert differing(got, want[:n]) == [] and differing(got, host[:n]) == [], n
    assert differing(~got, want[:n]) == list(range(n))
    for got_pt, (_, _, w) in zip(ffi.probe_g2_op(ctx, ffi.PROBE_G2_ADD, np.stack([t[0] for t in adds]), np.stack([t[1] for t in adds])), adds):
        assert M.from_abi(got_pt) == w  # and the device's own words read by the model


def test_fq12_ops_on_the_device_match_the_model_and_the_host_form(ctx):
    operands, sparse = fq12_grid()
    assert PM.ZERO in operands and PM.ONE in operands and operands[-1] == sparse
    assert sum(1 for c in sparse if c) == 6  # the shape of a Miller line: three Fq2 coefficients (the host form refuses any other shape)
    abi = [PM.gt_to_abi(x) for x in operands]
    assert np.array_equal(abi[5], np.tile(np.array(O.int_to_limbs((Q - 1) * O.MONT_R % Q), dtype=np.uint64), 12))  # q - 1 in every coefficient
    pairs = [(i, j) for i in range(7) for j in range(7)]
    a2, b2 = tile(np.stack([abi[i] for i, _ in pairs])), tile(np.stack([abi[j] for _, j in pairs]))
    want = tile(np.stack([PM.gt_to_abi(PM.f12_mul(operands[i], operands[j])) for i, j in pairs]))
    host = tile(np.stack([ffi.host_fq12_op(ffi.FQ12_MUL, abi[i], abi[j]) for i, j in pairs]))
    hold(("fq12", "mul"), lambda x, y: ffi.probe_fq12_op(ctx, ffi.FQ12_MUL, x, y), (a2, b2), want, host)
    a1, s1 = tile(np.stack(abi)), tile(np.stack([abi[-1]] * 7))
    want = tile(np.stack([PM.gt_to_abi(PM.f12_mul(x, sparse)) for x in operands]))  # the line routine against the dense product
    host = tile(np.stack([ffi.host_fq12_op(ffi.FQ12_MUL_SPARSE, X, abi[-1]) for X in abi]))
    hold(("fq12", "mul_sparse"), lambda x, y: ffi.probe_fq12_op(ctx, ffi.FQ12_MUL_SPARSE, x, y), (a1, s1), want, host)
    for op, model in ((ffi.FQ12_SQR, PM.f12_sqr), (ffi.FQ12_CONJ, PM.f12_conj)):
        want = tile(np.stack([PM.gt_to_abi(model(x)) for x in operands]))
        host = tile(np.stack([ffi.host_fq12_op(op, X) for X in abi]))
        hold(("fq12", op), lambda x, op=op: ffi.probe_fq12_op(ctx, op, x), (a1,), want, host)


# ------------------------------------------------------------------------------------------------------ suffixes
@pytest.mark.parametrize("length", list(range(0, 128, 8)))
def test_suffix_polynomials_on_the_device_match_the_model_the_oracle_and_the_host_form(ctx, length):
    """all 48 kinds over interesting_bits at the 16 suffix lengths of the phases, 0, 8, .., 120, which hold every length tests/test_oracle_read_raf.py parametrises:
    253 suffixes x 48 kinds per length"""
    grid = interesting_bits(np.random.default_rng(100 + length), length)
    assert len(grid) == 253
    n_kinds = len(KINDS)
    want = np.array([suffix_model(kind, bits, length) for bits in grid for kind in range(n_kinds)], dtype=np.uint64)
    table = want.reshape(len(grid), n_kinds)
    ops = [uninterleave(bits, length) for bits in grid]
    if length >= 8:  # what the grid is there for, on the model alone
        for kind in sorted(ZERO_ONE):
            values = set(table[:, KINDS.index(kind)].tolist())
            if kind == "One" or (kind == "OverflowBitsZero" and length <= 64):
                assert values == {1}, kind  # constant by definition: One always, OverflowBitsZero while the suffix has no bit above 64
            else:
                assert values == {0, 1}, (kind, length)
        assert any(y == 0 and x != 0 for x, _, y, _ in ops)  # ctz of zero (64, cut to y's length): RightShift(W), SignExtension
        assert any(x == 0 and y != 0 for x, _, y, _ in ops) and any(x == 0 and y == 0 for x, _, y, _ in ops)
        runs = [leading_ones(y, yl) for _, _, y, yl in ops]
        assert 0 in runs and ops[0][3] in runs and any(0 < r < ops[0][3] for r in runs)  # no leading one, all ones, a partial run
        assert any(y and y & (y - 1) == 0 for _, _, y, _ in ops) or length < 8  # a single bit of y: WindowSign reads bit ilog2(y) of x
        if length >= 64:  # shift amounts of 32 and more exist from here on; the helpers' 1 << k then leaves the low word
            assert any(r >= 32 for r in runs) and any(bin(y).count("1") >= 32 for _, _, y, _ in ops)
            for kind in ("RightShiftHelper", "PextHelper"):
                assert (table[:, KINDS.index(kind)] >= np.uint64(1 << 32)).any(), kind
        # amounts of 64 and more cannot come from a run or a count (y has at most 60 bits at length 120); they come from ctz(0) = 64, asserted above
    kinds = np.tile(np.arange(n_kinds, dtype=np.uint32), len(grid))
    bits = [b for b in grid for _ in range(n_kinds)]
    lens = np.full(len(bits), length, dtype=np.uint32)
    host = np.array([ffi.host_suffix_mle(int(k), b, length) for k, b in zip(kinds, bits)], dtype=np.uint64)
    oracle = np.array([O.suffix_mle(int(k), b, length) for k, b in zip(kinds, bits)], dtype=np.uint64)
    assert differing(oracle, want) == []
    bits_arr = np.array(bits, dtype=object)
    hold(("suffix", length), lambda k, b, l: ffi.probe_suffix_mle(ctx, k, list(b), l), (kinds, bits_arr, lens), want, host)


# ------------------------------------------------------------------------------------------------------ Dory field rows
def test_dory_field_row_digits_on_the_device_recombine_and_match_the_host_form(ctx):
    values = dory_fr_scalars()
    assert len(values) == 207 and all(v in values for v in (0, 1, R - 1, (R - 1) // 2, (R + 1) // 2)) and sum(min(s, R - s).bit_length() > 250 for s in values) > 100
    mont = O.to_mont(values)
    for c in range(3, 14):
        B, W = 1 << (c - 1), (254 + c) // c
        digits, negative = ffi.probe_dory_fr_digits(ctx, mont, c, W)
        for i, s in enumerate(values):  # (a) the big-integer reconstruction
            total = sum(int(d) << (c * w) for w, d in enumerate(digits[i]))
            assert all(-B <= int(d) <= B for d in digits[i]) and total == min(s, R - s) and bool(negative[i]) == (R - s < s), (c, s)
            h_digits, h_neg = ffi.host_dory_fr_digits(mont[i], c, W)  # (b)
            assert h_digits == digits[i].tolist() and h_neg == bool(negative[i]), (c, s)
        for n in SIZES:
            part, part_neg = ffi.probe_dory_fr_digits(ctx, mont[:n], c, W)
            assert differing(part, digits[:n]) == [] and differing(part_neg, negative[:n]) == [], (c, n)
    # the comparers' control, at the last window width: one flipped bit is seen by the comparison with the host form and by the recombination
    host = np.array([ffi.host_dory_fr_digits(m, c, W)[0] for m in mont], dtype=np.int64)
    recombined = lambda rows: [sum(int(d) << (c * w) for w, d in enumerate(row)) for row in rows]
    magnitudes = [min(s, R - s) for s in values]
    assert differing(digits, host) == [] and recombined(digits) == magnitudes
    flipped = digits.copy()
    flipped[99, 0] ^= 1
    assert differing(flipped, host) == [99] and [i for i, (x, y) in enumerate(zip(recombined(flipped), magnitudes)) if x != y] == [99]


# ------------------------------------------------------------------------------------------------------ small-scalar accumulator
@pytest.mark.parametrize("name", ["i128", "i64", "u64"])
def test_small_scalar_dots_on_the_device_match_python_integers_and_the_host_form(ctx, name):
    kind = {"i128": ffi.INT_I128, "i64": ffi.INT_I64, "u64": ffi.INT_U64}[name]
    values, ints, offsets = small_scalar_columns()[name]
    lo_, hi_ = {"i128": (-2**127, 2**127 - 1), "i64": (-2**63, 2**63 - 1), "u64": (0, 2**64 - 1)}[name]
    slices = list(zip(offsets, offsets[1:]))
    assert all(lo_ <= x <= hi_ for x in ints) and lo_ in ints and hi_ in ints and 0 in ints and (name == "u64" or -1 in ints)  # the kind's extremes
    assert (0, 0) in slices and max(hi - lo for lo, hi in slices) == (5000 if name == "i128" else 5) and len(slices) >= MIN_TUPLES
    big = hi_ if name == "u64" else lo_
    assert name == "i128" or any(ints[lo:hi] == [big] * 3 for lo, hi in slices)  # a slice of nothing but the largest magnitude
    v_int = O.from_mont(values)
    want = O.to_mont([sum(v * s for v, s in zip(v_int[lo:hi], ints[lo:hi])) % R for lo, hi in slices])
    host = ffi.host_small_scalar_dots(values, ints, kind, offsets)
    offs = np.array(offsets, dtype=np.uint64)
    assert differing(host, want) == []
    for n in (len(slices),) + SIZES:
        got = ffi.probe_small_scalar_dots(ctx, values, ints, kind, offs[:n + 1])
        assert differing(got, want[:n]) == [] and differing(got, host[:n]) == [], (name, n)
    flipped = got.copy()
    flipped[7, 0] ^= np.uint64(1 << 63)
    assert differing(flipped, want[:n]) == [7]


# ------------------------------------------------------------------------------------------------------ refusals
def test_refused_calls_launch_nothing_write_nothing_and_leave_the_context_usable(ctx):
    """null arrays, n over the cap, operands that are not canonical where the host form refuses them, a mul_shifted operand with non-zero low limbs, unknown ops: the
    host form's status, the output's sentinel untouched.  Nothing here reaches a kernel."""
    SENT, SENT32 = np.uint64(0xA5A5A5A5A5A5A5A5), np.uint32(0xA5A5A5A5)
    a = limbs64([3, 4, 5])
    not_canonical_fq = np.array(O.int_to_limbs(Q), dtype=np.uint64)

    def refused(status, call, out):
        before = out.copy()
        assert (before == before.flat[0]).all() and before.flat[0] in (SENT, SENT32)
        with pytest.raises(ffi.JoltError) as e:
            call(out)
        assert e.value.status == status and np.array_equal(out, before)

    fresh = lambda *shape: np.full(shape, SENT, dtype=np.uint64)
    cap = (1 << 20) + 1
    refused(1, lambda o: ffi.probe_field_op(ctx, 0, ffi.PROBE_MUL, a, None, out=o), fresh(3, 4))                 # a binary op without b
    refused(1, lambda o: ffi.probe_field_op(ctx, 0, ffi.PROBE_NEG, None, None, n=3, out=o), fresh(3, 4))         # no operand at all
    refused(1, lambda o: ffi.probe_field_op(None, 0, ffi.PROBE_MUL, a, a, out=o), fresh(3, 4))                   # no context
    refused(1, lambda o: ffi.probe_field_op(ctx, 2, ffi.PROBE_MUL, a, a, out=o), fresh(3, 4))                    # unknown field
    refused(1, lambda o: ffi.probe_field_op(ctx, 0, 9, a, a, out=o), fresh(3, 4))                                # unknown op
    refused(1, lambda o: ffi.probe_field_op(ctx, 0, -1, a, a, out=o), fresh(3, 4))
    refused(1, lambda o: ffi.probe_field_op(ctx, 1, ffi.PROBE_MUL_SHIFTED, a, np.zeros_like(a), out=o), fresh(3, 4))  # the four-row product is Fr's
    refused(1, lambda o: ffi.probe_field_op(ctx, 0, ffi.PROBE_MUL_SHIFTED, a, a, out=o), fresh(3, 4))            # low limbs not zero, as jolt_host_fr_mul_shifted
    with pytest.raises(ffi.JoltError) as e:
        ffi.host_fr_mul_shifted(a[0], a[1])
    assert e.value.status == 1
    refused(6, lambda o: ffi.probe_field_op(ctx, 0, ffi.PROBE_MUL, a, a, n=cap, out=o), fresh(3, 4))             # over the cap: refused before anything is read
    refused(6, lambda o: ffi.probe_fq_limb_op(ctx, 0, a, a, n=cap, out=o), fresh(3, 4))
    refused(1, lambda o: ffi.probe_fq_limb_op(ctx, 2, a, a, a, None, out=o), fresh(3, 4))
    refused(1, lambda o: ffi.probe_fq_limb_op(ctx, 5, a, a, a, a, out=o), fresh(3, 4))
    good2 = np.stack([M.fq2_to_abi((3, 4))] * 3)
    bad2 = good2.copy()
    bad2[1, 4:8] = not_canonical_fq
    refused(1, lambda o: ffi.probe_fq2_op(ctx, ffi.FQ2_MUL, bad2, good2, out=o), fresh(3, 8))                     # not canonical: whichever side, as jolt_host_fq2_op
    refused(1, lambda o: ffi.probe_fq2_op(ctx, ffi.FQ2_ADD, good2, bad2, out=o), fresh(3, 8))
    refused(1, lambda o: ffi.probe_fq2_op(ctx, ffi.FQ2_SQR, bad2, out=o), fresh(3, 8))
    refused(1, lambda o: ffi.probe_fq2_op(ctx, 5, good2, good2, out=o), fresh(3, 8))
    refused(6, lambda o: ffi.probe_fq2_op(ctx, ffi.FQ2_ADD, good2, good2, n=cap, out=o), fresh(3, 8))
    with pytest.raises(ffi.JoltError) as e:
        ffi.host_fq2_op(ffi.FQ2_MUL, bad2[1], good2[1])
    assert e.value.status == 1
    good12 = np.stack([PM.gt_to_abi(list(range(1, 13)))] * 2)
    bad12 = good12.copy()
    bad12[1, 20:24] = not_canonical_fq
    refused(1, lambda o: ffi.probe_fq12_op(ctx, ffi.FQ12_MUL, good12, bad12, out=o), fresh(2, 48))
    refused(1, lambda o: ffi.probe_fq12_op(ctx, ffi.FQ12_SQR, bad12, out=o), fresh(2, 48))
    refused(1, lambda o: ffi.probe_fq12_op(ctx, ffi.FQ12_MUL_SPARSE, good12, good12, out=o), fresh(2, 48))        # not of the sparse shape, as jolt_host_fq12_op
    refused(1, lambda o: ffi.probe_fq12_op(ctx, 8, good12, good12, out=o), fresh(2, 48))
    refused(6, lambda o: ffi.probe_fq12_op(ctx, ffi.FQ12_INV, good12, out=o), fresh(2, 48))                       # host only: no kernel inverts in Fq12
    refused(6, lambda o: ffi.probe_fq12_op(ctx, ffi.FQ12_FROBENIUS2, good12, out=o), fresh(2, 48))
    refused(1, lambda o: ffi.probe_suffix_mle(ctx, [48, 0], [1, 2], [8, 8], out=o), fresh(2))                     # unknown kind, as jolt_host_suffix_mle
    refused(1, lambda o: ffi.probe_suffix_mle(ctx, [0, 1], [1, 2], [8, 129], out=o), fresh(2))
    refused(6, lambda o: ffi.probe_suffix_mle(ctx, [0, 1], [1, 2], [8, 8], n=cap, out=o), fresh(2))
    digits = np.full((3, 20), 0xA5A5A5A5, dtype=np.uint32)
    for c, W in ((2, 20), (14, 20), (13, 0), (13, 86)):
        with pytest.raises(ffi.JoltError) as e:
            ffi.probe_dory_fr_digits(ctx, a, c, W, out=digits)
        assert e.value.status == 1 and (digits == 0xA5A5A5A5).all()
    with pytest.raises(ffi.JoltError) as e:
        ffi.probe_dory_fr_digits(ctx, np.array([O.int_to_limbs(R)] * 3, dtype=np.uint64), 13, 20, out=digits)    # the limbs of r: not a canonical scalar
    assert e.value.status == 1 and (digits == 0xA5A5A5A5).all()
    refused(6, lambda o: ffi.probe_dory_fr_digits(ctx, a, 13, 20, n=cap, out=o), np.full((3, 20), SENT32, dtype=np.uint32))
    refused(1, lambda o: ffi.probe_dory_fr_digits(ctx, None, 13, 20, n=3, out=o), np.full((3, 20), SENT32, dtype=np.uint32))
    # the entries with several outputs, through the library itself: every output keeps its sentinel
    lib, p_ = ffi.lib(), ffi._p
    g2 = np.stack([M.to_abi(M.GENERATOR)] * 3)
    for op, p, q, n in ((ffi.PROBE_G2_ADD, g2, None, 3), (ffi.PROBE_G2_EQ, None, g2, 3), (ffi.PROBE_G2_DOUBLE, None, None, 3), (3, g2, g2, 3), (-1, g2, g2, 3),
                        (ffi.PROBE_G2_ADD, g2, g2, cap), (ffi.PROBE_G2_EQ, g2, g2, cap)):
        out, equal = fresh(3, 24), np.full(3, 0x5A5A5A5A, dtype=np.int32)
        assert lib.jolt_probe_g2_op(ctx.h, op, p_(p), p_(q), n, p_(out), p_(equal)) == (6 if n == cap else 1), (op, n)
        assert (out == SENT).all() and (equal == 0x5A5A5A5A).all(), (op, n)
    out, equal = fresh(3, 24), np.full(3, 0x5A5A5A5A, dtype=np.int32)
    assert lib.jolt_probe_g2_op(ctx.h, ffi.PROBE_G2_ADD, p_(g2), p_(g2), 3, None, p_(equal)) == 1 and lib.jolt_probe_g2_op(ctx.h, ffi.PROBE_G2_EQ, p_(g2), p_(g2), 3, p_(out), None) == 1
    assert lib.jolt_probe_g2_op(None, ffi.PROBE_G2_ADD, p_(g2), p_(g2), 3, p_(out), p_(equal)) == 1 and (out == SENT).all() and (equal == 0x5A5A5A5A).all()
    acc, q18, neg = np.ones((3, 36), dtype=np.uint32), np.ones((3, 18), dtype=np.uint32), np.zeros(3, dtype=np.int32)
    for which, n in [(k, 3) for k in range(8)] + [(None, cap), ("ctx", 3)]:
        outs = [np.full((3, 36), SENT32, dtype=np.uint32) for _ in range(3)] + [np.full(3, 0x5A5A5A5A, dtype=np.int32), np.full((3, 64), SENT32, dtype=np.uint32)]
        args = [acc, q18, neg] + outs
        if isinstance(which, int):
            args[which] = None  # each of the three inputs and five outputs in turn
        status = lib.jolt_probe_g1xl_add_paths(None if which == "ctx" else ctx.h, p_(args[0]), p_(args[1]), p_(args[2]), n, *[p_(x) for x in args[3:]])
        assert status == (6 if n == cap else 1), (which, n)
        assert all((o == SENT32).all() for o in outs[:3] + outs[4:]) and (outs[3] == 0x5A5A5A5A).all(), (which, n)
    refused(1, lambda o: ffi.probe_small_scalar_dots(ctx, a, [1, 2, 3], 3, [0, 3], out=o), fresh(1, 4))                  # unknown integer kind
    refused(1, lambda o: ffi.probe_small_scalar_dots(ctx, a, [1, 2, 3], ffi.INT_I64, [0, 4], out=o), fresh(1, 4))        # a slice past the column
    refused(1, lambda o: ffi.probe_small_scalar_dots(ctx, a, [1, 2, 3], ffi.INT_I64, [2, 1, 3], out=o), fresh(2, 4))     # offsets that descend
    refused(6, lambda o: ffi.probe_small_scalar_dots(ctx, a, [1, 2, 3], ffi.INT_U64, [0, 3], n_terms=cap, out=o), fresh(1, 4))
    # n = 0 is fine and writes nothing
    empty = np.zeros((0, 4), dtype=np.uint64)
    out = fresh(1, 4)
    ffi.probe_field_op(ctx, 0, ffi.PROBE_MUL, empty, empty, out=out)
    ffi.probe_fq_limb_op(ctx, 0, empty, empty, out=out)
    assert (out == SENT).all()
    # the context still works
    one = O.to_mont([1])
    assert np.array_equal(ffi.probe_field_op(ctx, 0, ffi.PROBE_MUL, one, one), one)
    assert np.array_equal(ffi.probe_field_op(ctx, 1, ffi.PROBE_ADD, a, a), O.fq_add(a, a))
