"""The two paths of the limb-form mixed addition (fq_limb.hip.h), host build: g1xl_add_mixed_common (no test on the straight line, a one-limb
`suspect` filter, the point's sign as a mask inside R) against the unchanged full function g1xl_add_mixed, and the slow path behind the flag.

The field arithmetic is exact integer arithmetic, so this file carries its own model of it in Python integers: a limb-form value is the integer
its nine 29-bit limbs spell (the top limb takes what a lazily reduced value has above 2^261), a product is (a b + M p) / 2^261 with the unique
M < 2^261 that makes the division exact, a difference is a + m p - b.  The model predicts every limb the common path may produce; the oracle
supplies the field inverse and the group law."""
import numpy as np

import oracle_lib as O
from jolt_amd import ffi

from corner_grids import MASK, P0, Q, RL, add_paths_false_positive_cases, add_paths_random_cases, add_paths_special_cases, curve_points, limbs, model_common, oracle_inv, value


def run(acc, q, negate):
    out = ffi.host_g1xl_add_paths(np.array([limbs(v) for v in acc], dtype=np.uint32), np.array([limbs(v) for v in q], dtype=np.uint32), negate)
    for k in ("common", "full", "step"):
        assert (out[k][:, :8] <= MASK).all(), k  # every output limb normalised
    return out


def check_common(out, acc, q, negate, want_suspect):
    """common path == model limb for limb; == the full function limb for limb (point as stored) or as canonical field elements (negated)"""
    want = model_common(*acc, *q, negate)
    assert [value(r) for r in out["common"]] == want
    assert out["suspect"] == want_suspect
    if negate:
        assert np.array_equal(out["canon_common"], out["canon_full"])
        assert all(value(a) % Q == value(b) % Q for a, b in zip(out["common"], out["full"]))
    else:
        assert np.array_equal(out["common"], out["full"])
    assert np.array_equal(out["step"], out["common"])  # nothing special happened: the loop keeps the common path's limbs


def test_common_path_equals_full_function_on_random_inputs():
    cases = list(add_paths_random_cases())
    assert len(cases) == 406
    for acc, q, negate in cases:
        out = run(acc, q, negate)
        hit = value(out["common"][2]) & MASK in (0, P0)  # ~2^-28 per case; the seed is fixed
        check_common(out, acc, q, negate, hit)
        assert not hit


def test_every_true_special_case_raises_suspect():
    seen_rep, count = set(), 0
    for kind, acc, q, negate, info in add_paths_special_cases():
        count += 1
        out = run(acc, q, negate)
        if kind == "identity":
            # identity accumulator, both representatives of ZZ = 0; the other coordinates are whatever the last addition left there
            ys = (Q - q[1]) if negate else q[1]
            assert out["suspect"]
            assert np.array_equal(out["step"], out["full"])
            assert [value(r) for r in out["step"]] == [q[0], ys, RL, RL]
            seen_rep.add(value(out["common"][2]))
        elif kind in ("double", "cancel"):
            # the accumulator holds +-(the point added), as (x zz, y zzz, zz, zzz) with zz = z^2, zzz = z^3 and any representatives
            x, y = info["x"], info["y"]
            assert out["suspect"], (info["sign"], negate, info["k"])
            assert value(out["common"][2]) in (0, Q)
            seen_rep.add(value(out["common"][2]))
            assert np.array_equal(out["step"], out["full"])
            if kind == "double":  # the same point again: doubling; otherwise its negative: the identity
                xs, yv, zv = [value(r) % Q for r in out["step"][:3]]
                lam = 3 * x * x * oracle_inv(2 * y % Q) % Q
                x2 = (lam * lam - 2 * x) % Q
                assert zv != 0 and xs * oracle_inv(zv) % Q == x2  # X / ZZ (the L-form factors cancel)
            else:
                assert not out["step"].any()
        else:
            # P = 0 as an integer (X = U2 + 8p, above the documented entry range but inside what the products accept): the representative 0 of the zero product
            assert kind == "p_zero" and not negate
            assert out["suspect"] and value(out["common"][2]) == 0 and np.array_equal(out["step"], out["full"])
    assert count == 6 * (2 * (2 + 6) + 1)
    assert seen_rep == {0, Q}  # both representatives of a zero ZZ3 went through the filter


def test_false_positives_keep_the_common_path():
    """limb 0 of ZZ3 is 0 or P(0) although ZZ3 != 0 mod p, built without search: choose the difference P and a target t, set ZZ = t P^-2 (L-form: ZZ3 = ZZ P^2 2^-522)
    and X = qx ZZ - P; the lazily reduced ZZ3 is then t or t + p."""
    found = {(lo, rep): 0 for lo in (0, P0) for rep in ("t", "t+p")}
    count = 0
    for kind, acc, q, negate, info in add_paths_false_positive_cases():
        count += 1
        out = run(acc, q, negate)
        if kind == "planted":
            t, lo = info["t"], info["lo"]
            zz3 = value(out["common"][2])
            assert zz3 in (t, t + Q) and zz3 % Q != 0
            hit = zz3 & MASK in (0, P0)
            assert hit == (zz3 == t or lo == 0)
            check_common(out, acc, q, negate, hit)
            if hit and not negate:
                found[(zz3 & MASK, "t" if zz3 == t else "t+p")] += 1
        else:
            # limb 0 of the INCOMING ZZ is 0 or P(0), value non-zero: not a special case either (the filter looks at ZZ3 alone, which covers ZZ = 0)
            assert kind == "incoming"
            check_common(out, acc, q, negate, value(out["common"][2]) & MASK in (0, P0))
    assert count == 2 * 80 + 2 * 16
    assert found[(0, "t")] >= 16 and found[(P0, "t")] >= 16 and found[(P0, "t+p")] >= 1, found


def test_lists_through_the_loop_match_the_group_law():
    jac, aff = curve_points(8, 75)
    inf = np.zeros(8, dtype=np.uint64)

    def check(order, negate):
        pts = np.stack([aff[k] if k >= 0 else inf for k in order])
        want = O.g1_identity()
        for k, s in zip(order, negate):
            if k >= 0:
                want = O.g1_add(want, O.g1_neg(jac[k]) if s else jac[k])
        got = ffi.host_g1_sum_limb_form(pts, np.array(negate, dtype=np.uint8))
        assert O.g1_eq(got, want) and O.g1_serialize_compressed(got) == O.g1_serialize_compressed(want), (order, negate)

    check([0, 1, 2, 3], [1, 0, 0, 0])              # the first point of a list negated
    check([0], [1])
    check([0, 1, 2, 3, 4, 5, 6, 7], [1, 0, 1, 0, 1, 1, 0, 1])
    check([0, 0, 1], [0, 0, 0])                    # the same point twice in a row
    check([0, 0, 1], [1, 1, 0])                    # ... both negated
    check([1, 2, 2, 2, 3], [0, 0, 0, 0, 1])        # ... and a third time onto 2P
    check([0, 0, 1, 2, 3], [0, 1, 0, 0, 1])        # P then -P with more points after it
    check([0, 0, 1, 2], [1, 0, 1, 0])              # -P then P
    check([1, 0, 0, 2, 2], [0, 0, 1, 1, 0])        # back to the identity in the middle of a list, twice
    check([0, 1, 1, 0], [0, 1, 0, 1])              # P - Q + Q - P = identity at the end
    check([-1, 0, 1], [0, 1, 0])                   # infinity first: the accumulator starts as the identity
    check([0, -1, 1, -1], [1, 1, 0, 0])            # infinity inside and at the end of a list
    check([-1, -1], [0, 1])
