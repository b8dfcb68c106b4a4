"""The two paths of the limb-form mixed addition (fq_limb.hip.h), host build: g1xl_add_mixed_common (no test on the straight line, a one-limb
`suspect` filter, the point's sign as a mask inside R) against the unchanged full function g1xl_add_mixed, and the slow path behind the flag.

The field arithmetic is exact integer arithmetic, so this file carries its own model of it in Python integers: a limb-form value is the integer
its nine 29-bit limbs spell (the top limb takes what a lazily reduced value has above 2^261), a product is (a b + M p) / 2^261 with the unique
M < 2^261 that makes the division exact, a difference is a + m p - b.  The model predicts every limb the common path may produce; the oracle
supplies the field inverse and the group law."""
import numpy as np

import oracle_lib as O
from jolt_amd import ffi

Q = O.Q_MOD
W = 261
RL = (1 << W) % Q                 # the L-form of 1
NP = (-pow(Q, -1, 1 << W)) % (1 << W)
MASK = (1 << 29) - 1
P0 = Q & MASK                     # fql::P(0)


def limbs(v):
    assert 0 <= v < 1 << (W + 3)
    return [(v >> (29 * k)) & MASK for k in range(8)] + [v >> 232]


def value(l):
    return sum(int(x) << (29 * k) for k, x in enumerate(l))


def mont(a, b, c=0, d=0):         # fql_mul / fql_sqr / fql_mul2 as integers
    t = a * b + c * d
    assert t < 169 * Q * Q
    return (t + (t * NP % (1 << W)) * Q) >> W


def model_common(X, Y, ZZ, ZZZ, qx, qy, negate):
    """the integers g1xl_add_mixed_common must produce, with the documented range of every difference asserted on the way"""
    U2, S2 = mont(qx, ZZ), mont(qy, ZZZ)
    P = U2 + 8 * Q - X
    R = 7 * Q - S2 - Y if negate else S2 + 4 * Q - Y
    assert 0.4 * Q < P < 9.6 * Q and ((1.8 * Q < R < 7 * Q) if negate else (0.4 * Q < R < 5.6 * Q))
    PP = mont(P, P)
    PPP, Qv, ZZ3 = mont(P, PP), mont(X, PP), mont(ZZ, PP)
    X3 = mont(R, R) + 6 * Q - PPP - 2 * Qv
    assert 1.2 * Q < X3 < 7.6 * Q
    Y3 = mont(R, Qv + 8 * Q - X3, 4 * Q - Y, PPP)
    assert Y3 < 1.44 * Q and ZZ3 < 1.6 * Q
    return [X3, Y3, ZZ3, mont(ZZZ, PPP)]


def oracle_inv(v):
    r = O.from_mont(O.fq_inv(O.to_mont([v], Q)), Q)[0]
    assert r * v % Q == 1
    return r


def run(acc, q, negate):
    out = ffi.host_g1xl_add_paths(np.array([limbs(v) for v in acc], dtype=np.uint32), np.array([limbs(v) for v in q], dtype=np.uint32), negate)
    for k in ("common", "full", "step"):
        assert (out[k][:, :8] <= MASK).all(), k  # every output limb normalised
    return out


def rand_below(rng, bound):
    return int.from_bytes(rng.bytes(40), "little") % int(bound)


def rand_acc(rng):                # any representative inside the documented entry ranges
    return [rand_below(rng, 7.6 * Q), rand_below(rng, 3.6 * Q), rand_below(rng, 1.6 * Q), rand_below(rng, 1.6 * Q)]


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
    rng = np.random.default_rng(71)
    edge = [int(7.6 * Q) - 1, int(3.6 * Q) - 1, int(1.6 * Q) - 1, int(1.6 * Q) - 1]
    cases = [rand_acc(rng) for _ in range(200)] + [edge, [1, 1, 1, 1], [edge[0], 0, 1, edge[3]]]
    for i, acc in enumerate(cases):
        q = [rand_below(rng, Q), rand_below(rng, Q)] if i % 7 else [Q - 1, Q - 1]
        for negate in (False, True):
            out = run(acc, q, negate)
            hit = value(out["common"][2]) & MASK in (0, P0)  # ~2^-28 per case; the seed is fixed
            check_common(out, acc, q, negate, hit)
            assert not hit


def curve_points(n, seed):
    rng = np.random.default_rng(seed)
    g = O.g1_generator()
    jac = [O.g1_scalar_mul(g, np.array([int(rng.integers(1, 2**62)), 0, 0, 0], dtype=np.uint64)) for _ in range(n)]
    return jac, O.g1_to_affine(np.stack(jac))


def aff_ints(a):                  # (x, y) of an affine point of the oracle (standard Montgomery words) as integers
    return O.from_mont(a[:4], Q)[0], O.from_mont(a[4:], Q)[0]


def test_every_true_special_case_raises_suspect():
    rng = np.random.default_rng(72)
    _, aff = curve_points(6, 73)
    seen_rep = set()
    for a in aff:
        x, y = aff_ints(a)
        q = [x * RL % Q, y * RL % Q]
        one = RL
        for negate in (False, True):
            ys = (Q - q[1]) if negate else q[1]
            # identity accumulator, both representatives of ZZ = 0; the other coordinates are whatever the last addition left there
            for zz in (0, Q):
                acc = rand_acc(rng)
                acc[2] = zz
                out = run(acc, q, negate)
                assert out["suspect"]
                assert np.array_equal(out["step"], out["full"])
                assert [value(r) for r in out["step"]] == [q[0], ys, one, one]
                seen_rep.add(value(out["common"][2]))
            # the accumulator holds +-(the point added), as (x zz, y zzz, zz, zzz) with zz = z^2, zzz = z^3 and any representatives
            for sign in (1, -1):
                z = rand_below(rng, Q - 1) + 1
                zz, zzz = z * z % Q, z * z * z % Q
                for k in range(3):
                    X = (x * zz * RL) % Q + k * Q
                    Y = (sign * y * zzz * RL) % Q + (k % 2) * Q
                    acc = [X, Y, zz * RL % Q, zzz * RL % Q]
                    out = run(acc, q, negate)
                    assert out["suspect"], (sign, negate, k)
                    assert value(out["common"][2]) in (0, Q)
                    seen_rep.add(value(out["common"][2]))
                    assert np.array_equal(out["step"], out["full"])
                    same = (sign == 1) != negate  # the same point again: doubling; otherwise its negative: the identity
                    if same:
                        xs, yv, zv = [value(r) % Q for r in out["step"][:3]]
                        lam = 3 * x * x * oracle_inv(2 * y % Q) % Q
                        x2 = (lam * lam - 2 * x) % Q
                        assert zv != 0 and xs * oracle_inv(zv) % Q == x2  # X / ZZ (the L-form factors cancel)
                    else:
                        assert not out["step"].any()
        # P = 0 as an integer (X = U2 + 8p, above the documented entry range but inside what the products accept): the representative 0 of the zero product
        zz = rand_below(rng, Q - 1) + 1
        acc = [mont(q[0], zz) + 8 * Q, rand_below(rng, 3.6 * Q), zz, rand_below(rng, 1.6 * Q)]
        out = run(acc, q, False)
        assert out["suspect"] and value(out["common"][2]) == 0 and np.array_equal(out["step"], out["full"])
    assert seen_rep == {0, Q}  # both representatives of a zero ZZ3 went through the filter


def test_false_positives_keep_the_common_path():
    """limb 0 of ZZ3 is 0 or P(0) although ZZ3 != 0 mod p, built without search: choose the difference P and a target t, set ZZ = t P^-2 (L-form: ZZ3 = ZZ P^2 2^-522)
    and X = qx ZZ - P; the lazily reduced ZZ3 is then t or t + p."""
    rng = np.random.default_rng(74)
    found = {(lo, rep): 0 for lo in (0, P0) for rep in ("t", "t+p")}
    for i in range(80):
        lo = (0, P0)[i % 2]
        small = i % 8 >= 6  # a tiny t: the product comes out as t + p whenever t < ZZ PP / 2^261 (limb 0 = lo + P(0): still in the filter only for lo = 0)
        t = (rand_below(rng, (Q // 4000 if small else Q) >> 29) << 29) | lo
        assert 0 < t < Q
        Pres = rand_below(rng, Q - 1) + 1
        zz = t * RL * RL * oracle_inv(Pres * Pres % Q) % Q
        q = [rand_below(rng, Q), rand_below(rng, Q)]
        X = (mont(q[0], zz) - Pres) % Q + (i % 7) * Q
        acc = [X, rand_below(rng, 3.6 * Q), zz, rand_below(rng, 1.6 * Q)]
        for negate in (False, True):
            out = run(acc, q, negate)
            zz3 = value(out["common"][2])
            assert zz3 in (t, t + Q) and zz3 % Q != 0
            hit = zz3 & MASK in (0, P0)
            assert hit == (zz3 == t or lo == 0)
            check_common(out, acc, q, negate, hit)
            if hit and not negate:
                found[(zz3 & MASK, "t" if zz3 == t else "t+p")] += 1
    assert found[(0, "t")] >= 16 and found[(P0, "t")] >= 16 and found[(P0, "t+p")] >= 1, found
    # limb 0 of the INCOMING ZZ is 0 or P(0), value non-zero: not a special case either (the filter looks at ZZ3 alone, which covers ZZ = 0)
    for i in range(16):
        acc = rand_acc(rng)
        acc[2] = ((rand_below(rng, Q >> 29) << 29) | (0, P0)[i % 2]) or (1 << 29)
        q = [rand_below(rng, Q), rand_below(rng, Q)]
        for negate in (False, True):
            out = run(acc, q, negate)
            check_common(out, acc, q, negate, value(out["common"][2]) & MASK in (0, P0))


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
