"""The corner grids of the host forms (TEST INFRASTRUCTURE): the operand sets at which the CPU suite holds each piece of the kernels' arithmetic to an independent
reference, built in ONE place so that tests/test_gpu_device_probe.py runs the very same tuples through the device build (jolt_probe_*).

A builder draws from a generator it seeds itself, so the tuples do not depend on who asks or in which order.  Nothing here calls the library: a grid is operands
and, where the reference needs one, the integers of the exact model (the limb-form mixed addition below).
"""
import numpy as np

import oracle_lib as O

Q = O.Q_MOD
R = O.R_MOD
M64 = 2**64 - 1


def limbs64(ints):
    """Python integers below 2^256 -> (n, 4) uint64 little-endian limbs"""
    return np.array([[(v >> (64 * k)) & M64 for k in range(4)] for v in ints], dtype=np.uint64).reshape(-1, 4)


# ---------------------------------------------------------------------------------------------------- Fr / Fq: the device multiplication algorithm
def saturated_operands(mod):
    """the largest values below the modulus whose limbs are saturated: nine 29-bit limbs all 0x1FFFFFFF is 2^261 - 1 and eight 32-bit words all ones is 2^256 - 1,
    both above either modulus, so the low eight 29-bit limbs (seven 32-bit words) stay all ones and the top one is the largest that keeps the value below the modulus"""
    sat29 = (((mod >> 232) - 1) << 232) | ((1 << 232) - 1)
    sat32 = (((mod >> 224) - 1) << 224) | ((1 << 224) - 1)
    assert sat29 < mod and sat32 < mod and sat29 + (1 << 232) >= mod and sat32 + (1 << 224) >= mod
    assert all((sat29 >> (29 * k)) & 0x1FFFFFFF == 0x1FFFFFFF for k in range(8)) and all((sat32 >> (32 * k)) & 0xFFFFFFFF == 0xFFFFFFFF for k in range(7))
    return [sat29, sat32]


def field_grid(field):
    """(ints, vals, pairs) for field 0 = Fr, 1 = Fq: raw limbs (= Montgomery residues) and the index pairs (i, j) that are multiplied.  The first 160 operands and
    their 480 pairs are 0, 1, p - 1, p - 2, all-ones limb patterns and random values; then the saturated operands, each paired with itself, with each other and with
    the ten corner values on either side."""
    mod = (R, Q)[field]
    rng = np.random.default_rng(29)
    if field == 1:  # one generator served both fields in turn: Fq's draws follow Fr's
        rng.bytes(32 * 150)
    ints = [0, 1, 2, mod - 1, mod - 2, (1 << 253) - 1, (1 << 254) - 1 if (1 << 254) - 1 < mod else mod - 3, 0x1FFFFFFF, (1 << 29), ((1 << 232) - 1)]
    ints += [int.from_bytes(rng.bytes(32), "little") % mod for _ in range(150)]
    n = len(ints)
    pairs = [(i, j) for i in range(n) for j in (i, (i * 7 + 3) % n, n - 1 - i)]
    sat = saturated_operands(mod)
    ints += sat
    for s in range(n, n + len(sat)):
        pairs += [(s, t) for t in range(n, n + len(sat))]
        pairs += [(s, k) for k in range(10)] + [(k, s) for k in range(10)]
    return ints, limbs64(ints), pairs


def shifted_challenge_grid():
    """(a, c) for the four-row product of Fr: c's four low u32 limbs are zero (the shape of a sumcheck challenge); random challenges of 125 bits, the all-ones high limbs
    below the modulus, zero, single bits, against the corner values of the field grid"""
    ints, vals, _ = field_grid(0)
    rng = np.random.default_rng(30)
    highs = [0, 1, (1 << 125) - 1, ((1 << 61) - 1) << 64 | M64, 1 << 124, M64, 1 << 64] + [int.from_bytes(rng.bytes(16), "little") >> 3 for _ in range(24)]
    c = limbs64([h << 128 for h in highs])
    assert all(int(h) << 128 < R for h in highs)
    idx = [(i, k) for i in list(range(10)) + [160, 161] + list(range(10, 30)) for k in range(len(highs)) if i < 12 or k % 4 == i % 4]
    return vals[[i for i, _ in idx]], c[[k for _, k in idx]]


# ---------------------------------------------------------------------------------------------------- limb-form Fq (fq_limb.hip.h)
def limb_form_grid():
    """(vals, tuples): canonical Fq operands and the index tuples (a, b, c, d) the five limb-form ops are held to the oracle at"""
    rng = np.random.default_rng(61)
    mod = Q
    ints = [0, 1, 2, mod - 1, mod - 2, (1 << 253) - 1, mod - 3, 0x1FFFFFFF, 1 << 29, (1 << 232) - 1] + [int.from_bytes(rng.bytes(32), "little") % mod for _ in range(60)]
    n = len(ints)
    return limbs64(ints), [(i, (7 * i + 3) % n, n - 1 - i, (5 * i + 11) % n) for i in range(n)]


# The mixed addition on raw limbs.  The field arithmetic is exact integer arithmetic, so the grid carries its own model of it in Python integers: a limb-form value
# is the integer its nine 29-bit limbs spell (the top limb takes what a lazily reduced value has above 2^261), a product is (a b + M p) / 2^261 with the unique
# M < 2^261 that makes the division exact, a difference is a + m p - b.
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
    R_ = 7 * Q - S2 - Y if negate else S2 + 4 * Q - Y
    assert 0.4 * Q < P < 9.6 * Q and ((1.8 * Q < R_ < 7 * Q) if negate else (0.4 * Q < R_ < 5.6 * Q))
    PP = mont(P, P)
    PPP, Qv, ZZ3 = mont(P, PP), mont(X, PP), mont(ZZ, PP)
    X3 = mont(R_, R_) + 6 * Q - PPP - 2 * Qv
    assert 1.2 * Q < X3 < 7.6 * Q
    Y3 = mont(R_, Qv + 8 * Q - X3, 4 * Q - Y, PPP)
    assert Y3 < 1.44 * Q and ZZ3 < 1.6 * Q
    return [X3, Y3, ZZ3, mont(ZZZ, PPP)]


def oracle_inv(v):
    r = O.from_mont(O.fq_inv(O.to_mont([v], Q)), Q)[0]
    assert r * v % Q == 1
    return r


def rand_below(rng, bound):
    return int.from_bytes(rng.bytes(40), "little") % int(bound)


def rand_acc(rng):                # any representative inside the documented entry ranges
    return [rand_below(rng, 7.6 * Q), rand_below(rng, 3.6 * Q), rand_below(rng, 1.6 * Q), rand_below(rng, 1.6 * Q)]


def curve_points(n, seed):
    rng = np.random.default_rng(seed)
    g = O.g1_generator()
    jac = [O.g1_scalar_mul(g, np.array([int(rng.integers(1, 2**62)), 0, 0, 0], dtype=np.uint64)) for _ in range(n)]
    return jac, O.g1_to_affine(np.stack(jac))


def aff_ints(a):                  # (x, y) of an affine point of the oracle (standard Montgomery words) as integers
    return O.from_mont(a[:4], Q)[0], O.from_mont(a[4:], Q)[0]


def add_paths_random_cases():
    """(acc, q, negate): random representatives inside the entry ranges, the ranges' upper ends, tiny values; every seventh point (p - 1, p - 1)"""
    rng = np.random.default_rng(71)
    edge = [int(7.6 * Q) - 1, int(3.6 * Q) - 1, int(1.6 * Q) - 1, int(1.6 * Q) - 1]
    cases = [rand_acc(rng) for _ in range(200)] + [edge, [1, 1, 1, 1], [edge[0], 0, 1, edge[3]]]
    for i, acc in enumerate(cases):
        q = [rand_below(rng, Q), rand_below(rng, Q)] if i % 7 else [Q - 1, Q - 1]
        for negate in (False, True):
            yield acc, q, negate


def add_paths_special_cases():
    """(kind, acc, q, negate, info): every TRUE special case of the mixed addition.  kind "identity": the accumulator is the identity, both representatives of ZZ = 0
    (info: zz); "double" / "cancel": it holds the point added / its negative, as (x zz, y zzz, zz, zzz) in any representatives (info: x, y, sign, k);
    "p_zero": the difference P is 0 as an integer"""
    rng = np.random.default_rng(72)
    _, aff = curve_points(6, 73)
    for a in aff:
        x, y = aff_ints(a)
        q = [x * RL % Q, y * RL % Q]
        for negate in (False, True):
            for zz in (0, Q):
                acc = rand_acc(rng)
                acc[2] = zz
                yield "identity", acc, q, negate, {"zz": zz}
            for sign in (1, -1):
                z = rand_below(rng, Q - 1) + 1
                zz, zzz = z * z % Q, z * z * z % Q
                for k in range(3):
                    X = (x * zz * RL) % Q + k * Q
                    Y = (sign * y * zzz * RL) % Q + (k % 2) * Q
                    acc = [X, Y, zz * RL % Q, zzz * RL % Q]
                    same = (sign == 1) != negate  # the same point again: doubling; otherwise its negative: the identity
                    yield ("double" if same else "cancel"), acc, q, negate, {"x": x, "y": y, "sign": sign, "k": k}
        # P = 0 as an integer (X = U2 + 8p, above the documented entry range but inside what the products accept): the representative 0 of the zero product
        zz = rand_below(rng, Q - 1) + 1
        acc = [mont(q[0], zz) + 8 * Q, rand_below(rng, 3.6 * Q), zz, rand_below(rng, 1.6 * Q)]
        yield "p_zero", acc, q, False, {}


def add_paths_false_positive_cases():
    """(kind, acc, q, negate, info): limb 0 of ZZ3 is 0 or P(0) although ZZ3 != 0 mod p, built without search -- "planted": choose the difference P and a target t, set
    ZZ = t P^-2 (L-form: ZZ3 = ZZ P^2 2^-522) and X = qx ZZ - P; the lazily reduced ZZ3 is then t or t + p (info: t, lo).  "incoming": limb 0 of the INCOMING ZZ is
    0 or P(0), value non-zero."""
    rng = np.random.default_rng(74)
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
            yield "planted", acc, q, negate, {"t": t, "lo": lo}
    for i in range(16):
        acc = rand_acc(rng)
        acc[2] = ((rand_below(rng, Q >> 29) << 29) | (0, P0)[i % 2]) or (1 << 29)
        q = [rand_below(rng, Q), rand_below(rng, Q)]
        for negate in (False, True):
            yield "incoming", acc, q, negate, {}


# ---------------------------------------------------------------------------------------------------- the fixed-base MSM's digit recoding
def fx_digit_corners(c):
    """canonical scalars at which the recoding of c-bit windows (msm_fixed.hip fx_digits_of) has its worst cases: r - 1, (r - 1) / 2 and its neighbours (the negation
    threshold), digits of exactly 2^(c-1) and one beyond, all-ones windows whose carry runs through every window to the top"""
    return [0, 1, 2, R - 1, R - 2, (R - 1) // 2, (R - 1) // 2 + 1, (R + 1) // 2 + 1, (1 << 253) - 1, (1 << 252), (1 << (c - 1)), (1 << (c - 1)) + 1, (1 << c) - 1,
            sum(((1 << c) - 1) << (c * w) for w in range(253 // c)) % R, sum((1 << (c - 1)) << (c * w) for w in range(253 // c)) % R]


def fx_corner_grid(c):
    """the corners above, then the same digit corners one window at a time (2^(c-1), 2^(c-1) + 1 and the all-ones digit alone in every window, each also negated:
    r - s), as canonical integers: the scalars the sort paths of the device are fed in tests/test_gpu_msm_fixed_paths.py"""
    out = fx_digit_corners(c)
    for w in range(-(-253 // c)):
        for d in (1 << (c - 1), (1 << (c - 1)) + 1, (1 << c) - 1):
            s = (d << (c * w)) % R
            out += [s, R - s]
    return out


def fx_uniform_scalars(n, seed):
    """n uniform canonical scalars as Python integers"""
    rng = np.random.default_rng(seed)
    raw = rng.bytes(40 * n)
    return [int.from_bytes(raw[40 * i:40 * i + 40], "little") % R for i in range(n)]


def fx_planted_scalars(c, n, planted, seed):
    """n uniform canonical scalars with `planted` of them, spread evenly, replaced by scalars whose every c-bit digit is drawn from [1, 255]: all their entries land
    in segment 0 of the sort (buckets 1 .. 255), none carries, none is negated"""
    out = fx_uniform_scalars(n, seed)
    rng = np.random.default_rng(seed + 1)
    W = -(-253 // c)
    for k in range(planted):
        out[(k * n) // planted] = sum(int(d) << (c * w) for w, d in enumerate(rng.integers(1, 256, size=W)))
    return out


# ---------------------------------------------------------------------------------------------------- the small-scalar accumulator
def small_scalar_cases():
    """(n, values, scalars): n field elements against i128 scalars with the corners 0, -2^127, 2^127 - 1, -1 first"""
    from util import rand_fr
    rng = np.random.default_rng(90)
    for n in (0, 1, 4, 300, 5000):
        values = rand_fr(max(n, 1), 91 + n)[:n]
        scalars = [int(rng.integers(-2**62, 2**62)) * int(rng.integers(0, 2**63)) for _ in range(n)]
        scalars[: min(n, 4)] = [0, -(2**127), 2**127 - 1, -1][: min(n, 4)]
        yield n, values, scalars
    yield 200, rand_fr(200, 95), rng.integers(-2**48, 2**48, size=200, dtype=np.int64)  # small enough for the reference accumulator's five limbs


def small_scalar_columns():
    """{kind name: (values, ints, offsets)}: one column of machine integers per kind against field elements, cut into consecutive slices [offsets[i], offsets[i + 1])
    that are summed separately.  i128: the cases above end to end, each its own slice (1, 4, 300 and 5000 terms, the corners first), an empty slice, and the 200 small
    terms in pieces of one and two; i64 and u64: after an empty slice, three times the kind's largest magnitude as one slice, its other extremes, then random values, in pieces of 1, 2, 3 and 5 terms."""
    from util import rand_fr
    cases = [c for c in small_scalar_cases() if c[0]]
    values = np.concatenate([c[1] for c in cases])
    ints = [int(x) for c in cases for x in c[2]]
    offsets = [0, 0, 1, 5, 305, 5305]
    while offsets[-1] < len(ints):
        offsets.append(min(offsets[-1] + 1 + len(offsets) % 2, len(ints)))
    out = {"i128": (values, ints, offsets)}
    rng = np.random.default_rng(96)
    for name, corners, draw in (("i64", [-2**63] * 3 + [0, 2**63 - 1, -1, 1], lambda: int(rng.integers(-2**63, 2**63 - 1, endpoint=True))),
                                ("u64", [2**64 - 1] * 3 + [0, 1, 2**63, 2**32 - 1, 2**32], lambda: int(rng.integers(0, 2**64 - 1, endpoint=True, dtype=np.uint64)))):
        col = corners + [draw() for _ in range(360 - len(corners))]
        offs = [0, 0]
        while offs[-1] < len(col):
            offs.append(min(offs[-1] + (1, 2, 3, 5)[len(offs) % 4], len(col)))
        out[name] = (rand_fr(len(col), 97 + len(name)), col, offs)
    return out


# ---------------------------------------------------------------------------------------------------- Fq2, G2, Fq12
def fq2_grid():
    """(corners, rand): pairs of integers (c0, c1).  Binary ops run a in corners + rand against b in corners + rand[:2], unary ops a in corners + rand"""
    rng = np.random.default_rng(5)
    corners = [(0, 0), (1, 0), (0, 1), (Q - 1, Q - 1)]
    rand = [(int.from_bytes(rng.bytes(40), "little") % Q, int.from_bytes(rng.bytes(40), "little") % Q) for _ in range(4)]
    return corners, rand


def g2_grid():
    """add: (P, Q, want), double: (P, want), eq: (P, Q, want) with P, Q in the ABI's words and want a point of tests/g2_model.py (None = identity) or a bool: distinct
    points, P + P across representatives, P - P, the identity on either side and doubled, equality across representatives and of identities with garbage x, y"""
    import g2_model as M
    from dory_groups import rand_ints
    a, b = rand_ints(2, 21)
    pa, pb = M.mul_generator(a), M.mul_generator(b)
    A, B = M.to_abi(pa), M.to_abi(pb, M.f2(5, 7))
    ident = M.to_abi(None)
    garbage_identity = B.copy()
    garbage_identity[16:] = 0  # z = 0 with any x, y is the identity
    return {"points": (pa, pb, A, B, ident, garbage_identity),
            "add": [(A, B, M.add(pa, pb)), (A, M.to_abi(pa, M.f2(2, 9)), M.double(pa)), (A, M.to_abi(M.neg(pa), M.f2(3, 1)), None), (ident, B, pb), (B, ident, pb)],
            "double": [(B, M.double(pb)), (ident, None)],
            "eq": [(A, M.to_abi(pa, M.f2(11, 13)), True), (A, B, False), (A, M.to_abi(M.neg(pa)), False), (ident, garbage_identity, True), (ident, A, False)]}


def fq12_grid():
    """(operands, sparse): seven elements of the flat model (three random, zero, one, q - 1 in every coefficient, a sparse Miller-line shape); sparse is the last"""
    import pairing_model as PM
    rng = np.random.default_rng(6)
    rand = [[int.from_bytes(rng.bytes(40), "little") % Q for _ in range(12)] for _ in range(3)]
    sparse = PM.f12_add(PM.f12_from_fq2((rand[0][0], rand[0][1]), 0), PM.f12_add(PM.f12_from_fq2((rand[0][2], rand[0][3]), 1), PM.f12_from_fq2((rand[0][4], rand[0][5]), 3)))
    all_top = PM.gt_from_abi(PM.gt_to_abi([0] * 12) + np.tile(np.array(O.int_to_limbs((Q - 1) * O.MONT_R % Q), dtype=np.uint64), 12))  # q - 1 in every coefficient
    return rand + [PM.ZERO, PM.ONE, all_top, sparse], sparse


# ---------------------------------------------------------------------------------------------------- suffixes
def interesting_bits(rng, length):
    """lookup-index suffixes that exercise the corner branches: zero, all ones, one operand zero / all ones, single bits, random"""
    full = (1 << length) - 1 if length else 0
    odd = sum(1 << k for k in range(1, 128, 2)) & full    # x all ones, y zero
    even = sum(1 << k for k in range(0, 128, 2)) & full   # y all ones, x zero
    out = [0, full, odd, even, 1 & full, 2 & full, 3 & full, 4 & full, (1 << 62) & full, (1 << 63) & full, (1 << 31) & full, full >> 1, full ^ 1]
    for _ in range(40):
        v = int.from_bytes(rng.bytes(16), "little") & full
        out += [v, v & even, v & odd, v | even, v | odd]
        hi_ones = int(rng.integers(0, 64))
        out.append((v | (even ^ (even >> (2 * hi_ones)))) & full)  # y with a run of leading ones
    return out


# ---------------------------------------------------------------------------------------------------- Dory field rows
def dory_fr_scalars():
    rng = np.random.default_rng(2000)
    return [0, 1, R - 1, (R - 1) // 2, (R + 1) // 2, 2**64 - 1, 2**128] + [int.from_bytes(rng.bytes(40), "little") % R for _ in range(200)]
