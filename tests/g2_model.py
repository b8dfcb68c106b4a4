"""A Python big-integer model of Fq2 = Fq[u] / (u^2 + 1) and of BN254 G2, the twist y^2 = x^3 + 3 / (9 + u), for the Dory routine tests.

Independent of the library: affine coordinates and the chord-and-tangent formulas, where the library is Jacobian.  No memorised constant beyond the two
moduli oracle_lib already holds: the twist coefficient is computed, the subgroup generator is found (first x = 1, 2, ... with x^3 + b' a square in Fq2,
times the cofactor 2q - r) and its order is checked when the module is imported.  The identity is None.
"""
import numpy as np

from oracle_lib import MONT_R, Q_MOD, R_MOD, int_to_limbs, limbs_to_int

Q, R = Q_MOD, R_MOD


# ---------------------------------------------------------------- Fq2: pairs (c0, c1) of integers below q
def f2(a, b=0):
    return (a % Q, b % Q)


def f2_add(a, b): return ((a[0] + b[0]) % Q, (a[1] + b[1]) % Q)
def f2_sub(a, b): return ((a[0] - b[0]) % Q, (a[1] - b[1]) % Q)
def f2_neg(a): return (-a[0] % Q, -a[1] % Q)
def f2_mul(a, b): return ((a[0] * b[0] - a[1] * b[1]) % Q, (a[0] * b[1] + a[1] * b[0]) % Q)
def f2_sqr(a): return f2_mul(a, a)


def f2_inv(a):
    n = pow(a[0] * a[0] + a[1] * a[1], -1, Q)
    return (a[0] * n % Q, -a[1] * n % Q)


def _fq_sqrt(a):
    """q = 3 mod 4; None when a is no square"""
    s = pow(a, (Q + 1) // 4, Q)
    return s if s * s % Q == a % Q else None


def f2_sqrt(a):
    """a square root of a in Fq2, or None"""
    if a[1] == 0:
        s = _fq_sqrt(a[0])
        if s is not None:
            return (s, 0)
        s = _fq_sqrt(-a[0] % Q)  # (s u)^2 = -s^2
        return (0, s)
    alpha = _fq_sqrt((a[0] * a[0] + a[1] * a[1]) % Q)
    if alpha is None:
        return None
    half = pow(2, -1, Q)
    for delta in ((a[0] + alpha) * half % Q, (a[0] - alpha) * half % Q):
        x0 = _fq_sqrt(delta)
        if x0:
            r = (x0, a[1] * pow(2 * x0, -1, Q) % Q)
            if f2_sqr(r) == a:
                return r
    return None


assert Q % 4 == 3
B_TWIST = f2_mul(f2(3), f2_inv(f2(9, 1)))  # b' = 3 / (9 + u)
COFACTOR = 2 * Q - R


# ---------------------------------------------------------------- G2, affine, identity = None
def on_curve(p):
    return p is None or f2_sqr(p[1]) == f2_add(f2_mul(f2_sqr(p[0]), p[0]), B_TWIST)


def neg(p):
    return None if p is None else (p[0], f2_neg(p[1]))


def double(p):
    if p is None or p[1] == (0, 0):
        return None
    lam = f2_mul(f2_mul(f2(3), f2_sqr(p[0])), f2_inv(f2_add(p[1], p[1])))
    x = f2_sub(f2_sqr(lam), f2_add(p[0], p[0]))
    return (x, f2_sub(f2_mul(lam, f2_sub(p[0], x)), p[1]))


def add(p, q):
    if p is None:
        return q
    if q is None:
        return p
    if p[0] == q[0]:
        return double(p) if p[1] == q[1] else None
    lam = f2_mul(f2_sub(q[1], p[1]), f2_inv(f2_sub(q[0], p[0])))
    x = f2_sub(f2_sub(f2_sqr(lam), p[0]), q[0])
    return (x, f2_sub(f2_mul(lam, f2_sub(p[0], x)), p[1]))


def mul(p, k):
    """k * p for any non-negative integer k"""
    acc = None
    for bit in bin(k)[2:] if k else "":
        acc = double(acc)
        if bit == "1":
            acc = add(acc, p)
    return acc


def _first_point():
    x = 1
    while True:
        y = f2_sqrt(f2_add(f2_mul(f2_sqr(f2(x)), f2(x)), B_TWIST))
        if y is not None:
            return (f2(x), y)
        x += 1


TWIST_POINT = _first_point()           # on the twist, of no particular order
GENERATOR = mul(TWIST_POINT, COFACTOR)  # of order r
assert on_curve(TWIST_POINT) and on_curve(GENERATOR)
assert GENERATOR is not None and mul(GENERATOR, R) is None


_GEN_TABLE = []


def mul_generator(k):
    """(k mod r) * GENERATOR through a table of d * 256^w * GENERATOR (32 windows of 8 bits, built on first use): 32 additions at most, where mul takes ~380
    group operations -- what lets the GPU tests check every element of a vector.  tests/test_dory_routines_cpu.py holds it against mul."""
    if not _GEN_TABLE:
        base = GENERATOR
        for _ in range(32):
            row, acc = [None], None
            for _ in range(255):
                acc = add(acc, base)
                row.append(acc)
            _GEN_TABLE.append(row)
            base = add(acc, base)  # 256 * base
    k %= R
    acc = None
    for w in range(32):
        acc = add(acc, _GEN_TABLE[w][(k >> (8 * w)) & 255])
    return acc


# ---------------------------------------------------------------- the library's representation: (24,) uint64, Jacobian, Montgomery
def _fq_limbs(v):
    return int_to_limbs(v % Q * MONT_R % Q)


def fq2_to_abi(a):
    return np.array(_fq_limbs(a[0]) + _fq_limbs(a[1]), dtype=np.uint64)


_RINV = pow(MONT_R, -1, Q)


def fq2_from_abi(a):
    a = np.asarray(a, dtype=np.uint64).reshape(8)
    return (limbs_to_int(a[:4]) * _RINV % Q, limbs_to_int(a[4:]) * _RINV % Q)


def to_abi(p, z=None):
    """p as a Jacobian point; z (an Fq2 pair, non-zero) picks the representative (x z^2, y z^3, z), default z = 1.  The identity is (1, 1, 0)."""
    if p is None:
        return np.concatenate([fq2_to_abi(f2(1)), fq2_to_abi(f2(1)), fq2_to_abi(f2(0))])
    z = f2(1) if z is None else z
    z2 = f2_sqr(z)
    return np.concatenate([fq2_to_abi(f2_mul(p[0], z2)), fq2_to_abi(f2_mul(p[1], f2_mul(z2, z))), fq2_to_abi(z)])


def from_abi(a):
    """a (24,) Jacobian point as an affine model point (None: z == 0)"""
    a = np.asarray(a, dtype=np.uint64).reshape(24)
    x, y, z = fq2_from_abi(a[:8]), fq2_from_abi(a[8:16]), fq2_from_abi(a[16:])
    if z == (0, 0):
        return None
    zi = f2_inv(z)
    zi2 = f2_sqr(zi)
    return (f2_mul(x, zi2), f2_mul(y, f2_mul(zi2, zi)))
