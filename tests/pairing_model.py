"""A Python big-integer model of Fq12 and of the BN254 optimal ate pairing, for the Dory multi-pairing tests.  Independent of the library, in two layers.

Fq12 is ONE flat field here, Fq[w] / (w^12 - 18 w^6 + 82): w^6 = xi = 9 + u and u^2 = -1 give (w^6 - 9)^2 = -1.  The library's tower
Fq2[v] / (v^3 - xi), [w] / (w^2 - v) is the same field with the coefficient c_h.c_j = a + b u standing at w^(2 j + h): a w^k + b (w^6 - 9) w^k.

Layer (a), from the definition (pairing_definition): the G2 point untwisted to (x w^2, y w^3) on y^2 = x^3 + 3 over Fq12, chord-and-tangent lines with
every slope an Fq12 division, a Miller loop over the plain BITS of 6 z + 2, the two Frobenius steps with the Frobenius taken as the p-th power of each
coordinate, and the final power (p^12 - 1) / r * 2 z (6 z^2 + 3 z + 1) as one exponentiation.  Seconds per pairing.

Layer (b), what the tests use (pairing): the same loop with the point kept on the twist (g2_model), slopes in Fq2, the line embedded as the sparse element
y_P - lambda x_P w + (lambda x_T - y_T) w^3.  tests/test_pairing_model.py holds it to layer (a).

The generator of G2 is g2_model's own (the cofactor multiple of the first point found), not arkworks': bilinear checks do not care, a comparison of GT bytes
with a reference proof would.  The final power is the convention docs/parity.md calls unpinned by a reference vector.
"""
import numpy as np

import g2_model as M
from oracle_lib import MONT_R, Q_MOD, R_MOD, int_to_limbs, limbs_to_int

Q, R = Q_MOD, R_MOD
Z = 4965661367192848881
LOOP = 6 * Z + 2
assert Q == 36 * Z**4 + 36 * Z**3 + 24 * Z**2 + 6 * Z + 1 and R == 36 * Z**4 + 36 * Z**3 + 18 * Z**2 + 6 * Z + 1
FINAL_POWER = (Q**12 - 1) // R * (2 * Z * (6 * Z * Z + 3 * Z + 1))

# ---------------------------------------------------------------- Fq12: lists of 12 integers below q, index = power of w
ZERO = [0] * 12
ONE = [1] + [0] * 11


def f12(coeffs):
    """{power of w: integer} -> element"""
    out = [0] * 12
    for k, v in coeffs.items():
        out[k] = v % Q
    return out


def f12_add(a, b): return [(x + y) % Q for x, y in zip(a, b)]
def f12_sub(a, b): return [(x - y) % Q for x, y in zip(a, b)]
def f12_neg(a): return [-x % Q for x in a]


def f12_mul(a, b):
    t = [0] * 23
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                t[i + j] += x * y
    for k in range(22, 11, -1):  # w^12 = 18 w^6 - 82
        c = t[k]
        if c:
            t[k - 6] += 18 * c
            t[k - 12] -= 82 * c
    return [v % Q for v in t[:12]]


def f12_sqr(a): return f12_mul(a, a)


def f12_pow(a, e):
    acc = ONE
    for bit in bin(e)[2:] if e else "":
        acc = f12_sqr(acc)
        if bit == "1":
            acc = f12_mul(acc, a)
    return acc


def f12_conj(a):
    """the p^6-th power: w -> -w"""
    return [(-x % Q) if k & 1 else x for k, x in enumerate(a)]


def _poly_trim(a):
    while a and a[-1] == 0:
        a.pop()
    return a


def _poly_divmod(a, b):
    a, quo = list(a), [0] * max(len(a) - len(b) + 1, 1)
    lead = pow(b[-1], -1, Q)
    while len(a) >= len(b):
        c, s = a[-1] * lead % Q, len(a) - len(b)
        quo[s] = c
        for i, y in enumerate(b):
            a[s + i] = (a[s + i] - c * y) % Q
        _poly_trim(a)
    return _poly_trim(quo), a


def f12_inv(a):
    """extended Euclid on polynomials over Fq against w^12 - 18 w^6 + 82; raises for zero"""
    if not any(a):
        raise ZeroDivisionError("0 has no inverse in Fq12")
    modulus = [82] + [0] * 5 + [Q - 18] + [0] * 5 + [1]
    r0, r1, s0, s1 = modulus, _poly_trim(list(a)), [], [1]
    while r1:
        quo, rem = _poly_divmod(r0, r1)
        prod = [0] * (len(quo) + len(s1))
        for i, x in enumerate(quo):
            for j, y in enumerate(s1):
                prod[i + j] += x * y
        nxt = [((s0[i] if i < len(s0) else 0) - prod[i]) % Q for i in range(max(len(s0), len(prod)))]
        r0, r1, s0, s1 = r1, rem, s1, _poly_trim(nxt)
    c = pow(r0[0], -1, Q)  # the gcd is a non-zero constant
    out = [x * c % Q for x in s0]
    return out + [0] * (12 - len(out))


def f12_from_fq2(a, k=0):
    """(a0 + a1 u) w^k, k < 6"""
    out = [0] * 12
    out[k], out[k + 6] = (a[0] - 9 * a[1]) % Q, a[1] % Q
    return out


# ---------------------------------------------------------------- the library's jolt_gt_t: 12 Montgomery Fq, c_h.c_j at index 6 h + 2 j (+ 1 for the u part)
_RINV = pow(MONT_R, -1, Q)


def gt_to_abi(a):
    out = np.zeros(48, dtype=np.uint64)
    for k in range(6):
        b = a[k + 6]
        pos = 6 * (k & 1) + 2 * (k >> 1)
        out[4 * pos:4 * pos + 4] = int_to_limbs((a[k] + 9 * b) % Q * MONT_R % Q)
        out[4 * pos + 4:4 * pos + 8] = int_to_limbs(b * MONT_R % Q)
    return out


def gt_from_abi(arr):
    arr = np.asarray(arr, dtype=np.uint64).reshape(12, 4)
    out = [0] * 12
    for k in range(6):
        pos = 6 * (k & 1) + 2 * (k >> 1)
        c0, c1 = limbs_to_int(arr[pos]) * _RINV % Q, limbs_to_int(arr[pos + 1]) * _RINV % Q
        out[k], out[k + 6] = (c0 - 9 * c1) % Q, c1
    return out


# ---------------------------------------------------------------- layer (a): the definition, over E(Fq12): y^2 = x^3 + 3, affine, identity = None
def _e12_slope_line(t, s, p):
    """(t + s, the line through t and s at p); t, s affine points over Fq12 with t != -s"""
    if t[0] == s[0]:
        lam = f12_mul(f12_mul(f12({0: 3}), f12_sqr(t[0])), f12_inv(f12_add(t[1], t[1])))
    else:
        lam = f12_mul(f12_sub(s[1], t[1]), f12_inv(f12_sub(s[0], t[0])))
    x = f12_sub(f12_sub(f12_sqr(lam), t[0]), s[0])
    y = f12_sub(f12_mul(lam, f12_sub(t[0], x)), t[1])
    line = f12_sub(f12_sub(p[1], t[1]), f12_mul(lam, f12_sub(p[0], t[0])))
    return (x, y), line


def untwist(q):
    return (f12_from_fq2(q[0], 2), f12_from_fq2(q[1], 3))


def miller_definition(p, q):
    """f_{6z+2,Q}(P) l_{[6z+2]Q, pi(Q)}(P) l_{[6z+2]Q + pi(Q), -pi^2(Q)}(P); p = (x, y) integers, q a g2_model point, neither the identity"""
    p12 = (f12({0: p[0]}), f12({0: p[1]}))
    q12 = untwist(q)
    assert f12_sqr(q12[1]) == f12_add(f12_mul(f12_sqr(q12[0]), q12[0]), f12({0: 3}))
    t, f = q12, ONE
    for bit in bin(LOOP)[3:]:
        t, line = _e12_slope_line(t, t, p12)
        f = f12_mul(f12_sqr(f), line)
        if bit == "1":
            t, line = _e12_slope_line(t, q12, p12)
            f = f12_mul(f, line)
    q1 = (f12_pow(q12[0], Q), f12_pow(q12[1], Q))
    q2 = (f12_pow(q1[0], Q), f12_neg(f12_pow(q1[1], Q)))
    t, line = _e12_slope_line(t, q1, p12)
    f = f12_mul(f, line)
    t, line = _e12_slope_line(t, q2, p12)
    return f12_mul(f, line)


def pairing_definition(p, q):
    return f12_pow(miller_definition(p, q), FINAL_POWER)


# ---------------------------------------------------------------- layer (b): on the twist, slopes in Fq2
def _f2_pow(a, e):
    acc = M.f2(1)
    for bit in bin(e)[2:]:
        acc = M.f2_sqr(acc)
        if bit == "1":
            acc = M.f2_mul(acc, a)
    return acc


_XI = M.f2(9, 1)
_G12, _G13 = _f2_pow(_XI, (Q - 1) // 3), _f2_pow(_XI, (Q - 1) // 2)
_G22, _G23 = _f2_pow(_XI, (Q * Q - 1) // 3), _f2_pow(_XI, (Q * Q - 1) // 2)


def _conj2(a): return (a[0], -a[1] % Q)


def _twist_line(t, s, p):
    """(t + s on the twist, the line through their untwisted images at p = (x, y) in Fq)"""
    if t == s:
        lam = M.f2_mul(M.f2_mul(M.f2(3), M.f2_sqr(t[0])), M.f2_inv(M.f2_add(t[1], t[1])))
    else:
        lam = M.f2_mul(M.f2_sub(s[1], t[1]), M.f2_inv(M.f2_sub(s[0], t[0])))
    line = f12_add(f12({0: p[1]}), f12_add(f12_from_fq2(M.f2_neg(M.f2_mul(lam, M.f2(p[0]))), 1), f12_from_fq2(M.f2_sub(M.f2_mul(lam, t[0]), t[1]), 3)))
    return M.add(t, s), line


def miller(p, q):
    t, f = q, ONE
    for bit in bin(LOOP)[3:]:
        t, line = _twist_line(t, t, p)
        f = f12_mul(f12_sqr(f), line)
        if bit == "1":
            t, line = _twist_line(t, q, p)
            f = f12_mul(f, line)
    q1 = (M.f2_mul(_conj2(q[0]), _G12), M.f2_mul(_conj2(q[1]), _G13))
    q2 = (M.f2_mul(q[0], _G22), M.f2_neg(M.f2_mul(q[1], _G23)))
    t, line = _twist_line(t, q1, p)
    f = f12_mul(f, line)
    t, line = _twist_line(t, q2, p)
    return f12_mul(f, line)


def final_exponentiation(f):
    return f12_pow(f, FINAL_POWER)


def pairing(p, q):
    """e(P, Q); one when either side is the identity (None)"""
    if p is None or q is None:
        return ONE
    return final_exponentiation(miller(p, q))


G1_GENERATOR = (1, 2)
_E = []


def generator_pairing():
    """E = e((1, 2), g2_model.GENERATOR), computed once per process"""
    if not _E:
        _E.append(pairing(G1_GENERATOR, M.GENERATOR))
    return _E[0]


def expected(ks, ls):
    """prod_i e(k_i G1, l_i G2) = E^(sum k_i l_i mod r)"""
    return f12_pow(generator_pairing(), sum(k * l for k, l in zip(ks, ls)) % R)


# ---------------------------------------------------------------- G1 for the tests: affine (x, y) integers on y^2 = x^3 + 3, identity = None
def g1_add(p, s):
    if p is None:
        return s
    if s is None:
        return p
    if p[0] == s[0]:
        if (p[1] + s[1]) % Q == 0:
            return None
        lam = 3 * p[0] * p[0] * pow(2 * p[1], -1, Q) % Q
    else:
        lam = (s[1] - p[1]) * pow(s[0] - p[0], -1, Q) % Q
    x = (lam * lam - p[0] - s[0]) % Q
    return (x, (lam * (p[0] - x) - p[1]) % Q)


def g1_mul(k):
    """(k mod r) * (1, 2)"""
    acc = None
    for bit in bin(k % R)[2:] if k % R else "":
        acc = g1_add(acc, acc)
        if bit == "1":
            acc = g1_add(acc, G1_GENERATOR)
    return acc


def g1_to_abi(p, z=1):
    """p as the library's Jacobian point (12,) uint64 in the representative (x z^2, y z^3, z); the identity is (1, 1, 0)"""
    coords = (1, 1, 0) if p is None else (p[0] * z * z, p[1] * z * z * z, z)
    return np.array([limb for c in coords for limb in int_to_limbs(c % Q * MONT_R % Q)], dtype=np.uint64)
