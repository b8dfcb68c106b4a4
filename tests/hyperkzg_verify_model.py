"""HyperKZG verification in plain Python integers modulo r: an executable reading of crates/jolt-hyperkzg/src/scheme.rs:162-242 and kzg.rs:132-210, and a log-space
HyperKZG to hold it against.

In log space a G1 point is its discrete logarithm to g1 (g1 itself is 1), so the commitment of a polynomial p under the SRS (beta^i g1) is p(beta) mod r, and with g2 = 1
and beta g2 = beta the pairing check e(L, g2) = e(R, beta g2) reads L == beta * R (mod r).  Everything the verifier computes in Fr is computed here as the reference
writes it; nothing is taken from the library.
"""
R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001


def eval_univariate(coeffs, u):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * u + c) % R
    return acc


# ---- the verifier (scheme.rs:162-242, kzg.rs:132-210) ----
def folding_check(point, claimed_eval, v, r):
    """scheme.rs:203-234 -> the first failing level, or None"""
    ell = len(point)
    y_sq = list(v[2]) + [claimed_eval]
    for level in range(ell):
        y_next, y_pos, y_neg, x = y_sq[level + 1], v[0][level], v[1][level], point[ell - 1 - level]
        lhs = 2 * r * y_next % R
        rhs = (r * (1 - x) * (y_pos + y_neg) + x * (y_pos - y_neg)) % R
        if lhs != rhs:
            return level
    return None


def verify_scalars(v, r, q, d0):
    """kzg.rs:159-205 -> (the k + 4 scalars of L over [C_0 .. C_{k-1}, W_0, W_1, W_2, g1], (d_0, d_1))"""
    k = len(v[0])
    d1 = d0 * d0 % R
    q_powers = [pow(q, j, R) for j in range(k)]
    mult = (1 + d0 + d1) % R
    b_u = [sum(a * b for a, b in zip(row, q_powers)) % R for row in v]
    u = [r, -r % R, r * r % R]
    scalars = [qp * mult % R for qp in q_powers] + [u[0], u[1] * d0 % R, u[2] * d1 % R, -(b_u[0] + d0 * b_u[1] + d1 * b_u[2]) % R]
    return scalars, (d0, d1)


def verify(beta, commitments, commitment_scalars, point, claimed_eval, proof, challenges):
    """HyperKZGScheme::verify over log-space points, with C_0 = sum_i s_i commitments[i] (scheme.rs:346-352) entering L term by term.
    -> (accepted, failed_check, failed_level): failed_check 0 none, 1 the folding check, 2 the pairing check"""
    r, q, d0 = challenges
    ell = len(point)
    assert ell >= 1 and len(proof["com"]) == ell - 1 and all(len(row) == ell for row in proof["v"]) and r % R != 0
    level = folding_check(point, claimed_eval, proof["v"], r)
    if level is not None:
        return False, 1, level
    scalars, (d0, d1) = verify_scalars(proof["v"], r, q, d0)
    bases = [c for c in commitments] + list(proof["com"]) + list(proof["w"]) + [1]
    coeffs = [s * scalars[0] % R for s in commitment_scalars] + scalars[1:]
    assert len(bases) == len(coeffs) == len(commitments) + ell - 1 + 4
    lhs = sum(b * c for b, c in zip(bases, coeffs)) % R
    rhs = (proof["w"][0] + d0 * proof["w"][1] + d1 * proof["w"][2]) % R
    return (True, 0, 0) if lhs == beta * rhs % R else (False, 2, 0)


# ---- a log-space prover (scheme.rs:88-158, kzg.rs:34-126) ----
def fold_polynomials(evals, point):
    polys = [list(evals)]
    for xi in reversed(point[1:]):
        prev = polys[-1]
        polys.append([(prev[2 * j] + xi * (prev[2 * j + 1] - prev[2 * j])) % R for j in range(len(prev) // 2)])
    return polys


def witness_polynomial(f, u):
    """kzg.rs:34-46: the quotient of f by (X - u)"""
    d = len(f)
    h = [0] * (d - 1)
    if d > 1:
        h[d - 2] = f[d - 1]
        for i in range(d - 2, 0, -1):
            h[i - 1] = (f[i] + h[i] * u) % R
    return h


def commit(beta, coeffs):
    return eval_univariate(coeffs, beta)


def multilinear_eval(evals, point):
    """the value the claim is about: the last fold by point[0]"""
    last = fold_polynomials(evals, point)[-1]
    return (last[0] + point[0] * (last[1] - last[0])) % R


def open_(beta, evals, point, challenges):
    """HyperKZGScheme::open in log space under GIVEN challenges (r, q, d_0) -> dict(com, w, v)"""
    r, q, _ = challenges
    ell = len(point)
    assert len(evals) == 1 << ell
    polys = fold_polynomials(evals, point)
    com = [commit(beta, p) for p in polys[1:]]
    u = [r, -r % R, r * r % R]
    v = [[eval_univariate(p, ui) for p in polys] for ui in u]
    b_poly = [0] * len(polys[0])
    for j, p in enumerate(polys):
        qj = pow(q, j, R)
        for i, c in enumerate(p):
            b_poly[i] = (b_poly[i] + qj * c) % R
    w = [commit(beta, witness_polynomial(b_poly, ui)) for ui in u]
    return dict(com=com, w=w, v=v)
