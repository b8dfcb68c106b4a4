"""The two identities behind the opening's first pass (hyperkzg.hip, open_level_heads), in the oracle's field arithmetic against the oracle's own evaluations.

With mu = r^2 and P_j(X) = E_j(X^2) + X O_j(X^2), the chunk heads of the quotient scan over level j (Horner values of a chunk's even and of its odd coefficients
at mu, zero carry-in) sum, by the chunk-level Horner in mu^chunk, to E_j(mu) and O_j(mu), so
    v[0][j] = P_j(r) = E_j + r O_j,   v[1][j] = P_j(-r) = E_j - r O_j,
and level j being the fold of level j - 1 by x_j = point[ell - j],
    v[2][j] = P_j(mu) = (1 - x_j) E_(j-1)(mu) + x_j O_(j-1)(mu)   for j >= 1;
only P_0(mu) needs a sum of its own (a third chain over the chunk's plain coefficients, chunks weighed with mu^(2 chunk)).  Heads are linear, so the heads of
B = sum_j q^j P_j are the same combination of the levels' heads.  The chunk here is smaller than the polynomial: several chunks, partial chunks on the short levels."""
import numpy as np
import pytest

import oracle_lib as O
from util import rand_fr

ZERO, ONE = O.to_mont([0])[0], O.to_mont([1])[0]


def mul(a, b):
    return O.fr_mul(a, b)[0]


def add(a, b):
    return O.fr_add(a, b)[0]


def sub(a, b):
    return O.fr_sub(a, b)[0]


def power(a, e):
    out = ONE
    for _ in range(e):
        out = mul(out, a)
    return out


def level_heads(level, mu, chunk, third):
    """per chunk of `chunk` positions of both chains: (even head, odd head, plain Horner value of the chunk's 2 * chunk coefficients or zero)"""
    positions = level.shape[0] // 2
    out = []
    for lo in range(0, positions, chunk):
        e = o = t = ZERO
        for k in reversed(range(lo, min(lo + chunk, positions))):
            e = add(mul(e, mu), level[2 * k])
            o = add(mul(o, mu), level[2 * k + 1])
            if third:
                t = add(mul(add(mul(t, mu), level[2 * k + 1]), mu), level[2 * k])
        out.append((e, o, t))
    return out


def chunk_horner(values, w):
    acc = ZERO
    for v in reversed(values):
        acc = add(mul(acc, w), v)
    return acc


def evaluations_from_heads(levels, point, r, chunk):
    ell = len(levels)
    mu = mul(r, r)
    w, w_plain = power(mu, chunk), power(mu, 2 * chunk)
    tot = []
    for j, level in enumerate(levels):
        h = level_heads(level, mu, chunk, third=j == 0)
        tot.append((chunk_horner([c[0] for c in h], w), chunk_horner([c[1] for c in h], w), chunk_horner([c[2] for c in h], w_plain)))
    v = np.zeros((3, ell, 4), dtype=np.uint64)
    for j in range(ell):
        e, o, _ = tot[j]
        v[0, j] = add(e, mul(r, o))
        v[1, j] = sub(e, mul(r, o))
        if j == 0:
            v[2, j] = tot[0][2]
        else:
            x = point[ell - j]
            pe, po, _ = tot[j - 1]
            v[2, j] = add(mul(sub(ONE, x), pe), mul(x, po))
    return v


def challenge(kind, seed):
    return {"zero": ZERO, "one": ONE}.get(kind, rand_fr(1, seed)[0])


@pytest.mark.parametrize("chunk", [1, 2])
@pytest.mark.parametrize("kind", ["random", "zero", "one"])
@pytest.mark.parametrize("ell", [2, 3, 4, 5, 6])
def test_evaluations_from_chunk_heads_are_the_oracles(ell, kind, chunk):
    evals, point = rand_fr(1 << ell, 2100 + ell), rand_fr(ell, 2110 + ell)
    levels = O.hyperkzg_fold_polynomials(evals, point)
    r = challenge(kind, 2120 + ell)
    u = [r, O.fr_neg(r)[0], mul(r, r)]
    want = np.stack([np.stack([O.kzg_eval_univariate(level, u[t]) for level in levels]) for t in range(3)])
    got = evaluations_from_heads(levels, point, r, chunk)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("kind", ["random", "zero"])
@pytest.mark.parametrize("ell", [2, 4, 6])
def test_heads_of_the_combination_are_the_combination_of_the_heads(ell, kind):
    chunk = 2
    evals, point = rand_fr(1 << ell, 2130 + ell), rand_fr(ell, 2140 + ell)
    levels = O.hyperkzg_fold_polynomials(evals, point)
    mu, q = rand_fr(1, 2150 + ell)[0], challenge(kind, 2160 + ell)
    B, qj = np.zeros_like(levels[0]), ONE
    combined = [[ZERO, ZERO] for _ in range(0, levels[0].shape[0] // 2, chunk)]
    for level in levels:
        B[: level.shape[0]] = O.fr_add(B[: level.shape[0]], O.fr_mul(level, np.tile(qj, (level.shape[0], 1))))
        for c, (e, o, _) in enumerate(level_heads(level, mu, chunk, third=False)):
            combined[c] = [add(combined[c][0], mul(qj, e)), add(combined[c][1], mul(qj, o))]
        qj = mul(qj, q)
    want = level_heads(B, mu, chunk, third=False)
    assert all(np.array_equal(combined[c][l], want[c][l]) for c in range(len(want)) for l in range(2))
