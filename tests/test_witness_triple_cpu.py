"""The combination that turns commit(X^k Q3), k = 0, 1, 2, into the three witness commitments of a HyperKZG opening (hyperkzg.hip witness_triple_combine, exported
for the host as jolt_host_hyperkzg_witness_triple) against the oracle's three independent commitments (kzg.rs:108-116).  Everything that goes in -- q, Q3, a, alpha,
C0..C2 -- is computed with the oracle's own functions; the results are compared as compressed points.  No GPU."""
import numpy as np
import pytest

import oracle_lib as O
from jolt_amd import ffi
from util import rand_challenge, rand_fr

ZERO = np.zeros(4, dtype=np.uint64)


def _m(a, b):
    return O.fr_mul(np.asarray(a).reshape(1, 4), np.asarray(b).reshape(1, 4))[0]


def _a(a, b):
    return O.fr_add(np.asarray(a).reshape(1, 4), np.asarray(b).reshape(1, 4))[0]


def _neg(a):
    return O.fr_neg(np.asarray(a).reshape(1, 4))[0]


def triple_inputs(b_poly, r, srs):
    """u = r^2; q = B div (X^2 - u) as two linear divisions, alpha its X^1 remainder; Q3 = q div (X - u), a = q(u); C_k = commit(Q3) against the bases from G_k on"""
    u = _m(r, r)
    h_r = O.kzg_witness_polynomial(b_poly, r)
    q = O.kzg_witness_polynomial(h_r, _neg(r))
    alpha = _a(h_r[0], _m(q[0], _neg(r)))
    q3 = O.kzg_witness_polynomial(q, u)
    a = _a(q[0], _m(u, q3[0]))
    assert np.array_equal(a, O.kzg_eval_univariate(q, u))
    assert len(q3) == len(b_poly) - 3
    c = np.stack([O.kzg_commit(q3, srs[k:]) for k in range(3)])
    return c, a, alpha


def want_witnesses(b_poly, r, srs):
    return [O.kzg_commit(O.kzg_witness_polynomial(b_poly, x), srs) for x in (r, _neg(r), _m(r, r))]


def challenge_points():
    one = O.to_mont([1])[0]
    return [("random", rand_fr(1, 905)[0]), ("challenge", rand_challenge(906)), ("zero", ZERO.copy()), ("one", one)]


@pytest.fixture(scope="module")
def srs():
    return O.srs_setup_from_secret(rand_fr(1, 900)[0], 65)  # len + 1 points for the longest case; shorter cases use a prefix


@pytest.mark.parametrize("length", [4, 8, 64])
def test_triple_is_the_oracles_three_commitments(srs, length):
    s = srs[: length + 1]
    b_poly = rand_fr(length, 910 + length)
    for name, r in challenge_points():
        c, a, alpha = triple_inputs(b_poly, r, s)
        got = ffi.host_hyperkzg_witness_triple(c, s[0], s[1], r, a, alpha)
        for t, want in enumerate(want_witnesses(b_poly, r, s)):
            assert O.g1_serialize_compressed(got[t]) == O.g1_serialize_compressed(want), (length, name, t)


@pytest.mark.parametrize("length", [4, 8, 64])
def test_zero_quotient_leaves_the_remainder_terms(srs, length):
    """B of degree <= 2: Q3 = 0, every C_k is the identity and the witnesses are a (G_1 + x G_0) + alpha G_0 alone"""
    s = srs[: length + 1]
    b_poly = np.zeros((length, 4), dtype=np.uint64)
    b_poly[:3] = rand_fr(3, 930 + length)
    for name, r in challenge_points():
        c, a, alpha = triple_inputs(b_poly, r, s)
        assert all(O.g1_is_identity(c[k]) for k in range(3))
        got = ffi.host_hyperkzg_witness_triple(c, s[0], s[1], r, a, alpha)
        for t, want in enumerate(want_witnesses(b_poly, r, s)):
            assert O.g1_serialize_compressed(got[t]) == O.g1_serialize_compressed(want), (length, name, t)


def test_a_wrong_remainder_changes_the_witness_at_r_squared(srs):
    s = srs[:9]
    b_poly = rand_fr(8, 950)
    r = rand_fr(1, 951)[0]
    c, a, alpha = triple_inputs(b_poly, r, s)
    want = want_witnesses(b_poly, r, s)
    wrong = ffi.host_hyperkzg_witness_triple(c, s[0], s[1], r, _a(a, O.to_mont([1])[0]), alpha)
    assert O.g1_serialize_compressed(wrong[2]) != O.g1_serialize_compressed(want[2])
    wrong_alpha = ffi.host_hyperkzg_witness_triple(c, s[0], s[1], r, a, _a(alpha, O.to_mont([1])[0]))
    assert all(O.g1_serialize_compressed(wrong_alpha[t]) != O.g1_serialize_compressed(want[t]) for t in range(3))


def test_refuses_what_is_not_a_point_or_a_field_element(srs):
    s = srs[:9]
    c, a, alpha = triple_inputs(rand_fr(8, 960), rand_fr(1, 961)[0], s)
    r = rand_fr(1, 961)[0]
    off = c.copy()
    off[1, 0] ^= np.uint64(1)  # X of C1 moved off the curve
    with pytest.raises(ffi.JoltError) as e:
        ffi.host_hyperkzg_witness_triple(off, s[0], s[1], r, a, alpha)
    assert e.value.status == 1
    with pytest.raises(ffi.JoltError) as e:
        ffi.host_hyperkzg_witness_triple(c, s[0], s[1], np.full(4, 2**64 - 1, dtype=np.uint64), a, alpha)
    assert e.value.status == 1


def test_library_exports_the_entry_point():
    assert hasattr(ffi.lib(), "jolt_host_hyperkzg_witness_triple")
