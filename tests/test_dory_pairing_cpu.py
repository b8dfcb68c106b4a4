"""The host build of the Dory multi-pairings (dory_pairing.hip, pairing.hip.h, fq12.hip.h): Fq12 as the kernels compute it against the flat big-integer field of
tests/pairing_model.py, and single and multi-pairings through the code the device lanes run (line tables, Miller accumulation) plus the host's final
exponentiation against the model's E^(sum k_i l_i).  Points are made through their discrete logarithms.  No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

import g2_model as M
import oracle_lib as O
import pairing_model as PM
from dory_groups import R, fr_int, rand_ints
from jolt_amd import ffi

Q = O.Q_MOD
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
NOT_CANONICAL_FQ = np.array(O.int_to_limbs(Q), dtype=np.uint64)
G2_IDENTITY = M.to_abi(None)


def g1(k, z=1):
    return PM.g1_to_abi(PM.g1_mul(k), z)


def g2(l, z=None):
    return M.to_abi(M.mul_generator(l), z)


def host_pairing(g1s, g2s):
    return PM.gt_from_abi(ffi.host_final_exponentiation(ffi.host_miller_loop(np.array(g1s).reshape(-1, 12), np.array(g2s).reshape(-1, 24))))


def test_generated_constants_are_current():
    assert subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_pairing_constants.py"), "--check"]).returncode == 0


def test_host_fq12_matches_the_model_at_the_corners():
    from corner_grids import fq12_grid
    operands, sparse = fq12_grid()
    assert len(operands) == 7 and operands[-1] == sparse
    abi = [PM.gt_to_abi(x) for x in operands]
    for x, X in zip(operands, abi):
        for y, Y in zip(operands, abi):
            assert PM.gt_from_abi(ffi.host_fq12_op(ffi.FQ12_MUL, X, Y)) == PM.f12_mul(x, y)
        assert PM.gt_from_abi(ffi.host_fq12_op(ffi.FQ12_MUL_SPARSE, X, abi[-1])) == PM.f12_mul(x, sparse)  # the line routine against the dense product
        assert PM.gt_from_abi(ffi.host_fq12_op(ffi.FQ12_SQR, X)) == PM.f12_sqr(x)
        assert PM.gt_from_abi(ffi.host_fq12_op(ffi.FQ12_CONJ, X)) == PM.f12_conj(x)
        if any(x):
            assert PM.gt_from_abi(ffi.host_fq12_op(ffi.FQ12_INV, X)) == PM.f12_inv(x)
    for x, X in zip(operands[1:], abi[1:]):  # the Frobenius maps as plain powers: p, p^2, p^3
        for e, op in ((1, ffi.FQ12_FROBENIUS1), (2, ffi.FQ12_FROBENIUS2), (3, ffi.FQ12_FROBENIUS3)):
            assert PM.gt_from_abi(ffi.host_fq12_op(op, X)) == PM.f12_pow(x, Q ** e), e
    assert np.array_equal(ffi.host_fq12_op(ffi.FQ12_MUL_SPARSE, abi[0], PM.gt_to_abi(PM.ONE)), abi[0])


def test_host_fq12_refusals():
    good = PM.gt_to_abi(list(range(1, 13)))
    with pytest.raises(ffi.JoltError) as e:
        ffi.host_fq12_op(ffi.FQ12_INV, PM.gt_to_abi(PM.ZERO))
    assert e.value.status == 11
    for coeff in (0, 5, 11):
        bad = good.copy()
        bad[4 * coeff:4 * coeff + 4] = NOT_CANONICAL_FQ
        for args in ((ffi.FQ12_MUL, bad, good), (ffi.FQ12_MUL, good, bad), (ffi.FQ12_SQR, bad), (ffi.FQ12_INV, bad), (ffi.FQ12_FROBENIUS1, bad)):
            with pytest.raises(ffi.JoltError) as e:
                ffi.host_fq12_op(*args)
            assert e.value.status == 1
        with pytest.raises(ffi.JoltError):
            ffi.host_final_exponentiation(bad)
    with pytest.raises(ffi.JoltError) as e:
        ffi.host_fq12_op(ffi.FQ12_MUL_SPARSE, good, good)  # not of the sparse shape
    assert e.value.status == 1


def test_prepared_lines_do_not_depend_on_the_representative():
    l = rand_ints(1, 7)[0]
    a, skip_a = ffi.host_g2_prepare_one(g2(l))
    b, skip_b = ffi.host_g2_prepare_one(g2(l, M.f2(11, 5)))
    assert np.array_equal(a, b) and not skip_a and not skip_b
    assert ffi.host_g2_prepare_one(G2_IDENTITY)[1]
    off = g2(l)
    off[1] ^= np.uint64(1)
    with pytest.raises(ffi.JoltError) as e:
        ffi.host_g2_prepare_one(off)
    assert e.value.status == 1


def test_single_pairing_matches_the_model():
    """G2 in a Jacobian representative of its own, the G1 point with Z != 1"""
    k, l = rand_ints(2, 8)
    got = host_pairing([g1(k, z=12345)], [g2(l, M.f2(3, 4))])
    assert got == PM.expected([k], [l])
    assert got == PM.pairing(PM.g1_mul(k), M.mul_generator(l))  # and the model's own Miller loop, not only its bilinearity
    assert PM.f12_pow(got, R) == PM.ONE and got != PM.ONE


def test_multi_pairing_matches_the_model():
    ks, ls = rand_ints(3, 9), rand_ints(3, 10)
    ks[1] = R - 1
    assert host_pairing([g1(k, z=i + 2) for i, k in enumerate(ks)], [g2(l, M.f2(i + 1, 7) if i else None) for i, l in enumerate(ls)]) == PM.expected(ks, ls)
    # a product that cancels to exactly one: e(kP, lQ) e(-kP, lQ), and e(kP, lQ) e(kP, -lQ) e(2kP, lQ) e(kP, -2lQ)
    assert host_pairing([g1(ks[0]), g1(-ks[0], z=9)], [g2(ls[0]), g2(ls[0])]) == PM.ONE
    assert host_pairing([g1(ks[0]), g1(ks[0]), g1(2 * ks[0]), g1(ks[0])], [g2(ls[0]), g2(-ls[0]), g2(ls[0]), g2(-2 * ls[0])]) == PM.ONE
    # the identity on either side contributes one; no pair gives one
    assert host_pairing([g1(0), g1(ks[1])], [g2(ls[0]), g2(ls[1])]) == PM.expected([ks[1]], [ls[1]])
    assert host_pairing([g1(ks[0]), g1(ks[1])], [G2_IDENTITY, g2(ls[1])]) == PM.expected([ks[1]], [ls[1]])
    assert host_pairing([g1(0)], [G2_IDENTITY]) == PM.ONE
    assert host_pairing([], []) == PM.ONE
    assert np.array_equal(ffi.host_miller_loop(np.zeros((0, 12), dtype=np.uint64), np.zeros((0, 24), dtype=np.uint64)), PM.gt_to_abi(PM.ONE))


def test_reference_pairing_properties():
    """crates/jolt-crypto/tests/pairing.rs:9-72: bilinearity both ways, identity gives one, multi = product of singles, single multi = pairing"""
    a, b = rand_ints(2, 11)
    P, Q2 = g1(1), g2(1)
    e = host_pairing([P], [Q2])
    assert host_pairing([g1(a)], [Q2]) == PM.f12_pow(e, a)
    assert host_pairing([P], [g2(b)]) == PM.f12_pow(e, b)
    assert host_pairing([g1(a)], [g2(b)]) == PM.f12_pow(e, a * b % R)
    assert host_pairing([g1(0)], [Q2]) == PM.ONE and host_pairing([P], [G2_IDENTITY]) == PM.ONE
    singles = PM.f12_mul(host_pairing([g1(a)], [g2(3)]), host_pairing([g1(5)], [g2(b)]))
    assert host_pairing([g1(a), g1(5)], [g2(3), g2(b)]) == singles
    assert e == PM.generator_pairing()


def test_gt_pow_against_the_model():
    E = PM.generator_pairing()
    X = PM.gt_to_abi(E)
    for k in (0, 1, 2, R - 1, R):  # a scalar is an element of Fr: r crosses the ABI as zero, and the model's plain r-th power agrees that this is one
        assert PM.gt_from_abi(ffi.host_gt_pow(X, fr_int(k))) == PM.f12_pow(E, k), k
    assert PM.gt_from_abi(ffi.host_gt_pow(X, fr_int(R))) == PM.ONE
    # r as an integer, through the library's own arithmetic: E^(r - 1) E = 1; the limbs of r themselves are not a canonical scalar and are refused
    assert PM.f12_mul(PM.gt_from_abi(ffi.host_gt_pow(X, fr_int(R - 1))), E) == PM.ONE
    with pytest.raises(ffi.JoltError) as e:
        ffi.host_gt_pow(X, np.array(O.int_to_limbs(R), dtype=np.uint64))
    assert e.value.status == 1


def test_host_miller_loop_refusals():
    P, Q2 = g1(3).reshape(1, 12), g2(4).reshape(1, 24)
    off = Q2.copy()
    off[0, 1] ^= np.uint64(1)
    bad = P.copy()
    bad[0, 0:4] = NOT_CANONICAL_FQ
    for a, b in ((P, off), (bad, Q2)):
        with pytest.raises(ffi.JoltError) as e:
            ffi.host_miller_loop(a, b)
        assert e.value.status == 1
