"""GPU parity: Dory's multi-pairings (dory_pairing.hip) -- jolt_dory_multi_pair, the prepared G2 tables and jolt_dory_multi_pair_g2_setup -- against the big-integer
pairing model of tests/pairing_model.py.  Points are made through their discrete logarithms (tests/dory_groups.py), so the expected value of every multi-pairing is
E^(sum k_i l_i mod r) with E the model's pairing of the two generators: one model pairing per session and one Fq12 power per check.  Results are compared bit for
bit as twelve canonical Fq.  The model's G2 generator is its own, not arkworks'; nothing on the checking side comes from the library."""
import ctypes as C

import numpy as np
import pytest

import g2_model as M
import oracle_lib as O
import pairing_model as PM
from dory_groups import G1, G2, R, plant, progression, rand_ints
from jolt_amd import ffi

pytestmark = pytest.mark.gpu
ONE = PM.gt_to_abi(PM.ONE)


@pytest.fixture(scope="module")
def ctx():
    c = ffi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pairs():
    """1000 pairs with their discrete logarithms, shared by the tests and never written: G1 points as the oracle's additions leave them (Z != 1), every third G2
    point in a Jacobian representative of its own"""
    k0, dk, l0, dl = rand_ints(4, 200)
    ks, g1s = progression(G1, k0, dk, 1000)
    ls, g2s = progression(G2, l0, dl, 1000)
    one_q = np.array(O.int_to_limbs(O.MONT_R % O.Q_MOD), dtype=np.uint64)
    assert sum(1 for p in g1s[:65] if not np.array_equal(p[8:12], one_q)) > 32  # most G1 points are not normalised
    return ks, g1s, ls, g2s


def want(ks, ls):
    return PM.gt_to_abi(PM.expected(ks, ls))


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 129, 1000])
def test_multi_pair_at_every_size(ctx, pairs, n):
    """none, one, a ragged and a full wavefront, a second and third workgroup, odd levels of the product tree (65, 129, 1000 -> 500 -> 250 -> 125 -> 63 ...)"""
    ks, g1s, ls, g2s = pairs
    got = ctx.dory_multi_pair(g1s[:n], g2s[:n])
    assert np.array_equal(got, want(ks[:n], ls[:n]))
    if n == 0:
        assert np.array_equal(got, ONE)


@pytest.fixture(scope="module")
def planted(pairs):
    ks, g1s, ls, g2s = pairs
    ks, g1s, ls, g2s = list(ks[:65]), g1s[:65].copy(), list(ls[:65]), g2s[:65].copy()
    plant(G1, ks, g1s, 0, 0)                # the identity in G1 at lane 0
    plant(G2, ls, g2s, 64, 0)               # the identity in G2 at lane 64, the only lane of the second wavefront
    plant(G1, ks, g1s, 7, R - 1)
    plant(G2, ls, g2s, 9, R - 1)
    ks[5], g1s[5], ls[5], g2s[5] = ks[4], g1s[4], ls[4], g2s[4]  # the same pair twice
    plant(G1, ks, g1s, 11, -ks[10])
    plant(G2, ls, g2s, 11, ls[10])          # a pair and its negation: lanes 10 and 11 multiply to one
    return ks, g1s, ls, g2s


def test_planted_elements(ctx, planted):
    ks, g1s, ls, g2s = planted
    assert np.array_equal(ctx.dory_multi_pair(g1s, g2s), want(ks, ls))
    assert np.array_equal(ctx.dory_multi_pair(g1s[10:12], g2s[10:12]), ONE)
    assert np.array_equal(ctx.dory_multi_pair(g1s[:1], g2s[:1]), ONE) and np.array_equal(ctx.dory_multi_pair(g1s[64:], g2s[64:]), ONE)


def test_raw_miller_product_is_the_host_functions(ctx, planted):
    """before the final exponentiation, bit for bit: the lanes and jolt_host_miller_loop run the same lines and the same accumulation, field arithmetic is exact, so
    the order of the product does not matter"""
    _, g1s, _, g2s = planted
    raw = ctx.dory_multi_pair(g1s, g2s, final_exponentiation=False)
    assert np.array_equal(raw, ffi.host_miller_loop(g1s, g2s))
    assert np.array_equal(ffi.host_final_exponentiation(raw), ctx.dory_multi_pair(g1s, g2s))


def test_prepared_bases(ctx, pairs):
    ks, g1s, ls, g2s = pairs
    prepared = ctx.dory_g2_prepare(g2s[:130])
    for n in (1, 64, 65, 130):
        got = ctx.dory_multi_pair_g2_setup(g1s[:n], prepared)
        assert np.array_equal(got, ctx.dory_multi_pair(g1s[:n], g2s[:n])), n
        assert np.array_equal(got, want(ks[:n], ls[:n])), n
        assert np.array_equal(got, ctx.dory_multi_pair_g2_setup(g1s[:n], prepared)), n  # the same call twice: the same bytes
    with pytest.raises(ffi.JoltError) as e:
        ctx.dory_multi_pair_g2_setup(g1s[:131], prepared)
    assert e.value.status == 1
    assert np.array_equal(ctx.dory_multi_pair_g2_setup(g1s[:0], prepared), ONE)
    prepared.free()
    again = ctx.dory_g2_prepare(g2s[100:230])  # freed, then prepared again (other points in the recycled block)
    assert np.array_equal(ctx.dory_multi_pair_g2_setup(g1s[:130], again), want(ks[:130], ls[100:230]))
    again.free()


def _raw(name, *args):
    conv = [a.ctypes.data_as(C.c_void_p) if isinstance(a, np.ndarray) else a for a in args]
    return getattr(ffi.lib(), name)(*conv)


def test_refusals_write_nothing_and_leave_the_context_usable(ctx, pairs):
    ks, g1s, ls, g2s = pairs
    n = 5
    g1s, g2s = g1s[:n].copy(), g2s[:n].copy()
    off_curve = g2s.copy()
    off_curve[4, 1] ^= np.uint64(1)
    not_canonical = g1s.copy()
    not_canonical[2, 0:4] = np.array(O.int_to_limbs(O.Q_MOD), dtype=np.uint64)
    sentinel = np.full(48, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    h, N = ctx.h, C.c_size_t(n)
    prepared = ctx.dory_g2_prepare(g2s)
    for a, b in ((g1s, off_curve), (not_canonical, g2s), (None, g2s), (g1s, None)):
        for name in ("jolt_dory_multi_pair", "jolt_dory_multi_miller"):
            out = sentinel.copy()
            assert _raw(name, h, a, b, N, out) == 1 and np.array_equal(out, sentinel)
    for a in (not_canonical, None):
        out = sentinel.copy()
        assert _raw("jolt_dory_multi_pair_g2_setup", h, a, prepared.h, N, out) == 1 and np.array_equal(out, sentinel)
    handle = C.c_void_p()
    assert _raw("jolt_dory_g2_prepare", h, off_curve, N, C.byref(handle)) == 1 and not handle.value
    assert _raw("jolt_dory_g2_prepare", h, None, N, C.byref(handle)) == 1 and not handle.value
    # the same context, valid calls
    assert np.array_equal(ctx.dory_multi_pair(g1s, g2s), want(ks[:n], ls[:n]))
    assert np.array_equal(ctx.dory_multi_pair_g2_setup(g1s, prepared), want(ks[:n], ls[:n]))
    prepared.free()


def test_dory_shaped_commitment(ctx, pairs):
    """tier 1 then tier 2 on this library: jolt_dory_commit_rows of a 64 x 64 matrix of u8 values, then multi_pair_g2_setup of its row commitments against prepared
    bases.  The G1 bases are g * beta^j (jolt_srs_setup_from_secret over the generator (1, 2)), so the whole commitment is E^(sum_i (sum_j v_ij beta^j) h_i)"""
    _, _, ls, g2s = pairs
    beta = rand_ints(1, 210)[0]
    srs = ctx.srs_setup_from_secret(O.to_mont([beta])[0], 64, O.g1_generator())
    values = np.random.default_rng(211).integers(0, 256, size=64 * 64, dtype=np.uint64)
    values[64:128] = 0  # a row that commits to the identity
    rows = ctx.dory_commit_rows(srs, ctx.ints(values), 64)
    assert rows.shape == (64, 12) and not rows[1, 8:12].any()
    powers = [pow(beta, j, R) for j in range(64)]
    row_logs = [sum(int(v) * b for v, b in zip(values[64 * i:64 * i + 64], powers)) % R for i in range(64)]
    prepared = ctx.dory_g2_prepare(g2s[:64])
    assert np.array_equal(ctx.dory_multi_pair_g2_setup(rows, prepared), want(row_logs, ls[:64]))
    prepared.free()
