"""GPU parity of the opening whose three witness commitments come from ONE digit sort (hyperkzg.hip: Q3 = B div (X^2 - r^2)(X - r^2), three bucket passes against the
bases shifted by 0, 1, 2, combined on the host) against the oracle's proof, point for point.  The shapes are the ones where the three passes can go wrong and that
the other opening tests (10-13-bit windows) never reach: bucket sets of at least 2^16 put the row / column reduction on, and with it the alternation of the two
bucket sets over three passes with the reductions on the auxiliary stream."""
import numpy as np
import pytest

import oracle_lib as O
from jolt_amd import ffi
from util import rand_challenge, rand_fr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = ffi.Context(0)
    yield c
    c.close()


def same_point(a, b):
    return O.g1_eq(a, b) and O.g1_serialize_compressed(a) == O.g1_serialize_compressed(b)


def five_values(n, seed):
    """64-bit coefficients with many repeats: heavy buckets in every pass, and scalars that are not uniform behind a sort told that they are"""
    return O.fr_from_u64(np.random.default_rng(seed).integers(0, 5, size=n).astype(np.uint64) * np.uint64(0x0123456789ABCDEF))


def first_three(n, seed):
    """zero except the first three evaluations: B has degree <= 2, so Q3 = 0 and every pass returns the identity"""
    e = np.zeros((n, 4), dtype=np.uint64)
    e[:3] = rand_fr(3, seed)
    return e


MAX_ELL = 16


@pytest.fixture(scope="module")
def srs_points(ctx):
    """2^16 + 1 powers of one secret, made once (on the device: the oracle's repeated scalar multiplication takes tens of seconds at this length, and
    test_gpu_msm.py holds the device's setup to it) and shared: every case opens against a prefix, and the oracle commits to the same points"""
    dev = ctx.srs_setup_from_secret(rand_fr(1, 1100)[0], (1 << MAX_ELL) + 1, O.g1_generator())
    pts = dev.download()
    dev.free()
    return pts


def open_both(ctx, srs, srs_host, evals, ell, label):
    point = np.stack([rand_challenge(1130 + k) for k in range(ell)])
    tab = ctx.upload(evals)
    got = ctx.hyperkzg_open(srs, tab, point, label=label)
    tab.free()
    return got, O.hyperkzg_open(srs_host, evals, point, label=label)


def assert_same_proof(got, want, ell, tag):
    assert np.array_equal(got["challenges"], want["challenges"]), tag
    assert np.array_equal(got["v"], want["v"]), tag
    for i in range(ell - 1):
        assert same_point(got["com"][i], want["com"][i]), (tag, i)
    for t in range(3):
        assert same_point(got["w"][t], want["w"][t]), (tag, t)


CASES = [
    # ell, window_bits, evaluations
    (2, 17, "random"),   # B of 4 coefficients: Q3 has one
    (3, 17, "random"),
    (7, 17, "random"),
    (12, 17, "random"),
    (12, 17, "five"),    # heavy buckets under all three passes
    (16, 17, "random"),
    (7, 17, "three"),    # Q3 = 0: the identity from every pass, the witnesses from the remainder terms alone
]
# (The capacity-region sort needs the split entries, that is at most 13 windows, and 2^16 terms: 15 windows of 17 bits over 2^16 - 3 terms sort exactly.  Its outputs are
# read-only for the passes either way; the 2^26-coefficient opening of test_gpu_pcs.py runs the three passes behind it.)


@pytest.mark.parametrize("ell,window_bits,kind", CASES)
def test_open_with_three_passes_over_one_sort_is_the_oracle_proof(ctx, srs_points, ell, window_bits, kind):
    n = 1 << ell
    srs_host = srs_points[: n + 1]
    srs = ctx.srs_upload(srs_host)
    ctx.srs_precompute_windows(srs, window_bits, 1)  # min_terms = 1: every MSM of the opening on the tables; >= 17-bit windows: the row / column reduction
    evals = {"random": rand_fr, "five": five_values, "three": first_three}[kind](n, 1110 + ell)
    got, want = open_both(ctx, srs, srs_host, evals, ell, 21)
    assert_same_proof(got, want, ell, (ell, window_bits, kind))
    srs.free()


def test_repeated_opening_returns_the_same_bytes(ctx, srs_points):
    """the same opening three times on one context: a pass that read a bucket set before its memset, or a reduction still in flight when its set or scratch is taken
    again, shows as a different point"""
    ell = 12
    srs_host = srs_points[: (1 << ell) + 1]
    srs = ctx.srs_upload(srs_host)
    ctx.srs_precompute_windows(srs, 17, 1)
    evals = rand_fr(1 << ell, 1150)
    got, want = open_both(ctx, srs, srs_host, evals, ell, 22)
    assert_same_proof(got, want, ell, "first")
    first = [O.g1_serialize_compressed(p) for p in list(got["w"]) + list(got["com"])]
    point = np.stack([rand_challenge(1130 + k) for k in range(ell)])
    for rep in range(2):
        tab = ctx.upload(evals)
        again = ctx.hyperkzg_open(srs, tab, point, label=22)
        tab.free()
        assert [O.g1_serialize_compressed(p) for p in list(again["w"]) + list(again["com"])] == first, rep
        assert np.array_equal(again["v"], got["v"]) and np.array_equal(again["challenges"], got["challenges"])
    srs.free()


def test_short_and_tableless_openings_keep_the_plain_path(ctx, srs_points):
    """ell = 1 (B of two coefficients) under window tables, and an SRS without tables (the family answers UNSUPPORTED, nothing enqueued): three witness polynomials,
    three MSMs, the oracle's proof"""
    srs_host = srs_points[:3]
    srs = ctx.srs_upload(srs_host)
    ctx.srs_precompute_windows(srs, 17, 1)
    got, want = open_both(ctx, srs, srs_host, rand_fr(2, 1160), 1, 23)
    assert_same_proof(got, want, 1, "ell = 1")
    srs.free()
    for ell in (2, 7):
        srs_host = srs_points[: (1 << ell) + 1]
        srs = ctx.srs_upload(srs_host)
        got, want = open_both(ctx, srs, srs_host, rand_fr(1 << ell, 1170 + ell), ell, 24)
        assert_same_proof(got, want, ell, ("no tables", ell))
        srs.free()
