"""GPU: the special cases of the limb-form mixed addition behind its `suspect` branch (fq_limb.hip.h: g1xl_add_mixed_common / g1xl_add_mixed_rare), reached through
the public entries -- the bucket sums of the fixed-base MSM (k_fx_buckets_ordered_staged, k_fx_heavy_segments_staged) and the one-hot sums over the L-form tables
(k_grid_onehot_sum).  Repeated bases with equal scalars put the same point into a bucket twice in a row (doubling), a base and its negative cancel (the accumulator
goes back to the identity in the middle of a list), an identity among the bases is a point at infinity in the tables, and negative digits make the first point of a
list a negated one.  Everything is compared with the oracle as group elements and in compressed form."""
import numpy as np
import pytest

import oracle_lib as O
from jolt_amd import ffi
from util import rand_fr

pytestmark = pytest.mark.gpu
R = O.R_MOD


@pytest.fixture(scope="module")
def ctx():
    c = ffi.Context(0)
    yield c
    c.close()


def same_point(a, b):
    return O.g1_eq(a, b) and O.g1_serialize_compressed(a) == O.g1_serialize_compressed(b)


def special_bases(n, seed):
    """n bases in groups of eight: P, P, -P, P, infinity, Q, -Q, Q"""
    host = O.srs_setup_from_secret(rand_fr(1, seed)[0], n)
    for g in range(0, n - 7, 8):
        p, q = host[g].copy(), host[g + 5].copy()
        host[g + 1], host[g + 2], host[g + 3] = p, O.g1_neg(p), p
        host[g + 4] = O.g1_identity()
        host[g + 6], host[g + 7] = O.g1_neg(q), q
    return host


@pytest.mark.parametrize("window_bits", [10, 13])
def test_fixed_base_bucket_sums_with_repeated_and_negated_bases(ctx, window_bits):
    n = 1024
    host = special_bases(n, 900 + window_bits)
    dev = ctx.srs_upload(host)
    ctx.srs_precompute_windows(dev, window_bits, 1)
    rng = np.random.default_rng(901)
    per_group = rand_fr(n // 8, 902)
    cases = {
        # one scalar per group of eight: every bucket that receives P receives P, -P, P, infinity in a row, then Q, -Q, Q
        "equal_in_group": np.repeat(per_group, 8, axis=0),
        # the same with the scalar's negative on the odd positions: negative digits, P - P + (-P)(-1) ... inside one bucket
        "alternating_sign": np.stack([per_group[i // 8] if i % 2 == 0 else O.to_mont([(R - O.from_mont(per_group[i // 8 : i // 8 + 1])[0]) % R])[0] for i in range(n)]),
        # few distinct scalars: long lists, each with many doublings and cancellations (the heavy segments at the narrow window)
        "few_scalars": rand_fr(4, 903)[rng.integers(0, 4, size=n)],
        # R - 1 everywhere: every digit negative or a carry, every list starts with a negated point
        "minus_one": np.repeat(O.to_mont([R - 1]), n, axis=0),
        "uniform": rand_fr(n, 904),
    }
    for name, scalars in cases.items():
        got = ctx.msm(dev, scalars)
        assert same_point(got, O.g1_msm_pippenger(host, scalars)), name
        assert O.g1_on_curve(got), name
    for m in (1, 2, 3, 5, 8, 9):  # lists of one and two points
        scalars = np.repeat(per_group[:1], m, axis=0)
        assert same_point(ctx.msm(dev, scalars), O.g1_msm_pippenger(host[:m], scalars)), m
    dev.free()


def test_onehot_sums_over_lform_tables_with_cold_cycles_and_special_bases(ctx):
    """2048 columns of 1024 cycles: one workgroup per column on a 256-CU part, i.e. a lane owns the cycles t, t + 256, t + 512, t + 768.  The SRS repeats a base at
    distance 256 and holds its negative at distance 512, so a lane meets the same point twice in a row, then its negative; cold cycles (known from the index byte) and an
    identity among the bases (a point at infinity in the tables) add nothing; columns that are cold at the lane's first cycles start their accumulator later."""
    K, T, N = 4, 1024, 2048
    host = O.srs_setup_from_secret(rand_fr(1, 910)[0], K * T)
    for a in range(K):
        for t in range(0, 64):
            base = host[a * T + t].copy()
            host[a * T + t + 256] = base
            host[a * T + t + 512] = O.g1_neg(base)
        host[a * T + 100] = O.g1_identity()
        host[a * T + 100 + 256] = O.g1_identity()
    srs = ctx.srs_upload(host)
    ctx.srs_precompute_windows(srs, 10, 1)
    rng = np.random.default_rng(911)
    idx = rng.integers(0, K, size=(N, T), dtype=np.uint8)
    idx[rng.random((N, T)) < 0.3] = 0xFF
    idx[0, :] = 0xFF                      # entirely cold: the identity
    idx[1, :] = 2                         # no cold cycle, one address: P, P, -P, then a fresh point in every one of the first 64 lanes
    idx[2, :] = 1
    idx[2, :512] = 0xFF                   # cold for the first two cycles of every lane
    idx[3, :] = 0xFF
    idx[3, 700] = 3                       # one hot cycle in the whole column
    idx[4, :] = 0
    idx[4, 256:512] = 0xFF                # P, cold, -P: back to the identity, then on
    got = ctx.grid_commit_onehot(srs, ctx.onehot(idx, K))
    check = [0, 1, 2, 3, 4] + [int(c) for c in rng.integers(5, N, size=12)]
    for p in check:
        want = O.g1_identity()
        for j in np.nonzero(idx[p] != 0xFF)[0]:
            want = O.g1_add(want, host[int(idx[p, j]) * T + int(j)])
        assert same_point(got[p], want), p
    assert O.g1_is_identity(got[0])
    srs.free()
