"""GPU: the one-hot sums of bases over the commitment grid's pair tables (jolt_srs_precompute_grid_pairs, k_grid_onehot_sum_pairs).

With the table of (k, T >> shift) on the SRS a lane adds one table entry per pair of hot cycles, a single base where one cycle of the pair is cold, nothing where
both are.  The sums are the same group elements: jolt_grid_commit_onehot, jolt_grid_commit_onehot_classes and the opening hint's class sums (foreground and
background, two sources in one hint) are compared with the same calls on an SRS that has its window tables only (equal compressed points) and with the oracle's
commitments of the class parts (tests/test_gpu_pcs.py forms them the same way).  Shapes: every pair count from one upwards at the small end, K = 4 and 16, one
and five columns, and 2^12 cycles for more than one workgroup per column; cold patterns that put every case of the pair selection in both orders; SRSs with an
identity, with equal and with negated bases under the pairs the data hits (doubling and infinity entries)."""
import numpy as np
import pytest

import oracle_lib as O
from jolt_amd import ffi
from jolt_amd.workload import G1_GENERATOR
from util import rand_fr

pytestmark = pytest.mark.gpu
COLD = 0xFF


@pytest.fixture(scope="module")
def ctx():
    c = ffi.Context(0)
    yield c
    c.close()


def compressed(p):
    return ffi.host_g1_serialize_compressed(p)


def embed_onehot(idx_col, k, cycles):
    out = np.zeros((k * cycles, 4), dtype=np.uint64)
    hot = idx_col != COLD
    out[idx_col[hot].astype(np.int64) * cycles + np.nonzero(hot)[0]] = O.to_mont([1])[0]
    return out


def oracle_classes(host_srs, idx, K, shift):
    """[class][column]: the oracle's commitment of each column's class part on the grid folded `shift` times"""
    T = idx.shape[1]
    Tf = T >> shift
    return [[O.kzg_commit(embed_onehot(col[c::1 << shift], K, Tf), host_srs[: K * Tf]) for col in idx] for c in range(1 << shift)]


def columns(K, T, shift, seed):
    """one column of random 40 % cold cycles, and five: no cold cycle; all cold; every pair of the folded domain hot / cold; every pair cold / hot; an empty class
    (the last one; at shift 0 a tenth of the cycles cold instead)"""
    rng = np.random.default_rng(seed)
    one = rng.integers(0, K, size=(1, T), dtype=np.uint8)
    one[0, rng.random(T) < 0.4] = COLD
    five = rng.integers(0, K, size=(5, T), dtype=np.uint8)
    folded_odd = ((np.arange(T) >> shift) & 1).astype(bool)
    five[1, :] = COLD
    five[2, folded_odd] = COLD
    five[3, ~folded_odd] = COLD
    if shift:
        five[4, (1 << shift) - 1 :: 1 << shift] = COLD
    else:
        five[4, rng.random(T) < 0.1] = COLD
    return one, five


def srs_pair(ctx, host, K, T, shifts):
    """the same bases twice: with window tables only, and with the pair tables of `shifts` beside them"""
    plain, paired = ctx.srs_upload(host), ctx.srs_upload(host)
    for s in (plain, paired):
        ctx.srs_precompute_windows(s, 10, 1)
    built = ctx.srs_precompute_grid_pairs(paired, K, T, shifts)
    assert built == {s: 32 * K * K * (T >> s) for s in shifts}, built
    return plain, paired


def check_sums(ctx, plain, paired, host, idx, K, shift, oracle=True):
    src = ctx.onehot(idx, K)
    if shift == 0:
        got, ref = ctx.grid_commit_onehot(paired, src)[None], ctx.grid_commit_onehot(plain, src)[None]
    else:
        got, ref = ctx.grid_commit_onehot_classes(paired, src, shift), ctx.grid_commit_onehot_classes(plain, src, shift)
    assert got.shape == ref.shape == (1 << shift, idx.shape[0], 12)
    want = oracle_classes(host, idx, K, shift) if oracle else None
    for c in range(1 << shift):
        for p in range(idx.shape[0]):
            assert compressed(got[c, p]) == compressed(ref[c, p]), (shift, c, p)
            if oracle:
                assert O.g1_eq(got[c, p], want[c][p]), (shift, c, p)
    if shift == 0:  # the classes entry at shift 0 is the commitment, through the same launch
        again = ctx.grid_commit_onehot_classes(paired, src, 0)
        assert all(compressed(again[0, p]) == compressed(ref[0, p]) for p in range(idx.shape[0]))
    src.free()
    return ref


def check_hint(ctx, plain, paired, K, T, levels, seed):
    """two sources in one hint, on the main stream and in the background: level s = the classes entry of each source on the SRS without pair tables"""
    one, five = columns(K, T, 1, seed)
    sources = [ctx.onehot(one, K), ctx.onehot(five, K)]
    want = {s: np.concatenate([ctx.grid_commit_onehot_classes(plain, src, s) for src in sources], axis=1) for s in range(1, levels + 1)}
    for background in (False, True):
        hint = ctx.grid_hint(paired, sources, levels, background=background)
        for s in range(1, levels + 1):
            got = hint.download(s)
            assert got.shape == want[s].shape == (1 << s, 6, 12)
            assert all(compressed(got[c, p]) == compressed(want[s][c, p]) for c in range(1 << s) for p in range(6)), (background, s)
        hint.free()
    for src in sources:
        src.free()


@pytest.mark.parametrize("K", [16, 4])
@pytest.mark.parametrize("log_t", [2, 3, 4, 6, 12])
def test_sums_over_pair_tables_are_the_sums_over_single_bases(ctx, K, log_t):
    T = 1 << log_t
    shifts = [s for s in range(5) if (s <= 2 or T >= 64) and T >= (2 << s)]
    setup = ctx.srs_setup_from_secret(rand_fr(1, 8100 + log_t)[0], K * T, G1_GENERATOR)  # (the oracle's own setup takes seconds at 2^16 bases; the sums below are its own)
    host = setup.download()
    setup.free()
    plain, paired = srs_pair(ctx, host, K, T, shifts)
    assert ctx.memory_stats()["grid_pairs_bytes"] >= sum(32 * K * K * (T >> s) for s in shifts)
    for s in shifts:
        one, five = columns(K, T, s, 8200 + 10 * log_t + s)
        check_sums(ctx, plain, paired, host, one, K, s)
        check_sums(ctx, plain, paired, host, five, K, s, oracle=log_t < 12)  # (at 2^12 the five columns against the single bases, the one column against the oracle too)
    levels = max(s for s in shifts if T >= (1 << s))
    if levels:
        check_hint(ctx, plain, paired, K, T, min(levels, 4), 8300 + log_t)
    before = ctx.memory_stats()["grid_pairs_bytes"]
    paired.free()
    assert ctx.memory_stats()["grid_pairs_bytes"] == before - sum(32 * K * K * (T >> s) for s in shifts)  # freed with the SRS
    plain.free()


@pytest.mark.parametrize("K,log_t", [(4, 4), (16, 4), (4, 6), (16, 6)])
@pytest.mark.parametrize("variant", ["identity", "equal", "negated"])
def test_pair_tables_over_degenerate_bases(ctx, K, log_t, variant):
    """an identity among the bases (entries inf + Q, P + inf, inf + inf), and per shift a pair position whose two bases are equal (a doubling entry) or opposite (an
    infinity entry), under columns that select exactly those entries, first in a lane's list and later in it"""
    T = 1 << log_t
    shifts = [0, 1, 2]
    host = O.srs_setup_from_secret(rand_fr(1, 8400 + log_t)[0], K * T)
    a, b = 1, 2
    forced = {}  # shift -> [(cycle, hot index)]
    for s in shifts:
        D = T >> s
        forced[s] = []
        for m in ((0, 1) if variant != "identity" else (0,)):  # pair position m of class 0: cycles (2m) << s and (2m + 1) << s
            first, second = a * D + 2 * m, b * D + 2 * m + 1
            if variant == "identity":
                host[first] = O.g1_identity()
                host[(b + 1) * D + 2 * m + 3] = O.g1_identity()  # pair m + 1: P + inf
                host[a * D + 2 * m + 4], host[b * D + 2 * m + 5] = O.g1_identity(), O.g1_identity()  # pair m + 2: inf + inf
                forced[s] += [((2 * m) << s, a), ((2 * m + 1) << s, b), ((2 * m + 2) << s, a), ((2 * m + 3) << s, b + 1), ((2 * m + 4) << s, a), ((2 * m + 5) << s, b)]
            else:
                host[second] = host[first].copy() if variant == "equal" else O.g1_neg(host[first])
                forced[s] += [((2 * m) << s, a), ((2 * m + 1) << s, b)]
    for s in shifts:  # the later shifts' edits left the earlier ones' bases alone
        D = T >> s
        if variant != "identity":
            for m in (0, 1):
                second = host[b * D + 2 * m + 1]
                assert O.g1_eq(host[a * D + 2 * m], second if variant == "equal" else O.g1_neg(second)), (s, m)
    plain, paired = srs_pair(ctx, host, K, T, shifts)
    for s in shifts:
        one, five = columns(K, T, s, 8500 + 10 * log_t + s)
        if T >> s >= 8 or variant != "identity":
            for cycle, hot in forced[s]:
                one[0, cycle] = hot
                five[0, cycle] = hot
        check_sums(ctx, plain, paired, host, one, K, s)
        check_sums(ctx, plain, paired, host, five, K, s)
    check_hint(ctx, plain, paired, K, T, 2, 8600 + log_t)
    paired.free()
    plain.free()


def test_tables_that_cannot_be_built_and_range_commits_leave_everything_as_it_was(ctx):
    K, T = 16, 16
    host = O.srs_setup_from_secret(rand_fr(1, 8700)[0], 256 * T)
    srs = ctx.srs_upload(host)
    one, five = columns(K, T, 0, 8701)
    src = ctx.onehot(five, K)
    bare = ctx.grid_commit_onehot(srs, src)
    stats = ctx.memory_stats()["grid_pairs_bytes"]
    assert ctx.srs_precompute_grid_pairs(srs, K, T, (0,)) == {0: 0}  # no window tables yet: nothing is built
    ctx.srs_precompute_windows(srs, 10, 1)
    ref = ctx.grid_commit_onehot(srs, src)
    assert ctx.srs_precompute_grid_pairs(srs, 256, T, (0, 1)) == {0: 0, 1: 0}  # k = 256
    assert ctx.srs_precompute_grid_pairs(srs, K, T, (4,)) == {4: 0}  # 16 cycles are too short for shift 4
    assert ctx.srs_precompute_grid_pairs(srs, K, 3 * T, (0,)) == {0: 0}  # not a power of two
    assert ctx.srs_precompute_grid_pairs(srs, K, 32 * T, (0,)) == {0: 0}  # a grid larger than the SRS
    assert ctx.memory_stats()["grid_pairs_bytes"] == stats
    again = ctx.grid_commit_onehot(srs, src)
    classes = ctx.grid_commit_onehot_classes(srs, src, 1)
    assert all(compressed(again[p]) == compressed(ref[p]) == compressed(bare[p]) for p in range(5))
    # a wide source (K = 256) over the same SRS keeps the single bases whatever tables there are
    wide_idx = np.random.default_rng(8702).integers(0, 256, size=(2, T), dtype=np.uint16)
    wide = ctx.onehot(wide_idx, 256)
    wide_ref = ctx.grid_commit_onehot(srs, wide)
    built = ctx.srs_precompute_grid_pairs(srs, K, T, (0, 1))
    assert built == {0: 32 * K * K * T, 1: 16 * K * K * T}
    assert ctx.srs_precompute_grid_pairs(srs, K, T, (0, 1)) == built and ctx.memory_stats()["grid_pairs_bytes"] == stats + sum(built.values())  # found again, not rebuilt
    wide_again = ctx.grid_commit_onehot(srs, wide)
    assert all(compressed(wide_again[p]) == compressed(wide_ref[p]) for p in range(2))
    with_tables = ctx.grid_commit_onehot(srs, src)
    with_classes = ctx.grid_commit_onehot_classes(srs, src, 1)
    assert all(compressed(with_tables[p]) == compressed(ref[p]) for p in range(5))
    assert all(compressed(with_classes[c, p]) == compressed(classes[c, p]) for c in range(2) for p in range(5))
    # range commits ignore the tables: the whole range and two halves that add up to the commitment
    def range_commit(lo, hi):
        out = ffi.g1_array(5)
        ffi._call("jolt_grid_commit_onehot_range", ctx, ctx.h, srs.h, src.h, lo, hi, ffi._p(out))
        return out
    whole, left, right = range_commit(0, T), range_commit(0, T // 2), range_commit(T // 2, T)
    for p in range(5):
        assert compressed(whole[p]) == compressed(ref[p])
        assert O.g1_eq(O.g1_add(left[p], right[p]), ref[p])
    src.free()
    wide.free()
    srs.free()
