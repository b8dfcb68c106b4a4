"""GPU: every sort path and the reduction's edges of the fixed-base MSM (jolt_amd/csrc/msm_fixed.hip) at small term counts.

Which kernels sort an MSM is a function of (window bits, windows, terms, the caller's full-width mark): docs/kernels.md section 3.5c has the table.  Every MSM here
names the path it means through tests/fx_model.py's prediction AND the plan the library reports for the call it just made (ffi.Context.msm_fixed_last_plan), so a
case that silently took another path fails.  Points are compared with the oracle as group elements and in compressed form; the device's own count of non-zero digits
(jolt_msm_profile_buckets_last: what bench.py divides by) is compared with the model's.  Every comparison is an equality."""
import numpy as np
import pytest

import fx_model as M
import oracle_lib as O
from corner_grids import fx_corner_grid, fx_planted_scalars, fx_uniform_scalars
from jolt_amd import ffi
from test_gpu_limb_add_paths import special_bases
from util import rand_fr

pytestmark = pytest.mark.gpu
R = O.R_MOD
HOST_PLAN = ffi.FX_PLAN_FIELDS[:12]
INVALID_ARG = 1


@pytest.fixture(scope="module")
def ctx():
    c = ffi.Context(0)
    yield c
    c.close()


def same_point(a, b):
    return O.g1_eq(a, b) and O.g1_serialize_compressed(a) == O.g1_serialize_compressed(b)


def fixed_msm(ctx, dev, scalars, c, path, full_width=False):
    """one MSM over Montgomery-form scalars on the window tables of dev -> (point, additions, plan, model plan); the plan the library reports is the model's, word for
    word, and the model's path is the one the caller names"""
    tab = ctx.upload(np.ascontiguousarray(scalars))
    ctx.msm_profile_buckets(True)
    got = ctx.msm(dev, tab, full_width=full_width)
    _, additions = ctx.msm_profile_buckets_last()
    ctx.msm_profile_buckets(False)
    plan = ctx.msm_fixed_last_plan()
    tab.free()
    model = M.plan(c, len(scalars), full_width=full_width, max_lds=plan["max_lds_per_block"])
    assert {k: plan[k] for k in HOST_PLAN} == {k: model[k] for k in HOST_PLAN}
    assert not model["refused"] and model["path"] == path, (model["path"], path)
    return got, additions, plan, model


def tables(ctx, host, c):
    dev = ctx.srs_upload(host)
    ctx.srs_precompute_windows(dev, c, 1)  # min_terms = 1: every length takes the fixed-base method
    return dev


PATH = {17: "keys two-pass", 20: "soa wide", 22: "soa", 23: "soa", 24: "keys one-pass"}


# ---------------------------------------------------------------------------------------------------- a. corner scalars on the scalar-fed sort
@pytest.mark.parametrize("c", [20, 22, 23])
def test_corner_scalars_on_the_scalar_fed_sort(ctx, c):
    """k_fx_hist_scalars / k_fx_partition_groups_scalars (12- and 13-entry instantiations) / k_fx_partition_segments_soa / k_fx_segment_sort_staged<8, true> on the corner
    grid of c followed by uniform scalars: prefixes of one entry, around a wavefront and a workgroup, on either side of one tile of the segments pass (W n = 8192), the
    whole grid, and 2200 terms"""
    n_max, W = 2200, M.windows(c)
    grid = fx_corner_grid(c)
    ints = grid + fx_uniform_scalars(n_max - len(grid), 9000 + c)
    scalars = O.to_mont(ints)
    nonzero = np.count_nonzero(M.magnitudes(ints, c), axis=1).cumsum()
    host = O.srs_setup_from_secret(rand_fr(1, 9100 + c)[0], n_max)
    dev = tables(ctx, host, c)
    lengths = [1, 2, 63, 64, 65, 1023, 1024, 1025, M.PART_TILE // W, M.PART_TILE // W + 1, len(grid), n_max]
    assert W * lengths[8] <= M.PART_TILE < W * lengths[9]
    for n in lengths:
        got, additions, plan, _ = fixed_msm(ctx, dev, scalars[:n], c, PATH[c])
        assert plan["soa"] and plan["wide"] == (c == 20) and not plan["capacity"], n
        assert additions == int(nonzero[n - 1]), (n, additions)
        assert same_point(got, O.g1_msm_pippenger(host[:n], scalars[:n])), n
    dev.free()


@pytest.mark.parametrize("c", [17, 24])
def test_corner_grid_on_the_key_array_sort(c):
    """c = 17: k_fx_digits, k_fx_hist<8>, the two-pass k_fx_partition_*<8>, k_fx_segment_sort_staged<8, false> under the row / column reduction.  c = 24: 257 segment groups
    are more than the partition has bins, so the one-pass k_fx_scatter<8> sorts with a 131076-byte LDS histogram -- or, on a device whose LDS cannot hold it, the
    fixed-base method refuses and the per-window method computes the MSM.  Either is right; the plan says which ran and the point is checked."""
    ctx = ffi.Context(0)
    ints = fx_corner_grid(c)
    n = len(ints)
    scalars = O.to_mont(ints)
    host = O.srs_setup_from_secret(rand_fr(1, 9200 + c)[0], n)
    dev = tables(ctx, host, c)
    tab = ctx.upload(scalars)
    got = ctx.msm(dev, tab)
    try:
        plan = ctx.msm_fixed_last_plan()
    except ffi.JoltError as e:  # no fixed-base MSM ran on this context: the method refused the call
        assert c == 24 and e.status == INVALID_ARG
        plan = None
    if plan is None:
        print(f"c = {c}: the fixed-base method refused the MSM, the per-window method ran")
    else:
        model = M.plan(c, n, max_lds=plan["max_lds_per_block"])
        assert {k: plan[k] for k in HOST_PLAN} == {k: model[k] for k in HOST_PLAN} and not model["refused"]
        assert model["path"] == PATH[c] and plan["two_pass"] == (c == 17) and not plan["soa"] and plan["grid_reduce"]
        assert plan["largest_segment"] == int(M.Census(ints, c).segment.max()) and plan["heavy_segments"] == 0
        print(f"c = {c}: {model['path']} ran (nb1 = {plan['nb1']}, LDS {plan['max_lds_per_block']} bytes)")
    assert c == 24 or plan is not None
    assert same_point(got, O.g1_msm_pippenger(host, scalars))
    ctx.close()


# ---------------------------------------------------------------------------------------------------- b. degenerate bases
@pytest.mark.parametrize("c", [20, 23])
def test_repeated_negated_and_identity_bases_on_the_scalar_fed_sort(ctx, c):
    """the base groups P, P, -P, P, infinity, Q, -Q, Q of test_gpu_limb_add_paths.py under its five scalar cases and its lists of one and two points: the scalar-fed segment
    sort orders a bucket's list itself, so the doublings and cancellations at the heads of the lists are met in the order IT produces"""
    n = 1024
    host = special_bases(n, 9300 + c)
    dev = tables(ctx, host, c)
    rng = np.random.default_rng(9301)
    per_group = rand_fr(n // 8, 9302 + c)
    neg = lambda row: O.to_mont([(R - O.from_mont(row.reshape(1, 4))[0]) % R])[0]
    cases = {"equal_in_group": np.repeat(per_group, 8, axis=0),
             "alternating_sign": np.stack([per_group[i // 8] if i % 2 == 0 else neg(per_group[i // 8]) for i in range(n)]),
             "few_scalars": rand_fr(4, 9303 + c)[rng.integers(0, 4, size=n)],
             "minus_one": np.repeat(O.to_mont([R - 1]), n, axis=0),
             "uniform": rand_fr(n, 9304 + c)}
    for m in (1, 2, 3, 5, 8, 9):  # lists of one and two points
        cases[f"first {m}"] = np.repeat(per_group[:1], m, axis=0)
    for name, scalars in cases.items():
        got, additions, plan, model = fixed_msm(ctx, dev, scalars, c, PATH[c])
        census = M.Census(O.from_mont(scalars), c)
        assert additions == census.nonzero, name
        assert plan["heavy_segments"] == census.heavy_segments(model["heavy_threshold"]) and plan["largest_segment"] == int(census.segment.max()), name
        assert same_point(got, O.g1_msm_pippenger(host[:len(scalars)], scalars)) and O.g1_on_curve(got), name
    dev.free()


# ---------------------------------------------------------------------------------------------------- c. bucket lengths around the heavy rule
def test_bucket_lengths_around_the_heavy_rule(ctx):
    """c = 23: n equal scalars d < 2^22 put n points into bucket d.  Up to 256 the list is summed by one lane (k_fx_buckets_ordered_staged); from 257 on it is cut into
    ceil(n / 128) segments (k_fx_heavy_segments_staged / k_fx_heavy_combine) -- the device's count of them is read back.  Then one bucket of 11 * 2048 entries: every digit
    of every scalar is 5.  Reference: d * (P_0 + ... + P_(n-1)) through the oracle."""
    c, n_max = 23, 2048
    host = O.srs_setup_from_secret(rand_fr(1, 9400)[0], n_max)
    dev = tables(ctx, host, c)
    prefix = [O.g1_identity()]
    for p in host:
        prefix.append(O.g1_add(prefix[-1], p))
    d = 0x2D5A93
    assert 0 < d < 1 << 22 and M.digits(d, c) == [d] + [0] * 10
    for n in (127, 128, 129, 255, 256, 257, 383, 384, 385):
        got, additions, plan, model = fixed_msm(ctx, dev, O.to_mont([d] * n), c, "soa")
        assert model["heavy_threshold"] == 256 and plan["heavy_segments"] == (0 if n <= 256 else -(-n // 128)), (n, plan["heavy_segments"])
        assert additions == n and plan["largest_segment"] == n
        assert same_point(got, O.g1_scalar_mul(prefix[n], O.to_mont([d])[0])), n
    fives = sum(5 << (c * w) for w in range(11))
    assert M.digits(fives, c) == [5] * 11
    got, additions, plan, _ = fixed_msm(ctx, dev, O.to_mont([fives] * n_max), c, "soa")
    assert additions == 11 * n_max == 22528 and plan["heavy_segments"] == 176 and plan["largest_segment"] == 22528
    assert same_point(got, O.g1_scalar_mul(prefix[n_max], O.to_mont([fives])[0]))
    dev.free()


# ---------------------------------------------------------------------------------------------------- d. reduction weights
@pytest.mark.parametrize("c", [17, 20, 23])
def test_reduction_weights_bucket_by_bucket(ctx, c):
    """k_fx_red_cols (chunks of 16 rows of 2048 buckets), k_fx_red_rows (16 buckets per lane), their guard b <= B on the last row and the recombination
    2^11 sum_h h R_h + sum_l l C_l with KNOWN weights: every scalar puts exactly one point into a chosen bucket -- a low bucket by s = b, at c = 23 a bucket of the top
    window by s = b << 230, each also negated as r - s -- at the edges of a lane's 16 buckets, of a row, of a chunk of rows, and of the bucket set.  (r - 1) / 2 and its
    neighbours ride along: the model says which of them carries into bucket B itself.  The same scalars then run as single-term MSMs against P_0, so that a failure
    names its bucket.  Reference: sum_i (+-b_i 2^(c w_i)) P_i, the oracle's MSM over the same scalars."""
    half = 1 << (c - 1)
    B = M.buckets(c)
    low = [b for b in (1, 15, 16, 17, 2047, 2048, 2049, 16 * 2048 - 1, 16 * 2048, 16 * 2048 + 1, half - 1, half) if b <= half]
    chosen = [(b, b) for b in low]
    if c == 23:
        assert B == M.top_max(c) == 6342813
        chosen += [(b, M.top_bucket_scalar(b, c)) for b in low + [half + 1, B - 2, B - 1]]
    ints, where = [], []
    for b, s in chosen:
        for t in (s, R - s):
            assert [abs(x) for x in M.digits(t, c) if x] == [b], (b, hex(t))  # one entry, in bucket b
            ints.append(t)
            where.append((b, "+" if t == s else "-", "top" if s != b else "low"))
    edge = [(R - 1) // 2 - 1, (R - 1) // 2, (R - 1) // 2 + 1, (R - 1) // 2 + 2]
    reaches_B = [s for s in edge if any(abs(x) == B for x in M.digits(s, c))]
    assert c != 23 or reaches_B, "at c = 23 the top window's carry fills bucket B = top_max at the negation threshold"
    ints += edge
    where += [("edge", hex(s), "B" if s in reaches_B else "") for s in edge]
    scalars = O.to_mont(ints)
    census = M.Census(ints, c)
    assert all(int(census.bucket[b]) >= 2 for b, _ in chosen) and (not reaches_B or int(census.bucket[B]) >= 1)
    host = O.srs_setup_from_secret(rand_fr(1, 9500 + c)[0], len(ints))
    dev = tables(ctx, host, c)
    got, additions, plan, _ = fixed_msm(ctx, dev, scalars, c, PATH[c])
    assert plan["grid_reduce"] and additions == census.nonzero and plan["largest_segment"] == int(census.segment.max())
    assert same_point(got, O.g1_msm_naive(host, scalars))
    for i, s in enumerate(scalars):
        got, additions, plan, _ = fixed_msm(ctx, dev, s.reshape(1, 4), c, PATH[c])
        assert plan["grid_reduce"] and additions == int(np.count_nonzero(M.magnitudes([ints[i]], c)))
        assert same_point(got, O.g1_scalar_mul(host[0], s)), where[i]
    dev.free()


# ---------------------------------------------------------------------------------------------------- e. staged output, stage windows, partial overflow
LOG_N, C_MID = 18, 20


@pytest.fixture(scope="module")
def mid(ctx):
    """2^18 powers of beta with 20-bit window tables (the smallest shape that stages on the scalar-fed path) and the two inputs of the tests below"""
    n = 1 << LOG_N
    beta = rand_fr(1, 9600)[0]
    g = O.g1_generator()
    dev = ctx.srs_setup_from_secret(beta, n, g)
    ctx.srs_precompute_windows(dev, C_MID, 1)
    planted = fx_planted_scalars(C_MID, n, 600, 8100)
    uniform = fx_uniform_scalars(n, 8200)
    want = lambda mont: O.g1_scalar_mul(g, O.kzg_eval_univariate(mont, beta))
    yield {"dev": dev, "want": want, "planted": planted, "planted_mont": O.to_mont(planted), "uniform": uniform, "uniform_mont": O.to_mont(uniform)}
    dev.free()


def test_staged_output_in_several_stage_windows(ctx, mid):
    """exact sort (no full-width mark) of 2^18 terms at c = 20 with 600 planted scalars: k_fx_segment_sort_staged<8, true> stages every segment through LDS, and segment 0
    -- the top window's 6.2 K values crowd the low 25 segments, and the planted digits add 7800 entries -- takes several stage windows"""
    census = M.Census(mid["planted"], C_MID)
    got, additions, plan, model = fixed_msm(ctx, mid["dev"], mid["planted_mont"], C_MID, "soa wide")
    assert not plan["capacity"] and plan["overflow"] == 0 and plan["stage_cap"] >= M.STAGE_MIN
    staged, n_windows = M.stage_windows(plan["stage_cap"], int(census.segment[0]), int(census.largest[0]))
    assert staged and n_windows >= 2, (plan["stage_cap"], int(census.segment[0]), int(census.largest[0]))
    assert all(M.stage_windows(plan["stage_cap"], int(t), int(l))[0] for t, l in zip(census.segment, census.largest))
    assert plan["largest_segment"] == int(census.segment.max()) == int(census.segment[0])
    assert additions == census.nonzero and plan["heavy_segments"] == census.heavy_segments(model["heavy_threshold"])
    assert same_point(got, mid["want"](mid["planted_mont"]))


def test_capacity_sort_with_one_overflowing_region_then_a_clean_run(ctx, mid):
    """capacity sort (full-width mark) of the same input: segment 0 alone receives more than its region, the flag goes up and the exact passes redo a sort the first
    one had finished everywhere else; the count of additions is the exact sort's.  A purely uniform MSM right after it runs with the flag down: nothing leaks."""
    census = M.Census(mid["planted"], C_MID)
    assert census.overflowing() == [0]
    got, additions, plan, _ = fixed_msm(ctx, mid["dev"], mid["planted_mont"], C_MID, "soa wide", full_width=True)
    assert plan["capacity"] and plan["overflow"] == 1
    assert additions == census.nonzero and plan["largest_segment"] == int(census.segment[0])
    assert same_point(got, mid["want"](mid["planted_mont"]))
    uniform = M.Census(mid["uniform"], C_MID)
    assert uniform.overflowing() == []
    got, additions, plan, model = fixed_msm(ctx, mid["dev"], mid["uniform_mont"], C_MID, "soa wide", full_width=True)
    assert plan["capacity"] and plan["overflow"] == 0
    assert additions == uniform.nonzero and plan["largest_segment"] == max(M.segment_capacity(1 << LOG_N, C_MID, s) for s in range(model["nb1"]))
    assert same_point(got, mid["want"](mid["uniform_mont"]))


@pytest.mark.parametrize("n,capacity", [(1 << 16, True), ((1 << 16) - 1, False)])
def test_capacity_sort_starts_at_2_16_terms(ctx, mid, n, capacity):
    ints, mont = mid["uniform"][:n], mid["uniform_mont"][:n]
    census = M.Census(ints, C_MID)
    assert census.overflowing() == []
    got, additions, plan, _ = fixed_msm(ctx, mid["dev"], mont, C_MID, "soa wide", full_width=True)
    assert plan["capacity"] == capacity and plan["overflow"] == 0 and additions == census.nonzero
    assert same_point(got, mid["want"](mont))


# ---------------------------------------------------------------------------------------------------- f. refusal and state
def test_plan_read_out_before_and_after_other_msms():
    """no fixed-base MSM yet: JOLT_ERR_INVALID_ARG, also after a per-window MSM; after a fixed-base one the plan; after another per-window MSM the same plan, its
    device words marked stale (the per-window method has laid the workspace out again)"""
    ctx = ffi.Context(0)
    host = O.srs_setup_from_secret(rand_fr(1, 9700)[0], 300)
    scalars = rand_fr(300, 9701)
    want = O.g1_msm_pippenger(host, scalars)
    plain, tab = ctx.srs_upload(host), ctx.upload(scalars)
    for _ in range(2):
        with pytest.raises(ffi.JoltError) as e:
            ctx.msm_fixed_last_plan()
        assert e.value.status == INVALID_ARG
        assert same_point(ctx.msm(plain, tab), want)  # per-window: no tables
    dev = tables(ctx, host, 13)
    got, additions, plan, _ = fixed_msm(ctx, dev, scalars, 13, "keys two-pass")
    assert same_point(got, want) and additions == M.Census(O.from_mont(scalars), 13).nonzero
    assert None not in plan.values() and not plan["grid_reduce"] and not plan["soa"]
    assert ctx.msm_fixed_last_plan() == plan  # reading changes nothing
    assert same_point(ctx.msm(plain, tab), want)
    after = ctx.msm_fixed_last_plan()
    assert {k: after[k] for k in HOST_PLAN} == {k: plan[k] for k in HOST_PLAN}
    assert (after["overflow"], after["largest_segment"], after["heavy_segments"]) == (None, None, None)
    ctx.close()
