"""CPU: tests/fx_model.py -- the fixed-base MSM's digit recoding, capacity regions and host-side plan restated in Python integers -- held to the library's host forms
(jolt_host_fx_digits, jolt_host_fx_segment_capacity) and to the path table of docs/kernels.md section 3.5c.  tests/test_gpu_msm_fixed_paths.py then holds the device to
the model: every MSM there asserts the path the model predicts against the plan the library reports (jolt_msm_fixed_last_plan)."""
import numpy as np
import pytest

import fx_model as M
import oracle_lib as O
from corner_grids import fx_corner_grid, fx_digit_corners, fx_planted_scalars, fx_uniform_scalars
from jolt_amd import ffi

R = O.R_MOD


@pytest.mark.parametrize("c", [9, 10, 13, 17, 19, 20, 22, 23, 24, 26])
def test_model_digits_are_the_library_s(c):
    """the corner list of test_abi_cpu.py's recoding test, the per-window corner grid and 200 uniform scalars: signed digits, window count and bucket count of
    jolt_host_fx_digits equal the model's; the vectorised magnitudes the census uses are the digits' absolute values"""
    grid = fx_corner_grid(c)
    assert grid[:len(fx_digit_corners(c))] == fx_digit_corners(c)
    samples = grid + fx_uniform_scalars(200, 7000 + c)
    mont = O.to_mont(samples)
    mags = M.magnitudes(samples, c)
    assert mags.shape == (len(samples), M.windows(c))
    for i, s in enumerate(samples):
        got, n_buckets = ffi.host_fx_digits(mont[i], c)
        want = M.digits(s, c)
        assert got == want, (hex(s), c)
        assert n_buckets == M.buckets(c) and len(got) == M.windows(c)
        assert sum(d << (c * w) for w, d in enumerate(want)) % R == s
        assert [abs(d) for d in want] == [int(x) for x in mags[i]], hex(s)
    # whether a carry puts a point into bucket B = 2^(c-1) itself, or one past the top window's range, at the negation threshold: the model's answer is the library's
    # (checked above), and every magnitude addresses a bucket of the set
    for s in ((R - 1) // 2 - 1, (R - 1) // 2, (R - 1) // 2 + 1, (R - 1) // 2 + 2):
        assert all(abs(d) <= M.buckets(c) for d in M.digits(s, c))
    assert abs(M.digits((R - 1) // 2, c)[-1]) in (M.top_max(c) - 1, M.top_max(c))


@pytest.mark.parametrize("c,n", [(20, 1 << 16), (20, 1 << 18), (22, 1 << 17), (23, 1 << 16), (23, 1 << 20), (23, 1 << 26), (17, 1 << 20), (26, 1 << 20)])
def test_model_capacity_regions_are_the_library_s(c, n):
    """segment_capacity in Python floats == fx_segment_capacity in C doubles, at the segments where the formula changes (2^(c-1) and the top window's end inside a
    segment, the segments around them, the first and the last) and at 40 others"""
    per = 1 << M.lo_bits(c)
    nb1 = (M.buckets(c) >> M.lo_bits(c)) + 1
    half_seg, top_seg = (1 << (c - 1)) // per, M.top_max(c) // per
    segs = {0, 1, nb1 - 1, nb1, nb1 + 4} | {s + d for s in (half_seg, top_seg) for d in (-1, 0, 1) if s + d >= 0}
    segs |= {int(s) for s in np.random.default_rng(c * n % 9973).integers(0, nb1, size=40)}
    for seg in sorted(segs):
        assert M.segment_capacity(n, c, seg) == ffi.host_fx_segment_capacity(n, c, seg), (c, n, seg)


# c: (W, nb1, path, reduction by rows and columns): the table of docs/kernels.md section 3.5c
PATH_TABLE = {10: (26, 3, "keys two-pass", False), 13: (20, 17, "keys two-pass", False), 17: (15, 257, "keys two-pass", True), 18: (15, 513, "keys two-pass", True),
              20: (13, 2049, "soa wide", True), 21: (13, 4097, "soa wide", True), 22: (12, 8193, "soa", True), 23: (11, 24777, "soa", True),
              24: (11, 32769, "keys one-pass", True), 25: (11, 8193, "keys two-pass", True), 26: (10, 16385, "keys two-pass", True)}


def test_plan_of_every_window_width():
    """the sort path, segment count and reduction the model derives for c = 9 ... 26 on a 160 KiB LDS: the documented table, the structural rules behind it, and what
    changes on a 64 KiB device (no scalar-fed sort, no two-pass partition; where the segment histogram does not fit -- c = 23, 24, 26 -- the fixed-base method
    refuses and the per-window method takes the MSM)"""
    for c in range(9, 27):
        p = M.plan(c, 1 << 20)
        assert p["W"] == -(-253 // c) and p["lo_bits"] == (11 if c > 24 else 8) and p["nb1"] == (p["B"] >> p["lo_bits"]) + 1
        assert p["B"] == max(1 << (c - 1), M.top_max(c)) and p["grid_reduce"] == (c >= 17) and not p["refused"] and not p["capacity"]
        assert p["soa"] == (c in (20, 21, 22, 23)) and p["wide"] == (p["W"] > 12) and p["two_pass"] == (c != 24)
        assert (p["stage_cap"] > 0) == (c <= 24)
        if c in PATH_TABLE:
            assert (p["W"], p["nb1"], p["path"], p["grid_reduce"]) == PATH_TABLE[c], c
        small = M.plan(c, 1 << 20, max_lds=64 * 1024)
        # neither partition stage fits 64 KiB (68624 + 2048 bytes for 8192 eight-byte items): the one-pass scatter, wherever the segment histogram itself fits
        assert not small["soa"] and not small["two_pass"] and small["path"] == "keys one-pass" and small["refused"] == (c in (23, 24, 26))
    assert M.part_shared_bytes(12) == 101392 and M.part_shared_bytes(13) == 109584 and M.part_shared_bytes(8) == 68624
    # the capacity sort: the scalar-fed path, the caller's full-width mark, 2^16 terms
    for c, n, fw, want in ((23, 1 << 16, True, True), (23, (1 << 16) - 1, True, False), (23, 1 << 16, False, False), (20, 1 << 18, True, True), (24, 1 << 20, True, False),
                           (17, 1 << 20, True, False)):
        assert M.plan(c, n, full_width=fw)["capacity"] == want, (c, n, fw)
    # the heavy rule: 256 entries until four times the average list passes it, never more than 510
    assert M.plan(23, 2048)["heavy_threshold"] == 256 and M.plan(23, 1 << 26)["heavy_threshold"] == 4 * -(-(11 << 26) // M.buckets(23)) == 468
    assert M.plan(20, 1 << 26)["heavy_threshold"] == 510
    # the stage: 2 (total / nb1) + 2048 entries, at most what the LDS leaves; at c = 23 it reaches 4096 only from ~2.3 M terms, at c = 20 from 2^18 on
    first_staged = -(-1024 * 24777 // 11)  # the average segment holds 1024 entries
    assert M.plan(23, 1 << 20)["stage_cap"] == 2 * ((11 << 20) // 24777) + 2048 < M.STAGE_MIN and 2300000 < first_staged < 2310000
    assert M.plan(23, first_staged - 1)["stage_cap"] < M.STAGE_MIN == M.plan(23, first_staged)["stage_cap"]
    assert M.plan(20, 1 << 17)["stage_cap"] < M.STAGE_MIN <= M.plan(20, 1 << 18)["stage_cap"] == 5374
    assert M.plan(23, 1 << 26)["stage_cap"] == (M.MI355X_LDS - 12288) // 4
    assert M.stage_windows(5374, 20000, 90) == (True, 4) and M.stage_windows(5374, 20000, 2687) == (False, 1) and M.stage_windows(4095, 100, 1) == (False, 1)
    assert M.stage_windows(37888, 43700, 700) == (True, 2)  # the low segments of the 2^26-term MSM at c = 23: two windows


def test_census_counts_what_the_definition_says():
    """entries per bucket and segment from the vectorised recoding == a plain count over the signed digits, on the corner grid and uniform scalars"""
    for c in (10, 20, 23, 26):
        scalars = fx_corner_grid(c) + fx_uniform_scalars(300, 7100 + c)
        census = M.Census(scalars, c)
        lo, counts = M.lo_bits(c), {}
        for s in scalars:
            for d in M.digits(s, c):
                if d:
                    counts[abs(d)] = counts.get(abs(d), 0) + 1
        assert census.nonzero == sum(counts.values())
        assert {int(b): int(census.bucket[b]) for b in np.nonzero(census.bucket)[0]} == counts
        for seg in {b >> lo for b in counts}:
            inside = [v for b, v in counts.items() if b >> lo == seg]
            assert (int(census.segment[seg]), int(census.largest[seg])) == (sum(inside), max(inside))
        assert census.heavy_segments(2) == sum(-(-v // 128) for v in counts.values() if v > 2)


def test_planted_input_stages_in_several_windows_and_overflows_segment_zero_alone():
    """The input of the GPU suite's staged / partial-overflow test (c = 20, 2^18 terms, 600 scalars with every digit in [1, 255]): the model must predict what that
    test relies on -- the stage is on, segment 0 takes at least two stage windows, and in the capacity sort segment 0 alone receives more than its region -- and for
    uniform scalars alone no region overflows (here, at 2^18 and 2^16 terms, and at c = 23)."""
    c, n = 20, 1 << 18
    p = M.plan(c, n, full_width=True)
    assert p["path"] == "soa wide" and p["capacity"] and p["stage_cap"] >= M.STAGE_MIN
    census = M.Census(fx_planted_scalars(c, n, 600, 8100), c)
    assert census.overflowing() == [0]
    assert int(census.segment[0]) > M.segment_capacity(n, c, 0) + 5000  # far beyond the region, not a near miss
    staged, windows_ = M.stage_windows(p["stage_cap"], int(census.segment[0]), int(census.largest[0]))
    assert staged and windows_ >= 2
    assert all(M.stage_windows(p["stage_cap"], int(t), int(l))[0] for t, l in zip(census.segment, census.largest))  # every segment is staged
    uniform = M.Census(fx_uniform_scalars(n, 8200), c)
    assert uniform.overflowing() == [] and M.stage_windows(p["stage_cap"], int(uniform.segment[0]), int(uniform.largest[0]))[1] >= 2
    for cc, nn, seed in ((20, 1 << 16, 8300), (23, 1 << 16, 8400)):
        assert M.Census(fx_uniform_scalars(nn, seed), cc).overflowing() == []
