"""The fixed-base MSM's digit recoding and host-side plan in Python integers (TEST INFRASTRUCTURE), from their definitions -- what jolt_amd/csrc/msm_fixed.hip states in
fx_digits_of and at the head of jolt_internal_msm_fixed_enqueue, restated so that a test can say BEFORE it runs an MSM which sort kernels that MSM takes, how many
entries it sorts, which buckets are over-full, whether a segment is staged through LDS and in how many stage windows, and which capacity regions overflow.
tests/test_msm_fixed_paths_cpu.py holds this model to the library's host forms; tests/test_gpu_msm_fixed_paths.py holds the device to the model.

Nothing here calls the library.
"""
import numpy as np

import oracle_lib as O

R = O.R_MOD
HALF_R = (R - 1) // 2

# constants of msm_fixed.hip / msm_kernels.hip.h
LANE_CAP = 128            # kLaneCap
HEAVY_SEG = 128           # kFxHeavySeg
CLASSES = 512             # kClasses
GROUP_BITS = 7            # kGroupBits: 128 segments per group
PART_BINS = 256           # kPartBins
PART_TILE = 8192          # kPartTile: entries per tile of the segments pass
PART_PER_S, PART_PER_WIDE = 12, 13
RED_S = 11                # kRedS: the reduction's columns are the low 11 bits of a bucket
STAGE_MIN = 4096          # k_fx_segment_sort_staged stages only into >= this many entries
MI355X_LDS = 160 * 1024   # hipDeviceProp::sharedMemPerBlock on gfx950


def part_shared_bytes(per, threads=1024):
    """sizeof(PartSharedN<per, threads>): the stage of 8-byte items, three tables of kPartBins words, four wave sums"""
    return 8 * threads * per + 3 * 4 * PART_BINS + 16


def windows(c):
    return -(-253 // c)


def top_max(c):
    """the unsigned top window's digits are < top_max"""
    return (HALF_R >> (c * (windows(c) - 1))) + 1


def buckets(c):
    """the largest |digit| a table set with c-bit windows addresses"""
    return max(1 << (c - 1), top_max(c))


def lo_bits(c):
    return 11 if c > 24 else 8


def digits(s, c):
    """the signed digits of the canonical scalar s: s above (r - 1) / 2 is replaced by r - s with every digit negated; c-bit windows from the bottom, a window whose value
    (carry in included) exceeds 2^(c-1) goes negative and carries; the top window takes what is left, unsigned.  sum_w digit_w 2^(c w) = s mod r."""
    W, half, full = windows(c), 1 << (c - 1), 1 << c
    flip = s > HALF_R
    t = R - s if flip else s
    out, carry = [], 0
    for w in range(W - 1):
        raw = ((t >> (w * c)) & (full - 1)) + carry
        d, carry = (raw - full, 1) if raw > half else (raw, 0)
        out.append(-d if flip else d)
    top = (t >> ((W - 1) * c)) + carry
    out.append(-top if flip else top)
    return out


def magnitudes(scalars, c):
    """(n, W) int64 array of |digit|, the recoding above over a whole list of canonical integers at once"""
    W, half, full = windows(c), 1 << (c - 1), 1 << c
    t = np.array([R - s if s > HALF_R else s for s in scalars], dtype=object).reshape(-1)
    out = np.zeros((len(t), W), dtype=np.int64)
    carry = np.zeros(len(t), dtype=np.int64)
    for w in range(W - 1):
        raw = ((t >> (w * c)) & (full - 1)).astype(np.int64) + carry if len(t) else carry
        neg = raw > half
        out[:, w] = np.where(neg, full - raw, raw)
        carry = neg.astype(np.int64)
    out[:, W - 1] = (t >> ((W - 1) * c)).astype(np.int64) + carry if len(t) else carry
    return out


class Census:
    """what the sort of one MSM sees: non-zero digits (= mixed additions), entries per bucket and per segment, the largest bucket of every segment"""

    def __init__(self, scalars, c):
        mags = magnitudes(scalars, c).reshape(-1)
        mags = mags[mags != 0]
        lo = lo_bits(c)
        nb1 = (buckets(c) >> lo) + 1
        self.c, self.n, self.nonzero = c, len(scalars), int(mags.size)
        assert mags.size == 0 or int(mags.max()) <= buckets(c)
        self.bucket = np.bincount(mags, minlength=nb1 << lo)
        self.segment = self.bucket.reshape(nb1, 1 << lo).sum(axis=1)
        self.largest = self.bucket.reshape(nb1, 1 << lo).max(axis=1)

    def heavy_segments(self, heavy_threshold):
        """the 128-entry segments of the buckets above the threshold: what the segment sort adds up in hcnt[0]"""
        over = self.bucket[self.bucket > heavy_threshold]
        return int(((over + HEAVY_SEG - 1) // HEAVY_SEG).sum())

    def overflowing(self):
        """segments that receive more entries than the region the capacity sort gives them"""
        return [int(s) for s in np.nonzero(self.segment)[0] if int(self.segment[s]) > segment_capacity(self.n, self.c, int(s))]


def segment_capacity(n, c, seg):
    """the region of segment seg in the capacity sort of n uniform scalars: expected entries + 8 standard deviations + 64, a multiple of 4; in the double arithmetic
    of fx_segment_capacity, operation for operation (Python floats are IEEE doubles)"""
    W, half, tmax, per = windows(c), 1 << (c - 1), top_max(c), 1 << lo_bits(c)
    p_signed = 2.0 / float(1 << c) * float(W - 1)
    p_top = 1.0 / float(tmax)
    lo, hi = seg * per, seg * per + per
    below_half = (min(hi, half) - lo) if lo < half else 0
    below_top = (min(hi, tmax) - lo) if lo < tmax else 0
    has_half = lo <= half < hi
    mean = float(n) * (float(below_half) * p_signed + (0.5 * p_signed if has_half else 0.0) + float(below_top) * p_top)
    root = 0.0
    if mean > 0.0:
        root = mean if mean > 1.0 else 1.0
        for _ in range(40):
            root = 0.5 * (root + mean / root)
    return (int(mean + 8.0 * root) + 64 + 3) & ~3


def plan(c, n, full_width=False, max_lds=MI355X_LDS):
    """the decisions of jolt_internal_msm_fixed_enqueue for n terms over a table set with c-bit windows, under the names of ffi.FX_PLAN_FIELDS, plus `B`, `n_groups`,
    `refused` (JOLT_ERR_UNSUPPORTED: the per-window method takes the MSM) and `path`, the sort that runs:
      "keys two-pass"  k_fx_digits, k_fx_hist<LO>, k_fx_partition_groups<LO> / _segments<LO>
      "keys one-pass"  k_fx_digits, k_fx_hist<LO>, k_fx_scatter<LO>
      "soa" / "soa wide"  k_fx_hist_scalars, k_fx_partition_groups_scalars (12 / 13 entries per thread), k_fx_partition_segments_soa<8>
    each followed by k_fx_segment_sort_staged<8, soa> (8-bit segments) or k_fx_segment_sort<11>"""
    W, B, lo = windows(c), buckets(c), lo_bits(c)
    nb1 = (B >> lo) + 1
    total = W * n
    n_groups = (nb1 + (1 << GROUP_BITS) - 1) >> GROUP_BITS
    avg = -(-total // B)
    wide = W > PART_PER_S
    soa = lo == 8 and W <= PART_PER_WIDE and n_groups <= PART_BINS and part_shared_bytes(PART_PER_WIDE if wide else PART_PER_S) + 2048 <= max_lds
    capacity = soa and full_width and n >= 1 << 16
    if capacity:
        top_shift = c * (W - 1) + 1
        capacity = 1 <= top_shift and 254 - top_shift <= 31 and 0 < top_max(c) <= 0xFFFFFFFF
    if capacity:
        capacity = sum(segment_capacity(n, c, s) + 8 for s in range(nb1)) < (1 << 32) - 4096
    two_pass = n_groups <= PART_BINS and part_shared_bytes(8) + 2048 <= max_lds
    stage_cap = min(max_lds - 12288 if max_lds > 12288 else 0, (2 * (total // nb1) + 2048) * 4) // 4 if lo == 8 else 0
    return {"c": c, "W": W, "lo_bits": lo, "soa": soa, "wide": wide, "capacity": capacity, "two_pass": two_pass, "grid_reduce": B >= 1 << 16,
            "heavy_threshold": min(max(2 * LANE_CAP, 4 * avg), CLASSES - 2), "stage_cap": stage_cap, "nb1": nb1, "max_lds_per_block": max_lds,
            "B": B, "n_groups": n_groups, "refused": total >= 1 << 32 or 4 * nb1 > max_lds,
            "path": ("soa wide" if wide else "soa") if soa else ("keys two-pass" if two_pass else "keys one-pass")}


def stage_windows(stage_cap, seg_total, seg_largest):
    """(staged, windows) of one segment in k_fx_segment_sort_staged: the sorted segment goes through the LDS stage iff the stage holds twice its largest bucket and at
    least 4096 entries, in windows of stage_cap - largest positions"""
    staged = stage_cap > 2 * seg_largest and stage_cap >= STAGE_MIN
    return staged, (-(-seg_total // (stage_cap - seg_largest)) if staged else 1)


def top_bucket_scalar(b, c):
    """the scalar whose only non-zero digit is b in the top window"""
    return b << (c * (windows(c) - 1))
