"""The host build of the per-row routine of jolt_dory_combine_hints (dory.hip: shared signed-digit plan, per-window walk by descending digit, Horner
recombination) against the oracle's sum of scalar multiplications; the hint transpose against the index formula of finish_one_hot_column_major_chunks
(crates/jolt-dory/src/streaming.rs:318-362); and the presence of the three entry points of the Dory opening.  No GPU."""
import numpy as np
import pytest

import oracle_lib as O
from jolt_amd import ffi
from util import rand_fr

R = O.R_MOD


def points(n, seed):
    """n points with non-trivial Jacobian Z: random multiples of the generator (the oracle's scalar multiplication leaves a projective representative)"""
    g = O.g1_generator()
    return np.stack([O.g1_scalar_mul(g, s) for s in rand_fr(n, seed)])


def want_row(pts, scalars):
    acc = O.g1_identity()
    for p, s in zip(pts, scalars):
        acc = O.g1_add(acc, O.g1_scalar_mul(p, s))
    return acc


def extreme_digit_scalars():
    """for every window width c in 3..8: all c-bit groups equal to 2^(c-1) (every signed digit +2^(c-1), the top bucket, no carries) and to 2^(c-1) + 1
    (every digit negative with a carry into the next window: -(2^(c-1) - 1) throughout), cut below r"""
    out = []
    for c in range(3, 9):
        for group in (1 << (c - 1), (1 << (c - 1)) + 1):
            v = sum(group << (c * k) for k in range(254 // c + 1)) & ((1 << 253) - 1)
            assert v < R
            out.append(v)
    return out


SPECIAL = [0, 1, 2, R - 1, R - 2, 1 << 128]


@pytest.mark.parametrize("n", [1, 2, 7, 40])
def test_combine_row_matches_oracle(n):
    pts = points(n, 100 + n)
    pool = SPECIAL + extreme_digit_scalars()
    rng = np.random.default_rng(n)
    for rep in range(3 if n < 40 else 1):
        vals = [int.from_bytes(rng.bytes(32), "little") % R for _ in range(n)]
        # the special and extreme scalars rotate through the terms; n = 1 sees every one of them below
        for k in range(0, n, 2):
            vals[k] = pool[(rep * n + k) % len(pool)]
        sc = O.to_mont(vals)
        assert O.g1_eq(ffi.host_dory_combine_row(pts, sc), want_row(pts, sc)), (n, rep)


def test_combine_row_every_special_scalar_alone():
    p = points(1, 7)
    for v in SPECIAL + extreme_digit_scalars():
        sc = O.to_mont([v])
        assert O.g1_eq(ffi.host_dory_combine_row(p, sc), O.g1_scalar_mul(p[0], sc[0])), hex(v)


def test_combine_row_special_points():
    pts = points(4, 11)
    s = rand_fr(3, 12)
    ident = O.g1_identity()
    # the identity among the terms
    mix = np.stack([pts[0], ident, pts[1]])
    assert O.g1_eq(ffi.host_dory_combine_row(mix, s), want_row(mix, s))
    # the same point twice with equal scalars: the doubling branch of the addition, in every window
    twice = np.stack([pts[2], pts[2]])
    ss = np.stack([s[0], s[0]])
    assert O.g1_eq(ffi.host_dory_combine_row(twice, ss), want_row(twice, ss))
    # P with s and -P with s: the sum passes through the identity; with a third term it comes back
    cancel = np.stack([pts[3], O.g1_neg(pts[3])])
    assert O.g1_is_identity(ffi.host_dory_combine_row(cancel, ss))
    cancel3 = np.stack([pts[3], O.g1_neg(pts[3]), pts[0]])
    s3 = np.stack([s[0], s[0], s[1]])
    assert O.g1_eq(ffi.host_dory_combine_row(cancel3, s3), O.g1_scalar_mul(pts[0], s[1]))
    # all scalars zero, all points the identity
    zeros = O.to_mont([0, 0, 0, 0])
    assert O.g1_is_identity(ffi.host_dory_combine_row(pts, zeros))
    assert O.g1_is_identity(ffi.host_dory_combine_row(np.stack([ident, ident]), ss))


def test_combine_row_refuses_a_non_canonical_scalar():
    bad = np.full((1, 4), 2**64 - 1, dtype=np.uint64)
    with pytest.raises(ffi.JoltError) as e:
        ffi.host_dory_combine_row(points(1, 3), bad)
    assert e.value.status == 1


def test_hint_transpose_is_the_references_index_formula():
    """finish_one_hot_column_major_chunks: hint[row * chunks + chunk] = out[chunk * k + row]; with chunk_width = 2^sigma the hint's entry is row
    (row << (log_t - sigma)) + chunk of the cycle-major grid matrix"""
    chunks, k = 8, 5
    flat = np.arange(chunks * k * 12, dtype=np.uint64).reshape(chunks * k, 12)  # out[chunk * k + row], as jolt_dory_commit_onehot writes it
    hint = ffi.dory_onehot_hint(flat.reshape(chunks, k, 12))
    assert hint.shape == (k * chunks, 12)
    for row in range(k):
        for chunk in range(chunks):
            assert np.array_equal(hint[row * chunks + chunk], flat[chunk * k + row])
    log_t, sigma = 6, 3  # chunks = 2^(log_t - sigma)
    for row in range(k):
        for chunk in range(chunks):
            assert row * chunks + chunk == (row << (log_t - sigma)) + chunk


def test_library_exports_the_opening_entry_points():
    lib = ffi.lib()
    for name in ("jolt_dory_fold_rows_grid", "jolt_dory_combine_hints", "jolt_host_dory_combine_row"):
        assert hasattr(lib, name), name


def test_operation_count_beats_double_and_add():
    for n in (5, 40):  # the fixed cost of a window (16 levels, 5 doublings) needs four terms to pay for itself
        assert ffi.dory_combine_ops_per_row(n) < 1.5 * 254 * n
    assert ffi.dory_combine_ops_per_row(40) == 51 * (40 + 16 + 5 + 1)
