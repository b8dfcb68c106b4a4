"""GPU parity: Dory for polynomials held as field elements -- jolt_dory_commit_rows_fr / jolt_dory_hints_rows_fr (StreamingCommitment::feed(&[Fr]) per row) and
jolt_dory_fold_rows_blocks (BlockOpeningPoly::fold_rows, the dense vector_matrix_product).  Expected values come from the definition through the oracle: over the
bases beta^j G a row commitment is (sum_j v_j beta^j) G; folds are Python integers modulo r.  Points are compared as group elements, hints in addition bit for bit
as normalised points or the neutral element; no tolerance anywhere."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle_lib as O
from dory_groups import G1, R, fr_int, fr_ints, progression, rand_ints
from jolt_amd import ffi
from test_gpu_dory_commit import IDENT, assert_hint_element, eval_point
from util import rand_fr

pytestmark = pytest.mark.gpu
SRS_LEN = 2048
INVALID, MISMATCH, UNSUPPORTED, TOO_SMALL = 1, 5, 6, 9


@pytest.fixture(scope="module")
def ctx():
    c = ffi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def srs(ctx):
    beta = rand_fr(1, 1700)[0]
    return beta, ctx.srs_setup_from_secret(beta, SRS_LEN, O.g1_generator())


def same_group_element(a, b):
    return O.g1_is_identity(a) == O.g1_is_identity(b) and (O.g1_is_identity(a) or O.g1_eq(a, b))


def check_rows(ctx, srs, values, width, msm=False, out_first=0, tail=0):
    """values (Python integers mod r) as one table: the hints against the definition, the host-pointer entry against the hints, optionally jolt_dory_g1_msm per row"""
    beta, dev_srs = srs
    rows = len(values) // width
    table = ctx.upload(fr_ints(values))
    out = ctx.dory_state_alloc(ffi.DORY_KIND_G1, out_first + rows + tail)
    assert ctx.dory_hints_rows_fr(dev_srs, table, width, out, out_first=out_first) == rows
    got = out.download()
    assert all(np.array_equal(got[i], IDENT) for i in list(range(out_first)) + list(range(out_first + rows, out_first + rows + tail)))  # nothing outside the view
    host = ctx.dory_commit_rows_fr(dev_srs, table, width)
    assert host.shape[0] == rows
    bases = dev_srs.download(0, width) if msm else None
    for r in range(rows):
        row = values[r * width:(r + 1) * width]
        assert_hint_element(got[out_first + r], eval_point(beta, row), (width, r))
        assert O.g1_on_curve(host[r]) and same_group_element(host[r], got[out_first + r]), (width, r)
        if not any(v % R for v in row):
            assert np.array_equal(host[r], IDENT)
        if msm:
            assert same_group_element(ctx.dory_g1_msm(bases, fr_ints(row)), host[r]), (width, r)
    out.free()
    table.free()
    return got[out_first:out_first + rows]


# ------------------------------------------------------------------------------------------------------ rows
@pytest.mark.parametrize("width", [1, 2, 4, 8, 16, 32, 64])
def test_full_width_scalars_at_every_narrow_width(ctx, srs, width):
    """254-bit scalars where the rule c = log2(width) - 4 >= 3 would ask for up to 85 windows: the plan widens the digits instead"""
    for rows in (1, 3, 4):
        check_rows(ctx, srs, rand_ints(rows * width, 1710 + 10 * width + rows), width, msm=True)


def test_special_scalars_zero_rows_and_views(ctx, srs):
    half = (R - 1) // 2
    top = 1 << 252  # the top window of a 253-bit magnitude: below (r - 1) / 2, so it stays positive
    special = [0, 1, R - 1, half, half + 1, top, R - top, (1 << 253) - 1 - half, 2**64 - 1, 2**128, R - 2**64, 5]
    assert top < half and len(special) == 12
    values = special + [0] * 4 + [0] * 16 + rand_ints(15, 1721) + [0]  # row 0: the specials; row 1: all zero, between the others; row 2: one zero
    got = check_rows(ctx, srs, values, 16, msm=True, out_first=3, tail=2)
    assert np.array_equal(got[1], IDENT) and not np.array_equal(got[0], IDENT)
    # an all-zero table: identities written on the device, over whatever the view held
    beta, dev_srs = srs
    _, sentinel = progression(G1, 777, 13, 4)
    out = ctx.dory_vec_upload(ffi.DORY_KIND_G1, sentinel)
    zeros = ctx.upload(fr_ints([0] * 32))
    ctx.dory_hints_rows_fr(dev_srs, zeros, 8, out)
    assert all(np.array_equal(e, IDENT) for e in out.download())
    assert all(np.array_equal(e, IDENT) for e in ctx.dory_commit_rows_fr(dev_srs, zeros, 8))
    out.free()
    zeros.free()


def test_a_stretch_of_a_table(ctx, srs):
    """first > 0: rows 1 and 2 of a four-row table, nothing read before or after"""
    beta, dev_srs = srs
    width = 32
    values = rand_ints(4 * width, 1725)
    table = ctx.upload(fr_ints(values))
    out = ctx.dory_state_alloc(ffi.DORY_KIND_G1, 4)
    assert ctx.dory_hints_rows_fr(dev_srs, table, width, out, out_first=1, first=width, count=2 * width) == 2
    got = out.download()
    assert np.array_equal(got[0], IDENT) and np.array_equal(got[3], IDENT)
    host = ctx.dory_commit_rows_fr(dev_srs, table, width, first=width, count=2 * width)
    for r in (1, 2):
        assert_hint_element(got[r], eval_point(beta, values[r * width:(r + 1) * width]), r)
        assert same_group_element(host[r - 1], got[r])
    out.free()
    table.free()


def integer_rule(bits, width):
    """jolt_dory_commit_rows' plan: c = log2(width) - 4 in [3, 13], W = ceil((bits + 1) / c)"""
    c = max(3, min(13, width.bit_length() - 1 - 4))
    return c, (bits + c) // c


@pytest.mark.parametrize("width", [8, 256])
def test_small_values_run_the_integer_rows_windows(ctx, srs, width):
    """a u64-range table and a table of small negatives: the group elements of jolt_dory_commit_rows on the same integers, and its window plan"""
    beta, dev_srs = srs
    rng = np.random.default_rng(1730 + width)
    u = rng.integers(0, 2**63, size=2 * width, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    s = -rng.integers(1, 2**40, size=2 * width, dtype=np.int64)
    s[0], s[1], u[0] = -1, -2**63, np.uint64(2**64 - 1)
    for ints_host, bits in ((u, 64), (s, 64)):
        values = [int(x) % R for x in ints_host]
        assert max(min(v, R - v) for v in values).bit_length() == bits
        table, ints = ctx.upload(fr_ints(values)), ctx.ints(ints_host)
        got, want = ctx.dory_commit_rows_fr(dev_srs, table, width), ctx.dory_commit_rows(dev_srs, ints, width)
        for r in range(2):
            assert same_group_element(got[r], want[r]) and same_group_element(got[r], eval_point(beta, values[r * width:(r + 1) * width])), r
        assert ffi.host_dory_rows_fr_plan(bits, width) == integer_rule(bits, width)  # not the 254-bit count
        assert ffi.host_dory_rows_fr_plan(bits, width)[1] < ffi.host_dory_rows_fr_plan(254, width)[1]
        table.free()
        ints.free()


def test_heavy_bucket_in_every_window(ctx, srs):
    """two rows of 2048 copies of one full-width value: every window has a single bucket of 2048 points; v (beta^2048 - 1) / (beta - 1)"""
    beta, dev_srs = srs
    width = 2048
    v = rand_ints(1, 1740)[0]
    assert min(v, R - v).bit_length() >= 250
    table = ctx.upload(np.ascontiguousarray(np.broadcast_to(fr_int(v), (2 * width, 4))))
    b = O.from_mont(beta)[0]
    want = G1.point(v * (pow(b, width, R) - 1) * pow(b - 1, -1, R) % R)
    out = ctx.dory_state_alloc(ffi.DORY_KIND_G1, 2)
    ctx.dory_hints_rows_fr(dev_srs, table, width, out)
    got = out.download()
    host = ctx.dory_commit_rows_fr(dev_srs, table, width)
    for r in range(2):
        assert_hint_element(got[r], want, r)
        assert same_group_element(host[r], want)
    out.free()
    table.free()


def test_digit_kernel_without_the_lds_sort(monkeypatch):
    """JOLT_MSM_LDS_SORT=0 (the seam of tests/test_gpu_msm.py::test_msm_sort_paths_agree): the rows go through k_rows_digits, scan and scatter, whose eight-word digit
    loop is its own.  Full-width scalars at a narrow and a wider row, the special scalars, a u64-range row (fewer windows) and an all-zero row."""
    monkeypatch.setenv("JOLT_MSM_LDS_SORT", "0")
    c = ffi.Context(0)
    beta = rand_fr(1, 1700)[0]
    srs = (beta, c.srs_setup_from_secret(beta, 256, O.g1_generator()))
    half = (R - 1) // 2
    check_rows(c, srs, rand_ints(3 * 4, 1745), 4, msm=True)
    check_rows(c, srs, rand_ints(2 * 256, 1746), 256)
    check_rows(c, srs, [0, 1, R - 1, half, half + 1, 1 << 252, 2**64 - 1, 2**128] + [0] * 8 + rand_ints(8, 1747), 8, out_first=1, tail=1)
    check_rows(c, srs, [int(x) for x in np.random.default_rng(1748).integers(0, 2**64, size=32, dtype=np.uint64)] + [R - 1] * 32, 32)
    srs[1].free()
    c.close()


def test_batches_cut_by_bucket_slots(ctx, srs):
    """6000 rows of one full-width value each: c = 6 gives every row 43 windows of 33 bucket slots, so the batch is cut by kMaxBatchSlots (not by its keys) into two
    launch sets; the rows on both sides of the cut, and every row as hint against host entry"""
    beta, dev_srs = srs
    src = open(os.path.join(os.path.dirname(ffi.__file__), "csrc", "dory_rows_fr.hip.h")).read()
    slots = 1 << int(re.search(r"kMaxBatchSlots = \(size_t\)1 << (\d+);", src).group(1))
    c, W = ffi.host_dory_rows_fr_plan(254, 1)
    cut = slots // (W * ((1 << (c - 1)) + 1))
    rows = 6000
    assert 0 < cut < rows < 2 * cut and cut < (1 << 26) // W
    values = rand_ints(rows, 1749)
    table = ctx.upload(fr_ints(values))
    out = ctx.dory_state_alloc(ffi.DORY_KIND_G1, rows)
    assert ctx.dory_hints_rows_fr(dev_srs, table, 1, out) == rows
    got, host = out.download(), ctx.dory_commit_rows_fr(dev_srs, table, 1)
    for r in (0, 1, cut - 1, cut, cut + 1, rows - 1):
        assert_hint_element(got[r], eval_point(beta, [values[r]]), r)
    assert np.array_equal(O.g1_to_affine(host), O.g1_to_affine(got))  # the host entry's points and the hints are the same group elements: all 6000 rows
    out.free()
    table.free()


def test_row_refusals_keep_their_codes_write_nothing_and_leave_the_context_usable(ctx, srs):
    beta, dev_srs = srs
    size_t = C.c_size_t
    small_srs = ctx.srs_setup_from_secret(beta, 64, O.g1_generator())
    values = rand_ints(128, 1750)
    table = ctx.upload(fr_ints(values))
    odd = ctx.upload(fr_ints(values[:96]))
    _, sentinel = progression(G1, 4321, 99, 8)
    out = ctx.dory_vec_upload(ffi.DORY_KIND_G1, sentinel)
    g2v, frv = ctx.dory_state_alloc(ffi.DORY_KIND_G2, 8), ctx.dory_state_alloc(ffi.DORY_KIND_FR, 8)
    other = ffi.Context(0)
    foreign = other.dory_state_alloc(ffi.DORY_KIND_G1, 8)
    host = ffi.g1_array(8)
    host[:] = sentinel

    def hints(dst, t=table, first=0, count=128, rw=32, out_first=0, srs_h=small_srs.h, ctx_h=ctx.h):
        return ffi.lib().jolt_dory_hints_rows_fr(ctx_h, srs_h, t.h if t else None, size_t(first), size_t(count), size_t(rw), dst, size_t(out_first))

    def commit(t=table, first=0, count=128, rw=32, dst=host, srs_h=small_srs.h, ctx_h=ctx.h):
        return ffi.lib().jolt_dory_commit_rows_fr(ctx_h, srs_h, t.h if t else None, size_t(first), size_t(count), size_t(rw), ffi._p(dst) if dst is not None else None)

    assert hints(g2v.h) == INVALID and hints(frv.h) == INVALID and hints(None) == INVALID and hints(foreign.h) == INVALID
    assert hints(out.h, out_first=5) == INVALID               # 4 rows from element 5 of 8
    assert hints(out.h, out_first=2**64 - 1) == INVALID       # first + n wraps
    for call in (lambda **kw: hints(out.h, **kw), commit):
        assert call(rw=24) == INVALID                         # not a power of two
        assert call(rw=0) == INVALID
        assert call(rw=128) == TOO_SMALL                      # 128 divides the count but the SRS holds 64 bases
        assert call(t=odd, count=96, rw=64) == MISMATCH       # 96 values in rows of 64
        assert call(first=64, count=96) == INVALID            # past the table
        assert call(first=2**64 - 32, count=64) == INVALID    # first + count wraps
        assert call(first=129, count=0) == INVALID
        assert call(t=None) == INVALID and call(srs_h=None) == INVALID and call(ctx_h=None) == INVALID
    assert commit(dst=None) == INVALID
    # nothing was enqueued: the destinations hold their bytes; then valid calls on the same context
    assert np.array_equal(out.download(), sentinel) and np.array_equal(host, sentinel)
    assert np.array_equal(foreign.download(), np.stack([IDENT] * 8))
    assert hints(out.h, out_first=4) == 0 and commit() == 0
    got = out.download()
    assert np.array_equal(got[:4], sentinel[:4])
    for r in range(4):
        assert_hint_element(got[4 + r], eval_point(beta, values[r * 32:(r + 1) * 32]), r)
        assert same_group_element(host[r], got[4 + r])
    assert np.array_equal(host[4:], sentinel[4:])
    assert hints(out.h, first=128, count=0) == 0              # an empty stretch at the end of the table: nothing to do
    foreign.free()
    other.close()
    for v in (out, g2v, frv, table, odd, small_srs):
        v.free()


# ------------------------------------------------------------------------------------------------------ the block fold
def test_slice_constant_is_the_kernels():
    src = open(os.path.join(os.path.dirname(ffi.__file__), "csrc", "dory.hip")).read()
    assert int(re.search(r"constexpr uint32_t kBlockFoldSlice = (\d+);", src).group(1)) == ffi.DORY_BLOCK_FOLD_SLICE


def fold_definition(tables, sigmas, scalars, sigma, left, base=None):
    """out[c] = base[c] + sum_d s_d sum_r left[r] table_d[(r << sigma_d) + c] for c < 2^sigma_d, in Python integers"""
    out = list(base) if base is not None else [0] * (1 << sigma)
    for t, sd, s in zip(tables, sigmas, scalars):
        for i, x in enumerate(t):
            out[i & ((1 << sd) - 1)] = (out[i & ((1 << sd) - 1)] + s * left[i >> sd] * x) % R
    return out


def run_fold(ctx, tables, sigmas, scalars, sigma, left, base=None):
    dev = [ctx.upload(fr_ints(t)) for t in tables]
    lt = ctx.upload(fr_ints(left))
    bt = ctx.upload(fr_ints(base)) if base is not None else None
    out = ctx.dory_fold_rows_blocks(dev, sigmas, fr_ints(scalars), sigma, lt, bt)
    got = out.download()
    for t in dev + [lt, out] + ([bt] if bt is not None else []):
        t.free()
    return got


SLICE = ffi.DORY_BLOCK_FOLD_SLICE
# (log rows, log columns): 32 x 32; rows across the slice boundary with few and with many columns; a single entry; two entries as a row and as a column
WHOLE_SHAPES = [(5, 5), (8, 3), (3, 8), (0, 0), (0, 1), (1, 0)]


@pytest.mark.parametrize("log_rows,log_cols", WHOLE_SHAPES)
def test_whole_table_fold_against_python_integers(ctx, log_rows, log_cols):
    """one table of sigma_d = sigma, no base: the dense vector_matrix_product"""
    assert (1 << 8) > SLICE and (1 << 5) <= SLICE  # 256 rows are several slices (the last cases of a slice's loop included), 32 are one
    table = rand_ints(1 << (log_rows + log_cols), 1760 + 16 * log_rows + log_cols)
    left = rand_ints(1 << log_rows, 1761 + log_rows)
    got = run_fold(ctx, [table], [log_cols], [1], log_cols, left)
    assert np.array_equal(got, fr_ints(fold_definition([table], [log_cols], [1], log_cols, left)))


def test_a_row_count_that_is_no_multiple_of_the_slice_or_of_the_reduction_run(ctx):
    """a block with a single entry (sigma_d = 0) beside one of 128 rows, left longer than either: slices past a block's rows contribute nothing"""
    tables = [rand_ints(1, 1770), rand_ints(128 * 4, 1771), rand_ints(2, 1772)]
    sigmas, scalars, sigma = [0, 2, 0], rand_ints(3, 1773), 3
    left = rand_ints(256, 1774)
    base = rand_ints(8, 1775)
    for b in (None, base):
        got = run_fold(ctx, tables, sigmas, scalars, sigma, left, b)
        assert np.array_equal(got, fr_ints(fold_definition(tables, sigmas, scalars, sigma, left, b)))


@pytest.mark.parametrize("with_base", [False, True])
def test_blocks_in_a_ten_variable_grid(ctx, with_base):
    """blocks of m = 4 and 5 (sigma_p = 2 and 3) top-left in a 32 x 32 grid, distinct scalars; the columns past a block stay the base's"""
    tables, sigmas, sigma = [rand_ints(16, 1780), rand_ints(32, 1781)], [2, 3], 5
    scalars, left = rand_ints(2, 1782), rand_ints(32, 1783)
    base = rand_ints(32, 1784) if with_base else None
    got = run_fold(ctx, tables, sigmas, scalars, sigma, left, base)
    want = fold_definition(tables, sigmas, scalars, sigma, left, base)
    assert np.array_equal(got, fr_ints(want))
    assert np.array_equal(got[8:], fr_ints(base[8:] if with_base else [0] * 24))
    for t, sd in zip(tables, sigmas):  # the formula behind the definition: the host form of the embedding
        assert all(ffi.host_dory_block_index(sd, sigma, i) == ((i >> sd) << sigma) + (i & ((1 << sd) - 1)) for i in range(len(t)))


@pytest.mark.parametrize("order", ["cycle_major", "address_major"])
def test_joint_fold_of_a_trace_and_blocks(ctx, order):
    """base = the trace's fold in either placement; against the dense joint matrix with the blocks added top-left"""
    from test_gpu_dory_opening import joint_dense_table, make_batch
    log_t, log_k, sigma, nu = 6, 4, 5, 5
    n, T, K = 1 << sigma, 1 << log_t, 1 << log_k
    batch = make_batch(log_t, log_k, n_dense=1, seed=1790)
    left = rand_ints(1 << nu, 1791)
    srcs = [ctx.onehot(i, K) for i in batch["idx"]]
    dense = [ctx.upload(batch["dense"][0])]
    lt = ctx.upload(fr_ints(left))
    cells = [int(x) for x in O.from_mont(joint_dense_table(batch))]  # cycle-major: index k * T + t
    if order == "address_major":
        trace = ctx.dory_fold_rows_grid_am(srcs, batch["gamma"], dense, batch["dgamma"], log_k, 0, sigma, lt)
        cells = [cells[(i & (K - 1)) * T + (i >> log_k)] for i in range(K * T)]
    else:
        trace = ctx.dory_fold_rows_grid(srcs, batch["gamma"], dense, batch["dgamma"], log_k, sigma, lt)
    blocks, sigmas, scalars = [rand_ints(16, 1792), rand_ints(32, 1793)], [2, 3], rand_ints(2, 1794)
    for t, sd, s in zip(blocks, sigmas, scalars):
        for i, x in enumerate(t):
            at = ffi.host_dory_block_index(sd, sigma, i)
            cells[at] = (cells[at] + s * x) % R
    want = [sum(left[r] * cells[r * n + c] for r in range(1 << nu)) % R for c in range(n)]
    dev = [ctx.upload(fr_ints(t)) for t in blocks]
    out = ctx.dory_fold_rows_blocks(dev, sigmas, fr_ints(scalars), sigma, lt, trace)
    assert np.array_equal(out.download(), fr_ints(want))
    for t in srcs + dense + dev + [lt, trace, out]:
        t.free()


def test_fold_refusals(ctx):
    t16, t32, t12 = (ctx.upload(fr_ints(rand_ints(k, 1800 + k))) for k in (16, 32, 12))
    left4, left8, base8, base4 = (ctx.upload(fr_ints(rand_ints(k, 1810 + j))) for j, k in enumerate((4, 8, 8, 4)))
    one = fr_ints([1] * 9)
    result = C.c_void_p()

    def fold(tables=(t16,), sigmas=(2,), sigma=3, lt=left4, base=None, n=None, res=C.byref(result), ctx_h=ctx.h, sc=one):
        hs = (C.c_void_p * max(len(tables), 1))(*[t.h if t else None for t in tables])
        sg = (C.c_uint32 * max(len(sigmas), 1))(*sigmas)
        return ffi.lib().jolt_dory_fold_rows_blocks(ctx_h, hs, sg, C.c_size_t(len(tables) if n is None else n), ffi._p(sc) if sc is not None else None, C.c_uint32(sigma),
                                                    lt.h if lt else None, base.h if base else None, res)

    assert fold(tables=(t12,)) == INVALID                       # not a power of two
    assert fold(sigmas=(5,), sigma=5) == INVALID                # sigma_d above m_d
    assert fold(sigmas=(3,), sigma=2) == INVALID                # sigma_d above the grid's sigma
    assert fold(n=0) == INVALID and fold(tables=(None,)) == INVALID
    assert fold(lt=None) == INVALID and fold(res=None) == INVALID and fold(ctx_h=None) == INVALID and fold(sc=None) == INVALID
    assert fold(tables=(t16,) * 9, sigmas=(2,) * 9) == UNSUPPORTED
    assert fold(sigmas=(1,)) == MISMATCH                        # 8 rows against 4 entries of left
    assert fold(tables=(t16, t32), sigmas=(2, 2)) == MISMATCH   # the second block has 8 rows
    assert fold(base=base4) == MISMATCH                         # a base that is not 2^sigma long
    bad = one.copy()
    bad[0] = 2**64 - 1
    assert fold(sc=bad) == INVALID                              # not a canonical scalar
    assert result.value is None
    assert fold(tables=(t16, t32), sigmas=(2, 2), lt=left8, base=base8) == 0 and result.value
    out = ffi.Table(ctx, result)
    assert len(out) == 8
    for t in (t16, t32, t12, left4, left8, base8, base4, out):
        t.free()
