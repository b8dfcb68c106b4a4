"""GPU parity: Dory commitment and opening in the address-major trace placement -- jolt_dory_hints_onehot_am / jolt_dory_hints_rows_am / jolt_dory_fold_rows_grid_am
(dory_am.hip.h, dory.hip) and DoryWitnessCommitment(order="address_major").  Expected values come from the definition: over the bases beta^j G a row commitment is
(sum_c M[r][c] beta^c) G through the oracle's field arithmetic and one scalar multiplication, over planted progressions it is a discrete logarithm, and the row fold
is L^T M in Python integers from the placement formula.  Points are compared as group elements, the normalised representative and the identity bit for bit, Fr
tables bit for bit; no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from dory_groups import G1, G2, R, fr_ints, progression, rand_ints
from jolt_amd import ffi
from util import rand_fr

pytestmark = pytest.mark.gpu
IDENT = O.g1_identity()
ONE = IDENT[0:4]  # the Montgomery one of Fq
SRS_LEN = 1024


@pytest.fixture(scope="module")
def ctx():
    c = ffi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def srs(ctx):
    beta = rand_fr(1, 1600)[0]
    return beta, ctx.srs_setup_from_secret(beta, SRS_LEN, O.g1_generator())


def eval_point(beta, coeffs):
    """(sum_c coeffs[c] beta^c) G"""
    return O.g1_scalar_mul(O.g1_generator(), O.kzg_eval_univariate(O.to_mont([v % R for v in coeffs]), beta))


def assert_hint_element(got, want, what):
    if O.g1_is_identity(want):
        assert np.array_equal(got, IDENT), what
    else:
        assert np.array_equal(got[8:12], ONE), what
        assert O.g1_on_curve(got) and O.g1_eq(got, want), what


def cold_of(idx):
    return 0xFFFF if idx.dtype == np.uint16 else 0xFF


def onehot_row(column, r, per_row, log_block, log_stride, sigma):
    """row r of a one-hot column's matrix: 2^sigma coefficients"""
    coeffs = [0] * (1 << sigma)
    for j in range(per_row):
        h = int(column[r * per_row + j])
        if h != cold_of(column):
            coeffs[(j << log_block) + (h << log_stride)] += 1
    return coeffs


def make_indices(rng, n_polys, cycles, k, dtype=np.uint8, cold=0.25):
    idx = rng.integers(0, k, size=(n_polys, cycles)).astype(dtype)
    idx[rng.random((n_polys, cycles)) < cold] = 0xFFFF if dtype == np.uint16 else 0xFF
    return idx


def check_onehot(beta, idx, hints, log_block, log_stride, sigma, rows_to_check=None):
    """hints: (columns, rows, 12)"""
    per_row = 1 << (sigma - log_block)
    rows = idx.shape[1] // per_row
    assert hints.shape[:2] == (idx.shape[0], rows)
    n_ident = 0
    for p in range(idx.shape[0]):
        for r in (range(rows) if rows_to_check is None else rows_to_check):
            coeffs = onehot_row(idx[p], r, per_row, log_block, log_stride, sigma)
            want = eval_point(beta, coeffs) if any(coeffs) else IDENT
            assert_hint_element(hints[p, r], want, (p, r))
            n_ident += not any(coeffs)
    return n_ident


# ------------------------------------------------------------------------------------------------------ one-hot columns
def test_onehot_hints_into_a_view_with_a_cold_row(ctx, srs):
    """(8, 4, 0, 6): C = 4, three columns, 5 elements before the view and 4 after it stay identities; an aligned block of 4 cold cycles is bit for bit the identity"""
    beta, dev_srs = srs
    log_t, log_block, sigma, cols, out_first, tail = 8, 4, 6, 3, 5, 4
    idx = make_indices(np.random.default_rng(1601), cols, 1 << log_t, 16)
    idx[1, 4 * 7:4 * 8] = 0xFF  # row 7 of column 1
    source = ctx.onehot(idx, 16)
    rows = (1 << log_t) >> (sigma - log_block)
    total = cols * rows
    out = ctx.dory_state_alloc(ffi.DORY_KIND_G1, out_first + total + tail)
    assert ctx.dory_hints_onehot_am(dev_srs, source, out, sigma, log_block, out_first=out_first) == total
    got = out.download()
    assert all(np.array_equal(got[i], IDENT) for i in list(range(out_first)) + list(range(out_first + total, out_first + total + tail)))
    hints = got[out_first:out_first + total].reshape(cols, rows, 12)
    assert check_onehot(beta, idx, hints, log_block, 0, sigma) >= 1
    assert np.array_equal(hints[1, 7], IDENT)
    out.free()
    source.free()


def test_onehot_hints_long_rows(ctx, srs):
    """(12, 2, 0, 10): C = 256, 16 rows per column, two columns"""
    beta, dev_srs = srs
    idx = make_indices(np.random.default_rng(1602), 2, 1 << 12, 4)
    source = ctx.onehot(idx, 4)
    out = ctx.dory_state_alloc(ffi.DORY_KIND_G1, 32)
    assert ctx.dory_hints_onehot_am(dev_srs, source, out, 10, 2) == 32
    check_onehot(beta, idx, out.download().reshape(2, 16, 12), 2, 0, 10)
    out.free()
    source.free()


def test_onehot_hints_16_bit_indices(ctx, srs):
    """K = 300 in blocks of 2^9, (7, 9, 0, 10), C = 2: addresses 0, 255, 256 and 299 are hot, cold is 0xFFFF"""
    beta, dev_srs = srs
    idx = make_indices(np.random.default_rng(1603), 2, 1 << 7, 300, np.uint16)
    for p in range(2):
        for s, a in enumerate([0, 255, 256, 299]):
            idx[p, 10 * s + p] = a
    source = ctx.onehot(idx, 300)
    out = ctx.dory_state_alloc(ffi.DORY_KIND_G1, 128)
    assert ctx.dory_hints_onehot_am(dev_srs, source, out, 10, 9) == 128
    check_onehot(beta, idx, out.download().reshape(2, 64, 12), 9, 0, 10)
    out.free()
    source.free()


def test_onehot_hints_widened_grid(ctx, srs):
    """(6, 4, 2, 8): log_block = 6, log_stride = 2"""
    beta, dev_srs = srs
    idx = make_indices(np.random.default_rng(1604), 2, 1 << 6, 16)
    source = ctx.onehot(idx, 16)
    out = ctx.dory_state_alloc(ffi.DORY_KIND_G1, 32)
    assert ctx.dory_hints_onehot_am(dev_srs, source, out, 8, 6, 2) == 32
    check_onehot(beta, idx, out.download().reshape(2, 16, 12), 6, 2, 8)
    out.free()
    source.free()


def test_onehot_hints_one_cycle_per_row(ctx, srs):
    """(6, 4, 0, 4): C = 1, every row a single base or the identity"""
    beta, dev_srs = srs
    idx = make_indices(np.random.default_rng(1605), 2, 1 << 6, 16)
    source = ctx.onehot(idx, 16)
    out = ctx.dory_state_alloc(ffi.DORY_KIND_G1, 128)
    assert ctx.dory_hints_onehot_am(dev_srs, source, out, 4, 4) == 128
    assert check_onehot(beta, idx, out.download().reshape(2, 64, 12), 4, 0, 4) >= 1
    out.free()
    source.free()


def test_onehot_hints_in_forced_launch_sets(ctx, srs, monkeypatch):
    """192 rows in launch sets of 40: the cuts fall inside columns and a launch set spans two columns; also a range of columns"""
    beta, dev_srs = srs
    idx = make_indices(np.random.default_rng(1606), 3, 1 << 8, 16)
    source = ctx.onehot(idx, 16)
    whole, cut, last_two = (ctx.dory_state_alloc(ffi.DORY_KIND_G1, n) for n in (192, 192, 128))
    ctx.dory_hints_onehot_am(dev_srs, source, whole, 6, 4)
    monkeypatch.setenv("JOLT_DORY_AM_BATCH_ROWS", "40")
    ctx.dory_hints_onehot_am(dev_srs, source, cut, 6, 4)
    ctx.dory_hints_onehot_am(dev_srs, source, last_two, 6, 4, first_poly=1, n_polys=2)
    monkeypatch.delenv("JOLT_DORY_AM_BATCH_ROWS")
    a, b, c = whole.download(), cut.download(), last_two.download()
    assert np.array_equal(a, b) and np.array_equal(a[64:], c)
    check_onehot(beta, idx, b.reshape(3, 64, 12), 4, 0, 6)
    for v in (whole, cut, last_two):
        v.free()
    source.free()


# ------------------------------------------------------------------------------------------------------ exceptional additions on the device
def test_exceptional_additions(ctx):
    """K = 4, sigma = 6 (C = 16) over 64 bases that are all P (every addition after a row's first is a doubling) and over P, -P, P, ... (address parity is the sign:
    partial sums return to the identity in the middle of a row and the row goes on)"""
    k0 = 424242
    p = ffi.host_dory_g1_normalise(G1.point(k0)[None, :], 1)[0]
    same = ctx.srs_upload(np.stack([p] * 64))
    alternating = ctx.srs_upload(np.stack([p if i % 2 == 0 else O.g1_neg(p) for i in range(64)]))
    rng = np.random.default_rng(1607)
    idx = make_indices(rng, 1, 16 * 8, 4)
    idx[0, 0:16] = 0xFF                            # row 0: all cold
    idx[0, 16:32] = [0, 1] * 8                     # row 1: P - P + P - P ...
    idx[0, 32:48] = [0, 0, 1, 1, 3, 2, 2, 3] * 2   # row 2: 2P, 0, -P, 0, ...
    idx[0, 48:64] = [2] * 16                       # row 3: one base sixteen times
    idx[0, 80:96] = 0xFF                           # row 5: all cold
    idx[0, 96:112] = [0xFF, 1, 0, 0xFF, 0, 1, 0xFF, 0xFF, 3, 3, 2, 2, 0xFF, 0xFF, 0xFF, 0xFF]  # row 6: net zero with cold cycles between
    source = ctx.onehot(idx, 4)
    out = ctx.dory_state_alloc(ffi.DORY_KIND_G1, 8)
    n_ident = [0, 0]
    for which, dev_srs in enumerate((same, alternating)):
        assert ctx.dory_hints_onehot_am(dev_srs, source, out, 6, 2) == 8
        got = out.download()
        for r in range(8):
            hot = [int(h) for h in idx[0, 16 * r:16 * (r + 1)] if h != 0xFF]
            m = len(hot) if which == 0 else sum(1 if h % 2 == 0 else -1 for h in hot)
            assert_hint_element(got[r], G1.point(k0 * m % R), (which, r))
            n_ident[which] += m == 0
    assert n_ident[0] >= 2 and n_ident[0] <= 6 and n_ident[1] >= 2 and n_ident[1] <= 6
    for v in (out, source, same, alternating):
        v.free()


# ------------------------------------------------------------------------------------------------------ dense columns
@pytest.mark.parametrize("log_t,log_block,sigma", [(8, 4, 6), (12, 2, 10)])
def test_rows_hints_all_kinds(ctx, srs, log_t, log_block, sigma):
    beta, dev_srs = srs
    T, per_row = 1 << log_t, 1 << (sigma - log_block)
    rows = T // per_row
    rng = np.random.default_rng(1608 + log_t)
    u = rng.integers(0, 2**63, size=T, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    u[per_row:2 * per_row] = 0  # an all-zero row between the others
    s = rng.integers(-2**63, 2**63, size=T, dtype=np.int64)
    s[0], s[1], s[2], s[3] = -2**63, 2**63 - 1, -1, 0
    big = [int(rng.integers(0, 2**63)) * int(rng.integers(0, 2**63)) * (1 if j % 3 else -1) for j in range(T)]
    big[0], big[1], big[2], big[3] = -2**127, 2**127 - 1, -1, 0
    check = range(rows) if rows <= 16 else [0, 1, 2, rows // 2, rows - 1]
    for values, ints in ((u, ctx.ints(u)), (s, ctx.ints(s)), (big, ctx.ints(big, "i128"))):
        out = ctx.dory_state_alloc(ffi.DORY_KIND_G1, rows + 3)
        assert ctx.dory_hints_rows_am(dev_srs, ints, sigma, log_block, out, out_first=2) == rows
        got = out.download()
        assert all(np.array_equal(got[i], IDENT) for i in (0, 1, rows + 2))
        for r in check:
            coeffs = [0] * (1 << sigma)
            for j in range(per_row):
                coeffs[j << log_block] = int(values[r * per_row + j])
            assert_hint_element(got[2 + r], eval_point(beta, coeffs) if any(coeffs) else IDENT, r)
        assert all(np.array_equal(e, IDENT) or np.array_equal(e[8:12], ONE) for e in got)
        out.free()
        ints.free()
    # an all-zero column: identities over whatever the view held
    out = ctx.dory_vec_upload(ffi.DORY_KIND_G1, np.stack([G1.point(7 + i) for i in range(rows)]))
    zeros = ctx.ints(np.zeros(T, dtype=np.uint64))
    ctx.dory_hints_rows_am(dev_srs, zeros, sigma, log_block, out)
    assert all(np.array_equal(e, IDENT) for e in out.download())
    out.free()
    zeros.free()


# ------------------------------------------------------------------------------------------------------ the row fold
def fold_definition(batch, left_ints, log_block, log_stride, sigma):
    """L^T M in Python integers from the placement formula"""
    per_row = 1 << (sigma - log_block)
    out = [0] * (1 << sigma)
    g, dg = O.from_mont(batch["gamma"]), O.from_mont(batch["dgamma"])
    columns = np.concatenate(batch["idx"], axis=0)
    cold = cold_of(columns)
    for p, col in enumerate(columns):
        for t in np.nonzero(col != cold)[0]:
            t = int(t)
            c = ((t % per_row) << log_block) + (int(col[t]) << log_stride)
            out[c] = (out[c] + int(g[p]) * left_ints[t // per_row]) % R
    for d, col in enumerate(batch["dense_ints"]):
        for t in range(len(col)):
            c = (t % per_row) << log_block
            out[c] = (out[c] + int(dg[d]) * left_ints[t // per_row] % R * int(col[t])) % R
    return out


@pytest.mark.parametrize("log_t,log_k,e,sigma", [(8, 4, 0, 6), (12, 2, 0, 10), (6, 4, 2, 8), (6, 4, 0, 4), (6, 8, 0, 9)])
def test_fold_rows_against_python_integers(ctx, log_t, log_k, e, sigma):
    from test_gpu_dory_opening import make_batch
    log_block, log_stride = log_k + e, e
    batch = make_batch(log_t, log_k, n_dense=2, seed=1620 + log_t + log_k, wide=log_k == 8)
    rows = (1 << log_t) >> (sigma - log_block)
    left_host = rand_fr(rows, 1630 + sigma)
    srcs = [ctx.onehot(i, batch["k"]) for i in batch["idx"]]
    dense = [ctx.upload(t) for t in batch["dense"]]
    left = ctx.upload(left_host)
    out = ctx.dory_fold_rows_grid_am(srcs, batch["gamma"], dense, batch["dgamma"], log_block, log_stride, sigma, left)
    got = out.download()
    want = fold_definition(batch, [int(x) for x in O.from_mont(left_host)], log_block, log_stride, sigma)
    assert np.array_equal(got, fr_ints(want))
    unmapped = [c for c in range(1 << sigma) if (c & ((1 << log_block) - 1)) & ((1 << log_stride) - 1)]
    assert len(unmapped) == (0 if e == 0 else (1 << sigma) - ((1 << sigma) >> e)) and not got[unmapped].any()
    assert any(want)
    for t in srcs + dense + [left, out]:
        t.free()


# ------------------------------------------------------------------------------------------------------ refusals
def test_refusals_keep_their_codes_write_nothing_and_leave_the_context_usable(ctx, srs):
    beta, dev_srs = srs
    INVALID, MISMATCH, UNSUPPORTED, TOO_SMALL = 1, 5, 6, 9
    size_t, u32 = C.c_size_t, C.c_uint32
    lib = ffi.lib()
    rng = np.random.default_rng(1640)
    cols, cycles, sigma, log_block = 2, 128, 6, 4
    rows = cycles >> (sigma - log_block)
    total = cols * rows
    source = ctx.onehot(make_indices(rng, cols, cycles, 16), 16)
    odd_source = ctx.onehot(make_indices(rng, 1, 126, 16), 16)  # 126 cycles in rows of 4
    ints = ctx.ints(rng.integers(1, 2**62, size=cycles, dtype=np.uint64))
    odd_ints = ctx.ints(np.arange(1, 127, dtype=np.uint64))
    small_srs = ctx.srs_upload(ffi.host_dory_g1_normalise(O.srs_setup_from_secret(beta, 32), 1))
    _, sentinel = progression(G1, 12345, 678, total)  # valid points, none normalised, none the identity
    out = ctx.dory_vec_upload(ffi.DORY_KIND_G1, sentinel)
    g2v = ctx.dory_state_alloc(ffi.DORY_KIND_G2, total)
    frv = ctx.dory_state_alloc(ffi.DORY_KIND_FR, total)
    other = ffi.Context(0)
    foreign = other.dory_state_alloc(ffi.DORY_KIND_G1, total)

    def onehot(dst, src=source, first_poly=0, n_polys=cols, sg=sigma, lb=log_block, ls=0, out_first=0, srs_h=dev_srs.h, ctx_h=ctx.h):
        return lib.jolt_dory_hints_onehot_am(ctx_h, srs_h, src.h if src else None, size_t(first_poly), size_t(n_polys), u32(sg), u32(lb), u32(ls), dst, size_t(out_first))

    def dense_rows(dst, values=ints, sg=sigma, lb=log_block, out_first=0, srs_h=dev_srs.h, ctx_h=ctx.h):
        return lib.jolt_dory_hints_rows_am(ctx_h, srs_h, values.h if values else None, u32(sg), u32(lb), dst, size_t(out_first))

    assert onehot(out.h, sg=3) == UNSUPPORTED and dense_rows(out.h, sg=3) == UNSUPPORTED   # sigma < log_block
    assert onehot(out.h, lb=4, ls=5) == INVALID                                            # log_stride > log_block
    assert onehot(out.h, lb=3, sg=5) == INVALID                                            # 16 addresses in blocks of 8
    assert onehot(out.h, lb=4, ls=1) == INVALID                                            # 16 addresses, stride 2, blocks of 16
    assert onehot(out.h, src=odd_source, n_polys=1) == INVALID                             # C = 4 does not divide 126
    assert dense_rows(out.h, values=odd_ints) == INVALID
    assert onehot(out.h, sg=11, lb=9) == TOO_SMALL and dense_rows(out.h, sg=11, lb=9) == TOO_SMALL  # 2^11 bases of 1024
    assert onehot(out.h, srs_h=small_srs.h) == TOO_SMALL and dense_rows(out.h, srs_h=small_srs.h) == TOO_SMALL
    assert onehot(out.h, out_first=1) == INVALID and onehot(out.h, out_first=2**64 - 1) == INVALID  # a view that does not hold the result
    assert dense_rows(out.h, out_first=total - rows + 1) == INVALID
    assert onehot(g2v.h) == INVALID and onehot(frv.h) == INVALID and onehot(foreign.h) == INVALID and onehot(None) == INVALID
    assert dense_rows(g2v.h) == INVALID and dense_rows(frv.h) == INVALID and dense_rows(foreign.h) == INVALID and dense_rows(None) == INVALID
    assert onehot(out.h, first_poly=1, n_polys=cols) == INVALID and onehot(out.h, first_poly=2**64 - 1, n_polys=2) == INVALID
    assert onehot(out.h, src=None) == INVALID and onehot(out.h, srs_h=None) == INVALID and onehot(out.h, ctx_h=None) == INVALID
    assert dense_rows(out.h, values=None) == INVALID and dense_rows(out.h, srs_h=None) == INVALID and dense_rows(out.h, ctx_h=None) == INVALID

    # ---- the fold
    T = cycles
    dense = [ctx.upload(rand_fr(T, 1641))]
    left, short_left = ctx.upload(rand_fr(rows, 1642)), ctx.upload(rand_fr(rows // 2, 1643))
    gamma, dgamma = rand_fr(cols, 1644), rand_fr(1, 1645)
    osc, dsc = ffi.fr(gamma).reshape(-1, 4), ffi.fr(dgamma).reshape(-1, 4)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    result = C.c_void_p(0xDEAD)

    def fold(srcs=(source,), lb=log_block, ls=0, sg=sigma, lt=left, res=C.byref(result), ctx_h=ctx.h):
        hs = (C.c_void_p * 1)(*[s.h for s in srcs])
        ds = (C.c_void_p * 1)(dense[0].h)
        return lib.jolt_dory_fold_rows_grid_am(ctx_h, hs, size_t(len(srcs)), p(osc), ds, size_t(1), p(dsc), u32(lb), u32(ls), u32(sg), lt.h if lt else None, res)

    assert fold(sg=3) == UNSUPPORTED
    assert fold(lb=4, ls=5) == INVALID
    assert fold(lb=3, sg=5) == INVALID                # source->k too large for the block
    assert fold(lb=12, ls=0, sg=12) == UNSUPPORTED    # log_k > 8, the limit of jolt_dory_fold_rows_grid
    assert fold(srcs=(odd_source,)) == INVALID        # C = 4 does not divide 126
    assert fold(lt=short_left) == MISMATCH            # left of the wrong length
    assert fold(lt=None) == INVALID and fold(res=None) == INVALID and fold(ctx_h=None) == INVALID
    assert result.value == 0xDEAD
    # nothing was enqueued: the destination holds its bytes; then valid calls on the same context
    assert np.array_equal(out.download(), sentinel)
    assert np.array_equal(foreign.download(), np.stack([IDENT] * total))
    assert dense_rows(out.h, out_first=total - rows) == 0
    got = out.download()
    assert np.array_equal(got[:total - rows], sentinel[:total - rows]) and all(np.array_equal(e[8:12], ONE) for e in got[total - rows:])
    assert onehot(out.h) == 0
    assert all(np.array_equal(e, IDENT) or np.array_equal(e[8:12], ONE) for e in out.download())
    assert fold() == 0 and result.value not in (0, 0xDEAD)
    ffi.Table(ctx, result).free()
    foreign.free()
    other.close()
    for v in (out, g2v, frv, source, odd_source, ints, odd_ints, small_srs, left, short_left, dense[0]):
        v.free()


# ------------------------------------------------------------------------------------------------------ commit, then open
N_SETUP = 32


@pytest.fixture(scope="module")
def bases():
    a0, ad, b0, bd, kh1, kh2 = rand_ints(6, 1410)
    kg1, gamma1 = progression(G1, a0, ad, N_SETUP)
    kg2, gamma2 = progression(G2, b0, bd, N_SETUP)
    return dict(kg1=kg1, gamma1=gamma1, kg2=kg2, gamma2=gamma2, kh1=kh1, h1=G1.point(kh1), kh2=kh2, h2=G2.point(kh2, rep=3))


def test_commit_to_open_address_major_with_nothing_uploaded_in_between(ctx, bases):
    """The instance of test_gpu_dory_commit.py::test_commit_to_open_with_nothing_uploaded_in_between (log_t = 6, log_k = 4, sigma = nu = 5, five one-hot columns and
    one dense) committed and opened address-major: every hint has 32 rows of C = 2 cycles; DoryOpening runs unchanged over the hints."""
    import dory_open_model as OM
    import pairing_model as PM
    from jolt_amd.dory_commit import DoryWitnessCommitment
    from jolt_amd.dory_open import DorySetup
    from test_gpu_dory_open import check_message, run_opening
    from test_gpu_dory_opening import joint_dense_table, make_batch
    log_t, log_k, sigma, nu = 6, 4, 5, 5
    rows, n, T = 1 << nu, 1 << sigma, 1 << log_t
    per_row = 1 << (sigma - log_k)
    batch = make_batch(log_t, log_k, n_dense=1, seed=1300)
    K = batch["k"]
    kg1, kg2, kh1, kh2 = bases["kg1"][:n], bases["kg2"][:n], bases["kh1"], bases["kh2"]
    setup = DorySetup(ctx, bases["gamma1"], bases["gamma2"], bases["h1"], bases["h2"])
    dev_srs = ctx.srs_upload(bases["gamma1"][:n])
    srcs = [ctx.onehot(i, K) for i in batch["idx"]]
    dense_ints = ctx.ints(batch["dense_ints"][0])
    commitment = DoryWitnessCommitment(setup, dev_srs, srcs, [dense_ints], sigma, order="address_major", log_k=log_k)
    assert [r for _, _, r in commitment.hints] == [rows] * 6
    # ---- tier 1 and tier 2 from the definition: the logarithm of every hint element, then of <hint, Gamma2>
    columns = np.concatenate(batch["idx"], axis=0)
    hint_logs = []
    for col in columns:
        hint_logs.append([sum(kg1[(j << log_k) + int(col[r * per_row + j])] for j in range(per_row) if col[r * per_row + j] != 0xFF) % R for r in range(rows)])
    hint_logs.append([sum(int(batch["dense_ints"][0][r * per_row + j]) * kg1[j << log_k] for j in range(per_row)) % R for r in range(rows)])
    for (vec, first, count), logs in zip(commitment.hints, hint_logs):
        got = vec.download(first, count)
        for i in range(count):
            assert G1.same(got[i], logs[i]) if logs[i] else np.array_equal(got[i], IDENT)
        assert all(np.array_equal(e, IDENT) if lg == 0 else np.array_equal(e[8:12], ONE) for e, lg in zip(got, logs))
    assert all(lg == 0 for lg in hint_logs[1])  # column 1 of the first source is cold throughout
    tier2 = commitment.commit()
    assert len(tier2) == 6
    for got, logs in zip(tier2, hint_logs):
        assert np.array_equal(got, PM.gt_to_abi(PM.expected([sum(lg * kg2[i] for i, lg in enumerate(logs)) % R], [1])))
    # ---- the opening over the same vectors
    scalars = np.concatenate([batch["gamma"], batch["dgamma"]])
    r_row, r_col = rand_fr(nu, 1301), rand_fr(sigma, 1302)
    left_host, right_host = O.eq_evals(r_row), O.eq_evals(r_col)
    left, right = ctx.upload(left_host), ctx.upload(right_host)
    dense = [ctx.upload(batch["dense"][0])]
    v_table = ctx.dory_fold_rows_grid_am(srcs, batch["gamma"], dense, batch["dgamma"], log_k, 0, sigma, left)
    cells = [int(x) for x in O.from_mont(joint_dense_table(batch))]  # cycle-major: index k * T + t
    flat = [0] * (K * T)
    for k in range(K):
        for t in range(T):
            flat[(t << log_k) + k] = cells[k * T + t]  # the address-major matrix of the same polynomial
    matrix = [flat[r * n:(r + 1) * n] for r in range(rows)]
    L, Rr = [int(x) for x in O.from_mont(left_host)], [int(x) for x in O.from_mont(right_host)]
    t_rows, combined, v, y = OM.statement(kg1, kg2, matrix, L, Rr)
    assert np.array_equal(v_table.download(), fr_ints(v))
    challenges, gamma, d = [tuple(rand_ints(2, 1310 + j)) for j in range(sigma)], rand_ints(1, 1303)[0], rand_ints(1, 1304)[0]
    proof = OM.prove(kg1, kg2, kh1, kh2, t_rows, v, L, Rr, challenges, gamma)
    inp = dict(nu=nu, sigma=sigma, hints=commitment.hints, scalars=scalars, tables=[v_table, left, right], challenges=challenges, gamma=gamma)
    vmv, rounds, final, _ = run_opening(setup, inp)
    check_message(vmv, proof["vmv"], "tta", "vmv")
    for r, ((first, second), (want_first, want_second)) in enumerate(zip(rounds, proof["rounds"])):
        check_message(first, want_first, "ttttab", ("first", r))
        check_message(second, want_second, "ttaabb", ("second", r))
    check_message(final, proof["final"], "ab", "final")
    assert OM.verify(kg1, kg2, kh1, kh2, combined, y, L, Rr, proof, challenges, gamma, d)
    commitment.close()
    assert commitment.hints == []
    for t in dense + [v_table, left, right, dense_ints] + srcs:
        t.free()
    setup.close()


def test_address_major_commitment_checks_shapes_before_anything_is_enqueued(ctx, bases):
    from jolt_amd.dory_commit import DoryWitnessCommitment
    from jolt_amd.dory_open import DorySetup
    setup = DorySetup(ctx, bases["gamma1"], bases["gamma2"], bases["h1"], bases["h2"])
    dev_srs = ctx.srs_upload(bases["gamma1"][:16])
    rng = np.random.default_rng(1650)
    source, odd = ctx.onehot(make_indices(rng, 2, 64, 4), 4), ctx.onehot(make_indices(rng, 1, 66, 4), 4)
    for kwargs in (dict(order="address_major"),                        # log_k missing
                   dict(order="address_major", log_k=5),               # sigma < log_block
                   dict(order="address_major", log_k=1),               # 4 addresses in blocks of 2
                   dict(order="address_major", log_k=2, log_extra=3),
                   dict(order="column_major", log_k=2)):
        with pytest.raises(ValueError):
            DoryWitnessCommitment(setup, dev_srs, [source], [], 4, **kwargs)
    with pytest.raises(ValueError):
        DoryWitnessCommitment(setup, dev_srs, [odd], [], 4, order="address_major", log_k=2)  # 66 cycles in rows of 4
    with pytest.raises(ValueError):
        DoryWitnessCommitment(setup, dev_srs, [source], [], 2, order="address_major", log_k=2)  # 64 rows against 32 Gamma2 bases
    commitment = DoryWitnessCommitment(setup, dev_srs, [source], [], 4, order="address_major", log_k=2)
    assert [r for _, _, r in commitment.hints] == [16, 16]
    commitment.close()
    for v in (source, odd):
        v.free()
    setup.close()
