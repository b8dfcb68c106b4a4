"""GPU parity: the witness commitment on the device -- jolt_dory_hints_onehot / jolt_dory_hints_rows (row commitments written normalised, in hint order, into
resident G1 vectors) and jolt_amd/dory_commit.py (every tier-2 commitment from one product batch, the hints consumed by DoryOpening as they are).  Expected values
come from the definition through the oracle: over the bases beta^j G a row commitment is (sum_j v_j beta^j) G, over planted progressions it is a discrete
logarithm.  Group equality with the host-pointer entries is checked in addition.  Points are compared as group elements, the normalised representative and the
neutral element bit for bit; no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from dory_groups import G1, G2, R, fr_ints, progression, rand_ints
from jolt_amd import ffi
from util import rand_fr

pytestmark = pytest.mark.gpu
SRS_LEN = 64
IDENT = O.g1_identity()
ONE = IDENT[0:4]  # the Montgomery one of Fq


@pytest.fixture(scope="module")
def ctx():
    c = ffi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def srs(ctx):
    beta = rand_fr(1, 1400)[0]
    return beta, ctx.srs_setup_from_secret(beta, SRS_LEN, O.g1_generator())


def eval_point(beta, ints):
    """(sum_j v_j beta^j) * G: the commitment to a row over the bases beta^j G, from field arithmetic alone (tests/test_gpu_dory.py::_eval_point)"""
    return O.g1_scalar_mul(O.g1_generator(), O.kzg_eval_univariate(O.to_mont([v % R for v in ints]), beta))


def onehot_definition(beta, column, width, row, chunk):
    """hint[row * chunks + chunk] of a hot-index column: the sum of the bases of the chunk's cycles whose hot address is `row`"""
    return eval_point(beta, [int(x) for x in (column[chunk * width:(chunk + 1) * width] == row)])


def assert_hint_element(got, want, what):
    """a normalised point (or bit for bit the neutral element) that is on the curve and equals `want` as a group element"""
    if O.g1_is_identity(want):
        assert np.array_equal(got, IDENT), what
    else:
        assert np.array_equal(got[8:12], ONE), what
        assert O.g1_on_curve(got) and O.g1_eq(got, want), what


def assert_matches_host_entry(ctx, dev_srs, source, width, hints, first_poly=0):
    """column by column the group elements of dory_onehot_hint(dory_commit_onehot(...)); hints: (columns, k * chunks, 12)"""
    for p in range(hints.shape[0]):
        ref = ffi.dory_onehot_hint(ctx.dory_commit_onehot(dev_srs, source, first_poly + p, width))
        assert ref.shape[0] == hints.shape[1]
        for i in range(ref.shape[0]):
            assert O.g1_is_identity(ref[i]) == (not hints[p, i, 8:12].any()) and (O.g1_is_identity(ref[i]) or O.g1_eq(hints[p, i], ref[i])), (p, i)


def make_indices(rng, n_polys, cycles, k, empty_row, dtype=np.uint8):
    cold = 0xFFFF if dtype == np.uint16 else 0xFF
    idx = rng.integers(0, k, size=(n_polys, cycles)).astype(dtype)
    idx[idx == empty_row] = (empty_row + 1) % k  # one row is never hot in any column
    idx[rng.random((n_polys, cycles)) < 0.25] = cold
    return idx


# ------------------------------------------------------------------------------------------------------ one-hot columns
def test_onehot_hints_8_bit_indices_into_a_view(ctx, srs):
    beta, dev_srs = srs
    k, cycles, width, cols, empty_row, out_first, tail = 16, 64, 32, 3, 11, 5, 4
    chunks = cycles // width
    idx = make_indices(np.random.default_rng(1401), cols, cycles, k, empty_row)
    source = ctx.onehot(idx, k)
    total = cols * k * chunks
    out = ctx.dory_state_alloc(ffi.DORY_KIND_G1, out_first + total + tail)
    assert ctx.dory_hints_onehot(dev_srs, source, out, chunk_width=width, out_first=out_first) == total
    got = out.download()
    assert all(np.array_equal(got[i], IDENT) for i in list(range(out_first)) + list(range(out_first + total, out_first + total + tail)))  # nothing outside the view
    hints = got[out_first:out_first + total].reshape(cols, k * chunks, 12)
    n_ident = 0
    for p in range(cols):
        for row in range(k):
            for chunk in range(chunks):
                want = onehot_definition(beta, idx[p], width, row, chunk)
                assert_hint_element(hints[p, row * chunks + chunk], want, (p, row, chunk))
                n_ident += O.g1_is_identity(want)
        assert all(np.array_equal(hints[p, empty_row * chunks + chunk], IDENT) for chunk in range(chunks))
    assert n_ident >= cols * chunks  # the empty row at least
    assert_matches_host_entry(ctx, dev_srs, source, width, hints)
    out.free()
    source.free()


def test_onehot_hints_16_bit_indices(ctx, srs):
    """K = 300 over 128 cycles: 16-bit hot addresses, most rows empty; rows 0, 255, 256 and 299 are hot in both chunks"""
    beta, dev_srs = srs
    k, cycles, width, cols, empty_row = 300, 128, 64, 2, 17
    chunks = cycles // width
    rng = np.random.default_rng(1402)
    idx = make_indices(rng, cols, cycles, k, empty_row, np.uint16)
    sample = [0, 255, 256, 299]
    for p in range(cols):
        for chunk in range(chunks):
            for s, row in enumerate(sample):
                idx[p, chunk * width + 7 * s + p] = row
    source = ctx.onehot(idx, k)
    total = cols * k * chunks
    out = ctx.dory_state_alloc(ffi.DORY_KIND_G1, total)
    assert ctx.dory_hints_onehot(dev_srs, source, out, chunk_width=width) == total
    hints = out.download().reshape(cols, k * chunks, 12)
    for p in range(cols):
        for row, chunk in [(row, 0) for row in sample] + [(row, 1) for row in range(k)]:
            want = onehot_definition(beta, idx[p], width, row, chunk)
            assert_hint_element(hints[p, row * chunks + chunk], want, (p, row, chunk))
            assert row not in sample or not O.g1_is_identity(want)
        assert all(np.array_equal(hints[p, empty_row * chunks + chunk], IDENT) for chunk in range(chunks))
        # every element is normalised or the neutral element, whether or not the oracle was asked about it
        assert all(np.array_equal(e, IDENT) or np.array_equal(e[8:12], ONE) for e in hints[p])
    assert_matches_host_entry(ctx, dev_srs, source, width, hints)
    out.free()
    source.free()


def test_onehot_hints_in_forced_batches(ctx, srs):
    """12 windows in launch sets of 3: the cuts fall inside a column and a launch set spans two columns.  The loop these cuts drive (bucket_batches,
    jolt_amd/csrc/dory_batches.hip.h) is also the one under jolt_dory_commit_onehot, whose own cut -- 2^26 / chunk_width chunks, no parameter moves it -- no test of
    a sensible size can reach: what changes there beside the batch length is the sink, which every host-entry comparison of this file runs."""
    beta, dev_srs = srs
    k, cycles, width, cols, empty_row = 16, 128, 32, 3, 3
    chunks = cycles // width
    idx = make_indices(np.random.default_rng(1403), cols, cycles, k, empty_row)
    source = ctx.onehot(idx, k)
    per = k * chunks
    whole, cut, last_two = (ctx.dory_state_alloc(ffi.DORY_KIND_G1, n) for n in (cols * per, cols * per, 2 * per))
    ctx.dory_hints_onehot(dev_srs, source, whole, chunk_width=width)
    ctx.dory_hints_onehot(dev_srs, source, cut, chunk_width=width, batch_points=3 * width)
    ctx.dory_hints_onehot(dev_srs, source, last_two, first_poly=1, n_polys=2, chunk_width=width, batch_points=3 * width)
    a, b, c = whole.download(), cut.download(), last_two.download()
    for p in range(cols):
        for row in range(k):
            for chunk in range(chunks):
                i = p * per + row * chunks + chunk
                want = onehot_definition(beta, idx[p], width, row, chunk)
                assert_hint_element(a[i], want, ("whole", p, row, chunk))
                assert_hint_element(b[i], want, ("cut", p, row, chunk))
                if p >= 1:
                    assert_hint_element(c[i - per], want, ("last two", p, row, chunk))
    for v in (whole, cut, last_two):
        v.free()
    source.free()


# ------------------------------------------------------------------------------------------------------ dense columns
def test_rows_hints_all_kinds(ctx, srs):
    beta, dev_srs = srs
    width, rows = 32, 4
    rng = np.random.default_rng(1404)
    u = rng.integers(0, 2**63, size=rows * width, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    u[width:2 * width] = 0  # an all-zero row between the others
    s = rng.integers(-2**63, 2**63, size=rows * width, dtype=np.int64)
    s[0], s[1], s[2], s[3] = -2**63, 2**63 - 1, -1, 0
    big = [int(rng.integers(0, 2**63)) * int(rng.integers(0, 2**63)) * (1 if j % 3 else -1) for j in range(rows * width)]
    big[0], big[1], big[2], big[3] = -2**127, 2**127 - 1, -1, 0
    for values, ints in ((u, ctx.ints(u)), (s, ctx.ints(s)), (big, ctx.ints(big, "i128"))):
        out = ctx.dory_state_alloc(ffi.DORY_KIND_G1, rows + 3)
        assert ctx.dory_hints_rows(dev_srs, ints, width, out, out_first=2) == rows
        got = out.download()
        assert all(np.array_equal(got[i], IDENT) for i in (0, 1, rows + 2))
        ref = ctx.dory_commit_rows(dev_srs, ints, width)
        for r in range(rows):
            assert_hint_element(got[2 + r], eval_point(beta, [int(x) for x in values[r * width:(r + 1) * width]]), r)
            assert O.g1_is_identity(ref[r]) == (not got[2 + r, 8:12].any()) and (O.g1_is_identity(ref[r]) or O.g1_eq(got[2 + r], ref[r]))
        out.free()
        ints.free()
    # an all-zero column: identities written on the device, over whatever the view held
    pts = np.stack([G1.point(7 + i) for i in range(rows)])
    out = ctx.dory_vec_upload(ffi.DORY_KIND_G1, pts)
    zeros = ctx.ints(np.zeros(rows * width, dtype=np.uint64))
    ctx.dory_hints_rows(dev_srs, zeros, width, out)
    assert all(np.array_equal(e, IDENT) for e in out.download())
    out.free()
    zeros.free()


def test_rows_hints_across_the_key_cut(ctx):
    """Integer rows into a resident view in more than one batch: 1024 rows x 4096 i128 values (the shape of tests/test_gpu_dory.py::test_rows_multiple_batches) with
    one value of magnitude 2^127, so the magnitudes take 128 bits, c = 8 gives 17 windows and a batch holds 2^26 // (17 * 4096) = 963 rows: the cut falls at row 963.
    Every row of the view equals the row jolt_dory_commit_rows gives for the same values; rows 0, 962, 963 and 1023 -- both sides of the cut -- equal p_row(beta) G."""
    beta = rand_fr(1, 1406)[0]
    width, rows = 1 << 12, 1 << 10
    dev_srs = ctx.srs_setup_from_secret(beta, width, O.g1_generator())
    rng = np.random.default_rng(1407)
    packed = np.stack([rng.integers(0, 2**64, size=rows * width, dtype=np.uint64) for _ in range(2)], axis=1)
    packed[5 * width + 9] = (0, 2**63)  # i128::MIN
    assert (2**26) // (17 * width) == 963 < rows
    ints = ctx.ints(packed, "i128")
    out = ctx.dory_state_alloc(ffi.DORY_KIND_G1, rows)
    assert ctx.dory_hints_rows(dev_srs, ints, width, out) == rows
    got = out.download()
    ref = ctx.dory_commit_rows(dev_srs, ints, width)
    assert ref.shape[0] == rows
    for r in range(rows):
        assert np.array_equal(got[r, 8:12], ONE) and O.g1_eq(got[r], ref[r]), r

    def as_int(r, j):
        v = int(packed[r * width + j, 0]) | (int(packed[r * width + j, 1]) << 64)
        return v - (1 << 128) if v >> 127 else v
    for r in (0, 962, 963, 1023):
        assert_hint_element(got[r], eval_point(beta, [as_int(r, j) for j in range(width)]), r)
    out.free()
    ints.free()
    dev_srs.free()


# ------------------------------------------------------------------------------------------------------ refusals
def test_refusals_keep_their_codes_write_nothing_and_leave_the_context_usable(ctx, srs):
    beta, dev_srs = srs
    INVALID, MISMATCH, TOO_SMALL = 1, 5, 9
    size_t = C.c_size_t
    k, cycles, width, cols = 16, 128, 32, 2
    chunks = cycles // width
    total = cols * k * chunks
    rng = np.random.default_rng(1405)
    source = ctx.onehot(make_indices(rng, cols, cycles, k, 2), k)
    odd_source = ctx.onehot(make_indices(rng, 1, 96, k, 2), k)
    ints = ctx.ints(rng.integers(1, 2**62, size=128, dtype=np.uint64))
    odd_ints = ctx.ints(np.arange(1, 97, dtype=np.uint64))  # 96 values: not a whole number of rows of 64
    _, sentinel = progression(G1, 12345, 678, total)  # valid points, none normalised, none the identity
    out = ctx.dory_vec_upload(ffi.DORY_KIND_G1, sentinel)
    g2v = ctx.dory_state_alloc(ffi.DORY_KIND_G2, total)
    frv = ctx.dory_state_alloc(ffi.DORY_KIND_FR, total)
    other = ffi.Context(0)
    foreign = other.dory_state_alloc(ffi.DORY_KIND_G1, total)

    def onehot(dst, src=source, first_poly=0, n_polys=cols, cw=width, out_first=0, batch=0, srs_h=dev_srs.h, ctx_h=ctx.h):
        return ffi.lib().jolt_dory_hints_onehot(ctx_h, srs_h, src.h if src else None, size_t(first_poly), size_t(n_polys), size_t(cw), dst, size_t(out_first), size_t(batch))

    def rows(dst, values=ints, rw=width, out_first=0, ctx_h=ctx.h):
        return ffi.lib().jolt_dory_hints_rows(ctx_h, dev_srs.h, values.h if values else None, size_t(rw), dst, size_t(out_first))

    assert onehot(g2v.h) == INVALID and onehot(frv.h) == INVALID and onehot(None) == INVALID
    assert onehot(out.h, out_first=1) == INVALID                  # one element too long
    assert onehot(out.h, out_first=2**64 - 1) == INVALID          # first + n wraps
    assert onehot(foreign.h) == INVALID                           # a vector of another context
    assert onehot(out.h, cw=24) == INVALID                        # not a power of two
    assert onehot(out.h, cw=2 * SRS_LEN) == TOO_SMALL             # 128 divides the cycle count but the SRS holds 64 bases
    assert onehot(out.h, src=odd_source, n_polys=1, cw=64) == MISMATCH  # 96 cycles in chunks of 64
    assert onehot(out.h, first_poly=1, n_polys=cols) == INVALID   # past the source
    assert onehot(out.h, first_poly=cols + 1, n_polys=0) == INVALID
    assert onehot(out.h, first_poly=2**64 - 1, n_polys=2) == INVALID
    assert onehot(out.h, batch=width + width // 2) == INVALID     # not a whole number of chunks
    assert onehot(out.h, batch=width // 2) == INVALID             # less than one chunk
    assert onehot(out.h, src=None) == INVALID and onehot(out.h, srs_h=None) == INVALID and onehot(out.h, ctx_h=None) == INVALID
    assert rows(g2v.h) == INVALID and rows(frv.h) == INVALID and rows(None) == INVALID and rows(foreign.h) == INVALID
    assert rows(out.h, out_first=total - 3) == INVALID            # 4 rows from element total - 3
    assert rows(out.h, rw=24) == INVALID
    assert rows(out.h, rw=2 * SRS_LEN) == TOO_SMALL
    assert rows(out.h, rw=64, values=odd_ints) == MISMATCH
    assert rows(out.h, values=None) == INVALID
    # nothing was enqueued: the destination holds its bytes; then valid calls on the same context
    assert np.array_equal(out.download(), sentinel)
    assert np.array_equal(foreign.download(), np.stack([IDENT] * total))
    assert rows(out.h, out_first=total - 4) == 0
    got = out.download()
    assert np.array_equal(got[:total - 4], sentinel[:total - 4]) and all(np.array_equal(e[8:12], ONE) for e in got[total - 4:])
    assert onehot(out.h) == 0
    got = out.download()
    assert all(np.array_equal(e, IDENT) or np.array_equal(e[8:12], ONE) for e in got)
    foreign.free()
    other.close()
    for v in (out, g2v, frv, source, odd_source, ints, odd_ints):
        v.free()


# ------------------------------------------------------------------------------------------------------ commit, then open
N_SETUP = 32


@pytest.fixture(scope="module")
def bases():
    a0, ad, b0, bd, kh1, kh2 = rand_ints(6, 1410)
    kg1, gamma1 = progression(G1, a0, ad, N_SETUP)
    kg2, gamma2 = progression(G2, b0, bd, N_SETUP)
    return dict(kg1=kg1, gamma1=gamma1, kg2=kg2, gamma2=gamma2, kh1=kh1, h1=G1.point(kh1), kh2=kh2, h2=G2.point(kh2, rep=3))


def test_commit_to_open_with_nothing_uploaded_in_between(ctx, bases):
    """The instance of test_gpu_dory_open.py::test_opening_of_a_committed_batch (log_t = 6, log_k = 4, sigma = nu = 5) with the hints left where the commitment
    wrote them: no hint is ever uploaded -- this test never calls dory_vec_upload for one.  Gamma1 / Gamma2 / H1 / H2 are planted progressions, so a hint element's
    logarithm is a sum of Gamma1's logarithms and a tier-2 commitment one model power."""
    import dory_open_model as OM
    import pairing_model as PM
    from jolt_amd.dory_commit import DoryWitnessCommitment
    from jolt_amd.dory_open import DorySetup
    from test_gpu_dory_open import check_message, run_opening
    from test_gpu_dory_opening import joint_dense_table, make_batch
    log_t, log_k, sigma, nu = 6, 4, 5, 5
    rows, n, T = 1 << nu, 1 << sigma, 1 << log_t
    chunks = T >> sigma
    batch = make_batch(log_t, log_k, n_dense=1, seed=1300)
    K = batch["k"]
    kg1, kg2, kh1, kh2 = bases["kg1"][:n], bases["kg2"][:n], bases["kh1"], bases["kh2"]
    setup = DorySetup(ctx, bases["gamma1"], bases["gamma2"], bases["h1"], bases["h2"])
    dev_srs = ctx.srs_upload(bases["gamma1"][:n])
    srcs = [ctx.onehot(i, K) for i in batch["idx"]]
    dense_ints = ctx.ints(batch["dense_ints"][0])
    commitment = DoryWitnessCommitment(setup, dev_srs, srcs, [dense_ints], sigma)
    assert [r for _, _, r in commitment.hints] == [rows] * 5 + [T >> sigma]
    # ---- tier 1 and tier 2 from the definition: the logarithm of every hint element, then of <hint, Gamma2>
    columns = np.concatenate(batch["idx"], axis=0)
    hint_logs = []
    for col in columns:
        hint_logs.append([sum(kg1[j] for j in range(n) if col[chunk * n + j] == row) % R for row in range(K) for chunk in range(chunks)])
    hint_logs.append([sum(int(batch["dense_ints"][0][r * n + j]) * kg1[j] for j in range(n)) % R for r in range(T >> sigma)])
    for (vec, first, count), logs in zip(commitment.hints, hint_logs):
        got = vec.download(first, count)
        for i in (0, 1, count // 2, count - 1):
            assert G1.same(got[i], logs[i])
        assert all(np.array_equal(e, IDENT) if lg == 0 else np.array_equal(e[8:12], ONE) for e, lg in zip(got, logs))
    assert any(lg == 0 for lg in hint_logs[1]) and all(lg == 0 for lg in hint_logs[1])  # column 1 of the first source is cold throughout
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
    v_table = ctx.dory_fold_rows_grid(srcs, batch["gamma"], dense, batch["dgamma"], log_k, sigma, left)
    cells = O.from_mont(joint_dense_table(batch))
    matrix = [[int(x) for x in cells[r * n:(r + 1) * n]] for r in range(rows)]
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


def test_witness_commitment_checks_shapes_before_anything_is_enqueued(ctx, bases):
    from jolt_amd.dory_commit import DoryWitnessCommitment
    from jolt_amd.dory_open import DorySetup, dory_commit_tier2
    setup = DorySetup(ctx, bases["gamma1"], bases["gamma2"], bases["h1"], bases["h2"])  # 32 bases
    dev_srs = ctx.srs_upload(bases["gamma1"][:16])
    rng = np.random.default_rng(1420)
    source = ctx.onehot(make_indices(rng, 2, 80, 4, 1), 4)
    tall = ctx.onehot(make_indices(rng, 1, 80, 16, 1), 16)
    ints, odd = ctx.ints(np.arange(1, 49, dtype=np.uint64)), ctx.ints(np.arange(1, 41, dtype=np.uint64))
    for sources, dense, sigma in (([source], [ints], 5),   # 2^sigma above the SRS
                                  ([source], [], 3 + 2),
                                  ([source], [odd], 4),    # 40 values in rows of 16
                                  ([tall], [ints], 4),     # 16 * 5 rows against 32 Gamma2 bases
                                  ([], [], 4)):            # no column at all
        with pytest.raises(ValueError):
            DoryWitnessCommitment(setup, dev_srs, sources, dense, sigma)
    cycles80 = ctx.onehot(make_indices(rng, 1, 72, 4, 1), 4)
    with pytest.raises(ValueError):
        DoryWitnessCommitment(setup, dev_srs, [cycles80], [], 4)  # 72 cycles in chunks of 16
    commitment = DoryWitnessCommitment(setup, dev_srs, [source], [ints], 4)
    assert [r for _, _, r in commitment.hints] == [20, 20, 3]
    tier2 = commitment.commit()
    assert len(tier2) == 3 and all(np.array_equal(t, dory_commit_tier2(setup, h)) for t, h in zip(tier2, commitment.hints))  # the batch against one call per column
    commitment.close()
    for v in (source, tall, ints, odd, cycles80):
        v.free()
    setup.close()
