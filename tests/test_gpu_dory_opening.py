"""GPU parity: the Dory opening ahead of the pairing rounds (dory.hip) -- jolt_dory_fold_rows_grid, the lazy vector-matrix product
(RlcSource::fold_rows over TraceOpeningPoly, crates/jolt-kernels/src/optimized/opening.rs:439-511), and jolt_dory_combine_hints
(DoryScheme::combine_hints, crates/jolt-dory/src/scheme.rs:325-360) -- against the CPU oracle and Python integers.  Field results are compared
bit for bit, points as group elements; nothing on the checking side comes from the library, except the one device-versus-device cross-check
of the fold at scale, which says so."""
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


# ---------------------------------------------------------------------------------------------------------------- inputs
def make_indices(rng, n_polys, T, k, wide, cold=0.4):
    idx = rng.integers(0, k, size=(n_polys, T)).astype(np.uint16 if wide else np.uint8)
    idx[rng.random((n_polys, T)) < cold] = 0xFFFF if wide else 0xFF
    return idx


def make_batch(log_t, log_k, n_dense, seed, k=None, wide=False):
    """two sources with 3 + 2 columns, 40 % cold; column 1 of the first is cold throughout, column 0 of the second is hot at address k - 1 on every cycle;
    dense columns of i64 values with negative and zero entries"""
    rng = np.random.default_rng(seed)
    T = 1 << log_t
    k = k if k is not None else 1 << log_k
    a, b = make_indices(rng, 3, T, k, wide), make_indices(rng, 2, T, k, wide)
    a[1, :] = 0xFFFF if wide else 0xFF
    b[0, :] = k - 1
    dense_ints = []
    for d in range(n_dense):
        v = rng.integers(-2**63, 2**63, size=T, dtype=np.int64)
        v[rng.random(T) < 0.25] = 0
        v[0], v[T - 1] = -1, -2**63
        dense_ints.append(v)
    gamma = rand_fr(5, seed + 1)
    dgamma = rand_fr(n_dense, seed + 2)
    return dict(log_t=log_t, log_k=log_k, k=k, wide=wide, idx=[a, b], dense_ints=dense_ints, dense=[O.fr_from_i64(v) for v in dense_ints], gamma=gamma, dgamma=dgamma)


def joint_dense_table(batch):
    """the joint polynomial over the 2^log_k x T grid, index k * T + j: the oracle's baseline_grid_joint for 8-bit indices (0xFF = cold); for 16-bit indices from
    the definition, Python integers mod r, out[hot * T + j] += gamma_p, dense columns on address 0"""
    K, T = 1 << batch["log_k"], 1 << batch["log_t"]
    idx = np.concatenate(batch["idx"], axis=0)
    if not batch["wide"]:
        return O.baseline_grid_joint(idx, K, batch["gamma"], batch["dense"], batch["dgamma"])
    g = O.from_mont(batch["gamma"])
    dg = O.from_mont(batch["dgamma"]) if len(batch["dense_ints"]) else []
    cells = {}
    for p in range(idx.shape[0]):
        for j in np.nonzero(idx[p] != 0xFFFF)[0]:
            pos = int(idx[p, j]) * T + int(j)
            cells[pos] = (cells.get(pos, 0) + g[p]) % R
    for d, col in enumerate(batch["dense_ints"]):
        for j in range(T):
            cells[j] = (cells.get(j, 0) + dg[d] * int(col[j])) % R
    out = O.fr_array(K * T)
    pos = sorted(cells)
    out[pos] = O.to_mont([cells[q] for q in pos])
    return out


def fold_dense_definition(M, left, sigma):
    """out[c] = sum_r left[r] * M[r][c] over the table reshaped to 2^nu x 2^sigma, with the oracle's field operations"""
    cols = 1 << sigma
    rows = M.shape[0] // cols
    acc = O.fr_array(cols)
    for r in range(rows):
        if not left[r].any():
            continue
        acc = O.fr_add(acc, O.fr_mul(M[r * cols:(r + 1) * cols], np.ascontiguousarray(np.broadcast_to(left[r], (cols, 4)))))
    return acc


def device_fold(ctx, batch, sigma, left):
    srcs = [ctx.onehot(i, batch["k"]) for i in batch["idx"]]
    dense = [ctx.upload(d) for d in batch["dense"]]
    lt = ctx.upload(left)
    out = ctx.dory_fold_rows_grid(srcs, batch["gamma"], dense, batch["dgamma"], batch["log_k"], sigma, lt)
    got = out.download()
    for t in dense + [lt, out]:
        t.free()
    for s in srcs:
        s.free()
    return got


# ------------------------------------------------------------------------------------------------------------------ 1
FOLD_SHAPES = [(6, 4, 5, None, False), (6, 4, 0, None, False), (6, 4, 10, None, False), (6, 8, 7, 200, False), (10, 4, 7, None, False), (12, 8, 10, 256, True)]


@pytest.mark.parametrize("case", range(len(FOLD_SHAPES)))
def test_fold_matches_the_dense_definition(ctx, case):
    log_t, log_k, sigma, k, wide = FOLD_SHAPES[case]
    batch = make_batch(log_t, log_k, n_dense=case % 3, seed=300 + case, k=k, wide=wide)
    if wide:
        assert any((i == 255).any() for i in batch["idx"])
    M = joint_dense_table(batch)
    nu = log_k + log_t - sigma
    single = O.fr_array(1 << nu)
    single[(1 << nu) // 3] = rand_fr(1, 77)[0]
    for name, left in (("random", rand_fr(1 << nu, 400 + case)), ("one row", single)):
        got = device_fold(ctx, batch, sigma, left)
        assert got.shape == (1 << sigma, 4)
        assert np.array_equal(got, fold_dense_definition(M, left, sigma)), (FOLD_SHAPES[case], name)


def test_fold_with_dense_columns_only(ctx):
    """n_sources = 0: two dense columns, sigma on both sides of log_t"""
    batch = make_batch(6, 4, n_dense=2, seed=350)
    batch["idx"], batch["gamma"] = [], O.fr_array(0)
    K, T = 16, 64
    M = O.fr_array(K * T)
    M[:T] = O.fr_add(O.fr_mul(batch["dense"][0], np.ascontiguousarray(np.broadcast_to(batch["dgamma"][0], (T, 4)))),
                     O.fr_mul(batch["dense"][1], np.ascontiguousarray(np.broadcast_to(batch["dgamma"][1], (T, 4)))))
    for sigma in (3, 5, 8):
        left = rand_fr(1 << (10 - sigma), 360 + sigma)
        assert np.array_equal(device_fold(ctx, batch, sigma, left), fold_dense_definition(M, left, sigma)), sigma


# ------------------------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("shape", [(6, 4, 5), (10, 4, 7), (6, 4, 8)])
def test_fold_satisfies_the_references_identities(ctx, shape):
    """left = eq(r_row, .): the fold is the joint table bound in its top nu variables, and its inner product with eq(r_col, .) is the joint polynomial at
    r_row || r_col (fold_rows_matches_dense, crates/jolt-poly/src/one_hot.rs:268, at the batch level)"""
    log_t, log_k, sigma = shape
    batch = make_batch(log_t, log_k, n_dense=1, seed=500 + sigma)
    joint = joint_dense_table(batch)
    nu = log_k + log_t - sigma
    r_row, r_col = rand_fr(nu, 510), rand_fr(sigma, 511)
    got = device_fold(ctx, batch, sigma, O.eq_evals(r_row))
    bound = joint
    for i in range(nu):
        bound = O.bind_high_to_low(bound, r_row[i])
    assert np.array_equal(got, bound)
    weights = O.eq_evals(r_col)
    acc = O.fr_array(1)
    for c in range(1 << sigma):
        acc = O.fr_add(acc, O.fr_mul(got[c:c + 1], weights[c:c + 1]))
    assert np.array_equal(acc[0], O.poly_evaluate(joint, np.concatenate([r_row, r_col])))


# ------------------------------------------------------------------------------------------------------------------ 3
def workload_onehot_columns():
    """the one-hot columns workload.build() commits, per source"""
    from jolt_amd import workload
    tables, members = workload.build(6)[:2]
    return [len(ms.tables) - 1 for ms in members if ms.uniform is not None and all(tables[t].kind == "onehot" for t in ms.tables[1:])]


def test_fold_at_scale_without_the_grid():
    log_t, log_k, sigma = 20, 4, 12
    T, K, nu = 1 << log_t, 1 << log_k, log_k + log_t - sigma
    counts = workload_onehot_columns()
    assert sum(counts) >= 36 and len(counts) <= 4
    rng = np.random.default_rng(2026)
    idx = [make_indices(rng, n, T, K, False, cold=0.1) for n in counts]
    dense_ints = rng.integers(-2**63, 2**63, size=T, dtype=np.int64)
    dense_ints[rng.random(T) < 0.25] = 0
    gamma, dgamma, left = rand_fr(sum(counts), 601), rand_fr(1, 602), rand_fr(1 << nu, 603)
    ctx = ffi.Context(0)  # peak_bytes is a high-water mark over the life of a context: a context of its own
    try:
        srcs = [ctx.onehot(i, K) for i in idx]
        dense = [ctx.upload(O.fr_from_i64(dense_ints))]
        lt = ctx.upload(left)
        ctx.synchronize()
        ctx.trim()
        before = ctx.memory_stats()
        out = ctx.dory_fold_rows_grid(srcs, gamma, dense, dgamma, log_k, sigma, lt)
        got = out.download()
        after = ctx.memory_stats()
        grid_bytes = 32 << (log_k + log_t)
        growth = after["peak_bytes"] - before["peak_bytes"]
        print(f"fold at scale: peak_bytes {before['peak_bytes']} -> {after['peak_bytes']} (+{growth}); dense joint polynomial {grid_bytes}")
        assert growth < grid_bytes // 8, (before, after)

        # the sparse definition in Python integers: the 256 cycles of a column, one left entry each
        gi, dgi, li = O.from_mont(gamma), O.from_mont(dgamma)[0], O.from_mont(left)
        allidx = np.concatenate(idx, axis=0)
        cols = sorted(set([0, (1 << sigma) - 1] + [int(c) for c in np.random.default_rng(604).integers(0, 1 << sigma, size=64)]))
        want = []
        for c in cols:
            acc = 0
            for m in range(T >> sigma):
                j = (m << sigma) | c
                for p in range(allidx.shape[0]):
                    h = int(allidx[p, j])
                    if h != 0xFF:
                        acc += gi[p] * li[(h << (log_t - sigma)) + m]
                acc += dgi * li[m] * int(dense_ints[j])
            want.append(acc % R)
        assert np.array_equal(got[cols], O.to_mont(want))

        # device versus device: the materialised route, jolt_grid_joint_polynomial then jolt_address_fold with weights = left (2^nu rows of 2^sigma columns)
        grid = ctx.grid_joint_polynomial(srcs, gamma, dense, dgamma, log_k)
        ref = ctx.address_fold(grid, lt)
        assert np.array_equal(got, ref.download())
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------------------------ 4
def point_pool(n, seed):
    g = O.g1_generator()
    return np.stack([O.g1_scalar_mul(g, s) for s in rand_fr(n, seed)])


def oracle_combine_row(hints, scalars, row):
    acc = O.g1_identity()
    for h, s in zip(hints, scalars):
        if row < h.shape[0]:
            acc = O.g1_add(acc, O.g1_scalar_mul(h[row], s))
    return acc


def plant_special_rows(hints, pool, base):
    """rows base .. base + 3 of the first two hints (equal scalars): all identity; the same point twice; P and -P; P and -P beside the other hints' points"""
    ident = O.g1_identity()
    for h in hints:
        if h.shape[0] > base:
            h[base] = ident
    if len(hints) >= 2 and hints[1].shape[0] > base + 3:
        hints[0][base + 1], hints[1][base + 1] = pool[0], pool[0]
        hints[0][base + 2], hints[1][base + 2] = pool[1], O.g1_neg(pool[1])
        for h in hints[2:]:
            if h.shape[0] > base + 2:
                h[base + 2] = ident
        hints[0][base + 3], hints[1][base + 3] = pool[2], O.g1_neg(pool[2])


def real_hints(ctx, log_t, log_k, sigma, n_onehot, seed, beta_seed):
    """hints of n_onehot one-hot columns and one i64 dense column from the commit entry points over an SRS of 2^sigma bases from a known secret"""
    T, K, width = 1 << log_t, 1 << log_k, 1 << sigma
    rng = np.random.default_rng(seed)
    idx = make_indices(rng, n_onehot, T, K, False)
    dense_ints = rng.integers(-2**63, 2**63, size=T, dtype=np.int64)
    dense_ints[rng.random(T) < 0.25] = 0
    beta = rand_fr(1, beta_seed)[0]
    srs = ctx.srs_setup_from_secret(beta, width, O.g1_generator())
    oh = ctx.onehot(idx, K)
    hints = [ffi.dory_onehot_hint(ctx.dory_commit_onehot(srs, oh, p, width)) for p in range(n_onehot)]
    hints.append(np.array(ctx.dory_commit_rows(srs, ctx.ints(dense_ints), width)))
    oh.free()
    return idx, dense_ints, beta, hints


@pytest.mark.parametrize("rows,n_hints", [(1, 1), (16, 3), (1024, 5), (8192, 40)])
def test_combine_matches_the_oracle(ctx, rows, n_hints):
    pool = point_pool(24, 700 + n_hints)
    rng = np.random.default_rng(rows)
    if (rows, n_hints) == (1024, 5):
        # three one-hot hints of 16 * 64 rows and the dense hint of 64 rows (a sixteenth) from real commitments: log_t = 10, log_k = 4, sigma = 4
        idx, _, _, hints = real_hints(ctx, 10, 4, 4, 3, seed=710, beta_seed=711)
        host_srs = O.srs_setup_from_secret(rand_fr(1, 711)[0], 16)
        for p, (k, chunk) in enumerate([(0, 0), (7, 13), (15, 63)]):  # the transposed entry is the oracle's chunk commitment
            want = O.dory_onehot_chunk(host_srs, idx[p, chunk * 16:(chunk + 1) * 16], 16)
            assert O.g1_eq(hints[p][k * 64 + chunk], want[k])
        hints.insert(1, pool[rng.integers(0, len(pool), size=rows // 2)].copy())  # and one of half the rows
        assert [h.shape[0] for h in hints] == [1024, 512, 1024, 1024, 64]
    else:
        lengths = [rows] * n_hints
        if n_hints >= 3:
            lengths[-2], lengths[-1] = max(rows // 2, 1), max(rows // 16, 1)
        hints = [pool[rng.integers(0, len(pool), size=n)].copy() for n in lengths]
    scalars = rand_fr(n_hints, 720 + n_hints)
    if n_hints >= 2:
        scalars[1] = scalars[0]
    if n_hints >= 5:
        scalars[2], scalars[3], scalars[4] = O.to_mont([0, 1, R - 1])
    if rows >= 16:
        plant_special_rows(hints, pool, 2)
    got = ctx.dory_combine_hints(hints, scalars)
    assert got.shape == (rows, 12)
    if rows <= 1024:
        check = range(rows)
    else:
        check = sorted(set([0, 1, 2, 3, 4, 5, rows // 16 - 1, rows // 16, rows // 2 - 1, rows // 2, rows - 1] + [int(r) for r in np.random.default_rng(730).integers(0, rows, size=16)]))
    for r in check:
        assert O.g1_eq(got[r], oracle_combine_row(hints, scalars, r)), (rows, n_hints, r)
    if rows >= 16:
        assert O.g1_is_identity(got[2])


# ------------------------------------------------------------------------------------------------------------------ 5
def test_fold_and_combined_hints_commit_to_the_same_vector(ctx):
    """MSM(srs[..2^sigma], fold) == sum_r left[r] * combined[r]: the vector-matrix product is consistent with the row commitments, which the Dory verifier's
    first message rests on.  A wrong gamma order or a wrong transpose fails here."""
    log_t, log_k, sigma = 10, 4, 7
    nu = log_k + log_t - sigma
    idx, dense_ints, beta, hints = real_hints(ctx, log_t, log_k, sigma, 5, seed=800, beta_seed=801)
    assert [h.shape[0] for h in hints] == [1 << nu] * 5 + [1 << (log_t - sigma)]
    gamma, dgamma, left = rand_fr(5, 802), rand_fr(1, 803), rand_fr(1 << nu, 804)
    combined = ctx.dory_combine_hints(hints, np.concatenate([gamma, dgamma]))
    srcs = [ctx.onehot(idx[:3], 1 << log_k), ctx.onehot(idx[3:], 1 << log_k)]
    dense = [ctx.upload(O.fr_from_i64(dense_ints))]
    lt = ctx.upload(left)
    fold = ctx.dory_fold_rows_grid(srcs, gamma, dense, dgamma, log_k, sigma, lt).download()
    lhs = O.kzg_commit(fold, O.srs_setup_from_secret(beta, 1 << sigma))
    rhs = O.g1_identity()
    for r in range(1 << nu):
        rhs = O.g1_add(rhs, O.g1_scalar_mul(combined[r], left[r]))
    assert O.g1_eq(lhs, rhs)


# ------------------------------------------------------------------------------------------------------------------ 6
def test_argument_checks_enqueue_nothing(ctx):
    batch = make_batch(6, 4, n_dense=1, seed=900)
    srcs = [ctx.onehot(i, 16) for i in batch["idx"]]
    dense = [ctx.upload(batch["dense"][0])]
    left = ctx.upload(rand_fr(1 << 5, 901))
    g, dg = batch["gamma"], batch["dgamma"]

    def refused(status, *args):
        with pytest.raises(ffi.JoltError) as e:
            ctx.dory_fold_rows_grid(*args)
        assert e.value.status == status, e.value

    refused(1, srcs, g, dense, dg, 4, 11, left)                                   # sigma > log_k + log_t
    assert "sigma" in ffi.lib().jolt_last_error(ctx.h).decode()
    refused(1, srcs, g, dense, dg, 3, 5, ctx.upload(rand_fr(1 << 4, 902)))       # source->k = 16 > 2^3
    refused(5, srcs, g, dense, dg, 4, 5, ctx.upload(rand_fr(1 << 4, 903)))       # left of the wrong length
    refused(5, srcs, g, [ctx.upload(rand_fr(32, 904))], dg, 4, 5, left)          # a dense column of the wrong length
    other = ctx.onehot(make_indices(np.random.default_rng(5), 2, 128, 16, False), 16)
    refused(5, [srcs[0], other], g, dense, dg, 4, 5, left)                        # sources with different cycle counts
    refused(6, srcs * 3, np.concatenate([g, g, g]), dense, dg, 4, 5, left)        # more than 4 sources
    refused(6, srcs, g, dense * 9, np.concatenate([dg] * 9), 4, 5, left)          # more than 8 dense columns
    refused(6, [], O.fr_array(0), [], O.fr_array(0), 4, 5, left)                  # no column at all
    with pytest.raises(ffi.JoltError) as e:                                       # empty hints
        ctx.dory_combine_hints([], [])
    assert e.value.status == 1
    bad = np.full((1, 4), 2**64 - 1, dtype=np.uint64)
    with pytest.raises(ffi.JoltError) as e:                                       # a scalar that is no field element
        ctx.dory_combine_hints([point_pool(1, 9)], bad)
    assert e.value.status == 1
    # the context is usable for the next call, and that call is right
    M = joint_dense_table(batch)
    want = fold_dense_definition(M, left.download(), 5)
    assert np.array_equal(ctx.dory_fold_rows_grid(srcs, g, dense, dg, 4, 5, left).download(), want)
    p = point_pool(2, 10)
    s = rand_fr(1, 905)
    assert O.g1_eq(ctx.dory_combine_hints([p[:1], p[1:]], np.stack([s[0], s[0]]))[0], O.g1_scalar_mul(O.g1_add(p[0], p[1]), s[0]))
