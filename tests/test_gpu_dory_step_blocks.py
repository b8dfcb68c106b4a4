"""GPU parity: stage 8 under Dory over trace columns AND block-embedded polynomials, in both trace placements -- jolt_dory_evaluate_blocks (the blocks' claims from
one pass), jolt_dory_fold_rows_blocks_many (the block fold past eight tables), jolt_host_dory_prove_batch_blocks and DeviceWorkload(pcs="dory", dory_blocks=...,
dory_order=...) over them.

Expected values come from definitions in Python integers: a block's claim is sum_i t[i] * eq(point, index(i)) with index the top-left embedding; the fold is the
definition of tests/test_gpu_dory_rows_fr.py; the opening is held to the log-space model of tests/test_gpu_dory_step.py over the materialised embedded grids (every
hint element and proof element has a known discrete logarithm under the planted bases).  Field and GT elements bit for bit, points as group elements; no tolerance."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as O
from dory_groups import R, fr_int, fr_ints, rand_ints
from jolt_amd import ffi
from jolt_amd.workload import DeviceWorkload
from test_gpu_dory_step import LOG_K, bases, check_opening, ctx, hint_logs, oracle_claims, planted, workload_grids  # noqa: F401 -- ctx and bases are fixtures

pytestmark = pytest.mark.gpu
INVALID_ARG, SIZE_MISMATCH, UNSUPPORTED, ROUND_CHECK = 1, 5, 6, 8
CAP = "JOLT_DORY_EVAL_BLOCKS_CAP"  # workgroups per table of k_dory_eval_blocks (dory.hip)


# ---------------------------------------------------------------------------------------------- the definitions, in Python integers
def eq_at(point, index):
    """eq(point, index): point[0] on the most significant bit of index, as jolt_eq_evals indexes"""
    n, acc = len(point), 1
    for j, p in enumerate(point):
        acc = acc * (p if (index >> (n - 1 - j)) & 1 else 1 - p) % R
    return acc


def block_index(sigma_d, sigma, i):
    """jolt_host_dory_block_index: coefficient i of a block of 2^sigma_d columns, top-left in a grid of 2^sigma columns"""
    return ((i >> sigma_d) << sigma) | (i & ((1 << sigma_d) - 1))


def block_claim(table, sigma_d, sigma, point):
    """sum_i t[i] * eq(point, index(i)) over the nu + sigma coordinates of the grid-order point"""
    return sum(x * eq_at(point, block_index(sigma_d, sigma, i)) for i, x in enumerate(table) if x) % R


def embedded_grid(table, sigma_d, nu, sigma):
    grid = [0] * (1 << (nu + sigma))
    for i, x in enumerate(table):
        grid[block_index(sigma_d, sigma, i)] = x
    return grid


def sigma_choices(m, nu, sigma):
    """ceil(m / 2), 0 and min(m, sigma), where the block then fits the grid"""
    return sorted({sd for sd in ((m + 1) // 2, 0, min(m, sigma)) if sd <= sigma and m - sd <= nu})


def block_values(m, kind, seed):
    n = 1 << m
    return [0] * n if kind == 0 else [R - 1] * n if kind == 1 else rand_ints(n, seed)


# ---------------------------------------------------------------------------------------------- 1. the claims of blocks against the definition
@pytest.mark.parametrize("grid_vars", [6, 9, 10])
def test_block_claims_against_the_definition(ctx, grid_vars):
    """m = 0, 1, 2, 5 and nu + sigma (a single entry; a block that fills the grid), every sigma_d of sigma_choices, entries 0, r - 1 and full width; 1, 8, 9 and 20
    tables in one call; the same call under launch caps of one and of three workgroups per table gives the same bytes"""
    sigma = (grid_vars + 1) // 2
    nu = grid_vars - sigma
    point = rand_ints(grid_vars, 8100 + grid_vars)
    shapes = [(m, sd) for m in (0, 1, 2, 5, grid_vars) for sd in sigma_choices(m, nu, sigma)]
    assert (grid_vars, sigma) in shapes and (0, 0) in shapes and len(shapes) >= 8
    shapes = (shapes * 3)[:20]
    values = [block_values(m, k % 3 if k < 18 else 2, 8200 + 32 * grid_vars + k) for k, (m, _) in enumerate(shapes)]
    want = [block_claim(t, sd, sigma, point) for t, (_, sd) in zip(values, shapes)]
    assert want[0] == 0 and any(want)
    tables = [ctx.upload(fr_ints(t)) for t in values]
    sigmas = [sd for _, sd in shapes]
    try:
        for count in (1, 8, 9, 20):
            got = ctx.dory_evaluate_blocks(tables[:count], sigmas[:count], fr_ints(point), sigma)
            assert got.shape == (count, 4) and np.array_equal(got, fr_ints(want[:count])), count
        # the fill-the-grid block alone is the table's multilinear evaluation: the oracle's
        k = shapes.index((grid_vars, sigma))
        assert np.array_equal(fr_int(want[k]), O.poly_evaluate(fr_ints(values[k]), fr_ints(point)))
        capped = []
        for cap in ("1", "3"):
            os.environ[CAP] = cap
            try:
                capped.append(ctx.dory_evaluate_blocks(tables, sigmas, fr_ints(point), sigma))
            finally:
                del os.environ[CAP]
        assert capped[0].tobytes() == capped[1].tobytes() == fr_ints(want).tobytes()
    finally:
        for t in tables:
            t.free()


def test_block_claim_with_waves_striding_and_several_workgroups(ctx):
    """one block of 2^14 entries (128 rows of 128 columns) in a 16-variable grid: 128 units, 32 workgroups of four waves by default (several partial sums); under a cap
    of two workgroups a wave strides over 16 units.  Beside it a single entry and a short block, so that workgroups without work write their zero."""
    nu = sigma = 8
    point = rand_ints(16, 8300)
    values = [rand_ints(1 << 14, 8301), [R - 1], rand_ints(1 << 5, 8302)]
    sigmas = [7, 0, 3]
    want = fr_ints([block_claim(t, sd, sigma, point) for t, sd in zip(values, sigmas)])
    tables = [ctx.upload(fr_ints(t)) for t in values]
    try:
        assert np.array_equal(ctx.dory_evaluate_blocks(tables, sigmas, fr_ints(point), sigma), want)
        os.environ[CAP] = "2"
        try:
            assert np.array_equal(ctx.dory_evaluate_blocks(tables, sigmas, fr_ints(point), sigma), want)
        finally:
            del os.environ[CAP]
    finally:
        for t in tables:
            t.free()


def test_block_claim_refusals(ctx):
    """every refusal is a returned status and the context stays usable"""
    sigma, nu = 3, 2
    t16, t12 = ctx.upload(fr_ints(rand_ints(16, 8400))), ctx.upload(fr_ints(rand_ints(12, 8401)))
    other = ffi.Context(0)
    foreign = other.upload(fr_ints(rand_ints(16, 8402)))
    point = fr_ints(rand_ints(nu + sigma, 8403))
    out = ffi.fr_array(300)

    def status(tables=(t16,), sigmas=(2,), pt=point, nu_=nu, sigma_=sigma, n=None, ctx_h=ctx.h):
        hs = (C.c_void_p * max(len(tables), 1))(*[t.h if t is not None else None for t in tables])
        sg = (C.c_uint32 * max(len(sigmas), 1))(*sigmas)
        return ffi.lib().jolt_dory_evaluate_blocks(ctx_h, hs, sg, len(tables) if n is None else n, ffi._p(pt), pt.shape[0], nu_, sigma_, ffi._p(out))

    assert status(n=0) == INVALID_ARG and status(tables=(None,)) == INVALID_ARG and status(ctx_h=None) == INVALID_ARG
    assert status(tables=(t16,) * 257, sigmas=(2,) * 257) == UNSUPPORTED
    assert status(tables=(t16,) * 256, sigmas=(2,) * 256) == 0
    assert status(tables=(foreign,)) == INVALID_ARG            # a table of another context
    assert status(tables=(t12,)) == INVALID_ARG                # not a power of two
    assert status(sigmas=(5,)) == INVALID_ARG                  # sigma_d above m_d
    assert status(sigmas=(3,), sigma_=2, nu_=3) == INVALID_ARG  # sigma_d above the grid's sigma
    assert status(sigmas=(1,)) == SIZE_MISMATCH                # 8 rows in a grid of 4
    assert status(pt=point[:-1]) == INVALID_ARG                # n_point != nu + sigma
    bad = point.copy()
    bad[1] = np.full(4, 2**64 - 1, dtype=np.uint64)
    assert status(pt=bad) == INVALID_ARG                       # a coordinate that is not canonical
    assert status() == 0
    foreign.free()
    other.close()
    t16.free()
    t12.free()


# ---------------------------------------------------------------------------------------------- 2. the fold past eight tables
@pytest.mark.parametrize("n_tables", [9, 20])
@pytest.mark.parametrize("with_base", [False, True])
def test_fold_of_more_than_eight_blocks(ctx, n_tables, with_base):
    """two and three launch sets (the last one short); blocks of one entry up to 256 rows (several slices) in a grid of 32 columns, against Python integers"""
    from test_gpu_dory_rows_fr import fold_definition
    sigma = 5
    shapes = [(0, 0), (1, 1), (4, 2), (5, 3), (10, 5), (8, 0), (3, 0), (5, 5), (13, 5), (2, 1)]  # (m, sigma_d); (13, 5): 256 rows
    shapes = (shapes * 2)[:n_tables]
    tables = [rand_ints(1 << m, 8500 + k) for k, (m, _) in enumerate(shapes)]
    sigmas = [sd for _, sd in shapes]
    scalars, left = rand_ints(n_tables, 8540), rand_ints(256, 8541)
    base = rand_ints(1 << sigma, 8542) if with_base else None
    dev = [ctx.upload(fr_ints(t)) for t in tables]
    lt = ctx.upload(fr_ints(left))
    bt = ctx.upload(fr_ints(base)) if with_base else None
    out = ctx.dory_fold_rows_blocks_many(dev, sigmas, fr_ints(scalars), sigma, lt, bt)
    try:
        assert np.array_equal(out.download(), fr_ints(fold_definition(tables, sigmas, scalars, sigma, left, base)))
        with pytest.raises(ffi.JoltError) as e:
            ctx.dory_fold_rows_blocks_many([dev[0]] * 257, [0] * 257, fr_ints([1] * 257), sigma, lt)
        assert e.value.status == UNSUPPORTED
    finally:
        for t in dev + [lt, out] + ([bt] if bt is not None else []):
            t.free()


# ---------------------------------------------------------------------------------------------- the step with blocks
BLOCKS = {4: [8, 4, 1], 6: [10, 5, 1]}  # log2 sizes: 2^nu rows (the block fills the grid); ragged (4 rows of 4 / 4 rows of 8 columns); a single row of two entries


def block_tables(w):
    """the blocks of a workload as Python integers, from what was uploaded"""
    return [[int(x) for x in O.from_mont(b.download())] for b in w.dory_blocks]


def trace_grids(w):
    """the trace's columns materialised in the workload's placement"""
    grids = workload_grids(w)  # cycle-major: index k * T + j
    if w.dory_order != "address_major":
        return grids
    T, K, log_block, log_stride = 1 << w.n_vars, 1 << w.log_k, w.log_k + w.dory_log_extra, w.dory_log_extra
    out = []
    for g in grids:
        am = [0] * (1 << w.grid_vars)
        for k in range(K):
            for j in range(T):
                am[(j << log_block) + (k << log_stride)] = g[k * T + j]
        out.append(am)
    return out


def all_grids(w):
    return trace_grids(w) + [embedded_grid(t, sd, w.dory_nu, w.dory_sigma) for t, sd in zip(block_tables(w), w.dory_block_sigmas)]


def check_step(w, bases, label, order=None, d_seed=8600):
    """the claims against the definitions; hints of the blocks from the definition; the opening against the model; the joint commitment from the model's own hint
    logs of the materialised embedded grids"""
    sigma, nu = w.dory_sigma, w.dory_nu
    n, rows = 1 << sigma, 1 << nu
    trace, tables = trace_grids(w), block_tables(w)
    point = [int(x) for x in O.from_mont(w.open_point)]
    n_trace = len(trace)
    assert np.array_equal(w.opening_claims[:n_trace], oracle_claims(trace, w.open_point))
    assert np.array_equal(w.opening_claims[n_trace:], fr_ints([block_claim(t, sd, sigma, point) for t, sd in zip(tables, w.dory_block_sigmas)]))
    if w.dory_commitment is None:
        w.dory_commit()
    hints = w.dory_commitment.hints
    assert [r for _, _, r in hints[n_trace:]] == [len(t) >> sd for t, sd in zip(tables, w.dory_block_sigmas)]
    grids = all_grids(w)
    out = w.dory_open(label, column_of_claim=order)
    evaluations = w.opening_claims if order is None else w.opening_claims[list(order)]
    model = check_opening(w, bases, grids, out, label, evaluations, order=order, d_seed=d_seed)
    kg1, kg2 = bases["kg1"][:n], bases["kg2"][:n]
    logs = [hint_logs(g, n, kg1, rows) for g in grids]
    for (vec, first, count), lg in zip(hints[n_trace:], logs[n_trace:]):  # a ragged hint is the leading rows; the rows past it are zero in the embedded grid
        got = vec.download(first, count)
        assert not any(lg[count:])
        from dory_groups import G1
        assert all(G1.same(got[i], lg[i]) for i in sorted({0, count - 1}))
    position = list(range(len(grids))) if order is None else [list(order).index(c) for c in range(len(grids))]
    assert model.commitment == sum(model.powers[position[c]] * sum(k * kg2[i] for i, k in enumerate(lg)) for c, lg in enumerate(logs)) % R
    return out


STEP_LABEL = {4: ffi.TRANSCRIPT_BLAKE2B | 8704, 6: ffi.TRANSCRIPT_KECCAK | 8706}


@pytest.mark.parametrize("n_vars", [4, 6])
def test_step_with_blocks(ctx, bases, n_vars):
    """n_vars = 4: grid 2^8, sigma = nu = 4; 6: grid 2^10, sigma = nu = 5.  Three blocks behind the 38 columns: 41 claims."""
    w = DeviceWorkload(ctx, n_vars, seed=8700 + n_vars, pcs="dory", dory_bases=planted(bases), dory_blocks=BLOCKS[n_vars])
    try:
        assert (w.grid_vars, w.dory_order, len(w.dory_blocks)) == (LOG_K + n_vars, "cycle_major", 3)
        nu = w.dory_nu
        assert [len(b) >> sd for b, sd in zip(w.dory_blocks, w.dory_block_sigmas)] == [1 << nu, 4, 1]
        assert all(sd < w.dory_sigma for sd in w.dory_block_sigmas[1:])
        out = check_step(w, bases, STEP_LABEL[n_vars])
        again = w.dory_open(STEP_LABEL[n_vars])
        for key in ("gts", "g1s", "g2s", "challenges", "scalars", "joint_eval"):
            assert np.array_equal(again[key], out[key]), key
    finally:
        w.close()


@pytest.fixture(scope="module")
def step6(ctx, bases):
    w = DeviceWorkload(ctx, 6, seed=8806, pcs="dory", dory_bases=planted(bases), dory_blocks=BLOCKS[6])
    w.dory_commit()
    yield w
    w.close()


def test_a_batch_order_that_interleaves_blocks_with_columns(bases, step6):
    w = step6
    n_cols = len(w.dory_commitment.hints)
    n_trace = n_cols - 3
    order = list(np.random.default_rng(8900).permutation(n_cols))
    where = [order.index(c) for c in range(n_trace, n_cols)]
    assert min(where) < n_trace and sorted(where) != list(range(min(where), min(where) + 3))  # blocks among the columns, not as one run
    check_step(w, bases, ffi.TRANSCRIPT_BLAKE2B | 8906, order=order)


# ---------------------------------------------------------------------------------------------- 5. the address-major placement
@pytest.mark.parametrize("log_extra", [0, 1])
def test_step_with_blocks_address_major(ctx, bases, log_extra):
    """n_vars = 6: grid 2^10 (sigma = nu = 5: a matrix row is two cycles) and, widened, 2^11 (sigma = 6, nu = 5: a row is two cycles of 32 columns each)"""
    w = DeviceWorkload(ctx, 6, seed=9000 + log_extra, pcs="dory", dory_bases=planted(bases), dory_blocks=BLOCKS[6], dory_order="address_major", dory_log_extra=log_extra)
    try:
        assert (w.grid_vars, w.dory_sigma, w.dory_nu) == (10 + log_extra, 5 + log_extra, 5)
        check_step(w, bases, ffi.TRANSCRIPT_BLAKE2B | (9006 + log_extra))
        assert all(r == 1 << w.dory_nu for _, _, r in w.dory_commitment.hints[:-3])  # every trace column, one-hot or dense, has 2^nu rows in this placement
    finally:
        w.close()


# ---------------------------------------------------------------------------------------------- 3. n_blocks = 0, cycle-major: the guard that nothing existing moved
def prove_batch_blocks_raw(ctx, w, label, blocks=(), sigmas=(), order=0, log_extra=0):
    """jolt_host_dory_prove_batch_blocks called directly (Context.dory_prove_batch routes a call without blocks to the old entry)"""
    views = [ffi._dory_view(h) for h in w.dory_commitment.hints]
    hs, firsts, rows = ffi._dory_view_arrays(views)
    ev, pt = ffi.fr(w.opening_claims), ffi.fr(w.open_point)
    sigma = (pt.shape[0] + 1) // 2
    n_gt, n_g1, n_g2, n_ch = ffi.host_dory_proof_counts(sigma)
    gts, g1s, g2s, ch = np.zeros((n_gt, 48), dtype=np.uint64), np.zeros((n_g1, 12), dtype=np.uint64), np.zeros((n_g2, 24), dtype=np.uint64), ffi.fr_array(n_ch)
    scalars, joint = ffi.fr_array(len(views)), ffi.fr_array(1)
    sources, dense = w._dory_columns()
    ss = (C.c_void_p * len(sources))(*[s.h for s in sources])
    ds = (C.c_void_p * len(dense))(*[t.h for t in dense])
    bs = (C.c_void_p * max(len(blocks), 1))(*[b.h for b in blocks])
    sg = (C.c_uint32 * max(len(blocks), 1))(*sigmas)
    t = ffi.HostTranscript(label)
    try:
        ffi._call("jolt_host_dory_prove_batch_blocks", ctx, ctx.h, w.dory_setup.h, hs, firsts, rows, len(views), ffi._p(ev), ss, len(sources), ds, len(dense),
                  bs if blocks else None, sg if blocks else None, len(blocks), w.log_k, order, log_extra, None, ffi._p(pt), pt.shape[0], t.h, ffi._p(gts), ffi._p(g1s),
                  ffi._p(g2s), ffi._p(ch), ffi._p(scalars), ffi._p(joint))
        return dict(gts=gts, g1s=g1s, g2s=g2s, challenges=ch, scalars=scalars, joint_eval=joint[0], transcript_state=t.state())
    finally:
        t.close()


def test_without_blocks_the_new_entry_is_the_old_one_byte_for_byte(ctx, bases):
    w = DeviceWorkload(ctx, 4, seed=9104, pcs="dory", dory_bases=planted(bases))
    try:
        label = ffi.TRANSCRIPT_BLAKE2B | 9104
        old = w.dory_open(label)
        new = prove_batch_blocks_raw(ctx, w, label)
        for key in ("gts", "g1s", "g2s", "challenges", "scalars", "joint_eval"):
            assert old[key].tobytes() == new[key].tobytes(), key
        assert old["transcript_state"] == new["transcript_state"]
    finally:
        w.close()


# ---------------------------------------------------------------------------------------------- 6. a wrong block claim
def test_a_wrong_block_claim_is_refused_and_leaves_nothing_behind(ctx, bases, step6):
    w = step6
    label = ffi.TRANSCRIPT_BLAKE2B | 9206
    good = w.dory_open(label)
    before = ctx.memory_stats()["live_bytes"]
    wrong = w.opening_claims.copy()
    wrong[-2] = O.fr_add(wrong[-2:-1], fr_int(1).reshape(1, 4))[0]  # the ragged block's claim
    with pytest.raises(ffi.JoltError) as e:
        w.dory_open(label, evaluations=wrong)
    assert e.value.status == ROUND_CHECK
    assert ctx.memory_stats()["live_bytes"] == before
    after = w.dory_open(label)  # a correct proof follows on the same context
    for key in ("gts", "g1s", "g2s", "challenges", "scalars", "joint_eval"):
        assert np.array_equal(after[key], good[key]), key
    assert ctx.memory_stats()["live_bytes"] == before
    check_opening(w, bases, all_grids(w), after, label, w.opening_claims)


# ---------------------------------------------------------------------------------------------- 7. refusals before the transcript moves
def test_refusals_before_the_transcript_moves(ctx, step6):
    w = step6
    sources, dense = w._dory_columns()
    hints, claims = list(w.dory_commitment.hints), w.opening_claims
    blocks, sigmas = list(w.dory_blocks), list(w.dory_block_sigmas)
    sigma, nu = w.dory_sigma, w.dory_nu
    assert (len(blocks[0]), sigmas[0]) == (1 << (nu + sigma), sigma) and hints[-3][2] != hints[-2][2]
    t12 = ctx.upload(fr_ints(rand_ints(12, 9300)))
    other = ffi.Context(0)
    foreign = other.upload(blocks[1].download())
    n_trace = len(hints) - 3

    def status(hints=hints, claims=claims, blocks=blocks, sigmas=sigmas, **kw):
        t = ffi.HostTranscript(ffi.TRANSCRIPT_BLAKE2B | 9306)
        start, before = t.state(), ctx.memory_stats()["live_bytes"]
        try:
            with pytest.raises(ffi.JoltError) as e:
                ctx.dory_prove_batch(w.dory_setup, hints, claims, sources, dense, w.log_k, w.open_point, t, blocks=blocks, block_sigmas=sigmas, **kw)
            assert t.state() == start and ctx.memory_stats()["live_bytes"] == before  # nothing absorbed, nothing allocated
            return e.value.status
        finally:
            t.close()

    assert status(sigmas=[sigma + 1] + sigmas[1:]) == INVALID_ARG                      # sigma_d > sigma
    assert status(sigmas=[sigma - 1] + sigmas[1:]) == SIZE_MISMATCH                    # 2^(nu + 1) rows
    assert status(hints=hints[:-3] + [hints[-2], hints[-3], hints[-1]]) == INVALID_ARG  # hints whose rows differ from their blocks'
    assert status(blocks=[blocks[0], t12, blocks[2]]) == INVALID_ARG                   # a length that is not a power of two
    assert status(blocks=[blocks[0], foreign, blocks[2]]) == INVALID_ARG               # a table of another context
    assert status(log_extra=1) == INVALID_ARG                                          # log_extra in the cycle-major placement
    many = 257
    assert status(hints=hints[:n_trace] + [hints[-1]] * many, claims=np.concatenate([claims[:n_trace]] + [claims[-1:]] * many), blocks=[blocks[2]] * many,
                  sigmas=[sigmas[2]] * many) == UNSUPPORTED
    foreign.free()
    other.close()
    t12.free()
    out = w.dory_open(ffi.TRANSCRIPT_BLAKE2B | 9306)  # the context opens afterwards
    assert out["sigma"] == sigma


def test_shapes_are_refused_at_construction(ctx):
    """before anything is uploaded: the live bytes of the context do not move"""
    before = ctx.memory_stats()["live_bytes"]
    for kw in (dict(dory_blocks=[11]),                                   # more entries than the 2^10 grid
               dict(dory_blocks=[np.zeros((12, 4), dtype=np.uint64)]),   # not a power of two
               dict(dory_order="row_major"),
               dict(dory_log_extra=1)):                                  # cycle-major has no extra
        with pytest.raises(ValueError):
            DeviceWorkload(ctx, 6, pcs="dory", **kw)
    with pytest.raises(ValueError):
        DeviceWorkload(ctx, 4, pcs="dory", dory_order="address_major", dory_log_extra=2)  # grid 2^10: sigma = 5 < log_k + log_extra = 6
    with pytest.raises(ValueError):
        DeviceWorkload(ctx, 6, pcs="grid", dory_blocks=[4])
    assert ctx.memory_stats()["live_bytes"] == before
