"""GPU parity: stage 8 under Dory -- jolt_grid_evaluate_columns (the statement's claims from one pass over the witness), jolt_host_dory_prove_batch
(HomomorphicBatch::prove_batch as one library call) and DeviceWorkload(pcs="dory") over them.

Expected values come from definitions: a column's claim is the oracle's multilinear evaluation of the materialised column; Gamma1 / Gamma2 / H1 / H2 are planted
progressions, so every hint element, tier-2 commitment and proof element has a known discrete logarithm and is held against the log-space model
(tests/dory_open_model.py, tests/pairing_model.py); the transcript is replayed through the entry points of the framing and of the group elements.  GT elements
and field elements bit for bit, points as group elements; no tolerance anywhere.  One test is a cross-check of two device routes and says so in its name."""
import numpy as np
import pytest

import dory_open_model as OM
import oracle_lib as O
import pairing_model as PM
from dory_groups import G1, G2, R, fr_int, fr_ints, progression, rand_ints
from jolt_amd import dory_proof, ffi
from jolt_amd.workload import DeviceWorkload
from test_gpu_dory_proof import check_against_the_model, mont_int
from util import rand_fr

pytestmark = pytest.mark.gpu
N_SETUP = 64  # 2^sigma of the largest step below (n_vars = 7: sigma = 6)
LOG_K = 4
IDENT = O.g1_identity()
ONE = IDENT[0:4]  # the Montgomery one of Fq
ROUND_CHECK, INVALID_ARG = 8, 1


@pytest.fixture(scope="module")
def ctx():
    c = ffi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def bases():
    a0, ad, b0, bd, kh1, kh2 = rand_ints(6, 4100)
    kg1, gamma1 = progression(G1, a0, ad, N_SETUP)
    kg2, gamma2 = progression(G2, b0, bd, N_SETUP)
    return dict(kg1=kg1, gamma1=gamma1, kg2=kg2, gamma2=gamma2, kh1=kh1, h1=G1.point(kh1), kh2=kh2, h2=G2.point(kh2, rep=3))


def planted(bases):
    return {k: bases[k] for k in ("gamma1", "gamma2", "h1", "h2")}


# ---------------------------------------------------------------------------------------------- the claims: one pass over the witness against the oracle
def grid_of_onehot(column, K, cold):
    """the materialised column on the cycle-major grid, index k * T + j, as canonical integers"""
    T = len(column)
    grid = [0] * (K * T)
    for j, h in enumerate(column):
        if h != cold:
            grid[int(h) * T + j] = 1
    return grid


def grid_of_dense(values, K):
    return [int(v) % R for v in values] + [0] * ((K - 1) * len(values))


def oracle_claims(grids, point):
    return np.stack([O.poly_evaluate(O.to_mont(g), point) for g in grids])


def make_columns(rng, log_t, shapes, n_dense):
    """shapes: (columns, dtype) per source; column 1 of the first source is cold throughout, the others are cold on a quarter of the cycles"""
    T, K = 1 << log_t, 1 << LOG_K
    idx = []
    for s, (cols, dtype) in enumerate(shapes):
        cold = 0xFFFF if dtype == np.uint16 else 0xFF
        a = rng.integers(0, K, size=(cols, T)).astype(dtype)
        a[rng.random((cols, T)) < 0.25] = cold
        if s == 0 and cols > 1:
            a[1, :] = cold
        idx.append(a)
    dense = [rng.integers(-2**40, 2**40, size=T, dtype=np.int64) for _ in range(n_dense)]
    return idx, dense


CLAIM_CASES = [(4, [(5, np.uint8), (2, np.uint16)], 3), (6, [(5, np.uint16), (3, np.uint8)], 1), (7, [(4, np.uint8), (1, np.uint16)], 5), (12, [(5, np.uint8), (2, np.uint16)], 2),
               (6, [], 2), (6, [(3, np.uint8)], 0)]


@pytest.mark.parametrize("log_t,shapes,n_dense", CLAIM_CASES, ids=["t4", "t6", "t7", "t12", "dense-only", "onehot-only"])
def test_claims_from_one_pass_are_the_oracles_evaluations(ctx, log_t, shapes, n_dense):
    """T = 2^4, 2^6, 2^7 (one workgroup, partly filled) and 2^12 (sixteen), log_k = 4, both index widths in either source position, groups of 4, 1, 2, 3 and 5 columns
    (a full pass, a short one, two passes), a column that is cold throughout, dense columns of negative integers.  Bit for bit."""
    rng = np.random.default_rng(4200 + log_t)
    K = 1 << LOG_K
    idx, dense = make_columns(rng, log_t, shapes, n_dense)
    point = rand_fr(LOG_K + log_t, 4300 + log_t)
    sources = [ctx.onehot(a, K) for a in idx]
    tables = [ctx.upload(O.fr_from_i64(d)) for d in dense]
    got = ctx.grid_evaluate_columns(sources, tables, LOG_K, point)
    grids = [grid_of_onehot(col, K, 0xFFFF if a.dtype == np.uint16 else 0xFF) for a in idx for col in a] + [grid_of_dense(d, K) for d in dense]
    want = oracle_claims(grids, point)
    assert got.shape == want.shape and np.array_equal(got, want)
    if shapes and shapes[0][0] > 1:
        assert not got[1].any()  # the cold column evaluates to zero
    assert np.array_equal(ctx.grid_evaluate_columns(sources, tables, LOG_K, point), got)
    for t in sources + tables:
        t.free()


def test_claims_with_lanes_striding_over_several_cycles(ctx):
    """33 groups (four sources of 32 columns and a dense column) cap the launch at 62 workgroups per group; at T = 2^14 = 64 x 256 a lane then serves more than one
    cycle and the last stride is partly idle.  A sample of columns against the oracle, every source and both ends of a source among them."""
    log_t, K = 14, 1 << LOG_K
    rng = np.random.default_rng(4400)
    idx, dense = make_columns(rng, log_t, [(32, np.uint8)] * 4, 1)
    point = rand_fr(LOG_K + log_t, 4401)
    sources = [ctx.onehot(a, K) for a in idx]
    tables = [ctx.upload(O.fr_from_i64(d)) for d in dense]
    got = ctx.grid_evaluate_columns(sources, tables, LOG_K, point)
    assert got.shape == (129, 4)
    for s, p in [(0, 0), (0, 1), (0, 31), (1, 17), (2, 4), (3, 0), (3, 31)]:
        want = O.poly_evaluate(O.to_mont(grid_of_onehot(idx[s][p], K, 0xFF)), point)
        assert np.array_equal(got[32 * s + p], want), (s, p)
    assert np.array_equal(got[128], O.poly_evaluate(O.to_mont(grid_of_dense(dense[0], K)), point))
    for t in sources + tables:
        t.free()


def test_claims_refusals(ctx):
    K = 1 << LOG_K
    rng = np.random.default_rng(4500)
    idx, dense = make_columns(rng, 6, [(3, np.uint8)], 1)
    source, table = ctx.onehot(idx[0], K), ctx.upload(O.fr_from_i64(dense[0]))
    short = ctx.upload(O.fr_from_i64(dense[0][:32]))
    point = rand_fr(LOG_K + 6, 4501)

    def status(*args):
        with pytest.raises(ffi.JoltError) as e:
            ctx.grid_evaluate_columns(*args)
        return e.value.status

    assert status([source], [table], LOG_K, point[:-1]) == INVALID_ARG       # a point of another length
    bad = point.copy()
    bad[3] = np.full(4, 2**64 - 1, dtype=np.uint64)
    assert status([source], [table], LOG_K, bad) == INVALID_ARG              # a coordinate that is not canonical
    assert status([source], [short], LOG_K, point) == 5                      # JOLT_ERR_SIZE_MISMATCH
    assert status([source], [table], 3, point[1:]) == INVALID_ARG            # a hot address outside the grid
    assert status([], [], LOG_K, point) == 6                                 # JOLT_ERR_UNSUPPORTED: no column at all
    assert status([source] * 5, [], LOG_K, point) == 6
    assert ctx.grid_evaluate_columns([source], [table], LOG_K, point).shape == (4, 4)  # the context stays usable
    for t in (source, table, short):
        t.free()


# ---------------------------------------------------------------------------------------------- the step
def workload_grids(w):
    """the committed columns of a workload, materialised from the hot indices its sources hold (what was uploaded, byte for byte) and its specification's integer
    columns, in the column order of the opening"""
    K = 1 << w.log_k
    grids = []
    for i in sorted(w.sources):
        grids += [grid_of_onehot(col, K, 0xFF) for col in w.sources[i].download()]
    for name in w.committed_dense:
        grids.append(grid_of_dense(w.tables_spec[name].data, K))
    return grids


def hint_logs(grid, n, kg1, rows):
    """the discrete logarithms of a column's row commitments: row r of the matrix against Gamma1[:n]"""
    return [sum(grid[r * n + j] * kg1[j] for j in range(n)) % R for r in range(rows)]


class StepModel:
    """everything the log-space model says about one batch opening: grids (column order), the claims' order, the scalars gamma^i"""

    def __init__(self, w, bases, grids, order, gamma):
        self.sigma, self.nu = w.dory_sigma, w.dory_nu
        n, rows = 1 << self.sigma, 1 << self.nu
        self.n, self.rows = n, rows
        self.kg1, self.kg2, self.kh1, self.kh2 = bases["kg1"][:n], bases["kg2"][:n], bases["kh1"], bases["kh2"]
        order = list(range(len(grids))) if order is None else list(order)
        self.powers = [pow(gamma, i, R) for i in range(len(grids))]
        weight = [0] * len(grids)
        for i, c in enumerate(order):
            weight[c] = self.powers[i]
        joint = [sum(wt * g[x] for wt, g in zip(weight, grids)) % R for x in range(n * rows)]
        self.matrix = [joint[r * n:(r + 1) * n] for r in range(rows)]
        point = O.from_mont(w.open_point)
        self.L = [int(x) for x in O.from_mont(O.eq_evals(w.open_point[:self.nu]))]
        self.Rr = [int(x) for x in O.from_mont(O.eq_evals(w.open_point[self.nu:]))]
        assert len(point) == self.sigma + self.nu
        self.t_rows, self.commitment, self.v, self.y = OM.statement(self.kg1, self.kg2, self.matrix, self.L, self.Rr)

    def prove(self, challenges, gamma):
        return OM.prove(self.kg1, self.kg2, self.kh1, self.kh2, self.t_rows, self.v, self.L, self.Rr, challenges, gamma)

    def verify(self, proof, challenges, gamma, d, y=None):
        return OM.verify(self.kg1, self.kg2, self.kh1, self.kh2, self.commitment, self.y if y is None else y, self.L, self.Rr, proof, challenges, gamma, d)


def replay(label, evaluations, out, point):
    """a second transcript: the statement, the proof's elements through jolt_host_dory_transcript_append_* in the header's phase order, the closing claim
    -> (scalars, challenges drawn, final state)"""
    t = ffi.HostTranscript(label)
    scalars = ffi.host_opening_statement_absorb(t, evaluations)
    proof = dory_proof.DoryProof(out["sigma"], out["gts"], out["g1s"], out["g2s"], out["challenges"])
    drawn = []
    dory_proof.absorb(t, proof.vmv)
    for first, second in proof.rounds:
        dory_proof.absorb(t, first)  # gts, then g1s, then g2s
        drawn.append(t.challenge(full_width=True))
        dory_proof.absorb(t, second)
        drawn.append(t.challenge(full_width=True))
    drawn.append(t.challenge(full_width=True))
    dory_proof.absorb(t, proof.final)
    ffi.host_opening_claim_absorb(t, point, out["joint_eval"])
    state = t.state()
    t.close()
    return scalars, drawn, state


def check_opening(w, bases, grids, out, label, evaluations, order=None, d_seed=4600):
    """scalars, joint evaluation, every proof element against the model under the reported challenges, the log-space verifier, the transcript replay"""
    scalars, drawn, state = replay(label, evaluations, out, w.open_point)
    assert np.array_equal(out["scalars"], scalars)
    gamma_rlc = mont_int(scalars[1]) if len(scalars) > 1 else 1
    model = StepModel(w, bases, grids, order, gamma_rlc)
    assert [mont_int(s) for s in out["scalars"]] == model.powers
    assert np.array_equal(out["joint_eval"], fr_int(model.y))
    assert (out["nu"], out["sigma"]) == (model.nu, model.sigma)
    flat = list(out["challenges"])
    assert len(drawn) == len(flat) == 2 * model.sigma + 1 and all(np.array_equal(a, b) for a, b in zip(drawn, flat))
    assert state == out["transcript_state"]
    proof = dory_proof.DoryProof(model.sigma, out["gts"], out["g1s"], out["g2s"], out["challenges"])
    challenges = [(mont_int(b), mont_int(a)) for b, a in proof.challenges]
    gamma = mont_int(proof.gamma)
    assert all(b and a for b, a in challenges) and gamma
    want = model.prove(challenges, gamma)
    check_against_the_model(proof, want)
    d = rand_ints(1, d_seed)[0]
    assert model.verify(want, challenges, gamma, d)
    assert not model.verify(want, challenges, gamma, d, y=model.y + 1)
    return model


STEP_LABEL = {4: ffi.TRANSCRIPT_BLAKE2B | 7104, 6: ffi.TRANSCRIPT_KECCAK | 7106, 7: ffi.TRANSCRIPT_BLAKE2B | 7107}


@pytest.mark.parametrize("n_vars", [4, 6, 7])
def test_step_under_dory(ctx, bases, n_vars):
    """n_vars = 4: grid 2^8, sigma = nu = 4, a dense hint of ONE row; 6: grid 2^10, sigma = nu = 5, dense hints of 2 rows among hints of 32; 7: grid 2^11, sigma = 6,
    nu = 5 < sigma, so the state is padded with identities and zeros"""
    w = DeviceWorkload(ctx, n_vars, seed=4700 + n_vars, pcs="dory", dory_bases=planted(bases))
    try:
        sigma, nu = (LOG_K + n_vars + 1) // 2, (LOG_K + n_vars) // 2
        assert (w.grid_vars, w.dory_sigma, w.dory_nu) == (LOG_K + n_vars, sigma, nu)
        n, rows, T = 1 << sigma, 1 << nu, 1 << n_vars
        grids = workload_grids(w)
        n_cols = len(grids)
        assert n_cols == sum(w.sources[i].n_polys for i in w.sources) + 2
        # ---- the statement's claims: the oracle's evaluation of every materialised column; the pushforward route gives the same field elements
        want_claims = oracle_claims(grids, w.open_point)
        assert np.array_equal(w.opening_claims, want_claims)
        assert np.array_equal(w.evaluate_columns_pushforward(), want_claims)
        label = STEP_LABEL[n_vars]
        out = w.step(label)
        assert set(out) == {"commit", "stages", "open"}
        # ---- tier 1 and tier 2 from the definition
        hints = w.dory_commitment.hints
        assert [r for _, _, r in hints] == [rows] * (n_cols - 2) + [T >> sigma] * 2
        kg1, kg2 = bases["kg1"][:n], bases["kg2"][:n]
        logs = [hint_logs(g, n, kg1, r) for g, (_, _, r) in zip(grids, hints)]
        for (vec, first, count), lg in zip(hints, logs):
            got = vec.download(first, count)
            assert all(np.array_equal(e, IDENT) if k == 0 else np.array_equal(e[8:12], ONE) for e, k in zip(got, lg))
            for i in sorted({0, count // 2, count - 1}):
                assert G1.same(got[i], lg[i])
        tier2 = out["commit"]["tier2"]
        assert tier2.shape == (n_cols, 48)
        for got, lg in zip(tier2, logs):
            assert np.array_equal(got, PM.gt_to_abi(PM.expected([sum(k * kg2[i] for i, k in enumerate(lg)) % R], [1])))
        # ---- the opening
        model = check_opening(w, bases, grids, out["open"], label, w.opening_claims)
        assert model.commitment == sum(p * sum(k * kg2[i] for i, k in enumerate(lg)) for p, lg in zip(model.powers, logs)) % R  # the combined commitment is the RLC of the 38
        # ---- a second step is the same bytes
        again = w.step(label)
        for key in ("gts", "g1s", "g2s", "challenges", "scalars", "joint_eval"):
            assert np.array_equal(again["open"][key], out["open"][key]), key
        assert again["open"]["transcript_state"] == out["open"]["transcript_state"]
        assert np.array_equal(again["commit"]["tier2"], tier2)
    finally:
        w.close()


@pytest.fixture(scope="module")
def step6(ctx, bases):
    w = DeviceWorkload(ctx, 6, seed=4706, pcs="dory", dory_bases=planted(bases))
    w.dory_commit()
    yield w, workload_grids(w)
    w.close()


def test_a_non_identity_batch_order_proves_the_permuted_batch(bases, step6):
    w, grids = step6
    n_cols = len(grids)
    order = list(np.random.default_rng(4800).permutation(n_cols))
    assert order != sorted(order)
    label = ffi.TRANSCRIPT_BLAKE2B | 7206
    out = w.dory_open(label, column_of_claim=order)
    check_opening(w, bases, grids, out, label, w.opening_claims[order], order=order)
    plain = w.dory_open(label)
    assert not np.array_equal(plain["joint_eval"], out["joint_eval"])


def test_one_wrong_evaluation_is_refused_and_leaves_nothing_behind(ctx, bases, step6):
    w, grids = step6
    label = ffi.TRANSCRIPT_BLAKE2B | 7306
    good = w.dory_open(label)
    before = ctx.memory_stats()["live_bytes"]
    wrong = w.opening_claims.copy()
    wrong[7] = O.fr_add(wrong[7:8], fr_int(1).reshape(1, 4))[0]
    with pytest.raises(ffi.JoltError) as e:
        w.dory_open(label, evaluations=wrong)
    assert e.value.status == ROUND_CHECK
    assert ctx.memory_stats()["live_bytes"] == before
    after = w.dory_open(label)  # a correct proof follows on the same context
    for key in ("gts", "g1s", "g2s", "challenges", "scalars", "joint_eval"):
        assert np.array_equal(after[key], good[key]), key
    assert ctx.memory_stats()["live_bytes"] == before
    check_opening(w, bases, grids, after, label, w.opening_claims)


def test_a_batch_order_that_is_no_permutation_is_refused_before_the_transcript_moves(ctx, step6):
    w, grids = step6
    n_cols = len(grids)
    sources, dense = w._dory_columns()
    for order in ([0] + list(range(n_cols - 1)), list(range(1, n_cols + 1))):  # a repeat; an index past the columns
        t = ffi.HostTranscript(ffi.TRANSCRIPT_BLAKE2B | 7406)
        start, before = t.state(), ctx.memory_stats()["live_bytes"]
        with pytest.raises(ffi.JoltError) as e:
            ctx.dory_prove_batch(w.dory_setup, [w.dory_commitment.hints[c % n_cols] for c in order], w.opening_claims, sources, dense, w.log_k, w.open_point, t, column_of_claim=order)
        assert e.value.status == INVALID_ARG
        assert t.state() == start and ctx.memory_stats()["live_bytes"] == before  # nothing absorbed, nothing allocated
        t.close()
    t = ffi.HostTranscript(ffi.TRANSCRIPT_BLAKE2B | 7406)
    start = t.state()
    with pytest.raises(ffi.JoltError) as e:  # one claim short of the columns
        ctx.dory_prove_batch(w.dory_setup, w.dory_commitment.hints[:-1], w.opening_claims[:-1], sources, dense, w.log_k, w.open_point, t)
    assert e.value.status == INVALID_ARG and t.state() == start
    t.close()


def test_cross_check_device_against_device_the_opening_through_dory_proof_prove(ctx, step6):
    """NOT parity: two routes through the same device code.  The batch call against dory_proof.prove with the scalars handed in, over tables built by the separate
    entries, on a transcript that was given the same prefix."""
    w, _ = step6
    label = ffi.TRANSCRIPT_BLAKE2B | 7506
    out = w.dory_open(label)
    sources, dense = w._dory_columns()
    n_onehot = sum(s.n_polys for s in sources)
    t = ffi.HostTranscript(label)
    scalars = ffi.host_opening_statement_absorb(t, w.opening_claims)
    left, right = ctx.eq_evals(w.open_point[:w.dory_nu]), ctx.eq_evals(w.open_point[w.dory_nu:])
    v = ctx.dory_fold_rows_grid(sources, scalars[:n_onehot], dense, scalars[n_onehot:], w.log_k, w.dory_sigma, left)
    assert np.array_equal(ctx.table_dot(v, right), out["joint_eval"])
    proof = dory_proof.prove(w.dory_setup, w.dory_commitment.hints, list(scalars), v, left, right, w.dory_nu, w.dory_sigma, transcript=t)
    ffi.host_opening_claim_absorb(t, w.open_point, out["joint_eval"])
    assert np.array_equal(proof.gts, out["gts"]) and np.array_equal(proof.g1s, out["g1s"]) and np.array_equal(proof.g2s, out["g2s"])
    assert t.state() == out["transcript_state"]
    t.close()
    for x in (left, right, v):
        x.free()


def test_a_column_that_is_cold_throughout(ctx, bases):
    """its hint is neutral elements, its commitment one, its claim zero; the opening verifies"""
    w = DeviceWorkload(ctx, 6, seed=4906, pcs="dory", dory_bases=planted(bases))
    try:
        i = sorted(w.sources)[-1]
        idx = w.sources[i].download()
        idx[1, :] = 0xFF
        k = w.sources[i].k
        w.sources[i].free()
        w.sources[i] = ctx.onehot(idx, k)
        w.opening_claims = w.evaluate_columns()
        grids = workload_grids(w)
        cold = sum(w.sources[j].n_polys for j in sorted(w.sources)[:-1]) + 1
        assert not any(grids[cold]) and not w.opening_claims[cold].any()
        tier2 = w.dory_commit()["tier2"]
        vec, first, count = w.dory_commitment.hints[cold]
        assert all(np.array_equal(e, IDENT) for e in vec.download(first, count))
        assert np.array_equal(tier2[cold], PM.gt_to_abi(PM.expected([0], [1])))  # the empty product: one
        label = ffi.TRANSCRIPT_BLAKE2B | 7606
        check_opening(w, bases, grids, w.dory_open(label), label, w.opening_claims)
    finally:
        w.close()


def test_step_over_a_generated_setup_verifies_in_the_groups(ctx):
    """Without dory_bases= the setup comes from jolt_amd/dory_setup.py: bases on their curves, the same for the same seed.  Their logarithms are unknown, so the
    log-space model does not apply; the step's proof is held to the verifier's equation IN THE GROUPS instead (library host code and the oracle on the checking
    side, tests/test_gpu_dory_open.py), against the RLC of the step's own 38 commitments, and the equation fails for another evaluation."""
    import g2_model as M
    from jolt_amd import dory_setup
    from test_gpu_dory_open import gt_mul, gt_pow, verify_in_the_groups
    n_vars = 4
    w = DeviceWorkload(ctx, n_vars, seed=5004, pcs="dory")
    try:
        bases, n = w.dory_bases, 1 << w.dory_sigma
        assert bases["gamma1"].shape == (n, 12) and bases["gamma2"].shape == (n, 24)
        assert all(O.g1_on_curve(p) and not O.g1_is_identity(p) for p in list(bases["gamma1"]) + [bases["h1"]])
        g2s = [M.from_abi(p) for p in list(bases["gamma2"]) + [bases["h2"]]]
        assert all(p is not None and M.on_curve(p) for p in g2s) and len(set(g2s)) == n + 1
        assert M.mul(g2s[0], M.R) is None and M.mul(g2s[-1], M.R) is None  # multiples of the order-r generator
        again = dory_setup.generate(ctx, n, 5004 + 2)
        assert all(np.array_equal(again[k], bases[k]) for k in ("gamma1", "gamma2", "h1", "h2"))
        assert not np.array_equal(dory_setup.generate(ctx, n, 5004 + 3)["gamma1"], bases["gamma1"])
        label = ffi.TRANSCRIPT_BLAKE2B | 7704
        step = w.step(label)
        out, tier2 = step["open"], step["commit"]["tier2"]
        grids = workload_grids(w)
        assert np.array_equal(w.opening_claims, oracle_claims(grids, w.open_point))
        scalars, drawn, state = replay(label, w.opening_claims, out, w.open_point)
        assert np.array_equal(out["scalars"], scalars) and state == out["transcript_state"]
        assert all(np.array_equal(a, b) for a, b in zip(drawn, out["challenges"]))
        powers = [mont_int(s) for s in scalars]
        y = sum(p * int(c) for p, c in zip(powers, O.from_mont(w.opening_claims))) % R
        assert np.array_equal(out["joint_eval"], fr_int(y))
        commitment = gt_mul(*[gt_pow(t, p) for t, p in zip(tier2, powers)])  # the statement's commitment: the RLC of the 38, in GT
        proof = dory_proof.DoryProof(w.dory_sigma, out["gts"], out["g1s"], out["g2s"], out["challenges"])
        challenges, gamma, d = [(mont_int(b), mont_int(a)) for b, a in proof.challenges], mont_int(proof.gamma), rand_ints(1, 5005)[0]
        L = [int(x) for x in O.from_mont(O.eq_evals(w.open_point[:w.dory_nu]))]
        Rr = [int(x) for x in O.from_mont(O.eq_evals(w.open_point[w.dory_nu:]))]
        assert verify_in_the_groups(bases, commitment, y, L, Rr, proof.vmv, proof.rounds, proof.final, challenges, gamma, d)
        assert not verify_in_the_groups(bases, commitment, y + 1, L, Rr, proof.vmv, proof.rounds, proof.final, challenges, gamma, d)
    finally:
        w.close()


def test_other_schemes_are_still_refused(ctx):
    with pytest.raises(ValueError):
        DeviceWorkload(ctx, 4, pcs="kzg")
    with pytest.raises(ValueError):
        DeviceWorkload(ctx, 3, pcs="dory")  # sigma = 4 > n_vars: a matrix row wider than an address's cycles
