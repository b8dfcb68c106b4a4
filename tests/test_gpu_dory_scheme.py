"""GPU parity: jolt_amd/dory_scheme.py -- DoryScheme::{commit, open} for one polynomial held as field elements (the reference's commit_open_verify_round_trip) --
and DoryWitnessCommitment(blocks=...) joined into the opening of a committed trace in both placements.  Gamma1 / Gamma2 / H1 / H2 are planted progressions, so
every hint element, tier-2 value and message is a number modulo r from tests/dory_open_model.py; the evaluation is the oracle's.  No tolerance anywhere."""
import numpy as np
import pytest

import dory_open_model as OM
import oracle_lib as O
import pairing_model as PM
from dory_groups import G1, G2, R, fr_int, fr_ints, progression, rand_ints
from jolt_amd import dory_scheme, ffi
from jolt_amd.dory_commit import DoryWitnessCommitment
from jolt_amd.dory_open import DorySetup
from test_gpu_dory_commit import ONE
from test_gpu_dory_open import check_message
from util import rand_fr

pytestmark = pytest.mark.gpu
N_SETUP = 32


@pytest.fixture(scope="module")
def ctx():
    c = ffi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def bases():
    a0, ad, b0, bd, kh1, kh2 = rand_ints(6, 1410)
    kg1, gamma1 = progression(G1, a0, ad, N_SETUP)
    kg2, gamma2 = progression(G2, b0, bd, N_SETUP)
    return dict(kg1=kg1, gamma1=gamma1, kg2=kg2, gamma2=gamma2, kh1=kh1, h1=G1.point(kh1), kh2=kh2, h2=G2.point(kh2, rep=3))


@pytest.fixture(scope="module")
def setup(ctx, bases):
    s = DorySetup(ctx, bases["gamma1"], bases["gamma2"], bases["h1"], bases["h2"])
    yield s
    s.close()


def drive(opening, challenges, gamma):
    """every message of a DoryOpening under the given challenges"""
    vmv = opening.vmv_message()
    rounds = [opening.reduce.round(fr_int(b), fr_int(pow(b, -1, R)), fr_int(a), fr_int(pow(a, -1, R))) for b, a in challenges]
    final = opening.final_message(fr_int(gamma), fr_int(pow(gamma, -1, R)))
    return vmv, rounds, final


def check_proof(got, proof):
    vmv, rounds, final = got
    check_message(vmv, proof["vmv"], "tta", "vmv")
    assert len(rounds) == len(proof["rounds"])
    for r, ((first, second), (want_first, want_second)) in enumerate(zip(rounds, proof["rounds"])):
        check_message(first, want_first, "ttttab", ("first", r))
        check_message(second, want_second, "ttaabb", ("second", r))
    check_message(final, proof["final"], "ab", "final")


def flat(vmv, rounds, final):
    return list(vmv) + [x for f, s in rounds for x in f + s] + list(final)


def tampered(proof):
    """the proof with one element changed, once per message kind"""
    c, d2, e1 = proof["vmv"]
    yield dict(proof, vmv=(c, d2, (e1 + 1) % R))
    first, second = proof["rounds"][0]
    yield dict(proof, rounds=[(((first[0] + 1) % R,) + tuple(first[1:]), second)] + proof["rounds"][1:])
    w1, w2 = proof["final"]
    yield dict(proof, final=(w1, (w2 + 1) % R))


@pytest.mark.parametrize("n", [4, 5, 10])
def test_commit_then_open_a_random_polynomial(ctx, bases, setup, n):
    """n = 4: the reference's own test size; n = 5: nu < sigma; n = 10: the setup's full width"""
    nu, sigma = dory_scheme.matrix_shape(1 << n)
    assert (nu, sigma) == (n - (n + 1) // 2, (n + 1) // 2)
    rows, cols = 1 << nu, 1 << sigma
    kg1, kg2, kh1, kh2 = bases["kg1"][:cols], bases["kg2"][:cols], bases["kh1"], bases["kh2"]
    dev_srs = ctx.srs_upload(bases["gamma1"][:cols])
    evals = rand_fr(1 << n, 1900 + n)
    ints = [int(x) for x in O.from_mont(evals)]
    matrix = [ints[r * cols:(r + 1) * cols] for r in range(rows)]
    table = ctx.upload(evals)
    commitment, hint = dory_scheme.commit(setup, dev_srs, table)
    # ---- every hint row, and the tier-2 value against the pairing model
    point = rand_fr(n, 1910 + n)
    L, Rr = [int(x) for x in O.from_mont(O.eq_evals(point[:nu]))], [int(x) for x in O.from_mont(O.eq_evals(point[nu:]))]
    t_rows, combined, v, y = OM.statement(kg1, kg2, matrix, L, Rr)
    got_hint = hint.download()
    assert got_hint.shape[0] == rows
    for r in range(rows):
        assert np.array_equal(got_hint[r, 8:12], ONE) and G1.same(got_hint[r], t_rows[r]), r
    assert np.array_equal(commitment, PM.gt_to_abi(PM.expected([combined], [1])))
    # ---- the opening: L^T M R is the multilinear evaluation under the library's variable order
    op = dory_scheme.open(setup, table, hint, point)
    assert (op.nu, op.sigma) == (nu, sigma)
    assert np.array_equal(op.left.download(), fr_ints(L)) and np.array_equal(op.right.download(), fr_ints(Rr))
    assert np.array_equal(op.v.download(), fr_ints(v))
    want_y = O.poly_evaluate(evals, point)
    assert np.array_equal(np.asarray(op.evaluation()).reshape(-1), np.asarray(want_y).reshape(-1)) and np.array_equal(fr_int(y), np.asarray(want_y).reshape(-1))
    challenges, gamma, d = [tuple(rand_ints(2, 1920 + 16 * n + j)) for j in range(sigma)], rand_ints(1, 1903)[0], rand_ints(1, 1904)[0]
    proof = OM.prove(kg1, kg2, kh1, kh2, t_rows, v, L, Rr, challenges, gamma)
    got = drive(op.opening, challenges, gamma)
    check_proof(got, proof)
    args = (kg1, kg2, kh1, kh2, combined, y, L, Rr)
    assert OM.verify(*args, proof, challenges, gamma, d)
    assert not any(OM.verify(*args, bad, challenges, gamma, d) for bad in tampered(proof))
    assert not OM.verify(kg1, kg2, kh1, kh2, combined, (y + 1) % R, L, Rr, proof, challenges, gamma, d)
    op.close()
    # ---- a second commitment and opening of the same inputs: the same bytes
    commitment2, hint2 = dory_scheme.commit(setup, dev_srs, table)
    assert np.array_equal(commitment2, commitment) and np.array_equal(hint2.download(), got_hint)
    op2 = dory_scheme.open(setup, table, hint2, point)
    got2 = drive(op2.opening, challenges, gamma)
    assert all(np.array_equal(a, b) for a, b in zip(flat(*got), flat(*got2)))
    op2.close()
    for t in (hint, hint2, table, dev_srs):
        t.free()


def test_scheme_checks_shapes_before_anything_is_enqueued(ctx, bases, setup):
    dev_srs = ctx.srs_upload(bases["gamma1"][:4])
    odd, wide, fine = ctx.upload(rand_fr(12, 1930)), ctx.upload(rand_fr(1 << 11, 1931)), ctx.upload(rand_fr(16, 1932))
    mid = ctx.upload(rand_fr(64, 1933))
    with pytest.raises(ValueError):
        dory_scheme.commit(setup, dev_srs, odd)    # not a power of two
    with pytest.raises(ValueError):
        dory_scheme.commit(setup, dev_srs, wide)   # sigma = 6 against a setup of 32
    with pytest.raises(ValueError):
        dory_scheme.commit(setup, dev_srs, mid)    # sigma = 3 against an SRS of 4
    commitment, hint = dory_scheme.commit(setup, dev_srs, fine)
    g2v = ctx.dory_state_alloc(ffi.DORY_KIND_G2, 4)
    for args in ((fine, hint, rand_fr(3, 1934)),           # a point of the wrong length
                 (fine, (hint, 0, 2), rand_fr(4, 1935)),   # half the hint
                 (fine, g2v, rand_fr(4, 1936)),            # not a G1 vector
                 (odd, hint, rand_fr(4, 1937))):
        with pytest.raises(ValueError):
            dory_scheme.open(setup, *args)
    op = dory_scheme.open(setup, fine, hint, rand_fr(4, 1938))
    op.close()
    for t in (odd, wide, fine, mid, hint, g2v, dev_srs):
        t.free()


@pytest.mark.parametrize("order", ["cycle_major", "address_major"])
def test_commit_to_open_with_blocks_joined(ctx, bases, order):
    """The commit-to-open instance of test_gpu_dory_commit.py (log_t = 6, log_k = 4, sigma = nu = 5) with one block of m = 4 and one of m = 5 joined: ragged hints (4
    rows of 4 and 4 rows of 8 columns beside the trace's 32 rows of 32), the model's matrix is the joint matrix with the blocks added top-left, nothing is uploaded between commit
    and open."""
    from test_gpu_dory_opening import joint_dense_table, make_batch
    log_t, log_k, sigma, nu = 6, 4, 5, 5
    rows, n, T = 1 << nu, 1 << sigma, 1 << log_t
    batch = make_batch(log_t, log_k, n_dense=1, seed=1300)
    K = batch["k"]
    kg1, kg2, kh1, kh2 = bases["kg1"][:n], bases["kg2"][:n], bases["kh1"], bases["kh2"]
    setup = DorySetup(ctx, bases["gamma1"], bases["gamma2"], bases["h1"], bases["h2"])
    dev_srs = ctx.srs_upload(bases["gamma1"][:n])
    srcs = [ctx.onehot(i, K) for i in batch["idx"]]
    dense_ints = ctx.ints(batch["dense_ints"][0])
    block_host = [rand_fr(16, 1940), rand_fr(32, 1941)]
    block_ints = [[int(x) for x in O.from_mont(b)] for b in block_host]
    block_sigmas = [2, 3]
    blocks = [ctx.upload(b) for b in block_host]
    am = order == "address_major"
    commitment = DoryWitnessCommitment(setup, dev_srs, srcs, [dense_ints], sigma, order=order, log_k=log_k if am else None, blocks=blocks)
    trace_rows = [rows] * 6 if am else [rows] * 5 + [T >> sigma]
    assert [r for _, _, r in commitment.hints] == trace_rows + [4, 4]  # ragged: the blocks have 2^(4 - 2) and 2^(5 - 3) rows
    # ---- the block hints and their tier-2 values from the definition
    for (vec, first, count), ints, sd in zip(commitment.hints[6:], block_ints, block_sigmas):
        got = vec.download(first, count)
        logs = [sum(ints[(r << sd) + j] * kg1[j] for j in range(1 << sd)) % R for r in range(count)]
        assert all(np.array_equal(e[8:12], ONE) and G1.same(e, lg) for e, lg in zip(got, logs))
    tier2 = commitment.commit()
    assert len(tier2) == 8
    for got, ints, sd in zip(tier2[6:], block_ints, block_sigmas):
        logs = [sum(ints[(r << sd) + j] * kg1[j] for j in range(1 << sd)) % R for r in range(len(ints) >> sd)]
        assert np.array_equal(got, PM.gt_to_abi(PM.expected([sum(lg * kg2[i] for i, lg in enumerate(logs)) % R], [1])))
    # ---- the joint opening over the same vectors
    block_scalars = rand_fr(2, 1942)
    scalars = np.concatenate([batch["gamma"], batch["dgamma"], block_scalars])
    r_row, r_col = rand_fr(nu, 1301), rand_fr(sigma, 1302)
    left_host, right_host = O.eq_evals(r_row), O.eq_evals(r_col)
    left, right = ctx.upload(left_host), ctx.upload(right_host)
    dense = [ctx.upload(batch["dense"][0])]
    cells = [int(x) for x in O.from_mont(joint_dense_table(batch))]  # cycle-major: index k * T + t
    if am:
        trace = ctx.dory_fold_rows_grid_am(srcs, batch["gamma"], dense, batch["dgamma"], log_k, 0, sigma, left)
        cells = [cells[(i & (K - 1)) * T + (i >> log_k)] for i in range(K * T)]
    else:
        trace = ctx.dory_fold_rows_grid(srcs, batch["gamma"], dense, batch["dgamma"], log_k, sigma, left)
    v_table = ctx.dory_fold_rows_blocks(blocks, block_sigmas, block_scalars, sigma, left, trace)
    for ints, sd, s in zip(block_ints, block_sigmas, [int(x) for x in O.from_mont(block_scalars)]):
        for i, x in enumerate(ints):
            at = ffi.host_dory_block_index(sd, sigma, i)
            cells[at] = (cells[at] + s * x) % R
    matrix = [cells[r * n:(r + 1) * n] for r in range(rows)]
    L, Rr = [int(x) for x in O.from_mont(left_host)], [int(x) for x in O.from_mont(right_host)]
    t_rows, combined, v, y = OM.statement(kg1, kg2, matrix, L, Rr)
    assert np.array_equal(v_table.download(), fr_ints(v))
    challenges, gamma, d = [tuple(rand_ints(2, 1310 + j)) for j in range(sigma)], rand_ints(1, 1303)[0], rand_ints(1, 1304)[0]
    proof = OM.prove(kg1, kg2, kh1, kh2, t_rows, v, L, Rr, challenges, gamma)
    from jolt_amd.dory_open import DoryOpening
    op = DoryOpening(setup, commitment.hints, scalars, v_table, left, right, nu, sigma)
    check_proof(drive(op, challenges, gamma), proof)
    op.close()
    assert OM.verify(kg1, kg2, kh1, kh2, combined, y, L, Rr, proof, challenges, gamma, d)
    commitment.close()
    assert commitment.hints == []
    for t in dense + blocks + [trace, v_table, left, right, dense_ints, dev_srs] + srcs:
        t.free()
    setup.close()
