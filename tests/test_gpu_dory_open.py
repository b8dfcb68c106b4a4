"""GPU parity: Dory evaluation proofs on resident vectors (jolt_amd/dory_open.py) -- the four entries that build an opening's state on the device
(jolt_dory_state_alloc, _from_table, _combine_hints, _fixed_base_mul of dory_resident.hip), whole openings against the log-space model of tests/dory_open_model.py
and its verifier, the verifier's final equation in the groups themselves, and an opening of a committed batch.  Points are made through their discrete logarithms
(tests/dory_groups.py), so every expected value is arithmetic modulo r plus one model power or one reference scalar multiplication.  Points are compared as group
elements, GT and Fr bit for bit; no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import dory_open_model as OM
import g2_model as M
import oracle_lib as O
import pairing_model as PM
from dory_groups import G1, G2, GROUPS, R, SHARED_SCALARS, fr_int, fr_ints, plant, progression, rand_ints
from jolt_amd import ffi
from jolt_amd.dory_open import DoryOpening, DorySetup, dory_commit_tier2
from util import rand_fr

pytestmark = pytest.mark.gpu
group_ids = lambda G: G.name  # noqa: E731
KIND = {"g1": ffi.DORY_KIND_G1, "g2": ffi.DORY_KIND_G2}
WIDTH = {ffi.DORY_KIND_G1: 12, ffi.DORY_KIND_G2: 24, ffi.DORY_KIND_FR: 4}
SENTINEL = 0xA5A5A5A5A5A5A5A5
N_SETUP = 64  # 2^sigma of the largest opening below


@pytest.fixture(scope="module")
def ctx():
    c = ffi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def bases():
    """Gamma1, Gamma2 of 64 points and H1, H2 with their logarithms; never written"""
    a0, ad, b0, bd, kh1, kh2 = rand_ints(6, 900)
    kg1, gamma1 = progression(G1, a0, ad, N_SETUP)
    kg2, gamma2 = progression(G2, b0, bd, N_SETUP)
    return dict(kg1=kg1, gamma1=gamma1, kg2=kg2, gamma2=gamma2, kh1=kh1, h1=G1.point(kh1), kh2=kh2, h2=G2.point(kh2, rep=3))


@pytest.fixture(scope="module")
def setup(ctx, bases):
    s = DorySetup(ctx, bases["gamma1"], bases["gamma2"], bases["h1"], bases["h2"])
    yield s
    s.close()


def gt_of(log):
    return PM.gt_to_abi(PM.expected([log], [1]))


def same_element(G, a, b):
    if G is G1:
        return bool(O.g1_on_curve(a)) and bool(O.g1_eq(a, b))
    p = M.from_abi(a)
    return M.on_curve(p) and p == M.from_abi(b)


def _raw(name, *args):
    conv = [a.ctypes.data_as(C.c_void_p) if isinstance(a, np.ndarray) else a for a in args]
    return getattr(ffi.lib(), name)(*conv)


def identity(kind):
    out = np.zeros(WIDTH[kind], dtype=np.uint64)
    if kind != ffi.DORY_KIND_FR:
        w = WIDTH[kind] // 3
        one = G1.point(0)[:4]  # the Montgomery one of Fq, from the oracle's identity (1, 1, 0)
        out[0:4], out[w:w + 4] = one, one
    return out


# ------------------------------------------------------------------------------------------------------ the four entries
@pytest.mark.parametrize("kind", [ffi.DORY_KIND_G1, ffi.DORY_KIND_G2, ffi.DORY_KIND_FR], ids=["g1", "g2", "fr"])
def test_alloc_gives_neutral_elements(ctx, kind):
    assert np.array_equal(identity(ffi.DORY_KIND_G1), G1.point(0)) and np.array_equal(identity(ffi.DORY_KIND_G2), G2.point(0))
    for n in (0, 1, 65):
        v = ctx.dory_state_alloc(kind, n)
        assert len(v) == n and v.device_kind() == kind
        got = v.download()
        assert got.shape == (n, WIDTH[kind]) and all(np.array_equal(row, identity(kind)) for row in got)
        v.free()


@pytest.mark.parametrize("n", [1, 64, 65])
def test_from_table_copies_a_range(ctx, n):
    host = rand_fr(n + 7, 910 + n)
    table = ctx.upload(host)
    dst = ctx.dory_state_alloc(ffi.DORY_KIND_FR, n + 5)
    ctx.dory_state_from_table(table, (dst, 3, n), table_first=5)  # odd firsts on both sides
    got = dst.download()
    assert np.array_equal(got[3:3 + n], host[5:5 + n]) and not got[:3].any() and not got[3 + n:].any()
    dst.free()
    table.free()


def combine_case(rows, n_hints, seed):
    """n_hints progressions of ragged lengths with their logarithms, and scalars with 0, 1 and r - 1 among them"""
    lengths = [rows] * n_hints
    if n_hints >= 3:
        lengths[-2], lengths[-1] = max(rows // 2, 1), max(rows // 16, 1)
    starts = rand_ints(2 * n_hints, seed)
    logs, pts = zip(*[progression(G1, starts[2 * i], starts[2 * i + 1], lengths[i]) for i in range(n_hints)])
    scalars = rand_ints(n_hints, seed + 1)
    if n_hints >= 3:
        scalars[0], scalars[1] = 1, R - 1
    if n_hints >= 5:
        scalars[3] = 0
    if n_hints == 1:
        scalars[0] = R - 1
    return lengths, [list(k) for k in logs], [p.copy() for p in pts], scalars


@pytest.mark.parametrize("rows,n_hints", [(1, 1), (16, 3), (130, 5)])
def test_combine_hints_on_resident_views(ctx, rows, n_hints):
    lengths, logs, pts, scalars = combine_case(rows, n_hints, 920 + rows)
    if rows >= 16:  # row 2 of the first two hints (scalars 1 and r - 1) the same point: with the others at the identity, the combined row is the identity
        plant(G1, logs[1], pts[1], 2, logs[0][2])
        for k in range(2, n_hints):
            if lengths[k] > 2:
                plant(G1, logs[k], pts[k], 2, 0)
    # every hint sits at an odd first inside a longer vector
    vecs = [ctx.dory_vec_upload(ffi.DORY_KIND_G1, np.concatenate([pts[k][:1]] * (k + 1) + [pts[k]])) for k in range(n_hints)]
    views = [(vecs[k], k + 1, lengths[k]) for k in range(n_hints)]
    out_first = 3
    out = ctx.dory_state_alloc(ffi.DORY_KIND_G1, rows + 5)
    assert ctx.dory_state_combine_hints(views, fr_ints(scalars), out, out_first) == rows
    got = out.download()
    ident = identity(ffi.DORY_KIND_G1)
    assert all(np.array_equal(got[i], ident) for i in list(range(out_first)) + list(range(out_first + rows, rows + 5)))  # nothing outside the view is written
    want = [sum(scalars[k] * logs[k][r] for k in range(n_hints) if r < lengths[k]) % R for r in range(rows)]
    ref = ctx.dory_combine_hints(pts, fr_ints(scalars))  # the host-pointer entry on the same arrays
    for r in range(rows):
        assert same_element(G1, got[out_first + r], ref[r]), r
    for r in sorted({0, min(1, rows - 1), min(2, rows - 1), rows // 16, rows // 2, rows - 1}):
        assert G1.same(got[out_first + r], want[r]), r
    if rows >= 16:
        assert want[2] == 0 and G1.z_is_zero(got[out_first + 2])
    for v in vecs + [out]:
        v.free()


@pytest.mark.parametrize("n", [1, 64, 65])
@pytest.mark.parametrize("G", GROUPS, ids=group_ids)
def test_fixed_base_mul_on_resident_views(ctx, G, n):
    kb = rand_ints(1, 930 + G.width)[0]
    base = G.point(kb, rep=2)
    ss = (SHARED_SCALARS + rand_ints(n, 931 + n))[:n] if n > 1 else [SHARED_SCALARS[3]]
    scalars = ctx.dory_vec_upload(ffi.DORY_KIND_FR, np.concatenate([fr_ints([7]), fr_ints(ss)]))
    out = ctx.dory_state_alloc(KIND[G.name], n + 4)
    ctx.dory_state_fixed_base_mul(KIND[G.name], base, (scalars, 1, n), (out, 3, n))
    got = out.download()
    ident = identity(KIND[G.name])
    assert all(np.array_equal(got[i], ident) for i in (0, 1, 2, n + 3))
    ref = getattr(ctx, f"dory_{G.name}_fixed_base_mul")(base, fr_ints(ss))
    assert all(same_element(G, got[3 + i], ref[i]) for i in range(n))
    for i in sorted({0, min(1, n - 1), min(3, n - 1), min(4, n - 1), n - 1}):
        assert G.same(got[3 + i], ss[i] * kb), i
        if ss[i] % R == 0:
            assert G.z_is_zero(got[3 + i])
    # base = the identity: every multiple is the identity, as (1, 1, 0)
    ctx.dory_state_fixed_base_mul(KIND[G.name], G.point(0), (scalars, 1, n), (out, 3, n))
    assert all(np.array_equal(row, ident) for row in out.download())
    scalars.free()
    out.free()


def test_refusals_write_nothing_and_leave_the_context_usable(ctx, bases):
    n = 8
    h, size_t = ctx.h, C.c_size_t
    zero, two, big = size_t(0), size_t(2), size_t(2**64 - 1)
    g1v = ctx.dory_vec_upload(ffi.DORY_KIND_G1, bases["gamma1"][:n])
    g2v = ctx.dory_vec_upload(ffi.DORY_KIND_G2, bases["gamma2"][:n])
    frv = ctx.dory_vec_upload(ffi.DORY_KIND_FR, fr_ints(list(range(1, n + 1))))
    table = ctx.upload(fr_ints(list(range(10, 10 + n))))
    g1_0, g2_0, fr_0 = g1v.download(), g2v.download(), frv.download()
    handle = C.c_void_p()
    assert _raw("jolt_dory_state_alloc", h, C.c_int32(7), size_t(4), C.byref(handle)) == 1 and not handle.value
    assert _raw("jolt_dory_state_alloc", h, C.c_int32(0), size_t(4), None) == 1
    # from_table: a vector of the wrong kind, one past the end on either side, a first that wraps
    assert _raw("jolt_dory_state_from_table", h, table.h, zero, g1v.h, zero, two) == 1
    assert _raw("jolt_dory_state_from_table", h, table.h, size_t(n - 1), frv.h, zero, two) == 1
    assert _raw("jolt_dory_state_from_table", h, table.h, zero, frv.h, size_t(n - 1), two) == 1
    assert _raw("jolt_dory_state_from_table", h, table.h, big, frv.h, zero, two) == 1
    assert _raw("jolt_dory_state_from_table", h, table.h, zero, frv.h, big, two) == 1
    assert _raw("jolt_dory_state_from_table", h, None, zero, frv.h, zero, two) == 1
    # combine_hints: no hints, a G2 hint, an Fr out, a view past the end, a wrapping first, out overlapping a hint, a scalar that is not canonical
    sc = fr_ints([3, 5])
    bad_sc = sc.copy()
    bad_sc[1] = np.array(O.int_to_limbs(R), dtype=np.uint64)
    out = ctx.dory_state_alloc(ffi.DORY_KIND_G1, n)
    out_0 = out.download()

    def combine(hints, firsts, rows, scalars, dst, dst_first, count=2):
        return _raw("jolt_dory_state_combine_hints", h, (C.c_void_p * 2)(*hints), (size_t * 2)(*firsts), (size_t * 2)(*rows), size_t(count), scalars, dst, size_t(dst_first))

    assert combine([g1v.h, g1v.h], [0, 0], [4, 4], sc, out.h, 0, count=0) == 1
    assert combine([g1v.h, g2v.h], [0, 0], [4, 4], sc, out.h, 0) == 1
    assert combine([g1v.h, g1v.h], [0, 0], [4, 4], sc, frv.h, 0) == 1
    assert combine([g1v.h, g1v.h], [0, n - 3], [4, 4], sc, out.h, 0) == 1          # [5, 9) leaves the hint
    assert combine([g1v.h, g1v.h], [0, 2**64 - 1], [4, 2], sc, out.h, 0) == 1      # first + rows wraps to 1
    assert combine([g1v.h, g1v.h], [0, 0], [4, 4], sc, out.h, n - 3) == 1          # [5, 9) leaves out
    assert combine([g1v.h, g1v.h], [0, 0], [4, 4], sc, out.h, 2**64 - 1) == 1
    assert combine([g1v.h, g1v.h], [0, 4], [4, 2], sc, g1v.h, 3) == 1              # out [3, 7) of the vector that holds the hints [0, 4) and [4, 6)
    assert combine([g1v.h, g1v.h], [0, 0], [4, 4], bad_sc, out.h, 0) == 1
    assert combine([g1v.h, None], [0, 0], [4, 4], sc, out.h, 0) == 1
    # fixed_base_mul: kinds, views, a base off its curve or not canonical
    base1, base2 = bases["h1"], bases["h2"]
    off1, off2 = base1.copy(), base2.copy()
    off1[4] ^= np.uint64(1)
    off2[1] ^= np.uint64(1)
    not_canonical = base1.copy()
    not_canonical[0:4] = np.array(O.int_to_limbs(O.Q_MOD), dtype=np.uint64)

    def fixed(kind, base, s, s_first, dst, dst_first, count):
        return _raw("jolt_dory_state_fixed_base_mul", h, C.c_int32(kind), base, s, size_t(s_first), dst, size_t(dst_first), size_t(count))

    assert fixed(ffi.DORY_KIND_FR, base1, frv.h, 0, out.h, 0, 2) == 1
    assert fixed(ffi.DORY_KIND_G2, base2, frv.h, 0, out.h, 0, 2) == 1              # out is a G1 vector
    assert fixed(ffi.DORY_KIND_G1, base1, g1v.h, 0, out.h, 0, 2) == 1              # the scalars are no Fr vector
    assert fixed(ffi.DORY_KIND_G1, base1, frv.h, n - 1, out.h, 0, 2) == 1
    assert fixed(ffi.DORY_KIND_G1, base1, frv.h, 0, out.h, n - 1, 2) == 1
    assert fixed(ffi.DORY_KIND_G1, base1, frv.h, 2**64 - 1, out.h, 0, 2) == 1
    assert fixed(ffi.DORY_KIND_G1, base1, frv.h, 0, out.h, 2**64 - 1, 2) == 1
    assert fixed(ffi.DORY_KIND_G1, off1, frv.h, 0, out.h, 0, 2) == 1
    assert fixed(ffi.DORY_KIND_G1, not_canonical, frv.h, 0, out.h, 0, 2) == 1
    assert fixed(ffi.DORY_KIND_G2, off2, frv.h, 0, g2v.h, 0, 2) == 1
    assert fixed(ffi.DORY_KIND_G1, None, frv.h, 0, out.h, 0, 2) == 1
    # nothing was enqueued: every destination holds its bytes; then valid calls on the same context
    assert np.array_equal(g1v.download(), g1_0) and np.array_equal(g2v.download(), g2_0) and np.array_equal(frv.download(), fr_0) and np.array_equal(out.download(), out_0)
    assert combine([g1v.h, g1v.h], [0, 4], [2, 2], sc, g1v.h, 6) == 0              # out [6, 8) beside the hints [0, 2) and [4, 6) of the same vector
    kg1 = bases["kg1"]
    got = g1v.download()
    assert G1.same(got[6], 3 * kg1[0] + 5 * kg1[4]) and G1.same(got[7], 3 * kg1[1] + 5 * kg1[5]) and np.array_equal(got[:6], g1_0[:6])
    ctx.dory_state_from_table(table, (frv, 1, 2), table_first=3)
    assert np.array_equal(frv.download(1, 2), fr_ints([13, 14]))
    for v in (g1v, g2v, frv, out, table):
        v.free()


# ------------------------------------------------------------------------------------------------------ whole openings
def opening_inputs(ctx, bases, nu, sigma, seed):
    """A random 2^nu x 2^sigma matrix of small entries with L, R; its row commitments T' split into three hints with known logarithms -- a progression A, a short
    progression S of half the rows (the ragged case) and B chosen so that c_A A + c_B B + c_S S = T' row by row"""
    rng = np.random.default_rng(seed)
    rows, n = 1 << nu, 1 << sigma
    kg1, kg2 = bases["kg1"][:n], bases["kg2"][:n]
    matrix = [[int(x) for x in rng.integers(0, 1 << 62, size=n)] for _ in range(rows)]
    left, right = rand_ints(rows, seed + 1), rand_ints(n, seed + 2)
    t_rows, commitment, v, y = OM.statement(kg1, kg2, matrix, left, right)
    a0, ad, s0, sd, c_a, c_b, c_s = rand_ints(7, seed + 3)
    short = max(rows // 2, 1)
    ka, pa = progression(G1, a0, ad, rows)
    ks, ps = progression(G1, s0, sd, short)
    kb = [(t_rows[i] - c_a * ka[i] - (c_s * ks[i] if i < short else 0)) * pow(c_b, -1, R) % R for i in range(rows)]
    pb = np.stack([G1.point(k) for k in kb])
    hints = [ctx.dory_vec_upload(ffi.DORY_KIND_G1, p) for p in (pa, pb, ps)]
    tables = [ctx.upload(fr_ints(x)) for x in (v, left, right)]
    return dict(nu=nu, sigma=sigma, t_rows=t_rows, commitment=commitment, v=v, y=y, left=left, right=right, hints=hints, scalars=fr_ints([c_a, c_b, c_s]),
                tables=tables, challenges=[tuple(rand_ints(2, seed + 10 + k)) for k in range(sigma)], gamma=rand_ints(1, seed + 4)[0], d=rand_ints(1, seed + 5)[0])


def check_message(got, want, kinds, what):
    assert len(got) == len(want) == len(kinds)
    for j, (g, w, kind) in enumerate(zip(got, want, kinds)):
        if kind == "t":
            assert np.array_equal(g, gt_of(w)), (what, j)
        else:
            assert (G1 if kind == "a" else G2).same(g, w), (what, j)


def run_opening(setup, inp):
    """every message of one opening, as the device gives it"""
    v_table, left, right = inp["tables"]
    op = DoryOpening(setup, inp["hints"], inp["scalars"], v_table, left, right, inp["nu"], inp["sigma"])
    vmv = op.vmv_message()
    padding = (op.v1.download(), op.s2.download())
    rounds = []
    for beta, alpha in inp["challenges"]:
        rounds.append(op.reduce.round(fr_int(beta), fr_int(pow(beta, -1, R)), fr_int(alpha), fr_int(pow(alpha, -1, R))))
    gamma = inp["gamma"]
    with pytest.raises(ValueError):
        op.final_message(fr_int(gamma), fr_int(gamma))
    final = op.final_message(fr_int(gamma), fr_int(pow(gamma, -1, R)))
    op.close()
    return vmv, rounds, final, padding


@pytest.mark.parametrize("nu,sigma", [(1, 1), (2, 2), (2, 3), (3, 3), (5, 6)])
def test_whole_opening_against_the_model(ctx, bases, setup, nu, sigma):
    inp = opening_inputs(ctx, bases, nu, sigma, 1000 + 10 * nu + sigma)
    n, rows = 1 << sigma, 1 << nu
    kg1, kg2, kh1, kh2 = bases["kg1"][:n], bases["kg2"][:n], bases["kh1"], bases["kh2"]
    proof = OM.prove(kg1, kg2, kh1, kh2, inp["t_rows"], inp["v"], inp["left"], inp["right"], inp["challenges"], inp["gamma"])
    vmv, rounds, final, (v1, s2) = run_opening(setup, inp)
    check_message(vmv, proof["vmv"], "tta", "vmv")
    assert len(rounds) == sigma
    for r, ((first, second), (want_first, want_second)) in enumerate(zip(rounds, proof["rounds"])):
        check_message(first, want_first, "ttttab", ("first", r))
        check_message(second, want_second, "ttaabb", ("second", r))
    check_message(final, proof["final"], "ab", "final")
    # the messages were just checked to be the model's: its verifier accepts them, and rejects a wrong evaluation
    args = (kg1, kg2, kh1, kh2, inp["commitment"])
    assert OM.verify(*args, inp["y"], inp["left"], inp["right"], proof, inp["challenges"], inp["gamma"], inp["d"])
    assert not OM.verify(*args, inp["y"] + 1, inp["left"], inp["right"], proof, inp["challenges"], inp["gamma"], inp["d"])
    # the padding: rows past 2^nu of v1 are identities, entries past 2^nu of s2 are zero, before the first round
    ident = identity(ffi.DORY_KIND_G1)
    assert v1.shape[0] == s2.shape[0] == n and np.array_equal(s2[:rows], fr_ints(inp["left"]))
    assert all(np.array_equal(v1[i], ident) for i in range(rows, n)) and not s2[rows:].any()
    if (nu, sigma) == (2, 3):
        assert n - rows == 4
    # the tier-2 commitment of the combined rows
    combined = ctx.dory_state_alloc(ffi.DORY_KIND_G1, rows)
    ctx.dory_state_combine_hints(inp["hints"], inp["scalars"], combined)
    assert np.array_equal(dory_commit_tier2(setup, combined), gt_of(inp["commitment"]))
    combined.free()
    # a second opening of the same inputs: the same bytes
    vmv2, rounds2, final2, _ = run_opening(setup, inp)
    flat = lambda vmv, rounds, final: list(vmv) + [x for f, s in rounds for x in f + s] + list(final)  # noqa: E731
    assert all(np.array_equal(x, y) for x, y in zip(flat(vmv, rounds, final), flat(vmv2, rounds2, final2)))
    for t in inp["hints"] + inp["tables"]:
        t.free()


def test_opening_refuses_wrong_shapes_before_anything_is_enqueued(ctx, bases, setup):
    inp = opening_inputs(ctx, bases, 1, 2, 1100)
    v_table, left, right = inp["tables"]
    with pytest.raises(ValueError):
        DoryOpening(setup, inp["hints"], inp["scalars"], v_table, right, left, 2, 1)       # nu > sigma
    with pytest.raises(ValueError):
        DoryOpening(setup, inp["hints"], inp["scalars"], v_table, right, right, 1, 2)      # left of 2^sigma entries
    with pytest.raises(ValueError):
        DoryOpening(setup, inp["hints"], inp["scalars"], left, left, right, 1, 2)          # v of 2^nu entries
    with pytest.raises(ValueError):
        DoryOpening(setup, inp["hints"], inp["scalars"][:2], v_table, left, right, 1, 2)   # a scalar short
    with pytest.raises(ValueError):
        DoryOpening(setup, inp["hints"], inp["scalars"], v_table, left, right, 1, 7)       # more columns than the setup has bases
    op = DoryOpening(setup, inp["hints"], inp["scalars"], v_table, left, right, 1, 2)
    with pytest.raises(ValueError):
        op.final_message(fr_int(2), fr_int(pow(2, -1, R)))                                 # before the rounds: n != 1
    op.vmv_message()
    with pytest.raises(ValueError):
        op.final_message(fr_int(2), fr_int(pow(2, -1, R)))
    op.close()
    for t in inp["hints"] + inp["tables"]:
        t.free()


# ------------------------------------------------------------------------------- the verifier's equation in the groups
def gt_mul(*xs):
    acc = xs[0]
    for x in xs[1:]:
        acc = ffi.host_fq12_op(ffi.FQ12_MUL, acc, x)
    return acc


def gt_pow(x, k):
    return ffi.host_gt_pow(x, fr_int(k))


def pair(g1s, g2s):
    return ffi.host_final_exponentiation(ffi.host_miller_loop(np.asarray(g1s).reshape(-1, 12), np.asarray(g2s).reshape(-1, 24)))


def g1_lin(*terms):
    """sum of k * P over (k, P), with the oracle's group law"""
    acc = O.g1_identity()
    for k, p in terms:
        acc = O.g1_add(acc, O.g1_scalar_mul(p, fr_int(k)))
    return acc


def g2_lin(*terms):
    acc = G2.point(0)
    for k, p in terms:
        acc = ffi.host_g2_add(acc, ffi.host_g2_scalar_mul(p, fr_int(k)))
    return acc


def verify_in_the_groups(bases, commitment_gt, y, left, right, vmv, rounds, final, challenges, gamma, d):
    """The verifier of tests/dory_open_model.py on group elements: GT through the library's HOST functions (jolt_host_fq12_op MUL, jolt_host_gt_pow,
    jolt_host_miller_loop + jolt_host_final_exponentiation, which tests/pairing_model.py pins), G2 through jolt_host_g2_scalar_mul / _add, G1 through the oracle.
    This is library host code on the checking side; none of it is the device code under test."""
    inv = lambda x: pow(x, -1, R)  # noqa: E731
    n = len(right)
    g1, g2, h1, h2 = bases["gamma1"][:n], bases["gamma2"][:n], bases["h1"], bases["h2"]
    c, d2, e1 = vmv
    if not np.array_equal(pair([e1], [h2]), d2):
        return False
    d1, e2 = commitment_gt, g2_lin((y, h2))
    s1, s2 = list(right), OM.pad(left, n)
    for (first, second), (beta, alpha) in zip(rounds, challenges):
        h, bi, ai = n // 2, inv(beta), inv(alpha)
        chi, delta_l, delta_1r, delta_2r = pair(g1[:n], g2[:n]), pair(g1[:h], g2[:h]), pair(g1[h:n], g2[:h]), pair(g1[:h], g2[h:n])
        d1l, d1r, d2l, d2r, e1b, e2b = first
        cp, cm, e1p, e1m, e2p, e2m = second
        c = gt_mul(c, chi, gt_pow(d2, beta), gt_pow(d1, bi), gt_pow(cp, alpha), gt_pow(cm, ai))
        d1 = gt_mul(gt_pow(gt_mul(d1l, gt_pow(delta_l, beta)), alpha), d1r, gt_pow(delta_1r, beta))
        d2 = gt_mul(gt_pow(gt_mul(d2l, gt_pow(delta_l, bi)), ai), d2r, gt_pow(delta_2r, bi))
        e1 = g1_lin((1, e1), (beta, e1b), (alpha, e1p), (ai, e1m))
        e2 = g2_lin((1, e2), (bi, e2b), (alpha, e2p), (ai, e2m))
        s1 = [(alpha * l + r) % R for l, r in zip(s1[:h], s1[h:])]  # noqa: E741
        s2 = [(ai * l + r) % R for l, r in zip(s2[:h], s2[h:])]  # noqa: E741
        n = h
    gi, di = inv(gamma), inv(d)
    c = gt_mul(c, gt_pow(pair([h1], [h2]), s1[0] * s2[0]), gt_pow(pair([h1], [e2]), gamma), gt_pow(pair([e1], [h2]), gi))
    d1 = gt_mul(d1, gt_pow(pair([h1], [g2[0]]), gamma * s1[0]))
    d2 = gt_mul(d2, gt_pow(pair([g1[0]], [h2]), gi * s2[0]))
    w1, w2 = final
    lhs = pair([g1_lin((1, w1), (d, g1[0]))], [g2_lin((1, w2), (di, g2[0]))])
    return np.array_equal(lhs, gt_mul(pair([g1[0]], [g2[0]]), c, gt_pow(d2, d), gt_pow(d1, di)))


@pytest.mark.parametrize("nu,sigma", [(1, 1), (2, 2)])
def test_the_verifiers_equation_holds_in_the_groups(ctx, bases, setup, nu, sigma):
    """from the device's own message bytes; and fails after w1 is replaced by w1 + G"""
    inp = opening_inputs(ctx, bases, nu, sigma, 1200 + sigma)
    vmv, rounds, final, _ = run_opening(setup, inp)
    combined = ctx.dory_state_alloc(ffi.DORY_KIND_G1, 1 << nu)
    ctx.dory_state_combine_hints(inp["hints"], inp["scalars"], combined)
    commitment = dory_commit_tier2(setup, combined)
    args = (bases, commitment, inp["y"], inp["left"], inp["right"], vmv, rounds)
    assert verify_in_the_groups(*args, final, inp["challenges"], inp["gamma"], inp["d"])
    w1_plus_g = O.g1_add(final[0], O.g1_generator())
    assert not verify_in_the_groups(*args, (w1_plus_g, final[1]), inp["challenges"], inp["gamma"], inp["d"])
    for t in inp["hints"] + inp["tables"] + [combined]:
        t.free()


# ------------------------------------------------------------------------------------------- from a committed batch
def test_opening_of_a_committed_batch(ctx, bases, setup):
    """log_t = 6, log_k = 4, sigma = nu = 5: hints from jolt_dory_commit_onehot (transposed) and jolt_dory_commit_rows against an SRS of planted points, v from
    jolt_dory_fold_rows_grid, L and R eq tables of a random point; the model runs on the dense joint table from the definition"""
    from test_gpu_dory_opening import joint_dense_table, make_batch
    log_t, log_k, sigma, nu = 6, 4, 5, 5
    rows, n = 1 << nu, 1 << sigma
    batch = make_batch(log_t, log_k, n_dense=1, seed=1300)
    kg1, kg2, kh1, kh2 = bases["kg1"][:n], bases["kg2"][:n], bases["kh1"], bases["kh2"]
    srs = ctx.srs_upload(bases["gamma1"][:n])
    srcs = [ctx.onehot(i, batch["k"]) for i in batch["idx"]]
    host_hints = [ffi.dory_onehot_hint(ctx.dory_commit_onehot(srs, s, p, n)) for s, idx in zip(srcs, batch["idx"]) for p in range(idx.shape[0])]
    host_hints.append(np.array(ctx.dory_commit_rows(srs, ctx.ints(batch["dense_ints"][0]), n)))
    assert [h.shape[0] for h in host_hints] == [rows] * 5 + [(1 << log_t) >> sigma]
    hints = [ctx.dory_vec_upload(ffi.DORY_KIND_G1, h) for h in host_hints]
    scalars = np.concatenate([batch["gamma"], batch["dgamma"]])
    r_row, r_col = rand_fr(nu, 1301), rand_fr(sigma, 1302)
    left_host, right_host = O.eq_evals(r_row), O.eq_evals(r_col)
    left, right = ctx.upload(left_host), ctx.upload(right_host)
    dense = [ctx.upload(batch["dense"][0])]
    v_table = ctx.dory_fold_rows_grid(srcs, batch["gamma"], dense, batch["dgamma"], log_k, sigma, left)
    # the model, from the definition
    joint = joint_dense_table(batch)
    cells = O.from_mont(joint)
    matrix = [[int(x) for x in cells[r * n:(r + 1) * n]] for r in range(rows)]
    L, Rr = [int(x) for x in O.from_mont(left_host)], [int(x) for x in O.from_mont(right_host)]
    t_rows, commitment, v, y = OM.statement(kg1, kg2, matrix, L, Rr)
    assert np.array_equal(v_table.download(), fr_ints(v))
    assert np.array_equal(fr_int(y), O.poly_evaluate(joint, np.concatenate([r_row, r_col])))  # y = <v, R> is the joint polynomial at the point
    challenges, gamma, d = [tuple(rand_ints(2, 1310 + k)) for k in range(sigma)], rand_ints(1, 1303)[0], rand_ints(1, 1304)[0]
    proof = OM.prove(kg1, kg2, kh1, kh2, t_rows, v, L, Rr, challenges, gamma)
    inp = dict(nu=nu, sigma=sigma, hints=hints, scalars=scalars, tables=[v_table, left, right], challenges=challenges, gamma=gamma)
    vmv, rounds, final, _ = run_opening(setup, inp)
    check_message(vmv, proof["vmv"], "tta", "vmv")
    for r, ((first, second), (want_first, want_second)) in enumerate(zip(rounds, proof["rounds"])):
        check_message(first, want_first, "ttttab", ("first", r))
        check_message(second, want_second, "ttaabb", ("second", r))
    check_message(final, proof["final"], "ab", "final")
    assert OM.verify(kg1, kg2, kh1, kh2, commitment, y, L, Rr, proof, challenges, gamma, d)
    for t in hints + dense + [v_table, left, right]:
        t.free()
    for s in srcs:
        s.free()
