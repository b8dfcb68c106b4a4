"""GPU parity: Dory's reduce-and-fold rounds on resident vectors (dory_resident.hip, jolt_amd/dory_reduce.py) -- jolt_dory_vec, the in-place routines on views,
jolt_dory_products and whole reductions through DoryReduce.  Points are made through their discrete logarithms (tests/dory_groups.py, tests/pairing_model.py), so
every expected value is arithmetic modulo r plus one model power or one reference scalar multiplication; a vector whose logarithms form a progression is checked
element by element with one reference ADDITION each.  GT values are compared bit for bit, points as group elements.  Nothing on the checking side comes from the
new code."""
import ctypes as C

import numpy as np
import pytest

import dory_reduce_model as DM
import g2_model as M
import oracle_lib as O
import pairing_model as PM
from dory_groups import G1, G2, GROUPS, R, SHARED_SCALARS, fr_int, fr_ints, plant, progression, rand_ints
from jolt_amd import ffi
from jolt_amd.dory_reduce import DoryReduce
from util import rand_fr

pytestmark = pytest.mark.gpu
group_ids = lambda G: G.name  # noqa: E731
KIND = {"g1": ffi.DORY_KIND_G1, "g2": ffi.DORY_KIND_G2}
ONE = PM.gt_to_abi(PM.ONE)
SENTINEL = 0xA5A5A5A5A5A5A5A5


@pytest.fixture(scope="module")
def ctx():
    c = ffi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pool():
    """300 G1 points, 300 G2 points and 300 scalars with their logarithms, shared by the tests and never written.  Planted for the product batch (its views are
    listed in BATCH): the G1 identity at 1, the G2 identity at 67, a pair and its negation at G1 10 / 11 against G2 12 / 13, the scalars 0 at 4 and r - 1 at 6"""
    k0, dk, l0, dl = rand_ints(4, 700)
    ks, g1s = progression(G1, k0, dk, 300)
    ls, g2s = progression(G2, l0, dl, 300)
    plant(G1, ks, g1s, 1, 0)
    plant(G2, ls, g2s, 67, 0)
    plant(G1, ks, g1s, 11, -ks[10])
    plant(G2, ls, g2s, 13, ls[12])
    ss = rand_ints(300, 701)
    ss[4], ss[6] = 0, R - 1
    return ks, g1s, ls, g2s, ss, fr_ints(ss)


def same_element(G, a, b):
    if G is G1:
        return bool(O.g1_on_curve(a)) and bool(O.g1_eq(a, b))
    p = M.from_abi(a)
    return M.on_curve(p) and p == M.from_abi(b)


def assert_logs(G, got, want, k0, d):
    """got[i] = want[i] * generator.  want[i] is k0 + i d except at planted positions: the progression is walked with one reference addition per element, the
    planted positions get a reference multiplication each; the identity must come back as z = 0"""
    assert got.shape[0] == len(want)
    _, walk = progression(G, k0, d, len(want))
    for i, w in enumerate(want):
        if w % R == (k0 + i * d) % R and w % R:
            assert same_element(G, got[i], walk[i]), i
        else:
            assert G.same(got[i], w), i
        if w % R == 0:
            assert G.z_is_zero(got[i]), i


def _raw(name, *args):
    conv = [a.ctypes.data_as(C.c_void_p) if isinstance(a, np.ndarray) else a for a in args]
    return getattr(ffi.lib(), name)(*conv)


def test_round_trips_at_odd_sub_ranges(ctx, pool):
    ks, g1s, ls, g2s, ss, frs = pool
    for kind, host in ((ffi.DORY_KIND_G1, g1s[:70]), (ffi.DORY_KIND_G2, g2s[:70]), (ffi.DORY_KIND_FR, frs[:70])):
        v = ctx.dory_vec_upload(kind, host)
        assert len(v) == 70 and v.device_kind() == kind
        assert np.array_equal(v.download(), host)
        assert np.array_equal(v.download(3, 40), host[3:43]) and np.array_equal(v.download(69, 1), host[69:]) and v.download(70, 0).shape[0] == 0
        v.truncate(35)
        assert len(v) == 35 and np.array_equal(v.download(1), host[1:35])
        with pytest.raises(ffi.JoltError) as e:
            v.truncate(36)
        assert e.value.status == 1
        v.free()
    empty = ctx.dory_vec_upload(ffi.DORY_KIND_G2, np.zeros((0, 24), dtype=np.uint64))
    assert len(empty) == 0
    empty.free()


def test_refusals_write_nothing_and_leave_the_context_usable(ctx, pool):
    ks, g1s, ls, g2s, ss, frs = pool
    n = 64
    h, N = ctx.h, C.c_size_t(n)
    size_t = C.c_size_t
    # uploads: an off-curve G2 point, a G1 coordinate that is not canonical, a scalar that is not canonical -- no handle comes back
    off_curve = g2s[2:2 + n].copy()
    off_curve[n - 1, 1] ^= np.uint64(1)
    not_canonical = g1s[2:2 + n].copy()
    not_canonical[2, 0:4] = np.array(O.int_to_limbs(O.Q_MOD), dtype=np.uint64)
    bad_scalars = frs[:n].copy()
    bad_scalars[3] = np.array(O.int_to_limbs(R), dtype=np.uint64)
    for kind, bad in ((ffi.DORY_KIND_G2, off_curve), (ffi.DORY_KIND_G1, not_canonical), (ffi.DORY_KIND_FR, bad_scalars), (7, frs[:n]), (ffi.DORY_KIND_G1, None)):
        handle = C.c_void_p()
        assert _raw("jolt_dory_vec_upload", h, C.c_int32(kind), bad, N, C.byref(handle)) == 1 and not handle.value
    a, b, s = ctx.dory_vec_upload(ffi.DORY_KIND_G1, g1s[2:2 + n]), ctx.dory_vec_upload(ffi.DORY_KIND_G2, g2s[2:2 + n]), ctx.dory_vec_upload(ffi.DORY_KIND_FR, frs[:n])
    prepared = ctx.dory_g2_prepare_vec(b)
    a0, b0, s0 = a.download(), b.download(), s.download()
    big = size_t(2**64 - 1)
    two, five, zero, three = size_t(2), size_t(5), size_t(0), size_t(3)
    sc = fr_int(11)
    bad_sc = np.array(O.int_to_limbs(R), dtype=np.uint64)
    # views: another kind, first = 2^64 - 1 with n = 2 (first + n wraps to 1), ranges that overlap, a scalar that is not canonical
    assert _raw("jolt_dory_vec_scale_bases_add", h, b.h, zero, a.h, zero, five, sc) == 1
    assert _raw("jolt_dory_vec_scale_vs_add", h, a.h, zero, b.h, zero, five, sc) == 1
    assert _raw("jolt_dory_vec_scale_vs_add", h, s.h, zero, s.h, size_t(10), five, sc) == 1     # Fr vectors hold no points
    assert _raw("jolt_dory_vec_fold_field", h, a.h, zero, a.h, size_t(10), five, sc) == 1
    assert _raw("jolt_dory_vec_scale_bases_add", h, a.h, big, a.h, zero, two, sc) == 1
    assert _raw("jolt_dory_vec_scale_vs_add", h, a.h, zero, a.h, big, two, sc) == 1
    assert _raw("jolt_dory_vec_fold_field", h, s.h, big, s.h, zero, two, sc) == 1
    assert _raw("jolt_dory_vec_scale_vs_add", h, a.h, zero, a.h, three, five, sc) == 1           # [0, 5) and [3, 8)
    assert _raw("jolt_dory_vec_scale_bases_add", h, a.h, size_t(4), a.h, zero, five, sc) == 1     # [4, 9) and [0, 5)
    assert _raw("jolt_dory_vec_fold_field", h, s.h, size_t(7), s.h, size_t(7), size_t(1), sc) == 1
    assert _raw("jolt_dory_vec_scale_vs_add", h, a.h, zero, a.h, size_t(60), five, sc) == 1      # [60, 65) leaves the vector
    assert _raw("jolt_dory_vec_scale_vs_add", h, a.h, zero, a.h, size_t(10), five, bad_sc) == 1
    assert _raw("jolt_dory_vec_fold_field", h, s.h, zero, s.h, size_t(10), five, bad_sc) == 1
    host = np.full((2, 12), SENTINEL, dtype=np.uint64)
    assert _raw("jolt_dory_vec_download", h, a.h, big, two, host) == 1 and (host == SENTINEL).all()
    assert _raw("jolt_dory_vec_download", h, a.h, size_t(63), two, host) == 1 and (host == SENTINEL).all()
    handle = C.c_void_p()
    assert _raw("jolt_dory_g2_prepare_vec", h, a.h, zero, five, C.byref(handle)) == 1 and not handle.value  # a G1 vector
    assert _raw("jolt_dory_g2_prepare_vec", h, b.h, big, two, C.byref(handle)) == 1 and not handle.value
    # product items: kinds, a wrapping view, a prepared range past its table, both or neither G2 side, an unknown op; a good item beside the bad one changes nothing
    good = ffi.dory_item(ffi.DORY_PAIR, (a, 0, 5), (b, 0, 5))
    D = ffi.DoryItem
    bad_items = [D(ffi.DORY_PAIR, b.h, 0, b.h, 0, None, 0, 5), D(ffi.DORY_PAIR, a.h, 0, a.h, 0, None, 0, 5), D(ffi.DORY_MSM_G1, b.h, 0, s.h, 0, None, 0, 5),
                 D(ffi.DORY_MSM_G2, b.h, 0, a.h, 0, None, 0, 5), D(ffi.DORY_MSM_G1, a.h, 2**64 - 1, s.h, 0, None, 0, 2), D(ffi.DORY_PAIR, a.h, 0, b.h, 2**64 - 1, None, 0, 2),
                 D(ffi.DORY_PAIR, a.h, 0, None, 0, prepared.h, 60, 5), D(ffi.DORY_PAIR, a.h, 0, None, 0, prepared.h, 2**64 - 1, 2), D(ffi.DORY_PAIR, a.h, 0, b.h, 0, prepared.h, 0, 5),
                 D(ffi.DORY_PAIR, a.h, 0, None, 0, None, 0, 5), D(ffi.DORY_MSM_G1, a.h, 0, s.h, 0, prepared.h, 0, 5), D(3, a.h, 0, b.h, 0, None, 0, 5)]
    for k, bad in enumerate(bad_items):
        outs = np.full((2, 48), SENTINEL, dtype=np.uint64)
        assert _raw("jolt_dory_products", h, (D * 2)(good, bad), size_t(2), outs) == 1 and (outs == SENTINEL).all(), k
    assert _raw("jolt_dory_products", h, None, size_t(2), np.zeros((2, 48), dtype=np.uint64)) == 1
    # nothing was enqueued: the vectors hold their bytes; then valid calls on the same context
    assert np.array_equal(a.download(), a0) and np.array_equal(b.download(), b0) and np.array_equal(s.download(), s0)
    got = ctx.dory_products([good, ffi.dory_item(ffi.DORY_PAIR, (a, 1, 9), prepared, prepared_first=3)])
    assert np.array_equal(got[0], PM.gt_to_abi(PM.expected(ks[2:7], ls[2:7]))) and np.array_equal(got[1], PM.gt_to_abi(PM.expected(ks[3:12], ls[5:14])))
    ctx.dory_vec_scale_bases_add((a, 1, 3), (a, 5, 3), sc)
    assert_logs(G1, a.download(5, 3), [ks[7 + i] + 11 * ks[3 + i] for i in range(3)], 0, 0)
    for v in (a, b, s, prepared):
        v.free()


@pytest.fixture(scope="module")
def vectors():
    """per group: 70 bases and 135 vs with the progressions they are made of (k0, d), never written"""
    out = {}
    for G in GROUPS:
        b0, bd, v0, vd = rand_ints(4, 710 + G.width)
        out[G.name] = (b0, bd, progression(G, b0, bd, 70)[1], v0, vd, progression(G, v0, vd, 135)[1])
    return out


@pytest.mark.parametrize("s", SHARED_SCALARS, ids=["0", "1", "2", "r-1", "2^253-1"])
@pytest.mark.parametrize("G", GROUPS, ids=group_ids)
def test_in_place_routines(ctx, vectors, G, s):
    """both shared-scalar routines on views with odd firsts at n = 1, 64 and 65 (a second workgroup of one lane), with an identity on either side and a pair
    (P, -s P) whose result is the identity; the halves of ONE vector (v <- s v_L + v_R); and the host-pointer routines on the same arrays"""
    b0, bd, bases, v0, vd, vs = vectors[G.name]
    kb, kv = [(b0 + i * bd) % R for i in range(70)], [(v0 + i * vd) % R for i in range(135)]
    bases, vs = bases.copy(), vs.copy()
    plant(G, kb, bases, 4, 0)                 # an identity base
    plant(G, kv, vs, 8, 0)                    # an identity vs
    plant(G, kv, vs, 5, -s * kb[3])           # vs = -s * bases at element 2 of the views below: the identity
    dev_bases = ctx.dory_vec_upload(KIND[G.name], bases)
    fs = fr_int(s)
    bf, vf = 1, 3                              # odd firsts
    for n in (1, 64, 65):
        dev = ctx.dory_vec_upload(KIND[G.name], vs)
        ctx.dory_vec_scale_bases_add((dev_bases, bf, n), (dev, vf, n), fs)
        got = dev.download()
        assert np.array_equal(got[:vf], vs[:vf]) and np.array_equal(got[vf + n:], vs[vf + n:])  # nothing outside the view is written
        assert_logs(G, got[vf:vf + n], [kv[vf + i] + s * kb[bf + i] for i in range(n)], v0 + vf * vd + s * (b0 + bf * bd), vd + s * bd)
        if n == 65:
            ref = getattr(ctx, f"dory_{G.name}_scale_bases_add")(bases[bf:bf + n], vs[vf:vf + n], fs)
            assert all(same_element(G, got[vf + i], ref[i]) for i in range(n))
        dev.free()
        dev = ctx.dory_vec_upload(KIND[G.name], vs)
        ctx.dory_vec_scale_vs_add((dev, vf, n), (dev_bases, bf, n), fs)
        got = dev.download()
        assert np.array_equal(got[:vf], vs[:vf]) and np.array_equal(got[vf + n:], vs[vf + n:])
        assert_logs(G, got[vf:vf + n], [s * kv[vf + i] + kb[bf + i] for i in range(n)], s * (v0 + vf * vd) + b0 + bf * bd, s * vd + bd)
        if n == 65:
            ref = getattr(ctx, f"dory_{G.name}_scale_vs_add")(vs[vf:vf + n], bases[bf:bf + n], fs)
            assert all(same_element(G, got[vf + i], ref[i]) for i in range(n))
        dev.free()
    # the fold of one vector: halves of 67 elements at firsts 0 and 67; element 3 of the right half is -s * (element 3 of the left half)
    half = 67
    kh, vh = list(kv[:2 * half]), vs[:2 * half].copy()
    plant(G, kh, vh, 3, kv[3 + half])
    plant(G, kh, vh, 3 + half, -s * kh[3])
    dev = ctx.dory_vec_upload(KIND[G.name], vh)
    ctx.dory_vec_scale_vs_add((dev, 0, half), (dev, half, half), fs)
    got = dev.download()
    assert np.array_equal(got[half:], vh[half:])
    want = [s * kh[i] + kh[half + i] for i in range(half)]
    assert want[3] % R == 0
    assert_logs(G, got[:half], want, s * v0 + v0 + half * vd, (s + 1) * vd)
    dev.truncate(half)
    assert len(dev) == half
    dev.free()
    dev_bases.free()


@pytest.mark.parametrize("n", [1, 64, 65, 4097])
def test_field_fold_in_place(ctx, n):
    """bit for bit against the oracle, on two vectors at odd firsts and on the halves of one"""
    left, right, s = rand_fr(n + 3, 720), rand_fr(n + 1, 721), rand_fr(1, 722)[0]
    if n >= 3:
        left[3:6] = O.to_mont([0, 1, R - 1])
    dl, dr = ctx.dory_vec_upload(ffi.DORY_KIND_FR, left), ctx.dory_vec_upload(ffi.DORY_KIND_FR, right)
    ctx.dory_vec_fold_field((dl, 3, n), (dr, 1, n), s)
    got = dl.download()
    assert np.array_equal(got[:3], left[:3])
    assert np.array_equal(got[3:], O.fr_add(O.fr_mul(left[3:], np.tile(s, (n, 1))), right[1:]))
    assert np.array_equal(got[3:], ctx.dory_fold_field_vectors(left[3:], right[1:], s))
    both = np.concatenate([left[3:], right[1:]])
    dv = ctx.dory_vec_upload(ffi.DORY_KIND_FR, both)
    ctx.dory_vec_fold_field((dv, 0, n), (dv, n, n), s)
    assert np.array_equal(dv.download(), np.concatenate([got[3:], right[1:]]))
    for v in (dl, dr, dv):
        v.free()


# the views of the product batch: (op, first of a, first of b, n); b = "prepared" reads the table made from G2 points [9, 149) from point 5 on
BATCH = [(ffi.DORY_PAIR, 1, 3, 65),         # lane 0 the G1 identity, lane 64 (alone in its wavefront) the G2 identity, lanes 9 / 10 a pair and its negation
         (ffi.DORY_MSM_G1, 1, 3, 129),       # lane 0 the identity base, lane 1 the scalar 0, lane 3 the scalar r - 1
         (ffi.DORY_PAIR, 5, 3, 65),          # the G2 range of item 0 again
         (ffi.DORY_MSM_G2, 3, 1, 65),        # lane 64 the identity base
         (ffi.DORY_PAIR, 7, 11, 129),
         (ffi.DORY_PAIR, 9, 0, 0),
         (ffi.DORY_MSM_G1, 5, 5, 0),
         (ffi.DORY_MSM_G2, 7, 7, 0),
         (ffi.DORY_PAIR, 1, 67, 1),          # one pair with the G2 identity: one
         (ffi.DORY_PAIR, 21, 33, 2),
         (ffi.DORY_PAIR, 3, "prepared", 64),
         (ffi.DORY_PAIR, 101, 55, 63),
         (ffi.DORY_MSM_G1, 11, 9, 63),
         (ffi.DORY_MSM_G1, 1, 1, 1),         # the identity base alone: the identity
         (ffi.DORY_MSM_G2, 67, 4, 1),        # the identity base times zero
         (ffi.DORY_MSM_G2, 21, 5, 2),        # the second scalar is r - 1
         (ffi.DORY_MSM_G2, 101, 3, 64),
         (ffi.DORY_MSM_G1, 151, 100, 64)]


def test_product_batch(ctx, pool):
    """one call with all three kinds, item lengths 0, 1, 2, 63, 64, 65 and 129 at odd firsts: segments whose ends are not wavefront-aligned, odd tree levels
    (65 -> 33 -> 17 -> 9 -> 5 -> 3 -> 2 -> 1) beside shorter segments that have finished, a G2 range two items share, a range of a prepared table"""
    ks, g1s, ls, g2s, ss, frs = pool
    a, b, s = ctx.dory_vec_upload(ffi.DORY_KIND_G1, g1s), ctx.dory_vec_upload(ffi.DORY_KIND_G2, g2s), ctx.dory_vec_upload(ffi.DORY_KIND_FR, frs)
    prepared = ctx.dory_g2_prepare_vec((b, 9, 140))
    items = []
    for op, fa, fb, n in BATCH:
        if op == ffi.DORY_PAIR:
            items.append(ffi.dory_item(op, (a, fa, n), prepared, prepared_first=5) if fb == "prepared" else ffi.dory_item(op, (a, fa, n), (b, fb, n)))
        else:
            items.append(ffi.dory_item(op, (a if op == ffi.DORY_MSM_G1 else b, fa, n), (s, fb, n)))
    got = ctx.dory_products(items)
    again = ctx.dory_products(items)
    assert all(np.array_equal(x, y) for x, y in zip(got, again))  # the same call twice: the same bytes
    for k, (op, fa, fb, n) in enumerate(BATCH):
        if op == ffi.DORY_PAIR:
            fb = 14 if fb == "prepared" else fb
            assert got[k].shape == (48,)
            assert np.array_equal(got[k], PM.gt_to_abi(PM.expected(ks[fa:fa + n], ls[fb:fb + n]))), k
            assert np.array_equal(got[k], ctx.dory_multi_pair(g1s[fa:fa + n], g2s[fb:fb + n])), k  # bit-identical to the host-pointer entry on the same arrays
        else:
            G, logs = (G1, ks) if op == ffi.DORY_MSM_G1 else (G2, ls)
            want = sum(x * y for x, y in zip(logs[fa:fa + n], ss[fb:fb + n]))
            assert got[k].shape == (G.width,) and G.same(got[k], want), k
            if want % R == 0:
                assert G.z_is_zero(got[k]), k
    assert np.array_equal(got[5], ONE) and np.array_equal(got[8], ONE)
    assert G1.z_is_zero(got[6]) and G2.z_is_zero(got[7]) and G1.z_is_zero(got[13]) and G2.z_is_zero(got[14])
    assert np.array_equal(ctx.dory_products([ffi.dory_item(ffi.DORY_PAIR, (a, 10, 2), (b, 12, 2))])[0], ONE)  # the pair and its negation alone
    assert ctx.dory_products([]) == []
    for v in (a, b, s, prepared):
        v.free()


def gt_of(log):
    return PM.gt_to_abi(PM.expected([log], [1]))


@pytest.mark.parametrize("n", [8, 128])
def test_whole_reduction(ctx, n):
    """n = 8: three rounds; n = 128: seven rounds, from two workgroups down to one lane.  Challenges from a seeded generator; every message of every round against
    the log-space model, the first, middle and last element of every vector after every round, the single elements at the end, and the five invariants"""
    seeds = rand_ints(8, 730 + n)
    k1, v1 = progression(G1, seeds[0], seeds[1], n)
    k2, v2 = progression(G2, seeds[2], seeds[3], n)
    kg1, gamma1 = progression(G1, seeds[4], seeds[5], n)
    kg2, gamma2 = progression(G2, seeds[6], seeds[7], n)
    s1, s2 = rand_ints(n, 740 + n), rand_ints(n, 750 + n)
    model = DM.State(k1, k2, s1, s2, kg1, kg2)
    red = DoryReduce(ctx, v1, v2, fr_ints(s1), fr_ints(s2), gamma1, gamma2)
    challenges = rand_ints(2 * n.bit_length(), 760 + n)
    kinds_first, kinds_second = "ttttab", "ttaabb"   # t: GT, a: G1, b: G2

    def check_message(got, want, kinds, what):
        for j, (g, w, kind) in enumerate(zip(got, want, kinds)):
            if kind == "t":
                assert np.array_equal(g, gt_of(w)), (what, j)
            else:
                assert (G1 if kind == "a" else G2).same(g, w), (what, j)

    rounds = 0
    while red.n > 1:
        beta, alpha = challenges[2 * rounds], challenges[2 * rounds + 1]
        beta_inv, alpha_inv = pow(beta, -1, R), pow(alpha, -1, R)
        before, setup = model.claims(), model.setup()
        first, want_first = red.first_message(), model.first_message()
        check_message(first, want_first, kinds_first, ("first", rounds))
        red.apply_beta(fr_int(beta), fr_int(beta_inv))
        model.apply_beta(beta, beta_inv)
        second, want_second = red.second_message(), model.second_message()
        check_message(second, want_second, kinds_second, ("second", rounds))
        red.apply_alpha(fr_int(alpha), fr_int(alpha_inv))
        model.apply_alpha(alpha, alpha_inv)
        rounds += 1
        assert red.n == model.n == n >> rounds and all(len(v) == red.n for v in (red.v1, red.v2, red.s1, red.s2))
        for i in sorted({0, red.n // 2, red.n - 1}):
            assert G1.same(red.v1.download(i, 1)[0], model.v1[i]) and G2.same(red.v2.download(i, 1)[0], model.v2[i]), (rounds, i)
            assert np.array_equal(red.s1.download(i, 1)[0], fr_int(model.s1[i])) and np.array_equal(red.s2.download(i, 1)[0], fr_int(model.s2[i])), (rounds, i)
        # the five invariants, in log space, over messages that were just checked to be the device's
        assert model.claims() == DM.invariants(before, setup, want_first, want_second, beta, alpha), rounds
    assert rounds == n.bit_length() - 1 and red.n == 1
    assert G1.same(red.v1.download()[0], model.v1[0]) and G2.same(red.v2.download()[0], model.v2[0])
    with pytest.raises(ValueError):
        red.first_message()
    red.close()


def test_challenge_and_inverse_must_multiply_to_one(ctx):
    """refused before anything is enqueued: the vectors keep their bytes"""
    n = 4
    _, v1 = progression(G1, 3, 5, n)
    _, v2 = progression(G2, 7, 11, n)
    red = DoryReduce(ctx, v1, v2, fr_ints([1, 2, 3, 4]), fr_ints([5, 6, 7, 8]), v1, v2)
    with pytest.raises(ValueError):
        red.apply_beta(fr_int(5), fr_int(5))
    with pytest.raises(ValueError):
        red.apply_alpha(fr_int(5), fr_int(pow(5, -1, R) + 1))
    assert red.n == n and np.array_equal(red.v1.download(), v1) and np.array_equal(red.v2.download(), v2)
    red.apply_alpha(fr_int(5), fr_int(pow(5, -1, R)))
    assert red.n == 2 and G1.same(red.v1.download()[1], 5 * (3 + 5) + 3 + 15)
    red.close()
