"""GPU parity: the group and field routines of dory::prove's reduce-and-fold rounds (dory_routines.hip), DoryRoutines<ArkG1> and DoryRoutines<ArkG2> of
crates/jolt-dory/src/routines.rs, against the CPU oracle (G1, Fr) and the big-integer model of tests/g2_model.py (G2).  Points are made and checked through their
discrete logarithms (tests/dory_groups.py), so every expected value is arithmetic modulo r and one reference multiplication; points are compared as group
elements, field results bit for bit.  Nothing on the checking side comes from the library."""
import ctypes as C

import numpy as np
import pytest

import g2_model as M
import oracle_lib as O
from dory_groups import G1, G2, GROUPS, R, SHARED_SCALARS, fr_int, fr_ints, plant, progression, rand_ints
from jolt_amd import ffi
from util import rand_fr

pytestmark = pytest.mark.gpu
group_ids = lambda G: G.name  # noqa: E731


@pytest.fixture(scope="module")
def ctx():
    c = ffi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def vectors():
    """per group: 257 bases and 257 vs with their discrete logarithms, shared by the tests and never written"""
    out = {}
    for G in GROUPS:
        kb, kv, d1, d2 = rand_ints(4, 100 + G.width)
        out[G.name] = progression(G, kb, d1, 257) + progression(G, kv, d2, 257)
    return out


def checked_indices(n, seed=7):
    """every element up to n = 65; beyond that the ends of the first wavefronts, the last two and eight seeded ones (the reference multiplication limits the count)"""
    if n <= 65:
        return list(range(n))
    rng = np.random.default_rng(seed)
    return sorted({0, 63, 64, 255, 256} | {int(i) for i in rng.integers(0, n, size=8)})


def call(ctx, G, routine, *args):
    return getattr(ctx, f"dory_{G.name}_{routine}")(*args)


def assert_points(G, got, want_ks, idx=None):
    assert got.shape[0] == len(want_ks)
    for i in (range(len(want_ks)) if idx is None else idx):
        assert G.same(got[i], want_ks[i]), i
        if want_ks[i] % R == 0:
            assert G.z_is_zero(got[i]), i


@pytest.mark.parametrize("G", GROUPS, ids=group_ids)
def test_reference_shapes(ctx, G):
    """the shapes of the reference's own tests (routines.rs:168-247): n = 33 for G1 and 17 for G2, bases[5] the identity, scalars[9] = 0, vs[3] the identity; all five"""
    n = 33 if G is G1 else 17
    kb, bases = progression(G, *rand_ints(2, 1), n)
    kv, vs = progression(G, *rand_ints(2, 2), n)
    plant(G, kb, bases, 5, 0)
    plant(G, kv, vs, 3, 0)
    ks = rand_ints(n, 3)
    ks[9] = 0
    s = rand_ints(1, 4)[0]
    scalars = fr_ints(ks)
    assert G.same(call(ctx, G, "msm", bases, scalars), sum(a * b for a, b in zip(ks, kb)))
    assert_points(G, call(ctx, G, "fixed_base_mul", bases[0], scalars), [k * kb[0] for k in ks])
    assert_points(G, call(ctx, G, "fixed_base_mul", G.point(0), scalars), [0] * n)
    vs1 = call(ctx, G, "scale_bases_add", bases, vs, fr_int(s))
    kv1 = [v + s * b for v, b in zip(kv, kb)]
    assert_points(G, vs1, kv1)
    vs2 = call(ctx, G, "scale_vs_add", vs1, bases, fr_int(s))  # the reference goes on from the first result, with the bases as addends
    assert_points(G, vs2, [s * v + b for v, b in zip(kv1, kb)])
    left, right = rand_fr(n, 5), rand_fr(n, 6)
    assert np.array_equal(ctx.dory_fold_field_vectors(left, right, fr_int(s)), O.fr_add(O.fr_mul(left, np.tile(fr_int(s), (n, 1))), right))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
@pytest.mark.parametrize("G", GROUPS, ids=group_ids)
def test_vector_routines_at_every_size(ctx, vectors, G, n):
    """a ragged last wavefront (63, 65), a full one (64), a second, third ... workgroup (65, 257), one element and none"""
    kb, bases, kv, vs = vectors[G.name]
    kb, bases, kv, vs = kb[:n], bases[:n], kv[:n], vs[:n]
    s = rand_ints(1, 20 + n)[0]
    idx = checked_indices(n)
    assert_points(G, call(ctx, G, "scale_bases_add", bases, vs, fr_int(s)), [v + s * b for v, b in zip(kv, kb)], idx)
    assert_points(G, call(ctx, G, "scale_vs_add", vs, bases, fr_int(s)), [s * v + b for v, b in zip(kv, kb)], idx)
    ks = rand_ints(n, 30 + n)
    assert_points(G, call(ctx, G, "fixed_base_mul", bases[0] if n else G.point(3), fr_ints(ks)), [k * (kb[0] if n else 3) for k in ks], idx)


@pytest.mark.parametrize("s", SHARED_SCALARS, ids=["0", "1", "2", "r-1", "2^253-1"])
@pytest.mark.parametrize("G", GROUPS, ids=group_ids)
def test_shared_scalars_and_planted_elements(ctx, G, s):
    """the final addition's special cases and identity inputs, for both vector routines: the result the identity (asserted as z = 0), the last addition a doubling,
    an identity base beside an ordinary vs, an identity vs, both"""
    n = 9
    kb, bases = progression(G, *rand_ints(2, 40), n)
    kv, vs = progression(G, *rand_ints(2, 41), n)
    plant(G, kv, vs, 1, -s * kb[1])      # vs = -s * bases: the identity
    plant(G, kv, vs, 2, s * kb[2])       # vs = s * bases: the last addition doubles
    plant(G, kb, bases, 3, 0)            # an identity base beside an ordinary vs
    plant(G, kv, vs, 4, 0)               # an identity vs
    plant(G, kb, bases, 5, 0)
    plant(G, kv, vs, 5, 0)               # both
    want = [v + s * b for v, b in zip(kv, kb)]
    assert want[1] % R == 0
    assert_points(G, call(ctx, G, "scale_bases_add", bases, vs, fr_int(s)), want)
    ka, addends = list(kb), bases.copy()
    plant(G, ka, addends, 6, -s * kv[6])  # addends = -s * vs: the identity
    plant(G, ka, addends, 7, s * kv[7])   # addends = s * vs: the last addition doubles
    want = [s * v + a for v, a in zip(kv, ka)]
    assert want[6] % R == 0
    assert_points(G, call(ctx, G, "scale_vs_add", vs, addends, fr_int(s)), want)


@pytest.mark.parametrize("n", [0, 1, 17, 33, 300])
@pytest.mark.parametrize("G", GROUPS, ids=group_ids)
def test_msm_matches_the_naive_sum(ctx, G, n):
    """sum_i scalars[i] * bases[i] with repeated bases, a base beside its negative under equal scalars, an identity base and a zero scalar; then all scalars zero"""
    kb, bases = progression(G, *rand_ints(2, 50 + n), n)
    ks = rand_ints(n, 60 + n)
    if n >= 17:
        plant(G, kb, bases, 4, kb[2])        # a repeated base (another representative of it)
        plant(G, kb, bases, 8, -kb[7])       # a base and its negative ...
        ks[8] = ks[7]                        # ... with equal scalars
        plant(G, kb, bases, 11, 0)
        ks[13] = 0
    got = call(ctx, G, "msm", bases, fr_ints(ks))
    want = sum(a * b for a, b in zip(ks, kb))
    assert G.same(got, want)
    if n == 0:
        assert G.z_is_zero(got)
    zero = call(ctx, G, "msm", bases, fr_ints([0] * n))
    assert G.same(zero, 0) and G.z_is_zero(zero)


@pytest.mark.parametrize("n", [0, 1, 65, 4096])
def test_field_fold_bit_for_bit(ctx, n):
    left, right, s = rand_fr(n, 70), rand_fr(n, 71), rand_fr(1, 72)[0]
    if n >= 65:
        left[:3] = O.to_mont([0, 1, R - 1])
        right[1:4] = O.to_mont([R - 1, 0, 1])
    want = O.fr_add(O.fr_mul(left, np.tile(s, (n, 1))), right) if n else left
    got = ctx.dory_fold_field_vectors(left, right, s)
    assert got.shape == (n, 4) and np.array_equal(got, want)


def _raw(name, *args):
    conv = [a.ctypes.data_as(C.c_void_p) if isinstance(a, np.ndarray) else a for a in args]
    return getattr(ffi.lib(), name)(*conv)


@pytest.mark.parametrize("G", GROUPS, ids=group_ids)
def test_refusals_write_nothing_and_leave_the_context_usable(ctx, vectors, G):
    """JOLT_ERR_INVALID_ARG (1) for a null pointer with n > 0, a scalar that is not canonical, a point off its curve, a coordinate that is not canonical; the
    output keeps its bytes, and the next valid call on the same context is right"""
    n = 5
    kb, bases, kv, vs = (v[:n] for v in vectors[G.name])
    bases, vs = bases.copy(), vs.copy()
    s, ks = fr_int(11), fr_ints([1, 2, 3, 4, 5])
    bad_scalar = np.array(O.int_to_limbs(R), dtype=np.uint64)
    bad_scalars = ks.copy()
    bad_scalars[3] = bad_scalar
    off_curve = bases.copy()
    off_curve[4, 1] ^= np.uint64(1)
    not_canonical = bases.copy()
    not_canonical[2, 0:4] = np.array(O.int_to_limbs(O.Q_MOD), dtype=np.uint64)
    sentinel = np.full((n, G.width), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    h, N = ctx.h, C.c_size_t(n)
    pre = f"jolt_dory_{G.name}_"
    before = vs.copy()
    for bad_bases in (off_curve, not_canonical, None):
        assert _raw(pre + "scale_bases_add", h, bad_bases, vs, N, s) == 1
        assert _raw(pre + "scale_vs_add", h, vs, bad_bases, N, s) == 1
        out = sentinel.copy()
        assert _raw(pre + "msm", h, bad_bases, ks, N, out) == 1 and np.array_equal(out, sentinel)
    assert _raw(pre + "scale_bases_add", h, bases, vs, N, bad_scalar) == 1
    assert _raw(pre + "scale_vs_add", h, vs, bases, N, bad_scalar) == 1
    assert _raw(pre + "scale_bases_add", h, bases, off_curve, N, s) == 1  # a bad vs: refused before anything is written back
    assert np.array_equal(vs, before)
    for args in ((off_curve[4], ks), (not_canonical[2], ks), (bases[0], bad_scalars), (bases[0], None)):
        out = sentinel.copy()
        assert _raw(pre + "fixed_base_mul", h, args[0], args[1], N, out) == 1 and np.array_equal(out, sentinel)
    out = sentinel.copy()
    assert _raw(pre + "msm", h, bases, bad_scalars, N, out) == 1 and np.array_equal(out, sentinel)
    left = rand_fr(n, 80)
    keep = left.copy()
    assert _raw("jolt_dory_fold_field_vectors", h, left, ks, N, bad_scalar) == 1 and _raw("jolt_dory_fold_field_vectors", h, left, None, N, s) == 1
    assert np.array_equal(left, keep)
    # the same context, valid calls
    assert_points(G, call(ctx, G, "scale_bases_add", bases, vs, s), [v + 11 * b for v, b in zip(kv, kb)])
    assert G.same(call(ctx, G, "msm", bases, ks), sum((i + 1) * b for i, b in enumerate(kb)))


def test_round_algebra_g2(ctx):
    """one n = 2^10 G2 run: scale_bases_add by s, then scale_vs_add by 1/s with the addends -B.  Each step against the model on the index subset, and every element
    against the identity the two satisfy together, (1/s) (v + s B) + (-B) = (1/s) v -- a wrong scalar or operand order fails it even where single calls agree"""
    n = 1 << 10
    kb, bases = progression(G2, *rand_ints(2, 90), n)
    kv, vs = progression(G2, *rand_ints(2, 91), n)
    _, neg_b = progression(G2, -kb[0], kb[0] - kb[1], n)  # -B, in representatives of its own
    s = rand_ints(1, 92)[0]
    s_inv = pow(s, -1, R)
    idx = checked_indices(n, seed=93)
    step1 = ctx.dory_g2_scale_bases_add(bases, vs, fr_int(s))
    assert_points(G2, step1, [v + s * b for v, b in zip(kv, kb)], idx)
    step2 = ctx.dory_g2_scale_vs_add(step1, neg_b, fr_int(s_inv))
    assert_points(G2, step2, [s_inv * v for v in kv], idx)
    # s_inv * kv[i] = s_inv * kv[0] + i * (s_inv * d): the expected vector is itself a progression, so EVERY element is checked with one model addition each
    p, step = M.mul_generator(s_inv * kv[0]), M.mul_generator(s_inv * (kv[1] - kv[0]))
    for i in range(n):
        assert M.from_abi(step2[i]) == p, i
        p = M.add(p, step)


@pytest.mark.parametrize("G", GROUPS, ids=group_ids)
def test_long_vectors_are_checked_to_their_last_element(ctx, G):
    """n = 2^12: the argument checks of long vectors are shared among host threads -- a bad point in the last stretch is still refused, in either vector, and the
    valid vectors give the right elements"""
    n = 1 << 12
    kb, bases = progression(G, *rand_ints(2, 95), n)
    kv, vs = progression(G, *rand_ints(2, 96), n)
    s = rand_ints(1, 97)[0]
    h, N, pre = ctx.h, C.c_size_t(n), f"jolt_dory_{G.name}_"
    for where in (n - 1, n - 1500, 1030, 0):
        bad = bases.copy()
        bad[where, 1] ^= np.uint64(1)
        keep = vs.copy()
        assert _raw(pre + "scale_bases_add", h, bad, keep, N, fr_int(s)) == 1 and _raw(pre + "scale_vs_add", h, bad, keep, N, fr_int(s)) == 1, where
        assert np.array_equal(keep, vs)
    assert_points(G, call(ctx, G, "scale_bases_add", bases, vs, fr_int(s)), [v + s * b for v, b in zip(kv, kb)], checked_indices(n, seed=98))
