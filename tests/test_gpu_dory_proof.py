"""GPU parity: Dory evaluation proofs as one library call (dory_scheme.hip) -- a round's in-place update as one call against the existing separate calls, the setup
object, whole openings under a callback and under the library's engines against the Python-driven DoryOpening and the log-space model of tests/dory_open_model.py,
the aborts, and one table from commit to proof.  GT elements, Fr and the updated vectors are compared bit for bit, points as group elements; no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import dory_open_model as OM
import oracle_lib as O
from dory_groups import G1, G2, R, fr_int, fr_ints, plant, progression, rand_ints
from jolt_amd import dory_proof, dory_scheme, ffi
from jolt_amd.dory_open import DorySetup
from test_dory_proof_cpu import g2_bytes, gt_bytes
from test_gpu_dory_open import check_message, gt_of, opening_inputs, run_opening, verify_in_the_groups
from util import rand_challenge, rand_fr

pytestmark = pytest.mark.gpu
N_SETUP = 128  # 2^sigma of the largest opening below: two wavefronts per vector
KIND = {G1: ffi.DORY_KIND_G1, G2: ffi.DORY_KIND_G2}
PHASES = (ffi.DORY_PHASE_VMV, ffi.DORY_PHASE_FIRST, ffi.DORY_PHASE_SECOND, ffi.DORY_PHASE_GAMMA, ffi.DORY_PHASE_FINAL)


@pytest.fixture(scope="module")
def ctx():
    c = ffi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def bases():
    """Gamma1, Gamma2 of 128 points and H1, H2 with their logarithms; never written"""
    a0, ad, b0, bd, kh1, kh2 = rand_ints(6, 2100)
    kg1, gamma1 = progression(G1, a0, ad, N_SETUP)
    kg2, gamma2 = progression(G2, b0, bd, N_SETUP)
    return dict(kg1=kg1, gamma1=gamma1, kg2=kg2, gamma2=gamma2, kh1=kh1, h1=G1.point(kh1), kh2=kh2, h2=G2.point(kh2, rep=3))


@pytest.fixture(scope="module")
def py_setup(ctx, bases):
    s = DorySetup(ctx, bases["gamma1"], bases["gamma2"], bases["h1"], bases["h2"])
    yield s
    s.close()


@pytest.fixture(scope="module")
def lib_setup(ctx, bases):
    s = dory_proof.DoryProofSetup(ctx, bases["gamma1"], bases["gamma2"], bases["h1"], bases["h2"])
    yield s
    s.close()


def _raw(name, *args):
    conv = [a.ctypes.data_as(C.c_void_p) if isinstance(a, np.ndarray) else a for a in args]
    return getattr(ffi.lib(), name)(*conv)


def inv(x):
    return pow(x, -1, R)


def mont_int(c):
    return int(O.from_mont(np.asarray(c, dtype=np.uint64).reshape(1, 4))[0])


# the scalars of the issue: 1, r - 1, a 125-bit challenge, a full-width value
UPDATE_SCALARS = {"one": 1, "r-1": R - 1, "challenge": mont_int(rand_challenge(2101)), "full": rand_ints(1, 2102)[0]}


# ------------------------------------------------------------------------------------------------------ a round's update as one call
@pytest.fixture(scope="module")
def update_pool():
    """host vectors with their logarithms, longer than every view below: v1 / v2 and bases in both groups, two Fr vectors"""
    m = 140
    seeds = rand_ints(8, 2110)
    out = {}
    for G, j in ((G1, 0), (G2, 4)):
        out[G] = (progression(G, seeds[j], seeds[j + 1], m), progression(G, seeds[j + 2], seeds[j + 3], m))
    out["fr"] = (rand_fr(m, 2111), rand_fr(m, 2112))
    return out


def planted(G, pool, first, n, s, fold):
    """copies of the pool's (vector, base) in group G with the exceptional cases inside the view [first, first + n): the identity on either side, an element equal to
    what is added to it (a doubling) and to its negation (the identity comes out), for the unit scalars and for s itself.  fold: the partner of element i is element
    i + n / 2 of the same vector and IT is scaled (v[i] <- s v[i] + v[i + h]); otherwise the base is scaled (v[i] += s base[i])."""
    (kv, v), (kb, b) = pool[G]
    kv, v, kb, b = list(kv), v.copy(), list(kb), b.copy()
    h = n // 2
    slots = list(range(h if fold else n))

    def at(j):
        return first + slots[j % len(slots)]

    if fold:
        cases = [(0, None), (None, 0), ("same", None), ("neg", None), ("s", None), ("-s", None)]
        for j, (left, right) in enumerate(cases[:max(len(slots), 1)] if len(slots) < len(cases) else cases):
            i = at(j * 7 + 1) if len(slots) >= 40 else at(j)
            if right == 0:
                plant(G, kv, v, i + h, 0)
            elif left == 0:
                plant(G, kv, v, i, 0)
            elif left == "same":
                plant(G, kv, v, i + h, kv[i])
            elif left == "neg":
                plant(G, kv, v, i + h, -kv[i])
            elif left == "s":
                plant(G, kv, v, i + h, s * kv[i])
            else:
                plant(G, kv, v, i + h, -s * kv[i])
    else:
        cases = ["v0", "b0", "same", "neg", "s", "-s"]
        for j, what in enumerate(cases[:len(slots)] if len(slots) < len(cases) else cases):
            i = at(j * 7 + 1) if len(slots) >= 40 else at(j)
            if what == "v0":
                plant(G, kv, v, i, 0)
            elif what == "b0":
                plant(G, kb, b, i, 0)
            elif what == "same":
                plant(G, kv, v, i, kb[i])
            elif what == "neg":
                plant(G, kv, v, i, -kb[i])
            elif what == "s":
                plant(G, kv, v, i, s * kb[i])
            else:
                plant(G, kv, v, i, -s * kb[i])
    return kv, v, kb, b


@pytest.mark.parametrize("name", list(UPDATE_SCALARS))
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_beta_update_is_the_two_separate_calls(ctx, update_pool, n, name):
    beta = UPDATE_SCALARS[name]
    b, bi = fr_int(beta), fr_int(inv(beta))
    f1, f2, fa, fb = 3, 5, 2, 7  # every view at its own non-zero first inside a vector of 140
    k1, v1, ka, g1 = planted(G1, update_pool, f1, n, beta, fold=False)
    k2, v2, kb, g2 = planted(G2, update_pool, f2, n, inv(beta), fold=False)
    # the bases are read at their own firsts: shift them so that base element fa + i is the one planted against v element f1 + i
    g1s, g2s = np.roll(g1, fa - f1, axis=0), np.roll(g2, fb - f2, axis=0)
    up = ctx.dory_vec_upload
    new = [up(ffi.DORY_KIND_G1, v1), up(ffi.DORY_KIND_G2, v2)]
    old = [up(ffi.DORY_KIND_G1, v1), up(ffi.DORY_KIND_G2, v2)]
    gam = [up(ffi.DORY_KIND_G1, g1s), up(ffi.DORY_KIND_G2, g2s)]
    ctx.dory_round_update(ffi.DORY_UPDATE_BETA, (new[0], f1, n), (new[1], f2, n), (gam[0], fa, n), (gam[1], fb, n), b, bi)
    ctx.dory_vec_scale_bases_add((gam[0], fa, n), (old[0], f1, n), b)
    ctx.dory_vec_scale_bases_add((gam[1], fb, n), (old[1], f2, n), bi)
    got1, got2 = new[0].download(), new[1].download()
    assert np.array_equal(got1, old[0].download()) and np.array_equal(got2, old[1].download())
    # the margins hold their bytes, the bases too
    assert np.array_equal(got1[:f1], v1[:f1]) and np.array_equal(got1[f1 + n:], v1[f1 + n:])
    assert np.array_equal(got2[:f2], v2[:f2]) and np.array_equal(got2[f2 + n:], v2[f2 + n:])
    assert np.array_equal(gam[0].download(), g1s) and np.array_equal(gam[1].download(), g2s)
    # and a few elements by their logarithms, the planted ones among them
    for i in sorted({0, min(1, n - 1), min(2, n - 1), min(3, n - 1), n - 1}):
        assert G1.same(got1[f1 + i], k1[f1 + i] + beta * ka[f1 + i]), i
        assert G2.same(got2[f2 + i], k2[f2 + i] + inv(beta) * kb[f2 + i]), i
    for v in new + old + gam:
        v.free()


@pytest.mark.parametrize("name", list(UPDATE_SCALARS))
@pytest.mark.parametrize("n", [2, 64, 128, 130])
def test_alpha_update_is_the_four_separate_calls_and_the_truncation(ctx, update_pool, n, name):
    alpha = UPDATE_SCALARS[name]
    a, ai = fr_int(alpha), fr_int(inv(alpha))
    h = n // 2
    f1, f2, fs1, fs2 = 3, 5, 1, 6
    k1, v1, _, _ = planted(G1, update_pool, f1, n, alpha, fold=True)
    k2, v2, _, _ = planted(G2, update_pool, f2, n, inv(alpha), fold=True)
    s1, s2 = update_pool["fr"]
    up = ctx.dory_vec_upload
    make = lambda: [up(ffi.DORY_KIND_G1, v1), up(ffi.DORY_KIND_G2, v2), up(ffi.DORY_KIND_FR, s1), up(ffi.DORY_KIND_FR, s2)]  # noqa: E731
    new, old = make(), make()
    firsts = (f1, f2, fs1, fs2)
    ctx.dory_round_update(ffi.DORY_UPDATE_ALPHA, *[(v, f, n) for v, f in zip(new, firsts)], a, ai)
    ctx.dory_vec_scale_vs_add((old[0], f1, h), (old[0], f1 + h, h), a)
    ctx.dory_vec_scale_vs_add((old[1], f2, h), (old[1], f2 + h, h), ai)
    ctx.dory_vec_fold_field((old[2], fs1, h), (old[2], fs1 + h, h), a)
    ctx.dory_vec_fold_field((old[3], fs2, h), (old[3], fs2 + h, h), ai)
    for v, f, host in zip(new, firsts, (v1, v2, s1, s2)):
        assert len(v) == f + h  # truncated to the folded half
    for v, w, f, host in zip(new, old, firsts, (v1, v2, s1, s2)):
        got = v.download()
        assert np.array_equal(got, w.download(0, f + h)) and np.array_equal(got[:f], host[:f])
    got1, got2 = new[0].download(), new[1].download()
    for i in sorted({0, min(1, h - 1), min(2, h - 1), min(3, h - 1), h - 1}):
        assert G1.same(got1[f1 + i], alpha * k1[f1 + i] + k1[f1 + h + i]), i
        assert G2.same(got2[f2 + i], inv(alpha) * k2[f2 + i] + k2[f2 + h + i]), i
    want_s1 = O.fr_add(O.fr_mul(s1[fs1:fs1 + h], np.repeat(a.reshape(1, 4), h, axis=0)), s1[fs1 + h:fs1 + n])
    assert np.array_equal(new[2].download(fs1, h), want_s1)
    for v in new + old:
        v.free()


def test_update_refusals_write_nothing_and_leave_the_context_usable(ctx, update_pool):
    n, size_t = 8, C.c_size_t
    (_, v1h), (_, g1h) = update_pool[G1]
    (_, v2h), (_, g2h) = update_pool[G2]
    s1h, s2h = update_pool["fr"]
    up = ctx.dory_vec_upload
    v1, g1, v2, g2 = up(ffi.DORY_KIND_G1, v1h[:16]), up(ffi.DORY_KIND_G1, g1h[:16]), up(ffi.DORY_KIND_G2, v2h[:16]), up(ffi.DORY_KIND_G2, g2h[:16])
    s1, s2 = up(ffi.DORY_KIND_FR, s1h[:16]), up(ffi.DORY_KIND_FR, s2h[:16])
    other = ffi.Context(0)
    foreign = other.dory_vec_upload(ffi.DORY_KIND_G1, v1h[:16])
    vecs = (v1, g1, v2, g2, s1, s2)
    before = [v.download() for v in vecs]
    x = 12345
    sc, sci, not_inv = fr_int(x), fr_int(inv(x)), fr_int(x + 1)
    not_canonical = np.array(O.int_to_limbs(R), dtype=np.uint64)
    BETA, ALPHA = C.c_int32(ffi.DORY_UPDATE_BETA), C.c_int32(ffi.DORY_UPDATE_ALPHA)

    def call(mode, a, af, b, bf, c, cf, d, df, count, s=sc, si=sci):
        return _raw("jolt_dory_round_update", ctx.h, mode, a, size_t(af), b, size_t(bf), c, size_t(cf), d, size_t(df), size_t(count), s, si)

    assert call(BETA, None, 0, v2.h, 0, g1.h, 0, g2.h, 0, n) == 1                 # a null handle
    assert call(BETA, v1.h, 0, v2.h, 0, g1.h, 0, None, 0, n) == 1
    assert _raw("jolt_dory_round_update", None, BETA, v1.h, size_t(0), v2.h, size_t(0), g1.h, size_t(0), g2.h, size_t(0), size_t(n), sc, sci) == 1
    assert call(BETA, v1.h, 0, v2.h, 0, g1.h, 0, g2.h, 0, n, s=None) == 1
    assert call(BETA, v2.h, 0, v1.h, 0, g1.h, 0, g2.h, 0, n) == 1                 # the wrong kinds
    assert call(BETA, v1.h, 0, v2.h, 0, s1.h, 0, s2.h, 0, n) == 1                 # beta mode over Fr vectors
    assert call(ALPHA, v1.h, 0, v2.h, 0, g1.h, 0, g2.h, 0, n) == 1                # alpha mode over bases
    assert call(C.c_int32(2), v1.h, 0, v2.h, 0, g1.h, 0, g2.h, 0, n) == 1         # an unknown mode
    assert call(BETA, foreign.h, 0, v2.h, 0, g1.h, 0, g2.h, 0, n) == 1            # a vector of another context
    assert call(BETA, v1.h, 9, v2.h, 0, g1.h, 0, g2.h, 0, n) == 1                 # [9, 17) leaves the vector
    assert call(BETA, v1.h, 0, v2.h, 0, g1.h, 0, g2.h, 2**64 - 1, n) == 1         # a first that wraps
    assert call(ALPHA, v1.h, 0, v2.h, 0, s1.h, 0, s2.h, 10, n) == 1
    assert call(BETA, v1.h, 0, v2.h, 0, v1.h, 4, g2.h, 0, n) == 1                 # v1 against itself, overlapping
    assert call(ALPHA, v1.h, 0, v2.h, 0, s1.h, 0, s2.h, 0, 7) == 1                # an odd n in alpha mode
    assert call(ALPHA, v1.h, 0, v2.h, 0, s1.h, 0, s1.h, 8, n) == 1                # s1 and s2 one vector
    assert call(BETA, v1.h, 0, v2.h, 0, g1.h, 0, g2.h, 0, n, s=not_canonical) == 1
    assert call(ALPHA, v1.h, 0, v2.h, 0, s1.h, 0, s2.h, 0, n, si=not_canonical) == 1
    assert call(BETA, v1.h, 0, v2.h, 0, g1.h, 0, g2.h, 0, n, si=not_inv) == 1     # scalar * scalar_inv != 1
    assert call(ALPHA, v1.h, 0, v2.h, 0, s1.h, 0, s2.h, 0, n, si=sc) == 1
    # nothing was enqueued or truncated; then valid calls on the same context
    assert all(len(v) == 16 for v in vecs)
    assert all(np.array_equal(v.download(), b) for v, b in zip(vecs, before))
    assert call(BETA, v1.h, 1, v2.h, 2, g1.h, 3, g2.h, 4, n) == 0
    assert call(ALPHA, v1.h, 1, v2.h, 2, s1.h, 3, s2.h, 4, n) == 0
    assert [len(v) for v in (v1, v2, s1, s2)] == [5, 6, 7, 8]
    assert call(BETA, v1.h, 0, v2.h, 0, g1.h, 0, g2.h, 0, 0) == 0                 # nothing to do
    foreign.free()
    other.close()
    for v in vecs:
        v.free()


# ------------------------------------------------------------------------------------------------------ the setup object
def test_setup_tier2_is_the_multi_pairing_against_the_prepared_bases(ctx, bases, lib_setup):
    assert lib_setup.n == N_SETUP
    k0, kd = rand_ints(2, 2120)
    _, rows = progression(G1, k0, kd, 70)
    rows[3] = G1.point(0)
    vec = ctx.dory_vec_upload(ffi.DORY_KIND_G1, rows)
    views = [(vec, 0, 70), (vec, 5, 9), (vec, 11, 0), (vec, 6, 64), (vec, 69, 1)]  # a short hint, an empty one, whole wavefronts, one row
    got = lib_setup.tier2(views)
    prepared = ctx.dory_g2_prepare(bases["gamma2"])
    for g, (_, first, n) in zip(got, views):
        assert np.array_equal(g, ctx.dory_multi_pair_g2_setup(rows[first:first + n], prepared, n)), (first, n)
    assert np.array_equal(got[2], gt_of(0))
    assert lib_setup.tier2([]) == []
    # a view longer than the setup, a G2 vector, a foreign setup handle
    long_vec = ctx.dory_state_alloc(ffi.DORY_KIND_G1, N_SETUP + 1)
    g2v = ctx.dory_state_alloc(ffi.DORY_KIND_G2, 4)
    for bad in ([(long_vec, 0, N_SETUP + 1)], [(vec, 0, 4), (g2v, 0, 4)], [(vec, 68, 3)]):
        with pytest.raises(ffi.JoltError) as e:
            lib_setup.tier2(bad)
        assert e.value.status == 1
    assert np.array_equal(lib_setup.tier2([(vec, 5, 9)])[0], got[1])
    prepared.free()
    for v in (vec, long_vec, g2v):
        v.free()


def test_setup_create_refusals(ctx, bases):
    g1, g2, h1, h2 = bases["gamma1"], bases["gamma2"], bases["h1"], bases["h2"]
    handle = C.c_void_p()

    def create(a, b, n, c=h1, d=h2, out=C.byref(handle)):
        return _raw("jolt_dory_setup_create", ctx.h, a, b, C.c_size_t(n), c, d, out)

    off1, off2 = g1[:4].copy(), g2[:4].copy()
    off1[2, 4] ^= np.uint64(1)
    off2[1, 1] ^= np.uint64(1)
    bad_h2 = h2.copy()
    bad_h2[9] ^= np.uint64(1)
    assert create(g1, g2, 0) == 1 and create(g1, g2, 3) == 1 and create(g1, g2, 96) == 1  # not a power of two
    assert create(None, g2, 4) == 1 and create(g1, None, 4) == 1 and create(g1, g2, 4, c=None) == 1 and create(g1, g2, 4, out=None) == 1
    assert create(off1, g2, 4) == 1 and create(g1, off2, 4) == 1 and create(g1, g2, 4, d=bad_h2) == 1  # a point off its curve
    assert not handle.value
    with pytest.raises(ValueError):
        dory_proof.DoryProofSetup(ctx, g1[:8], g2[:4], h1, h2)  # the lengths differ
    size = C.c_size_t()
    assert _raw("jolt_dory_setup_size", None, C.byref(size)) == 1
    s = dory_proof.DoryProofSetup(ctx, g1[:4], g2[:4], h1, h2)
    assert s.n == 4
    s.close()
    assert _raw("jolt_dory_setup_free", ctx.h, None) == 0


# ------------------------------------------------------------------------------------------------------ whole openings under a callback
class Recorder:
    """a caller's transcript that hands back fixed challenges and keeps what it was shown"""

    def __init__(self, challenges, gamma, abort=None, zero_at=None):
        self.challenges, self.gamma, self.abort, self.zero_at = challenges, gamma, abort, zero_at
        self.seen = []

    def __call__(self, phase, rnd, gts, g1s, g2s):
        self.seen.append((phase, rnd, gts, g1s, g2s))
        if self.abort == (phase, rnd):
            return 7
        if self.zero_at == (phase, rnd):
            return np.zeros(4, dtype=np.uint64)
        if phase == ffi.DORY_PHASE_FIRST:
            return fr_int(self.challenges[rnd][0])
        if phase == ffi.DORY_PHASE_SECOND:
            return fr_int(self.challenges[rnd][1])
        if phase == ffi.DORY_PHASE_GAMMA:
            return fr_int(self.gamma)
        return None


def prove_with(lib_setup, inp, **how):
    v_table, left, right = inp["tables"]
    return dory_proof.prove(lib_setup, inp["hints"], inp["scalars"], v_table, left, right, inp["nu"], inp["sigma"], **how)


def check_against_the_model(proof, want):
    check_message(proof.vmv, want["vmv"], "tta", "vmv")
    assert len(proof.rounds) == len(want["rounds"])
    for r, ((first, second), (want_first, want_second)) in enumerate(zip(proof.rounds, want["rounds"])):
        check_message(first, want_first, "ttttab", ("first", r))
        check_message(second, want_second, "ttaabb", ("second", r))
    check_message(proof.final, want["final"], "ab", "final")


def model_proof(bases, inp, challenges, gamma):
    n = 1 << inp["sigma"]
    return OM.prove(bases["kg1"][:n], bases["kg2"][:n], bases["kh1"], bases["kh2"], inp["t_rows"], inp["v"], inp["left"], inp["right"], challenges, gamma)


def free_inputs(inp):
    for t in inp["hints"] + inp["tables"]:
        t.free()


@pytest.mark.parametrize("nu,sigma", [(1, 1), (2, 3), (5, 6), (6, 7)])
def test_callback_opening_against_the_python_driver_and_the_model(ctx, bases, py_setup, lib_setup, nu, sigma):
    inp = opening_inputs(ctx, bases, nu, sigma, 2200 + 10 * nu + sigma)  # three hints, one of them short
    rec = Recorder(inp["challenges"], inp["gamma"])
    proof = prove_with(lib_setup, inp, callback=rec)
    # ---- the Python-driven DoryOpening under the same challenges: GT bit for bit, points as group elements
    vmv, rounds, final, _ = run_opening(py_setup, inp)
    theirs = list(vmv) + [x for f, s in rounds for x in f + s] + list(final)
    mine = proof.elements()
    assert len(mine) == len(theirs) == sum(ffi.host_dory_proof_counts(sigma)[:3])
    for j, (a, b) in enumerate(zip(mine, theirs)):
        if a.size == 48:
            assert np.array_equal(a, b), j
        elif a.size == 12:
            assert O.g1_on_curve(a) and O.g1_eq(a, b), j
        else:
            assert a.size == b.size == 24 and ffi.host_g2_serialize_compressed(a) == ffi.host_g2_serialize_compressed(b) == g2_bytes(b), j
    # ---- the model
    check_against_the_model(proof, model_proof(bases, inp, inp["challenges"], inp["gamma"]))
    # ---- the challenges that came back, and what the callback saw: exactly the elements of each phase, in order
    assert all(np.array_equal(c[0], fr_int(b)) and np.array_equal(c[1], fr_int(a)) for c, (b, a) in zip(proof.challenges, inp["challenges"]))
    assert np.array_equal(proof.gamma, fr_int(inp["gamma"]))
    want_calls = [(ffi.DORY_PHASE_VMV, 0, (2, 1, 0))]
    for k in range(sigma):
        want_calls += [(ffi.DORY_PHASE_FIRST, k, (4, 1, 1)), (ffi.DORY_PHASE_SECOND, k, (2, 2, 2))]
    want_calls += [(ffi.DORY_PHASE_GAMMA, sigma, (0, 0, 0)), (ffi.DORY_PHASE_FINAL, sigma, (0, 1, 1))]
    assert [(p, r, (a.shape[0], b.shape[0], c.shape[0])) for p, r, a, b, c in rec.seen] == want_calls
    shown = [x for _, _, a, b, c in rec.seen for x in list(a) + list(b) + list(c)]
    assert len(shown) == len(mine) and all(np.array_equal(x, y) for x, y in zip(shown, mine))
    # ---- the inputs stay the caller's: a second proof from them is the same bytes
    again = prove_with(lib_setup, inp, callback=Recorder(inp["challenges"], inp["gamma"]))
    assert np.array_equal(again.gts, proof.gts) and np.array_equal(again.g1s, proof.g1s) and np.array_equal(again.g2s, proof.g2s)
    free_inputs(inp)


# ------------------------------------------------------------------------------------------------------ under the library's engines
def element_bytes(e):
    e = np.asarray(e)
    return gt_bytes(e) if e.size == 48 else O.g1_serialize_compressed(e) if e.size == 12 else g2_bytes(e)


def replay(label, proof, alter=None):
    """a second transcript absorbing the proof's messages in phase order with this file's byte forms: (challenges, final state).  alter = (index into
    proof.elements(), replacement element)"""
    t = ffi.HostTranscript(label)
    elements = proof.elements()
    if alter is not None:
        elements[alter[0]] = alter[1]

    def absorb(chunk):
        for e in chunk:
            data = element_bytes(e)
            t.append_label(b"dory_group", count=len(data))
            t.append_bytes(data)

    drawn = []
    absorb(elements[:3])
    at = 3
    for _ in range(proof.sigma):
        absorb(elements[at:at + 6])
        drawn.append(t.challenge(full_width=True))
        absorb(elements[at + 6:at + 12])
        drawn.append(t.challenge(full_width=True))
        at += 12
    drawn.append(t.challenge(full_width=True))
    absorb(elements[at:at + 2])
    state = t.state()
    t.close()
    return drawn, state


ENGINE_CASES = [(2, 3, ffi.TRANSCRIPT_TEST), (2, 3, ffi.TRANSCRIPT_BLAKE2B), (2, 3, ffi.TRANSCRIPT_KECCAK), (2, 3, ffi.TRANSCRIPT_BLAKE2B_SPONGE),
                (5, 6, ffi.TRANSCRIPT_BLAKE2B), (1, 1, ffi.TRANSCRIPT_BLAKE2B)]


@pytest.mark.parametrize("nu,sigma,engine", ENGINE_CASES, ids=["2-3-test", "2-3-blake2b_legacy", "2-3-keccak", "2-3-blake2b_sponge", "5-6-blake2b_legacy", "1-1-blake2b_legacy"])
def test_opening_under_a_library_transcript(ctx, bases, lib_setup, nu, sigma, engine):
    inp = opening_inputs(ctx, bases, nu, sigma, 2300 + 10 * nu + sigma)
    label = engine | 4242
    t = ffi.HostTranscript(label)
    proof = prove_with(lib_setup, inp, transcript=t)
    state = t.state()
    t.close()
    # ---- the replay reproduces every challenge and the final state
    drawn, replay_state = replay(label, proof)
    flat = [c for pair in proof.challenges for c in pair] + [proof.gamma]
    assert len(drawn) == len(flat) == 2 * sigma + 1 and all(np.array_equal(a, b) for a, b in zip(drawn, flat))
    assert replay_state == state
    # ---- with those challenges the model's proof is this one, and the log-space verifier accepts it (and refuses another evaluation)
    challenges = [(mont_int(b), mont_int(a)) for b, a in proof.challenges]
    gamma, d = mont_int(proof.gamma), inp["d"]
    assert all(b and a for b, a in challenges) and gamma
    want = model_proof(bases, inp, challenges, gamma)
    check_against_the_model(proof, want)
    n = 1 << sigma
    args = (bases["kg1"][:n], bases["kg2"][:n], bases["kh1"], bases["kh2"], inp["commitment"])
    assert OM.verify(*args, inp["y"], inp["left"], inp["right"], want, challenges, gamma, d)
    assert not OM.verify(*args, inp["y"] + 1, inp["left"], inp["right"], want, challenges, gamma, d)
    # ---- the verifier's equation in the groups, from the library's own bytes
    if (nu, sigma) in ((1, 1), (2, 3)) and engine == ffi.TRANSCRIPT_BLAKE2B:
        combined = ctx.dory_state_alloc(ffi.DORY_KIND_G1, 1 << nu)
        ctx.dory_state_combine_hints(inp["hints"], inp["scalars"], combined)
        commitment = lib_setup.tier2([combined])[0]
        assert np.array_equal(commitment, gt_of(inp["commitment"]))
        group_bases = {k: (v[:n] if k in ("gamma1", "gamma2") else v) for k, v in bases.items()}
        assert verify_in_the_groups(group_bases, commitment, inp["y"], inp["left"], inp["right"], proof.vmv, proof.rounds, proof.final, challenges, gamma, d)
        w1_plus_g = O.g1_add(proof.final[0], O.g1_generator())
        assert not verify_in_the_groups(group_bases, commitment, inp["y"], inp["left"], inp["right"], proof.vmv, proof.rounds, (w1_plus_g, proof.final[1]), challenges, gamma, d)
        combined.free()
    free_inputs(inp)


def test_every_element_is_absorbed(ctx, bases, lib_setup):
    """one element of each phase and kind replaced in the replay: the next challenge (after the final message: the state) changes"""
    nu, sigma = 2, 3
    inp = opening_inputs(ctx, bases, nu, sigma, 2400)
    label = ffi.TRANSCRIPT_BLAKE2B | 99
    t = ffi.HostTranscript(label)
    proof = prove_with(lib_setup, inp, transcript=t)
    t.close()
    drawn, state = replay(label, proof)
    other = {48: gt_of(12345), 12: G1.point(12345), 24: G2.point(12345)}
    # index into proof.elements() -> the challenge that follows the element's message.  Round 1 starts at 3 + 12: first = 15..20 (4 GT, G1, G2), second = 21..26
    cases = {0: 0, 2: 0,                      # VMV: a GT element and the G1 point -> beta_0
             16: 2, 19: 2, 20: 2,             # FIRST of round 1: GT, G1, G2 -> beta_1
             22: 3, 24: 3, 26: 3,             # SECOND of round 1: GT, G1, G2 -> alpha_1
             3 + 12 * sigma: None, 4 + 12 * sigma: None}  # FINAL: w1, w2 -> the state
    kinds = set()
    for index, which in cases.items():
        size = proof.elements()[index].size
        kinds.add((index, size))
        changed, changed_state = replay(label, proof, alter=(index, other[size]))
        if which is None:
            assert changed_state != state and all(np.array_equal(a, b) for a, b in zip(changed, drawn)), index
        else:
            assert not np.array_equal(changed[which], drawn[which]), index
            assert all(np.array_equal(a, b) for a, b in zip(changed[:which], drawn[:which])), index
    assert sorted(s for _, s in kinds) == [12, 12, 12, 12, 24, 24, 24, 48, 48, 48]
    free_inputs(inp)


# ------------------------------------------------------------------------------------------------------ aborts and refusals
def test_aborts_come_back_and_leave_the_context_usable(ctx, bases, lib_setup):
    nu, sigma = 2, 3
    inp = opening_inputs(ctx, bases, nu, sigma, 2500)
    honest = prove_with(lib_setup, inp, callback=Recorder(inp["challenges"], inp["gamma"]))
    hint_bytes = [h.download() for h in inp["hints"]]
    rec = Recorder(inp["challenges"], inp["gamma"], abort=(ffi.DORY_PHASE_FIRST, 1))
    with pytest.raises(ffi.JoltError) as e:
        prove_with(lib_setup, inp, callback=rec)
    assert e.value.status == 7 and rec.seen[-1][:2] == (ffi.DORY_PHASE_FIRST, 1) and len(rec.seen) == 4  # the caller's status, and nothing after it
    after_abort = prove_with(lib_setup, inp, callback=Recorder(inp["challenges"], inp["gamma"]))
    rec = Recorder(inp["challenges"], inp["gamma"], zero_at=(ffi.DORY_PHASE_FIRST, 0))
    with pytest.raises(ffi.JoltError) as e:
        prove_with(lib_setup, inp, callback=rec)
    assert e.value.status == 11 and len(rec.seen) == 2  # JOLT_ERR_NOT_INVERTIBLE
    after_zero = prove_with(lib_setup, inp, callback=Recorder(inp["challenges"], inp["gamma"]))
    for p in (after_abort, after_zero):
        assert np.array_equal(p.gts, honest.gts) and np.array_equal(p.g1s, honest.g1s) and np.array_equal(p.g2s, honest.g2s)
    # a challenge that is not canonical is the caller's bug
    with pytest.raises(ffi.JoltError) as e:
        prove_with(lib_setup, inp, callback=lambda phase, *_: np.array(O.int_to_limbs(R), dtype=np.uint64) if phase == ffi.DORY_PHASE_FIRST else None)
    assert e.value.status == 1
    # an exception in the callback does not unwind through the library
    def raising(phase, *_):
        raise KeyError("transcript")
    with pytest.raises(KeyError):
        prove_with(lib_setup, inp, callback=raising)
    assert all(np.array_equal(h.download(), b) for h, b in zip(inp["hints"], hint_bytes))
    free_inputs(inp)


def test_wrong_shapes_are_refused_before_anything_is_enqueued(ctx, bases, lib_setup):
    inp = opening_inputs(ctx, bases, 1, 2, 2600)
    v_table, left, right = inp["tables"]
    hints, scalars = inp["hints"], inp["scalars"]
    calls = []
    cb = lambda *a: calls.append(a)  # noqa: E731
    prove = lambda *a: dory_proof.prove(lib_setup, *a, callback=cb)  # noqa: E731
    hint_bytes = [h.download() for h in hints]
    big = ctx.upload(rand_fr(256, 2601))
    g2v = ctx.dory_state_alloc(ffi.DORY_KIND_G2, 2)
    bad_scalars = scalars.copy()
    bad_scalars[1] = np.array(O.int_to_limbs(R), dtype=np.uint64)
    for args, status in [((hints, scalars, v_table, right, left, 2, 1), 1),           # nu > sigma
                         ((hints, scalars, v_table, right, right, 1, 2), 1),          # left of 2^sigma entries
                         ((hints, scalars, left, left, right, 1, 2), 1),              # v of 2^nu entries
                         ((hints, scalars, big, left, big, 1, 8), 9),                 # more columns than the setup has bases: JOLT_ERR_SRS_TOO_SMALL
                         (([(hints[0], 0, 2)], scalars[:1], v_table, left, right, 0, 2), 1),  # a hint of more than 2^nu rows
                         (([(hints[0], 1, 2)], scalars[:1], v_table, left, right, 1, 2), 1),  # a view that leaves its vector
                         (([g2v], scalars[:1], v_table, left, right, 1, 2), 1),       # not a G1 vector
                         (([], scalars[:0], v_table, left, right, 1, 2), 1),          # no hints
                         ((hints, bad_scalars, v_table, left, right, 1, 2), 1)]:      # a scalar that is not canonical
        with pytest.raises(ffi.JoltError) as e:
            prove(*args)
        assert e.value.status == status, args[5:]
    with pytest.raises(ValueError):
        prove(hints, scalars[:2], v_table, left, right, 1, 2)                         # a scalar short
    with pytest.raises(ValueError):
        dory_proof.prove(lib_setup, hints, scalars, v_table, left, right, 1, 2)       # neither a transcript nor a callback
    assert calls == []
    assert all(np.array_equal(h.download(), b) for h, b in zip(hints, hint_bytes))
    proof = dory_proof.prove(lib_setup, hints, scalars, v_table, left, right, 1, 2, callback=Recorder(inp["challenges"], inp["gamma"]))
    check_against_the_model(proof, model_proof(bases, inp, inp["challenges"], inp["gamma"]))
    for t in (big, g2v):
        t.free()
    free_inputs(inp)


# ------------------------------------------------------------------------------------------------------ one table, from commit to proof
@pytest.mark.parametrize("n", [4, 5])
def test_commit_then_prove_one_table(ctx, bases, py_setup, lib_setup, n):
    nu, sigma = dory_scheme.matrix_shape(1 << n)
    rows, cols = 1 << nu, 1 << sigma
    kg1, kg2, kh1, kh2 = bases["kg1"][:cols], bases["kg2"][:cols], bases["kh1"], bases["kh2"]
    srs = ctx.srs_upload(bases["gamma1"][:cols])
    evals = rand_fr(1 << n, 2700 + n)
    ints = [int(x) for x in O.from_mont(evals)]
    matrix = [ints[r * cols:(r + 1) * cols] for r in range(rows)]
    table = ctx.upload(evals)
    commitment, hint = dory_scheme.commit(py_setup, srs, table)
    assert np.array_equal(lib_setup.tier2([hint])[0], commitment)
    point = rand_fr(n, 2710 + n)
    label = ffi.TRANSCRIPT_BLAKE2B | (2720 + n)
    t = ffi.HostTranscript(label)
    proof, y = dory_scheme.prove(lib_setup, table, hint, point, t)
    t.close()
    L, Rr = [int(x) for x in O.from_mont(O.eq_evals(point[:nu]))], [int(x) for x in O.from_mont(O.eq_evals(point[nu:]))]
    t_rows, combined, v, want_y = OM.statement(kg1, kg2, matrix, L, Rr)
    assert np.array_equal(np.asarray(y).reshape(-1), fr_int(want_y)) and np.array_equal(fr_int(want_y), np.asarray(O.poly_evaluate(evals, point)).reshape(-1))
    assert np.array_equal(commitment, gt_of(combined))
    drawn, _ = replay(label, proof)
    assert all(np.array_equal(a, b) for a, b in zip(drawn, [c for pair in proof.challenges for c in pair] + [proof.gamma]))
    challenges, gamma = [(mont_int(b), mont_int(a)) for b, a in proof.challenges], mont_int(proof.gamma)
    want = OM.prove(kg1, kg2, kh1, kh2, t_rows, v, L, Rr, challenges, gamma)
    check_against_the_model(proof, want)
    d = rand_ints(1, 2730 + n)[0]
    assert OM.verify(kg1, kg2, kh1, kh2, combined, want_y, L, Rr, want, challenges, gamma, d)
    assert not OM.verify(kg1, kg2, kh1, kh2, combined, (want_y + 1) % R, L, Rr, want, challenges, gamma, d)
    spare = ffi.HostTranscript(1)
    with pytest.raises(ValueError):
        dory_scheme.prove(lib_setup, table, hint, point[:-1], spare)  # a point of the wrong length
    spare.close()
    for x in (hint, table, srs):
        x.free()
