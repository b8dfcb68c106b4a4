"""GPU parity: Dory verification on the device (dory_verify.hip) -- GT powers and multi-exponentiations bit for bit against the library's host functions
(jolt_host_gt_pow, jolt_host_fq12_op MUL, which tests/pairing_model.py pins), the verifier's precomputed values against host pairings of the same slices, whole
verifications of the library's own proofs (accepted, with the prover's transcript state; the same decision as the verifier written out in the groups in
tests/test_gpu_dory_open.py), one rejection per tampered element with the check that fails, and the stage-8 batch through DeviceWorkload in both placements.
GT and Fr are compared bit for bit; no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from dory_groups import G1, G2, R, fr_int, fr_ints, progression, rand_ints
from jolt_amd import dory_proof, ffi
from jolt_amd.workload import DeviceWorkload
from test_gpu_dory_open import gt_mul, gt_pow, opening_inputs, pair, verify_in_the_groups

pytestmark = pytest.mark.gpu
N_SETUP = 16
SENTINEL = np.uint64(0xA5A5A5A5A5A5A5A5)
SIZES = [0, 1, 2, 63, 64, 65, 130]
INVALID_ARG, UNSUPPORTED = ffi.ERR_INVALID_ARG, ffi.ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def ctx():
    c = ffi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def bases():
    """Gamma1, Gamma2 of 16 points and H1, H2 with their logarithms; never written"""
    a0, ad, b0, bd, kh1, kh2 = rand_ints(6, 12000)
    kg1, gamma1 = progression(G1, a0, ad, N_SETUP)
    kg2, gamma2 = progression(G2, b0, bd, N_SETUP)
    return dict(kg1=kg1, gamma1=gamma1, kg2=kg2, gamma2=gamma2, kh1=kh1, h1=G1.point(kh1), kh2=kh2, h2=G2.point(kh2, rep=3))


def make_setup(ctx, bases, n):
    return dory_proof.DoryProofSetup(ctx, bases["gamma1"][:n], bases["gamma2"][:n], bases["h1"], bases["h2"])


@pytest.fixture(scope="module")
def setup16(ctx, bases):
    s = make_setup(ctx, bases, 16)
    yield s
    s.close()


@pytest.fixture(scope="module")
def setup8(ctx, bases):
    s = make_setup(ctx, bases, 8)
    yield s
    s.close()


def _raw(name, *args):
    conv = [a.ctypes.data_as(C.c_void_p) if isinstance(a, np.ndarray) else a for a in args]
    return getattr(ffi.lib(), name)(*conv)


# ------------------------------------------------------------------------------------------------------ GT powers
def random_fq12(rng):
    """twelve uniform canonical words: an element of Fq12 that lies in no particular subgroup (a cyclotomic squaring would give another value for it)"""
    return np.array([w for _ in range(12) for w in O.int_to_limbs(int.from_bytes(rng.bytes(40), "little") % O.Q_MOD)], dtype=np.uint64)


@pytest.fixture(scope="module")
def powers(bases):
    """130 bases -- one, pairing values, random Fq12 elements -- with scalars 0, 1, 2, r - 1, 2^253 and random ones, and the host's powers of them, computed once"""
    rng = np.random.default_rng(12100)
    x = random_fq12(rng)
    one = ffi.host_fq12_op(ffi.FQ12_MUL, x, ffi.host_fq12_op(ffi.FQ12_INV, x))
    pairings = [pair([bases["gamma1"][i]], [bases["gamma2"][i + 1]]) for i in range(3)]
    n = max(SIZES)
    gts = np.stack([one, pairings[0], pairings[1]] + [random_fq12(rng) if i % 3 else pairings[i % 2 + 1] for i in range(n - 3)])
    special = [0, 1, 2, R - 1, 1 << 253]
    ks = (special + special + rand_ints(n, 12101))[:n]  # the special scalars meet a pairing value, one, and random elements
    ks[0] = 5  # one^5; ks[5] = 0 meets a random element
    scalars = fr_ints(ks)
    host = np.stack([ffi.host_gt_pow(g, s) for g, s in zip(gts, scalars)])
    return gts, scalars, host, one


def test_fixture_elements_are_what_they_claim(powers):
    gts, scalars, host, one = powers
    assert np.array_equal(ffi.host_fq12_op(ffi.FQ12_MUL, one, gts[5]), gts[5])  # `one` is the one
    assert np.array_equal(host[0], one) and np.array_equal(host[5], one) and not np.array_equal(gts[5], one)
    # a random element is outside the cyclotomic subgroup: its inverse is not its conjugate
    assert not np.array_equal(ffi.host_fq12_op(ffi.FQ12_INV, gts[4]), ffi.host_fq12_op(ffi.FQ12_CONJ, gts[4]))
    assert np.array_equal(ffi.host_fq12_op(ffi.FQ12_INV, gts[1]), ffi.host_fq12_op(ffi.FQ12_CONJ, gts[1]))  # a pairing value is inside it


@pytest.mark.parametrize("n", SIZES)
def test_powers_and_their_product_are_the_hosts_bit_for_bit(ctx, powers, n):
    gts, scalars, host, one = powers
    got = ctx.dory_gt_pow_many(gts[:n], scalars[:n])
    assert got.shape == (n, 48) and np.array_equal(got, host[:n])
    want = one
    for x in host[:n]:
        want = ffi.host_fq12_op(ffi.FQ12_MUL, want, x)
    prod = ctx.dory_gt_multi_exp(gts[:n], scalars[:n])
    assert np.array_equal(prod, want)
    # a second call gives the same bytes
    assert np.array_equal(ctx.dory_gt_pow_many(gts[:n], scalars[:n]), got) and np.array_equal(ctx.dory_gt_multi_exp(gts[:n], scalars[:n]), prod)


def test_power_refusals_leave_out_untouched(ctx, powers):
    gts, scalars, host, _ = powers
    n = 3
    g, s = gts[:n].copy(), scalars[:n].copy()
    bad_g, bad_s = g.copy(), s.copy()
    bad_g[1, 44:48] = np.array(O.int_to_limbs(O.Q_MOD), dtype=np.uint64)  # the last Fq coordinate = q: not canonical
    bad_s[2] = np.array(O.int_to_limbs(R), dtype=np.uint64)
    outs, out = np.full((n, 48), SENTINEL), np.full(48, SENTINEL)
    h, size_t = ctx.h, C.c_size_t
    for name, dst in (("jolt_dory_gt_pow_many", outs), ("jolt_dory_gt_multi_exp", out)):
        assert _raw(name, h, None, s, size_t(n), dst) == INVALID_ARG
        assert _raw(name, h, g, None, size_t(n), dst) == INVALID_ARG
        assert _raw(name, h, bad_g, s, size_t(n), dst) == INVALID_ARG
        assert _raw(name, h, g, bad_s, size_t(n), dst) == INVALID_ARG
        assert _raw(name, h, g, s, size_t((1 << 20) + 1), dst) == UNSUPPORTED  # refused on the count alone: nothing is read
        assert _raw(name, None, g, s, size_t(n), dst) == INVALID_ARG
    assert _raw("jolt_dory_gt_pow_many", h, g, s, size_t(n), None) == INVALID_ARG
    assert _raw("jolt_dory_gt_multi_exp", h, g, s, size_t(n), None) == INVALID_ARG
    assert (outs == SENTINEL).all() and (out == SENTINEL).all()
    # the context stays usable
    assert np.array_equal(ctx.dory_gt_pow_many(g, s), host[:n])


# ------------------------------------------------------------------------------------------------------ the verifier's setup
def test_verifier_setup_values_are_host_pairings_of_the_same_slices(bases, setup8):
    n, s = 8, 3
    g1, g2, h1, h2 = bases["gamma1"][:n], bases["gamma2"][:n], bases["h1"], bases["h2"]
    got = setup8.verifier().values()
    assert got.shape == (3 * s + 4, 48)
    want = [pair(g1[:n >> k], g2[:n >> k]) for k in range(s + 1)]
    want += [pair(g1[(n >> k) // 2:n >> k], g2[:(n >> k) // 2]) for k in range(s)]
    want += [pair(g1[:(n >> k) // 2], g2[(n >> k) // 2:n >> k]) for k in range(s)]
    want += [pair([h1], [h2]), pair([h1], [g2[0]]), pair([g1[0]], [h2])]
    for j, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), j
    assert setup8.verifier() is setup8.verifier()  # built once


# ------------------------------------------------------------------------------------------------------ accept
def mont_int(c):
    return int(O.from_mont(np.asarray(c, dtype=np.uint64).reshape(1, 4))[0])


def opened(ctx, setup, bases, nu, sigma, seed, label):
    """one opening under a LegacyBlake2b transcript: the inputs, the proof, the tier-2 commitment of the combined rows, the prover's final transcript state"""
    inp = opening_inputs(ctx, bases, nu, sigma, seed)
    v_table, left, right = inp["tables"]
    t = ffi.HostTranscript(label)
    proof = dory_proof.prove(setup, inp["hints"], inp["scalars"], v_table, left, right, nu, sigma, transcript=t)
    state = t.state()
    t.close()
    combined = ctx.dory_state_alloc(ffi.DORY_KIND_G1, 1 << nu)
    ctx.dory_state_combine_hints(inp["hints"], inp["scalars"], combined)
    commitment = setup.tier2([combined])[0]
    for x in inp["hints"] + inp["tables"] + [combined]:
        x.free()
    return dict(inp=inp, proof=proof, commitment=commitment, state=state, y=fr_int(inp["y"]), left=fr_ints(inp["left"]), right=fr_ints(inp["right"]), nu=nu, sigma=sigma, label=label)


def verify(setup, o, label=None, **changed):
    """(accepted, failed_check, final transcript state) of jolt_host_dory_verify on a fresh transcript, with any of commitment, y, left, right, proof replaced"""
    a = dict(commitment=o["commitment"], y=o["y"], left=o["left"], right=o["right"], proof=o["proof"])
    a.update(changed)
    t = ffi.HostTranscript(o["label"] if label is None else label)
    try:
        accepted, failed = dory_proof.verify(setup, a["commitment"], a["y"], a["left"], a["right"], o["nu"], o["sigma"], a["proof"], transcript=t)
        return accepted, failed, t.state()
    finally:
        t.close()


@pytest.mark.parametrize("nu,sigma", [(1, 1), (2, 2), (1, 3), (3, 3)])
def test_the_librarys_own_proofs_are_accepted(ctx, bases, setup16, setup8, nu, sigma):
    o = opened(ctx, setup16, bases, nu, sigma, 12200 + 10 * nu + sigma, ffi.TRANSCRIPT_BLAKE2B | (12200 + sigma))
    assert verify(setup16, o) == (True, 0, o["state"])  # the caller's transcript ends where the prover's did: d came from a copy
    assert verify(setup8, o) == (True, 0, o["state"])   # another setup size: the proof uses prefixes of the bases, the verifier the matching levels
    # the callback form with the challenges replayed, and a d of the caller's
    proof = o["proof"]
    flat = [c for pair_ in proof.challenges for c in pair_] + [proof.gamma]
    seen = []

    def replayed(phase, rnd, gts, g1s, g2s):
        seen.append((phase, rnd, gts.shape[0], g1s.shape[0], g2s.shape[0]))
        if phase == ffi.DORY_PHASE_FIRST:
            return flat[2 * rnd]
        if phase == ffi.DORY_PHASE_SECOND:
            return flat[2 * rnd + 1]
        if phase == ffi.DORY_PHASE_GAMMA:
            return flat[2 * sigma]
        if phase == ffi.DORY_PHASE_D:
            return fr_int(o["inp"]["d"])
        return None

    assert dory_proof.verify(setup16, o["commitment"], o["y"], o["left"], o["right"], nu, sigma, proof, callback=replayed) == (True, 0)
    want_calls = [(ffi.DORY_PHASE_VMV, 0, 2, 1, 0)]
    for k in range(sigma):
        want_calls += [(ffi.DORY_PHASE_FIRST, k, 4, 1, 1), (ffi.DORY_PHASE_SECOND, k, 2, 2, 2)]
    want_calls += [(ffi.DORY_PHASE_GAMMA, sigma, 0, 0, 0), (ffi.DORY_PHASE_FINAL, sigma, 0, 1, 1), (ffi.DORY_PHASE_D, sigma, 0, 0, 0)]
    assert seen == want_calls
    # a zero challenge from the callback is JOLT_ERR_NOT_INVERTIBLE
    with pytest.raises(ffi.JoltError) as e:
        dory_proof.verify(setup16, o["commitment"], o["y"], o["left"], o["right"], nu, sigma, proof,
                          callback=lambda phase, *_: np.zeros(4, dtype=np.uint64) if phase == ffi.DORY_PHASE_D else replayed(phase, *_))
    assert e.value.status == ffi.ERR_NOT_INVERTIBLE
    if (nu, sigma) in ((1, 1), (2, 2)):  # the same decision as the verifier written out in the groups, on the same bytes
        inp = o["inp"]
        challenges = [(mont_int(b), mont_int(a)) for b, a in proof.challenges]
        args = (bases, o["commitment"], inp["y"], inp["left"], inp["right"], proof.vmv, proof.rounds)
        assert verify_in_the_groups(*args, proof.final, challenges, mont_int(proof.gamma), inp["d"]) is True
        w1_plus_g = O.g1_add(proof.final[0], O.g1_generator())
        assert verify_in_the_groups(*args, (w1_plus_g, proof.final[1]), challenges, mont_int(proof.gamma), inp["d"]) is False
        g1s = proof.g1s.copy()
        g1s[-1] = w1_plus_g
        assert verify(setup16, o, proof=dict(gts=proof.gts, g1s=g1s, g2s=proof.g2s))[:2] == (False, 2)


# ------------------------------------------------------------------------------------------------------ reject
def test_one_tampered_element_at_a_time_is_rejected_with_the_check_that_fails(ctx, bases, setup16):
    nu, sigma = 3, 3
    o = opened(ctx, setup16, bases, nu, sigma, 12300, ffi.TRANSCRIPT_BLAKE2B | 12300)
    proof = o["proof"]
    ht = setup16.verifier().values()[3 * 4 + 1]
    assert np.array_equal(ht, pair([bases["h1"]], [bases["h2"]]))
    times_ht = lambda x: ffi.host_fq12_op(ffi.FQ12_MUL, x, ht)  # noqa: E731
    plus_g1 = lambda p: O.g1_add(p, O.g1_generator())  # noqa: E731
    plus_g2 = lambda p: ffi.host_g2_add(p, G2.point(1))  # noqa: E731

    def altered(kind, i, f):
        p = dict(gts=proof.gts.copy(), g1s=proof.g1s.copy(), g2s=proof.g2s.copy())
        p[kind][i] = f(p[kind][i])
        return dict(proof=p)

    middle = 1  # the middle round of three
    cases = [("C", altered("gts", 0, times_ht), 2), ("D2", altered("gts", 1, times_ht), 1), ("E1", altered("g1s", 0, plus_g1), 1),
             ("a GT of the middle round", altered("gts", 2 + 6 * middle + 1, times_ht), 2), ("C+ of the middle round", altered("gts", 2 + 6 * middle + 4, times_ht), 2),
             ("a G1 of the middle round", altered("g1s", 1 + 3 * middle + 1, plus_g1), 2), ("a G2 of the middle round", altered("g2s", 3 * middle, plus_g2), 2),
             ("w1", altered("g1s", 1 + 3 * sigma, plus_g1), 2), ("w2", altered("g2s", 3 * sigma, plus_g2), 2),
             ("y", dict(y=fr_int(o["inp"]["y"] + 1)), 2), ("the commitment", dict(commitment=times_ht(o["commitment"])), 2),
             ("a coordinate of L", dict(left=fr_ints([o["inp"]["left"][0] + 1] + o["inp"]["left"][1:])), 2),
             ("a coordinate of R", dict(right=fr_ints(o["inp"]["right"][:-1] + [o["inp"]["right"][-1] + 1])), 2),
             ("the transcript label", dict(label=ffi.TRANSCRIPT_BLAKE2B | 12301), 2)]
    for what, change, failed in cases:
        accepted, failed_check, _ = verify(setup16, o, **change)  # JOLT_OK: a rejected proof raises nothing
        assert (accepted, failed_check) == (False, failed), what
    # the context stays usable, and the honest proof still verifies
    assert verify(setup16, o) == (True, 0, o["state"])


def test_malformed_input_is_a_status_and_the_transcript_does_not_move(ctx, bases, setup16):
    o = opened(ctx, setup16, bases, 1, 2, 12400, ffi.TRANSCRIPT_BLAKE2B | 12400)
    proof = o["proof"]
    fresh = ffi.HostTranscript(o["label"])
    start = fresh.state()
    as_dict = lambda **kw: dict(dict(gts=proof.gts, g1s=proof.g1s, g2s=proof.g2s), **kw)  # noqa: E731
    bad_gt, bad_g1, bad_y = proof.gts.copy(), proof.g1s.copy(), np.array(O.int_to_limbs(R), dtype=np.uint64)
    bad_gt[3, 0:4] = np.array(O.int_to_limbs(O.Q_MOD), dtype=np.uint64)
    bad_g1[0, 4] ^= np.uint64(1)  # E1 off the curve (with nu < sigma some of the rounds' points are the identity, whatever x and y hold)
    vs = setup16.verifier()

    def status(**kw):
        a = dict(commitment=o["commitment"], y=o["y"], left=o["left"], right=o["right"], nu=1, sigma=2, proof=as_dict())
        a.update(kw)
        with pytest.raises(ffi.JoltError) as e:
            ctx.dory_verify(vs, a["commitment"], a["y"], a["left"], a["right"], a["nu"], a["sigma"], a["proof"], transcript=fresh)
        return e.value.status

    assert status(proof=as_dict(gts=bad_gt)) == INVALID_ARG
    assert status(proof=as_dict(g1s=bad_g1)) == INVALID_ARG
    assert status(y=bad_y) == INVALID_ARG
    assert status(commitment=bad_gt[3]) == INVALID_ARG
    # nu > sigma, and more columns than the setup has bases (the proof arrays sized for the sigma named)
    big = dict(gts=np.tile(proof.gts[:1], (2 + 6 * 5, 1)), g1s=np.tile(proof.g1s[:1], (2 + 3 * 5, 1)), g2s=np.tile(proof.g2s[:1], (1 + 3 * 5, 1)))
    assert status(nu=1, sigma=5, proof=big, right=fr_ints([1] * 32)) == ffi.ERR_SRS_TOO_SMALL
    small = dict(gts=proof.gts[:8], g1s=proof.g1s[:5], g2s=proof.g2s[:4])
    assert status(nu=2, sigma=1, proof=small, left=fr_ints([1] * 4), right=fr_ints([1] * 2)) == INVALID_ARG
    assert fresh.state() == start  # everything was checked before the transcript absorbed anything
    fresh.close()
    assert verify(setup16, o) == (True, 0, o["state"])


# ------------------------------------------------------------------------------------------------------ the batch of stage 8
@pytest.mark.parametrize("how", [dict(dory_blocks=[4, 1]), dict(dory_order="address_major")], ids=["blocks", "address_major"])
def test_workload_batch_verifies_and_rejects(ctx, how):
    """n_vars = 4: the smallest grid the workload allows, sigma = 4; two small blocks behind the 38 columns, and the address-major placement"""
    w = DeviceWorkload(ctx, 4, seed=12500, pcs="dory", **how)
    try:
        label = ffi.TRANSCRIPT_BLAKE2B | 12500
        commit = w.dory_commit()
        out = w.dory_open(label)
        assert w.dory_sigma == 4 and len(commit["tier2"]) == 38 + len(how.get("dory_blocks", []))
        assert w.dory_verify(commit, out, label) is True
        res = w.dory_verify_result
        assert res["failed_check"] == 0 and res["transcript_state"] == out["transcript_state"] and np.array_equal(res["joint_eval"], out["joint_eval"])
        # combine: the RLC of the commitments under gamma's powers, against the host loop
        order = w.column_of_claim
        tier2 = commit["tier2"] if order is None else commit["tier2"][list(order)]
        host = gt_mul(*[gt_pow(t, mont_int(s)) for t, s in zip(tier2, out["scalars"])])
        assert np.array_equal(w.dory_setup.combine(tier2, out["scalars"]), host)
        # one altered evaluation
        claims = (w.opening_claims if order is None else w.opening_claims[list(order)]).copy()
        claims[3] = fr_int(mont_int(claims[3]) + 1)
        assert w.dory_verify(commit, out, label, evaluations=claims) is False and w.dory_verify_result["failed_check"] == 2
        # two swapped commitments
        swapped = commit["tier2"].copy()
        j = next(k for k in range(1, len(swapped)) if not np.array_equal(swapped[k], swapped[0]))
        swapped[[0, j]] = swapped[[j, 0]]
        assert w.dory_verify(dict(tier2=swapped), out, label) is False and w.dory_verify_result["failed_check"] == 2
        # one altered proof GT
        forged = dict(out, gts=out["gts"].copy())
        forged["gts"][3] = out["gts"][2]
        assert not np.array_equal(out["gts"][3], out["gts"][2])
        assert w.dory_verify(commit, forged, label) is False and w.dory_verify_result["failed_check"] == 2
        # and the honest one again
        assert w.dory_verify(commit, out, label) is True
    finally:
        w.close()
