"""CPU checks of the Dory verifier's host half (dory_verify.hip): every exponent of the final equation (jolt_host_dory_verify_exponents) against the log-space model of
tests/dory_open_model.py -- on honest proofs the one product of powers equals the pairing side, and on random or perturbed elements "the VMV check and that identity"
is exactly the model's decision -- the refusals, the transcript copy the verifier draws d from, and the bindings.  Everything here is arithmetic modulo r."""
import os
import re

import numpy as np
import pytest

import dory_open_model as OM
import dory_reduce_model as DM
import oracle_lib as O
from dory_groups import R, fr_int, fr_ints, rand_ints
from jolt_amd import abi, ffi

NEW_SYMBOLS = ["jolt_dory_gt_pow_many", "jolt_dory_gt_multi_exp", "jolt_dory_verifier_setup_create", "jolt_dory_verifier_setup_free", "jolt_dory_verifier_setup_values",
               "jolt_host_dory_verify_exponents", "jolt_host_dory_verify_with_transcript", "jolt_host_dory_verify", "jolt_host_dory_verify_batch",
               "jolt_host_transcript_clone", "jolt_dory_verifier_setup_timing"]
SHAPES = [(1, 1), (1, 2), (2, 2), (1, 3), (3, 3)]  # (nu, sigma): nu <= sigma, nu < sigma among them


def ints(a):
    return [int(x) for x in O.from_mont(np.asarray(a, dtype=np.uint64).reshape(-1, 4))]


def case(nu, sigma, seed):
    """a random log-space setup, statement, challenges and the model's honest proof"""
    rows, n = 1 << nu, 1 << sigma
    g1, g2 = rand_ints(n, seed), rand_ints(n, seed + 1)
    h1, h2, gamma, d = rand_ints(4, seed + 2)
    matrix = [rand_ints(n, seed + 10 + i) for i in range(rows)]
    left, right = rand_ints(rows, seed + 3), rand_ints(n, seed + 4)
    t_rows, commitment, v, y = OM.statement(g1, g2, matrix, left, right)
    challenges = [tuple(rand_ints(2, seed + 30 + k)) for k in range(sigma)]
    proof = OM.prove(g1, g2, h1, h2, t_rows, v, left, right, challenges, gamma)
    return dict(nu=nu, sigma=sigma, g1=g1, g2=g2, h1=h1, h2=h2, gamma=gamma, d=d, left=left, right=right, commitment=commitment, y=y, challenges=challenges, proof=proof)


def folded_scalars(c):
    n = len(c["right"])
    s1, s2 = list(c["right"]), OM.pad(c["left"], n)
    for _, alpha in c["challenges"]:
        h, ai = n // 2, pow(alpha, -1, R)
        s1 = [(alpha * l + r) % R for l, r in zip(s1[:h], s1[h:])]  # noqa: E741
        s2 = [(ai * l + r) % R for l, r in zip(s2[:h], s2[h:])]  # noqa: E741
        n = h
    return s1[0], s2[0]


def setup_logs(c):
    """the verifier's values in the order of jolt_dory_verifier_setup_values, from dory_reduce_model.State.setup() and the bases"""
    sigma, g1, g2 = c["sigma"], c["g1"], c["g2"]
    levels = [DM.State([0] * (1 << (sigma - k)), [0] * (1 << (sigma - k)), [], [], g1, g2).setup() for k in range(sigma)]
    chi = [lv[0] for lv in levels] + [g1[0] * g2[0] % R]  # the last level is the single pair; State.setup() halves, so it stops one level above
    for k in range(sigma):  # Delta1L = Delta2L = chi of the next level: they need no entry of their own
        assert levels[k][1] == levels[k][3] == chi[k + 1]
    return chi + [lv[2] for lv in levels] + [lv[4] for lv in levels] + [c["h1"] * c["h2"] % R, c["h1"] * g2[0] % R, g1[0] * c["h2"] % R]


def exponents(c):
    flat = [x for pair in c["challenges"] for x in pair] + [c["gamma"]]
    s1, s2 = folded_scalars(c)
    e = ffi.host_dory_verify_exponents(c["sigma"], fr_ints(flat), fr_int(c["d"]), fr_int(s1), fr_int(s2), fr_int(c["y"]))
    return {k: (ints(v) if np.asarray(v).ndim == 2 else ints(v)[0]) for k, v in e.items()}


def identity_holds(c, proof, commitment, e):
    """sum exponent * log over the proof's GT elements, the commitment and the setup values == the three pairings of the final check, in logs"""
    gts = list(proof["vmv"][:2]) + [x for first, second in proof["rounds"] for x in list(first[:4]) + list(second[:2])]
    rhs = (DM.ip(e["proof_gt"], gts) + e["commitment"] * commitment + DM.ip(e["setup"], setup_logs(c))) % R
    g1s = [proof["vmv"][2]] + [x for first, second in proof["rounds"] for x in (first[4], second[2], second[3])]
    g2s = [x for first, second in proof["rounds"] for x in (first[5], second[4], second[5])]
    e1 = DM.ip(e["g1"], g1s)
    e2 = (e["h2"] * c["h2"] + DM.ip(e["g2"], g2s)) % R
    w1, w2 = proof["final"]
    gamma, d = c["gamma"], c["d"]
    lhs = ((w1 + d * c["g1"][0]) * (w2 + pow(d, -1, R) * c["g2"][0]) - gamma * c["h1"] * e2 - pow(gamma, -1, R) * e1 * c["h2"]) % R
    return lhs == rhs


def decision(c, proof, commitment, y):
    """the decision the library's verifier takes, in logs: the VMV check and the one identity"""
    c2 = dict(c, y=y)
    vmv = proof["vmv"][2] * c["h2"] % R == proof["vmv"][1] % R
    return vmv and identity_holds(c2, proof, commitment, exponents(c2))


def model_decision(c, proof, commitment, y):
    return OM.verify(c["g1"], c["g2"], c["h1"], c["h2"], commitment, y, c["left"], c["right"], proof, c["challenges"], c["gamma"], c["d"])


@pytest.mark.parametrize("nu,sigma", SHAPES)
def test_honest_proofs_satisfy_the_one_product_of_powers(nu, sigma):
    c = case(nu, sigma, 5000 + 100 * nu + sigma)
    e = exponents(c)
    assert len(e["proof_gt"]) == 2 + 6 * sigma and len(e["setup"]) == 3 * sigma + 4 and len(e["g1"]) == 1 + 3 * sigma and len(e["g2"]) == 3 * sigma
    assert e["g1"][0] == 1 and e["h2"] == c["y"] and e["proof_gt"][0] == 1
    assert identity_holds(c, c["proof"], c["commitment"], e)
    assert model_decision(c, c["proof"], c["commitment"], c["y"]) and decision(c, c["proof"], c["commitment"], c["y"])


def perturbed(proof, where):
    """the proof with one element replaced by itself + 1"""
    vmv, rounds, final = list(proof["vmv"]), [(list(f), list(s)) for f, s in proof["rounds"]], list(proof["final"])
    kind, i = where
    if kind == "vmv":
        vmv[i] = (vmv[i] + 1) % R
    elif kind == "first":
        rounds[len(rounds) // 2][0][i] = (rounds[len(rounds) // 2][0][i] + 1) % R
    elif kind == "second":
        rounds[len(rounds) // 2][1][i] = (rounds[len(rounds) // 2][1][i] + 1) % R
    else:
        final[i] = (final[i] + 1) % R
    return dict(vmv=tuple(vmv), rounds=[(tuple(f), tuple(s)) for f, s in rounds], final=tuple(final))


@pytest.mark.parametrize("nu,sigma", [(1, 1), (1, 2), (3, 3)])
def test_the_decision_is_the_models_on_honest_perturbed_and_random_elements(nu, sigma):
    c = case(nu, sigma, 5200 + 100 * nu + sigma)
    honest = c["proof"]
    # one perturbed element per class: the VMV GTs and E1, a round's GTs of both messages, its G1 and G2 elements, w1 and w2
    places = [("vmv", 0), ("vmv", 1), ("vmv", 2), ("first", 0), ("first", 1), ("first", 2), ("first", 3), ("first", 4), ("first", 5), ("second", 0), ("second", 1),
              ("second", 2), ("second", 3), ("second", 4), ("second", 5), ("final", 0), ("final", 1)]
    for where in places:
        p = perturbed(honest, where)
        assert model_decision(c, p, c["commitment"], c["y"]) is False and decision(c, p, c["commitment"], c["y"]) is False, where
    # the statement's side: y, the commitment
    assert not model_decision(c, honest, c["commitment"], c["y"] + 1) and not decision(c, honest, c["commitment"], (c["y"] + 1) % R)
    assert not model_decision(c, honest, c["commitment"] + 1, c["y"]) and not decision(c, honest, (c["commitment"] + 1) % R, c["y"])
    # random elements everywhere: both decisions are the same predicate of the elements, and both reject
    rnd = iter(rand_ints(3 + 12 * sigma + 2, 5300 + sigma))
    p = dict(vmv=tuple(next(rnd) for _ in range(3)), rounds=[(tuple(next(rnd) for _ in range(6)), tuple(next(rnd) for _ in range(6))) for _ in range(sigma)],
             final=(next(rnd), next(rnd)))
    assert model_decision(c, p, c["commitment"], c["y"]) == decision(c, p, c["commitment"], c["y"]) == False  # noqa: E712


def test_a_dishonest_proof_the_model_accepts_is_accepted():
    """random round messages, then C chosen so that the model's final equation holds: the model accepts, so the product of powers must hold too (the two decisions
    agree on accepted inputs that no honest prover made)"""
    c = case(1, 2, 5400)
    rnd = iter(rand_ints(64, 5401))
    e1 = next(rnd)
    base = dict(vmv=(0, e1 * c["h2"] % R, e1), rounds=[(tuple(next(rnd) for _ in range(6)), tuple(next(rnd) for _ in range(6))) for _ in range(2)], final=(next(rnd), next(rnd)))
    # the model's equation is  lhs == const + C  (C enters with coefficient one): solve for C by evaluating both sides at C = 0
    g1, g2, h1, h2, gamma, d = c["g1"], c["g2"], c["h1"], c["h2"], c["gamma"], c["d"]
    claims = (0, c["commitment"] % R, base["vmv"][1], e1, c["y"] * h2 % R)
    n, s1, s2 = 4, list(c["right"]), OM.pad(c["left"], 4)
    for (first, second), (beta, alpha) in zip(base["rounds"], c["challenges"]):
        claims = DM.invariants(claims, DM.State([0] * n, [0] * n, [0] * n, [0] * n, g1, g2).setup(), first, second, beta, alpha)
        h, ai = n // 2, pow(alpha, -1, R)
        s1 = [(alpha * l + r) % R for l, r in zip(s1[:h], s1[h:])]  # noqa: E741
        s2 = [(ai * l + r) % R for l, r in zip(s2[:h], s2[h:])]  # noqa: E741
        n = h
    cc, d1, d2, ee1, ee2 = claims
    gi, di = pow(gamma, -1, R), pow(d, -1, R)
    rhs0 = (g1[0] * g2[0] + cc + s1[0] * s2[0] * h1 * h2 + gamma * h1 * ee2 + gi * ee1 * h2 + d * (d2 + gi * s2[0] * g1[0] * h2) + di * (d1 + gamma * s1[0] * h1 * g2[0])) % R
    w1, w2 = base["final"]
    lhs = (w1 + d * g1[0]) * (w2 + di * g2[0]) % R
    forged = dict(base, vmv=((lhs - rhs0) % R, base["vmv"][1], e1))
    assert model_decision(c, forged, c["commitment"], c["y"]) is True
    assert decision(c, forged, c["commitment"], c["y"]) is True


def test_exponents_refuse_malformed_input():
    c = case(1, 2, 5500)
    flat = fr_ints([x for pair in c["challenges"] for x in pair] + [c["gamma"]])
    one = fr_int(1)
    good = (fr_int(c["d"]), one, one, one)
    ffi.host_dory_verify_exponents(2, flat, *good)
    with pytest.raises(ffi.JoltError) as e:
        ffi.host_dory_verify_exponents(31, np.zeros((63, 4), dtype=np.uint64) + one, *good)
    assert e.value.status == ffi.ERR_INVALID_ARG
    not_canonical = np.array(O.int_to_limbs(R), dtype=np.uint64)
    for slot in range(4):
        args = list(good)
        args[slot] = not_canonical
        with pytest.raises(ffi.JoltError) as e:
            ffi.host_dory_verify_exponents(2, flat, *args)
        assert e.value.status == ffi.ERR_INVALID_ARG
    bad = flat.copy()
    bad[1] = not_canonical
    with pytest.raises(ffi.JoltError) as e:
        ffi.host_dory_verify_exponents(2, bad, *good)
    assert e.value.status == ffi.ERR_INVALID_ARG
    for slot in (0, 3, 4):  # a zero beta, a zero alpha, a zero gamma; then a zero d
        zero = flat.copy()
        zero[slot] = 0
        with pytest.raises(ffi.JoltError) as e:
            ffi.host_dory_verify_exponents(2, zero, *good)
        assert e.value.status == ffi.ERR_NOT_INVERTIBLE
    with pytest.raises(ffi.JoltError) as e:
        ffi.host_dory_verify_exponents(2, flat, np.zeros(4, dtype=np.uint64), one, one, one)
    assert e.value.status == ffi.ERR_NOT_INVERTIBLE


@pytest.mark.parametrize("engine", [ffi.TRANSCRIPT_TEST, ffi.TRANSCRIPT_BLAKE2B, ffi.TRANSCRIPT_KECCAK, ffi.TRANSCRIPT_BLAKE2B_SPONGE])
def test_a_transcript_copy_draws_what_the_original_would_and_leaves_it_alone(engine):
    t = ffi.HostTranscript(engine | 77)
    t.append(fr_ints([3, 5, 7]))
    t.challenge(full_width=True)
    t.append_bytes(b"between")
    before = t.state()
    copy = t.clone()
    assert copy.state() == before
    d = copy.challenge(full_width=True)
    copy.append(fr_ints([9]))
    assert t.state() == before  # nothing the copy did reached the original
    assert np.array_equal(t.challenge(full_width=True), d)
    copy.close()
    t.close()


def test_the_bindings_declare_the_new_entries():
    root = os.path.join(os.path.dirname(__file__), "..")
    header = open(os.path.join(root, "include", "jolt_hip.h")).read()
    ffi_rs = open(os.path.join(root, "rust", "jolt-kernels-hip", "src", "ffi.rs")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert re.search(r"\bpub fn %s\s*\(" % name, ffi_rs), name
        fn = getattr(ffi.lib(), name)
        assert fn.argtypes is not None and fn.restype is not None, name  # abi.py parsed the prototype from the header
    assert ffi.DORY_PHASE_D == 5 and abi.CONSTANTS["JOLT_DORY_PHASE_D"] == 5
    for method in ("dory_gt_pow_many", "dory_gt_multi_exp", "dory_verify", "dory_verify_batch"):
        assert callable(getattr(ffi.Context, method))
    assert callable(ffi.DoryLibSetup.verifier) and callable(ffi.DoryLibSetup.combine)


def test_no_device_no_verifier():
    """the device entries refuse a null context instead of computing on the host"""
    out = np.zeros(48, dtype=np.uint64)
    assert ffi.lib().jolt_dory_gt_multi_exp(None, None, None, 0, out.ctypes.data_as(ffi.C.c_void_p)) == ffi.ERR_INVALID_ARG
    assert not out.any()
