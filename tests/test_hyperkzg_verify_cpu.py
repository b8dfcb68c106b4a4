"""CPU checks of the HyperKZG verifier's host half (hyperkzg_verify.hip): the model of tests/hyperkzg_verify_model.py accepts its own honest log-space openings and
rejects every one-off error with the right code; jolt_host_hyperkzg_verify_scalars gives the model's folding decision and the model's scalars; the refusals; the
device entries without a device; the bindings.  Everything here is arithmetic modulo r."""
import os
import re

import numpy as np
import pytest

import hyperkzg_verify_model as M
import oracle_lib as O
from dory_groups import R, fr_int, fr_ints, rand_ints
from jolt_amd import ffi

NEW_SYMBOLS = ["jolt_hyperkzg_verifier_setup_create", "jolt_hyperkzg_verifier_setup_from_secret", "jolt_hyperkzg_verifier_setup_points", "jolt_hyperkzg_verifier_setup_free",
               "jolt_host_hyperkzg_verify_scalars", "jolt_host_hyperkzg_verify_with_transcript", "jolt_host_hyperkzg_verify",
               "jolt_host_hyperkzg_prove_batch", "jolt_host_hyperkzg_verify_batch"]
ELLS = [1, 2, 3, 5]


def ints(a):
    return [int(x) for x in O.from_mont(np.asarray(a, dtype=np.uint64).reshape(-1, 4))]


def case(ell, seed):
    """a random log-space setup, polynomial, point, challenges and the model's honest opening"""
    beta, r, q, d0 = rand_ints(4, seed)
    evals, point = rand_ints(1 << ell, seed + 1), rand_ints(ell, seed + 2)
    ch = (r, q, d0)
    return dict(ell=ell, beta=beta, evals=evals, point=point, ch=ch, commitment=M.commit(beta, evals), y=M.multilinear_eval(evals, point),
                proof=M.open_(beta, evals, point, ch))


def model_verify(c, proof=None, y=None, commitment=None):
    return M.verify(c["beta"], [c["commitment"] if commitment is None else commitment], [1], c["point"], c["y"] if y is None else y, proof or c["proof"], c["ch"])


def with_v(proof, t, j, delta=1):
    v = [list(row) for row in proof["v"]]
    v[t][j] = (v[t][j] + delta) % R
    return dict(proof, v=v)


def library_scalars(c, proof=None, y=None):
    p = proof or c["proof"]
    out = ffi.host_hyperkzg_verify_scalars(fr_ints(c["point"]), fr_int(c["y"] if y is None else y), fr_ints([x for row in p["v"] for x in row]), *[fr_int(x) for x in c["ch"]])
    return dict(folding_ok=out["folding_ok"], failed_level=out["failed_level"], l_scalars=ints(out["l_scalars"]), d=ints(out["d"]))


@pytest.mark.parametrize("ell", ELLS)
def test_the_model_accepts_its_own_honest_openings(ell):
    c = case(ell, 7000 + ell)
    assert len(c["proof"]["com"]) == ell - 1 and all(len(row) == ell for row in c["proof"]["v"])
    assert model_verify(c) == (True, 0, 0)
    # ... and the combination of several commitments under scalars, C_0 never built (scheme.rs:346-352)
    parts = [rand_ints(1 << ell, 7100 + 10 * ell + i) for i in range(3)]
    s = rand_ints(3, 7200 + ell)
    joint = [sum(si * p[k] for si, p in zip(s, parts)) % R for k in range(1 << ell)]
    proof = M.open_(c["beta"], joint, c["point"], c["ch"])
    coms = [M.commit(c["beta"], p) for p in parts]
    y = M.multilinear_eval(joint, c["point"])
    assert M.verify(c["beta"], coms, s, c["point"], y, proof, c["ch"]) == (True, 0, 0)
    assert M.verify(c["beta"], coms, [s[0], s[1] + 1, s[2]], c["point"], y, proof, c["ch"]) == (False, 2, 0)


@pytest.mark.parametrize("ell", ELLS)
def test_the_model_rejects_each_one_off_error(ell):
    c = case(ell, 7300 + ell)
    for j in range(ell):  # a changed v entry at every level, in each row
        # v[0][j] and v[1][j] enter level j's equation alone; v[2][j] is level j - 1's y_next (v[2][0] enters no equation: the pairing check catches it)
        assert model_verify(c, with_v(c["proof"], 0, j)) == (False, 1, j)
        assert model_verify(c, with_v(c["proof"], 1, j)) == (False, 1, j)
        assert model_verify(c, with_v(c["proof"], 2, j)) == ((False, 1, j - 1) if j else (False, 2, 0))
    assert model_verify(c, y=(c["y"] + 1) % R) == (False, 1, ell - 1)
    for k in range(3):
        w = list(c["proof"]["w"])
        w[k] = (w[k] + 1) % R
        assert model_verify(c, dict(c["proof"], w=w)) == (False, 2, 0)
    for i in range(ell - 1):
        com = list(c["proof"]["com"])
        com[i] = (com[i] + 1) % R
        assert model_verify(c, dict(c["proof"], com=com)) == (False, 2, 0)
    assert model_verify(c, commitment=(c["commitment"] + 1) % R) == (False, 2, 0)
    assert M.verify((c["beta"] + 1) % R, [c["commitment"]], [1], c["point"], c["y"], c["proof"], c["ch"]) == (False, 2, 0)


@pytest.mark.parametrize("ell", ELLS)
def test_the_librarys_scalars_are_the_models(ell):
    c = case(ell, 7400 + ell)
    want, (d0, d1) = M.verify_scalars(c["proof"]["v"], *c["ch"])
    got = library_scalars(c)
    assert got["folding_ok"] is True and got["failed_level"] == 0
    assert got["l_scalars"] == want and len(want) == ell + 4 and got["d"] == [d0, d1] and d1 == d0 * d0 % R
    # the honest opening satisfies L == beta R under them: the scalars are the verifier's, not merely equal lists
    bases = [c["commitment"]] + c["proof"]["com"] + c["proof"]["w"] + [1]
    w = c["proof"]["w"]
    assert sum(b * s for b, s in zip(bases, got["l_scalars"])) % R == c["beta"] * (w[0] + got["d"][0] * w[1] + got["d"][1] * w[2]) % R
    # random values in place of a proof: any folding decision, the same scalars as the model
    rnd = dict(v=[rand_ints(ell, 7500 + 10 * ell + t) for t in range(3)])
    want, _ = M.verify_scalars(rnd["v"], *c["ch"])
    got = library_scalars(c, rnd)
    assert got["l_scalars"] == want
    level = M.folding_check(c["point"], c["y"], rnd["v"], c["ch"][0])
    assert got["folding_ok"] == (level is None) and got["failed_level"] == (level or 0)


@pytest.mark.parametrize("ell", ELLS)
def test_the_first_failing_level_is_named(ell):
    c = case(ell, 7600 + ell)
    for j in range(ell):
        got = library_scalars(c, with_v(c["proof"], 0, j))
        assert (got["folding_ok"], got["failed_level"]) == (False, j)
        if j + 1 < ell:  # two levels fail: the first is reported
            got = library_scalars(c, with_v(with_v(c["proof"], 0, j), 1, ell - 1))
            assert (got["folding_ok"], got["failed_level"]) == (False, j)
    got = library_scalars(c, y=(c["y"] + 1) % R)
    assert (got["folding_ok"], got["failed_level"]) == (False, ell - 1)
    assert M.folding_check(c["point"], (c["y"] + 1) % R, c["proof"]["v"], c["ch"][0]) == ell - 1


def test_the_scalars_refuse_malformed_input():
    c = case(2, 7700)
    point, y, v = fr_ints(c["point"]), fr_int(c["y"]), fr_ints([x for row in c["proof"]["v"] for x in row])
    ch = [fr_int(x) for x in c["ch"]]
    ffi.host_hyperkzg_verify_scalars(point, y, v, *ch)
    with pytest.raises(ffi.JoltError) as e:  # ell = 0: EmptyPoint
        ffi.host_hyperkzg_verify_scalars(np.zeros((0, 4), dtype=np.uint64), y, np.zeros((0, 4), dtype=np.uint64), *ch)
    assert e.value.status == ffi.ERR_INVALID_ARG
    not_canonical = np.array(O.int_to_limbs(R), dtype=np.uint64)
    bad_point, bad_v = point.copy(), v.copy()
    bad_point[1], bad_v[5] = not_canonical, not_canonical
    for args in [(bad_point, y, v, *ch), (point, not_canonical, v, *ch), (point, y, bad_v, *ch), (point, y, v, not_canonical, ch[1], ch[2]),
                 (point, y, v, ch[0], not_canonical, ch[2]), (point, y, v, ch[0], ch[1], not_canonical)]:
        with pytest.raises(ffi.JoltError) as e:
            ffi.host_hyperkzg_verify_scalars(*args)
        assert e.value.status == ffi.ERR_INVALID_ARG
    with pytest.raises(ffi.JoltError) as e:  # r = 0: DegenerateChallenge
        ffi.host_hyperkzg_verify_scalars(point, y, v, np.zeros(4, dtype=np.uint64), ch[1], ch[2])
    assert e.value.status == ffi.ERR_NOT_INVERTIBLE


def test_no_device_no_verifier():
    """the device entries refuse a null context instead of computing on the host, and write nothing"""
    lib, p = ffi.lib(), lambda a: a.ctypes.data_as(ffi.C.c_void_p)  # noqa: E731
    g1, g2, fr1 = np.zeros(12, dtype=np.uint64), np.zeros(24, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    out = ffi.C.c_void_p()
    assert lib.jolt_hyperkzg_verifier_setup_create(None, p(g1), p(g2), p(g2), ffi.C.byref(out)) == ffi.ERR_INVALID_ARG and not out
    assert lib.jolt_hyperkzg_verifier_setup_from_secret(None, p(fr1), p(g1), p(g2), ffi.C.byref(out)) == ffi.ERR_INVALID_ARG and not out
    accepted, failed, level = ffi.C.c_int32(-1), ffi.C.c_int32(-1), ffi.C.c_size_t(99)
    w, v = np.zeros((3, 12), dtype=np.uint64), np.zeros((3, 4), dtype=np.uint64)
    t = ffi.HostTranscript(5)
    before = t.state()
    tail = (ffi.C.byref(accepted), ffi.C.byref(failed), ffi.C.byref(level))
    assert lib.jolt_host_hyperkzg_verify(None, None, p(g1), p(fr1), 1, p(fr1), 1, p(fr1), None, p(w), p(v), t.h, *tail) == ffi.ERR_INVALID_ARG
    joint = np.zeros(4, dtype=np.uint64)
    assert lib.jolt_host_hyperkzg_verify_batch(None, None, p(g1), p(fr1), 1, p(fr1), 1, None, p(w), p(v), t.h, *tail, p(joint)) == ffi.ERR_INVALID_ARG
    fn = ffi.OPEN_TRANSCRIPT_FN(lambda *a: 1 / 0)
    assert lib.jolt_host_hyperkzg_verify_with_transcript(None, None, p(g1), p(fr1), 1, p(fr1), 1, p(fr1), None, p(w), p(v), fn, None, *tail) == ffi.ERR_INVALID_ARG
    ch = np.zeros((3, 4), dtype=np.uint64)
    assert lib.jolt_host_hyperkzg_prove_batch(None, None, None, 0, None, 0, 0, p(fr1), 1, p(fr1), 1, None, 0, t.h, None, p(w), p(v), p(ch), p(joint)) == ffi.ERR_INVALID_ARG
    assert (accepted.value, failed.value, level.value) == (-1, -1, 99) and t.state() == before and not joint.any()
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
    assert "pub struct jolt_hyperkzg_verifier_setup" in ffi_rs
    for method in ("hyperkzg_verifier_setup", "hyperkzg_verify", "hyperkzg_prove_batch", "hyperkzg_verify_batch"):
        assert callable(getattr(ffi.Context, method))
    from jolt_amd import build, workload
    assert "hyperkzg_verify.hip" in build.SOURCES and callable(workload.DeviceWorkload.verify)
