"""CPU checks of the Dory evaluation proof as one library call (dory_scheme.hip): the G2 and GT byte forms against a restatement in Python integers, the transcript
appends on all four engines against a replay through the existing bindings, the element counts, the bindings, and the refusal to run without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import g2_model as M
import oracle_lib as O
import pairing_model as PM
from dory_groups import G1, G2, rand_ints
from jolt_amd import ffi

Q = O.Q_MOD
ENGINES = [ffi.TRANSCRIPT_TEST, ffi.TRANSCRIPT_BLAKE2B, ffi.TRANSCRIPT_KECCAK, ffi.TRANSCRIPT_BLAKE2B_SPONGE]
NEW_SYMBOLS = ["jolt_dory_setup_create", "jolt_dory_setup_free", "jolt_dory_setup_size", "jolt_dory_setup_tier2", "jolt_dory_round_update",
               "jolt_host_dory_open_with_transcript", "jolt_host_dory_open", "jolt_host_dory_proof_counts", "jolt_host_g2_serialize_compressed",
               "jolt_host_gt_serialize", "jolt_host_dory_transcript_append_gt", "jolt_host_dory_transcript_append_g1", "jolt_host_dory_transcript_append_g2"]


# ---------------------------------------------------------------- the byte forms, restated: ark-serialize's compressed short-Weierstrass form over Fp2, Fp12 as its coefficients
def le32(v):
    return int(v).to_bytes(32, "little")


def g2_bytes_affine(p):
    """p: None or ((x0, x1), (y0, y1)) in canonical integers"""
    if p is None:
        return bytes(63) + bytes([0x40])
    (x0, x1), (y0, y1) = p
    out = bytearray(le32(x0) + le32(x1))
    if (y1, y0) > (-y1 % Q, -y0 % Q):  # Fp2's order: c1 first, then c0
        out[63] |= 0x80
    return bytes(out)


def g2_bytes(abi):
    return g2_bytes_affine(M.from_abi(abi))


def gt_bytes(abi):
    a = np.asarray(abi, dtype=np.uint64).reshape(12, 4)
    rinv = pow(1 << 256, -1, Q)
    return b"".join(le32(O.limbs_to_int(a[k]) * rinv % Q) for k in range(12))


def raw_g2(x, y, z=(1, 0)):
    return np.concatenate([M.fq2_to_abi(x), M.fq2_to_abi(y), M.fq2_to_abi(z)])


def test_g2_byte_form_is_its_restatement():
    assert ffi.host_g2_serialize_compressed(G2.point(0)) == bytes(63) + bytes([0x40])
    # the identity in another representative: z = 0 decides, whatever x and y hold
    assert ffi.host_g2_serialize_compressed(raw_g2((5, 7), (11, 13), (0, 0))) == bytes(63) + bytes([0x40])
    seen = set()
    for k in [1, 2, 3, 7, O.R_MOD - 1, O.R_MOD - 2] + rand_ints(6, 2000):
        for rep in (0, 4):
            pt = G2.point(k, rep=rep)
            got = ffi.host_g2_serialize_compressed(pt)
            assert got == g2_bytes(pt) and len(got) == 64 and not got[63] & 0x40, k
            seen.add(got[63] >> 7)
        # k G and -k G: one x, the two signs of y, exactly one of them flagged
        neg = ffi.host_g2_serialize_compressed(G2.point(-k))
        assert neg[:63] == got[:63] and (neg[63] ^ got[63]) == 0x80
    assert seen == {0, 1}
    # the serialiser takes canonical coordinates and checks nothing else, so the comparison's corners are reached with chosen y: c1 = 0 (c0 decides), c0 = 0
    t_small, t_large = 5, Q - 5
    for y, flag in [((t_small, 0), 0), ((t_large, 0), 0x80), ((0, t_small), 0), ((0, t_large), 0x80), ((t_large, t_small), 0), ((t_small, t_large), 0x80),
                    (((Q - 1) // 2, 0), 0), (((Q + 1) // 2, 0), 0x80)]:  # the last two: y and -y one apart
        for z in ((1, 0), (3, 4)):
            z2 = M.f2_sqr(z)
            pt = raw_g2(M.f2_mul((9, 2), z2), M.f2_mul(y, M.f2_mul(z2, z)), z)
            got = ffi.host_g2_serialize_compressed(pt)
            assert got == g2_bytes_affine(((9, 2), y)) and got[63] & 0x80 == flag, (y, z)
    # refusals: a null pointer, a coordinate that is not reduced
    bad = G2.point(3).copy()
    bad[0:4] = np.array(O.int_to_limbs(Q), dtype=np.uint64)
    out = (C.c_uint8 * 64)()
    assert ffi.lib().jolt_host_g2_serialize_compressed(bad.ctypes.data_as(C.c_void_p), out) == 1
    assert ffi.lib().jolt_host_g2_serialize_compressed(None, out) == 1


def test_gt_byte_form_is_its_restatement():
    values = [PM.gt_to_abi(PM.ONE)]
    for a, b in [(1, 1), (2, 3), (O.R_MOD - 1, 5)]:
        values.append(ffi.host_final_exponentiation(ffi.host_miller_loop(G1.point(a).reshape(1, 12), G2.point(b, rep=2).reshape(1, 24))))
    values.append(ffi.host_miller_loop(G1.point(7).reshape(1, 12), G2.point(9).reshape(1, 24)))  # before the final exponentiation: any Fq12 value has a form
    for v in values:
        got = ffi.host_gt_serialize(v)
        assert got == gt_bytes(v) and len(got) == 384
        # the coefficients come back out of the bytes in jolt_gt_t order
        assert [int.from_bytes(got[32 * k:32 * k + 32], "little") for k in range(12)] == [O.limbs_to_int(np.asarray(v).reshape(12, 4)[k]) * pow(1 << 256, -1, Q) % Q for k in range(12)]
    assert ffi.host_gt_serialize(values[0]) == le32(1) + bytes(352)
    bad = values[1].copy()
    bad[44:48] = np.array(O.int_to_limbs(Q), dtype=np.uint64)
    out = (C.c_uint8 * 384)()
    assert ffi.lib().jolt_host_gt_serialize(bad.ctypes.data_as(C.c_void_p), out) == 1


@pytest.mark.parametrize("engine", ENGINES, ids=["test", "blake2b_legacy", "keccak_sponge", "blake2b_sponge"])
def test_transcript_appends_are_label_with_count_and_the_bytes(engine):
    gt = ffi.host_final_exponentiation(ffi.host_miller_loop(G1.point(3).reshape(1, 12), G2.point(4).reshape(1, 24)))
    elements = [(gt, gt_bytes(gt)), (G1.point(5), O.g1_serialize_compressed(G1.point(5))), (G2.point(6, rep=1), g2_bytes(G2.point(6, rep=1))),
                (G1.point(0), O.g1_serialize_compressed(G1.point(0))), (G2.point(0), g2_bytes(G2.point(0)))]
    assert [len(b) for _, b in elements] == [384, 32, 64, 32, 64]
    mine, replay = ffi.HostTranscript(engine | 77), ffi.HostTranscript(engine | 77)
    for element, data in elements:
        ffi.host_dory_transcript_append(mine, element)
        replay.append_label(b"dory_group", count=len(data))
        replay.append_bytes(data)
        assert mine.state() == replay.state()
        assert np.array_equal(mine.challenge(full_width=True), replay.challenge(full_width=True))
    # a different byte changes what follows
    other = ffi.HostTranscript(engine | 77)
    ffi.host_dory_transcript_append(other, G2.point(7))
    fresh = ffi.HostTranscript(engine | 77)
    ffi.host_dory_transcript_append(fresh, G2.point(-7))
    assert not np.array_equal(other.challenge(full_width=True), fresh.challenge(full_width=True))
    assert ffi.lib().jolt_host_dory_transcript_append_g1(None, G1.point(1).ctypes.data_as(C.c_void_p)) == 1
    assert ffi.lib().jolt_host_dory_transcript_append_gt(mine.h, None) == 1
    for t in (mine, replay, other, fresh):
        t.close()


def test_proof_counts():
    for sigma in range(21):
        assert ffi.host_dory_proof_counts(sigma) == (2 + 6 * sigma, 2 + 3 * sigma, 1 + 3 * sigma, 2 * sigma + 1)
    with pytest.raises(ffi.JoltError):
        ffi.host_dory_proof_counts(31)
    n = C.c_size_t(99)
    assert ffi.lib().jolt_host_dory_proof_counts(C.c_uint32(4), None, C.byref(n), None, None) == 0 and n.value == 14


def test_proof_object_names_the_messages():
    from jolt_amd.dory_proof import DoryProof
    sigma = 2
    n_gt, n_g1, n_g2, n_ch = ffi.host_dory_proof_counts(sigma)
    tag = lambda n, w, base: (np.arange(n, dtype=np.uint64).reshape(n, 1) + np.uint64(base)) * np.ones((1, w), dtype=np.uint64)  # noqa: E731
    p = DoryProof(sigma, tag(n_gt, 48, 100), tag(n_g1, 12, 200), tag(n_g2, 24, 300), tag(n_ch, 4, 400))
    ids = lambda xs: [int(x[0]) for x in xs]  # noqa: E731
    assert ids(p.vmv) == [100, 101, 200]
    assert ids(p.rounds[0][0]) == [102, 103, 104, 105, 201, 300] and ids(p.rounds[0][1]) == [106, 107, 202, 203, 301, 302]
    assert ids(p.rounds[1][0]) == [108, 109, 110, 111, 204, 303] and ids(p.rounds[1][1]) == [112, 113, 205, 206, 304, 305]
    assert ids(p.final) == [207, 306] and [ids(c) for c in p.challenges] == [[400, 401], [402, 403]] and int(p.gamma[0]) == 404
    assert len(p.elements()) == n_gt + n_g1 + n_g2
    with pytest.raises(ValueError):
        DoryProof(3, tag(n_gt, 48, 0), tag(n_g1, 12, 0), tag(n_g2, 24, 0), tag(n_ch, 4, 0))


def test_ffi_binds_every_new_header_symbol():
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "jolt_hip.h")).read(), flags=re.S)
    binding = open(os.path.join(root, "jolt_amd", "ffi.py")).read()
    declared = set(re.findall(r"\bint32_t\s+(jolt_dory_(?:setup_\w+|round_update)|jolt_host_dory_(?:open\w*|proof_counts|transcript_append_\w+)|jolt_host_(?:g2_serialize_compressed|gt_serialize))\s*\(", header))
    assert declared == set(NEW_SYMBOLS)
    for name in NEW_SYMBOLS:
        assert f"lib().{name}(" in binding or f'_call("{name}", ' in binding, name
        assert hasattr(ffi.lib(), name), name
    assert "jolt_dory_transcript_fn" in header and ffi.lib().jolt_abi_version() == 1
    for method in ("dory_setup_create", "dory_round_update", "dory_open"):
        assert callable(getattr(ffi.Context, method))
    from jolt_amd import dory_proof, dory_scheme
    assert callable(dory_proof.prove) and callable(dory_scheme.prove) and dory_proof.DoryProofSetup is ffi.DoryLibSetup


def test_no_fallback_without_a_device():
    """nothing of the opening runs on the host: every entry that touches the device needs a context, and a context needs a gfx950 device"""
    lib, null, z = ffi.lib(), None, C.c_size_t(0)
    one, pt1, pt2 = G1.point(1)[:4].copy(), G1.point(1), G2.point(1)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    handle = C.c_void_p()
    assert lib.jolt_dory_setup_create(null, p(pt1), p(pt2), C.c_size_t(1), p(pt1), p(pt2), C.byref(handle)) == 1 and not handle.value
    assert lib.jolt_dory_setup_tier2(null, null, null, null, null, z, null) == 1
    assert lib.jolt_dory_round_update(null, C.c_int32(0), null, z, null, z, null, z, null, z, z, p(one), p(one)) == 1
    t = ffi.HostTranscript(1)
    assert lib.jolt_host_dory_open(null, null, null, null, null, z, null, null, null, null, C.c_uint32(0), C.c_uint32(0), t.h, null, null, null, null) == 1
    assert lib.jolt_host_dory_open_with_transcript(null, null, null, null, null, z, null, null, null, null, C.c_uint32(0), C.c_uint32(0), null, null, null, null, null, null) == 1
    t.close()
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(ffi.JoltError) as e:
            ffi.Context(0)
        assert e.value.status == 2  # JOLT_ERR_NO_DEVICE: no context, so no setup and no opening
