"""GPU checks of HyperKZG verification (hyperkzg_verify.hip): the verifier's setup, jolt_host_hyperkzg_verify / _with_transcript on the device's openings, the oracle's
and hand-made ones, every rejection with its code, the refusals, stage 8's batch framing (jolt_host_hyperkzg_prove_batch / _verify_batch) against the same framing
composed from the existing entries, and DeviceWorkload.verify.  The verifier's decision is held to e(L, g2) = e(R, beta g2) itself: no test here knows beta's use
other than through the verifier setup."""
import numpy as np
import pytest

import oracle_lib as O
from dory_groups import R, fr_int, fr_ints
from jolt_amd import dory_setup, ffi
from jolt_amd.workload import DeviceWorkload
from kzg_check import same_point
from util import rand_challenge, rand_fr

pytestmark = pytest.mark.gpu

LABELS = {"test": ffi.TRANSCRIPT_TEST | 41, "blake2b": ffi.TRANSCRIPT_BLAKE2B | 42, "keccak": ffi.TRANSCRIPT_KECCAK | 43}
NOT_CANONICAL = np.array(O.int_to_limbs(R), dtype=np.uint64)


@pytest.fixture(scope="module")
def ctx():
    c = ffi.Context(0)
    yield c
    c.close()


def ints(a):
    return [int(x) for x in O.from_mont(np.asarray(a, dtype=np.uint64).reshape(-1, 4))]


def multilinear_eval(evals, point):
    """the claim of an opening: the oracle's last fold (two entries) closed by point[0], in Python integers"""
    last = ints(O.hyperkzg_fold_polynomials(evals, point)[-1])
    x0 = ints(point[0])[0]
    return fr_int(last[0] + x0 * (last[1] - last[0]))


_CASES = {}


def case(ctx, ell):
    """one setup, polynomial and point per ell, shared by the tests: (beta, host SRS, device SRS, verifier setup, evals, table, point, commitment, claim)"""
    if ell not in _CASES:
        n = 1 << ell
        beta = rand_fr(1, 9000 + ell)[0]
        host_srs = O.srs_setup_from_secret(beta, n + 1)
        srs = ctx.srs_upload(host_srs)
        vs = ctx.hyperkzg_verifier_setup(O.g1_generator(), dory_setup.g2_generator(), beta=beta)
        evals, point = rand_fr(n, 9100 + ell), np.stack([rand_challenge(9200 + 16 * ell + k) for k in range(ell)])
        tab = ctx.upload(evals)
        _CASES[ell] = dict(ell=ell, beta=beta, host_srs=host_srs, srs=srs, vs=vs, evals=evals, tab=tab, point=point, commitment=ctx.hyperkzg_commit(srs, tab),
                           y=multilinear_eval(evals, point), proofs={})
    return _CASES[ell]


def opening(ctx, c, label):
    if label not in c["proofs"]:
        c["proofs"][label] = ctx.hyperkzg_open(c["srs"], c["tab"], c["point"], label=label)
    return c["proofs"][label]


class Replay:
    """a verifier's callback: over a HostTranscript (absorbing as the opening's documentation says: compressed points, field elements) or over recorded challenges"""

    def __init__(self, transcript=None, recorded=None):
        self.t, self.recorded, self.calls, self.drawn = transcript, recorded, [], []

    def __call__(self, phase, points, values):
        self.calls.append((phase, len(points), len(values)))
        if self.recorded is not None:
            return self.recorded[phase]
        for p in points:
            self.t.append_bytes(ffi.host_g1_serialize_compressed(p))
        if len(values):
            self.t.append(values)
        self.drawn.append(self.t.challenge())
        return self.drawn[-1]


def verify(ctx, c, proof, **kw):
    args = dict(commitments=c["commitment"], point=c["point"], eval_=c["y"])
    args.update({k: kw.pop(k) for k in list(kw) if k in ("commitments", "point", "eval_", "vs")})
    return ctx.hyperkzg_verify(args.pop("vs", c["vs"]), args["commitments"], args["point"], args["eval_"], proof, **kw)


def other_point(p):
    """another point of the curve: p + g1"""
    return O.g1_add(p, O.g1_generator())


def plus_one(x):
    return fr_int(ints(x)[0] + 1)


# ------------------------------------------------------------------------------------------------------------------ the setup
def test_setup_round_trips_and_refuses(ctx):
    beta = rand_fr(1, 9300)[0]
    g1, g2 = O.g1_generator(), dory_setup.g2_generator()
    vs = ctx.hyperkzg_verifier_setup(g1, g2, beta=beta)
    p1, p2, bp2 = vs.points()
    want = ffi.host_g2_scalar_mul(g2, beta)
    assert np.array_equal(p1, g1) and np.array_equal(p2, g2) and np.array_equal(bp2, want)
    assert ffi.host_g2_is_on_curve(bp2) and not ffi.host_g2_eq(bp2, g2)
    vs2 = ctx.hyperkzg_verifier_setup(g1, g2, beta_g2=want)  # the three points as a deployment holds them
    assert all(np.array_equal(a, b) for a, b in zip(vs2.points(), (g1, g2, want)))
    vs.close()
    vs2.close()
    off_twist, not_canonical = g2.copy(), g2.copy()
    off_twist[8] += np.uint64(1)  # y.c0
    not_canonical[0:4] = np.array(O.int_to_limbs(dory_setup.Q), dtype=np.uint64)  # x.c0 = q
    assert not ffi.host_g2_is_on_curve(off_twist)
    g2_identity = np.array(dory_setup._fq_mont(1) + dory_setup._fq_mont(0) + dory_setup._fq_mont(1) + dory_setup._fq_mont(0) + [0] * 8, dtype=np.uint64)
    bad_g1 = g1.copy()
    bad_g1[4] += np.uint64(1)
    for kw in [dict(g1=g1, g2=off_twist, beta_g2=want), dict(g1=g1, g2=g2, beta_g2=off_twist), dict(g1=g1, g2=not_canonical, beta_g2=want), dict(g1=bad_g1, g2=g2, beta_g2=want),
               dict(g1=O.g1_identity(), g2=g2, beta_g2=want), dict(g1=g1, g2=g2_identity, beta_g2=want), dict(g1=g1, g2=g2, beta_g2=g2_identity),
               dict(g1=g1, g2=g2, beta=np.zeros(4, dtype=np.uint64)), dict(g1=g1, g2=g2, beta=NOT_CANONICAL), dict(g1=g1, g2=off_twist, beta=beta)]:
        with pytest.raises(ffi.JoltError) as e:
            ctx.hyperkzg_verifier_setup(**kw)
        assert e.value.status == ffi.ERR_INVALID_ARG, list(kw)


# ------------------------------------------------------------------------------------------------------------------ accepted proofs
@pytest.mark.parametrize("engine", list(LABELS))
@pytest.mark.parametrize("ell", [1, 2, 3, 6, 10])
def test_device_openings_are_accepted_and_the_replay_draws_the_openings_challenges(ctx, ell, engine):
    c, label = case(ctx, ell), LABELS[engine]
    proof = opening(ctx, c, label)
    t = ffi.HostTranscript(label)
    assert verify(ctx, c, proof, transcript=t) == dict(accepted=True, failed_check=0, failed_level=0)
    t2 = ffi.HostTranscript(label)
    replay = Replay(t2)
    assert verify(ctx, c, proof, callback=replay) == dict(accepted=True, failed_check=0, failed_level=0)
    # the same three phases with the same elements as the opening's callback sees: ell - 1 points (none at ell = 1), 3 ell values, 3 points
    assert replay.calls == [(0, ell - 1, 0), (1, 0, 3 * ell), (2, 3, 0)]
    assert np.array_equal(np.stack(replay.drawn), proof["challenges"])
    assert t.state() == t2.state() and np.array_equal(t.challenge(), t2.challenge())
    t.close()
    t2.close()


@pytest.mark.parametrize("ell", [1, 3, 6])
def test_the_oracles_proof_is_accepted(ctx, ell):
    """an independent CPU prover (oracle/hyperkzg.c) on the same inputs, commitment included"""
    c, label = case(ctx, ell), LABELS["test"]
    proof = O.hyperkzg_open(c["host_srs"], c["evals"], c["point"], label=label)
    t = ffi.HostTranscript(label)
    out = verify(ctx, c, proof, transcript=t, commitments=O.kzg_commit(c["evals"], c["host_srs"]))
    assert out == dict(accepted=True, failed_check=0, failed_level=0)
    t.close()


@pytest.mark.parametrize("ell", [1, 3])
def test_the_zero_polynomial_is_accepted(ctx, ell):
    """every point the identity, every value zero: L and R are the identity and both pairs contribute one.  The proof is the device's own opening of the zero table."""
    c, label = case(ctx, ell), LABELS["test"]
    zero = ctx.upload(np.zeros((1 << ell, 4), dtype=np.uint64))
    proof = ctx.hyperkzg_open(c["srs"], zero, c["point"], label=label)
    commitment = ctx.hyperkzg_commit(c["srs"], zero)
    assert all(O.g1_is_identity(p) for p in list(proof["com"]) + list(proof["w"]) + [commitment]) and not proof["v"].any()
    t = ffi.HostTranscript(label)
    out = verify(ctx, c, proof, transcript=t, commitments=commitment, eval_=np.zeros(4, dtype=np.uint64))
    assert out == dict(accepted=True, failed_check=0, failed_level=0)
    t.close()
    zero.free()


def test_combine_70_commitments_inside_the_msm(ctx):
    """verify after combine (scheme.rs:346-352) with C_0 never built: 70 commitments cross one wavefront of MSM terms"""
    c, label, n = case(ctx, 3), LABELS["test"], 70
    polys = [rand_fr(8, 9400 + i) for i in range(n)]
    scalars = rand_fr(n, 9500)
    s_int, p_int = ints(scalars), [ints(p) for p in polys]
    joint = fr_ints([sum(s * p[k] for s, p in zip(s_int, p_int)) % R for k in range(8)])
    commitments = np.stack([O.kzg_commit(p, c["host_srs"]) for p in polys])
    tab = ctx.upload(joint)
    proof = ctx.hyperkzg_open(c["srs"], tab, c["point"], label=label)
    y = multilinear_eval(joint, c["point"])
    t = ffi.HostTranscript(label)
    out = verify(ctx, c, proof, transcript=t, commitments=commitments, commitment_scalars=scalars, eval_=y)
    assert out == dict(accepted=True, failed_check=0, failed_level=0)
    t.close()
    wrong = scalars.copy()
    wrong[37] = plus_one(wrong[37])
    t = ffi.HostTranscript(label)
    out = verify(ctx, c, proof, transcript=t, commitments=commitments, commitment_scalars=wrong, eval_=y)
    assert out == dict(accepted=False, failed_check=2, failed_level=0)
    t.close()
    tab.free()


# ------------------------------------------------------------------------------------------------------------------ rejected proofs
@pytest.mark.parametrize("ell", [1, 3])
def test_folding_failures_name_their_level_and_stop_the_transcript(ctx, ell):
    c, label = case(ctx, ell), LABELS["test"]
    proof = opening(ctx, c, label)
    replay = Replay(recorded=list(proof["challenges"]))
    assert verify(ctx, c, proof, callback=replay, eval_=plus_one(c["y"])) == dict(accepted=False, failed_check=1, failed_level=ell - 1)
    assert replay.calls == [(0, ell - 1, 0)]  # phases 1 and 2 are not run (scheme.rs:231-233)
    for j in range(ell):
        v = proof["v"].copy()
        v[0, j] = plus_one(v[0, j])
        replay = Replay(recorded=list(proof["challenges"]))
        assert verify(ctx, c, dict(proof, v=v), callback=replay) == dict(accepted=False, failed_check=1, failed_level=j)
        assert replay.calls == [(0, ell - 1, 0)]
    # under an engine the transcript stops after r as well: the state is the one after the level commitments and one challenge
    t, want = ffi.HostTranscript(label), ffi.HostTranscript(label)
    assert verify(ctx, c, proof, transcript=t, eval_=plus_one(c["y"]))["failed_check"] == 1
    Replay(want)(0, proof["com"], np.zeros((0, 4), dtype=np.uint64))
    assert t.state() == want.state()
    t.close()
    want.close()


def test_pairing_failures_under_recorded_challenges(ctx):
    """the callback replays the opening's challenges, so a tampered point moves no challenge: each of these reaches the pairing check and fails it"""
    c, label = case(ctx, 3), LABELS["test"]
    proof = opening(ctx, c, label)
    recorded = list(proof["challenges"])
    rejected = dict(accepted=False, failed_check=2, failed_level=0)
    assert verify(ctx, c, proof, callback=Replay(recorded=recorded))["accepted"]
    for i in range(2):
        com = proof["com"].copy()
        com[i] = other_point(com[i])
        assert verify(ctx, c, dict(proof, com=com), callback=Replay(recorded=recorded)) == rejected, i
    for k in range(3):
        w = proof["w"].copy()
        w[k] = other_point(w[k])
        assert verify(ctx, c, dict(proof, w=w), callback=Replay(recorded=recorded)) == rejected, k
    assert verify(ctx, c, proof, callback=Replay(recorded=recorded), commitments=other_point(c["commitment"])) == rejected
    v = proof["v"].copy()
    v[2, 0] = plus_one(v[2, 0])  # the one evaluation no folding equation reads
    assert verify(ctx, c, dict(proof, v=v), callback=Replay(recorded=recorded)) == rejected
    other = ctx.hyperkzg_verifier_setup(O.g1_generator(), dory_setup.g2_generator(), beta=plus_one(c["beta"]))
    assert verify(ctx, c, proof, callback=Replay(recorded=recorded), vs=other) == rejected
    other.close()


def test_malformed_input_is_a_status_and_leaves_the_transcript_alone(ctx):
    c, label = case(ctx, 3), LABELS["keccak"]
    proof = opening(ctx, c, label)
    t = ffi.HostTranscript(label)
    before = t.state()
    off_curve = proof["w"].copy()
    off_curve[1, 4] += np.uint64(1)
    bad_v = proof["v"].copy()
    bad_v[1, 2] = NOT_CANONICAL
    bad_com = proof["com"].copy()
    bad_com[0, 0:4] = np.array(O.int_to_limbs(dory_setup.Q), dtype=np.uint64)
    cases = [(dict(proof=dict(proof, w=off_curve)), ffi.ERR_INVALID_ARG), (dict(proof=dict(proof, v=bad_v)), ffi.ERR_INVALID_ARG),
             (dict(proof=dict(proof, com=bad_com)), ffi.ERR_INVALID_ARG), (dict(eval_=NOT_CANONICAL), ffi.ERR_INVALID_ARG),
             (dict(commitment_scalars=NOT_CANONICAL.reshape(1, 4)), ffi.ERR_INVALID_ARG),
             (dict(point=np.zeros((0, 4), dtype=np.uint64), proof=dict(com=proof["com"][:0], w=proof["w"], v=proof["v"][:, :0])), ffi.ERR_EMPTY_POINT)]
    for kw, status in cases:
        kw = dict(kw)
        with pytest.raises(ffi.JoltError) as e:
            verify(ctx, c, kw.pop("proof", proof), transcript=t, **kw)
        assert e.value.status == status, list(kw)
        assert t.state() == before
    # a setup of another context
    other_ctx = ffi.Context(0)
    foreign = other_ctx.hyperkzg_verifier_setup(O.g1_generator(), dory_setup.g2_generator(), beta=c["beta"])
    with pytest.raises(ffi.JoltError) as e:
        verify(ctx, c, proof, transcript=t, vs=foreign)
    assert e.value.status == ffi.ERR_INVALID_ARG and t.state() == before
    foreign.close()
    other_ctx.close()
    t.close()


# ------------------------------------------------------------------------------------------------------------------ the batch framing
def grid(ctx, log_k, log_t, seed, onehot=(2, 3), n_dense=2):
    K, T = 1 << log_k, 1 << log_t
    rng = np.random.default_rng(seed)
    beta = rand_fr(1, seed + 1)[0]
    srs = ctx.srs_setup_from_secret(beta, K * T, O.g1_generator())
    idx = [rng.integers(0, K, size=(n, T), dtype=np.uint8) for n in onehot]
    if idx:
        idx[0][0, rng.random(T) < 0.3] = 0xFF  # cold cycles in one column
    sources = [ctx.onehot(i, K) for i in idx]
    dense = [ctx.from_u64(rng.integers(0, 2**64, size=T, dtype=np.uint64)) for _ in range(n_dense)]
    point = rand_fr(log_k + log_t, seed + 2)
    commitments = [p for s in sources for p in ctx.grid_commit_onehot(srs, s)] + [ctx.hyperkzg_commit(srs, d) for d in dense]
    return dict(log_k=log_k, log_t=log_t, beta=beta, srs=srs, sources=sources, dense=dense, point=point, n_onehot=sum(onehot), commitments=np.stack(commitments),
                claims=ctx.grid_evaluate_columns(sources, dense, log_k, point), vs=ctx.hyperkzg_verifier_setup(O.g1_generator(), dory_setup.g2_generator(), beta=beta))


def composed(ctx, g, claims, transcript, hint, levels):
    """the framing from the existing entries: statement absorb, joint polynomial under gamma's powers, the grid opening through a callback on the same transcript,
    the closing claim"""
    powers = ffi.host_opening_statement_absorb(transcript, claims)
    osc, dsc = powers[:g["n_onehot"]], powers[g["n_onehot"]:]
    joint = ctx.grid_joint_polynomial(g["sources"], osc, g["dense"], dsc, g["log_k"])
    if not levels:
        proof = ctx.hyperkzg_open_with_transcript(g["srs"], joint, g["point"], lambda pts: [transcript.append_bytes(ffi.host_g1_serialize_compressed(p)) for p in pts],
                                                  transcript.append, transcript.challenge)
    else:
        proof = ctx.hyperkzg_open_grid(g["srs"], joint, g["point"], hint, levels, osc, g["dense"], dsc, callback=Replay(transcript))
    joint.free()
    joint_eval = fr_int(sum(a * b for a, b in zip(ints(powers), ints(claims))))
    ffi.host_opening_claim_absorb(transcript, g["point"], joint_eval)
    return proof, joint_eval


@pytest.mark.parametrize("levels", [0, 2])
@pytest.mark.parametrize("log_k,log_t", [(2, 3), (4, 6)])
def test_batch_framing_is_the_composition_of_the_existing_entries(ctx, log_k, log_t, levels):
    g, label = grid(ctx, log_k, log_t, 9600 + 10 * log_k + levels), LABELS["blake2b"]
    sources = g["sources"]
    t1, t2, t3 = (ffi.HostTranscript(label) for _ in range(3))
    hint1 = ctx.grid_hint(g["srs"], sources, levels, background=False) if levels else None
    got = ctx.hyperkzg_prove_batch(g["srs"], sources, g["dense"], log_k, g["claims"], g["point"], t1, hint=hint1, levels=levels)
    hint2 = ctx.grid_hint(g["srs"], sources, levels, background=False) if levels else None
    want, joint_eval = composed(ctx, g, g["claims"], t2, hint2, levels)
    ell = log_k + log_t
    assert np.array_equal(got["v"], want["v"]) and np.array_equal(got["challenges"], want["challenges"]) and np.array_equal(got["joint_eval"], joint_eval)
    assert all(same_point(got["com"][i], want["com"][i]) for i in range(ell - 1)) and all(same_point(got["w"][k], want["w"][k]) for k in range(3))
    out = ctx.hyperkzg_verify_batch(g["vs"], g["commitments"], g["claims"], g["point"], got, t3)
    assert (out["accepted"], out["failed_check"], out["failed_level"]) == (True, 0, 0) and np.array_equal(out["joint_eval"], joint_eval)
    assert t1.state() == t2.state() == t3.state()
    # a changed evaluation: the prover refuses the statement, the verifier rejects the proof and absorbs no closing claim
    claims = g["claims"].copy()
    claims[1] = plus_one(claims[1])
    t4, t5 = ffi.HostTranscript(label), ffi.HostTranscript(label)
    hint3 = ctx.grid_hint(g["srs"], sources, levels, background=False) if levels else None
    with pytest.raises(ffi.JoltError) as e:
        ctx.hyperkzg_prove_batch(g["srs"], sources, g["dense"], log_k, claims, g["point"], t4, hint=hint3, levels=levels)
    assert e.value.status == ffi.ERR_ROUND_CHECK
    before = t5.clone()
    out = ctx.hyperkzg_verify_batch(g["vs"], g["commitments"], claims, g["point"], got, t5)
    # the changed statement moves gamma and with it r: the proof's evaluations are at another r, so the FIRST folding equation already fails
    assert (out["accepted"], out["failed_check"], out["failed_level"]) == (False, 1, 0)
    # what each side absorbed, redone on the clone taken before: the refusing prover the statement alone (no level commitment), the verifier the statement, the level
    # commitments and r -- and no closing claim after them
    ffi.host_opening_statement_absorb(before, claims)
    assert t4.state() == before.state()
    Replay(before)(0, got["com"], np.zeros((0, 4), dtype=np.uint64))
    assert t5.state() == before.state()
    if levels:  # a hint of another shape is refused before the statement is absorbed
        narrow, t6 = ctx.grid_hint(g["srs"], sources[:1], levels, background=False), ffi.HostTranscript(label)
        fresh = t6.state()
        with pytest.raises(ffi.JoltError) as e:
            ctx.hyperkzg_prove_batch(g["srs"], sources, g["dense"], log_k, g["claims"], g["point"], t6, hint=narrow, levels=levels)
        assert e.value.status == ffi.ERR_INVALID_ARG and t6.state() == fresh
        narrow.free()
        t6.close()
    for h in (hint1, hint2, hint3):
        if h is not None:
            h.free()
    for t in (t1, t2, t3, t4, t5, before):
        t.close()


def test_a_batch_of_one_claim(ctx):
    g, label = grid(ctx, 2, 3, 9700, onehot=(), n_dense=1), LABELS["test"]
    t1, t2 = ffi.HostTranscript(label), ffi.HostTranscript(label)
    got = ctx.hyperkzg_prove_batch(g["srs"], [], g["dense"], 2, g["claims"], g["point"], t1)
    assert np.array_equal(got["joint_eval"], g["claims"][0])  # gamma^0 = 1
    out = ctx.hyperkzg_verify_batch(g["vs"], g["commitments"], g["claims"], g["point"], got, t2)
    assert out["accepted"] and t1.state() == t2.state()
    t1.close()
    t2.close()


# ------------------------------------------------------------------------------------------------------------------ the workload
def test_the_workload_verifies_its_own_step(ctx):
    w = DeviceWorkload(ctx, 6, seed=9800, pcs="grid")
    label = LABELS["blake2b"]
    commit_out = w.commit()
    open_out = w.open(label)
    assert w.verify(commit_out, open_out, label) is True
    assert w.verify_result["failed_check"] == 0 and len(w.verify_result["transcript_state"]) == 32
    swapped = dict(commit_out, onehot=commit_out["onehot"].copy())
    swapped["onehot"][0] = commit_out["onehot"][1]  # one commitment swapped for another column's
    assert w.verify(swapped, open_out, label) is False and w.verify_result["failed_check"] == 2
    claims = w.evaluate_columns()
    assert w.verify(commit_out, open_out, label, evaluations=claims) is True
    claims[3] = plus_one(claims[3])
    assert w.verify(commit_out, open_out, label, evaluations=claims) is False and w.verify_result["failed_check"] == 1
    assert w.verify(commit_out, open_out, LABELS["keccak"]) is False
    w.close()


def test_the_extended_workload_verifies_its_own_step(ctx):
    w = DeviceWorkload(ctx, 8, seed=9900, pcs="grid", extended=True)
    out = w.step(label=LABELS["test"])
    assert w.verify(out["commit"], out["open"], LABELS["test"]) is True
    w.close()
