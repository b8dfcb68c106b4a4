"""The uni-skip round over constraint rows, host side (no GPU): the Lagrange entries, the first-round polynomial, jolt_host_prove_uniskip on every transcript engine, the
derived remainder weights, the per-cycle integer body of the device kernel built for the host, the row object's refusals and jolt_host_prove_batch_ops_on -- against
tests/uniskip_twin.py (Python big integers mod r, the oracle's transcript, hashlib)."""
import json
import os

import numpy as np
import pytest

import oracle_lib as O
import uniskip_twin as TW
from jolt_amd import ffi
from jolt_amd import stages as S
from util import rand_challenge, rand_fr

R = O.R_MOD
DOMAINS = [2, 3, 10, 14]


def points(D, seed):
    """a random element, a 125-bit challenge, a value one past the domain, a domain node"""
    return [TW.challenge_int(rand_fr(1, seed)[0]), TW.challenge_int(rand_challenge(seed + 1)), (TW.centered_start(D) + D) % R, (TW.centered_start(D) + D - 1) % R,
            TW.centered_start(D) % R]


@pytest.mark.parametrize("D", DOMAINS)
def test_centered_lagrange_entries_match_the_big_integer_model(D):
    for k, r in enumerate(points(D, 100 + D)):
        got = ffi.host_centered_lagrange_evals(D, TW.mont([r])[0])
        assert TW.ints(got) == TW.lagrange_evals(D, r), (D, k)
        y = points(D, 200 + D)[k % 3]
        assert TW.challenge_int(ffi.host_centered_lagrange_kernel(D, TW.mont([r])[0], TW.mont([y])[0])) == TW.lagrange_kernel(D, r, y)
    assert sum(TW.lagrange_evals(D, points(D, 7)[0])) % R == 1  # a partition of unity: the model itself


@pytest.mark.parametrize("D", DOMAINS)
def test_interpolate_to_coeffs_matches_the_model_and_the_oracle(D):
    vals = TW.ints(rand_fr(2 * D - 1, 300 + D))
    for start in (TW.centered_start(2 * D - 1), TW.centered_start(D), 0):
        got = TW.ints(ffi.host_interpolate_to_coeffs(start, TW.mont(vals)))
        assert got == TW.interpolate_to_coeffs(start, vals)
        for k, v in enumerate(vals):  # it interpolates
            assert TW.evaluate(got, (start + k) % R) == v
    head = TW.mont(vals[:16])  # (the oracle's from_evals takes at most 16 values)
    assert np.array_equal(ffi.host_interpolate_to_coeffs(0, head), O.univariate_from_evals(head))  # domain_start = 0 is UnivariatePoly::from_evals


def test_interpolate_to_coeffs_reference_vectors():
    """the two interpolate_to_coeffs vectors of the reference's own tests (crates/jolt-poly/src/lagrange.rs:746-762, domain_start 0)"""
    cases = [c for c in json.load(open(os.path.join(os.path.dirname(__file__), "golden", "reference_kats.json")))["cases"] if c["kind"] == "interpolate_to_coeffs_prefix"]
    assert len(cases) == 2
    for case in cases:
        for got in (TW.ints(ffi.host_interpolate_to_coeffs(0, TW.mont(case["vals"]))), TW.interpolate_to_coeffs(0, [v % R for v in case["vals"]])):
            k = len(case["coeffs"])
            assert got[:k] == [c % R for c in case["coeffs"]] and not any(got[k:]), case["source"]


@pytest.mark.parametrize("D", DOMAINS)
def test_first_round_polynomial(D):
    tau_high = TW.challenge_int(rand_challenge(400 + D))
    t1 = TW.ints(rand_fr(2 * D - 1, 410 + D))
    got = TW.ints(ffi.host_uniskip_first_round_poly(D, TW.mont([tau_high])[0], TW.mont(t1)))
    assert len(got) == 3 * D - 2 and got == TW.first_round_poly(D, tau_high, t1)  # degree <= 3D - 3
    lo = TW.centered_start(2 * D - 1)
    want = sum(TW.lagrange_kernel(D, tau_high, y % R) * t1[y - lo] for y in range(TW.centered_start(D), TW.centered_start(D) + D)) % R
    assert TW.domain_sum(D, got) == want  # sum over the domain of s1 = sum_y LK(tau_high, y) t1(y)


def _uniskip_case(D, seed):
    tau_high = TW.challenge_int(rand_challenge(seed))
    t1 = TW.ints(rand_fr(2 * D - 1, seed + 1))
    coeffs = TW.first_round_poly(D, tau_high, t1)
    return coeffs, TW.domain_sum(D, coeffs)


ENGINES = [("test", 77, 77), ("blake2b_legacy", ffi.TRANSCRIPT_BLAKE2B | 78, O.TRANSCRIPT_BLAKE2B | 78), ("keccak", ffi.TRANSCRIPT_KECCAK | 79, O.TRANSCRIPT_KECCAK | 79),
           ("blake2b_sponge", ffi.TRANSCRIPT_BLAKE2B_SPONGE | 80, O.TRANSCRIPT_BLAKE2B_SPONGE | 80)]


@pytest.mark.parametrize("name,label,oracle_label", ENGINES, ids=[e[0] for e in ENGINES])
@pytest.mark.parametrize("D", [3, 10])
def test_prove_uniskip_on_every_engine_against_the_oracle_transcript(name, label, oracle_label, D):
    coeffs, claim = _uniskip_case(D, 500 + D)
    tr = ffi.HostTranscript(label)
    r0, out = ffi.host_prove_uniskip(tr, TW.mont(coeffs), D, TW.mont([claim])[0])
    otr = O.MockTranscript(oracle_label)
    want_r0, want_out = TW.prove_uniskip(otr, coeffs, D, claim)
    assert np.array_equal(r0, want_r0) and TW.challenge_int(out) == want_out
    assert tr.state() == otr.state()                                    # every absorbed byte, the claim absorb included
    assert np.array_equal(tr.challenge(), otr.challenge())              # and what is drawn next (the batch coefficient of the remainder)
    tr.close()


@pytest.mark.parametrize("D", [2, 10])
def test_prove_uniskip_bytes_against_hashlib(D):
    coeffs, claim = _uniskip_case(D, 600 + D)
    tr = ffi.HostTranscript(ffi.TRANSCRIPT_BLAKE2B | 31)
    r0, out = ffi.host_prove_uniskip(tr, TW.mont(coeffs), D, TW.mont([claim])[0])
    htr = TW.HashlibBlake2bTranscript(b"jolt-amd/31")
    want_r0, want_out = TW.prove_uniskip(htr, coeffs, D, claim)
    assert np.array_equal(r0, want_r0) and TW.challenge_int(out) == want_out and tr.state() == htr.state()
    # the absorbed payloads, spelled out: LabelWithCount("uniskip_poly", n), ALL n coefficients, Label("opening_claim"), the claim
    n = len(coeffs)
    assert htr.log[0] == b"uniskip_poly".ljust(24, b"\0") + n.to_bytes(8, "big") and len(htr.log) == n + 3
    assert htr.log[1:n + 1] == [c.to_bytes(32, "big") for c in coeffs]
    assert htr.log[n + 1] == b"opening_claim".ljust(32, b"\0") and htr.log[n + 2] == want_out.to_bytes(32, "big")
    tr.close()


def test_prove_uniskip_refusals():
    D = 3
    coeffs, claim = _uniskip_case(D, 700)
    tr = ffi.HostTranscript(5)
    before = tr.state()
    with pytest.raises(ffi.JoltError) as e:
        ffi.host_prove_uniskip(tr, TW.mont(coeffs), D, TW.mont([(claim + 1) % R])[0])
    assert e.value.status == 8  # JOLT_ERR_ROUND_CHECK
    with pytest.raises(ffi.JoltError) as e:
        ffi.host_prove_uniskip(tr, TW.mont(coeffs + [1]), D, TW.mont([claim])[0])  # degree 3D - 2
    assert e.value.status == 6
    assert tr.state() == before  # nothing was absorbed
    tr.close()


SHAPES = [(2, 10, None), (1, 3, None), (2, 2, 1), (2, 10, 7)]


def _rows(system, zero_on_domain=True):
    return ffi.R1csRows(system["streams"], system["domain_size"], system["n_inputs"], zero_on_domain)


@pytest.mark.parametrize("S_,D,second", SHAPES)
def test_derived_remainder_weights(S_, D, second):
    system = S.random_row_system(S_, D, second_stream_rows=second)
    rows = _rows(system)
    for seed in (1, 2):
        r0, tau_high = TW.challenge_int(rand_challenge(800 + seed)), TW.challenge_int(rand_challenge(810 + seed))
        fa, fb, scale = rows.remainder_weights(TW.mont([r0])[0], TW.mont([tau_high])[0])
        want_a, want_b, want_scale = TW.remainder_weights(system, r0, tau_high)
        for s in range(S_):
            assert TW.ints(fa[s]) == want_a[s] and TW.ints(fb[s]) == want_b[s]
        assert TW.challenge_int(scale) == want_scale
    ext = rows.extension()
    for p in range(2 * D - 1):
        assert [int(v) for v in ext[p]] == [TW.extension_int(D, i, TW.centered_start(2 * D - 1) + p) for i in range(D)]


EXTREMES = {"u64": [0, 1, 2**64 - 1], "i64": [0, 1, 2**63 - 1, -(2**63 - 1)], "i128": [0, 1, 2**127 - 1, -(2**127 - 1), 2**64 - 1]}


def extreme_system():
    """two streams over D = 4, the second shorter; coefficients of both signs, a 2^64 constant; A rows over small columns so that the range contract holds at the extremes"""
    kinds = ["u64", "u64", "u64", "i64", "i128", "i128", "u64"]
    s0 = [([(0, 1)], 0, [(2, 1), (4, -1)], 0), ([(0, 1), (1, -1)], 3, [(4, 1), (2, -1), (3, 1)], -(1 << 64)), ([(1, -2)], -1, [(5, -3), (3, 5)], (1 << 100) + 7),
          ([(6, 1)], 0, [(2, -1)], 1 << 64)]
    s1 = [([(1, 1)], 0, [(3, -7), (5, 1)], -5), ([(0, -1)], 2, [(4, 1), (5, 1)], 0)]
    return dict(streams=[s0, s1], kinds=kinds, n_inputs=len(kinds), domain_size=4)


def extreme_cycles(system, n, seed):
    rng = np.random.default_rng(seed)
    cols = []
    for c, kind in enumerate(system["kinds"]):
        pool = [0, 1] if c in (0, 1) else EXTREMES[kind]  # the A-side flag columns stay flags
        cols.append([pool[int(k)] for k in rng.integers(0, len(pool), size=n)])
    return cols


def test_host_cycle_body_against_big_integers():
    system = extreme_system()
    rows = _rows(system, zero_on_domain=False)
    cols = extreme_cycles(system, 48, 5)
    D = 4
    for t in range(48):
        values = [cols[c][t] for c in range(system["n_inputs"])]
        for s in range(2):
            for p in range(2 * D - 1):
                az, bz = TW.node_values_int(system, cols, s, TW.centered_start(2 * D - 1) + p, t)
                assert abs(az) < 2**127 and abs(bz) < 2**191 and abs(az * bz) < 2**254  # the range contract
                assert rows.host_cycle(values, system["kinds"], s, p) == (az, bz, az * bz), (t, s, p)


def test_rows_create_refusals():
    ok = [([(0, 1)], 0, [(1, 1)], 0)]
    ffi.R1csRows([ok * 2], 2, 2).destroy()
    cases = [
        ("column out of range", dict(streams=[[([(2, 1)], 0, [(1, 1)], 0)] * 2], domain_size=2, n_inputs=2)),
        ("B column out of range", dict(streams=[[([(0, 1)], 0, [(5, 1)], 0)] * 2], domain_size=2, n_inputs=2)),
        ("INT64_MIN coefficient", dict(streams=[[([(0, -2**63)], 0, [(1, 1)], 0)] * 2], domain_size=2, n_inputs=2)),
        ("INT64_MIN B coefficient", dict(streams=[[([(0, 1)], 0, [(1, -2**63)], 0)] * 2], domain_size=2, n_inputs=2)),
        ("more rows than D", dict(streams=[ok * 3], domain_size=2, n_inputs=2)),
        ("more rows than D in the second stream", dict(streams=[ok * 2, ok * 3], domain_size=2, n_inputs=2)),
        ("D below the range", dict(streams=[ok], domain_size=1, n_inputs=2)),
        ("D above the range", dict(streams=[ok * 17], domain_size=17, n_inputs=2)),
    ]
    for what, kw in cases:
        with pytest.raises(ffi.JoltError) as e:
            ffi.R1csRows(kw["streams"], kw["domain_size"], kw["n_inputs"])
        assert e.value.status == 1, what
    # the extension coefficients of every admitted D have an int64 (the JOLT_ERR_UNSUPPORTED branch of creation is unreachable for D <= 16); what does leave int64 is
    # the FOLDED column form of a system with a 2^64 constant: jolt_r1cs_rows_fold_small refuses it
    big = ffi.R1csRows([ok * 16], 16, 2)
    assert np.abs(big.extension()).max() < 2**62
    with pytest.raises(ffi.JoltError) as e:
        _rows(extreme_system()).fold_small()
    assert e.value.status == 6


def test_fold_small_of_the_bench_system_has_int64_weights():
    _rows(S.random_row_system(2, 10, seed=5, n_free=10, foldable=True)).fold_small()


def test_fold_small_is_the_column_form():
    system = S.random_row_system(2, 3, foldable=True)
    h = _rows(system)
    wa, wb = h.fold_small()
    nodes = TW.evaluated_nodes(3, True)
    assert wa.shape == (len(nodes), 2, 1 + system["n_inputs"])
    for k, p in enumerate(nodes):
        for s in range(2):
            want_a, want_b = [0] * (1 + system["n_inputs"]), [0] * (1 + system["n_inputs"])
            for i, (at, a0, bt, b0) in enumerate(system["streams"][s]):
                l = TW.extension_int(3, i, TW.centered_start(5) + p)
                want_a[0] += l * a0
                want_b[0] += l * b0
                for c, a in at:
                    want_a[1 + c] += l * a
                for c, a in bt:
                    want_b[1 + c] += l * a
            assert [int(v) for v in wa[k, s]] == want_a and [int(v) for v in wb[k, s]] == want_b


def test_prove_batch_ops_on_a_fresh_transcript_is_prove_batch_ops():
    n = 4
    tabs = [rand_fr(1 << n, 900 + k) for k in range(3)]
    one = O.to_mont([1])[0]
    terms = [(one, [0, 1]), (rand_fr(1, 910)[0], [0, 2])]
    for label in (9, ffi.TRANSCRIPT_BLAKE2B | 9):
        a, b = ffi.stage_host_expr(tabs, terms, 2), ffi.stage_host_expr(tabs, terms, 2)
        claim = O.Member.expr(tabs, terms, 2).input_claim()
        want = ffi.prove_batch_ops([a], [claim], [one], [0], n, 2, label=label)
        tr = ffi.HostTranscript(label)
        got = ffi.prove_batch_ops_on([b], [claim], [one], [0], n, 2, tr)
        for key in ("polys", "challenges", "member_claims", "final_claim"):
            assert np.array_equal(got[key], want[key]), key
        oracle = O.prove_batch([O.Member.expr(tabs, terms, 2)], [claim], [one], [0], n, 2, label=label)
        assert np.array_equal(got["polys"], oracle["polys"]) and np.array_equal(got["final_claim"], oracle["final_claim"])
        # the transcript went on from where the caller left it: absorbing first changes every challenge
        tr2 = ffi.HostTranscript(label)
        tr2.append(one)
        c = ffi.stage_host_expr(tabs, terms, 2)
        other = ffi.prove_batch_ops_on([c], [claim], [one], [0], n, 2, tr2)
        assert not np.array_equal(other["challenges"], want["challenges"])
        for h in (a, b, c):
            h.destroy()
        tr.close()
        tr2.close()


def test_generator_emits_a_satisfied_trace_deterministically():
    p = dict(rows_shape=(2, 10))
    b0, again, b1 = S.satisfied_rows_block(p, 5, 0), S.satisfied_rows_block(p, 5, 0), S.satisfied_rows_block(p, 5, 1)
    system = b0["system"]
    assert any(r[3] == -(1 << 64) for r in system["streams"][0]) and set(system["kinds"]) == {"u64", "i64", "i128"}
    assert all(np.array_equal(x, y) for x, y in zip(b0["cols"], again["cols"])) and not all(np.array_equal(x, y) for x, y in zip(b0["cols"], b1["cols"]))
    guarded = 0
    for s in range(2):
        for i in range(len(system["streams"][s])):
            for t in range(32):
                a, b = TW.row_values_int(system, b0["ints"], s, i, t)
                assert a * b == 0
                guarded += a != 0
    assert guarded > 50  # not trivially: many rows hold through left = right
    broken = S.satisfied_rows_block(p, 5, 0, broken_cycle=9)
    a, b = TW.row_values_int(system, broken["ints"], 0, 0, 9)
    assert a * b != 0
