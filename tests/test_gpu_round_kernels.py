"""GPU parity above the tail threshold: the dense round kernels group_enqueue (jolt_amd/csrc/capi.hip) picks at the PRODUCTION sizes -- k_round_evals_group in its
(order, skip, fused) forms, k_split_eq_product<fused>, the rows-major uniform kernel, and the hand-over to separate-bind-plus-tail -- against the CPU oracle, bit for
bit, on a default context with nothing set in the environment.  Every case names the path it means to reach and proves it from the context's launch counts
(ffi.Context.round_path_stats): a case that silently slid under a threshold fails instead of passing on the tail kernel.

The switches (defaults of ctx.hpp): an expression member with at most TAIL = 16384 pairs left runs the tail kernel; a pending bind is fused into the round kernel
when the member is LowToHigh, its unbound length / 4 exceeds TAIL, every table is mentioned and muls_per_pair <= 2 * tables; the uniform member goes rows-major at
65536 pairs when V > 1.  So n_vars 16 is: round 0 unfused group, then tail; n_vars 18: round 0 unfused, rounds 1 and 2 fused where the rule allows, round 3 the
hand-over to a separate bind and the tail kernel.  With two or more product groups at 18 the items exceed the default grid's threads (round_grid) and lanes take a
second grid-stride pass across a group boundary.

muls_per_pair (jolt_member_create_lc): (factors - 1) * NE per product group plus 2 per LC entry whose coefficient is not one; NE = degree + 1, or degree with skip-one."""
import numpy as np
import pytest

import oracle_lib as O
import test_gpu_sumcheck as S
from jolt_amd import ffi
from util import rand_challenge, rand_fr

pytestmark = pytest.mark.gpu

L2H, H2L = ffi.ORDER_LOW_TO_HIGH, ffi.ORDER_HIGH_TO_LOW
TAIL = 16384            # ctx.hpp tail_pairs
ROWS_MAJOR = 1 << 16    # ctx.hpp uniform_rows_pairs


@pytest.fixture(scope="module")
def ctx():
    c = ffi.Context(0)
    yield c
    c.close()


def one():
    return S.one()


def fmul(a, b):
    return O.fr_mul(np.asarray(a).reshape(1, 4), np.asarray(b).reshape(1, 4))[0]


def no_launches():
    return {"tail": 0, "group": {(o, s, f): 0 for o in (0, 1) for s in (False, True) for f in (False, True)}, "small": 0, "split_eq_product": (0, 0),
            "uniform_items": 0, "uniform_rows": 0, "lazy": 0, "bind": (0, 0)}


def expected_path(kind, n_vars, rnd, order=L2H, skip=False, fusable=False, V=1):
    """The launches of round `rnd` of ONE member proved alone, from the rule in the module docstring (not from the code under test)."""
    e = no_launches()
    unbound = 1 << (n_vars - rnd + 1)  # length the pending bind halves (rnd >= 1)
    half = 1 << (n_vars - rnd - 1)     # pairs the round sums run over
    fused = rnd >= 1 and fusable and order == L2H and unbound // 4 > TAIL
    if rnd >= 1 and not fused:
        e["bind"] = (1, 0) if order == L2H else (0, 1)
    if kind == "expr":
        if half <= TAIL:
            assert not fused  # the rule never fuses into a tail round
            e["tail"] = 1
        else:
            e["group"][(order, skip, fused)] = 1
    elif kind == "product":
        e["split_eq_product"] = (0, 1) if fused else (1, 0)
    elif kind == "uniform":
        e["uniform_rows" if half >= ROWS_MAJOR and V > 1 else "uniform_items"] = 1
    return e


class Traced:
    """A device member whose prove_round records the launch counts of that round alone."""

    def __init__(self, ctx, dev):
        self._ctx, self._dev, self.rounds = ctx, dev, []

    def __getattr__(self, name):
        return getattr(self._dev, name)

    def prove_round(self, bind=None, want_aux=False):
        self._ctx.round_path_stats(reset=True)
        out = self._dev.prove_round(bind, want_aux=want_aux)
        self.rounds.append(self._ctx.round_path_stats(reset=True))
        return out


def alternating(seed):
    """125-bit challenges in even rounds, full-width ones in odd rounds: the binds fused into rounds 1 and 2 take both branches of bind_pair_rt"""
    return lambda rnd: rand_challenge(seed + rnd) if rnd % 2 == 0 else rand_fr(1, seed + rnd)[0]


def launches(st):
    """the non-zero counts of one round_path_stats result, compactly"""
    names = {0: "LowToHigh", 1: "HighToLow"}
    out = [f"group<{names[o]}{', skip' if s else ''}{', FUSED' if f else ''}> x{n}" for (o, s, f), n in st["group"].items() if n]
    out += [f"{k} x{st[k]}" for k in ("tail", "small", "uniform_items", "uniform_rows", "lazy") if st[k]]
    out += [f"split_eq_product<{'true' if f else 'false'}> x{n}" for f, n in enumerate(st["split_eq_product"]) if n]
    out += [f"bind {names[o]} x{n}" for o, n in enumerate(st["bind"]) if n]
    return " + ".join(out)


def describe(rounds):
    """'r0: ..; r1-2: ..' -- the path of every round, equal neighbours joined (printed before the assertions: pytest -s shows the table of case -> path)"""
    runs = []
    for rnd, st in enumerate(rounds):
        text = launches(st)
        if runs and runs[-1][2] == text:
            runs[-1][1] = rnd
        else:
            runs.append([rnd, rnd, text])
    return "; ".join((f"r{a}" if a == b else f"r{a}-{b}") + f": {t}" for a, b, t in runs)


def check_paths(dev, kind, n_vars, **kw):
    assert len(dev.rounds) == n_vars
    print(f"\nPATH n_vars {n_vars}: {describe(dev.rounds)}")
    for rnd, got in enumerate(dev.rounds):
        assert got == expected_path(kind, n_vars, rnd, **kw), f"round {rnd}: launches {got}"
    return dev.rounds


def run_expr(ctx, dev, orc, n_vars, seed, order, skip, fusable):
    """Lock-step at 18 (LowToHigh, alternating challenge shapes) or 16 (either order; HighToLow with full-width challenges), then the path of every round."""
    dev = Traced(ctx, dev)
    if n_vars == 18:
        assert order == L2H
        S.lockstep(dev, orc, n_vars, seed, challenge=alternating(seed))
    else:
        S.lockstep(dev, orc, n_vars, seed, shifted=(order == L2H))
    rounds = check_paths(dev, "expr", n_vars, order=order, skip=skip, fusable=fusable)
    # what the case is about, spelled out once more: round 0 never on the tail kernel, the fused kernel exactly where it is due
    assert rounds[0]["tail"] == 0 and rounds[0]["group"][(order, skip, False)] == 1
    n_fused = sum(r["group"][(L2H, skip, True)] for r in rounds)
    assert n_fused == (2 if fusable and n_vars == 18 and order == L2H else 0)
    if n_vars == 18 and order == L2H:
        assert rounds[3]["tail"] == 1 and rounds[3]["bind"] == (1, 0)  # the hand-over: separate bind, then the tail kernel
    dev.destroy()


def tables(n_vars, k, seed):
    return [rand_fr(1 << n_vars, seed + 17 * i) for i in range(k)]


# ---- the catalogue shapes above the threshold ----------------------------------------------------------------------------------------------------------------
# fused at 18?  coefficients: term 0 has coefficient one, every further term a random one (2 multiplies per pair each); NE = degree + 1
CATALOGUE_FUSED = {
    "linear": True,                                  # 0 multiplies <= 2 * 1
    "claim_reduction eq*(o1+g o2+..)": False,        # 3 groups * 1 * 3 + 2 * 2 = 13 > 2 * 4
    "triple product": False,                         # 2 * 4 = 8 > 2 * 3
    "hamming booleanity eq*(H^2-H)": False,          # 2 * 4 + 1 * 4 + 2 = 14 > 2 * 2
    "instruction_input": False,                      # 2 * (2 * 4) + 2 = 18 > 2 * 5
    "ra virtualization deg5": False,                 # 4 * 6 = 24 > 2 * 5
    "with constant term": True,                      # 1 * 3 = 3 <= 2 * 2 (the constant term is a factor's constant: no multiply)
}


@pytest.mark.parametrize("name,degree,n_tables,terms_idx", S.CATALOGUE)
@pytest.mark.parametrize("order,n_vars", [(L2H, 18), (H2L, 16)])
def test_catalogue_shapes_above_the_tail_threshold(ctx, name, degree, n_tables, terms_idx, order, n_vars):
    tabs = tables(n_vars, n_tables, 11000 + degree)
    coeffs = rand_fr(len(terms_idx), 12000 + degree)
    coeffs[0] = one()
    terms = [(coeffs[i], f) for i, f in enumerate(terms_idx)]
    orc = O.Member.expr(tabs, terms, degree, order)
    dev = ctx.member_expr([ctx.upload(t) for t in tabs], terms, degree, order)
    run_expr(ctx, dev, orc, n_vars, 13000 + degree, order, False, CATALOGUE_FUSED[name])


def test_claim_reduction_in_lc_form_fuses(ctx):
    """eq * (o1 + g2 o2 + g3 o3) as ONE group of two factors (the descriptor rewrite of the optimized tier): 1 * 3 + 2 * 2 = 7 multiplies <= 2 * 4 tables, so rounds 1
    and 2 run k_round_evals_group<3, LowToHigh, no skip, FUSED> -- the flat form of the same summand (13 multiplies) does not fuse, see the catalogue."""
    n_vars = 18
    tabs = tables(n_vars, 4, 14000)
    g2, g3 = rand_fr(2, 14100)
    orc = O.Member.expr(tabs, [(one(), [0, 1]), (g2, [0, 2]), (g3, [0, 3])], 2)
    groups = [[(None, [(one(), 0)]), (None, [(one(), 1), (g2, 2), (g3, 3)])]]
    dev = ctx.member_lc([ctx.upload(t) for t in tabs], groups, 2)
    run_expr(ctx, dev, orc, n_vars, 14200, L2H, False, True)


# ---- every NE: products of single-table factors --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [L2H, H2L])
@pytest.mark.parametrize("degree", [1, 2, 3, 4, 5, 6, 7])
def test_product_of_single_table_factors_without_skip(ctx, degree, order):
    """NE = degree + 1 = 2..8 in k_round_evals_group<NE, order, no skip, unfused> at 16 (round 0), then the tail kernel"""
    n_vars = 16
    tabs = tables(n_vars, degree, 15000 + degree)
    terms = [(rand_fr(1, 15100 + degree)[0], list(range(degree)))]
    orc = O.Member.expr(tabs, terms, degree, order)
    dev = ctx.member_expr([ctx.upload(t) for t in tabs], terms, degree, order)
    run_expr(ctx, dev, orc, n_vars, 15200 + degree, order, False, False)


def skip_product(ctx, n_vars, degree, order, seed):
    tabs = tables(n_vars, degree, seed)
    orc = O.Member.expr(tabs, [(one(), list(range(degree)))], degree, order)
    groups = [[(None, [(one(), k)]) for k in range(degree)]]
    dev = ctx.member_lc([ctx.upload(t) for t in tabs], groups, degree, order=order, skip_one=True)
    return dev, orc


@pytest.mark.parametrize("order", [L2H, H2L])
@pytest.mark.parametrize("degree", [1, 2, 3, 4, 5, 6, 7])
def test_product_of_single_table_factors_with_skip_one(ctx, degree, order):
    """SKIP1 with NE = degree = 1..7 at 16: k_round_evals_group<NE, order, skip, unfused> in round 0.  NE = 1 exists only as degree 1 with skip-one, which
    jolt_member_create_lc accepts (degree >= 1 is its only bound): the one sum is s(0) and s(1) = claim - s(0)."""
    dev, orc = skip_product(ctx, 16, degree, order, 16000 + degree)
    assert dev.n_evals == degree
    run_expr(ctx, dev, orc, 16, 16200 + degree, order, True, False)


@pytest.mark.parametrize("degree", [1, 2, 3])
def test_skip_one_products_the_rule_fuses(ctx, degree):
    """SKIP1 and FUSED together at 18: unit coefficients, (degree - 1) * degree multiplies against 2 * degree tables -- 0 <= 2, 2 <= 4, 6 <= 6 (degree 4: 12 > 8)"""
    dev, orc = skip_product(ctx, 18, degree, L2H, 16500 + degree)
    run_expr(ctx, dev, orc, 18, 16700 + degree, L2H, True, True)


def test_fusion_without_skip_at_degree_two(ctx):
    """FUSED without SKIP1 beyond the linear member: a * b with unit coefficient, NE = 3, 1 * 3 = 3 multiplies <= 2 * 2 tables"""
    tabs = tables(18, 2, 17000)
    orc = O.Member.expr(tabs, [(one(), [0, 1])], 2)
    dev = ctx.member_expr([ctx.upload(t) for t in tabs], [(one(), [0, 1])], 2)
    run_expr(ctx, dev, orc, 18, 17100, L2H, False, True)


# ---- owner stores, unmentioned tables, constants ---------------------------------------------------------------------------------------------------------------
def test_hamming_booleanity_in_lc_form_stays_unfused(ctx):
    """[[0, 1, 1], [0, 1]] in LC form with every coefficient one: table 1 in two factors of group 0 and again in group 1.  The default rule does NOT fuse it --
    2 * 4 + 1 * 4 = 12 multiplies > 2 * 2 tables (9 > 4 with skip-one) -- so at 18 it runs the unfused group kernel for three rounds behind separate binds,
    which the counters show; the fused owner-stores-once path is pinned by the next test on a summand with the same repetitions that the rule does fuse."""
    n_vars = 18
    tabs = tables(n_vars, 2, 18000)
    orc = O.Member.expr(tabs, [(one(), [0, 1, 1]), (one(), [0, 1])], 3)
    f = lambda t: (None, [(one(), t)])
    dev = ctx.member_lc([ctx.upload(t) for t in tabs], [[f(0), f(1), f(1)], [f(0), f(1)]], 3)
    run_expr(ctx, dev, orc, n_vars, 18100, L2H, False, False)


def test_repeated_table_is_stored_once_by_its_owner_in_fused_rounds(ctx):
    """T0 (T1 + T2) (T1 + T3) + (T0 + T4) (T1 + T5): T1 sits in two factors of group 0 and again in group 1, T0 in both groups; unit coefficients, NE = 4,
    2 * 4 + 1 * 4 = 12 multiplies <= 2 * 6 tables, so rounds 1 and 2 are fused and only the FIRST entry naming a table (lc_owner) writes its bound values.  A second
    writer, or none, shows in the later rounds' sums and in the bound tables final_values returns (run_expr's lockstep compares them)."""
    n_vars = 18
    tabs = tables(n_vars, 6, 19000)
    flat = [[0, 1, 1], [0, 1, 3], [0, 2, 1], [0, 2, 3], [0, 1], [0, 5], [4, 1], [4, 5]]
    orc = O.Member.expr(tabs, [(one(), t) for t in flat], 3)
    lc = lambda *ts: (None, [(one(), t) for t in ts])
    dev = ctx.member_lc([ctx.upload(t) for t in tabs], [[lc(0), lc(1, 2), lc(1, 3)], [lc(0, 4), lc(1, 5)]], 3)
    run_expr(ctx, dev, orc, n_vars, 19100, L2H, False, True)


def test_unmentioned_table_blocks_fusion_and_is_still_bound(ctx):
    """T0 + T1 over three tables: 0 multiplies, but a fused round binds a table through its owner entry and T2 has none (all_tables_used == false), so every bind
    is a separate launch; T2 must come out bound all the same (final_values)."""
    n_vars = 18
    tabs = tables(n_vars, 3, 20000)
    orc = O.Member.expr(tabs, [(one(), [0]), (one(), [1])], 1)
    dev = ctx.member_lc([ctx.upload(t) for t in tabs], [[(None, [(one(), 0)])], [(None, [(one(), 1)])]], 1)
    run_expr(ctx, dev, orc, n_vars, 20100, L2H, False, False)


@pytest.mark.parametrize("order", [L2H, H2L])
def test_constant_one_group_and_factor_constant(ctx, order):
    """(c0 + T0) * (g T1) + 1: a factor with a non-zero constant and a group without factors (f1 == f0: the empty product, one per pair) in the group kernel at 16"""
    n_vars = 16
    tabs = tables(n_vars, 2, 21000)
    c0, g = rand_fr(2, 21100)
    orc = O.Member.expr(tabs, [(g, [0, 1]), (fmul(g, c0), [1]), (one(), [])], 2, order)
    dev = ctx.member_lc([ctx.upload(t) for t in tabs], [[(c0, [(one(), 0)]), (None, [(g, 1)])], []], 2, order=order)
    run_expr(ctx, dev, orc, n_vars, 21200, order, False, False)


# ---- members with the eq weight factored out --------------------------------------------------------------------------------------------------------------------
def lockstep_split_eq(dev, orc, n_vars, challenge):
    """test_split_eq_uniform_product_member_lockstep's loop: q sums -> gruen_poly_from_q against the flat member over the dense eq table; eq comes last on the device"""
    claim = orc.input_claim()
    assert np.array_equal(dev.input_claim(), claim)
    bind = None
    for rnd in range(n_vars):
        want = orc.prove_round(bind, claim)
        evals, aux = dev.prove_round(bind, want_aux=True)
        got = ffi.host_gruen_poly_from_q(aux[0], aux[1], evals, claim)
        assert np.array_equal(got, want), f"round {rnd}"
        bind = challenge(rnd)
        claim = O.univariate_evaluate(want, bind)
    orc.finish_rounds(bind)
    dev.finish(bind)
    fv, ofv = dev.final_values(), orc.final_values()
    assert np.array_equal(fv[:-1], ofv[1:]) and np.array_equal(fv[-1], ofv[0])


@pytest.mark.parametrize("n_vars", [16, 18])
def test_eq_weighted_lc_member_in_the_group_kernel(ctx, n_vars):
    """The inner summand of test_eq_weighted_lc_member_matches_oracle, where its round 0 (16) and rounds 0..2 (18) run k_round_evals_group<2, LowToHigh, skip> with
    the E_out * E_in row weight.  3 groups * 1 * 2 + 2 (g) + the row weight's 3 * 2 + 1 = 15 multiplies > 2 * 6 tables: never fused."""
    w, scale = rand_fr(n_vars, 22000), rand_fr(1, 22001)[0]
    tabs = tables(n_vars, 6, 22100)
    g, c0 = rand_fr(2, 22200)
    o = one()
    inner = [[(None, [(o, 0)]), (None, [(o, 1)])], [(None, [(o, 2)]), (None, [(o, 3)])], [(None, [(g, 4)]), (c0, [(o, 5)])]]
    dev = Traced(ctx, ctx.member_lc([ctx.upload(t) for t in tabs], inner, 2, eq_point=w, eq_scale=scale))
    orc = O.Member.expr([O.eq_evals(w, scale)] + tabs, [(o, [0, 1, 2]), (o, [0, 3, 4]), (g, [0, 5, 6]), (fmul(g, c0), [0, 5])], 3)
    lockstep_split_eq(dev, orc, n_vars, alternating(22300))
    rounds = check_paths(dev, "expr", n_vars, skip=True, fusable=False)
    assert rounds[0]["group"][(L2H, True, False)] == 1 and rounds[0]["tail"] == 0
    dev.destroy()


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("n_vars", [16, 18])
def test_split_eq_product_above_the_threshold(ctx, n_vars, scaled):
    """k_split_eq_product<false> at 16 (and in round 0 and from round 3 on at 18), k_split_eq_product<true> in rounds 1 and 2 at 18 under both challenge shapes"""
    a, b = rand_fr(1 << n_vars, 23000 + n_vars), rand_fr(1 << n_vars, 23100 + n_vars)
    w = rand_fr(n_vars, 23200 + n_vars)
    scale = rand_fr(1, 23300)[0] if scaled else None
    orc = O.Member.gruen_product(a, b, w, scale)
    dev = Traced(ctx, ctx.member_split_eq_product(ctx.upload(a), ctx.upload(b), w, scale))
    S.lockstep(dev, orc, n_vars, 23400, challenge=alternating(23400 + n_vars))
    rounds = check_paths(dev, "product", n_vars, fusable=True)
    assert sum(r["split_eq_product"][1] for r in rounds) == (2 if n_vars == 18 else 0)
    assert rounds[0]["split_eq_product"] == (1, 0)
    dev.destroy()


@pytest.mark.parametrize("V,F", [(2, 2), (3, 3), (8, 4), (1, 4)])
def test_split_eq_uniform_member_rows_major(ctx, V, F):
    """n_vars 17: round 0 has 65536 pairs, the size at which a uniform member with V > 1 runs k_split_eq_uniform_rows<F> (one item per pair); round 1 is back on
    (v, pair) items, and V = 1 never leaves them.  Against the flat member over the dense eq table, as test_split_eq_uniform_product_member_lockstep."""
    n_vars = 17
    w = rand_fr(n_vars, 24000 + F)
    tabs = tables(n_vars, V * F, 24100 + V)
    coeffs = rand_fr(V, 24200 + V)
    coeffs[0] = one()
    scale = rand_fr(1, 24300)[0] if V == 3 else None
    terms = [(coeffs[v], [0] + [1 + v * F + k for k in range(F)]) for v in range(V)]
    orc = O.Member.expr([O.eq_evals(w, scale)] + tabs, terms, F + 1)
    dev = Traced(ctx, ctx.member_split_eq_uniform([ctx.upload(t) for t in tabs], V, F, coeffs, w, scale=scale))
    lockstep_split_eq(dev, orc, n_vars, alternating(24400))
    rounds = check_paths(dev, "uniform", n_vars, V=V)
    assert (rounds[0]["uniform_rows"], rounds[0]["uniform_items"]) == ((1, 0) if V > 1 else (0, 1))
    assert sum(r["uniform_rows"] for r in rounds) == (1 if V > 1 else 0)
    dev.destroy()


# ---- batches ------------------------------------------------------------------------------------------------------------------------------------------------------
def same_batch(got, want, devs, orcs_final):
    for k in ("polys", "challenges", "member_claims", "final_claim"):
        assert np.array_equal(got[k], want[k]), k
    for i, (d, fv) in enumerate(zip(devs, orcs_final)):
        dv = d.final_values()
        if d.uniform:  # the flat oracle member carries eq first, the device member its bound eq scalar last
            assert np.array_equal(dv[:-1], fv[1:]) and np.array_equal(dv[-1], fv[0]), i
        else:
            assert np.array_equal(dv, fv), i


def mixed_members(ctx, want_oracle):
    """(rounds, device member, oracle member or None).  m0 and m2 share the class (NE 3, LowToHigh, no skip) at 18 and 16 rounds; m1 is HighToLow."""
    o = one()
    out = []

    def add(rounds, dev, orc):
        out.append((rounds, dev(), orc() if want_oracle else None))
    t0 = tables(18, 3, 30000); g0 = rand_fr(1, 30001)[0]
    # m0: eq * (a + g b) in LC form, 1 * 3 + 2 = 5 multiplies <= 2 * 3: fused in its rounds 1 and 2
    add(18, lambda: ctx.member_lc([ctx.upload(t) for t in t0], [[(None, [(o, 0)]), (None, [(o, 1), (g0, 2)])]], 2),
        lambda: O.Member.expr(t0, [(o, [0, 1]), (g0, [0, 2])], 2))
    t1 = tables(18, 2, 30100); c1 = rand_fr(1, 30101)[0]
    add(18, lambda: ctx.member_expr([ctx.upload(t) for t in t1], [(c1, [0, 1])], 2, H2L), lambda: O.Member.expr(t1, [(c1, [0, 1])], 2, H2L))
    t2 = tables(16, 3, 30200); g2 = rand_fr(1, 30201)[0]
    add(16, lambda: ctx.member_expr([ctx.upload(t) for t in t2], [(o, [0, 1]), (g2, [0, 2])], 2), lambda: O.Member.expr(t2, [(o, [0, 1]), (g2, [0, 2])], 2))
    a3, b3, w3 = rand_fr(1 << 12, 30300), rand_fr(1 << 12, 30301), rand_fr(12, 30302)
    add(12, lambda: ctx.member_split_eq_product(ctx.upload(a3), ctx.upload(b3), w3), lambda: O.Member.gruen_product(a3, b3, w3))
    t4 = tables(12, 4, 30400); w4 = rand_fr(12, 30401); c4 = rand_fr(2, 30402)
    add(12, lambda: ctx.member_split_eq_uniform([ctx.upload(t) for t in t4], 2, 2, c4, w4),
        lambda: O.Member.expr([O.eq_evals(w4)] + t4, [(c4[0], [0, 1, 2]), (c4[1], [0, 3, 4])], 3))
    t5 = tables(12, 3, 30500)
    add(12, lambda: ctx.member_lc([ctx.upload(t) for t in t5], [[(None, [(o, k)]) for k in range(3)]], 3, skip_one=True),
        lambda: O.Member.expr(t5, [(o, [0, 1, 2])], 3))
    t6 = tables(18, 3, 30600)
    # m6: triple product, 2 * 4 = 8 multiplies > 2 * 3: unfused group kernel behind separate binds in rounds 1 and 2
    add(18, lambda: ctx.member_expr([ctx.upload(t) for t in t6], [(o, [0, 1, 2])], 3), lambda: O.Member.expr(t6, [(o, [0, 1, 2])], 3))
    return out


MIXED_COEFFS = 30700
_mixed_oracle = {}


def mixed_oracle(align, mode, ctx):
    """the oracle's batch, computed once per (alignment, challenge mode) and left unchanged"""
    key = (align, mode)
    if key not in _mixed_oracle:
        ms = mixed_members(ctx, True)
        for _, d, _ in ms:
            d.destroy()
        orcs = [m for _, _, m in ms]
        claims = [m.input_claim() for m in orcs]
        offsets = [18 - r if align == "tail" else 0 for r, _, _ in ms]
        if align == "head":  # prove_batch pads a member's claim by 2^(18 - rounds) for the inactive rounds in front of it: none here, so hand in the claim over 2^(18 - rounds)
            half = O.fr_inv(O.to_mont([2]))[0]
            for i, (r, _, _) in enumerate(ms):
                for _ in range(18 - r):
                    claims[i] = fmul(claims[i], half)
        want = O.prove_batch(orcs, claims, list(rand_fr(len(ms), MIXED_COEFFS)), offsets, 18, 3, label=77, challenge_mode=mode)
        _mixed_oracle[key] = (claims, offsets, want, [m.final_values() for m in orcs])
    return _mixed_oracle[key]


@pytest.mark.parametrize("grouped", [True, False])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("align", ["tail", "head"])
def test_mixed_batch_of_18_16_and_12_rounds(ctx, align, mode, grouped):
    """Seven members of mixed kinds and 18, 16 and 12 rounds in one prove_batch, bit for bit against O.prove_batch, under 125-bit and full-width challenges.
    Tail-aligned (offset = 18 - rounds, what the reference prover builds), members active together always have equal lengths, so fused group, unfused group and tail
    kernels cannot meet in one round, nor can one class hold unequal halves.  Head-aligned (offset 0, every member active from round 0 and padded BEHIND its last
    round; its input claim is handed in divided by the 2^(18 - rounds) the batch pads in front) they do: round 0 puts m0 (2^17 pairs) and m2 (2^15 pairs) into
    ONE launch of their class (blockIdx.y = 1 with a smaller half), and rounds 1 and 2 each hold the fused group kernel (m0), the unfused one (m1 HighToLow, m6)
    and the tail kernel (m2, m5).  The launch counts below are worked out from the rule, per alignment:
      tail: group LowToHigh unfused  r0 {m0}, {m6};  r1 {m6};  r2 {m6}, {m2}            = 5     head: r0 {m0, m2}, {m6};  r1 {m6};  r2 {m6}   = 4 (5 if m0, m2 were apart)
            group LowToHigh fused    r1, r2 {m0}                                       = 2           r1, r2 {m0}                            = 2
            group HighToLow          r0, r1, r2 {m1}                                   = 3           r0, r1, r2 {m1}                        = 3
            tail                     r3 .. r17, one launch each                        = 15          r0 .. r17 (m5 from r0, m2 from r1)     = 18
      so head-aligned, 18 tail launches in 18 rounds put one beside the two fused launches, which can only be rounds 1 and 2, where m1 is in the unfused kernel."""
    claims, offsets, want, finals = mixed_oracle(align, mode, ctx)
    devs = [d for _, d, _ in mixed_members(ctx, False)]
    ctx.round_path_stats(reset=True)
    got = ctx.prove_batch(devs, claims, list(rand_fr(len(devs), MIXED_COEFFS)), offsets, 18, 3, label=77, challenge_mode=mode, use_round_group=grouped)
    st = ctx.round_path_stats(reset=True)
    print(f"\nPATH batch: {launches(st)}")
    same_batch(got, want, devs, finals)
    assert st["group"][(L2H, False, True)] == 2 and st["group"][(H2L, False, False)] == 3, st
    assert st["split_eq_product"] == (12, 0) and st["uniform_items"] == 12 and st["uniform_rows"] == 0, st
    assert sum(st["group"][(o, True, f)] for o in (0, 1) for f in (False, True)) == 0, st  # m5 (skip-one, 12 rounds) only ever on the tail kernel
    if grouped:
        assert st["group"][(L2H, False, False)] == (5 if align == "tail" else 4), st
        assert st["tail"] == (15 if align == "tail" else 18), st
    else:  # one member per launch: m0 r0, m2 r0, m6 r0..r2; tail rounds m0, m1, m6: 15 each, m2: 15, m5: 12
        assert st["group"][(L2H, False, False)] == 5 and st["tail"] == 3 * 15 + 15 + 12, st
    for d in devs:
        d.destroy()


def class_split_batch(ctx, n_members, tabs, entries_of, grouped):
    """n borrowed linear members over shared tables at 16 rounds, all in the class (NE 2, LowToHigh, no skip, unfused): prove_batch against the oracle's, and the launch
    counts.  Only round 0 is above the tail threshold, so the batch's group launches are round 0's."""
    n_vars = 16
    shared = [ctx.upload(t) for t in tabs]
    devs, orcs = [], []
    for i in range(n_members):
        ent = entries_of(i)
        devs.append(ctx.member_lc(shared, [[(None, ent)]], 1, borrow=True))
        orcs.append(O.Member.expr(tabs, [(c, [t]) for c, t in ent], 1))
    claims = [m.input_claim() for m in orcs]
    coeffs = list(rand_fr(n_members, 31900))
    want = O.prove_batch(orcs, claims, coeffs, [0] * n_members, n_vars, 1, label=9)
    ctx.round_path_stats(reset=True)
    got = ctx.prove_batch(devs, claims, coeffs, [0] * n_members, n_vars, 1, label=9, use_round_group=grouped)
    st = ctx.round_path_stats(reset=True)
    print(f"\nPATH batch: {launches(st)}")
    same_batch(got, want, devs, [m.final_values() for m in orcs])
    for t, h in zip(shared, tabs):
        assert np.array_equal(t.download(), h)  # borrowed tables stay as they were
    for d in devs:
        d.destroy()
    assert sum(st["group"][k] for k in st["group"] if k != (L2H, False, False)) == 0, st
    return st


@pytest.mark.parametrize("grouped", [True, False])
def test_seventeenth_member_of_a_class_goes_into_a_second_launch(ctx, grouped):
    """kMaxGroupMembers = 16: seventeen members of one class need two launches in round 0 (and two tail launches in each of the fifteen rounds after it)"""
    tabs = tables(16, 3, 31000)
    cs = rand_fr(17, 31100)
    st = class_split_batch(ctx, 17, tabs, lambda i: [(cs[i], i % 3)], grouped)
    assert st["group"][(L2H, False, False)] == (2 if grouped else 17), st
    assert st["tail"] == (2 * 15 if grouped else 17 * 15), st


def test_class_splits_when_its_tables_pass_96(ctx):
    """kMaxGroupTables = 96: three members over the same 33 borrowed tables (one factor of 33 entries each) are 99 table slots, so the third starts a second
    launch in round 0 and a second tail launch in every later round"""
    tabs = tables(16, 33, 32000)
    cs = rand_fr(3 * 33, 32100).reshape(3, 33, 4)
    st = class_split_batch(ctx, 3, tabs, lambda i: [(cs[i][t], t) for t in range(33)], True)
    assert st["group"][(L2H, False, False)] == 2 and st["tail"] == 2 * 15, st
