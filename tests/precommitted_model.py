"""The precommitted claim reductions written from their definition, in Python integers mod r (TEST INFRASTRUCTURE; nothing here calls the library under test).

Definition: crates/jolt-kernels/src/precommitted_reduction.rs (PrecommittedTables: the tables, the schedule walk, the hint algebra, the running scale, the 6b -> 7
carry; lsb_permutation, permute_coefficients, permute_challenges) and crates/jolt-kernels/src/optimized/precommitted_reduction.rs (the shifted eq slice -- here
GATHERED FROM THE FULL eq table, which is what the reference tier does -- and the bytecode eq template in both trace orders).  `prove_batch` restates
crates/jolt-sumcheck/src/prover.rs:193-362 for members at ANY offset (a head-aligned member is active from round 0 at the padded claim and halves after its
window); its challenges come from the oracle's transcript (tests/oracle_lib.py), which is the only thing taken from outside this file."""
import numpy as np

import oracle_lib as O

R = O.R_MOD
TWO_INV = pow(2, -1, R)
CYCLE_MAJOR, ADDRESS_MAJOR = 0, 1


def ints(limbs):
    """Montgomery limb array -> list of Python ints"""
    return O.from_mont(np.asarray(limbs, dtype=np.uint64).reshape(-1, 4))


def limbs(values):
    return O.to_mont([int(v) % R for v in values])


def bind_low_to_high(table, r):
    return [(table[2 * y] + r * (table[2 * y + 1] - table[2 * y])) % R for y in range(len(table) // 2)]


def evaluate(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R
    return acc


class Tables:
    """PrecommittedTables (:76-85): value, eq, the aux passengers, the running scale and its inverse"""

    def __init__(self, value, eq, aux):
        self.value, self.eq, self.aux = [v % R for v in value], [v % R for v in eq], [[v % R for v in t] for t in aux]
        assert all(len(t) == len(self.value) for t in [self.eq] + self.aux)
        self.scale, self.scale_inv = 1, 1

    def bind_round(self, active, challenge):  # :160-172
        if not active:
            self.scale = self.scale * TWO_INV % R
            self.scale_inv = self.scale_inv * 2 % R
            return
        self.value, self.eq = bind_low_to_high(self.value, challenge), bind_low_to_high(self.eq, challenge)
        self.aux = [bind_low_to_high(t, challenge) for t in self.aux]

    def round_message(self, active, previous_claim):  # :96-133
        if not active:
            return [previous_claim * TWO_INV % R]
        v, e = self.value, self.eq
        assert len(v) >= 2, "an active round over a fully bound table"
        e0 = sum(v[2 * j] * e[2 * j] for j in range(len(v) // 2)) % R
        e2 = sum((2 * v[2 * j + 1] - v[2 * j]) * (2 * e[2 * j + 1] - e[2 * j]) for j in range(len(v) // 2)) % R
        e1 = (previous_claim * self.scale_inv - e0) % R  # the hint
        c2 = (e0 - 2 * e1 + e2) * TWO_INV % R
        c1 = (e1 - e0 - c2) % R
        return [e0 * self.scale % R, c1 * self.scale % R, c2 * self.scale % R]

    def intermediate_claim(self):  # :176-192
        return sum(a * b for a, b in zip(self.value, self.eq)) * self.scale % R


class Phase:
    """CycleReductionKernel / AddressReductionKernel (:269-453) over one Tables: prove_round(bind, round, claim) -> 1 or 3 coefficients, finish_rounds, output_claims"""

    def __init__(self, tables, active, total, address_follows):
        assert list(active) == sorted(set(active)) and all(0 <= a < total for a in active)
        self.t, self.active, self.total, self.address_follows = tables, set(active), total, address_follows

    def num_rounds(self):
        return self.total

    def prove_round(self, bind, rnd, previous_claim):  # :140-151
        assert (bind is None) == (rnd == 0)
        if bind is not None:
            self.t.bind_round(rnd - 1 in self.active, bind)
        return self.t.round_message(rnd in self.active, previous_claim)

    def finish_rounds(self, bind):  # :154-156
        self.t.bind_round(self.total - 1 in self.active, bind)

    def output_claims(self):
        if self.address_follows:
            return [self.t.intermediate_claim()]
        if len(self.t.value) != 1:
            raise ValueError("precommitted reduction final claim requested before the polynomial is fully bound")
        return [self.t.value[0]] + [a[0] for a in self.t.aux]


class Reduction:
    """one reduction: .cycle, and after the cycle rounds .address() resumes from the SAME tables and scale under the address schedule"""

    def __init__(self, value, eq, aux, cycle_active, cycle_total, address_active=(), address_total=0):
        self.tables = Tables(value, eq, aux)
        assert (1 << (len(cycle_active) + len(address_active))) == len(self.tables.value)
        self.address_active, self.address_total = list(address_active), address_total
        self.cycle = Phase(self.tables, cycle_active, cycle_total, address_follows=len(address_active) > 0)

    def input_claim(self):
        return self.tables.intermediate_claim()

    def address(self):
        assert self.address_active
        return Phase(self.tables, self.address_active, self.address_total, address_follows=False)


def drive(phase, claim, challenges):
    """a phase alone under prescribed challenges -> (messages, the claim after the last round)"""
    msgs, bind = [], None
    for rnd in range(phase.num_rounds()):
        msgs.append(phase.prove_round(bind, rnd, claim))
        bind = challenges[rnd]
        claim = evaluate(msgs[-1], bind)
    if bind is not None:
        phase.finish_rounds(bind)
    return msgs, claim


# ---- schedules the suites share ------------------------------------------------------------------------------------------------------------------------
def schedule(kind, n):
    """-> (cycle_active, cycle_total, address_active, address_total) with n active rounds in all"""
    if kind == "all":
        return list(range(n)), n, [], 0
    if kind == "head":  # two inactive rounds in front
        return list(range(2, n + 2)), n + 2, [], 0
    if kind == "middle":  # two inactive rounds after the first half
        h = (n + 1) // 2
        return list(range(h)) + list(range(h + 2, n + 2)), n + 2, [], 0
    if kind == "tail":  # two inactive rounds at the end
        return list(range(n)), n + 2, [], 0
    if kind == "two_phase":  # k cycle rounds around an inactive one, the rest in the address phase behind an inactive head and around an inactive middle round
        k = n // 2
        cyc = [0] + list(range(2, k + 1)) if k else []
        m = n - k
        adr = [1] + list(range(3, m + 2))
        return cyc, k + 1, adr, m + 2
    raise ValueError(kind)


SCHEDULES = ["all", "head", "middle", "tail", "two_phase"]


# ---- the builders -----------------------------------------------------------------------------------------------------------------------------------
def lsb_permutation(perm_be):  # :595-609 (the identity is returned as a map too; `is_identity` says so)
    n = len(perm_be)
    if len(set(perm_be)) != n:
        raise ValueError("two variables in one opening round")
    by_round = sorted(range(n), key=lambda be: perm_be[be])
    out = [0] * n
    for new_lsb, be in enumerate(by_round):
        out[n - 1 - be] = new_lsb
    return out, all(a == b for a, b in enumerate(out))


def permute_coefficients(table, old_lsb_to_new_lsb):  # :615-636
    n = len(old_lsb_to_new_lsb)
    new_to_old = [0] * n
    for old, new in enumerate(old_lsb_to_new_lsb):
        new_to_old[new] = old
    out = []
    for new_index in range(len(table)):
        old_index = 0
        for new_lsb, old_lsb in enumerate(new_to_old):
            old_index |= ((new_index >> new_lsb) & 1) << old_lsb
        out.append(table[old_index])
    return out


def permute_challenges(challenges_be, old_lsb_to_new_lsb):  # :641-652
    n = len(challenges_be)
    out = list(challenges_be)
    for old_be, c in enumerate(challenges_be):
        out[n - 1 - old_lsb_to_new_lsb[n - 1 - old_be]] = c
    return out


def eq_table(r):
    """EqPolynomial::evals, big-endian: entry i = prod_k (bit (n - 1 - k) of i ? r[k] : 1 - r[k])"""
    out = [1]
    for x in r:
        out = [v for p in out for v in (p * (1 - x) % R, p * x % R)]
    return out


def shifted_eq(r, start_index, length):
    full = eq_table(r)
    return [full[(start_index + i) % len(full)] for i in range(length)]


def outer(lane_weights, cycle_table, order):
    lanes, cycles = len(lane_weights), len(cycle_table)
    out = []
    for index in range(lanes * cycles):
        lane, cycle = (index // cycles, index % cycles) if order == CYCLE_MAJOR else (index % lanes, index // lanes)
        out.append(lane_weights[lane] * cycle_table[cycle] % R)
    return out


def advice_tables(table, r_val, perm_be):
    """for_advice (optimized/precommitted_reduction.rs:223-249) -> (value, eq)"""
    m, same = lsb_permutation(perm_be)
    return (list(table), eq_table(r_val)) if same else (permute_coefficients(table, m), eq_table(permute_challenges(r_val, m)))


def program_image_tables(words, r_addr_rw, start_index, perm_be):
    """for_program_image (:298-334) -> (value, eq); `words` already padded to a power of two"""
    m, same = lsb_permutation(perm_be)
    eq = shifted_eq(r_addr_rw, start_index, len(words))
    return (list(words), eq) if same else (permute_coefficients(words, m), permute_coefficients(eq, m))


def bytecode_tables(chunks, chunk_weights, lane_weights, r_bc, order, perm_be):
    """for_bytecode (:396-465) -> (value, eq, aux)"""
    m, same = lsb_permutation(perm_be)
    value = [sum(c[i] * w for c, w in zip(chunks, chunk_weights)) % R for i in range(len(chunks[0]))]
    eq = outer(lane_weights, eq_table(r_bc), order)
    tabs = [value, eq] + [list(c) for c in chunks]
    if not same:
        tabs = [permute_coefficients(t, m) for t in tabs]
    return tabs[0], tabs[1], tabs[2:]


# ---- prove_batch (prover.rs:193-362) over members at any offset ----------------------------------------------------------------------------------------
class OracleExpr:
    """the oracle's dense member (O.Member.expr over Montgomery limb tables) behind the integer interface of Phase"""

    def __init__(self, tables, terms, degree):
        self.m = O.Member.expr(tables, terms, degree)

    def num_rounds(self):
        return self.m.num_rounds()

    def input_claim(self):
        return ints(self.m.input_claim())[0]

    def prove_round(self, bind, rnd, previous_claim):
        return ints(self.m.prove_round(None if bind is None else limbs([bind])[0], limbs([previous_claim])[0]))

    def finish_rounds(self, bind):
        self.m.finish_rounds(limbs([bind])[0])


def prove_batch(members, input_claims, coefficients, offsets, max_num_vars, max_degree, label=0, challenge_mode=0):
    """-> dict(polys [round][max_degree + 1], challenges, member_claims, final_claim), all Python ints"""
    n, stride = len(members), max_degree + 1
    rounds = [m.num_rounds() for m in members]
    assert all(off + r <= max_num_vars for off, r in zip(offsets, rounds))
    member_claims = [c * pow(2, max_num_vars - r, R) % R for c, r in zip(input_claims, rounds)]  # :246-250
    running = sum(a * c for a, c in zip(coefficients, member_claims)) % R
    pending = [None] * n
    tr = O.MockTranscript(label)
    polys, challenges = [], []
    for rnd in range(max_num_vars):
        batched, messages = [0] * stride, {}
        for i, m in enumerate(members):
            if not offsets[i] <= rnd < offsets[i] + rounds[i]:  # :271-281
                member_claims[i] = member_claims[i] * TWO_INV % R
                batched[0] = (batched[0] + coefficients[i] * member_claims[i]) % R
                continue
            msg = m.prove_round(pending[i], rnd - offsets[i], member_claims[i])
            pending[i] = None
            assert len(msg) <= stride
            messages[i] = msg
            for k, c in enumerate(msg):
                batched[k] = (batched[k] + coefficients[i] * c) % R
        assert (batched[0] + sum(batched)) % R == running, f"round {rnd}: s(0) + s(1) is not the running claim"  # :316-324
        ncoef = stride
        while ncoef > 2 and batched[ncoef - 1] == 0:
            ncoef -= 1
        tr.append_round_poly(limbs(batched[:ncoef]))
        challenge = ints(tr.challenge_scalar() if challenge_mode else tr.challenge())[0]
        running = evaluate(batched, challenge)
        polys.append(batched)
        challenges.append(challenge)
        for i, msg in messages.items():
            member_claims[i] = evaluate(msg, challenge)
            pending[i] = challenge
    for m, b in zip(members, pending):
        if b is not None:
            m.finish_rounds(b)
    return dict(polys=polys, challenges=challenges, member_claims=member_claims, final_claim=running)
