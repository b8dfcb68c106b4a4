"""Dory-Reduce with the scalar-product extension in LOG SPACE: every group element is its discrete logarithm modulo r (G1 and G2 to their generators, GT to the
pairing of the two generators), so an inner product <a, b> is sum a_i b_i mod r whatever the groups, and one round is plain modular arithmetic.  The model of
jolt_amd/dory_reduce.py for the GPU tests, and the statement of the five invariants a round keeps (Dory paper, Dory-Reduce):

    C'  = C + chi + beta D2 + (1/beta) D1 + alpha C+ + (1/alpha) C-
    D1' = alpha (D1L + beta Delta1L) + D1R + beta Delta1R           D2' = (1/alpha) (D2L + (1/beta) Delta2L) + D2R + (1/beta) Delta2R
    E1' = E1 + beta E1beta + alpha E1+ + (1/alpha) E1-              E2' = E2 + (1/beta) E2beta + alpha E2+ + (1/alpha) E2-

written additively (a GT power is a multiple of its logarithm).  Nothing here comes from the library."""
import oracle_lib as O

R = O.R_MOD


def ip(a, b):
    assert len(a) == len(b)
    return sum(x * y for x, y in zip(a, b)) % R


class State:
    def __init__(self, v1, v2, s1, s2, g1, g2):
        self.v1, self.v2, self.s1, self.s2, self.g1, self.g2 = (list(x) for x in (v1, v2, s1, s2, g1, g2))
        self.n = len(self.v1)

    def claims(self):
        """(C, D1, D2, E1, E2) of the current vectors against the current bases"""
        n = self.n
        return (ip(self.v1, self.v2), ip(self.v1, self.g2[:n]), ip(self.g1[:n], self.v2), ip(self.v1, self.s2), ip(self.s1, self.v2))

    def setup(self):
        """(chi, Delta1L, Delta1R, Delta2L, Delta2R): what the verifier holds precomputed for this n"""
        n, h = self.n, self.n // 2
        g1, g2 = self.g1[:n], self.g2[:n]
        return (ip(g1, g2), ip(g1[:h], g2[:h]), ip(g1[h:], g2[:h]), ip(g1[:h], g2[:h]), ip(g1[:h], g2[h:]))

    def first_message(self):
        n, h = self.n, self.n // 2
        return (ip(self.v1[:h], self.g2[:h]), ip(self.v1[h:], self.g2[:h]), ip(self.g1[:h], self.v2[:h]), ip(self.g1[:h], self.v2[h:]),
                ip(self.g1[:n], self.s2), ip(self.s1, self.g2[:n]))

    def apply_beta(self, beta, beta_inv):
        assert beta * beta_inv % R == 1
        n = self.n
        self.v1 = [(v + beta * g) % R for v, g in zip(self.v1, self.g1[:n])]
        self.v2 = [(v + beta_inv * g) % R for v, g in zip(self.v2, self.g2[:n])]

    def second_message(self):
        h = self.n // 2
        v1, v2, s1, s2 = self.v1, self.v2, self.s1, self.s2
        return (ip(v1[:h], v2[h:]), ip(v1[h:], v2[:h]), ip(v1[:h], s2[h:]), ip(v1[h:], s2[:h]), ip(s1[:h], v2[h:]), ip(s1[h:], v2[:h]))

    def apply_alpha(self, alpha, alpha_inv):
        assert alpha * alpha_inv % R == 1
        h = self.n // 2
        fold = lambda v, s: [(s * l + r) % R for l, r in zip(v[:h], v[h:])]  # noqa: E731, E741
        self.v1, self.v2, self.s1, self.s2 = fold(self.v1, alpha), fold(self.v2, alpha_inv), fold(self.s1, alpha), fold(self.s2, alpha_inv)
        self.n = h


def invariants(before, setup, first, second, beta, alpha):
    """the claims the five invariants give for the folded vectors, from the claims before the round, the setup values and the two messages"""
    c, d1, d2, e1, e2 = before
    chi, dl1, dr1, dl2, dr2 = setup
    d1l, d1r, d2l, d2r, e1b, e2b = first
    cp, cm, e1p, e1m, e2p, e2m = second
    bi, ai = pow(beta, -1, R), pow(alpha, -1, R)
    return ((c + chi + beta * d2 + bi * d1 + alpha * cp + ai * cm) % R,
            (alpha * (d1l + beta * dl1) + d1r + beta * dr1) % R,
            (ai * (d2l + bi * dl2) + d2r + bi * dr2) % R,
            (e1 + beta * e1b + alpha * e1p + ai * e1m) % R,
            (e2 + bi * e2b + alpha * e2p + ai * e2m) % R)
