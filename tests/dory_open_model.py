"""A Dory evaluation proof (Dory paper, Eval-VMV-RE, non-hiding) in LOG SPACE, on top of dory_reduce_model.State: every group element is its discrete logarithm
modulo r, a pairing is a product, GT is written additively.  The model of jolt_amd/dory_open.py for the GPU tests, and an independent verifier.

Setup: Gamma1, Gamma2 of N elements, H1, H2, HT = e(H1, H2).  Statement: a 2^nu x 2^sigma matrix M (nu <= sigma), row commitments T'_i = <M_i, Gamma1[:2^sigma]>,
commitment T = <T', Gamma2[:2^nu]>, evaluation y = L^T M R.  With n = 2^sigma, T' padded to n with the identity (0) and L padded to n with zero:

    prover    v = L^T M;  v1 = T', v2 = v H2, s1 = R, s2 = L;  VMV message C = <v1, v2>, D2 = <Gamma1[:n], v2>, E1 = <v1, s2>;
              sigma rounds of Dory-Reduce (alpha folds v1 and s1, 1/alpha folds v2 and s2);  final message w1 = v1 + (gamma s1) H1, w2 = v2 + (s2 / gamma) H2
    verifier  e(E1, H2) = D2;  claims (C, D1 = T, D2, E1, E2 = y H2), s1 = R, s2 = L;  per round the five invariants and the folds of s1 and s2;  then
              C'' = C + s1 s2 HT + gamma e(H1, E2) + e(E1, H2) / gamma,  D1'' = D1 + gamma s1 e(H1, Gamma2[0]),  D2'' = D2 + (s2 / gamma) e(Gamma1[0], H2)
              and, for a challenge d,  e(w1 + d Gamma1[0], w2 + Gamma2[0] / d) = e(Gamma1[0], Gamma2[0]) + C'' + d D2'' + D1'' / d

Nothing here comes from the library."""
import dory_reduce_model as DM

R = DM.R
ip = DM.ip


def inv(x):
    return pow(x, -1, R)


def statement(g1, g2, matrix, left, right):
    """(rows T', T, v, y) of the matrix (a list of 2^nu rows of 2^sigma integers) against the setup"""
    n = len(matrix[0])
    rows = [ip(row, g1[:n]) for row in matrix]
    v = [sum(left[i] * matrix[i][j] for i in range(len(matrix))) % R for j in range(n)]
    return rows, ip(rows, g2[:len(rows)]), v, ip(v, right)


def pad(a, n):
    return list(a) + [0] * (n - len(a))


def initial_state(g1, g2, h2, rows, v, left, right):
    n = len(v)
    return DM.State(pad(rows, n), [x * h2 % R for x in v], list(right), pad(left, n), g1, g2)


def prove(g1, g2, h1, h2, rows, v, left, right, challenges, gamma):
    """challenges: one (beta, alpha) per round.  dict(vmv=(C, D2, E1), rounds=[(first message, second message)], final=(w1, w2))"""
    st = initial_state(g1, g2, h2, rows, v, left, right)
    n = st.n
    assert n & (n - 1) == 0 and len(challenges) == n.bit_length() - 1
    vmv = (ip(st.v1, st.v2), ip(g1[:n], st.v2), ip(st.v1, st.s2))
    rounds = []
    for beta, alpha in challenges:
        first = st.first_message()
        st.apply_beta(beta, inv(beta))
        second = st.second_message()
        st.apply_alpha(alpha, inv(alpha))
        rounds.append((first, second))
    assert st.n == 1
    final = ((st.v1[0] + gamma * st.s1[0] * h1) % R, (st.v2[0] + inv(gamma) * st.s2[0] * h2) % R)
    return dict(vmv=vmv, rounds=rounds, final=final)


def verify(g1, g2, h1, h2, commitment, y, left, right, proof, challenges, gamma, d):
    c, d2, e1 = proof["vmv"]
    if e1 * h2 % R != d2 % R:
        return False
    n = len(right)
    if len(proof["rounds"]) != n.bit_length() - 1 or len(challenges) != len(proof["rounds"]):
        return False
    claims = (c % R, commitment % R, d2 % R, e1 % R, y * h2 % R)
    s1, s2 = list(right), pad(left, n)
    for (first, second), (beta, alpha) in zip(proof["rounds"], challenges):
        setup = DM.State([0] * n, [0] * n, [0] * n, [0] * n, g1, g2).setup()  # the verifier's tables of this level depend on the bases alone
        claims = DM.invariants(claims, setup, first, second, beta, alpha)
        h, ai = n // 2, inv(alpha)
        s1 = [(alpha * l + r) % R for l, r in zip(s1[:h], s1[h:])]  # noqa: E741
        s2 = [(ai * l + r) % R for l, r in zip(s2[:h], s2[h:])]  # noqa: E741
        n = h
    c, d1, d2, e1, e2 = claims
    gi, di = inv(gamma), inv(d)
    c2 = (c + s1[0] * s2[0] * h1 * h2 + gamma * h1 * e2 + gi * e1 * h2) % R
    d1_2 = (d1 + gamma * s1[0] * h1 * g2[0]) % R
    d2_2 = (d2 + gi * s2[0] * g1[0] * h2) % R
    w1, w2 = proof["final"]
    return (w1 + d * g1[0]) * (w2 + di * g2[0]) % R == (g1[0] * g2[0] + c2 + d * d2_2 + di * d1_2) % R
