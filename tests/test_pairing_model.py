"""The big-integer pairing model of tests/pairing_model.py held to itself: the fast layer the other tests use against the layer written from the definition,
and the properties that make a value a pairing.  No library code, no GPU."""
import g2_model as M
import pairing_model as PM
from dory_groups import R, rand_ints


def test_fq12_model_is_a_field_with_the_expected_frobenius():
    x = [v % PM.Q for v in rand_ints(12, 1)]
    y = [v % PM.Q for v in rand_ints(12, 2)]
    assert PM.f12_mul(x, PM.f12_inv(x)) == PM.ONE
    assert PM.f12_mul(x, y) == PM.f12_mul(y, x) and PM.f12_mul(x, PM.ONE) == x
    w6 = PM.f12_pow(PM.f12({1: 1}), 6)
    assert PM.f12_add(PM.f12_sqr(PM.f12_sub(w6, PM.f12({0: 9}))), PM.ONE) == PM.ZERO  # (w^6 - 9)^2 = -1: w^6 - 9 is u
    assert PM.f12_pow(x, PM.Q ** 6) == PM.f12_conj(x)
    assert PM.gt_from_abi(PM.gt_to_abi(x)) == x


def test_fast_layer_equals_the_definition_on_two_pairings():
    a, b = rand_ints(2, 3)
    for p, q in ((PM.G1_GENERATOR, M.GENERATOR), (PM.g1_mul(a), M.mul_generator(b))):
        assert PM.pairing(p, q) == PM.pairing_definition(p, q)


def test_model_pairing_is_bilinear_of_order_r_and_not_the_plain_power():
    E = PM.generator_pairing()
    assert E != PM.ONE and PM.f12_pow(E, R) == PM.ONE
    a, b = rand_ints(1, 4)[0] >> 197, rand_ints(1, 5)[0] >> 53  # a 57-bit and a 201-bit scalar
    assert PM.pairing(PM.g1_mul(a), M.mul_generator(b)) == PM.f12_pow(E, a * b % R) == PM.expected([a], [b])
    miller = PM.miller(PM.G1_GENERATOR, M.GENERATOR)
    assert PM.f12_pow(miller, (PM.Q ** 12 - 1) // R) != E  # the final power carries the factor 2 z (6 z^2 + 3 z + 1)
    assert PM.pairing(None, M.GENERATOR) == PM.ONE and PM.pairing(PM.G1_GENERATOR, None) == PM.ONE
