"""CPU-side checks of the address-major Dory entries (dory_am.hip.h): the five entries are declared, exported and bound; the placement against its formula and the
reference's address_cycle_to_index; the accumulation routine of k_dory_am_onehot_rows -- limb-form mixed additions with their exceptional cases -- through its
host form against the oracle.  Points are compared as group elements, the normalised representative and the identity bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle_lib as O
from dory_groups import G1, R
from jolt_amd import ffi
from util import rand_fr

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
ENTRIES = ["jolt_dory_hints_onehot_am", "jolt_dory_hints_rows_am", "jolt_dory_fold_rows_grid_am", "jolt_host_dory_am_place", "jolt_host_dory_am_row"]
SHAPES = [(8, 4, 0, 6), (12, 2, 0, 10), (7, 9, 0, 10), (6, 4, 2, 8), (6, 4, 0, 4), (10, 4, 0, 9)]  # (log_t, log_k, e, sigma)
IDENT = O.g1_identity()
ONE = IDENT[0:4]
COLD = 0xFFFF
SENTINEL = 0xA5A5A5A5A5A5A5A5


def test_entries_are_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jolt_hip.h")).read(), flags=re.S)
    ffi_rs = open(os.path.join(ROOT, "rust", "jolt-kernels-hip", "src", "ffi.rs")).read()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(ffi.lib(), name), name
        assert re.search(r"pub fn %s\(" % name, ffi_rs), name
    for method in ("dory_hints_onehot_am", "dory_hints_rows_am", "dory_fold_rows_grid_am"):
        assert callable(getattr(ffi.Context, method))
    assert callable(ffi.host_dory_am_place) and callable(ffi.host_dory_am_row)
    # the names stay outside the set tests/test_dory_reduce_cpu.py pins
    assert not any(re.fullmatch(r"jolt_(host_)?dory_(vec_\w+|g2_prepare_vec|products|batch_plan)", n) for n in ENTRIES)


def test_module_imports_without_a_gpu():
    import inspect

    from jolt_amd import dory_commit
    params = inspect.signature(dory_commit.DoryWitnessCommitment.__init__).parameters
    assert list(params)[1:] == ["setup", "srs", "sources", "dense", "sigma", "order", "log_k", "log_extra"]
    assert params["order"].default == "cycle_major" and params["log_k"].default is None and params["log_extra"].default == 0


# ------------------------------------------------------------------------------------------------------ the placement
@pytest.mark.parametrize("log_t,log_k,e,sigma", SHAPES)
def test_place_is_the_formula(log_t, log_k, e, sigma):
    log_block, log_stride = log_k + e, e
    cycles = range(1 << log_t)
    seen = set()
    for t in cycles:
        for k in range(1 << log_k):
            index = (t << log_block) + (k << log_stride)
            assert ffi.host_dory_am_place(log_block, log_stride, sigma, t, k) == (index >> sigma, index & ((1 << sigma) - 1))
            if e == 0:
                assert index == t * (1 << log_k) + k  # address_cycle_to_index: cycle * num_addresses + address
            seen.add(index)
    assert len(seen) == len(cycles) * (1 << log_k)  # injective
    if sigma >= log_block:  # row r holds the whole cycles [r C, (r + 1) C)
        per_row = 1 << (sigma - log_block)
        for t in (0, per_row - 1, per_row, (1 << log_t) - 1):
            for k in (0, (1 << log_k) - 1):
                row, col = ffi.host_dory_am_place(log_block, log_stride, sigma, t, k)
                assert row == t // per_row and col == ((t % per_row) << log_block) + (k << log_stride)


def test_place_power_of_two_analogue_of_the_reference_vector():
    """the reference's own vector is address 3, cycle 4, 10 addresses -> 43 = 4 * 10 + 3; with 16 addresses it is 4 * 16 + 3 = 67"""
    row, col = ffi.host_dory_am_place(4, 0, 5, 4, 3)
    assert (row << 5) + col == 4 * 16 + 3 == 67
    assert (row, col) == (2, 3)


def test_place_refusals():
    lib = ffi.lib()
    row, col = C.c_size_t(77), C.c_size_t(78)
    args = lambda lb, ls, r=C.byref(row), c=C.byref(col): (C.c_uint32(lb), C.c_uint32(ls), C.c_uint32(6), C.c_size_t(1), C.c_size_t(1), r, c)  # noqa: E731
    assert lib.jolt_host_dory_am_place(*args(2, 3)) == 1  # log_stride > log_block
    assert lib.jolt_host_dory_am_place(*args(4, 0, r=None)) == 1
    assert lib.jolt_host_dory_am_place(*args(4, 0, c=None)) == 1
    assert (row.value, col.value) == (77, 78)
    assert lib.jolt_host_dory_am_place(*args(4, 0)) == 0 and (row.value, col.value) == (0, 17)


# ------------------------------------------------------------------------------------------------------ one row through the kernel's accumulation routine
@pytest.fixture(scope="module")
def beta_bases():
    """64 bases beta^j G with z = 1"""
    beta = rand_fr(1, 1500)[0]
    return beta, ffi.host_dory_g1_normalise(O.srs_setup_from_secret(beta, 64), 1)


def assert_point(got, want, what=None):
    if O.g1_is_identity(want):
        assert np.array_equal(got, IDENT), what
    else:
        assert np.array_equal(got[8:12], ONE), what
        assert O.g1_on_curve(got) and O.g1_eq(got, want), what


def row_definition(beta, hot, log_block, log_stride, n_bases):
    """(sum over the hot cycles of beta^index) G through the oracle's field arithmetic"""
    coeffs = [0] * n_bases
    for j, h in enumerate(hot):
        if h != COLD:
            coeffs[(j << log_block) + (int(h) << log_stride)] += 1
    return O.g1_scalar_mul(O.g1_generator(), O.kzg_eval_univariate(O.to_mont(coeffs), beta))


@pytest.mark.parametrize("log_block,log_stride,k,cycles", [(4, 0, 16, 4), (2, 0, 4, 16), (2, 0, 3, 16), (4, 2, 4, 4), (6, 0, 64, 1), (0, 0, 1, 64), (3, 1, 4, 8)])
def test_random_rows_against_the_oracle(beta_bases, log_block, log_stride, k, cycles):
    beta, bases = beta_bases
    rng = np.random.default_rng(1501 + log_block * 10 + cycles)
    for trial in range(3):
        hot = rng.integers(0, k, size=cycles).astype(np.uint16)
        hot[rng.random(cycles) < (0.0, 0.25, 0.6)[trial]] = COLD
        got = ffi.host_dory_am_row(bases, hot, k, log_block, log_stride)
        assert_point(got, row_definition(beta, hot, log_block, log_stride, 64), (trial, hot))


def test_row_over_one_point_is_a_chain_of_doublings():
    """every base is P: the second addition is P + P, and the result is m P for m hot cycles"""
    p = ffi.host_dory_g1_normalise(G1.point(12345)[None, :], 1)[0]
    bases = np.stack([p] * 64)
    for hot in ([0] * 2, [1, 0, 3, 2] * 4, [COLD, 2, 2, COLD, 1, 0, COLD, 3, 3, 3, 0, COLD, COLD, 1, 2, 0], [3] * 16):
        m = sum(1 for h in hot if h != COLD)
        assert_point(ffi.host_dory_am_row(bases, np.array(hot, dtype=np.uint16), 4, 2), G1.point(12345 * m), hot)


def test_row_over_alternating_points_meets_the_identity_and_goes_on():
    """bases P, -P, P, ...: address parity picks the sign, so partial sums pass through the identity in the middle of a row and the row continues"""
    p = ffi.host_dory_g1_normalise(G1.point(777)[None, :], 1)[0]
    bases = np.stack([p if i % 2 == 0 else O.g1_neg(p) for i in range(64)])
    for hot in ([0, 1], [0, 1, 0, 1, 2, 3, 3, 2], [0, 1, 2, 2, 3, 3], [0, 0, 1, 1, 1, 1, 0, 0], [0, 1, COLD, 2, COLD, 3, 0, 0, 3, 1, COLD, COLD, 2, 1, 0, 3], [1, 0, 1, 0, 1]):
        net = sum(1 if h % 2 == 0 else -1 for h in hot if h != COLD)
        got = ffi.host_dory_am_row(bases, np.array(hot, dtype=np.uint16), 4, 2)
        assert_point(got, G1.point(777 * net % R), hot)
    # net zero after non-zero partial sums: bit for bit the identity
    assert np.array_equal(ffi.host_dory_am_row(bases, np.array([0, 0, 1, 1], dtype=np.uint16), 4, 2), IDENT)


def test_all_cold_and_empty_rows_are_the_identity(beta_bases):
    _, bases = beta_bases
    assert np.array_equal(ffi.host_dory_am_row(bases, np.full(16, COLD, dtype=np.uint16), 4, 2), IDENT)
    assert np.array_equal(ffi.host_dory_am_row(bases, np.zeros(0, dtype=np.uint16), 4, 2), IDENT)


def test_row_with_a_base_at_infinity(beta_bases):
    """z = 0 in the table: the point adds nothing"""
    beta, bases = beta_bases
    holed = bases.copy()
    holed[5] = IDENT
    hot = np.array([1, 1, 0, 3], dtype=np.uint16)  # indices 1, 5, 8, 15
    coeffs = [0] * 64
    for i in (1, 8, 15):
        coeffs[i] = 1
    assert_point(ffi.host_dory_am_row(holed, hot, 4, 2), O.g1_scalar_mul(O.g1_generator(), O.kzg_eval_univariate(O.to_mont(coeffs), beta)))


def test_row_refusals_write_nothing(beta_bases):
    _, bases = beta_bases
    lib = ffi.lib()
    hot = np.array([0, 1, 2, 3], dtype=np.uint16)
    out = np.full((1, 12), SENTINEL, dtype=np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731

    def call(b=bases, n=64, h=hot, cycles=4, k=4, log_block=2, log_stride=0, o=out):
        return lib.jolt_host_dory_am_row(p(b), C.c_size_t(n), p(h), C.c_size_t(cycles), C.c_uint32(k), C.c_uint32(log_block), C.c_uint32(log_stride), p(o))

    assert call(b=None) == 1 and call(h=None) == 1 and call(o=None) == 1
    assert call(k=0) == 1
    assert call(k=5) == 1                      # more addresses than the block holds
    assert call(log_block=2, log_stride=3) == 1
    assert call(log_block=3, log_stride=1, k=5) == 1
    assert call(n=15) == 1                     # (3 << 2) + 3 = 15 is the last base the row can touch
    assert (out == SENTINEL).all()
    assert call(n=16) == 0
    assert np.array_equal(out[0, 8:12], ONE)
