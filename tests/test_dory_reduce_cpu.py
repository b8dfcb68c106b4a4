"""CPU checks of the Dory rounds on resident vectors: the log-space model of tests/dory_reduce_model.py keeps the five invariants of Dory-Reduce, the launch plan of
a product batch (dory_batch_plan.hpp through jolt_host_dory_batch_plan) is the padding it is stated to be, and jolt_amd/ffi.py binds every new entry point."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dory_reduce_model as DM
from dory_groups import R, rand_ints
from jolt_amd import ffi

LANES = 64


@pytest.mark.parametrize("n", [2, 4, 8, 16])
def test_model_keeps_the_five_invariants(n):
    """random vectors, bases and challenges: after every round the claims of the folded vectors against the halved bases are what the invariants give from the
    claims before the round, the setup values and the two messages -- down to n = 1"""
    v1, v2, s1, s2, g1, g2 = (rand_ints(n, 300 + 10 * n + k) for k in range(6))
    st = DM.State(v1, v2, s1, s2, g1, g2)
    challenges = rand_ints(2 * n.bit_length(), 400 + n)
    rounds = 0
    while st.n > 1:
        beta, alpha = challenges[2 * rounds] or 1, challenges[2 * rounds + 1] or 1
        before, setup = st.claims(), st.setup()
        first = st.first_message()
        st.apply_beta(beta, pow(beta, -1, R))
        second = st.second_message()
        st.apply_alpha(alpha, pow(alpha, -1, R))
        assert st.claims() == DM.invariants(before, setup, first, second, beta, alpha), (n, rounds)
        rounds += 1
    assert rounds == n.bit_length() - 1 and len(st.v1) == len(st.v2) == len(st.s1) == len(st.s2) == 1


def test_model_invariants_notice_a_swapped_challenge():
    """negative control: alpha and its inverse exchanged in the fold break C'"""
    v1, v2, s1, s2, g1, g2 = (rand_ints(4, 500 + k) for k in range(6))
    st = DM.State(v1, v2, s1, s2, g1, g2)
    beta, alpha = rand_ints(2, 510)
    before, setup, first = st.claims(), st.setup(), st.first_message()
    st.apply_beta(beta, pow(beta, -1, R))
    second = st.second_message()
    st.apply_alpha(pow(alpha, -1, R), alpha)
    assert st.claims()[0] != DM.invariants(before, setup, first, second, beta, alpha)[0]


def plan_restated(lens):
    wg_item, wg_first, base, packed = [], [], [], 0
    for k, n in enumerate(lens):
        base.append(packed)
        wgs = -(-n // LANES)
        wg_item += [k] * wgs
        wg_first += [w * LANES for w in range(wgs)]
        packed += wgs * LANES
    longest = max(lens, default=0)
    levels = (longest - 1).bit_length() if longest > 1 else 0
    return wg_item, wg_first, base, levels


@pytest.mark.parametrize("lens", [[], [0], [1], [64], [65], [0, 1, 2, 63, 64, 65, 129], [129, 0, 0, 5], [1000, 1, 4096, 4097], [2, 2, 2], [0, 0]],
                         ids=lambda lens: "-".join(map(str, lens)) or "none")
def test_batch_plan_is_its_restatement(lens):
    """ragged lists, empty items, a single item: whole wavefronts per item, a workgroup in one item only, ceil(log2) of the longest item as the level count"""
    wg_item, wg_first, base, levels = ffi.host_dory_batch_plan(lens)
    want = plan_restated(lens)
    assert (list(wg_item), list(wg_first), base, levels) == want
    # the properties the kernels rely on, stated directly: every element of every item is some workgroup's lane exactly once, and no slot is shared
    slots = set()
    for it, first in zip(wg_item, wg_first):
        for lane in range(LANES):
            assert (base[it] + first + lane) not in slots
            slots.add(base[it] + first + lane)
    for k, n in enumerate(lens):
        assert all(base[k] + i in slots for i in range(n))
    m, steps = max(lens, default=0), 0
    while m > 1:
        m, steps = (m + 1) // 2, steps + 1
    assert steps == levels


def test_batch_plan_refusals():
    one = (C.c_size_t * 1)(1 << 25)
    base = (C.c_size_t * 2)()
    n_wgs, levels = C.c_size_t(), C.c_uint32()
    f = ffi.lib().jolt_host_dory_batch_plan
    assert f(one, C.c_size_t(1), C.c_size_t(0), None, None, base, C.byref(n_wgs), C.byref(levels)) == 6  # unsupported: past 2^24 slots
    huge = (C.c_size_t * 2)(2**64 - 1, 2)  # a sum that would wrap
    assert f(huge, C.c_size_t(2), C.c_size_t(0), None, None, base, C.byref(n_wgs), C.byref(levels)) == 6
    two = (C.c_size_t * 1)(129)
    small = np.zeros(2, dtype=np.uint32)
    p = small.ctypes.data_as(C.c_void_p)
    assert f(two, C.c_size_t(1), C.c_size_t(2), p, p, base, C.byref(n_wgs), C.byref(levels)) == 5 and not small.any()  # three workgroups do not fit two entries
    assert f(two, C.c_size_t(1), C.c_size_t(0), None, None, None, C.byref(n_wgs), C.byref(levels)) == 1


NEW_SYMBOLS = ["jolt_dory_vec_upload", "jolt_dory_vec_download", "jolt_dory_vec_len", "jolt_dory_vec_kind", "jolt_dory_vec_free", "jolt_dory_vec_truncate",
               "jolt_dory_g2_prepare_vec", "jolt_dory_vec_scale_bases_add", "jolt_dory_vec_scale_vs_add", "jolt_dory_vec_fold_field", "jolt_dory_products",
               "jolt_host_dory_batch_plan"]


def test_ffi_binds_every_new_header_symbol():
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    header = open(os.path.join(root, "include", "jolt_hip.h")).read()
    binding = open(os.path.join(root, "jolt_amd", "ffi.py")).read()
    declared = set(re.findall(r"\bint32_t\s+(jolt_(?:host_)?dory_(?:vec_\w+|g2_prepare_vec|products|batch_plan))\s*\(", header))
    assert declared == set(NEW_SYMBOLS)
    for name in NEW_SYMBOLS:
        assert f"lib().{name}(" in binding or f'_call("{name}", ' in binding, name
        assert hasattr(ffi.lib(), name), name
    assert C.sizeof(ffi.DoryItem) == 64  # jolt_dory_item: int32 + padding, seven 8-byte fields
    for method in ("dory_vec_upload", "dory_g2_prepare_vec", "dory_vec_scale_bases_add", "dory_vec_scale_vs_add", "dory_vec_fold_field", "dory_products"):
        assert callable(getattr(ffi.Context, method))
    from jolt_amd.dory_reduce import DoryReduce
    assert all(callable(getattr(DoryReduce, m)) for m in ("first_message", "apply_beta", "second_message", "apply_alpha"))
