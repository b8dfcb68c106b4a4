"""CPU-side checks of stage 8 over block-embedded polynomials (jolt_dory_evaluate_blocks, jolt_dory_fold_rows_blocks_many, jolt_host_dory_prove_batch_blocks): the ABI
surface in the header, the ctypes layer and the Rust declarations; the refusals that need no device; the workload's shape checks; and the GPU suite's expected-value
function for a block's claim held to the reference's `scale * claim` form, so that the tests' model is not only held to itself."""
import os
import re

import numpy as np
import pytest

import oracle_lib as O
from jolt_amd import ffi
from jolt_amd.workload import DeviceWorkload
from test_gpu_dory_step_blocks import block_claim, block_index, eq_at

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
R = O.R_MOD
ENTRIES = {"jolt_dory_evaluate_blocks": 9, "jolt_dory_fold_rows_blocks_many": 9, "jolt_host_dory_prove_batch_blocks": 27}  # name -> arity


def test_entries_are_declared_exported_and_bound_through_call():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jolt_hip.h")).read(), flags=re.S)
    ffi_rs = open(os.path.join(ROOT, "rust", "jolt-kernels-hip", "src", "ffi.rs")).read()
    ffi_py = open(os.path.join(ROOT, "jolt_amd", "ffi.py")).read()
    for name, arity in ENTRIES.items():
        c_decl = re.search(r"int32_t\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert c_decl and len(c_decl.group(1).split(",")) == arity, name
        rs_decl = re.search(r"pub fn %s\(([^;]*)\) -> i32;" % name, ffi_rs)
        assert rs_decl and len(rs_decl.group(1).split(",")) == arity, name
        assert hasattr(ffi.lib(), name), name
        assert getattr(ffi.lib(), name).argtypes is not None and len(getattr(ffi.lib(), name).argtypes) == arity  # declared to ctypes from the header
        assert '_call("%s", self, self.h, ' % name in ffi_py, name
    assert re.search(r"JOLT_DORY_ORDER_CYCLE_MAJOR = 0, JOLT_DORY_ORDER_ADDRESS_MAJOR = 1", header)
    assert ffi.DORY_ORDERS == {"cycle_major": 0, "address_major": 1}
    assert all(callable(getattr(ffi.Context, m)) for m in ("dory_evaluate_blocks", "dory_fold_rows_blocks_many", "dory_prove_batch"))
    # the old fold keeps its limit of eight and is a call of the wide form; the old batch opening is a call of the one body
    dory = open(os.path.join(ROOT, "jolt_amd", "csrc", "dory.hip")).read()
    old = dory[dory.index('extern "C" int32_t jolt_dory_fold_rows_blocks(jolt_ctx'):]
    assert "kFoldMaxDense) return JOLT_ERR_UNSUPPORTED" in old[:1200] and "return jolt_dory_fold_rows_blocks_many(" in old[:1200]
    assert int(re.search(r"constexpr size_t kBlocksMax = (\d+);", dory).group(1)) == 256
    scheme = open(os.path.join(ROOT, "jolt_amd", "csrc", "dory_scheme.hip")).read()
    assert scheme.count("return prove_batch_impl(") == 2 and scheme.count("jolt_host_opening_statement_absorb(t,") == 1


def test_refusals_that_need_no_device():
    lib = ffi.lib()
    assert lib.jolt_dory_evaluate_blocks(None, None, None, 1, None, 0, 0, 0, None) == 1
    assert lib.jolt_dory_fold_rows_blocks_many(None, None, None, 1, None, 3, None, None, None) == 1
    assert lib.jolt_host_dory_prove_batch_blocks(*([None] * 5), 1, None, None, 0, None, 0, None, None, 0, 4, 0, 0, None, None, 0, *([None] * 7)) == 1


def test_workload_shape_checks_need_no_device():
    check = DeviceWorkload._check_dory_shape
    blocks = check(6, 7, [10, 5, np.zeros((2, 4), dtype=np.uint64)], "cycle_major", 0)
    assert [b.shape for b in blocks] == [(1024, 4), (32, 4), (2, 4)]
    assert np.array_equal(check(6, 7, [5], "cycle_major", 0)[0], check(6, 7, [5], "address_major", 1)[0])  # drawn from the seed alone
    assert check(6, 7, [], "address_major", 2) == []            # grid 2^12: sigma = 6 = log_k + log_extra
    for args in ((6, 7, [11], "cycle_major", 0), (6, 7, [np.zeros((12, 4), dtype=np.uint64)], "cycle_major", 0), (6, 7, [], "row_major", 0), (6, 7, [], "cycle_major", 1),
                 (4, 7, [], "address_major", 2), (6, 7, [0] * 257, "cycle_major", 0), (6, 7, [], "address_major", -1)):
        with pytest.raises(ValueError):
            check(*args)


def test_the_gpu_suites_block_claim_is_the_scaled_claim_of_the_reference():
    """the second formulation: (the Lagrange factor of the high row and column coordinates at zero) x (the block's own multilinear evaluation at the low coordinates)
    -- entry.scale * opening_claim of crates/jolt-prover/src/dory/stages/stage8.rs:148-162 -- over random small shapes"""
    rng = np.random.default_rng(9500)
    draw = lambda n: [int.from_bytes(rng.bytes(40), "little") % R for _ in range(n)]  # noqa: E731
    seen = set()
    for _ in range(60):
        nu = int(rng.integers(0, 5))
        sigma = int(rng.integers(max(nu, 1), 6))
        m = int(rng.integers(0, nu + sigma + 1))
        lo, hi = max(0, m - nu), min(m, sigma)  # the sigma_d with which the block fits
        sigma_d = int(rng.integers(lo, hi + 1))
        log_rows = m - sigma_d
        table, point = draw(1 << m), draw(nu + sigma)
        row, col = point[:nu], point[nu:]
        scale = 1
        for p in row[:nu - log_rows] + col[:sigma - sigma_d]:
            scale = scale * (1 - p) % R
        own = row[nu - log_rows:] + col[sigma - sigma_d:]  # the block's own point: its row variables, then its column variables
        assert len(own) == m
        claim = sum(x * eq_at(own, i) for i, x in enumerate(table)) % R
        assert block_claim(table, sigma_d, sigma, point) == scale * claim % R
        if m:
            assert np.array_equal(O.to_mont([claim])[0], O.poly_evaluate(O.to_mont(table), O.to_mont(own)))  # eq_at is the oracle's indexing
        seen.add((log_rows == nu, sigma_d == sigma, m == 0))
    assert len(seen) >= 5
    assert all(block_index(sd, sg, i) == ffi.host_dory_block_index(sd, sg, i) for sd, sg, i in [(0, 3, 5), (2, 5, 13), (3, 3, 63), (1, 4, 0)])
