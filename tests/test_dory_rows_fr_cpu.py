"""CPU-side checks of Dory for polynomials held as field elements (jolt_dory_commit_rows_fr / _hints_rows_fr / _fold_rows_blocks, jolt_amd/dory_scheme.py,
DoryWitnessCommitment(blocks=...)): the signed digits and the window plan of the field rows through the code the kernels run, the block embedding's index formula,
the refusals that need no device, the Python layer's shape checks, and the ABI surface."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle_lib as O
from jolt_amd import ffi

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
R = O.R_MOD
ENTRIES = ["jolt_dory_commit_rows_fr", "jolt_dory_hints_rows_fr", "jolt_dory_fold_rows_blocks", "jolt_host_dory_fr_digits", "jolt_host_dory_rows_fr_plan",
           "jolt_host_dory_block_index"]
MAX_WINDOWS = 48  # kMaxRowWindows of dory.hip


def test_entries_are_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jolt_hip.h")).read(), flags=re.S)
    ffi_rs = open(os.path.join(ROOT, "rust", "jolt-kernels-hip", "src", "ffi.rs")).read()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(ffi.lib(), name), name
        assert re.search(r"pub fn %s\(" % name, ffi_rs), name
    assert all(callable(getattr(ffi.Context, m)) for m in ("dory_commit_rows_fr", "dory_hints_rows_fr", "dory_fold_rows_blocks"))
    # the Rust crate calls the two device entries a prover needs, with the header's arity (tests/test_abi_cpu.py checks every call's arity)
    resident = open(os.path.join(ROOT, "rust", "jolt-kernels-hip", "src", "dory_resident.rs")).read()
    assert "ffi::jolt_dory_hints_rows_fr(" in resident and "ffi::jolt_dory_fold_rows_blocks(" in resident
    src = open(os.path.join(ROOT, "jolt_amd", "csrc", "dory.hip")).read()
    assert int(re.search(r"constexpr int kMaxRowWindows = (\d+);", src).group(1)) == MAX_WINDOWS
    assert int(re.search(r"constexpr uint32_t kBlockFoldSlice = (\d+);", src).group(1)) == ffi.DORY_BLOCK_FOLD_SLICE


# ------------------------------------------------------------------------------------------------------ digits
from corner_grids import dory_fr_scalars as scalars  # noqa: E402


@pytest.mark.parametrize("c", range(3, 14))
def test_digits_recombine_to_the_scalar_or_to_the_scalar_minus_r(c):
    """sum_w +-digit_w 2^(c w) is s, or s - r when the magnitude r - s was taken; every digit in [-2^(c-1), 2^(c-1)].  Every input at every c, over the
    ceil(255 / c) windows of a full-width magnitude and its carry: up to 85 at c = 3, which the host form takes though the device's row fold holds 48."""
    B = 1 << (c - 1)
    W = (254 + c) // c
    assert W * c >= 255 and (c >= 6) == (W <= MAX_WINDOWS)
    values = scalars()
    assert len(values) == 207 and sum(min(s, R - s).bit_length() > 250 for s in values) > 100
    for s, m in zip(values, O.to_mont(values)):
        magnitude = min(s, R - s)
        digits, negative = ffi.host_dory_fr_digits(m, c, W)
        assert len(digits) == W and all(-B <= d <= B for d in digits)
        assert negative == (R - s < s)
        total = sum(d << (c * w) for w, d in enumerate(digits))
        assert total == magnitude
        assert (-total if negative else total) == (s - R if negative else s)


def test_digit_refusals():
    lib = ffi.lib()
    one = O.to_mont([1])
    out, neg = np.zeros(86, dtype=np.uint32), C.c_uint32(7)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    call = lambda s, c, W, o=out: lib.jolt_host_dory_fr_digits(s, C.c_int32(c), C.c_int32(W), p(o) if o is not None else None, C.byref(neg))  # noqa: E731
    assert call(None, 6, 43) == 1 and call(p(one), 6, 43, None) == 1
    assert call(p(one), 2, 43) == 1 and call(p(one), 14, 20) == 1 and call(p(one), 6, 0) == 1 and call(p(one), 3, 86) == 1
    bad = np.full((1, 4), 2**64 - 1, dtype=np.uint64)
    assert call(p(bad), 6, 43) == 1  # not a canonical field element
    assert not out.any() and neg.value == 7
    assert call(p(one), 6, 43) == 0 and out[0] == 1 and neg.value == 0
    assert call(p(one), 3, 85) == 0 and out[0] == 1 and not out[1:].any()


# ------------------------------------------------------------------------------------------------------ plan
def integer_rule(bits, width):
    c = max(3, min(13, width.bit_length() - 1 - 4))
    return c, (bits + c) // c


@pytest.mark.parametrize("log_width", range(0, 21))
def test_plan_covers_the_bit_length_and_fits_the_row_fold(log_width):
    width = 1 << log_width
    for bits in list(range(1, 255)):
        c, W = ffi.host_dory_rows_fr_plan(bits, width)
        assert 3 <= c <= 13 and 1 <= W <= MAX_WINDOWS
        assert W * c >= bits + 1            # the bit length and the signed-digit carry
        assert (W - 1) * c < bits + 1       # and no window more
        if bits <= 128:
            assert (c, W) == integer_rule(bits, width)  # the integer rows' plan for the same magnitudes and width
        assert c >= integer_rule(bits, width)[0]
        if integer_rule(bits, width)[1] <= MAX_WINDOWS:
            assert (c, W) == integer_rule(bits, width)  # digits widen only where the rule does not fit
    assert ffi.host_dory_rows_fr_plan(254, 1) == (6, 43)


def test_plan_is_the_integer_rows_rule_for_integer_magnitudes():
    """The integer rows (jolt_dory_commit_rows / _hints_rows) take their windows from this plan and keep no rule of their own: for every bit length an integer
    magnitude has and every row width up to 2^14 it gives c = clamp(wl - 4, 3, 13), W = (bits + c) // c, and never more windows than the row fold holds."""
    for wl in range(0, 15):
        for bits in range(1, 129):
            c = min(max(wl - 4, 3), 13)
            W = (bits + c) // c
            assert ffi.host_dory_rows_fr_plan(bits, 1 << wl) == (c, W), (bits, wl)
            assert W <= MAX_WINDOWS


def test_plan_refusals():
    lib = ffi.lib()
    c, W = C.c_int32(-1), C.c_int32(-1)
    call = lambda bits, width, pc=C.byref(c), pw=C.byref(W): lib.jolt_host_dory_rows_fr_plan(C.c_uint32(bits), C.c_size_t(width), pc, pw)  # noqa: E731
    assert call(0, 8) == 1 and call(255, 8) == 1 and call(64, 24) == 1 and call(64, 0) == 1 and call(64, 8, None) == 1 and call(64, 8, C.byref(c), None) == 1
    assert (c.value, W.value) == (-1, -1)
    assert call(64, 8) == 0 and (c.value, W.value) == (3, 22)


# ------------------------------------------------------------------------------------------------------ block index
@pytest.mark.parametrize("sigma_table,sigma_grid,m", [(0, 0, 3), (0, 4, 3), (2, 2, 5), (2, 5, 4), (3, 5, 5), (5, 5, 10)])
def test_block_index_over_every_coefficient(sigma_table, sigma_grid, m):
    seen = set()
    for i in range(1 << m):
        at = ffi.host_dory_block_index(sigma_table, sigma_grid, i)
        assert at == ((i >> sigma_table) << sigma_grid) | (i & ((1 << sigma_table) - 1))
        row, col = at >> sigma_grid, at & ((1 << sigma_grid) - 1)
        assert row == i >> sigma_table and col == i & ((1 << sigma_table) - 1) and col < 1 << sigma_table  # top-left: row r of the block is row r of the grid
        seen.add(at)
    assert len(seen) == 1 << m


def test_block_index_refusals():
    lib = ffi.lib()
    out = C.c_size_t(99)
    call = lambda st, sg, i, o=C.byref(out): lib.jolt_host_dory_block_index(C.c_uint32(st), C.c_uint32(sg), C.c_size_t(i), o)  # noqa: E731
    assert call(3, 2, 0) == 1 and call(0, 64, 0) == 1 and call(0, 4, 0, None) == 1
    assert call(0, 63, 2) == 1  # row 2 of a grid of 2^63 columns: past 64 bits
    assert out.value == 99
    assert call(1, 4, 3) == 0 and out.value == 17


# ------------------------------------------------------------------------------------------------------ refusals without a device
def test_device_entries_refuse_null_handles_without_a_device():
    lib = ffi.lib()
    z = C.c_size_t
    out = np.full((2, 12), 0xA5, dtype=np.uint64)
    assert lib.jolt_dory_commit_rows_fr(None, None, None, z(0), z(8), z(4), out.ctypes.data_as(C.c_void_p)) == 1
    assert lib.jolt_dory_hints_rows_fr(None, None, None, z(0), z(8), z(4), None, z(0)) == 1
    res = C.c_void_p()
    assert lib.jolt_dory_fold_rows_blocks(None, None, None, z(1), None, C.c_uint32(3), None, None, C.byref(res)) == 1
    assert (out == 0xA5).all() and res.value is None


# ------------------------------------------------------------------------------------------------------ the Python layer's shapes
class FakeTable:
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


class FakeSetup:
    """a setup with no context: a constructor that gets past its shape checks fails on the first device call"""
    ctx = None

    def __init__(self, n):
        self.n = n


def test_matrix_shapes():
    from jolt_amd import dory_scheme
    from jolt_amd.dory_commit import block_sigma
    for n in range(0, 27):
        nu, sigma = dory_scheme.matrix_shape(1 << n)
        assert sigma == (n + 1) // 2 and nu + sigma == n and 0 <= sigma - nu <= 1  # scheme.rs:242-243
        assert block_sigma(1 << n) == sigma                                         # BlockOpeningPoly::new: the same balanced split
    for bad in (0, 3, 12, 48):
        with pytest.raises(ValueError):
            dory_scheme.matrix_shape(bad)
        with pytest.raises(ValueError):
            block_sigma(bad)


def test_scheme_checks_shapes_before_anything_is_enqueued():
    from jolt_amd import dory_scheme
    setup = FakeSetup(8)
    for table, srs in ((FakeTable(12), FakeTable(8)),     # not a power of two
                       (FakeTable(256), FakeTable(16)),   # sigma = 4 against a setup of 8
                       (FakeTable(64), FakeTable(4))):    # sigma = 3 against an SRS of 4
        with pytest.raises(ValueError):
            dory_scheme.commit(setup, srs, table)
    with pytest.raises(ValueError):
        dory_scheme.open(setup, FakeTable(12), None, np.zeros((4, 4), dtype=np.uint64))
    with pytest.raises(ValueError):
        dory_scheme.open(setup, FakeTable(16), None, np.zeros((3, 4), dtype=np.uint64))  # a point of the wrong length
    with pytest.raises(AttributeError):
        dory_scheme.commit(setup, FakeTable(8), FakeTable(16))  # a fitting shape reaches the device: the checks came first


def test_witness_commitment_checks_block_shapes_before_anything_is_enqueued():
    from jolt_amd.dory_commit import DoryWitnessCommitment
    setup, srs = FakeSetup(4), FakeTable(8)
    for blocks in ([FakeTable(12)],                  # not a power of two
                   [FakeTable(16), FakeTable(0)],
                   [FakeTable(256)],                 # 2^4 columns against an SRS of 8
                   [FakeTable(16), FakeTable(128)]): # 2^(7 - 4) rows against 4 Gamma2 bases
        for order, kw in (("cycle_major", {}), ("address_major", dict(log_k=2))):
            with pytest.raises(ValueError):
                DoryWitnessCommitment(setup, srs, [], [], 3, order=order, blocks=blocks, **kw)
    with pytest.raises(ValueError):
        DoryWitnessCommitment(setup, srs, [], [], 3, blocks=())  # still no column at all
    with pytest.raises(AttributeError):
        DoryWitnessCommitment(setup, srs, [], [], 3, blocks=[FakeTable(16)])  # blocks alone are a witness: this one reaches the device
