"""CPU-side checks of the witness commitment on the device (jolt_dory_hints_onehot / _rows, jolt_amd/dory_commit.py): the entries are declared, exported and bound;
the per-lane routine of the hint kernel -- batched inversion by Montgomery's trick -- against the oracle through its host form; the kernel's index map against
ffi.dory_onehot_hint.  Points are compared as group elements, the normalised representative bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle_lib as O
from jolt_amd import ffi

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
ENTRIES = ["jolt_dory_hints_onehot", "jolt_dory_hints_rows", "jolt_host_dory_g1_normalise"]
SENTINEL = 0xA5A5A5A5A5A5A5A5


def test_entries_are_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jolt_hip.h")).read(), flags=re.S)
    ffi_rs = open(os.path.join(ROOT, "rust", "jolt-kernels-hip", "src", "ffi.rs")).read()
    for name in ENTRIES + ["jolt_host_dory_hint_map"]:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(ffi.lib(), name), name
        assert re.search(r"pub fn %s\(" % name, ffi_rs), name
    assert callable(ffi.Context.dory_hints_onehot) and callable(ffi.Context.dory_hints_rows) and callable(ffi.host_dory_g1_normalise)
    # the names stay outside the set tests/test_dory_reduce_cpu.py pins
    assert not any(re.fullmatch(r"jolt_(host_)?dory_(vec_\w+|g2_prepare_vec|products|batch_plan)", n) for n in ENTRIES + ["jolt_host_dory_hint_map"])


def test_module_imports_without_a_gpu():
    from jolt_amd import dory_commit
    assert callable(dory_commit.DoryWitnessCommitment)


# ------------------------------------------------------------------------------------------------------ the batched inversion
@pytest.fixture(scope="module")
def points():
    """80 multiples of the generator with Z of their own: an add / double chain of the oracle's Jacobian formulas (never normalised)"""
    g = O.g1_generator()
    out, p = [], O.g1_double(g)
    for i in range(80):
        p = O.g1_double(p) if i % 3 == 0 else O.g1_add(p, g)
        out.append(p)
    one = O.g1_identity()[0:4]
    assert sum(1 for q in out if not np.array_equal(q[8:12], one)) >= 79  # the chain does not hand back Z = 1
    return np.stack(out)


def check_normalised(got, src):
    ident = O.g1_identity()
    one = ident[0:4]
    assert got.shape == src.shape
    for i in range(src.shape[0]):
        if not src[i][8:12].any():
            assert np.array_equal(got[i], ident), i  # bit for bit (1, 1, 0)
        else:
            assert np.array_equal(got[i][8:12], one), i  # bit for bit the Montgomery one
            assert O.g1_on_curve(got[i]) and O.g1_eq(got[i], src[i]), i


@pytest.mark.parametrize("run", [1, 4, 64])
@pytest.mark.parametrize("n", [1, 2, 7, 64 + 3])
def test_normalise_against_the_oracle(points, n, run):
    src = points[:n].copy()
    check_normalised(ffi.host_dory_g1_normalise(src, run), src)


@pytest.mark.parametrize("run", [1, 4, 64])
def test_normalise_with_identities_in_the_runs(points, run):
    """identities first, last and in the middle of a run; a run that is all identities; an input that is all identities"""
    n = 64 + 3
    ident = O.g1_identity()
    odd_identity = np.concatenate([points[5][0:8], np.zeros(4, dtype=np.uint64)])  # z = 0 with x, y of some point: still the identity, written back as (1, 1, 0)
    src = points[:n].copy()
    first, last, middle = (0, run - 1, run // 2) if run > 1 else (0, 2, 4)
    for i in {first, last, middle, n - 1}:
        src[i] = ident
    src[first] = odd_identity
    check_normalised(ffi.host_dory_g1_normalise(src, run), src)
    src = points[:n].copy()
    lo = 2 * run if 3 * run <= n else 0  # the third run, or with run = 64 the first
    src[lo:lo + run] = ident
    src[lo] = odd_identity
    check_normalised(ffi.host_dory_g1_normalise(src, run), src)
    src = np.stack([ident] * n)
    src[3] = odd_identity
    check_normalised(ffi.host_dory_g1_normalise(src, run), src)


def test_normalise_refuses_null_pointers_and_writes_nothing(points):
    lib = ffi.lib()
    src = points[:4].copy()
    out = np.full((4, 12), SENTINEL, dtype=np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.jolt_host_dory_g1_normalise(None, C.c_size_t(4), C.c_size_t(2), p(out)) == 1
    assert lib.jolt_host_dory_g1_normalise(p(src), C.c_size_t(4), C.c_size_t(2), None) == 1
    assert lib.jolt_host_dory_g1_normalise(p(src), C.c_size_t(4), C.c_size_t(0), p(out)) == 1
    assert (out == SENTINEL).all()
    assert lib.jolt_host_dory_g1_normalise(None, C.c_size_t(0), C.c_size_t(2), None) == 0
    assert (out == SENTINEL).all()
    assert lib.jolt_host_dory_g1_normalise(p(src), C.c_size_t(4), C.c_size_t(2), p(out)) == 0
    check_normalised(out, src)


# ------------------------------------------------------------------------------------------------------ the index map
@pytest.mark.parametrize("batch", [8, 3, 1])
def test_hint_index_map_is_the_transposition_of_the_reference(batch):
    """K = 3, chunks = 4, 2 columns (not square: a transposed index cannot coincide with the plain one).  The workspace of a launch set holds K + 1 buckets per
    window; labelled points go through the kernel's map, launch set by launch set (8 windows at once, 3 -- cuts inside a column and between columns -- and 1),
    and must land where ffi.dory_onehot_hint puts the chunk-major commitments of each column."""
    K, chunks, cols = 3, 4, 2
    windows = cols * chunks
    label = lambda col, chunk, row: 1000 * col + 10 * chunk + row + 1  # noqa: E731
    hint = np.zeros(cols * K * chunks, dtype=np.int64)
    written = np.zeros_like(hint)
    for w0 in range(0, windows, batch):
        V = min(batch, windows - w0)
        workspace = np.full(V * (K + 1), -1, dtype=np.int64)  # bucket 0 of every window: the cold cycles, never read
        for v in range(V):
            col, chunk = divmod(w0 + v, chunks)
            for row in range(K):
                workspace[v * (K + 1) + row + 1] = label(col, chunk, row)
        for e in range(V * K):
            src, dst = ffi.host_dory_hint_map(K, chunks, w0, e)
            assert 0 <= src < V * (K + 1) and 0 <= dst < hint.shape[0]
            assert workspace[src] > 0
            hint[dst] = workspace[src]
            written[dst] += 1
    assert (written == 1).all()
    for col in range(cols):
        chunk_major = np.array([[[label(col, chunk, row)] for row in range(K)] for chunk in range(chunks)], dtype=np.uint64)  # dory_commit_onehot's (chunks, k, .)
        want = ffi.dory_onehot_hint(chunk_major).reshape(-1)
        assert np.array_equal(hint[col * K * chunks:(col + 1) * K * chunks].astype(np.uint64), want)
        # and the formula of the header: hint[row * chunks + chunk] = out[chunk * k + row]
        assert all(want[row * chunks + chunk] == label(col, chunk, row) for row in range(K) for chunk in range(chunks))
