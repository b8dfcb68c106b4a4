#!/usr/bin/env python3
"""One-hot sums over the L-form tables (k_grid_onehot_sum<true>): 16 columns of 2^20 cycles, K = 16 (an SRS of 2^24 points with window tables), 10 % cold
cycles, 5 commitments -- the kernel-trace target beside msm_bucket_one.py; then the pair table of that grid is built and the same 5 commitments run from it
(k_grid_onehot_sum_pairs), so that one trace holds both kernels on the same columns.   usage: onehot_sum_one.py"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from jolt_amd import ffi  # noqa: E402
from jolt_amd.workload import G1_GENERATOR, rand_fr  # noqa: E402

rng = np.random.default_rng(5)
ctx = ffi.Context(0)
K, T, N = 16, 1 << 20, 16
srs = ctx.srs_setup_from_secret(rand_fr(1, rng)[0], K * T, G1_GENERATOR)
ctx.srs_precompute_windows(srs, 0, 1)
idx = rng.integers(0, K, size=(N, T), dtype=np.uint8)
idx[rng.random((N, T)) < 0.1] = 0xFF
src = ctx.onehot(idx, K)
first = ctx.grid_commit_onehot(srs, src)
for _ in range(4):
    ctx.synchronize()
    t0 = time.perf_counter()
    got = ctx.grid_commit_onehot(srs, src)
    print("commit ms", round((time.perf_counter() - t0) * 1e3, 3), flush=True)
    assert all(ffi.host_g1_eq(got[p], first[p]) for p in range(N))
t0 = time.perf_counter()
built = ctx.srs_precompute_grid_pairs(srs, K, T, (0,))
print("pair table bytes", built[0], "build ms", round((time.perf_counter() - t0) * 1e3, 1), flush=True)
for _ in range(5 if built[0] else 0):
    ctx.synchronize()
    t0 = time.perf_counter()
    got = ctx.grid_commit_onehot(srs, src)
    print("commit from pairs ms", round((time.perf_counter() - t0) * 1e3, 3), flush=True)
    assert all(ffi.host_g1_eq(got[p], first[p]) for p in range(N))
print("point", [int(x) for x in np.asarray(first[0]).reshape(-1)[:4]])
