#!/usr/bin/env python3
"""The Dory opening ahead of the pairing rounds on the GPU (dory.hip): the lazy row fold against the materialised route, and the hint combination.

Fold, at the bench shape (log_t = 22, log_k = 4, sigma = 13; 4 + 32 one-hot columns and 2 dense columns as jolt_amd/workload.py commits, seeded random
contents): jolt_dory_fold_rows_grid against jolt_grid_joint_polynomial + jolt_address_fold, the only route to this vector without it.  Five alternated
pairs in one process after a warm-up of both, HIP events on the context's stream around synchronised work.
Combine: rows = 2^13, n_hints = 40.  The entry point takes host pointers, so the events around it include the transfers; the same bytes moved alone
(a table upload and download) are timed beside it and the difference is reported as the kernels' share.

Prints one JSON line per measurement and writes them all to profiles/dory_opening.json.

    python tools/bench_dory_opening.py [log_t]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from jolt_amd import ffi  # noqa: E402
from tools.bench_msm import rand_fr  # noqa: E402

BUCKET_KERNEL_ADDS_PER_S = 13.8e9  # mixed additions / s of the bucket-sum kernel (profiles/r06b_msm_bucket_rocprofv3_kernel_stats.csv)


def timed(ctx, fn):
    ctx.synchronize()
    ctx.timer_begin()
    out = fn()
    return out, ctx.timer_end()


def bench_fold(ctx, log_t, results):
    log_k, sigma = 4, (log_t + 4 + 1) // 2
    T, nu = 1 << log_t, log_k + log_t - sigma
    rng = np.random.default_rng(2026)
    counts, n_dense = [4, 32], 2
    srcs = []
    for n in counts:
        idx = rng.integers(0, 1 << log_k, size=(n, T), dtype=np.uint8)
        idx[rng.random((n, T)) < 0.1] = 0xFF
        srcs.append(ctx.onehot(idx, 1 << log_k))
    dense = [ctx.upload(rand_fr(T, 10 + d)) for d in range(n_dense)]
    gamma, dgamma = rand_fr(sum(counts), 3), rand_fr(n_dense, 4)
    left = ctx.upload(rand_fr(1 << nu, 5))

    def lazy():
        return ctx.dory_fold_rows_grid(srcs, gamma, dense, dgamma, log_k, sigma, left)

    def materialised():
        grid = ctx.grid_joint_polynomial(srcs, gamma, dense, dgamma, log_k)
        out = ctx.address_fold(grid, left)
        grid.free()
        return out

    a, b = lazy(), materialised()  # warm-up, and the two routes agree
    same = bool(np.array_equal(a.download(), b.download()))
    a.free()
    b.free()
    pairs = []
    for _ in range(5):
        o, t_lazy = timed(ctx, lazy)
        o.free()
        o, t_mat = timed(ctx, materialised)
        o.free()
        pairs.append({"lazy_ms": round(t_lazy, 4), "materialised_ms": round(t_mat, 4)})
    bytes_alg = sum(counts) * T + n_dense * T * 32 + (32 << nu) + (32 << sigma)
    best = min(p["lazy_ms"] for p in pairs)
    results.append({"what": "dory_fold_rows_grid", "log_t": log_t, "log_k": log_k, "sigma": sigma, "onehot_columns": sum(counts), "dense_columns": n_dense,
                    "routes_agree": same, "pairs": pairs, "lazy_faster_in_every_pair": all(p["lazy_ms"] < p["materialised_ms"] for p in pairs),
                    "algorithmic_bytes": bytes_alg, "materialised_grid_bytes": 32 << (log_k + log_t), "lazy_bytes_per_s": round(bytes_alg / best * 1e3)})
    print(json.dumps(results[-1]), flush=True)
    for t in dense + [left]:
        t.free()
    for s in srcs:
        s.free()


def bench_combine(ctx, results, rows=1 << 13, n_hints=40):
    g = np.zeros(12, dtype=np.uint64)
    one_q = [0xd35d438dc58f0d9d, 0x0a78eb28f5c70b3d, 0x666ea36f7879462c, 0x0e0a77c19a07df2f]
    two_q = [0xa6ba871b8b1e1b3a, 0x14f1d651eb8e167b, 0xccdd46def0f28c58, 0x1c14ef83340fbe5e]
    g[0:4], g[4:8], g[8:12] = one_q, two_q, one_q
    base = ctx.srs_setup_from_secret(rand_fr(1, 1)[0], rows, g).download()  # `rows` distinct points
    hints = [np.ascontiguousarray(np.roll(base, 17 * i + 1, axis=0)) for i in range(n_hints)]  # every row sees n_hints different points
    scalars = rand_fr(n_hints, 2)
    blob = np.zeros((rows * n_hints * 3, 4), dtype=np.uint64)  # the same bytes as the hints, for the transfers alone
    ctx.dory_combine_hints(hints, scalars)
    runs = []
    for _ in range(5):
        _, t_call = timed(ctx, lambda: ctx.dory_combine_hints(hints, scalars))

        def transfers():
            t = ctx.upload(blob)
            t2 = ctx.upload(blob[:rows * 3])
            t2.download()
            t.free()
            t2.free()
        _, t_copy = timed(ctx, transfers)
        runs.append({"call_ms": round(t_call, 3), "transfers_alone_ms": round(t_copy, 3)})
    ops = ffi.dory_combine_ops_per_row(n_hints)
    call = min(r["call_ms"] for r in runs)
    kernels = max(call - min(r["transfers_alone_ms"] for r in runs), 1e-3)
    results.append({"what": "dory_combine_hints", "rows": rows, "n_hints": n_hints, "window_bits": ffi.DORY_COMBINE_WINDOW, "runs": runs,
                    "with_transfers_ms": call, "without_transfers_ms": round(kernels, 3), "group_ops_per_row": ops,
                    "double_and_add_ops_per_row": 1.5 * 254 * n_hints, "group_ops_per_s": round(ops * rows / kernels * 1e3),
                    "bucket_kernel_mixed_adds_per_s": BUCKET_KERNEL_ADDS_PER_S})
    print(json.dumps(results[-1]), flush=True)


def main():
    log_t = int(sys.argv[1]) if len(sys.argv) > 1 else 22
    ctx = ffi.Context(0)
    results = []
    bench_fold(ctx, log_t, results)
    ctx.trim()
    bench_combine(ctx, results)
    ctx.close()
    out = os.path.join(ROOT, "profiles", "dory_opening.json")
    with open(out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
