#!/usr/bin/env python3
"""Dory row commitments of a device FIELD table and the block row fold, against the routes that existed before them.

    rows_fr     jolt_dory_commit_rows_fr over the whole table, full-width (254-bit) scalars: one call, every row
    msm_per_row the only earlier route for such a table: one jolt_dory_g1_msm per row through host pointers (bases and scalars on the host already; the copies
                of the call are part of it)
    rows_fr_u64 jolt_dory_commit_rows_fr over a table of u64-range values (the OR-reduction cuts the windows to 65 bits)
    rows_u64    jolt_dory_commit_rows on the same values as jolt_ints
    fold        jolt_dory_fold_rows_blocks of the whole table (sigma_d = sigma, no base): the dense vector_matrix_product; GB/s = the bytes the design reads and
                writes, (2^n + 2^nu + 2^sigma (1 + 2 slices)) * 32, over the time

Shape: a polynomial of 2^n field elements as its balanced matrix, sigma = ceil(n / 2), 2^(n - sigma) rows.  Wall milliseconds, every phase ending with the context
drained; per phase the smallest of five runs after one warm-up run.  Every shape runs in a child process of its own under a time limit, and a shape that fails or
runs out of time ends the measurement.  No threshold is set.

    python tools/bench_dory_rows_fr.py [--out profiles/dory_rows_fr.txt] [--shapes 16,20,22] [--limit 420]"""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

REPEATS = 5
PHASES = ["rows_fr", "msm_per_row", "rows_fr_u64", "rows_u64", "fold"]


def worker(n):
    from jolt_amd import ffi
    from tools.bench_dory_routines import g1_points
    from util import rand_fr

    sigma = (n + 1) // 2
    nu = n - sigma
    width, rows = 1 << sigma, 1 << nu
    ctx = ffi.Context(0)
    bases = g1_points(ctx, width)
    srs = ctx.srs_upload(bases)
    rng = np.random.default_rng(n)
    # full-width scalars: random words under the modulus' top word are canonical Montgomery forms of uniformly random elements
    full = rng.integers(0, 2**64, size=(1 << n, 4), dtype=np.uint64)
    full[:, 3] >>= np.uint64(4)
    table = ctx.upload(full)
    small = rng.integers(0, 2**64, size=1 << n, dtype=np.uint64)
    ints = ctx.ints(small)
    small_table = ctx.table_from_ints(ints)
    left = ctx.upload(rand_fr(rows, 5))
    one = ffi.host_fr_from_u64(1)

    def timed(fn):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def per_row():
        for r in range(rows):
            ctx.dory_g1_msm(bases, full[r * width:(r + 1) * width])

    def fold():
        ctx.dory_fold_rows_blocks([table], [sigma], [one], sigma, left).free()

    phases = {"rows_fr": lambda: ctx.dory_commit_rows_fr(srs, table, width), "msm_per_row": per_row,
              "rows_fr_u64": lambda: ctx.dory_commit_rows_fr(srs, small_table, width), "rows_u64": lambda: ctx.dory_commit_rows(srs, ints, width), "fold": fold}
    best = {p: min([timed(phases[p]) for _ in range(REPEATS + 1)][1:]) for p in PHASES}
    slices = (rows + ffi.DORY_BLOCK_FOLD_SLICE - 1) // ffi.DORY_BLOCK_FOLD_SLICE
    fold_bytes = 32 * ((1 << n) + rows + width * (1 + (2 * slices if slices > 1 else 0)))
    print("ROW %-4d %-6d %-6d %s %10.1f" % (n, sigma, rows, " ".join("%12.3f" % best[p] for p in PHASES), fold_bytes / best["fold"] / 1e6), flush=True)
    for t in (table, small_table, ints, left, srs):
        t.free()
    ctx.close()


def main():
    arg = lambda name, default: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default  # noqa: E731
    if "--worker" in sys.argv:
        worker(int(arg("--worker", "16")))
        return
    out_path = arg("--out", os.path.join(ROOT, "profiles", "dory_rows_fr.txt"))
    shapes = [int(v) for v in arg("--shapes", "16,20,22").split(",")]
    limit = int(arg("--limit", "420"))
    lines = ["# python tools/bench_dory_rows_fr.py --shapes %s --limit %d" % (",".join(str(v) for v in shapes), limit),
             "# tools/bench_dory_rows_fr.py: wall milliseconds, MI355X; per phase the smallest of %d runs after a warm-up run, every phase ending with the context drained" % REPEATS,
             "# a polynomial of 2^n field elements as 2^(n - sigma) rows of 2^sigma, sigma = ceil(n / 2)",
             "# rows_fr = jolt_dory_commit_rows_fr, 254-bit scalars; msm_per_row = one jolt_dory_g1_msm per row on the same scalars (the route before it);",
             "# rows_fr_u64 = jolt_dory_commit_rows_fr on u64-range values; rows_u64 = jolt_dory_commit_rows on the same integers; fold = jolt_dory_fold_rows_blocks of the",
             "# whole table, fold_GB/s = its design byte count over its time",
             "%-4s %-6s %-6s %s %10s" % ("n", "sigma", "rows", " ".join("%12s" % p for p in PHASES), "fold_GB/s")]
    for n in shapes:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", str(n)], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            lines.append("# n = %d: no result within %d s; the measurement ends here" % (n, limit))
            print(lines[-1], flush=True)
            break
        rows = [ln[4:] for ln in r.stdout.splitlines() if ln.startswith("ROW ")]
        if r.returncode != 0 or not rows:
            lines.append("# n = %d: the worker ended with status %d; the measurement ends here" % (n, r.returncode))
            print(lines[-1], flush=True)
            print(r.stderr[-2000:], flush=True)
            break
        lines.extend(rows)
        print(rows[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
