#!/usr/bin/env python3
"""The Dory commitment of a witness and the opening's row fold in the two trace placements, on the same columns in one process.

    am  address-major   DoryWitnessCommitment(order="address_major"): one jolt_dory_hints_onehot_am call per source, one jolt_dory_hints_rows_am call per dense
                        column (hints), one jolt_dory_products call (tier2), jolt_dory_fold_rows_grid_am (fold)
    cm  cycle-major     the default order: jolt_dory_hints_onehot / _rows (hints), one jolt_dory_products call (tier2), jolt_dory_fold_rows_grid (fold)

Shape: the columns of tools/bench_dory_commit.py -- 36 one-hot columns of K = 16 in three sources of 12, 75 % of the cycles hot, and 2 dense u64 columns, over
T = 2^log_t cycles in rows of 2^sigma; every column has K T / 2^sigma rows in either placement.  Gamma1 and Gamma2 synthetic (multiples of the generators).  Wall
milliseconds, each phase ending with the context drained; per phase the smallest of five runs after one warm-up run; ratio = cm_hints / am_hints.  Every shape runs
in a child process of its own under a time limit, and a shape that fails or runs out of time ends the measurement.

    python tools/bench_dory_commit_am.py [--out profiles/dory_commit_am.txt] [--shapes 20:12,22:13] [--limit 420]"""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

REPEATS = 5
LOG_K, SOURCES, PER_SOURCE, N_DENSE = 4, 3, 12, 2
K = 1 << LOG_K
PHASES = ["am_hints", "am_tier2", "am_fold", "cm_hints", "cm_tier2", "cm_fold"]


def worker(log_t, sigma):
    from jolt_amd import ffi
    from jolt_amd.dory_commit import DoryWitnessCommitment
    from jolt_amd.dory_open import DorySetup
    from tools.bench_dory_routines import g1_points, g2_points
    from util import rand_fr

    T, width = 1 << log_t, 1 << sigma
    rows = K * (T >> sigma)  # per column, in both placements
    n = max(width, rows)
    ctx = ffi.Context(0)
    pool = g1_points(ctx, n + 1)
    g2s = g2_points(n + 1)
    setup = DorySetup(ctx, pool[:n], g2s[:n], pool[n], g2s[n])
    srs = ctx.srs_upload(pool[:width])
    rng = np.random.default_rng(log_t)
    sources = []
    for _ in range(SOURCES):
        idx = rng.integers(0, K, size=(PER_SOURCE, T)).astype(np.uint8)
        idx[rng.random((PER_SOURCE, T)) < 0.25] = 0xFF
        sources.append(ctx.onehot(idx, K))
    dense = [ctx.ints(rng.integers(0, 2**64, size=T, dtype=np.uint64)) for _ in range(N_DENSE)]
    dense_tables = [ctx.table_from_ints(d) for d in dense]
    gamma, dgamma = rand_fr(SOURCES * PER_SOURCE, 3), rand_fr(N_DENSE, 4)
    left = ctx.upload(rand_fr(rows, 5))

    def lap(marks):
        ctx.synchronize()
        marks.append(time.perf_counter())
        return (marks[-1] - marks[-2]) * 1e3

    def one_order(ms, tag, **kwargs):
        ctx.synchronize()
        marks = [time.perf_counter()]
        commitment = DoryWitnessCommitment(setup, srs, sources, dense, sigma, **kwargs)
        ms[tag + "_hints"] = lap(marks)
        commitment.commit()
        ms[tag + "_tier2"] = lap(marks)
        if tag == "am":
            v = ctx.dory_fold_rows_grid_am(sources, gamma, dense_tables, dgamma, LOG_K, 0, sigma, left)
        else:
            v = ctx.dory_fold_rows_grid(sources, gamma, dense_tables, dgamma, LOG_K, sigma, left)
        ms[tag + "_fold"] = lap(marks)
        v.free()
        commitment.close()

    def one_run():
        ms = {}
        one_order(ms, "am", order="address_major", log_k=LOG_K)
        one_order(ms, "cm")
        return ms

    runs = [one_run() for _ in range(REPEATS + 1)][1:]
    best = {p: min(r[p] for r in runs) for p in PHASES}
    print("ROW %-6d %-6d %s %8.2f" % (log_t, sigma, " ".join("%12.3f" % best[p] for p in PHASES), best["cm_hints"] / best["am_hints"]), flush=True)
    for t in sources + dense + dense_tables + [left]:
        t.free()
    setup.close()
    ctx.close()


def main():
    arg = lambda name, default: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default  # noqa: E731
    if "--worker" in sys.argv:
        log_t, sigma = arg("--worker", "20:12").split(":")
        worker(int(log_t), int(sigma))
        return
    out_path = arg("--out", os.path.join(ROOT, "profiles", "dory_commit_am.txt"))
    shapes = [tuple(int(v) for v in s.split(":")) for s in arg("--shapes", "20:12,22:13").split(",")]
    limit = int(arg("--limit", "420"))
    lines = ["# tools/bench_dory_commit_am.py: wall milliseconds, MI355X; per phase the smallest of %d runs after a warm-up run, every phase ending with the context drained" % REPEATS,
             "# %d one-hot columns of K = %d in %d sources and %d dense u64 columns over 2^log_t cycles, rows of 2^sigma; both placements in one process on the same columns" % (SOURCES * PER_SOURCE, K, SOURCES, N_DENSE),
             "# am = address-major (jolt_dory_hints_onehot_am / _rows_am, jolt_dory_products, jolt_dory_fold_rows_grid_am); cm = cycle-major (jolt_dory_hints_onehot / _rows,",
             "# jolt_dory_products, jolt_dory_fold_rows_grid); ratio = cm_hints / am_hints",
             "%-6s %-6s %s %8s" % ("log_t", "sigma", " ".join("%12s" % p for p in PHASES), "ratio")]
    for log_t, sigma in shapes:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "%d:%d" % (log_t, sigma)], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            lines.append("# log_t = %d: no result within %d s; the measurement ends here" % (log_t, limit))
            print(lines[-1], flush=True)
            break
        rows = [ln[4:] for ln in r.stdout.splitlines() if ln.startswith("ROW ")]
        if r.returncode != 0 or not rows:
            lines.append("# log_t = %d: the worker ended with status %d; the measurement ends here" % (log_t, r.returncode))
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
