#!/usr/bin/env python3
"""The Dory commitment of a witness on the GPU, two ways on the same inputs in one process.

    (a) resident   jolt_amd/dory_commit.py: one jolt_dory_hints_onehot call per source, one jolt_dory_hints_rows call per dense column, the hints left on the device
                   (hints), then every tier-2 commitment from ONE jolt_dory_products call (tier2)
    (b) per column the route before it: jolt_dory_commit_onehot / jolt_dory_commit_rows per column with their read-back, ffi.dory_onehot_hint on the host (tier1),
                   jolt_dory_vec_upload of every hint (upload), one dory_commit_tier2 call per column (tier2)

Shape: 36 one-hot columns of K = 16 in three sources of 12, 75 % of the cycles hot, and 2 dense u64 columns, over T = 2^log_t cycles in rows of 2^sigma; Gamma1 and
Gamma2 synthetic (multiples of the generators).  Wall milliseconds, each phase ending with the context drained; per phase the smallest of five runs after one warm-up
run, `total` the smallest sum of one run; ratio = total (b) / total (a).  Every shape runs in a child process of its own under a time limit, and a shape that fails
or runs out of time ends the measurement.

    python tools/bench_dory_commit.py [--out profiles/dory_commit.txt] [--shapes 20:12,22:13] [--limit 420]"""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

REPEATS = 5
K, SOURCES, PER_SOURCE, N_DENSE = 16, 3, 12, 2
PHASES = ["a_hints", "a_tier2", "a_total", "b_tier1", "b_upload", "b_tier2", "b_total"]


def worker(log_t, sigma):
    from jolt_amd import ffi
    from jolt_amd.dory_commit import DoryWitnessCommitment
    from jolt_amd.dory_open import DorySetup, dory_commit_tier2
    from tools.bench_dory_routines import g1_points, g2_points

    T, width = 1 << log_t, 1 << sigma
    n = max(width, K * (T >> sigma))  # Gamma2 bases: the rows of a one-hot column
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

    def lap(marks):
        ctx.synchronize()
        marks.append(time.perf_counter())
        return (marks[-1] - marks[-2]) * 1e3

    def one_run():
        ms = {}
        ctx.synchronize()
        marks = [time.perf_counter()]
        commitment = DoryWitnessCommitment(setup, srs, sources, dense, sigma)
        ms["a_hints"] = lap(marks)
        new = commitment.commit()
        ms["a_tier2"] = lap(marks)
        ms["a_total"] = ms["a_hints"] + ms["a_tier2"]
        commitment.close()
        ctx.synchronize()
        marks = [time.perf_counter()]
        host_hints = [ffi.dory_onehot_hint(ctx.dory_commit_onehot(srs, s, p, width)) for s in sources for p in range(PER_SOURCE)]
        host_hints += [np.array(ctx.dory_commit_rows(srs, d, width)) for d in dense]
        ms["b_tier1"] = lap(marks)
        vecs = [ctx.dory_vec_upload(ffi.DORY_KIND_G1, h) for h in host_hints]
        ms["b_upload"] = lap(marks)
        old = [dory_commit_tier2(setup, v) for v in vecs]
        ms["b_tier2"] = lap(marks)
        ms["b_total"] = ms["b_tier1"] + ms["b_upload"] + ms["b_tier2"]
        for v in vecs:
            v.free()
        if not all(np.array_equal(x, y) for x, y in zip(new, old)):
            raise RuntimeError("the two routes disagree on a commitment")
        return ms

    runs = [one_run() for _ in range(REPEATS + 1)][1:]
    best = {p: min(r[p] for r in runs) for p in PHASES}
    print("ROW %-6d %-6d %s %8.2f" % (log_t, sigma, " ".join("%12.3f" % best[p] for p in PHASES), best["b_total"] / best["a_total"]), flush=True)
    for t in sources + dense:
        t.free()
    setup.close()
    ctx.close()


def main():
    arg = lambda name, default: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default  # noqa: E731
    if "--worker" in sys.argv:
        log_t, sigma = arg("--worker", "20:12").split(":")
        worker(int(log_t), int(sigma))
        return
    out_path = arg("--out", os.path.join(ROOT, "profiles", "dory_commit.txt"))
    shapes = [tuple(int(v) for v in s.split(":")) for s in arg("--shapes", "20:12,22:13").split(",")]
    limit = int(arg("--limit", "420"))
    lines = ["# tools/bench_dory_commit.py: wall milliseconds, MI355X; per phase the smallest of %d runs after a warm-up run, every phase ending with the context drained" % REPEATS,
             "# %d one-hot columns of K = %d in %d sources and %d dense u64 columns over 2^log_t cycles, rows of 2^sigma; both routes in one process on the same inputs" % (SOURCES * PER_SOURCE, K, SOURCES, N_DENSE),
             "# a = jolt_dory_hints_onehot / _rows into resident vectors, then one jolt_dory_products; b = jolt_dory_commit_onehot / _rows per column, dory_onehot_hint,",
             "# jolt_dory_vec_upload, one dory_commit_tier2 per column; ratio = b_total / a_total",
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
