#!/usr/bin/env python3
"""One step of the workload per commitment scheme: DeviceWorkload(pcs="dory") against DeviceWorkload(pcs="grid") (HyperKZG), the same seed, extended=True.

The legs of DeviceWorkload.step are timed apart, each from a drained context to a drained context:

    prepare   per-proof tables and members
    commit    dory: tier-1 hints of every column and tier 2 as one product batch      grid: the MSMs and sums of bases over the commitment grid, the opening hint begun
    stages    stages 1 - 7 (the stage operators beside the catalogue's batched sumchecks): the same work under both schemes
    open      dory: jolt_host_dory_prove_batch (statement, row fold, check, evaluation proof, closing claim)      grid: joint polynomial and one HyperKZG opening

Per leg the median, the smallest and the largest of five steps after two warm-up steps.  The setup (Dory: 2^sigma bases per group; grid: the SRS of 2^(4 + log T)
points and its window tables) is built before the first step and is not timed; its wall time is reported.  Every (scheme, log T) runs in a child process of its own
under a time limit; one that fails or runs out of time is recorded as such and ends the measurement.

    python tools/bench_dory_step.py [--out profiles/dory_step.txt] [--log-ts 20,22] [--schemes dory,grid] [--limit 900]

--blocks COUNTxLOG2[,COUNTxLOG2...] (e.g. 64x16,1x20: 64 bytecode chunks of 2^16 entries and an image of 2^20) measures the Dory step over trace columns AND
block-embedded polynomials instead: the parent-shaped step (dory) and the block step (dory+blocks: DeviceWorkload(pcs="dory", dory_blocks=...)) alternate in child
processes, --rounds times each (default 2), into profiles/dory_step_blocks.txt; the block worker also times jolt_dory_evaluate_blocks and the block fold
(jolt_dory_fold_rows_blocks_many, no base) of that set on their own.  Without --blocks the tool and its output are what they were."""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

WARMUPS, STEPS = 2, 5
LEGS = ("prepare", "commit", "stages", "open")


def parse_blocks(spec):
    """64x16,1x20 -> [16] * 64 + [20]"""
    return [int(part.split("x")[1]) for part in spec.split(",") if part for _ in range(int(part.split("x")[0]))]


def time_block_passes(ctx, w):
    """jolt_dory_evaluate_blocks and the block fold of the workload's blocks on their own: (median, smallest, largest) each, drained context to drained context"""
    left = ctx.eq_evals(w.open_point[:w.dory_nu])
    scalars = w.opening_claims[:len(w.dory_blocks)]  # any canonical field elements
    walls = {"evaluate_blocks": [], "fold_blocks": []}
    for step in range(WARMUPS + STEPS):
        ctx.synchronize()
        t = time.perf_counter()
        ctx.dory_evaluate_blocks(w.dory_blocks, w.dory_block_sigmas, w.open_point, w.dory_sigma)
        ctx.synchronize()
        t1 = time.perf_counter()
        v = ctx.dory_fold_rows_blocks_many(w.dory_blocks, w.dory_block_sigmas, scalars, w.dory_sigma, left)
        ctx.synchronize()
        t2 = time.perf_counter()
        v.free()
        if step >= WARMUPS:
            walls["evaluate_blocks"].append((t1 - t) * 1e3)
            walls["fold_blocks"].append((t2 - t1) * 1e3)
    left.free()
    return {k: (statistics.median(v), min(v), max(v)) for k, v in walls.items()}


def worker(pcs, log_t, seed, blocks=None):
    from jolt_amd import ffi
    from jolt_amd.workload import DeviceWorkload

    ctx = ffi.Context(0)
    t0 = time.perf_counter()
    if pcs == "dory+blocks":
        w = DeviceWorkload(ctx, log_t, seed=seed, pcs="dory", extended=True, dory_blocks=blocks)
    else:
        w = DeviceWorkload(ctx, log_t, seed=seed, pcs=pcs, extended=True)
    ctx.synchronize()
    print("SETUP %s log_t=%d %.1f s (construction: resident inputs, the scheme's setup, the input claims)" % (pcs, log_t, time.perf_counter() - t0), flush=True)
    walls = {leg: [] for leg in LEGS}

    def leg(name, fn, keep):
        ctx.synchronize()
        t = time.perf_counter()
        out = fn()
        ctx.synchronize()
        if keep:
            walls[name].append((time.perf_counter() - t) * 1e3)
        return out

    for step in range(WARMUPS + STEPS):
        keep, k = step >= WARMUPS, ffi.TRANSCRIPT_BLAKE2B | (100 * step)
        leg("prepare", w.prepare, keep)
        leg("commit", w.commit, keep)
        leg("stages", lambda: w.prove_stages(k) if w._stage_worker is not None else (w.ext.prove(k), w.prove(k)), keep)
        leg("open", lambda: w.open(k), keep)
    cells = "   ".join("%s %9.2f %9.2f %9.2f" % (name, statistics.median(walls[name]), min(walls[name]), max(walls[name])) for name in LEGS)
    total = [sum(walls[name][i] for name in LEGS) for i in range(STEPS)]
    print("ROW %-5s log_t=%-3d %s   step %9.2f %9.2f %9.2f" % (pcs, log_t, cells, statistics.median(total), min(total), max(total)), flush=True)
    if pcs == "dory+blocks":
        print("PASS %s log_t=%-3d %s" % (pcs, log_t, "   ".join("%s %9.3f %9.3f %9.3f" % ((k,) + v) for k, v in time_block_passes(ctx, w).items())), flush=True)
    w.close()
    ctx.close()


def main():
    arg = lambda name, default: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default  # noqa: E731
    if "--worker" in sys.argv:
        i = sys.argv.index("--worker")
        worker(sys.argv[i + 1], int(sys.argv[i + 2]), int(arg("--seed", "2026")), parse_blocks(arg("--blocks", "")))
        return
    blocks = arg("--blocks", "")
    out_path = arg("--out", os.path.join(ROOT, "profiles", "dory_step_blocks.txt" if blocks else "dory_step.txt"))
    log_ts = [int(v) for v in arg("--log-ts", "20" if blocks else "20,22").split(",") if v]
    schemes = [s for s in arg("--schemes", "dory,grid").split(",") if s]
    limit = int(arg("--limit", "900"))
    lines = ["# tools/bench_dory_step.py: wall milliseconds, MI355X, one step per scheme, extended=True, the same seed; per leg median, smallest, largest of %d steps after %d warm-up steps" % (STEPS, WARMUPS),
             "# dory: tier-1 hints + one tier-2 batch | jolt_host_dory_prove_batch under a LegacyBlake2b transcript.  grid: HyperKZG over the 2^(4 + log T) grid.  Setup untimed."]
    runs = [(p, t) for p in schemes for t in log_ts]
    extra = []
    if blocks:
        lines[1] = ("# dory: the parent-shaped step (38 trace columns).  dory+blocks: the same with --blocks %s block-embedded behind them (field elements drawn from the seed, committed by "
                    "jolt_dory_hints_rows_fr inside commit, opened by jolt_host_dory_prove_batch_blocks).  The two alternate in child processes." % blocks)
        lines.append("# PASS rows: jolt_dory_evaluate_blocks (eq tables, two launches, download) and jolt_dory_fold_rows_blocks_many (no base) of that set alone: median, smallest, largest")
        runs = [(p, t) for t in log_ts for _ in range(int(arg("--rounds", "2"))) for p in ("dory", "dory+blocks")]
        extra = ["--blocks", blocks]
    for pcs, log_t in runs:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", pcs, str(log_t)] + extra, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            lines.append("# %s log_t=%d: no result within %d s; the measurement ends here" % (pcs, log_t, limit))
            print(lines[-1], flush=True)
            break
        rows = [ln for ln in r.stdout.splitlines() if ln.startswith(("ROW ", "SETUP ", "PASS "))]
        if r.returncode != 0 or not any(ln.startswith("ROW ") for ln in rows):
            lines.append("# %s log_t=%d: the worker ended with status %d; the measurement ends here" % (pcs, log_t, r.returncode))
            print(lines[-1], flush=True)
            print(r.stderr[-2000:], flush=True)
            break
        for ln in rows:
            lines.append(ln[4:] if ln.startswith("ROW ") else ln if ln.startswith("PASS ") else "# " + ln[6:])
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
