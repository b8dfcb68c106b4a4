#!/usr/bin/env python3
"""Stages 1 .. 7 of one proof timed two ways in ONE process on ONE box, the two ways alternating (inputs resident in HBM, the per-proof tables prepared outside the
timed region):

  batches  DeviceWorkload.prove_stage_batches: one batched sumcheck per protocol stage on ONE context under one transcript -- the stage's operators and its catalogue
           relations in the same prove_batch, the wrapped members of a round in one launch set (jolt_host_prove_batch_ops_grouped).  Stage 1 (one operator: the
           Spartan outer uni-skip sums and remainder) and the product's uni-skip sums of stage 2, which no batch holds, run beside it as DeviceExtended runs them,
           so that both ways do the same work;
  stages   DeviceWorkload.prove_stages: the step's path -- per stage the operators on their own contexts and host threads BESIDE the catalogue's batch, every
           operator under a transcript of its own.

    python tools/bench_stage_batches.py [log_t = 22] [--reps 5] [--once batches|stages|setup]

Prints one JSON line per timed run and one summary line: per way the median and the spread (max - min) of the runs; a difference smaller than twice the larger spread
is "no measured difference" (DESIGN.md section 4.1c).  --once: ONE run of one way without a warm-up and nothing else (for a kernel trace of its own: the launch
count per proof is that trace's number of kernel dispatches minus the dispatches of `--once setup`, which builds the same resident inputs and tables and proves nothing)."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from jolt_amd import ffi  # noqa: E402
from jolt_amd.workload import DeviceWorkload  # noqa: E402


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def main():
    log_t = int(sys.argv[1]) if len(sys.argv) > 1 and not sys.argv[1].startswith("-") else 22
    reps, once = int(arg("--reps", 5)), arg("--once", None)
    label = ffi.TRANSCRIPT_BLAKE2B | 60  # the transcript bench.py proves under by default
    ctx = ffi.Context(0)
    wl = DeviceWorkload(ctx, log_t, extended=True)
    ext, d = wl.ext, wl.ext.d
    ext.bind_context(ctx)  # what THIS thread drives of the operators (stage 1 below) lives on the main context too; prove_stages' worker threads keep theirs

    def batches():
        out = ext.prove_stage(1, label)
        out["spartan_product_r0"] = ext.spartan_uniskip(ext.product_ints, ext.product_ia, ext.product_ib, d["product_tau"], 1, label + 200)[1]
        out["batches"] = wl.prove_stage_batches(label)
        return out

    ways = {"batches": batches, "stages": lambda: wl.prove_stages(label)}
    if once == "setup":  # everything but a proof: what a kernel trace of `--once <way>` holds beside the proof's launches
        ways["setup"] = lambda: None

    def timed(name):
        wl.prepare()  # a proof's tables and members: outside the timed region for both ways
        ctx.synchronize()
        t0 = time.perf_counter()
        ways[name]()
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3

    if once:
        print(json.dumps({"what": "stages_1_to_7", "way": once, "log_t": log_t, "ms": round(timed(once), 3), "run": "once (no warmup)"}), flush=True)
        wl.close()
        ctx.close()
        return
    for name in ways:  # warm up both ways: pools, the read-RAF orders, code objects
        timed(name)
    runs = {name: [] for name in ways}
    for rep in range(reps):
        for name in ways:  # alternating
            ms = timed(name)
            runs[name].append(ms)
            print(json.dumps({"what": "stages_1_to_7", "way": name, "log_t": log_t, "rep": rep, "ms": round(ms, 3)}), flush=True)
    summary = {name: {"median_ms": round(statistics.median(v), 3), "spread_ms": round(max(v) - min(v), 3)} for name, v in runs.items()}
    diff = summary["batches"]["median_ms"] - summary["stages"]["median_ms"]
    noise = 2 * max(s["spread_ms"] for s in summary.values())
    print(json.dumps({"what": "stages_1_to_7_summary", "log_t": log_t, "reps": reps, **summary, "batches_minus_stages_ms": round(diff, 3),
                      "verdict": "no measured difference" if abs(diff) < noise else ("batches faster" if diff < 0 else "stages faster")}), flush=True)
    wl.close()
    ctx.close()


if __name__ == "__main__":
    main()
