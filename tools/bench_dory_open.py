#!/usr/bin/env python3
"""A whole Dory opening on resident vectors (jolt_amd/dory_open.py) on the GPU, phase by phase, and its state built two ways.

    state      v1, v2, s1, s2 on the device through the jolt_dory_state_* entries: combine (a vector of identities, jolt_dory_state_combine_hints), copy (three
               vectors of zeros, three jolt_dory_state_from_table), fixed-base (a vector of identities, jolt_dory_state_fixed_base_mul by H2)
    host state the same four vectors through the host-pointer entries followed by jolt_dory_vec_upload: jolt_dory_combine_hints on host arrays, three table
               downloads, jolt_dory_g2_fixed_base_mul, the padding on the host, four uploads
    vmv        the VMV message, one jolt_dory_products call
    rounds     sigma rounds of DoryReduce
    final      the fold-scalars step and the final message
    total      state + vmv + rounds + final of one run

Shape: sigma = nu with 38 hints, four of them short (2^nu / 16 rows: a dense column's T / 2^sigma rows beside one-hot columns of K = 16), the ragged case of the
bench.  Hints and v are synthetic -- multiples of the generator and a random table: this measures the opening, not tier 1.  Wall milliseconds, each phase ending
with the context drained; per phase the smallest of five runs after one warm-up run, `total` the smallest sum of one run.  Every shape runs in a child process of
its own under a time limit, and a shape that fails or runs out of time ends the measurement.

    python tools/bench_dory_open.py [--out profiles/dory_open.txt] [--sigmas 10,13] [--limit 420]"""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

REPEATS = 5
N_HINTS, N_SHORT = 38, 4
PHASES = ["combine", "copy", "fixed_base", "state", "host_state", "vmv", "rounds", "final", "total"]


def worker(sigma):
    from jolt_amd import ffi
    from jolt_amd.dory_open import DoryOpening, DorySetup
    from tools.bench_dory_routines import g1_points, g2_points
    from util import rand_fr

    nu = sigma
    n, rows = 1 << sigma, 1 << nu
    ctx = ffi.Context(0)
    pool = g1_points(ctx, 2 * n + N_HINTS + 1)
    g2s = g2_points(n + 1)
    setup = DorySetup(ctx, pool[n + N_HINTS:2 * n + N_HINTS], g2s[:n], pool[2 * n + N_HINTS], g2s[n])
    hint_rows = [rows] * (N_HINTS - N_SHORT) + [max(rows // 16, 1)] * N_SHORT
    pool_vec = ctx.dory_vec_upload(ffi.DORY_KIND_G1, pool[:n + N_HINTS])
    hints = [(pool_vec, i, r) for i, r in enumerate(hint_rows)]  # overlapping views of one vector: the hints are only read
    host_hints = [np.ascontiguousarray(pool[i:i + r]) for i, r in enumerate(hint_rows)]
    scalars = rand_fr(N_HINTS, 21)
    v_table, left, right = ctx.upload(rand_fr(n, 22)), ctx.upload(rand_fr(rows, 23)), ctx.upload(rand_fr(n, 24))
    challenges = []
    for k in range(2 * sigma + 1):
        x = rand_fr(1, 30 + k)[0]
        challenges.append((x, ffi.host_fr_inv(x)))

    neutral = ctx.dory_state_alloc(ffi.DORY_KIND_G1, 1)
    identity = neutral.download()[0]
    neutral.free()

    def host_state():
        v1 = np.tile(identity, (n, 1))
        v1[:rows] = ctx.dory_combine_hints(host_hints, scalars)
        v = v_table.download()
        v2 = ctx.dory_g2_fixed_base_mul(setup.h2, v)
        s1 = right.download()
        s2 = np.zeros((n, 4), dtype=np.uint64)
        s2[:rows] = left.download()
        made = [ctx.dory_vec_upload(ffi.DORY_KIND_G1, v1), ctx.dory_vec_upload(ffi.DORY_KIND_G2, v2), ctx.dory_vec_upload(ffi.DORY_KIND_FR, s1),
                ctx.dory_vec_upload(ffi.DORY_KIND_FR, s2)]
        ctx.synchronize()
        for m in made:
            m.free()

    def one_run():
        ms = {}
        op = DoryOpening(setup, hints, scalars, v_table, left, right, nu, sigma)
        ctx.synchronize()
        marks = [time.perf_counter()]

        def mark():
            ctx.synchronize()
            marks.append(time.perf_counter())
            return (marks[-1] - marks[-2]) * 1e3

        op._build_v1()
        ms["combine"] = mark()
        op._build_scalars()
        ms["copy"] = mark()
        op._build_v2()
        ms["fixed_base"] = mark()
        ms["state"] = ms["combine"] + ms["copy"] + ms["fixed_base"]
        op.build_state()  # the three parts are there: this makes the DoryReduce over them, outside the timed phases
        marks[-1] = time.perf_counter()
        op.vmv_message()
        ms["vmv"] = mark()
        for k in range(sigma):
            (beta, beta_inv), (alpha, alpha_inv) = challenges[2 * k], challenges[2 * k + 1]
            op.reduce.round(beta, beta_inv, alpha, alpha_inv)
        ms["rounds"] = mark()
        op.final_message(*challenges[2 * sigma])
        ms["final"] = mark()
        ms["total"] = ms["state"] + ms["vmv"] + ms["rounds"] + ms["final"]
        op.close()
        t0 = time.perf_counter()
        host_state()
        ms["host_state"] = (time.perf_counter() - t0) * 1e3
        return ms

    runs = [one_run() for _ in range(REPEATS + 1)][1:]
    best = {p: min(r[p] for r in runs) for p in PHASES}
    print("ROW %-6d %-4d %s" % (sigma, N_HINTS, " ".join("%12.3f" % best[p] for p in PHASES)), flush=True)
    for t in (v_table, left, right, pool_vec):
        t.free()
    setup.close()
    ctx.close()


def main():
    arg = lambda name, default: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default  # noqa: E731
    if "--worker" in sys.argv:
        worker(int(arg("--worker", "10")))
        return
    out_path = arg("--out", os.path.join(ROOT, "profiles", "dory_open.txt"))
    sigmas = [int(v) for v in arg("--sigmas", "10,13").split(",")]
    limit = int(arg("--limit", "420"))
    lines = ["# tools/bench_dory_open.py: wall milliseconds, MI355X; per phase the smallest of %d runs after a warm-up run, every phase ending with the context drained" % REPEATS,
             "# sigma = nu, %d hints of 2^nu rows, %d of them short (2^nu / 16 rows); synthetic hints and v: the opening, not tier 1" % (N_HINTS, N_SHORT),
             "# state = combine + copy + fixed_base through the jolt_dory_state_* entries; host_state = the same vectors through jolt_dory_combine_hints, table downloads,",
             "# jolt_dory_g2_fixed_base_mul and four jolt_dory_vec_upload; total = state + vmv + rounds + final of one run",
             "%-6s %-4s %s" % ("sigma", "hint", " ".join("%12s" % p for p in PHASES))]
    for sigma in sigmas:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", str(sigma)], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            lines.append("# sigma = %d: no result within %d s; the measurement ends here" % (sigma, limit))
            print(lines[-1], flush=True)
            break
        rows = [ln[4:] for ln in r.stdout.splitlines() if ln.startswith("ROW ")]
        if r.returncode != 0 or not rows:
            lines.append("# sigma = %d: the worker ended with status %d; the measurement ends here" % (sigma, r.returncode))
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
