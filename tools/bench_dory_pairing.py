#!/usr/bin/env python3
"""Dory's multi-pairings on the GPU (dory_pairing.hip): jolt_dory_multi_pair and jolt_dory_multi_pair_g2_setup at n = 2^13, 2^14, 2^15.

A call is argument checks (on-curve and canonical, on host threads), host -> device copies, the prepare kernel (multi_pair only: multi_pair_g2_setup reads a table
prepared once, whose preparation is the `g2_prepare` row), the Miller kernel, the product tree, a device -> host copy of one GT element and the final exponentiation
on the host.  jolt_dory_pairing_timing makes the library drain its stream between those phases and report the wall time of each; the figure per phase is the
smallest of five calls after one warm-up call.  `call` is the wall time of a whole call with that timing switched OFF (the smallest of five), i.e. what a caller pays.
Inputs: distinct points in arbitrary Jacobian representatives, as tools/bench_dory_routines.py makes them.

The CPU figures of the reference (ark_bn254's multi_pairing under rayon) cannot be collected beside these: there is no Rust toolchain on either machine.

    python tools/bench_dory_pairing.py [--out profiles/dory_pairing.txt] [--logs 13,14,15]"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from jolt_amd import ffi  # noqa: E402
from tools.bench_dory_routines import g1_points, g2_points  # noqa: E402

REPEATS = 5
PHASES = ("checks", "h2d", "prepare", "miller", "product", "d2h", "final_exp")


def measure(ctx, fn):
    fn()  # warm-up: pool blocks, code objects
    walls = []
    for _ in range(REPEATS):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        walls.append((time.perf_counter() - t0) * 1e3)
    ctx.dory_pairing_timing(True)
    phases = []
    for _ in range(REPEATS):
        fn()
        phases.append(ctx.dory_pairing_timing(True))
    ctx.dory_pairing_timing(False)
    return min(walls), [min(p[k] for p in phases) for k in range(len(PHASES))]


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "dory_pairing.txt")
    logs = [int(v) for v in sys.argv[sys.argv.index("--logs") + 1].split(",")] if "--logs" in sys.argv else [13, 14, 15]
    ctx = ffi.Context(0)
    n_max = 1 << max(logs)
    g1s, g2s = g1_points(ctx, n_max), g2_points(n_max)
    lines = ["# tools/bench_dory_pairing.py: wall milliseconds per call, MI355X; smallest of %d calls after a warm-up call" % REPEATS,
             "# call = a whole call as a caller pays it; the other columns its phases, measured with the stream drained between them",
             "# no CPU figure of the reference beside these: no Rust toolchain on either machine",
             ("%-22s %6s %9s" + " %9s" * len(PHASES)) % (("entry", "n", "call") + PHASES)]
    lib, h = ffi.lib(), ctx.h
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    out = ffi.gt_array()

    def run(name, *args):  # the C entry points themselves: no numpy conversions inside the timed region
        st = getattr(lib, name)(h, *args)
        if st != 0:
            raise ffi.JoltError(st, name)

    def row(name, n, fn):
        wall, ph = measure(ctx, fn)
        lines.append(("%-22s %6d %9.3f" + " %9.3f" * len(PHASES)) % ((name, n, wall) + tuple(ph)))
        print(lines[-1], flush=True)

    for log_n in logs:
        n, N = 1 << log_n, C.c_size_t(1 << log_n)
        a, b = np.ascontiguousarray(g1s[:n]), np.ascontiguousarray(g2s[:n])
        row("multi_pair", n, lambda: run("jolt_dory_multi_pair", ptr(a), ptr(b), N, ptr(out)))
        handle = C.c_void_p()

        def prepare():
            if handle.value:
                run("jolt_g2_prepared_free", handle)
            run("jolt_dory_g2_prepare", ptr(b), N, C.byref(handle))

        row("g2_prepare", n, prepare)
        row("multi_pair_g2_setup", n, lambda: run("jolt_dory_multi_pair_g2_setup", ptr(a), handle, N, ptr(out)))
        run("jolt_g2_prepared_free", handle)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
