#!/usr/bin/env python3
"""The group and field routines of dory::prove's reduce-and-fold rounds on the GPU (dory_routines.hip): each routine, for G1 and for G2, at n = 2^13, 2^14, 2^15.

Every entry point takes host pointers, so a call is argument checks (on-curve and canonical, on host threads), host -> device copies, kernels and a device -> host
copy.  jolt_dory_routines_timing makes the library drain its stream between those phases and report the wall time of each; the figure per phase is the smallest
of five calls after one warm-up call.  `call` is the wall time of a whole call with that timing switched OFF (the smallest of five), i.e. what a caller pays.
Inputs: distinct points in arbitrary Jacobian representatives (G1: jolt_srs_setup_from_secret; G2: a progression built with jolt_host_g2_add from the generator of
tests/g2_model.py), seeded random scalars.

The CPU figures of the reference (jolt-optimizations' GLV routines under rayon) cannot be collected beside these: there is no Rust toolchain on either machine.

    python tools/bench_dory_routines.py [--out profiles/dory_routines.txt] [--logs 13,14,15]"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from jolt_amd import ffi  # noqa: E402
from tools.bench_msm import rand_fr  # noqa: E402

REPEATS = 5


def g1_points(ctx, n):
    g = np.zeros(12, dtype=np.uint64)
    one_q = [0xd35d438dc58f0d9d, 0x0a78eb28f5c70b3d, 0x666ea36f7879462c, 0x0e0a77c19a07df2f]
    two_q = [0xa6ba871b8b1e1b3a, 0x14f1d651eb8e167b, 0xccdd46def0f28c58, 0x1c14ef83340fbe5e]
    g[0:4], g[4:8], g[8:12] = one_q, two_q, one_q
    return np.ascontiguousarray(ctx.srs_setup_from_secret(rand_fr(1, 1)[0], n, g).download())


def g2_points(n):
    import g2_model as M
    out = np.zeros((n, 24), dtype=np.uint64)
    p, step = M.to_abi(M.mul_generator(12345)), M.to_abi(M.mul_generator(67891))
    for i in range(n):
        out[i] = p
        p = ffi.host_g2_add(p, step)
    return out


def measure(ctx, fn):
    fn()  # warm-up: pool blocks, code objects
    walls = []
    for _ in range(REPEATS):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        walls.append((time.perf_counter() - t0) * 1e3)
    ctx.dory_routines_timing(True)
    phases = []
    for _ in range(REPEATS):
        fn()
        phases.append(ctx.dory_routines_timing(True))
    ctx.dory_routines_timing(False)
    return min(walls), [min(p[k] for p in phases) for k in range(4)]


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "dory_routines.txt")
    logs = [int(v) for v in sys.argv[sys.argv.index("--logs") + 1].split(",")] if "--logs" in sys.argv else [13, 14, 15]
    ctx = ffi.Context(0)
    n_max = 1 << max(logs)
    pts = {"g1": g1_points(ctx, 2 * n_max), "g2": g2_points(2 * n_max)}
    scalars, s = rand_fr(n_max, 7), rand_fr(1, 8)[0]
    lines = ["# tools/bench_dory_routines.py: wall milliseconds per call, MI355X; smallest of %d calls after a warm-up call" % REPEATS,
             "# call = a whole call as a caller pays it; checks / h2d / kernels / d2h = its phases, measured with the stream drained between them",
             "# no CPU figure of the reference beside these: no Rust toolchain on either machine",
             "%-22s %-3s %6s %9s %9s %9s %9s %9s" % ("routine", "grp", "n", "call", "checks", "h2d", "kernels", "d2h")]
    lib, h = ffi.lib(), ctx.h
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def run(name, *args):  # the C entry points themselves: no numpy conversions inside the timed region
        st = getattr(lib, name)(h, *args)
        if st != 0:
            raise ffi.JoltError(st, name)

    def row(name, group, n, fn):
        wall, ph = measure(ctx, fn)
        lines.append("%-22s %-3s %6d %9.3f %9.3f %9.3f %9.3f %9.3f" % (name, group, n, wall, *ph))
        print(lines[-1], flush=True)

    for group in ("g1", "g2"):
        for log_n in logs:
            n, N = 1 << log_n, C.c_size_t(1 << log_n)
            bases, sc = np.ascontiguousarray(pts[group][:n]), np.ascontiguousarray(scalars[:n])
            vs = pts[group][n_max:n_max + n].copy()  # updated in place call after call: always valid points, and the time does not depend on which
            out = np.zeros_like(bases)
            row("msm", group, n, lambda: run(f"jolt_dory_{group}_msm", ptr(bases), ptr(sc), N, ptr(out)))
            row("fixed_base_mul", group, n, lambda: run(f"jolt_dory_{group}_fixed_base_mul", ptr(bases), ptr(sc), N, ptr(out)))
            row("scale_bases_add", group, n, lambda: run(f"jolt_dory_{group}_scale_bases_add", ptr(bases), ptr(vs), N, ptr(s)))
            row("scale_vs_add", group, n, lambda: run(f"jolt_dory_{group}_scale_vs_add", ptr(vs), ptr(bases), N, ptr(s)))
    for log_n in logs:
        n = 1 << log_n
        left, right = rand_fr(n, 9), rand_fr(n, 10)
        row("fold_field_vectors", "fr", n, lambda: run("jolt_dory_fold_field_vectors", ptr(left), ptr(right), C.c_size_t(n), ptr(s)))
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
