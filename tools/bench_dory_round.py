#!/usr/bin/env python3
"""One reduce-and-fold round of a Dory opening on the GPU, two ways, and a whole reduction.

    resident   jolt_amd.dory_reduce.DoryReduce: vectors that stay in HBM, each message one jolt_dory_products call, the updates enqueued in place
    composed   the same round from the host-pointer entry points (dory_routines.hip, dory_pairing.hip), one call per product or update: six multi-pairings
               (the two against Gamma2 through a table prepared once, outside the timed region, as the resident path's is), six MSMs, four shared-scalar
               routines, two field folds -- each uploads, runs alone, synchronises and downloads
    reduction  DoryReduce from n = 2^14 down to 1, fourteen rounds

Both rounds are timed in this one process on the same inputs at n = 2^13, 2^14, 2^15: the smallest of five runs after one warm-up run.  A timed run starts from a
fresh state made outside the timed region (the resident state is uploaded and checked there, the composed path's arrays are copied there) and ends with the context
drained.  `split` is one further resident round with the context drained after each of its four steps.  No CPU figure of the reference beside these: there is no
Rust toolchain on either machine.

    python tools/bench_dory_round.py [--out profiles/dory_round.txt] [--logs 13,14,15] [--reduction-log 14]"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from jolt_amd import ffi  # noqa: E402
from jolt_amd.dory_reduce import DoryReduce  # noqa: E402
from tools.bench_dory_routines import g1_points, g2_points  # noqa: E402
from util import rand_fr  # noqa: E402

REPEATS = 5


def challenge(seed):
    x = rand_fr(1, seed)[0]
    return x, ffi.host_fr_inv(x)


def smallest(setup, run):
    """the smallest wall time of REPEATS runs of run(state) after one warm-up run; setup() makes the state outside the timed region"""
    walls = []
    for k in range(REPEATS + 1):
        state = setup()
        t0 = time.perf_counter()
        run(state)
        if k:
            walls.append((time.perf_counter() - t0) * 1e3)
    return min(walls)


def main():
    arg = lambda name, default: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default  # noqa: E731
    out_path = arg("--out", os.path.join(ROOT, "profiles", "dory_round.txt"))
    logs = [int(v) for v in arg("--logs", "13,14,15").split(",")]
    reduction_log = int(arg("--reduction-log", "14"))
    ctx = ffi.Context(0)
    lib, h = ffi.lib(), ctx.h
    n_max = 1 << max(logs + [reduction_log])
    g1s, g2s = g1_points(ctx, 2 * n_max), g2_points(2 * n_max)
    s1_all, s2_all = rand_fr(n_max, 11), rand_fr(n_max, 12)
    (beta, beta_inv), (alpha, alpha_inv) = challenge(13), challenge(14)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def call(name, *args):  # the C entry points themselves: no numpy conversions inside the timed region
        st = getattr(lib, name)(h, *args)
        if st != 0:
            raise ffi.JoltError(st, name)

    def inputs(n):
        return (np.ascontiguousarray(g1s[:n]), np.ascontiguousarray(g2s[:n]), np.ascontiguousarray(s1_all[:n]), np.ascontiguousarray(s2_all[:n]),
                np.ascontiguousarray(g1s[n_max:n_max + n]), np.ascontiguousarray(g2s[n_max:n_max + n]))

    def resident_state(n):
        ctx.synchronize()
        red = DoryReduce(ctx, *inputs(n))
        ctx.synchronize()
        return red

    def resident_round(red):
        red.round(beta, beta_inv, alpha, alpha_inv)
        ctx.synchronize()
        red.close()

    def resident_split(n):
        red, marks = resident_state(n), [time.perf_counter()]
        for step in (red.first_message, lambda: red.apply_beta(beta, beta_inv), red.second_message, lambda: red.apply_alpha(alpha, alpha_inv)):
            step()
            ctx.synchronize()
            marks.append(time.perf_counter())
        red.close()
        return [(b - a) * 1e3 for a, b in zip(marks, marks[1:])]

    def composed_round(state):
        v1, v2, s1, s2, gamma1, gamma2, prepared = state
        n = v1.shape[0]
        hn, N, H = n // 2, C.c_size_t(n), C.c_size_t(n // 2)
        gt, p1, p2 = ffi.gt_array(), np.zeros(12, dtype=np.uint64), np.zeros(24, dtype=np.uint64)
        v1l, v1r, v2l, v2r, s1l, s1r, s2l, s2r = v1[:hn], v1[hn:], v2[:hn], v2[hn:], s1[:hn], s1[hn:], s2[:hn], s2[hn:]
        call("jolt_dory_multi_pair_g2_setup", ptr(v1l), prepared, H, ptr(gt))
        call("jolt_dory_multi_pair_g2_setup", ptr(v1r), prepared, H, ptr(gt))
        call("jolt_dory_multi_pair", ptr(gamma1), ptr(v2l), H, ptr(gt))
        call("jolt_dory_multi_pair", ptr(gamma1), ptr(v2r), H, ptr(gt))
        call("jolt_dory_g1_msm", ptr(gamma1), ptr(s2), N, ptr(p1))
        call("jolt_dory_g2_msm", ptr(gamma2), ptr(s1), N, ptr(p2))
        call("jolt_dory_g1_scale_bases_add", ptr(gamma1), ptr(v1), N, ptr(beta))
        call("jolt_dory_g2_scale_bases_add", ptr(gamma2), ptr(v2), N, ptr(beta_inv))
        call("jolt_dory_multi_pair", ptr(v1l), ptr(v2r), H, ptr(gt))
        call("jolt_dory_multi_pair", ptr(v1r), ptr(v2l), H, ptr(gt))
        call("jolt_dory_g1_msm", ptr(v1l), ptr(s2r), H, ptr(p1))
        call("jolt_dory_g1_msm", ptr(v1r), ptr(s2l), H, ptr(p1))
        call("jolt_dory_g2_msm", ptr(v2r), ptr(s1l), H, ptr(p2))
        call("jolt_dory_g2_msm", ptr(v2l), ptr(s1r), H, ptr(p2))
        call("jolt_dory_g1_scale_vs_add", ptr(v1l), ptr(v1r), H, ptr(alpha))
        call("jolt_dory_g2_scale_vs_add", ptr(v2l), ptr(v2r), H, ptr(alpha_inv))
        call("jolt_dory_fold_field_vectors", ptr(s1l), ptr(s1r), H, ptr(alpha))
        call("jolt_dory_fold_field_vectors", ptr(s2l), ptr(s2r), H, ptr(alpha_inv))
        ctx.synchronize()

    lines = ["# tools/bench_dory_round.py: wall milliseconds, MI355X; smallest of %d runs after a warm-up run, both paths in one process on the same inputs" % REPEATS,
             "# resident = one round through DoryReduce (two jolt_dory_products calls, four in-place updates); composed = the same round from the host-pointer entry points",
             "# (6 multi-pairings, 6 MSMs, 4 shared-scalar routines, 2 field folds, one call each); split = one resident round drained after each step",
             "# no CPU figure of the reference beside these: no Rust toolchain on either machine",
             "%-10s %6s %12s %12s %8s   %s" % ("row", "n", "resident_ms", "composed_ms", "ratio", "split: first_message apply_beta second_message apply_alpha")]
    for log_n in logs:
        n = 1 << log_n
        resident = smallest(lambda: resident_state(n), resident_round)
        prepared = C.c_void_p()
        call("jolt_dory_g2_prepare", ptr(inputs(n)[5]), C.c_size_t(n), C.byref(prepared))
        composed = smallest(lambda: tuple(a.copy() for a in inputs(n)) + (prepared,), composed_round)
        call("jolt_g2_prepared_free", prepared)
        split = resident_split(n)
        lines.append("%-10s %6d %12.3f %12.3f %8.2f   %s" % ("round", n, resident, composed, composed / resident, " ".join("%.3f" % v for v in split)))
        print(lines[-1], flush=True)

    n = 1 << reduction_log

    def reduction(red):
        k = 0
        while red.n > 1:
            red.round(beta, beta_inv, alpha, alpha_inv)
            k += 1
        ctx.synchronize()
        red.close()
        return k

    total = smallest(lambda: resident_state(n), reduction)
    lines.append("%-10s %6d %12.3f %12s %8s   %d rounds, n -> 1" % ("reduction", n, total, "-", "-", reduction_log))
    print(lines[-1], flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
