#!/usr/bin/env python3
"""A Dory evaluation proof as one library call against the same proof driven from Python, and a round's update as one call against the separate calls.

    open    sigma = nu with 38 hints, four of them short (the shape of tools/bench_dory_open.py), the same inputs for both:
              c_call   jolt_host_dory_open under a LegacyBlake2b HostTranscript: state, VMV message, sigma rounds, fold-scalars, final message, the transcript included
              python   dory_open.DoryOpening driven message by message with the challenges handed in (no transcript work at all: the yardstick is favoured)
    update  v1, v2, Gamma1, Gamma2 of n points and s1, s2 of n scalars, a full-width challenge:
              beta     jolt_dory_round_update(BETA) against jolt_dory_vec_scale_bases_add for G1 and then for G2
              alpha    jolt_dory_round_update(ALPHA) against two jolt_dory_vec_scale_vs_add, two jolt_dory_vec_fold_field and four truncations
            the vectors of an alpha run are uploaded afresh outside the timed part (the fold truncates them)

Wall milliseconds from a drained context to a drained context; per figure the smallest and the largest of five runs after one warm-up run, so that a difference can
be held against the spread.  Every shape runs in a child process of its own under a time limit, and a shape that fails or runs out of time ends the measurement.

    python tools/bench_dory_proof.py [--out profiles/dory_proof.txt] [--sigmas 10,13] [--log-ns 13,14,15] [--limit 420]"""
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


def timed(ctx, fn, prepare=None):
    """(min, max) wall ms of REPEATS runs of fn after one warm-up run; prepare() runs before each, outside the timed part"""
    walls = []
    for _ in range(REPEATS + 1):
        args = prepare() if prepare else ()
        ctx.synchronize()
        t0 = time.perf_counter()
        fn(*args)
        ctx.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    return min(walls[1:]), max(walls[1:])


def worker_open(sigma):
    from jolt_amd import dory_proof, ffi
    from jolt_amd.dory_open import DoryOpening, DorySetup
    from tools.bench_dory_routines import g1_points, g2_points
    from util import rand_fr

    nu = sigma
    n, rows = 1 << sigma, 1 << nu
    ctx = ffi.Context(0)
    pool = g1_points(ctx, 2 * n + N_HINTS + 1)
    g2s = g2_points(n + 1)
    gamma1, h1, h2 = pool[n + N_HINTS:2 * n + N_HINTS], pool[2 * n + N_HINTS], g2s[n]
    py_setup = DorySetup(ctx, gamma1, g2s[:n], h1, h2)
    lib_setup = dory_proof.DoryProofSetup(ctx, gamma1, g2s[:n], h1, h2)
    hint_rows = [rows] * (N_HINTS - N_SHORT) + [max(rows // 16, 1)] * N_SHORT
    pool_vec = ctx.dory_vec_upload(ffi.DORY_KIND_G1, pool[:n + N_HINTS])
    hints = [(pool_vec, i, r) for i, r in enumerate(hint_rows)]  # overlapping views of one vector: the hints are only read
    scalars = rand_fr(N_HINTS, 21)
    v_table, left, right = ctx.upload(rand_fr(n, 22)), ctx.upload(rand_fr(rows, 23)), ctx.upload(rand_fr(n, 24))
    challenges = []
    for k in range(2 * sigma + 1):
        x = rand_fr(1, 30 + k)[0]
        challenges.append((x, ffi.host_fr_inv(x)))

    def c_call():
        t = ffi.HostTranscript(ffi.TRANSCRIPT_BLAKE2B | 7)
        dory_proof.prove(lib_setup, hints, scalars, v_table, left, right, nu, sigma, transcript=t)
        t.close()

    def python_driven():
        op = DoryOpening(py_setup, hints, scalars, v_table, left, right, nu, sigma)
        op.vmv_message()
        for k in range(sigma):
            (beta, beta_inv), (alpha, alpha_inv) = challenges[2 * k], challenges[2 * k + 1]
            op.reduce.round(beta, beta_inv, alpha, alpha_inv)
        op.final_message(*challenges[2 * sigma])
        op.close()

    c_lo, c_hi = timed(ctx, c_call)
    p_lo, p_hi = timed(ctx, python_driven)
    print("ROW open    sigma=%-3d hints=%-3d c_call %10.3f %10.3f   python %10.3f %10.3f" % (sigma, N_HINTS, c_lo, c_hi, p_lo, p_hi), flush=True)
    for t in (v_table, left, right, pool_vec):
        t.free()
    py_setup.close()
    lib_setup.close()
    ctx.close()


def worker_update(log_n):
    from jolt_amd import ffi
    from tools.bench_dory_routines import g1_points, g2_points
    from util import rand_fr

    n, h = 1 << log_n, 1 << (log_n - 1)
    ctx = ffi.Context(0)
    p1, p2 = g1_points(ctx, 2 * n), g2_points(2 * n)
    s1h, s2h = rand_fr(n, 41), rand_fr(n, 42)
    gamma1, gamma2 = ctx.dory_vec_upload(ffi.DORY_KIND_G1, p1[n:]), ctx.dory_vec_upload(ffi.DORY_KIND_G2, p2[n:])
    x = rand_fr(1, 43)[0]
    xi = ffi.host_fr_inv(x)
    made = []

    def fresh():
        for v in made:
            v.free()
        made[:] = [ctx.dory_vec_upload(ffi.DORY_KIND_G1, p1[:n]), ctx.dory_vec_upload(ffi.DORY_KIND_G2, p2[:n]), ctx.dory_vec_upload(ffi.DORY_KIND_FR, s1h),
                   ctx.dory_vec_upload(ffi.DORY_KIND_FR, s2h)]
        return tuple(made)

    def beta_one(v1, v2, s1, s2):
        ctx.dory_round_update(ffi.DORY_UPDATE_BETA, v1, v2, gamma1, gamma2, x, xi)

    def beta_separate(v1, v2, s1, s2):
        ctx.dory_vec_scale_bases_add(gamma1, v1, x)
        ctx.dory_vec_scale_bases_add(gamma2, v2, xi)

    def alpha_one(v1, v2, s1, s2):
        ctx.dory_round_update(ffi.DORY_UPDATE_ALPHA, v1, v2, s1, s2, x, xi)

    def alpha_separate(v1, v2, s1, s2):
        ctx.dory_vec_scale_vs_add((v1, 0, h), (v1, h, h), x)
        ctx.dory_vec_scale_vs_add((v2, 0, h), (v2, h, h), xi)
        ctx.dory_vec_fold_field((s1, 0, h), (s1, h, h), x)
        ctx.dory_vec_fold_field((s2, 0, h), (s2, h, h), xi)
        for v in (v1, v2, s1, s2):
            v.truncate(h)

    figures = [timed(ctx, f, fresh) for f in (beta_one, beta_separate, alpha_one, alpha_separate)]
    print("ROW update  n=2^%-2d  beta one call %8.3f %8.3f  separate %8.3f %8.3f   alpha one call %8.3f %8.3f  separate %8.3f %8.3f"
          % ((log_n,) + tuple(v for lo_hi in figures for v in lo_hi)), flush=True)
    for v in made + [gamma1, gamma2]:
        v.free()
    ctx.close()


def main():
    arg = lambda name, default: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default  # noqa: E731
    if "--worker" in sys.argv:
        kind, size = sys.argv[sys.argv.index("--worker") + 1:sys.argv.index("--worker") + 3]
        (worker_open if kind == "open" else worker_update)(int(size))
        return
    out_path = arg("--out", os.path.join(ROOT, "profiles", "dory_proof.txt"))
    sigmas = [int(v) for v in arg("--sigmas", "10,13").split(",") if v]
    log_ns = [int(v) for v in arg("--log-ns", "13,14,15").split(",") if v]
    limit = int(arg("--limit", "420"))
    lines = ["# tools/bench_dory_proof.py: wall milliseconds, MI355X, drained context to drained context; per figure the smallest and the largest of %d runs after a warm-up run" % REPEATS,
             "# open: sigma = nu, %d hints of 2^nu rows, %d of them short (2^nu / 16 rows), synthetic hints and v; c_call = jolt_host_dory_open under a LegacyBlake2b transcript," % (N_HINTS, N_SHORT),
             "#       python = dory_open.DoryOpening driven message by message with the challenges handed in (no transcript work)",
             "# update: one call = jolt_dory_round_update (G1 on the main stream, G2 beside it on a side stream); separate = the existing calls in a row on the main stream"]
    for kind, size in [("open", s) for s in sigmas] + [("update", k) for k in log_ns]:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", kind, str(size)], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            lines.append("# %s %d: no result within %d s; the measurement ends here" % (kind, size, limit))
            print(lines[-1], flush=True)
            break
        rows = [ln[4:] for ln in r.stdout.splitlines() if ln.startswith("ROW ")]
        if r.returncode != 0 or not rows:
            lines.append("# %s %d: the worker ended with status %d; the measurement ends here" % (kind, size, r.returncode))
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
