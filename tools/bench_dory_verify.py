#!/usr/bin/env python3
"""Dory verification on the device, measured: the GT multi-exponentiation against the same product on 16 host threads, and the whole verifier of the stage-8 batch.

    multiexp   jolt_dory_gt_multi_exp at n = 64, 256, 1024 over random Fq12 elements and full-width scalars, split by jolt_dory_pairing_timing's clock into checks,
               host -> device, the power kernel, the product tree, device -> host; against jolt_host_gt_pow per element on 16 host threads (ctypes releases the GIL)
               and the product by jolt_host_fq12_op(MUL).  The two results are compared bit for bit before a figure is reported.
    verify     DeviceWorkload(pcs="dory").dory_verify of the step's own proof (38 claims; --blocks adds block-embedded polynomials behind them), split by
               jolt_dory_verifier_setup_timing into replay + exponents (host), the G1 / G2 folds, the pairings with their final exponentiations, the
               multi-exponentiation; the one-off build of the verifier's setup (3 sigma + 4 pairing products, one batch) is reported beside it.

Median, smallest and largest of five calls after two warm-up calls.  Every measurement runs in a child process of its own under a time limit; one that fails or runs
out of time is recorded as such and ends the measurement.

    python tools/bench_dory_verify.py [--out profiles/dory_verify.txt] [--sizes 64,256,1024] [--log-ts 20,22] [--blocks 64x16,1x20] [--limit 600]"""
import os
import statistics
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

WARMUPS, CALLS, HOST_THREADS = 2, 5, 16
Q = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001


def parse_blocks(spec):
    """64x16,1x20 -> [16] * 64 + [20]"""
    return [int(part.split("x")[1]) for part in spec.split(",") if part for _ in range(int(part.split("x")[0]))]


def stats(values):
    return "%9.3f %9.3f %9.3f" % (statistics.median(values), min(values), max(values))


def canonical_words(rng, count, modulus):
    """count uniform values below the modulus as four little-endian 64-bit words each: any such value is a canonical Montgomery word"""
    import numpy as np
    out = np.zeros((count, 4), dtype=np.uint64)
    for i in range(count):
        v = int.from_bytes(rng.bytes(40), "little") % modulus
        out[i] = [(v >> (64 * j)) & (2**64 - 1) for j in range(4)]
    return out


def worker_multiexp(n):
    import numpy as np
    from jolt_amd import ffi

    rng = np.random.default_rng(2026 + n)
    gts = canonical_words(rng, 12 * n, Q).reshape(n, 48)
    scalars = canonical_words(rng, n, R)
    ctx = ffi.Context(0)
    ctx.dory_pairing_timing(True)
    walls, phases = [], []
    for call in range(WARMUPS + CALLS):
        ctx.synchronize()
        t = time.perf_counter()
        device = ctx.dory_gt_multi_exp(gts, scalars)
        wall = (time.perf_counter() - t) * 1e3
        if call >= WARMUPS:
            walls.append(wall)
            phases.append(ctx.dory_pairing_timing(True))
    ctx.dory_pairing_timing(False)
    ctx.close()
    host_walls, host_pow = [], []
    with ThreadPoolExecutor(max_workers=HOST_THREADS) as pool:
        for call in range(1 + 3):
            t = time.perf_counter()
            powers = list(pool.map(lambda i: ffi.host_gt_pow(gts[i], scalars[i]), range(n)))
            t1 = time.perf_counter()
            host = powers[0]
            for x in powers[1:]:
                host = ffi.host_fq12_op(ffi.FQ12_MUL, host, x)
            t2 = time.perf_counter()
            if call >= 1:
                host_pow.append((t1 - t) * 1e3)
                host_walls.append((t2 - t) * 1e3)
    if not np.array_equal(host, device):
        raise SystemExit("the device's product is not the host's")
    col = lambda k: stats([p[k] for p in phases])  # noqa: E731
    print("ROW multiexp n=%-5d device %s | checks %s  h2d %s  powers %s  tree %s  d2h %s | host(%d threads) %s  of which powers %s" % (
        n, stats(walls), col(0), col(1), col(3), col(4), col(5), HOST_THREADS, stats(host_walls), stats(host_pow)), flush=True)


def worker_verify(log_t, blocks):
    from jolt_amd import ffi
    from jolt_amd.workload import DeviceWorkload

    ctx = ffi.Context(0)
    w = DeviceWorkload(ctx, log_t, seed=2026, pcs="dory", dory_blocks=blocks) if blocks else DeviceWorkload(ctx, log_t, seed=2026, pcs="dory")
    label = ffi.TRANSCRIPT_BLAKE2B | 77
    commit = w.dory_commit()
    out = w.dory_open(label)
    ctx.synchronize()
    t = time.perf_counter()
    vs = w.dory_setup.verifier()
    build = (time.perf_counter() - t) * 1e3
    vs.timing(True)
    walls, phases = [], []
    for call in range(WARMUPS + CALLS):
        ctx.synchronize()
        t = time.perf_counter()
        ok = w.dory_verify(commit, out, label)
        wall = (time.perf_counter() - t) * 1e3
        if not ok or w.dory_verify_result["transcript_state"] != out["transcript_state"]:
            raise SystemExit("the step's own proof was not accepted")
        if call >= WARMUPS:
            walls.append(wall)
            phases.append(vs.timing(True))
    col = lambda k: stats([p[k] for p in phases])  # noqa: E731
    print("ROW verify log_t=%-3d claims=%-4d sigma=%-3d terms=%-4d verify %s | replay+exponents %s  folds %s  pairings+final %s  multiexp %s | verifier setup build %9.1f" % (
        log_t, len(commit["tier2"]), w.dory_sigma, 9 * w.dory_sigma + 6 + len(commit["tier2"]), stats(walls), col(0), col(1), col(2), col(3), build), flush=True)
    w.close()
    ctx.close()


def main():
    arg = lambda name, default: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default  # noqa: E731
    if "--worker" in sys.argv:
        i = sys.argv.index("--worker")
        if sys.argv[i + 1] == "multiexp":
            worker_multiexp(int(sys.argv[i + 2]))
        else:
            worker_verify(int(sys.argv[i + 2]), parse_blocks(arg("--blocks", "")))
        return
    out_path = arg("--out", os.path.join(ROOT, "profiles", "dory_verify.txt"))
    sizes = [int(v) for v in arg("--sizes", "64,256,1024").split(",") if v]
    log_ts = [int(v) for v in arg("--log-ts", "20,22").split(",") if v]
    blocks = arg("--blocks", "64x16,1x20")
    limit = int(arg("--limit", "600"))
    lines = ["# tools/bench_dory_verify.py: wall milliseconds, MI355X; median, smallest, largest of %d calls after %d warm-up calls, each measurement in a child process" % (CALLS, WARMUPS),
             "# multiexp: jolt_dory_gt_multi_exp over random Fq12 elements and full-width scalars; the split is jolt_dory_pairing_timing's clock; host: jolt_host_gt_pow on %d threads + the product" % HOST_THREADS,
             "# verify: DeviceWorkload(pcs=\"dory\").dory_verify of the step's own proof; the split is jolt_dory_verifier_setup_timing's clock; terms = 9 sigma + 6 + claims"]
    runs = [(["multiexp", str(n)], []) for n in sizes] + [(["verify", str(t)], []) for t in log_ts]
    if blocks and log_ts:
        runs.append((["verify", str(log_ts[0])], ["--blocks", blocks]))
    for what, extra in runs:
        name = " ".join(what + extra)
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker"] + what + extra, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            lines.append("# %s: no result within %d s; the measurement ends here" % (name, limit))
            print(lines[-1], flush=True)
            break
        rows = [ln for ln in r.stdout.splitlines() if ln.startswith("ROW ")]
        if r.returncode != 0 or not rows:
            lines.append("# %s: the worker ended with status %d; the measurement ends here" % (name, r.returncode))
            print(lines[-1], flush=True)
            print(r.stderr[-2000:], flush=True)
            break
        for ln in rows:
            lines.append(ln[4:] + ("   (with --blocks %s)" % blocks if extra else ""))
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
