#!/usr/bin/env python3
"""A whole precommitted claim reduction (cycle phase + address phase), drained to drained: the fused round kernel of jolt_stage_precommitted_cycle_create against the
COMPOSED route over entry points the library had before it -- a degree-2 expression member over value * eq (jolt_member_create_expr) plus jolt_bind of the passenger
tables, one challenge at a time.

    python tools/bench_precommitted.py [--out profiles/precommitted.txt]

Shapes: the bytecode shape (4 chunk grids of 2^22 entries riding along, plus value and eq) and an advice shape (2^20 entries, no passengers).  Every variable is
active: the first half of the rounds in the cycle phase, the rest in the address phase (an inactive round costs neither route a launch).  Both routes start from the
same resident tables and include their own copies of them (the operator copies; the member takes ownership of clones and jolt_bind halves its tables in place), are
driven round by round from here under the same prescribed challenges, and end with the final claims on the host.  Per shape: a warm-up, then 5 runs, smallest and
largest.  The first FUSED round (round 1: the pending bind over all L entries of every table plus the sums) is timed on its own and its algorithmic traffic,
(2 + n_aux) * L * 32 B read and half of that written, set against the 6.1 TB/s of k_bind_low_to_high."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from jolt_amd import ffi  # noqa: E402

RUNS = 5


def rand_table(ctx, n, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 2**64, size=(1 << n, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64((1 << 60) - 1)  # below the modulus: canonical
    return ctx.upload(a)


def challenges(n, seed):
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)
    c[:, :2] = 0  # the reference's 125-bit challenge shape
    c[:, 3] &= np.uint64((1 << 60) - 1)
    return c


def fused(ctx, value, eq, aux, n, ch, round_times=None):
    k = n // 2
    op = ctx.stage_precommitted_cycle(value, eq, aux, list(range(k)), k, list(range(n - k)), n - k)
    claim = op.input_claim()
    ops = [op]
    for phase, rounds, base in ((0, k, 0), (1, n - k, k)):
        if phase:
            ops.append(ctx.stage_precommitted_address(op))
        o, bind = ops[-1], None
        for rnd in range(rounds):
            t0 = time.perf_counter()
            o.prove_round(bind, rnd, claim)  # (the claim only feeds the hint: the launches do not depend on it)
            if round_times is not None:
                round_times.append(time.perf_counter() - t0)
            bind = ch[base + rnd]
        o.finish_rounds(bind)
    out = ops[-1].output_claims()
    for o in reversed(ops):
        o.destroy()
    return out


def composed(ctx, value, eq, aux, n, ch, round_times=None):
    one = ffi.host_fr_from_u64(1)
    member = ctx.member_expr([value.clone(), eq.clone()], [(one, [0, 1])], 2)
    riders = [a.clone() for a in aux]
    bind = None
    for rnd in range(n):
        t0 = time.perf_counter()
        if bind is not None and riders:
            ctx.bind(riders, bind)
        member.prove_round(bind)
        if round_times is not None:
            round_times.append(time.perf_counter() - t0)
        bind = ch[rnd]
    member.finish(bind)
    if riders:
        ctx.bind(riders, bind)
    out = [member.final_values()[0]] + [r.download()[0] for r in riders]
    member.destroy()
    for r in riders:
        r.free()
    return np.stack(out)


def measure(ctx, fn, args):
    fn(ctx, *args)  # warm-up
    ctx.synchronize()
    times = []
    for _ in range(RUNS):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn(ctx, *args)
        ctx.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    per_round = []
    fn(ctx, *args, per_round)
    return min(times), max(times), per_round


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = ffi.Context(0)
    lines = []
    for name, n, n_aux in (("bytecode: 4 chunks of 2^22 + value + eq", 22, 4), ("advice: 2^20, no passengers", 20, 0)):
        value, eq = rand_table(ctx, n, 1), rand_table(ctx, n, 2)
        aux = [rand_table(ctx, n, 3 + i) for i in range(n_aux)]
        ch = challenges(n, 9)
        args = (value, eq, aux, n, ch)
        a_out, b_out = fused(ctx, *args), composed(ctx, *args)
        assert np.array_equal(a_out, b_out), "the two routes disagree on the final claims"
        f_lo, f_hi, f_rounds = measure(ctx, fused, args)
        c_lo, c_hi, c_rounds = measure(ctx, composed, args)
        traffic = (2 + n_aux) * (1 << n) * 32 * 1.5
        lines.append(f"{name}")
        lines.append(f"  fused    {f_lo:8.3f} .. {f_hi:8.3f} ms   (round 1: {f_rounds[1] * 1e3:.3f} ms, {traffic / f_rounds[1] / 1e12:.2f} TB/s of {traffic / 2**20:.0f} MiB algorithmic)")
        lines.append(f"  composed {c_lo:8.3f} .. {c_hi:8.3f} ms   (round 1: {c_rounds[1] * 1e3:.3f} ms, {traffic / c_rounds[1] / 1e12:.2f} TB/s of the same bytes)")
        spread = max(f_hi - f_lo, c_hi - c_lo)
        verdict = "fused ahead by more than the spread" if c_lo - f_hi > 0 and c_lo - f_lo > spread else ("composed ahead by more than the spread" if f_lo - c_hi > 0 and f_lo - c_lo > spread else "within the spread of the runs")
        lines.append(f"  composed / fused (smallest) = {c_lo / f_lo:.2f}; spread of the runs {spread:.3f} ms: {verdict}")
        for t in [value, eq] + aux:
            t.free()
    lines.append("k_bind_low_to_high alone (DESIGN.md section 3.2): 6.1 TB/s of its algorithmic traffic")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
