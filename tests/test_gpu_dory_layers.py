"""GPU: the two layers under Dory's entry points.  The host-pointer entries (dory_routines.hip) and the resident entries (dory_resident.hip) enqueue the same
kernels through one launch layer (dory_kernels.hip.h), so they give the same WORDS, not only the same group elements; and the phase clocks of the host-pointer
entries (jolt_dory_routines_timing, jolt_dory_pairing_timing) keep the indices include/jolt_hip.h states.  What the routines compute is pinned against the
reference in test_gpu_dory_routines.py / test_gpu_dory_resident.py; nothing here is compared with a model."""
import math
import time

import numpy as np
import pytest

from dory_groups import GROUPS, fr_int, fr_ints, plant, progression, rand_ints
from jolt_amd import ffi

pytestmark = pytest.mark.gpu
KIND = {"g1": ffi.DORY_KIND_G1, "g2": ffi.DORY_KIND_G2}
MSM_OP = {"g1": ffi.DORY_MSM_G1, "g2": ffi.DORY_MSM_G2}
N = 65  # one full wavefront and one lane alone in the second
MSM_LENGTHS = (1, 2, 63, 64, 65, 129)  # the odd levels of the addition tree


@pytest.fixture(scope="module")
def ctx():
    c = ffi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pool():
    """per group 2 x 129 points, the identity at lanes 0 and 64 of both; 129 scalars; never written"""
    pts = {}
    for j, G in enumerate(GROUPS):
        k0, dk, l0, dl = rand_ints(4, 900 + j)
        ks, a = progression(G, k0, dk, 129)
        ls, b = progression(G, l0, dl, 129)
        for i in (0, 64):
            plant(G, ks, a, i, 0)
            plant(G, ls, b, i, 0)
        pts[G.name] = (a, b)
    return pts, fr_ints(rand_ints(129, 902)), fr_int(rand_ints(1, 903)[0])


def test_host_pointer_entries_give_the_resident_entries_words(ctx, pool):
    pts, frs, s = pool
    for G in GROUPS:
        g, kind = G.name, KIND[G.name]
        a, b = pts[g][0][:N], pts[g][1][:N]
        up = lambda host, k=kind: ctx.dory_vec_upload(k, host)  # noqa: E731
        # vs += s * bases
        va, vb = up(a), up(b)
        ctx.dory_vec_scale_bases_add(va, vb, s)
        assert np.array_equal(getattr(ctx, f"dory_{g}_scale_bases_add")(a, b, s), vb.download()), g
        # vs = s * vs + addends
        vc = up(b)
        ctx.dory_vec_scale_vs_add(vc, va, s)
        assert np.array_equal(getattr(ctx, f"dory_{g}_scale_vs_add")(b, a, s), vc.download()), g
        # out[i] = scalars[i] * base
        vs, out = up(frs[:N], ffi.DORY_KIND_FR), ctx.dory_state_alloc(kind, N)
        ctx.dory_state_fixed_base_mul(kind, a[1], vs, out)
        assert np.array_equal(getattr(ctx, f"dory_{g}_fixed_base_mul")(a[1], frs[:N]), out.download()), g
        for v in (va, vb, vc, vs, out):
            v.free()
        # sums of n terms against a batch of one item
        bases, scalars = up(pts[g][0]), up(frs, ffi.DORY_KIND_FR)
        for n in MSM_LENGTHS:
            (batch,) = ctx.dory_products([ffi.dory_item(MSM_OP[g], (bases, 0, n), (scalars, 0, n))])
            assert np.array_equal(getattr(ctx, f"dory_{g}_msm")(pts[g][0][:n], frs[:n]), batch), (g, n)
        bases.free()
        scalars.free()
    left, right = ctx.dory_vec_upload(ffi.DORY_KIND_FR, frs[:N]), ctx.dory_vec_upload(ffi.DORY_KIND_FR, frs[N - 1:2 * N - 1])
    ctx.dory_vec_fold_field(left, right, s)
    assert np.array_equal(ctx.dory_fold_field_vectors(frs[:N], frs[N - 1:2 * N - 1], s), left.download())
    left.free()
    right.free()


def test_phase_clocks(ctx, pool):
    pts, frs, s = pool
    g1s, g2s = pts["g1"][0][:N], pts["g2"][0][:N]
    try:
        # ---- the routines: checks, host -> device, kernels, device -> host
        ctx.dory_routines_timing(True)
        t0 = time.perf_counter()
        ctx.dory_g1_scale_bases_add(g1s, pts["g1"][1][:N], s)
        wall = (time.perf_counter() - t0) * 1e3
        ms = ctx.dory_routines_timing(False)
        print("routines ms", ms, "wall", wall)
        assert len(ms) == 4 and all(math.isfinite(v) and v >= 0.0 for v in ms)
        assert ms[2] > 0.0
        assert sum(ms) <= wall  # the phases are sub-intervals of the call
        ctx.dory_g1_scale_bases_add(g1s, pts["g1"][1][:N], s)  # timing is off: the call touches no phase
        assert ctx.dory_routines_timing(False) == ms
        # ---- the pairings: checks, host -> device, prepare, Miller, product, device -> host, final exponentiation
        ctx.dory_pairing_timing(True)
        ctx.dory_multi_pair(g1s, g2s)
        ms = ctx.dory_pairing_timing(True)
        print("multi_pair ms", ms)
        assert len(ms) == 7 and all(math.isfinite(v) and v >= 0.0 for v in ms)
        assert ms[2] > 0.0 and ms[3] > 0.0 and ms[4] > 0.0 and ms[6] > 0.0
        prepared = ctx.dory_g2_prepare(g2s)
        ms = ctx.dory_pairing_timing(True)
        print("g2_prepare ms", ms)
        assert ms[3:] == (0.0, 0.0, 0.0, 0.0)
        ctx.dory_multi_pair_g2_setup(g1s, prepared)
        ms = ctx.dory_pairing_timing(False)
        print("multi_pair_g2_setup ms", ms)
        assert ms[2] == 0.0
        prepared.free()
    finally:
        ctx.dory_routines_timing(False)
        ctx.dory_pairing_timing(False)
