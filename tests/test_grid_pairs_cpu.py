"""CPU: the entry arithmetic and the index map of the commitment grid's pair tables (csrc/grid_pairs.hip.h), through their host twins.

An entry is the affine sum p + q stored in the bucket kernels' radix, (0, 0) for the point at infinity.  The stored words are taken back to a point with Python
integers and compared with the oracle's addition as group elements and in compressed form, for generic operands, a doubling, a cancellation and operands at
infinity."""
import numpy as np

import oracle_lib as O
from jolt_amd import ffi
from util import rand_fr


def stored_point(words):
    """the point behind an entry's words: a stored coordinate is the standard Montgomery form of 32 x (fq_limb.hip.h), undone here with Python integers"""
    if not words.any():
        return O.g1_identity()
    inv32 = pow(32, -1, O.Q_MOD)
    x, y = (v * inv32 % O.Q_MOD for v in O.from_mont(words.reshape(2, 4), O.Q_MOD))
    assert (y * y - x * x * x - 3) % O.Q_MOD == 0  # on the curve
    return O.to_mont([x, y, 1], O.Q_MOD).reshape(12)


def same_point(a, b):
    return O.g1_eq(a, b) and O.g1_serialize_compressed(a) == O.g1_serialize_compressed(b)


def test_pair_entry_is_the_oracles_sum_for_generic_and_degenerate_operands():
    pts = O.srs_setup_from_secret(rand_fr(1, 7001)[0], 6)  # Jacobian with z = 1 ...
    p, q = pts[1], pts[4]
    p_scaled = O.g1_add(O.g1_double(p), O.g1_neg(p))  # ... and the same point with another z
    inf = O.g1_identity()
    cases = {"generic": (p, q), "generic, other z": (p_scaled, q), "doubling": (p, p), "doubling, other z": (p_scaled, p), "negation": (p, O.g1_neg(p)),
             "negation, other z": (O.g1_neg(p_scaled), p), "inf + q": (inf, q), "p + inf": (p, inf), "inf + inf": (inf, inf)}
    for name, (a, b) in cases.items():
        words = ffi.host_grid_pair_entry(a, b)
        want = O.g1_add(a, b)
        assert same_point(stored_point(words), want), name
        assert (not words.any()) == O.g1_is_identity(want), name  # (0, 0) is the marker of infinity, and only that
    assert same_point(stored_point(ffi.host_grid_pair_entry(p, p)), O.g1_double(p))
    assert np.array_equal(ffi.host_grid_pair_entry(p, q), ffi.host_grid_pair_entry(p_scaled, q))  # canonical words: a function of the points alone
    assert np.array_equal(ffi.host_grid_pair_entry(inf, q), ffi.host_grid_pair_entry(q, inf))


def test_pair_index_map_matches_its_restatement():
    for k in (1, 4, 16):
        seen = set()
        for m in (0, 1, 2, 5, (1 << 21) - 1):
            for a in range(k):
                for b in range(k):
                    i = ffi.host_grid_pair_index(m, k, a, b)
                    assert i == (m * k + a) * k + b
                    seen.add(i)
        assert len(seen) == 5 * k * k  # one slot per (m, a, b)
        # the k^2 candidates of one pair position are one contiguous block
        assert [ffi.host_grid_pair_index(3, k, a, b) for a in range(k) for b in range(k)] == list(range(3 * k * k, 4 * k * k))
