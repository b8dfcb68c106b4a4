"""The two groups of the Dory routine tests behind one interface: points are made and checked through their discrete logarithms to the group's generator, so
the expected value of every routine is plain arithmetic modulo r and ONE reference scalar multiplication -- the oracle's for G1 (oracle_lib.g1_*), the
big-integer model's for G2 (g2_model)."""
import numpy as np

import g2_model as M
import oracle_lib as O

R = O.R_MOD
# the shared scalars of the issue: 0, 1, 2, r - 1, and 2^253 - 1 (non-adjacent form 2^253 - 1: the longest carry, into the spare top digit)
SHARED_SCALARS = [0, 1, 2, R - 1, (1 << 253) - 1]


def fr_int(k):
    """the integer k (mod r) as one Montgomery element, (4,) uint64"""
    return O.to_mont([k % R])[0]


def fr_ints(ks):
    return O.to_mont([k % R for k in ks]) if len(ks) else np.zeros((0, 4), dtype=np.uint64)


def rand_ints(n, seed):
    rng = np.random.default_rng(seed)
    return [int.from_bytes(rng.bytes(40), "little") % R for _ in range(n)]


class G1:
    name, width = "g1", 12
    _gen = None

    @classmethod
    def point(cls, k, rep=0):
        """k * generator as the oracle's Jacobian point (its own representative; `rep` is accepted for symmetry with G2)"""
        if k % R == 0:
            return O.g1_identity()
        if cls._gen is None:
            cls._gen = O.g1_generator()
        return O.g1_scalar_mul(cls._gen, fr_int(k))

    @classmethod
    def same(cls, a, k):
        return O.g1_on_curve(a) and O.g1_eq(a, cls.point(k))

    @staticmethod
    def z_is_zero(a):
        return not np.asarray(a)[8:12].any()


class G2:
    name, width = "g2", 24

    @staticmethod
    def point(k, rep=0):
        """k * generator; rep != 0 picks another Jacobian representative (z = rep + (rep + 1) u)"""
        return M.to_abi(M.mul_generator(k), M.f2(rep, rep + 1) if rep else None)

    @staticmethod
    def same(a, k):
        p = M.from_abi(a)
        return M.on_curve(p) and p == M.mul_generator(k)

    @staticmethod
    def z_is_zero(a):
        return not np.asarray(a)[16:24].any()


GROUPS = [G1, G2]


def progression(G, k0, d, n):
    """the discrete logarithms k0 + i d and their points, built with n reference ADDITIONS (a reference multiplication per element would cost the GPU tests
    seconds at n = 2^10); every third G2 point in a Jacobian representative of its own"""
    ks = [(k0 + i * d) % R for i in range(n)]
    out = np.zeros((n, G.width), dtype=np.uint64)
    if n == 0:
        return ks, out
    if G is G1:
        p, step = G1.point(k0), G1.point(d)
        for i in range(n):
            out[i] = p
            p = O.g1_add(p, step)
    else:
        p, step = M.mul_generator(k0), M.mul_generator(d)
        for i in range(n):
            out[i] = M.to_abi(p, M.f2(i + 2, i + 3) if i % 3 == 1 else None)
            p = M.add(p, step)
    return ks, out


def plant(G, ks, pts, i, k):
    """element i becomes k * generator"""
    ks[i] = k % R
    pts[i] = G.point(k, rep=i + 1)
