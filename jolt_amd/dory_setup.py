"""The bases of a Dory setup for the step: Gamma1, H1 in G1 and Gamma2, H2 in G2, generated from a seed.

    bases = generate(ctx, n, seed)      dict(gamma1 (n, 12), gamma2 (n, 24), h1 (12,), h2 (24,)): random multiples of the group generators, through the library's
                                        fixed-base routines (jolt_dory_g1_fixed_base_mul / jolt_dory_g2_fixed_base_mul)

The same dict is what DeviceWorkload(pcs="dory", dory_bases=...) takes, so a test can plant bases whose logarithms it knows.  This is a TRANSPARENT setup only in
the sense that the logarithms are thrown away: a production setup derives the bases by hashing to the curve, which nothing here does (dory-pcs's generator choice is
pinned by nothing in the reference checkout, docs/parity.md).  The timings of commitment and opening do not depend on which points the bases are.

G1's generator is (1, 2).  G2's generator is the point the test model (tests/g2_model.py) derives -- the first point of the twist y^2 = x^3 + 3 / (9 + u) with
x = 1, 2, ... (x in Fq), multiplied by the cofactor 2q - r -- written out here as a constant; tests/test_opening_batch_cpu.py holds it against that derivation.
"""
import numpy as np

Q = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47

# affine (x, y), each an Fq2 element (c0, c1), canonical integers
G2_GENERATOR = ((0x0717C5E8819CC397E17FF13EB1FB9E85595D28ADCFE99BE713BD9E60646014CE, 0x20391CF8DF1E17C18DA4A765A1AEE94F9A3D2B07DA6EEBB72BC28F5C42B0BD9A),
                (0x161B94AB47F657A4CB7CBD97D2BB6B8DE9EC87F3C35FE2BFEB3B468C43C09D9E, 0x27EF4F7C07B8829F711307683A9D7DEF634144A08E30C0596BDAEDE7FF70435A))


def _fq_mont(v):
    m = (v << 256) % Q
    return [(m >> (64 * i)) & (2**64 - 1) for i in range(4)]


def g1_generator():
    """(1, 2) as a (12,) Jacobian point in Montgomery limbs"""
    return np.array(_fq_mont(1) + _fq_mont(2) + _fq_mont(1), dtype=np.uint64)


def g2_generator():
    """G2_GENERATOR as a (24,) Jacobian point in Montgomery limbs: x.c0, x.c1, y.c0, y.c1, z = 1"""
    (x0, x1), (y0, y1) = G2_GENERATOR
    return np.array(_fq_mont(x0) + _fq_mont(x1) + _fq_mont(y0) + _fq_mont(y1) + _fq_mont(1) + _fq_mont(0), dtype=np.uint64)


def _rand_fr(n, rng):
    """n canonical field elements in Montgomery form: 31 random bytes each are below r, and every canonical value is some element's Montgomery form"""
    raw = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    raw[:, 31] = 0
    return np.ascontiguousarray(raw).view(np.uint64).reshape(n, 4)


def generate(ctx, n, seed):
    """the four bases of a setup of n = 2^sigma columns"""
    if n <= 0 or n & (n - 1):
        raise ValueError("a setup has a power of two of bases")
    rng = np.random.default_rng(seed)
    g1, g2 = g1_generator(), g2_generator()
    return dict(gamma1=ctx.dory_g1_fixed_base_mul(g1, _rand_fr(n, rng)), gamma2=ctx.dory_g2_fixed_base_mul(g2, _rand_fr(n, rng)),
                h1=ctx.dory_g1_fixed_base_mul(g1, _rand_fr(1, rng))[0], h2=ctx.dory_g2_fixed_base_mul(g2, _rand_fr(1, rng))[0])


def check(bases):
    """the arrays of a dory_bases= keyword, shaped: gamma1 (n, 12), gamma2 (n, 24), h1 (12,), h2 (24,), n a power of two"""
    missing = {"gamma1", "gamma2", "h1", "h2"} - set(bases)
    if missing:
        raise ValueError(f"dory_bases lacks {sorted(missing)}")
    out = dict(gamma1=np.ascontiguousarray(bases["gamma1"], dtype=np.uint64).reshape(-1, 12), gamma2=np.ascontiguousarray(bases["gamma2"], dtype=np.uint64).reshape(-1, 24),
               h1=np.ascontiguousarray(bases["h1"], dtype=np.uint64).reshape(12), h2=np.ascontiguousarray(bases["h2"], dtype=np.uint64).reshape(24))
    n = out["gamma1"].shape[0]
    if n == 0 or n & (n - 1) or out["gamma2"].shape[0] != n:
        raise ValueError("Gamma1 and Gamma2 have one length, a power of two")
    return out
