"""Dory-Reduce on resident vectors: the prover's side of the reduce-and-fold rounds of a Dory opening, driven on the layer above the C ABI.

The state is the witness vectors v1 (G1) and v2 (G2), the scalar vectors s1 and s2 (Fr) of the scalar-product extension, the bases Gamma1 (G1) and Gamma2 (G2) with
Gamma2's prepared line table, and the length n (a power of two).  One round is

    first_message()      D1L = <v1_L, Gamma2'>, D1R = <v1_R, Gamma2'>, D2L = <Gamma1', v2_L>, D2R = <Gamma1', v2_R>, E1beta = <Gamma1, s2>, E2beta = <s1, Gamma2>
    apply_beta(b, 1/b)   v1 += b Gamma1, v2 += (1/b) Gamma2
    second_message()     C+ = <v1_L, v2_R>, C- = <v1_R, v2_L>, E1+ = <v1_L, s2_R>, E1- = <v1_R, s2_L>, E2+ = <s1_L, v2_R>, E2- = <s1_R, v2_L>
    apply_alpha(a, 1/a)  v1 <- a v1_L + v1_R, v2 <- (1/a) v2_L + v2_R, s1 <- a s1_L + s1_R, s2 <- (1/a) s2_L + s2_R, n <- n / 2

with X' the first half of X, X_L / X_R the halves of the current vector.  Each message is ONE Context.dory_products call (one launch set, one synchronisation);
the updates are enqueued in place and never leave the device.  The caller hands in every challenge -- the transcript, the GT scalings of the verifier's side and
the final scalar-product message stay with the caller.

These are the definitions of the Dory paper (Lee, "Dory: Efficient, Transparent arguments for Generalised Inner Products and Polynomial Commitments", Dory-Reduce
with the scalar-product extension).  Which half a crate's own messages call left, their order, and which of alpha / 1/alpha folds which vector are that crate's
choice; the C layer takes views and scalars and is agnostic about it, only this module embodies the paper's (docs/parity.md).
"""
import numpy as np

from . import ffi


class DoryReduce:
    def __init__(self, ctx, v1, v2, s1, s2, gamma1, gamma2):
        """v1, gamma1: (n, 12) G1 points; v2, gamma2: (n, 24) G2 points; s1, s2: (n, 4) Fr; n a power of two.  Everything is checked and uploaded once, here."""
        n = np.asarray(v1).reshape(-1, 12).shape[0]
        if n == 0 or n & (n - 1):
            raise ValueError("the length of a Dory-Reduce is a power of two")
        self.ctx, self.n = ctx, n
        self._owned = []
        up = lambda kind, a: self._keep(ctx.dory_vec_upload(kind, a))  # noqa: E731
        self.v1, self.gamma1 = up(ffi.DORY_KIND_G1, v1), up(ffi.DORY_KIND_G1, gamma1)
        self.v2, self.gamma2 = up(ffi.DORY_KIND_G2, v2), up(ffi.DORY_KIND_G2, gamma2)
        self.s1, self.s2 = up(ffi.DORY_KIND_FR, s1), up(ffi.DORY_KIND_FR, s2)
        if any(len(v) != n for v in self._owned):
            self.close()
            raise ValueError("the vectors of a Dory-Reduce have one length")
        self.gamma2_prepared = ctx.dory_g2_prepare_vec(self.gamma2)  # once: a prefix of the table serves every later round
        self._owns_prepared = True
        self._one = ffi.host_fr_from_u64(1)

    @classmethod
    def from_resident(cls, ctx, v1, v2, s1, s2, gamma1, gamma2, gamma2_prepared):
        """The same reduction over six vectors that are on the device already (DoryVec) and the prepared table of gamma2, all of them the caller's: nothing is
        uploaded, and close() frees none of them.  v1, v2, s1, s2 have one length n, a power of two, and are folded in place (truncated to one element at the end);
        the bases and the table hold at least n elements and are only read."""
        n = len(v1)
        if n == 0 or n & (n - 1):
            raise ValueError("the length of a Dory-Reduce is a power of two")
        if any(len(v) != n for v in (v2, s1, s2)):
            raise ValueError("the vectors of a Dory-Reduce have one length")
        if len(gamma1) < n or len(gamma2) < n or gamma2_prepared.n < n:
            raise ValueError("the bases of a Dory-Reduce are at least as long as its vectors")
        self = cls.__new__(cls)
        self.ctx, self.n = ctx, n
        self._owned = []
        self.v1, self.v2, self.s1, self.s2, self.gamma1, self.gamma2 = v1, v2, s1, s2, gamma1, gamma2
        self.gamma2_prepared = gamma2_prepared
        self._owns_prepared = False
        self._one = ffi.host_fr_from_u64(1)
        return self

    def _keep(self, v):
        self._owned.append(v)
        return v

    def close(self):
        for v in self._owned:
            v.free()
        self._owned = []
        if getattr(self, "gamma2_prepared", None) is not None:
            if self._owns_prepared:
                self.gamma2_prepared.free()
            self.gamma2_prepared = None

    def _inverse_pair(self, x, x_inv, name):
        x, x_inv = ffi.fr(x).reshape(4), ffi.fr(x_inv).reshape(4)
        if not np.array_equal(ffi.host_fr_mul(x, x_inv), self._one):
            raise ValueError(f"{name} times its inverse is not one")
        return x, x_inv

    def _halves(self, v):
        h = self.n // 2
        return (v, 0, h), (v, h, h)

    def first_message(self):
        """(D1L, D1R, D2L, D2R, E1beta, E2beta): four GT elements, one G1 and one G2 point"""
        if self.n < 2:
            raise ValueError("a vector of one element is not reduced further")
        n, h = self.n, self.n // 2
        (v1l, v1r), (v2l, v2r) = self._halves(self.v1), self._halves(self.v2)
        g1_half = (self.gamma1, 0, h)
        I = ffi.dory_item  # noqa: E741
        return tuple(self.ctx.dory_products([
            I(ffi.DORY_PAIR, v1l, self.gamma2_prepared), I(ffi.DORY_PAIR, v1r, self.gamma2_prepared),
            I(ffi.DORY_PAIR, g1_half, v2l), I(ffi.DORY_PAIR, g1_half, v2r),
            I(ffi.DORY_MSM_G1, (self.gamma1, 0, n), (self.s2, 0, n)), I(ffi.DORY_MSM_G2, (self.gamma2, 0, n), (self.s1, 0, n))]))

    def apply_beta(self, beta, beta_inv):
        beta, beta_inv = self._inverse_pair(beta, beta_inv, "beta")
        n = self.n
        self.ctx.dory_vec_scale_bases_add((self.gamma1, 0, n), (self.v1, 0, n), beta)
        self.ctx.dory_vec_scale_bases_add((self.gamma2, 0, n), (self.v2, 0, n), beta_inv)

    def second_message(self):
        """(C+, C-, E1+, E1-, E2+, E2-): two GT elements, two G1 and two G2 points"""
        if self.n < 2:
            raise ValueError("a vector of one element is not reduced further")
        (v1l, v1r), (v2l, v2r) = self._halves(self.v1), self._halves(self.v2)
        (s1l, s1r), (s2l, s2r) = self._halves(self.s1), self._halves(self.s2)
        I = ffi.dory_item  # noqa: E741
        return tuple(self.ctx.dory_products([
            I(ffi.DORY_PAIR, v1l, v2r), I(ffi.DORY_PAIR, v1r, v2l),
            I(ffi.DORY_MSM_G1, v1l, s2r), I(ffi.DORY_MSM_G1, v1r, s2l),
            I(ffi.DORY_MSM_G2, v2r, s1l), I(ffi.DORY_MSM_G2, v2l, s1r)]))

    def apply_alpha(self, alpha, alpha_inv):
        alpha, alpha_inv = self._inverse_pair(alpha, alpha_inv, "alpha")
        if self.n < 2:
            raise ValueError("a vector of one element is not reduced further")
        h = self.n // 2
        (v1l, v1r), (v2l, v2r) = self._halves(self.v1), self._halves(self.v2)
        (s1l, s1r), (s2l, s2r) = self._halves(self.s1), self._halves(self.s2)
        self.ctx.dory_vec_scale_vs_add(v1l, v1r, alpha)
        self.ctx.dory_vec_scale_vs_add(v2l, v2r, alpha_inv)
        self.ctx.dory_vec_fold_field(s1l, s1r, alpha)
        self.ctx.dory_vec_fold_field(s2l, s2r, alpha_inv)
        for v in (self.v1, self.v2, self.s1, self.s2):
            v.truncate(h)
        self.n = h

    def round(self, beta, beta_inv, alpha, alpha_inv):
        """one whole round; the two messages"""
        first = self.first_message()
        self.apply_beta(beta, beta_inv)
        second = self.second_message()
        self.apply_alpha(alpha, alpha_inv)
        return first, second
