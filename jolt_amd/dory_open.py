"""A Dory evaluation proof on resident vectors: the prover's side of Eval-VMV-RE in transparent mode, from the committed hints to the final message, driven on the
layer above the C ABI as dory_reduce.py drives the rounds.

The polynomial is a 2^nu x 2^sigma matrix M (nu <= sigma) with row commitments T'_i = <M_i, Gamma1[:2^sigma]> and commitment T = <T', Gamma2[:2^nu]>; the evaluation
is y = L^T M R for L of 2^nu and R of 2^sigma entries.  With n = 2^sigma, T' padded to n with the identity and L padded to n with zero, and v = L^T M:

    state                v1 = T' (padded), v2[i] = v[i] H2, s1 = R, s2 = L (padded)
    vmv_message()        C = <v1, v2>, D2 = <Gamma1[:n], v2>, E1 = <v1, s2>                     -- ONE Context.dory_products call; the two pairings share the view v2
    reduce               sigma rounds of DoryReduce over the state: first message, beta, second message, alpha
    final_message(g, 1/g)  w1 = v1 + (g s1) H1, w2 = v2 + ((1/g) s2) H2 over the single remaining elements

The state is built on the device: v1 by jolt_dory_state_combine_hints from resident hints into a vector of identities, v2 by jolt_dory_state_fixed_base_mul from the
entries of the device table v, s1 and s2 by device copies of the tables R and L (s2 into a vector of zeros).  Only the messages come back, and the 64 bytes of
s1[0] and s2[0] for the two Fr products of the final message.  The caller hands in every challenge: the transcript, the verifier's GT scalings and commit_blind
stay with the caller.  Transparent mode only -- no blinds.

These are the definitions of the Dory paper (Lee, "Dory: Efficient, Transparent arguments for Generalised Inner Products and Polynomial Commitments", Eval-VMV-RE
over Dory-Reduce with the scalar-product extension, non-hiding), with the conventions of dory_reduce.py: alpha folds v1 and s1, 1/alpha folds v2 and s2.  The
names (C, D2, E1) and their order are the ones crates/jolt-dory/src/types.rs:219-231 reads off the wire; the order of the round messages, the final exponent and
the generators are dory-pcs's choice, which nothing in the reference checkout pins (docs/parity.md).  The C layer takes views and scalars and is agnostic about
all of it; only this module and dory_reduce.py embody the paper's protocol.
"""
import numpy as np

from . import ffi
from .dory_reduce import DoryReduce


class DorySetup:
    """Gamma1 (G1) and Gamma2 (G2), N points each, N a power of two, uploaded once; Gamma2's line table, prepared once; H1 and H2.  Serves every opening and
    tier-2 commitment of at most N columns."""

    def __init__(self, ctx, gamma1, gamma2, h1, h2):
        self.ctx = ctx
        self._made = []
        self.gamma2_prepared = None
        try:
            self.gamma1 = self._keep(ctx.dory_vec_upload(ffi.DORY_KIND_G1, gamma1))
            self.gamma2 = self._keep(ctx.dory_vec_upload(ffi.DORY_KIND_G2, gamma2))
            self.n = len(self.gamma1)
            if self.n == 0 or self.n & (self.n - 1) or len(self.gamma2) != self.n:
                raise ValueError("Gamma1 and Gamma2 have one length, a power of two")
            self.h1 = np.ascontiguousarray(h1, dtype=np.uint64).reshape(12).copy()
            self.h2 = np.ascontiguousarray(h2, dtype=np.uint64).reshape(24).copy()
            self.h1_vec = self._keep(ctx.dory_vec_upload(ffi.DORY_KIND_G1, self.h1))  # checked here, once; the bases of the final message
            self.h2_vec = self._keep(ctx.dory_vec_upload(ffi.DORY_KIND_G2, self.h2))
            self.gamma2_prepared = ctx.dory_g2_prepare_vec(self.gamma2)
        except Exception:
            self.close()
            raise

    def _keep(self, v):
        self._made.append(v)
        return v

    def close(self):
        for v in self._made:
            v.free()
        self._made = []
        if self.gamma2_prepared is not None:
            self.gamma2_prepared.free()
            self.gamma2_prepared = None


def dory_commit_tier2(setup, hint_vec):
    """T = <hint, Gamma2[:rows]> for a resident G1 vector of row commitments (DoryVec or a view of one): one PAIR item against the prepared table"""
    return setup.ctx.dory_products([ffi.dory_item(ffi.DORY_PAIR, hint_vec, setup.gamma2_prepared)])[0]


class DoryOpening:
    def __init__(self, setup, hints, scalars, v_table, left, right, nu, sigma):
        """hints: resident G1 vectors (DoryVec, or views) of at most 2^nu row commitments each, in the row order jolt_dory_combine_hints documents; scalars: one Fr
        per hint; v_table: device table of the 2^sigma entries of L^T M (jolt_dory_fold_rows_grid's output for a batch); left, right: device tables of 2^nu and
        2^sigma entries.  Everything is checked here, before anything is enqueued; the inputs stay the caller's."""
        if nu > sigma:
            raise ValueError("the matrix of a Dory opening has at most as many rows as columns: nu <= sigma")
        rows, n = 1 << nu, 1 << sigma
        if n > setup.n:
            raise ValueError("the setup holds fewer than 2^sigma bases")
        self.hints = [ffi._dory_view(h) for h in hints]
        if not self.hints:
            raise ValueError("an opening combines at least one hint")
        self.scalars = np.stack([ffi.fr(c).reshape(4) for c in scalars]) if len(scalars) else ffi.fr_array(0)
        if self.scalars.shape[0] != len(self.hints):
            raise ValueError("one scalar per hint")
        if any(v.kind != ffi.DORY_KIND_G1 or r > rows for v, _, r in self.hints):
            raise ValueError("a hint is a G1 vector of at most 2^nu rows")
        if len(v_table) != n or len(right) != n or len(left) != rows:
            raise ValueError("v and right have 2^sigma entries, left has 2^nu")
        self.setup, self.ctx, self.nu, self.sigma = setup, setup.ctx, nu, sigma
        self.v_table, self.left, self.right = v_table, left, right
        self._state = []
        self.v1 = self.v2 = self.s1 = self.s2 = None
        self.reduce = None
        self._vmv = self._final = None
        self._one = ffi.host_fr_from_u64(1)

    # ---- the state, in the three steps tools/bench_dory_open.py times ----
    def _alloc(self, kind):
        v = self.ctx.dory_state_alloc(kind, 1 << self.sigma)
        self._state.append(v)
        return v

    def _build_v1(self):
        self.v1 = self._alloc(ffi.DORY_KIND_G1)  # identities: the rows from 2^nu on stay the padding
        self.ctx.dory_state_combine_hints(self.hints, self.scalars, self.v1)

    def _build_scalars(self):
        n, rows = 1 << self.sigma, 1 << self.nu
        self.s1, self.s2, self._v = self._alloc(ffi.DORY_KIND_FR), self._alloc(ffi.DORY_KIND_FR), self._alloc(ffi.DORY_KIND_FR)
        self.ctx.dory_state_from_table(self.right, (self.s1, 0, n))
        self.ctx.dory_state_from_table(self.left, (self.s2, 0, rows))  # zeros from 2^nu on
        self.ctx.dory_state_from_table(self.v_table, (self._v, 0, n))

    def _build_v2(self):
        self.v2 = self._alloc(ffi.DORY_KIND_G2)
        self.ctx.dory_state_fixed_base_mul(ffi.DORY_KIND_G2, self.setup.h2, self._v, self.v2)

    def build_state(self):
        """v1, v2, s1, s2 on the device, and the DoryReduce over them; vmv_message() calls it"""
        if self.reduce is not None:
            return
        try:
            if self.v1 is None:
                self._build_v1()
            if self.s1 is None:
                self._build_scalars()
            if self.v2 is None:
                self._build_v2()
            self.reduce = DoryReduce.from_resident(self.ctx, self.v1, self.v2, self.s1, self.s2, self.setup.gamma1, self.setup.gamma2, self.setup.gamma2_prepared)
        except Exception:
            self.close()
            raise

    def vmv_message(self):
        """(C, D2, E1): two GT elements and one G1 point, ahead of the rounds"""
        if self._vmv is None:
            self.build_state()
            if self.reduce.n != 1 << self.sigma:
                raise ValueError("the VMV message is taken before the first round")
            n = 1 << self.sigma
            I = ffi.dory_item  # noqa: E741
            v2 = (self.v2, 0, n)
            self._vmv = tuple(self.ctx.dory_products([
                I(ffi.DORY_PAIR, (self.v1, 0, n), v2), I(ffi.DORY_PAIR, (self.setup.gamma1, 0, n), v2), I(ffi.DORY_MSM_G1, (self.v1, 0, n), (self.s2, 0, n))]))
        return self._vmv

    def final_message(self, gamma, gamma_inv):
        """(w1, w2): one G1 and one G2 point, after the last round (fold-scalars under gamma)"""
        if self.reduce is None or self.reduce.n != 1:
            raise ValueError("the final message follows the last round: one element per vector")
        gamma, gamma_inv = ffi.fr(gamma).reshape(4), ffi.fr(gamma_inv).reshape(4)
        if not np.array_equal(ffi.host_fr_mul(gamma, gamma_inv), self._one):
            raise ValueError("gamma times its inverse is not one")
        if self._final is not None:
            raise ValueError("the final message was taken: v1 and v2 hold it")
        s1, s2 = self.s1.download(0, 1)[0], self.s2.download(0, 1)[0]
        self.ctx.dory_vec_scale_bases_add((self.setup.h1_vec, 0, 1), (self.v1, 0, 1), ffi.host_fr_mul(gamma, s1))
        self.ctx.dory_vec_scale_bases_add((self.setup.h2_vec, 0, 1), (self.v2, 0, 1), ffi.host_fr_mul(gamma_inv, s2))
        self._final = (self.v1.download(0, 1)[0], self.v2.download(0, 1)[0])
        return self._final

    def close(self):
        if self.reduce is not None:
            self.reduce.close()
            self.reduce = None
        for v in self._state:
            v.free()
        self._state = []
