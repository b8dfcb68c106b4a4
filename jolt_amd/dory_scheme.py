"""DoryScheme::{commit, open} for ONE polynomial held as field elements on the device (crates/jolt-dory/src/scheme.rs): the reference's headline use of its PCS,
commit to a random multilinear polynomial and open it at a point.

A table of 2^n evaluations is the 2^nu x 2^sigma matrix M[r][c] = table[r * 2^sigma + c] with sigma = ceil(n / 2) and nu = n - sigma (scheme.rs:242-243):

    commit(setup, srs, table)   the row commitments T'_r = <M_r, Gamma1[:2^sigma]> by jolt_dory_hints_rows_fr into a resident G1 vector (the hint), and the
                                commitment T = <T', Gamma2[:2^nu]> as one PAIR item against the prepared Gamma2
    open(setup, table, hint, point)
                                L = eq(point[:nu]) and R = eq(point[nu:]) by the library's eq expansion, v = L^T M by jolt_dory_fold_rows_blocks (one table, sigma_d =
                                sigma, no base: the dense vector_matrix_product of scheme.rs:612-618), and a dory_open.DoryOpening over them

The library's tables are indexed with point[0] on the most significant bit (jolt_eq_evals), so the matrix row r takes the first nu coordinates and
L^T M R = sum_i eq(point, i) table[i] is the table's multilinear evaluation at the point.  Challenges are handed in, as everywhere in this layer: the opening
that open() returns is driven message by message like any DoryOpening.
"""
import numpy as np

from . import ffi
from .dory_open import DoryOpening, dory_commit_tier2


def matrix_shape(length):
    """(nu, sigma) of a table of `length` = 2^n evaluations: sigma = ceil(n / 2), nu = n - sigma"""
    if length <= 0 or length & (length - 1):
        raise ValueError("a polynomial has a power of two of evaluations")
    n = length.bit_length() - 1
    sigma = (n + 1) // 2
    return n - sigma, sigma


def _check(setup, table, n_srs=None):
    nu, sigma = matrix_shape(len(table))
    if 1 << sigma > setup.n:
        raise ValueError("the setup holds fewer than 2^sigma bases")
    if n_srs is not None and 1 << sigma > n_srs:
        raise ValueError("the SRS holds fewer than 2^sigma bases")
    return nu, sigma


def commit(setup, srs, table):
    """(T, hint): the GT commitment (48 words) and the resident G1 vector of the 2^nu normalised row commitments; the hint is the caller's to free.
    srs: a jolt_srs over Gamma1's first 2^sigma points at least.  Shapes are checked before anything is enqueued."""
    nu, sigma = _check(setup, table, len(srs))
    ctx = setup.ctx
    hint = ctx.dory_state_alloc(ffi.DORY_KIND_G1, 1 << nu)
    try:
        ctx.dory_hints_rows_fr(srs, table, 1 << sigma, hint)
        return dory_commit_tier2(setup, hint), hint
    except Exception:
        hint.free()
        raise


class DorySchemeOpening:
    """open(): the DoryOpening of one table at one point, with the tables it made (L, R, v = L^T M); .opening takes the challenges, .close() frees all of it"""

    def __init__(self, setup, table, hint, point):
        nu, sigma = _check(setup, table)
        point = ffi.fr(np.ascontiguousarray(point, dtype=np.uint64)).reshape(-1, 4)
        if point.shape[0] != nu + sigma:
            raise ValueError("the point has one coordinate per variable")
        view = ffi._dory_view(hint)
        if view[0].kind != ffi.DORY_KIND_G1 or view[2] != 1 << nu:
            raise ValueError("the hint is a G1 vector of 2^nu row commitments")
        ctx = setup.ctx
        self.nu, self.sigma = nu, sigma
        self._tables = []
        self.opening = None
        try:
            one = ffi.host_fr_from_u64(1)
            # nu = 0 (n <= 1): the single row has L = (1)
            self.left = self._keep(ctx.eq_evals(point[:nu]) if nu else ctx.upload(one.reshape(1, 4)))
            self.right = self._keep(ctx.eq_evals(point[nu:]) if sigma else ctx.upload(one.reshape(1, 4)))
            self.v = self._keep(ctx.dory_fold_rows_blocks([table], [sigma], [one], sigma, self.left))
            self.opening = DoryOpening(setup, [view], [one], self.v, self.left, self.right, nu, sigma)
        except Exception:
            self.close()
            raise

    def _keep(self, t):
        self._tables.append(t)
        return t

    def evaluation(self):
        """y = L^T M R = <v, R>, the table's multilinear evaluation at the point (one Fr)"""
        return self.opening.ctx.table_dot(self.v, self.right)

    def close(self):
        if self.opening is not None:
            self.opening.close()
            self.opening = None
        for t in self._tables:
            t.free()
        self._tables = []


def open(setup, table, hint, point):  # noqa: A001 -- the reference's name
    return DorySchemeOpening(setup, table, hint, point)


def prove(setup, table, hint, point, transcript):
    """The same opening as ONE call of the library under a transcript (dory_proof.prove): setup is a dory_proof.DoryProofSetup over the bases commit() was given,
    transcript a HostTranscript.  (proof, y): the DoryProof and the evaluation y = L^T M R (one Fr)."""
    from . import dory_proof
    nu, sigma = _check(setup, table)
    point = ffi.fr(np.ascontiguousarray(point, dtype=np.uint64)).reshape(-1, 4)
    if point.shape[0] != nu + sigma:
        raise ValueError("the point has one coordinate per variable")
    view = ffi._dory_view(hint)
    if view[0].kind != ffi.DORY_KIND_G1 or view[2] != 1 << nu:
        raise ValueError("the hint is a G1 vector of 2^nu row commitments")
    ctx = setup.ctx
    one = ffi.host_fr_from_u64(1)
    tables = []
    try:
        tables.append(ctx.eq_evals(point[:nu]) if nu else ctx.upload(one.reshape(1, 4)))
        tables.append(ctx.eq_evals(point[nu:]) if sigma else ctx.upload(one.reshape(1, 4)))
        left, right = tables
        tables.append(ctx.dory_fold_rows_blocks([table], [sigma], [one], sigma, left))
        v = tables[2]
        proof = dory_proof.prove(setup, [view], [one], v, left, right, nu, sigma, transcript=transcript)
        return proof, ctx.table_dot(v, right)
    finally:
        for t in tables:
            t.free()
