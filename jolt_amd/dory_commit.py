"""The Dory commitment of a whole witness on the device, in front of dory_open.DoryOpening: tier 1 into resident hints, tier 2 as one batch.

A column of the witness is a 2^nu x 2^sigma matrix in the cycle-major placement of jolt_dory_fold_rows_grid.  Its row commitments T'_i = <M_i, Gamma1[:2^sigma]> are the
column's OpeningHint, its commitment is T = <T', Gamma2[:rows]>:

    one-hot column p of a source   rows = k * chunks, chunks = cycles / 2^sigma; hint[row * chunks + chunk] = the sum of the bases of the cycles of that chunk whose hot
                                   address is `row` (finish_one_hot_column_major_chunks, crates/jolt-dory/src/streaming.rs:318-362); an empty row is the identity
    dense column                   rows = count / 2^sigma at address 0; hint[r] = sum_j values[r * 2^sigma + j] * Gamma1[j]

Every source is ONE jolt_dory_hints_onehot call over all of its columns, every dense column one jolt_dory_hints_rows call; both write normalised points in hint order
straight into resident G1 vectors, so nothing crosses the link between the witness and the first message of the opening.  `.hints` are views of those vectors,
`DoryOpening(setup, commitment.hints, ...)` takes them as they are, and `.commit()` is one Context.dory_products call with one PAIR item per column against the
setup's prepared Gamma2.
"""
from . import ffi


class DoryWitnessCommitment:
    def __init__(self, setup, srs, sources, dense, sigma):
        """setup: a dory_open.DorySetup; srs: a jolt_srs (ffi.Srs) over Gamma1's first 2^sigma points at least; sources: ffi.OneHot handles; dense: ffi.Ints columns.
        Every shape is checked here, before anything is enqueued; the inputs stay the caller's."""
        width = 1 << sigma
        if width > len(srs):
            raise ValueError("the SRS holds fewer than 2^sigma bases")
        shapes = []  # per vector: (source or column, rows per column, columns)
        for s in sources:
            if s.cycles % width:
                raise ValueError("2^sigma does not divide a source's cycle count")
            shapes.append((s, s.k * (s.cycles // width), s.n_polys))
        for d in dense:
            if d.count % width:
                raise ValueError("2^sigma does not divide a dense column's length")
            shapes.append((d, d.count // width, 1))
        if not shapes:
            raise ValueError("a witness has at least one column")
        if any(rows > setup.n for _, rows, _ in shapes):
            raise ValueError("a column has more rows than the setup has Gamma2 bases")
        self.setup, self.ctx, self.sigma = setup, setup.ctx, sigma
        self.hints = []
        self._vecs = []
        self._commitments = None
        try:
            for k, (col, rows, columns) in enumerate(shapes):
                vec = self.ctx.dory_state_alloc(ffi.DORY_KIND_G1, rows * columns)
                self._vecs.append(vec)
                if k < len(sources):
                    self.ctx.dory_hints_onehot(srs, col, vec, chunk_width=width)
                else:
                    self.ctx.dory_hints_rows(srs, col, width, vec)
                self.hints += [(vec, p * rows, rows) for p in range(columns)]
        except Exception:
            self.close()
            raise

    def commit(self):
        """the tier-2 commitment of every column, in the order of .hints: one product batch, one PAIR item per column"""
        if self._commitments is None:
            if not self._vecs:
                raise ValueError("the commitment was closed")
            self._commitments = self.ctx.dory_products([ffi.dory_item(ffi.DORY_PAIR, h, self.setup.gamma2_prepared) for h in self.hints])
        return self._commitments

    def close(self):
        for v in self._vecs:
            v.free()
        self._vecs = []
        self.hints = []
