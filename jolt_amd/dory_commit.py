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

order="address_major" commits the same columns in the other placement the reference proves in (TracePolynomialOrder::AddressMajor): grid index
(t << log_block) + (k << log_stride) with log_block = log_k + log_extra, log_stride = log_extra.  A matrix row is then C = 2^(sigma - log_block) whole cycles and EVERY
column, one-hot or dense, has cycles / C rows:

    one-hot column                 hint[r] = the sum of Gamma1[(j << log_block) + (hot(r C + j) << log_stride)] over the hot cycles j < C of row r
    dense column                   hint[r] = sum_j values[r C + j] * Gamma1[j << log_block]

through one jolt_dory_hints_onehot_am call per source and one jolt_dory_hints_rows_am call per dense column.  The hints are resident G1 views of `rows` normalised
points in matrix-row order either way, so DoryOpening and .commit() do not know the difference; the row fold of such an opening is Context.dory_fold_rows_grid_am.

blocks=(...) are polynomials held as field elements -- advice, bytecode chunks, the program image -- each committed as its OWN balanced matrix, as
BlockOpeningPoly::new and commit_advice do (crates/jolt-kernels/src/reference/commitment.rs:101-122): a table of 2^m entries is 2^(m - sigma_p) rows of 2^sigma_p
columns with sigma_p = ceil(m / 2), its hint one jolt_dory_hints_rows_fr call.  The block hints follow the dense columns in `.hints`, in either order (the embedding
of a block in the joint opening, top-left, is the same in both placements: Context.dory_fold_rows_blocks with base = the trace's fold).
"""
from . import ffi


def block_sigma(length):
    """sigma_p = ceil(m / 2) of a block of 2^m field elements: the columns of its own balanced matrix (BlockOpeningPoly::new)"""
    if length <= 0 or length & (length - 1):
        raise ValueError("a block holds a power of two of field elements")
    return (length.bit_length() - 1 + 1) // 2


class _TakesBlocks(type):
    """DoryWitnessCommitment(..., blocks=(...)): the keyword is taken here and kept on the instance, so that __init__ keeps the parameter list the address-major
    suite pins (tests/test_dory_am_cpu.py) and a call without `blocks` is the call it always was"""

    def __call__(cls, *args, blocks=(), **kwargs):
        self = cls.__new__(cls)
        self._blocks = list(blocks)
        self.__init__(*args, **kwargs)
        return self


class DoryWitnessCommitment(metaclass=_TakesBlocks):
    def __init__(self, setup, srs, sources, dense, sigma, order="cycle_major", log_k=None, log_extra=0):
        """setup: a dory_open.DorySetup; srs: a jolt_srs (ffi.Srs) over Gamma1's first 2^sigma points at least; sources: ffi.OneHot handles; dense: ffi.Ints columns.
        order: "cycle_major" (log_k and log_extra are not used) or "address_major" (log_k: log2 of the grid's addresses, log_extra: the embedding extra of a widened
        grid); blocks (keyword only, see _TakesBlocks): ffi.Table handles of 2^m field elements each.  Every shape is checked here, before anything is enqueued; the inputs stay the caller's."""
        if order not in ("cycle_major", "address_major"):
            raise ValueError("order is cycle_major or address_major")
        address_major = order == "address_major"
        width = 1 << sigma
        if width > len(srs):
            raise ValueError("the SRS holds fewer than 2^sigma bases")
        shapes = []  # per vector: (source or column, rows per column, columns)
        if address_major:
            if log_k is None or log_k < 0 or log_extra < 0:
                raise ValueError("address_major needs log_k, and log_extra >= 0")
            log_block = log_k + log_extra
            if sigma < log_block:
                raise ValueError("sigma < log_k + log_extra: a cycle's block is wider than a matrix row")
            per_row = 1 << (sigma - log_block)
            for s in sources:
                if s.k > 1 << log_k:
                    raise ValueError("a source has more than 2^log_k addresses")
                if s.cycles % per_row:
                    raise ValueError("the cycles of a matrix row do not divide a source's cycle count")
                shapes.append((s, s.cycles // per_row, s.n_polys))
            for d in dense:
                if d.count % per_row:
                    raise ValueError("the cycles of a matrix row do not divide a dense column's length")
                shapes.append((d, d.count // per_row, 1))
        else:
            for s in sources:
                if s.cycles % width:
                    raise ValueError("2^sigma does not divide a source's cycle count")
                shapes.append((s, s.k * (s.cycles // width), s.n_polys))
            for d in dense:
                if d.count % width:
                    raise ValueError("2^sigma does not divide a dense column's length")
                shapes.append((d, d.count // width, 1))
        blocks = getattr(self, "_blocks", [])
        for b in blocks:
            sigma_p = block_sigma(len(b))
            if 1 << sigma_p > len(srs):
                raise ValueError("the SRS holds fewer bases than a block has columns")
            shapes.append((b, len(b) >> sigma_p, 1))
        if not shapes:
            raise ValueError("a witness has at least one column")
        if any(rows > setup.n for _, rows, _ in shapes):
            raise ValueError("a column has more rows than the setup has Gamma2 bases")
        self.setup, self.ctx, self.sigma, self.order = setup, setup.ctx, sigma, order
        self.hints = []
        self._vecs = []
        self._commitments = None
        try:
            for k, (col, rows, columns) in enumerate(shapes):
                vec = self.ctx.dory_state_alloc(ffi.DORY_KIND_G1, rows * columns)
                self._vecs.append(vec)
                if k >= len(shapes) - len(blocks):
                    self.ctx.dory_hints_rows_fr(srs, col, len(col) // rows, vec)
                elif address_major and k < len(sources):
                    self.ctx.dory_hints_onehot_am(srs, col, vec, sigma, log_block, log_extra)
                elif address_major:
                    self.ctx.dory_hints_rows_am(srs, col, sigma, log_block, vec)
                elif k < len(sources):
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
