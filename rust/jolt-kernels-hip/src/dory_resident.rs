//! Dory's reduce-and-fold rounds on vectors that stay on the device: thin safe wrappers over `jolt_dory_vec_*`, `jolt_dory_g2_prepare_vec`
//! and `jolt_dory_products`; and the witness commitment that fills such vectors with opening hints (`jolt_dory_hints_onehot`, `jolt_dory_hints_rows`),
//! in either trace placement (`jolt_dory_hints_onehot_am`, `jolt_dory_hints_rows_am`, `jolt_dory_fold_rows_grid_am` for `TraceOrder::AddressMajor`).
//!
//! WRITTEN BLIND, like the rest of this crate: no Rust toolchain has seen this file.  dory's `DoryRoutines` seam works on host slices and its
//! `multi_pair` on host slices too, so nothing here binds to a trait: a caller reaches these wrappers from a prover loop of its own in front of
//! dory, handing every challenge in.  The library is agnostic about which half a message calls left and which of a challenge
//! and its inverse folds which vector; `jolt_amd/dory_reduce.py` is the statement of the Dory paper's choice (docs/parity.md).
//!
//! Elements are checked once, in [`HipDoryVec::upload`]; values of the arkworks types are always canonical and on their curves, so a refusal
//! there is a bug and surfaces as the `HipError` of the call.  Views are `(vector, first, n)`; the library refuses a view outside its vector.
use std::sync::Arc;

use dory::backends::arkworks::{ArkFr, ArkG1, ArkG2, ArkGT};

use crate::context::{HipContext, HipTable};
use crate::ffi;
use crate::msm::HipSrs;
use crate::ops::{HipHotIndices, HipInts};
use crate::pairing::HipG2Prepared;
use crate::status::{check, HipError};

#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum VecKind {
    G1,
    G2,
    Fr,
}

impl VecKind {
    fn raw(self) -> i32 {
        match self {
            VecKind::G1 => ffi::JOLT_DORY_KIND_G1,
            VecKind::G2 => ffi::JOLT_DORY_KIND_G2,
            VecKind::Fr => ffi::JOLT_DORY_KIND_FR,
        }
    }
}

/// The layout of the committed trace polynomials: the shape of `TracePolynomialOrder` (crates/jolt-claims/src/protocols/jolt/geometry/dimensions.rs:20-59).
/// `AddressMajor` carries the placement of `TracePlacement`: `log_block = log2 cycle_stride()`, `log_stride = log2 one_hot_stride()`; the coefficient of
/// (cycle t, address k) sits at grid index `(t << log_block) + (k << log_stride)`.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum TraceOrder {
    CycleMajor,
    AddressMajor { log_block: u32, log_stride: u32 },
}

/// A G1, G2 or Fr array resident on the device.
pub struct HipDoryVec {
    pub(crate) ctx: Arc<HipContext>,
    pub(crate) raw: *mut ffi::jolt_dory_vec,
    pub(crate) kind: VecKind,
}

impl HipDoryVec {
    fn upload(ctx: &Arc<HipContext>, kind: VecKind, host: *const core::ffi::c_void, n: usize) -> Result<Self, HipError> {
        let mut raw = core::ptr::null_mut();
        let _device = ctx.exclusive();
        // SAFETY: `host` points at `n` elements of the kind's ABI type (the callers below pass slices of the layout-compatible arkworks types).
        check(unsafe { ffi::jolt_dory_vec_upload(ctx.raw, kind.raw(), host, n, &mut raw) }, ctx.raw)?;
        Ok(Self { ctx: Arc::clone(ctx), raw, kind })
    }

    pub fn from_g1(ctx: &Arc<HipContext>, points: &[ArkG1]) -> Result<Self, HipError> {
        Self::upload(ctx, VecKind::G1, points.as_ptr().cast(), points.len())
    }

    pub fn from_g2(ctx: &Arc<HipContext>, points: &[ArkG2]) -> Result<Self, HipError> {
        Self::upload(ctx, VecKind::G2, points.as_ptr().cast(), points.len())
    }

    pub fn from_fr(ctx: &Arc<HipContext>, scalars: &[ArkFr]) -> Result<Self, HipError> {
        Self::upload(ctx, VecKind::Fr, scalars.as_ptr().cast(), scalars.len())
    }

    /// `n` neutral elements -- the identity (1, 1, 0), or zero for `Fr` -- made on the device: `jolt_dory_state_alloc`.  What [`HipDoryVec::hints_onehot`] and
    /// [`HipDoryVec::hints_rows`] write into.
    pub fn neutral(ctx: &Arc<HipContext>, kind: VecKind, n: usize) -> Result<Self, HipError> {
        let mut raw = core::ptr::null_mut();
        let _device = ctx.exclusive();
        // SAFETY: `ctx.raw` is a live context; the library allocates and fills the vector.
        check(unsafe { ffi::jolt_dory_state_alloc(ctx.raw, kind.raw(), n, &mut raw) }, ctx.raw)?;
        Ok(Self { ctx: Arc::clone(ctx), raw, kind })
    }

    pub fn kind(&self) -> VecKind {
        self.kind
    }

    /// The opening hints of columns `[first_column, first_column + n_columns)` of `source` into `self[out_first ..]`, element
    /// `p * k * chunks + row * chunks + chunk` (the order of `finish_one_hot_column_major_chunks`), every point normalised: `jolt_dory_hints_onehot`, enqueued.
    /// `chunk_width` is `2^sigma`; the launch sets hold the library's default number of keys.
    pub fn hints_onehot(&mut self, out_first: usize, srs: &HipSrs, source: &HipHotIndices, first_column: usize, n_columns: usize, chunk_width: usize) -> Result<(), HipError> {
        let _device = self.ctx.exclusive();
        // SAFETY: live handles of one context; the library refuses a vector that is not G1 and a view that does not hold the hints.
        check(unsafe { ffi::jolt_dory_hints_onehot(self.ctx.raw, srs.raw, source.raw, first_column, n_columns, chunk_width, self.raw, out_first, 0) }, self.ctx.raw)
    }

    /// The row commitments of a dense column of machine integers into `self[out_first ..]`, normalised: `jolt_dory_hints_rows` (`row_width` is `2^sigma`).
    pub fn hints_rows(&mut self, out_first: usize, srs: &HipSrs, values: &HipInts, row_width: usize) -> Result<(), HipError> {
        let _device = self.ctx.exclusive();
        // SAFETY: as hints_onehot.
        check(unsafe { ffi::jolt_dory_hints_rows(self.ctx.raw, srs.raw, values.raw, row_width, self.raw, out_first) }, self.ctx.raw)
    }

    /// `StreamingCommitment::feed(&[Fr])` per row (`crates/jolt-dory/src/streaming.rs:53-70`) for a polynomial held as field elements on the device -- advice, a bytecode
    /// chunk, the program image, or a whole dense polynomial: the commitments of the `row_width` windows of `table[first .. first + count]` into
    /// `self[out_first ..]`, normalised: `jolt_dory_hints_rows_fr`.  The same rows in both trace orders (a block is its own matrix).
    pub fn hints_rows_fr(&mut self, out_first: usize, srs: &HipSrs, table: &HipTable, first: usize, count: usize, row_width: usize) -> Result<(), HipError> {
        let _device = self.ctx.exclusive();
        // SAFETY: as hints_onehot; the library refuses a stretch that leaves the table.
        check(unsafe { ffi::jolt_dory_hints_rows_fr(self.ctx.raw, srs.raw, table.raw, first, count, row_width, self.raw, out_first) }, self.ctx.raw)
    }

    /// [`HipDoryVec::hints_onehot`] in the given trace order.  Address-major: element `p * rows + r`, `rows = cycles >> (sigma - log_block)`, row `r` the sum over
    /// the cycles `[r C, (r + 1) C)`: `jolt_dory_hints_onehot_am`, enqueued.
    pub fn hints_onehot_in(&mut self, order: TraceOrder, out_first: usize, srs: &HipSrs, source: &HipHotIndices, first_column: usize, n_columns: usize, sigma: u32) -> Result<(), HipError> {
        match order {
            TraceOrder::CycleMajor => self.hints_onehot(out_first, srs, source, first_column, n_columns, 1usize << sigma),
            TraceOrder::AddressMajor { log_block, log_stride } => {
                let _device = self.ctx.exclusive();
                // SAFETY: as hints_onehot; the library refuses sigma < log_block and a source with more addresses than the block holds.
                check(unsafe { ffi::jolt_dory_hints_onehot_am(self.ctx.raw, srs.raw, source.raw, first_column, n_columns, sigma, log_block, log_stride, self.raw, out_first) }, self.ctx.raw)
            }
        }
    }

    /// [`HipDoryVec::hints_rows`] in the given trace order.  Address-major: `self[out_first + r] = sum_j values[r C + j] * srs[j << log_block]`: `jolt_dory_hints_rows_am`.
    pub fn hints_rows_in(&mut self, order: TraceOrder, out_first: usize, srs: &HipSrs, values: &HipInts, sigma: u32) -> Result<(), HipError> {
        match order {
            TraceOrder::CycleMajor => self.hints_rows(out_first, srs, values, 1usize << sigma),
            TraceOrder::AddressMajor { log_block, .. } => {
                let _device = self.ctx.exclusive();
                // SAFETY: as hints_onehot.
                check(unsafe { ffi::jolt_dory_hints_rows_am(self.ctx.raw, srs.raw, values.raw, sigma, log_block, self.raw, out_first) }, self.ctx.raw)
            }
        }
    }

    pub fn len(&self) -> usize {
        let mut n = 0usize;
        // SAFETY: `raw` is a live handle.
        unsafe { ffi::jolt_dory_vec_len(self.raw, &mut n) };
        n
    }

    pub fn is_empty(&self) -> bool {
        self.len() == 0
    }

    /// The vector becomes its first `n` elements: after a fold, its first half.
    pub fn truncate(&mut self, n: usize) -> Result<(), HipError> {
        // SAFETY: `raw` is a live handle.
        check(unsafe { ffi::jolt_dory_vec_truncate(self.raw, n) }, self.ctx.raw)
    }

    /// Elements `[first, first + out.len())` of a G1 vector.
    pub fn download_g1(&self, first: usize, out: &mut [ArkG1]) -> Result<(), HipError> {
        assert_eq!(self.kind, VecKind::G1);
        self.download(first, out.len(), out.as_mut_ptr().cast())
    }

    pub fn download_g2(&self, first: usize, out: &mut [ArkG2]) -> Result<(), HipError> {
        assert_eq!(self.kind, VecKind::G2);
        self.download(first, out.len(), out.as_mut_ptr().cast())
    }

    pub fn download_fr(&self, first: usize, out: &mut [ArkFr]) -> Result<(), HipError> {
        assert_eq!(self.kind, VecKind::Fr);
        self.download(first, out.len(), out.as_mut_ptr().cast())
    }

    fn download(&self, first: usize, n: usize, host: *mut core::ffi::c_void) -> Result<(), HipError> {
        let _device = self.ctx.exclusive();
        // SAFETY: `host` has room for `n` elements of this vector's kind (asserted by the typed callers above).
        check(unsafe { ffi::jolt_dory_vec_download(self.ctx.raw, self.raw, first, n, host) }, self.ctx.raw)
    }

    /// The line table of G2 points `[first, first + n)`, built on the device: once per setup for the `g2_vec` bases.
    pub fn prepare_g2(&self, first: usize, n: usize) -> Result<HipG2Prepared, HipError> {
        let mut raw = core::ptr::null_mut();
        let _device = self.ctx.exclusive();
        // SAFETY: `self.raw` is a live handle; the library refuses a vector that is not G2 and a view outside it.
        check(unsafe { ffi::jolt_dory_g2_prepare_vec(self.ctx.raw, self.raw, first, n, &mut raw) }, self.ctx.raw)?;
        Ok(HipG2Prepared { ctx: Arc::clone(&self.ctx), raw, len: n })
    }

    /// `self[vs_first + i] += scalar * bases[bases_first + i]`: `fixed_scalar_mul_bases_then_add` in place, enqueued.
    pub fn scale_bases_add(&mut self, vs_first: usize, bases: &HipDoryVec, bases_first: usize, n: usize, scalar: &ArkFr) -> Result<(), HipError> {
        let _device = self.ctx.exclusive();
        // SAFETY: live handles; `ArkFr` is layout-compatible with `jolt_fr_t` (asserted in dory_routines.rs); the library validates kinds and views.
        check(unsafe { ffi::jolt_dory_vec_scale_bases_add(self.ctx.raw, bases.raw, bases_first, self.raw, vs_first, n, (scalar as *const ArkFr).cast()) }, self.ctx.raw)
    }

    /// `self[vs_first + i] = scalar * self[vs_first + i] + addends[addends_first + i]`: `fixed_scalar_mul_vs_then_add` in place, enqueued.
    pub fn scale_vs_add(&mut self, vs_first: usize, addends: &HipDoryVec, addends_first: usize, n: usize, scalar: &ArkFr) -> Result<(), HipError> {
        let _device = self.ctx.exclusive();
        // SAFETY: as scale_bases_add.
        check(unsafe { ffi::jolt_dory_vec_scale_vs_add(self.ctx.raw, self.raw, vs_first, addends.raw, addends_first, n, (scalar as *const ArkFr).cast()) }, self.ctx.raw)
    }

    /// The fold of one vector onto its first half: `self[i] = scalar * self[i] + self[n + i]` for `i < n` (points), or `self[i] * scalar + self[n + i]` (Fr);
    /// the vector is then truncated to `n`.
    pub fn fold_halves(&mut self, n: usize, scalar: &ArkFr) -> Result<(), HipError> {
        let s = (scalar as *const ArkFr).cast();
        {
            let _device = self.ctx.exclusive();
            // SAFETY: one live handle for both views; the library refuses ranges that overlap or leave the vector.
            let status = unsafe {
                match self.kind {
                    VecKind::Fr => ffi::jolt_dory_vec_fold_field(self.ctx.raw, self.raw, 0, self.raw, n, n, s),
                    _ => ffi::jolt_dory_vec_scale_vs_add(self.ctx.raw, self.raw, 0, self.raw, n, n, s),
                }
            };
            check(status, self.ctx.raw)?;
        }
        self.truncate(n)
    }
}

impl Drop for HipDoryVec {
    fn drop(&mut self) {
        let _device = self.ctx.exclusive();
        // SAFETY: `raw` came from jolt_dory_vec_upload on this context and is freed once.
        unsafe { ffi::jolt_dory_vec_free(self.ctx.raw, self.raw) };
    }
}

/// One inner product of a batch, over views `(vector, first)` of `n` elements.
pub enum DoryItem<'a> {
    /// `prod_i e(a[i], b[i])`
    Pair { a: (&'a HipDoryVec, usize), b: (&'a HipDoryVec, usize), n: usize },
    /// `prod_i e(a[i], prepared point first + i)`
    PairPrepared { a: (&'a HipDoryVec, usize), prepared: (&'a HipG2Prepared, usize), n: usize },
    /// `sum_i scalars[i] * points[i]`, G1 or G2 by the kind of `points`
    Msm { points: (&'a HipDoryVec, usize), scalars: (&'a HipDoryVec, usize), n: usize },
}

pub enum DoryProduct {
    Gt(ArkGT),
    G1(ArkG1),
    G2(ArkG2),
}

/// Every item in one launch set, one synchronisation: `jolt_dory_products`.
pub fn products(ctx: &Arc<HipContext>, items: &[DoryItem<'_>]) -> Result<Vec<DoryProduct>, HipError> {
    let raw_items: Vec<ffi::jolt_dory_item> = items
        .iter()
        .map(|it| match *it {
            DoryItem::Pair { a, b, n } => ffi::jolt_dory_item { op: ffi::JOLT_DORY_PAIR, a: a.0.raw, a_first: a.1, b: b.0.raw, b_first: b.1, prepared: core::ptr::null(), prepared_first: 0, n },
            DoryItem::PairPrepared { a, prepared, n } => {
                ffi::jolt_dory_item { op: ffi::JOLT_DORY_PAIR, a: a.0.raw, a_first: a.1, b: core::ptr::null(), b_first: 0, prepared: prepared.0.raw, prepared_first: prepared.1, n }
            }
            DoryItem::Msm { points, scalars, n } => {
                let op = if points.0.kind == VecKind::G1 { ffi::JOLT_DORY_MSM_G1 } else { ffi::JOLT_DORY_MSM_G2 };
                ffi::jolt_dory_item { op, a: points.0.raw, a_first: points.1, b: scalars.0.raw, b_first: scalars.1, prepared: core::ptr::null(), prepared_first: 0, n }
            }
        })
        .collect();
    let mut outs = vec![ffi::jolt_dory_result { w: [0u64; 48] }; items.len()];
    {
        let _device = ctx.exclusive();
        // SAFETY: `raw_items` and `outs` hold `items.len()` entries; every handle is borrowed for the call.
        check(unsafe { ffi::jolt_dory_products(ctx.raw, raw_items.as_ptr(), raw_items.len(), outs.as_mut_ptr()) }, ctx.raw)?;
    }
    Ok(raw_items
        .iter()
        .zip(outs.iter())
        .map(|(it, out)| {
            // SAFETY: the result block holds the item's value in its leading words; `ArkGT` / `ArkG1` / `ArkG2` are layout-compatible with
            // `jolt_gt_t` / `jolt_g1_t` / `jolt_g2_t` (asserted in pairing.rs and dory_routines.rs) and no larger than the block.
            unsafe {
                if it.op == ffi::JOLT_DORY_PAIR {
                    DoryProduct::Gt(core::mem::transmute_copy::<ffi::jolt_dory_result, ArkGT>(out))
                } else if it.op == ffi::JOLT_DORY_MSM_G1 {
                    DoryProduct::G1(core::mem::transmute_copy::<ffi::jolt_dory_result, ArkG1>(out))
                } else {
                    DoryProduct::G2(core::mem::transmute_copy::<ffi::jolt_dory_result, ArkG2>(out))
                }
            }
        })
        .collect())
}

/// `RlcSource::fold_rows(left, sigma)` of a batch's joint polynomial from its per-cycle columns, in the given trace order: `jolt_dory_fold_rows_grid` (`log_k` is the
/// grid's address bits) or `jolt_dory_fold_rows_grid_am` (`log_k` is not used: the placement says it).  `2^sigma` entries.
#[allow(clippy::too_many_arguments)]
pub fn fold_rows_in(ctx: &Arc<HipContext>, order: TraceOrder, sources: &[&HipHotIndices], onehot_scalars: &[ArkFr], dense: &[&HipTable], dense_scalars: &[ArkFr], log_k: u32,
                    sigma: u32, left: &HipTable) -> Result<HipTable, HipError> {
    let hs: Vec<*const ffi::jolt_onehot> = sources.iter().map(|s| s.raw as *const ffi::jolt_onehot).collect();
    let ds: Vec<*mut ffi::jolt_table> = dense.iter().map(|t| t.raw).collect();
    let mut raw = core::ptr::null_mut();
    let _device = ctx.exclusive();
    // SAFETY: live handles of one context, borrowed for the call; `ArkFr` is layout-compatible with `jolt_fr_t`; the library checks every length.
    let status = unsafe {
        match order {
            TraceOrder::CycleMajor => ffi::jolt_dory_fold_rows_grid(ctx.raw, hs.as_ptr(), hs.len(), onehot_scalars.as_ptr().cast(), ds.as_ptr(), ds.len(), dense_scalars.as_ptr().cast(), log_k, sigma, left.raw, &mut raw),
            TraceOrder::AddressMajor { log_block, log_stride } => ffi::jolt_dory_fold_rows_grid_am(ctx.raw, hs.as_ptr(), hs.len(), onehot_scalars.as_ptr().cast(), ds.as_ptr(), ds.len(), dense_scalars.as_ptr().cast(), log_block, log_stride, sigma, left.raw, &mut raw),
        }
    };
    check(status, ctx.raw)?;
    Ok(HipTable { ctx: Arc::clone(ctx), raw })
}

/// `BlockOpeningPoly::fold_rows` (`crates/jolt-kernels/src/optimized/opening.rs:594-611`): `base + sum_d scalars[d] * (left^T M_d)` with table `d` a
/// `2^(m_d - sigma_d) x 2^sigma_d` matrix embedded top-left in the grid of `2^sigma` columns: `jolt_dory_fold_rows_blocks`.  `base` is the trace's
/// [`fold_rows_in`] (either order) for a joint opening, `None` for the dense `vector_matrix_product` of one table with `sigma_d = sigma`.
pub fn fold_rows_blocks(ctx: &Arc<HipContext>, tables: &[&HipTable], sigma_tables: &[u32], scalars: &[ArkFr], sigma: u32, left: &HipTable, base: Option<&HipTable>) -> Result<HipTable, HipError> {
    if sigma_tables.len() != tables.len() || scalars.len() != tables.len() {
        return Err(HipError::size_mismatch("fold_rows_blocks: one sigma and one scalar per table"));
    }
    let ts: Vec<*mut ffi::jolt_table> = tables.iter().map(|t| t.raw).collect();
    let mut raw = core::ptr::null_mut();
    let _device = ctx.exclusive();
    // SAFETY: live handles of one context, borrowed for the call; `ArkFr` is layout-compatible with `jolt_fr_t`; the library checks every length.
    let status = unsafe {
        ffi::jolt_dory_fold_rows_blocks(ctx.raw, ts.as_ptr(), sigma_tables.as_ptr(), ts.len(), scalars.as_ptr().cast(), sigma, left.raw, base.map_or(core::ptr::null(), |b| b.raw as *const ffi::jolt_table), &mut raw)
    };
    check(status, ctx.raw)?;
    Ok(HipTable { ctx: Arc::clone(ctx), raw })
}
