//! Dory's multi-pairings on the device: thin safe wrappers over `jolt_dory_multi_pair`, `jolt_dory_g2_prepare` and
//! `jolt_dory_multi_pair_g2_setup`.
//!
//! WRITTEN BLIND, like the rest of this crate: no Rust toolchain has seen this file.  dory's `PairingCurve` for BN254 is implemented
//! inside the external `dory-pcs` crate (its arkworks backend), so these wrappers bind to NO trait: a caller reaches them by replacing
//! the call sites -- `multi_pair_g2_setup(row_commitments, g2_bases)` of the tier-2 commitment (`crates/jolt-dory/src/scheme.rs:548`)
//! and the `multi_pair` calls of the reduce-and-fold rounds of `dory::prove` -- or by a backend of its own in front of dory.
//!
//! The value is ark_bn254's pairing under the final exponent stated in `include/jolt_hip.h`, a convention no reference vector pins
//! (docs/parity.md); GT bytes must not be mixed with arkworks' until one does.  The library checks the curve equations only: there is
//! no subgroup check, as there is none in arkworks' pairing.  Values of the arkworks types are always canonical and on their curves,
//! so a refusal is a bug and surfaces as the `HipError` of the call.
use std::sync::Arc;

use dory::backends::arkworks::{ArkG1, ArkG2, ArkGT};

use crate::context::HipContext;
use crate::ffi;
use crate::status::{check, HipError};

// `ArkG1`, `ArkG2`, `ArkGT` are `#[repr(transparent)]` over `ark_bn254::{G1Projective, G2Projective, Fq12}` = `jolt_g1_t`, `jolt_g2_t`, `jolt_gt_t`.
const _: () = assert!(core::mem::size_of::<ArkG1>() == core::mem::size_of::<ffi::jolt_g1_t>());
const _: () = assert!(core::mem::size_of::<ArkG2>() == core::mem::size_of::<ffi::jolt_g2_t>());
const _: () = assert!(core::mem::size_of::<ArkGT>() == core::mem::size_of::<ffi::jolt_gt_t>());

/// `prod_i e(g1s[i], g2s[i])`: `PairingGroup::multi_pairing` (`crates/jolt-crypto/src/ec/bn254/mod.rs:274-284`), dory's `multi_pair`.
pub fn multi_pair(ctx: &HipContext, g1s: &[ArkG1], g2s: &[ArkG2]) -> Result<ArkGT, HipError> {
    assert_eq!(g1s.len(), g2s.len(), "lengths must match");
    let mut out = ffi::jolt_gt_t::default();
    let _device = ctx.exclusive();
    // SAFETY: layouts as above; both slices hold `g1s.len()` points, `out` is one jolt_gt_t.
    check(unsafe { ffi::jolt_dory_multi_pair(ctx.raw, g1s.as_ptr().cast(), g2s.as_ptr().cast(), g1s.len(), &mut out) }, ctx.raw)?;
    // SAFETY: `ArkGT` is layout-compatible with `jolt_gt_t` (asserted above).
    Ok(unsafe { core::mem::transmute_copy::<ffi::jolt_gt_t, ArkGT>(&out) })
}

/// The line tables of the setup's `g2_vec` bases, resident on the device: built once per setup.
pub struct HipG2Prepared {
    pub(crate) ctx: Arc<HipContext>,
    pub(crate) raw: *mut ffi::jolt_g2_prepared,
    pub(crate) len: usize,
}

impl HipG2Prepared {
    pub fn new(ctx: &Arc<HipContext>, g2s: &[ArkG2]) -> Result<Self, HipError> {
        let mut raw = core::ptr::null_mut();
        let _device = ctx.exclusive();
        // SAFETY: layouts as above; `g2s` holds `g2s.len()` points.
        check(unsafe { ffi::jolt_dory_g2_prepare(ctx.raw, g2s.as_ptr().cast(), g2s.len(), &mut raw) }, ctx.raw)?;
        Ok(Self { ctx: Arc::clone(ctx), raw, len: g2s.len() })
    }

    pub fn len(&self) -> usize {
        self.len
    }

    pub fn is_empty(&self) -> bool {
        self.len == 0
    }
}

impl Drop for HipG2Prepared {
    fn drop(&mut self) {
        let _device = self.ctx.exclusive();
        // SAFETY: `raw` came from jolt_dory_g2_prepare on this context and is freed once.
        unsafe { ffi::jolt_g2_prepared_free(self.ctx.raw, self.raw) };
    }
}

/// `prod_{i < g1s.len()} e(g1s[i], prepared point i)`: dory's `multi_pair_g2_setup` over `srs_prefix` (`crates/jolt-dory/src/scheme.rs:543-552`).
pub fn multi_pair_g2_setup(g1s: &[ArkG1], prepared: &HipG2Prepared) -> Result<ArkGT, HipError> {
    assert!(g1s.len() <= prepared.len, "more pairs than prepared bases");
    let ctx = &prepared.ctx;
    let mut out = ffi::jolt_gt_t::default();
    let _device = ctx.exclusive();
    // SAFETY: layouts as above; `g1s` holds `g1s.len()` points, `out` is one jolt_gt_t.
    check(unsafe { ffi::jolt_dory_multi_pair_g2_setup(ctx.raw, g1s.as_ptr().cast(), prepared.raw, g1s.len(), &mut out) }, ctx.raw)?;
    // SAFETY: `ArkGT` is layout-compatible with `jolt_gt_t` (asserted above).
    Ok(unsafe { core::mem::transmute_copy::<ffi::jolt_gt_t, ArkGT>(&out) })
}
