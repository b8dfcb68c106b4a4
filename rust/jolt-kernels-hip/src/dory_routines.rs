//! dory's `DoryRoutines` seam on the device, for both groups: the drop-in for `JoltG1Routines` / `JoltG2Routines`
//! (`crates/jolt-dory/src/routines.rs:58-147`), which `dory::prove` calls in every reduce-and-fold round.
//!
//! WRITTEN BLIND, like the rest of this crate: no Rust toolchain has seen this file, and the `DoryRoutines` trait itself lives in the
//! external `dory-pcs` crate, which is not available to read either.  The five function names, their parameter lists and their
//! semantics are those of the reference's own two impls (`routines.rs:60-97`, `:101-147`); `tools/rust_seam_audit.py` holds the names
//! and arities of this file against them.  Calls are checked against `ffi.rs` by `tests/test_abi_cpu.py`.
//!
//! | `DoryRoutines<G>` | entry point |
//! |---|---|
//! | `msm(bases, scalars)` | `jolt_dory_g{1,2}_msm` |
//! | `fixed_base_vector_scalar_mul(base, scalars)` | `jolt_dory_g{1,2}_fixed_base_mul` |
//! | `fixed_scalar_mul_bases_then_add(bases, vs, scalar)` | `jolt_dory_g{1,2}_scale_bases_add` |
//! | `fixed_scalar_mul_vs_then_add(vs, addends, scalar)` | `jolt_dory_g{1,2}_scale_vs_add` |
//! | `fold_field_vectors(left, right, scalar)` | `jolt_dory_fold_field_vectors` |
//!
//! The trait's functions have no `self`, so they work over ONE process-wide context, installed once with [`install`] and held under
//! its exclusive lock for the length of each call (`dory::prove` may be reached from several threads).  Pairings, GT and the control
//! flow of `dory::prove` stay with dory.
//!
//! The library refuses points that are not on their curve and scalars that are not canonical (`JOLT_ERR_INVALID_ARG`); values of the
//! arkworks types always are, so a refusal here is a bug and panics, as the reference's own `assert_eq!`s do.  For G2 the library
//! checks the twist equation only -- there is no subgroup check, as there is none in the reference's routines.
use std::sync::{Arc, OnceLock};

use dory::backends::arkworks::{ArkFr, ArkG1, ArkG2};
use dory::primitives::arithmetic::{DoryRoutines, Group};

use crate::context::HipContext;
use crate::ffi;
use crate::status::check;

/// The process-wide context of the routines.
struct RoutinesContext(Arc<HipContext>);

// SAFETY: every use of the inner context through this wrapper happens under `HipContext::exclusive` (see `with_device`).
unsafe impl Send for RoutinesContext {}
unsafe impl Sync for RoutinesContext {}

static CONTEXT: OnceLock<RoutinesContext> = OnceLock::new();

/// Installs the context the routines run on.  The first call wins; returns whether this call installed it.
pub fn install(ctx: &Arc<HipContext>) -> bool {
    CONTEXT.set(RoutinesContext(Arc::clone(ctx))).is_ok()
}

/// Runs one entry point under the context's device lock and turns a refusal into a panic (see the module comment).
fn with_device(what: &str, call: impl FnOnce(*mut ffi::jolt_ctx) -> i32) {
    let ctx = &CONTEXT.get().expect("jolt_kernels_hip::dory_routines::install has not been called").0;
    let _device = ctx.exclusive(); // one device call at a time per context
    if let Err(e) = check(call(ctx.raw), ctx.raw) {
        panic!("{what}: {e}");
    }
}

// Layouts the casts below rest on (the same facts `crates/jolt-dory/src/routines.rs:20-56` rests its transmutes on): `ArkFr`, `ArkG1`, `ArkG2` are
// `#[repr(transparent)]` over `ark_bn254::{Fr, G1Projective, G2Projective}` = `jolt_fr_t` (4 x u64 Montgomery limbs), `jolt_g1_t` (three Montgomery
// Fq) and `jolt_g2_t` (three Fq2 = six Montgomery Fq in the order x.c0, x.c1, y.c0, y.c1, z.c0, z.c1).
const _: () = assert!(core::mem::size_of::<ArkFr>() == core::mem::size_of::<ffi::jolt_fr_t>());
const _: () = assert!(core::mem::size_of::<ArkG1>() == core::mem::size_of::<ffi::jolt_g1_t>());
const _: () = assert!(core::mem::size_of::<ArkG2>() == core::mem::size_of::<ffi::jolt_g2_t>());

fn fold_field_vectors_on_device(left: &mut [ArkFr], right: &[ArkFr], scalar: &ArkFr) {
    assert_eq!(left.len(), right.len(), "lengths must match");
    // SAFETY: layouts as above; `left` and `right` hold `left.len()` elements each, `scalar` one.
    with_device("fold_field_vectors", |raw| unsafe {
        ffi::jolt_dory_fold_field_vectors(raw, left.as_mut_ptr().cast(), right.as_ptr().cast(), left.len(), (scalar as *const ArkFr).cast())
    });
}

pub struct HipG1Routines;

impl DoryRoutines<ArkG1> for HipG1Routines {
    fn msm(bases: &[ArkG1], scalars: &[ArkFr]) -> ArkG1 {
        assert_eq!(bases.len(), scalars.len(), "lengths must match");
        let mut out = ArkG1::identity();
        // SAFETY: layouts as above; `out` is one jolt_g1_t.
        with_device("G1 msm", |raw| unsafe { ffi::jolt_dory_g1_msm(raw, bases.as_ptr().cast(), scalars.as_ptr().cast(), bases.len(), (&mut out as *mut ArkG1).cast()) });
        out
    }

    fn fixed_base_vector_scalar_mul(base: &ArkG1, scalars: &[ArkFr]) -> Vec<ArkG1> {
        if scalars.is_empty() {
            return vec![];
        }
        let mut out = vec![ArkG1::identity(); scalars.len()];
        // SAFETY: layouts as above; `out` holds `scalars.len()` points.
        with_device("G1 fixed_base_vector_scalar_mul", |raw| unsafe {
            ffi::jolt_dory_g1_fixed_base_mul(raw, (base as *const ArkG1).cast(), scalars.as_ptr().cast(), scalars.len(), out.as_mut_ptr().cast())
        });
        out
    }

    fn fixed_scalar_mul_bases_then_add(bases: &[ArkG1], vs: &mut [ArkG1], scalar: &ArkFr) {
        assert_eq!(bases.len(), vs.len(), "lengths must match");
        // v[i] = v[i] + scalar * bases[i]
        // SAFETY: layouts as above; both slices hold `vs.len()` points.
        with_device("G1 fixed_scalar_mul_bases_then_add", |raw| unsafe {
            ffi::jolt_dory_g1_scale_bases_add(raw, bases.as_ptr().cast(), vs.as_mut_ptr().cast(), vs.len(), (scalar as *const ArkFr).cast())
        });
    }

    fn fixed_scalar_mul_vs_then_add(vs: &mut [ArkG1], addends: &[ArkG1], scalar: &ArkFr) {
        assert_eq!(vs.len(), addends.len(), "lengths must match");
        // v[i] = scalar * v[i] + addends[i]
        // SAFETY: layouts as above; both slices hold `vs.len()` points.
        with_device("G1 fixed_scalar_mul_vs_then_add", |raw| unsafe {
            ffi::jolt_dory_g1_scale_vs_add(raw, vs.as_mut_ptr().cast(), addends.as_ptr().cast(), vs.len(), (scalar as *const ArkFr).cast())
        });
    }

    fn fold_field_vectors(left: &mut [ArkFr], right: &[ArkFr], scalar: &ArkFr) {
        fold_field_vectors_on_device(left, right, scalar);
    }
}

pub struct HipG2Routines;

impl DoryRoutines<ArkG2> for HipG2Routines {
    fn msm(bases: &[ArkG2], scalars: &[ArkFr]) -> ArkG2 {
        assert_eq!(bases.len(), scalars.len(), "lengths must match");
        let mut out = ArkG2::identity();
        // SAFETY: layouts as above; `out` is one jolt_g2_t.
        with_device("G2 msm", |raw| unsafe { ffi::jolt_dory_g2_msm(raw, bases.as_ptr().cast(), scalars.as_ptr().cast(), bases.len(), (&mut out as *mut ArkG2).cast()) });
        out
    }

    fn fixed_base_vector_scalar_mul(base: &ArkG2, scalars: &[ArkFr]) -> Vec<ArkG2> {
        if scalars.is_empty() {
            return vec![];
        }
        let mut out = vec![ArkG2::identity(); scalars.len()];
        // SAFETY: layouts as above; `out` holds `scalars.len()` points.
        with_device("G2 fixed_base_vector_scalar_mul", |raw| unsafe {
            ffi::jolt_dory_g2_fixed_base_mul(raw, (base as *const ArkG2).cast(), scalars.as_ptr().cast(), scalars.len(), out.as_mut_ptr().cast())
        });
        out
    }

    fn fixed_scalar_mul_bases_then_add(bases: &[ArkG2], vs: &mut [ArkG2], scalar: &ArkFr) {
        assert_eq!(bases.len(), vs.len(), "lengths must match");
        // v[i] = v[i] + scalar * bases[i]
        // SAFETY: layouts as above; both slices hold `vs.len()` points.
        with_device("G2 fixed_scalar_mul_bases_then_add", |raw| unsafe {
            ffi::jolt_dory_g2_scale_bases_add(raw, bases.as_ptr().cast(), vs.as_mut_ptr().cast(), vs.len(), (scalar as *const ArkFr).cast())
        });
    }

    fn fixed_scalar_mul_vs_then_add(vs: &mut [ArkG2], addends: &[ArkG2], scalar: &ArkFr) {
        assert_eq!(vs.len(), addends.len(), "lengths must match");
        // v[i] = scalar * v[i] + addends[i]
        // SAFETY: layouts as above; both slices hold `vs.len()` points.
        with_device("G2 fixed_scalar_mul_vs_then_add", |raw| unsafe {
            ffi::jolt_dory_g2_scale_vs_add(raw, vs.as_mut_ptr().cast(), addends.as_ptr().cast(), vs.len(), (scalar as *const ArkFr).cast())
        });
    }

    fn fold_field_vectors(left: &mut [ArkFr], right: &[ArkFr], scalar: &ArkFr) {
        fold_field_vectors_on_device(left, right, scalar);
    }
}
