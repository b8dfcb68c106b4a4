//! A Dory evaluation proof as one call of the library, under the caller's transcript: [`HipDorySetup`] over `jolt_dory_setup_*`, [`HipDorySetup::open_with`] over
//! `jolt_host_dory_open_with_transcript`, and [`round_update`] over `jolt_dory_round_update` for a prover loop that keeps the rounds to itself.
//!
//! WRITTEN BLIND, like the rest of this crate: no Rust toolchain has seen this file.  The library runs the prover's side of Eval-VMV-RE in transparent mode (the
//! protocol `jolt_amd/dory_open.py` and `dory_reduce.py` state) and calls back after each message; the hook below absorbs the message's elements the way the
//! reference's `JoltToDoryTranscript` absorbs a group element (`crates/jolt-dory/src/transcript.rs:46-53`: `LabelWithCount(b"dory_group", len)`, then dory's
//! compressed bytes) and draws `Transcript::challenge_scalar`.  The ORDER of the appends is the library's phase order; dory-pcs's own order is pinned by nothing in
//! the reference checkout (docs/parity.md), so a caller with dory-pcs in hand that needs another order passes a hook of its own to the raw entry.
//!
//! The labels are the adapter's four; this module appends group elements only, the other three are here for a caller that extends the hook.
use std::sync::Arc;

use dory::backends::arkworks::{ArkFr, ArkG1, ArkG2, ArkGT};
use dory::primitives::arithmetic::Group as DoryGroup;
use dory::primitives::DorySerialize;
use jolt_field::Fr;
use jolt_transcript::domain::LabelWithCount;
use jolt_transcript::Transcript;

use crate::context::{HipContext, HipTable};
use crate::dory_resident::HipDoryVec;
use crate::ffi;
use crate::status::{check, HipError};

pub const DORY_BYTES_LABEL: &[u8] = b"dory_bytes";
pub const DORY_FIELD_LABEL: &[u8] = b"dory_field";
pub const DORY_GROUP_LABEL: &[u8] = b"dory_group";
pub const DORY_SERDE_LABEL: &[u8] = b"dory_serde";

const _: () = assert!(core::mem::size_of::<ArkGT>() == core::mem::size_of::<ffi::jolt_gt_t>());
const _: () = assert!(core::mem::size_of::<Fr>() == core::mem::size_of::<ffi::jolt_fr_t>());

/// `bytes` under one of the four labels: the count word, then the bytes.
pub fn append_labelled<T: Transcript<Challenge = Fr>>(transcript: &mut T, label: &'static [u8], bytes: &[u8]) {
    transcript.append(&LabelWithCount(label, bytes.len() as u64));
    transcript.append_bytes(bytes);
}

/// One group element (G1, G2 or GT) in dory's compressed form under `dory_group`; `false` when dory refuses to serialise it.
pub fn append_group<T: Transcript<Challenge = Fr>, G: DoryGroup>(transcript: &mut T, element: &G) -> bool {
    let mut buffer = Vec::new();
    if element.serialize_compressed(&mut buffer).is_err() {
        return false;
    }
    append_labelled(transcript, DORY_GROUP_LABEL, &buffer);
    true
}

/// A resident G1 view `(vector, first, rows)`.
pub type HintView<'a> = (&'a HipDoryVec, usize, usize);

/// Gamma1, Gamma2 (resident, checked once), Gamma2's prepared line table, H1 and H2 on the device: `jolt_dory_setup`.
pub struct HipDorySetup {
    ctx: Arc<HipContext>,
    raw: *mut ffi::jolt_dory_setup,
}

// SAFETY: see HipContext: every device call below is made under the context's exclusive lock.
unsafe impl Send for HipDorySetup {}

/// The prover's messages in protocol order and the challenges drawn between them (`jolt_host_dory_proof_counts`).
pub struct HipDoryProof {
    pub sigma: u32,
    /// C, D2; per round D1L, D1R, D2L, D2R, C+, C-
    pub gts: Vec<ArkGT>,
    /// E1; per round E1beta, E1+, E1-; w1
    pub g1s: Vec<ArkG1>,
    /// per round E2beta, E2+, E2-; w2
    pub g2s: Vec<ArkG2>,
    /// (beta_k, alpha_k) per round, then gamma
    pub challenges: Vec<Fr>,
}

struct Hook<'a, T: Transcript<Challenge = Fr>> {
    transcript: &'a mut T,
}

/// `jolt_dory_transcript_fn`: absorb the message of this phase (gts, then g1s, then g2s) and draw the challenge that follows it.
unsafe extern "C" fn dory_hook<T: Transcript<Challenge = Fr>>(
    user: *mut core::ffi::c_void,
    phase: i32,
    _round: usize,
    gts: *const ffi::jolt_gt_t,
    n_gt: usize,
    g1s: *const ffi::jolt_g1_t,
    n_g1: usize,
    g2s: *const ffi::jolt_g2_t,
    n_g2: usize,
    challenge_out: *mut ffi::jolt_fr_t,
) -> i32 {
    // The transcript is the caller's code: a panic must not unwind through the C frames of libjolt_hip.so.  It comes back as a status, which aborts the opening.
    let outcome = std::panic::catch_unwind(std::panic::AssertUnwindSafe(|| {
        // SAFETY: `user` is the `Hook` `open_with` passes for the duration of the call; the arrays hold the stated counts of elements with the layouts of
        // `ArkGT` / `ArkG1` / `ArkG2` (asserted above, in pairing.rs and in dory_routines.rs).
        let hook = unsafe { &mut *user.cast::<Hook<'_, T>>() };
        let mut ok = true;
        for i in 0..n_gt {
            // SAFETY: `i < n_gt` elements at `gts`.
            ok &= append_group(hook.transcript, unsafe { &*gts.add(i).cast::<ArkGT>() });
        }
        for i in 0..n_g1 {
            // SAFETY: `i < n_g1` elements at `g1s`.
            ok &= append_group(hook.transcript, unsafe { &*g1s.add(i).cast::<ArkG1>() });
        }
        for i in 0..n_g2 {
            // SAFETY: `i < n_g2` elements at `g2s`.
            ok &= append_group(hook.transcript, unsafe { &*g2s.add(i).cast::<ArkG2>() });
        }
        if phase == ffi::JOLT_DORY_PHASE_FIRST || phase == ffi::JOLT_DORY_PHASE_SECOND || phase == ffi::JOLT_DORY_PHASE_GAMMA {
            let challenge: Fr = hook.transcript.challenge_scalar();
            // SAFETY: `challenge_out` is one writable jolt_fr_t.
            unsafe { challenge_out.cast::<Fr>().write(challenge) };
        }
        ok
    }));
    match outcome {
        Ok(true) => ffi::JOLT_OK,
        _ => ffi::JOLT_ERR_INVALID_ARG,
    }
}

fn view_arrays(hints: &[HintView<'_>]) -> (Vec<*const ffi::jolt_dory_vec>, Vec<usize>, Vec<usize>) {
    (hints.iter().map(|h| h.0.raw.cast_const()).collect(), hints.iter().map(|h| h.1).collect(), hints.iter().map(|h| h.2).collect())
}

impl HipDorySetup {
    /// `gamma1` and `gamma2` have one length, a power of two; the library checks every point once, here.
    pub fn new(ctx: &Arc<HipContext>, gamma1: &[ArkG1], gamma2: &[ArkG2], h1: &ArkG1, h2: &ArkG2) -> Result<Self, HipError> {
        if gamma1.len() != gamma2.len() {
            return Err(HipError::size_mismatch("HipDorySetup: Gamma1 and Gamma2 have one length"));
        }
        let mut raw = core::ptr::null_mut();
        let _device = ctx.exclusive();
        // SAFETY: the slices hold `gamma1.len()` elements of the layout-compatible arkworks types; `h1` / `h2` are one element each; valid out-pointer.
        check(
            unsafe {
                ffi::jolt_dory_setup_create(ctx.raw, gamma1.as_ptr().cast(), gamma2.as_ptr().cast(), gamma1.len(), (h1 as *const ArkG1).cast(), (h2 as *const ArkG2).cast(), &mut raw)
            },
            ctx.raw,
        )?;
        Ok(Self { ctx: Arc::clone(ctx), raw })
    }

    pub fn size(&self) -> usize {
        let mut n = 0usize;
        // SAFETY: `raw` is a live handle.
        unsafe { ffi::jolt_dory_setup_size(self.raw, &mut n) };
        n
    }

    /// The tier-2 commitments of resident row commitments, one batch: `jolt_dory_setup_tier2`.
    pub fn tier2(&self, hints: &[HintView<'_>]) -> Result<Vec<ArkGT>, HipError> {
        let (vecs, firsts, rows) = view_arrays(hints);
        let mut outs = vec![ffi::jolt_gt_t::default(); hints.len()];
        {
            let _device = self.ctx.exclusive();
            // SAFETY: three arrays of `hints.len()` entries and as many results; live handles borrowed for the call.
            check(unsafe { ffi::jolt_dory_setup_tier2(self.ctx.raw, self.raw, vecs.as_ptr(), firsts.as_ptr(), rows.as_ptr(), hints.len(), outs.as_mut_ptr()) }, self.ctx.raw)?;
        }
        // SAFETY: `ArkGT` is layout-compatible with `jolt_gt_t` (asserted above and in pairing.rs).
        Ok(outs.iter().map(|o| unsafe { core::mem::transmute_copy::<ffi::jolt_gt_t, ArkGT>(o) }).collect())
    }

    /// The whole evaluation proof in one call, under the caller's transcript: hints of at most `2^nu` rows with one scalar each, the device tables
    /// `v = L^T M` (`2^sigma` entries), `left` (`2^nu`) and `right` (`2^sigma`).  The library checks everything before it enqueues anything.
    #[allow(clippy::too_many_arguments)]
    pub fn open_with<T: Transcript<Challenge = Fr>>(&self, hints: &[HintView<'_>], scalars: &[ArkFr], v: &HipTable, left: &HipTable, right: &HipTable, nu: u32, sigma: u32,
                                                    transcript: &mut T) -> Result<HipDoryProof, HipError> {
        if scalars.len() != hints.len() {
            return Err(HipError::size_mismatch("open_with: one scalar per hint"));
        }
        let (mut n_gt, mut n_g1, mut n_g2, mut n_challenges) = (0usize, 0usize, 0usize, 0usize);
        // SAFETY: four valid out-pointers; the call touches no device.
        check(unsafe { ffi::jolt_host_dory_proof_counts(sigma, &mut n_gt, &mut n_g1, &mut n_g2, &mut n_challenges) }, self.ctx.raw)?;
        let (vecs, firsts, rows) = view_arrays(hints);
        let mut gts = vec![ffi::jolt_gt_t::default(); n_gt];
        let mut g1s = vec![ffi::jolt_g1_t::default(); n_g1];
        let mut g2s = vec![ffi::jolt_g2_t::default(); n_g2];
        let mut challenges = vec![Fr::default(); n_challenges];
        let mut hook = Hook { transcript };
        {
            let _device = self.ctx.exclusive();
            // SAFETY: live handles of one context; the arrays are sized by jolt_host_dory_proof_counts; the hook and its transcript outlive the call; the library never unwinds.
            check(
                unsafe {
                    ffi::jolt_host_dory_open_with_transcript(
                        self.ctx.raw,
                        self.raw,
                        vecs.as_ptr(),
                        firsts.as_ptr(),
                        rows.as_ptr(),
                        hints.len(),
                        scalars.as_ptr().cast(),
                        v.raw,
                        left.raw,
                        right.raw,
                        nu,
                        sigma,
                        Some(dory_hook::<T>),
                        (&mut hook as *mut Hook<'_, T>).cast(),
                        gts.as_mut_ptr(),
                        g1s.as_mut_ptr(),
                        g2s.as_mut_ptr(),
                        challenges.as_mut_ptr().cast(),
                    )
                },
                self.ctx.raw,
            )?;
        }
        // SAFETY: the arkworks types are layout-compatible with the ABI's (asserted above, in pairing.rs and in dory_routines.rs).
        Ok(HipDoryProof {
            sigma,
            gts: gts.iter().map(|o| unsafe { core::mem::transmute_copy::<ffi::jolt_gt_t, ArkGT>(o) }).collect(),
            g1s: g1s.iter().map(|o| unsafe { core::mem::transmute_copy::<ffi::jolt_g1_t, ArkG1>(o) }).collect(),
            g2s: g2s.iter().map(|o| unsafe { core::mem::transmute_copy::<ffi::jolt_g2_t, ArkG2>(o) }).collect(),
            challenges,
        })
    }
}

impl Drop for HipDorySetup {
    fn drop(&mut self) {
        let _device = self.ctx.exclusive();
        // SAFETY: `raw` came from jolt_dory_setup_create on this context and is freed once.
        unsafe { ffi::jolt_dory_setup_free(self.ctx.raw, self.raw) };
    }
}

/// Which of a round's two updates [`round_update`] applies.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum RoundUpdate {
    /// `v1 += scalar * a`, `v2 += scalar_inv * b` with `a`, `b` views of Gamma1, Gamma2
    Beta,
    /// `v1`, `a = s1` folded onto their first halves under `scalar`, `v2`, `b = s2` under `scalar_inv`; the four vectors are truncated to `first + n / 2`
    Alpha,
}

/// One of a round's in-place updates as one call, the G1 work beside the G2 work: `jolt_dory_round_update`, enqueued.  Views are `(vector, first)` of `n` elements.
/// `a` and `b` are the bases in beta mode (only read) and the scalar vectors in alpha mode, where the library folds and truncates them on the device: the handle is
/// all that Rust holds of them, so a shared borrow serves both.
#[allow(clippy::too_many_arguments)]
pub fn round_update(ctx: &Arc<HipContext>, mode: RoundUpdate, v1: (&mut HipDoryVec, usize), v2: (&mut HipDoryVec, usize), a: (&HipDoryVec, usize), b: (&HipDoryVec, usize),
                    n: usize, scalar: &ArkFr, scalar_inv: &ArkFr) -> Result<(), HipError> {
    let raw_mode = match mode {
        RoundUpdate::Beta => ffi::JOLT_DORY_UPDATE_BETA,
        RoundUpdate::Alpha => ffi::JOLT_DORY_UPDATE_ALPHA,
    };
    let _device = ctx.exclusive();
    // SAFETY: live handles; `ArkFr` is layout-compatible with `jolt_fr_t` (asserted in dory_routines.rs); the library validates kinds, views and the scalar pair.
    check(
        unsafe {
            ffi::jolt_dory_round_update(ctx.raw, raw_mode, v1.0.raw, v1.1, v2.0.raw, v2.1, a.0.raw, a.1, b.0.raw, b.1, n, (scalar as *const ArkFr).cast(), (scalar_inv as *const ArkFr).cast())
        },
        ctx.raw,
    )
}
