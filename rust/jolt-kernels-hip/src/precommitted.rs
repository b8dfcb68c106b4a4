//! The precommitted claim-reduction family on the device: the stage-6b cycle phases and stage-7 address phases of the trusted-advice, untrusted-advice,
//! committed-bytecode and program-image reductions, plus the stage-4 advice opening evaluation -- the nine slots `OptimizedPrecommittedCycle` /
//! `OptimizedPrecommittedAddress` serve in the reference (`crates/jolt-kernels/src/optimized/precommitted_reduction.rs`).
//!
//! The phase kernels are ONE generic operator pair of `libjolt_hip.so` (`jolt_stage_precommitted_cycle_create` / `jolt_stage_precommitted_address_create`,
//! `jolt_amd/csrc/precommitted.hip`): the round algebra of `crates/jolt-kernels/src/precommitted_reduction.rs` over tables resident in HBM, with the round schedule
//! and the variable permutation read from the SAME accessors `OptimizedPrecommittedCycle` reads (`PrecommittedClaimReduction::cycle_phase_rounds`,
//! `address_phase_rounds`, the two totals, `poly_opening_round_permutation_be`).  What this module owns is the prepare side: the advice table / the padded program
//! image / the chunk grids of the public `build_committed_bytecode_chunk_coeffs` go up ONCE, and the eq tables, the value fold, the eq template and the permutes are
//! built on the device (`jolt_eq_evals`, `jolt_eq_evals_shifted`, `jolt_rlc`, `jolt_table_outer`, `jolt_table_permute_bits`).
//!
//! The 6b -> 7 carry.  The reference's `PrecommittedReductionCarry` has private fields, so a carry parked by this tier cannot be handed to the reference's address
//! kernel, nor the reverse: the mixed-tier promise of the reference (either tier's stage 6b feeds either tier's stage 7) does NOT hold for this tier.  A
//! [`HipPrecommittedCycle`] slot pairs only with a [`HipPrecommittedAddress`] slot: the cycle kernel's `park_residue` parks a [`HipPrecommittedCarry<R>`] (the finished
//! operator, whose bound tables and running scale the address operator reclaims on the device), and a missing carry is `KernelError::InvariantViolation` with the
//! reference's reason string.
//!
//! Written blind (no Rust toolchain in the image this repository is built in); `tools/rust_seam_audit.py` checks trait items, arity and the slot / relation pairing.
use core::marker::PhantomData;
use std::ptr;
use std::sync::Arc;

use jolt_claims::protocols::jolt::geometry::claim_reductions::advice::ram_val_check_advice_opening;
use jolt_claims::protocols::jolt::{JoltAdviceKind, JoltChallengeId, PrecommittedClaimReduction, TracePolynomialOrder};
use jolt_claims::{InputClaims, OutputClaims, SumcheckChallenges};
use jolt_field::Fr;
use jolt_kernels::committed_program::{build_committed_bytecode_chunk_coeffs, program_image_words_padded};
use jolt_kernels::opening::AdviceOpeningEvaluation;
use jolt_kernels::{KernelError, PrepareKernel, ProofSession, ProverInputs, SumcheckKernel};
use jolt_verifier::stages::relations::{ConcreteSumcheck, ConcreteSumcheckChallenges, SumcheckInputClaims, SumcheckOutputClaims};
use jolt_verifier::stages::stage6b::committed_reduction_cycle_phase::{
    BytecodeReductionCyclePhase, BytecodeReductionCyclePhaseOutputClaims, ProgramImageReductionCyclePhase, ProgramImageReductionCyclePhaseOutputClaims, TrustedAdviceCyclePhase,
    TrustedAdviceCyclePhaseOutputClaims, UntrustedAdviceCyclePhase, UntrustedAdviceCyclePhaseOutputClaims,
};
use jolt_verifier::stages::stage7::advice_address_phase::{
    TrustedAdviceAddressPhase, TrustedAdviceAddressPhaseOutputClaims, UntrustedAdviceAddressPhase, UntrustedAdviceAddressPhaseOutputClaims,
};
use jolt_verifier::stages::stage7::committed_reduction_address_phase::{
    BytecodeReductionAddressPhase, BytecodeReductionAddressPhaseOutputClaims, ProgramImageReductionAddressPhase, ProgramImageReductionAddressPhaseOutputClaims,
};
use jolt_witness::{JoltWitnessOracle, JoltWitnessPlane};

use crate::context::{HipContext, HipTable};
use crate::ffi;
use crate::ops::HipInts;
use crate::stage::{kernel, kernel_parking, short, Extract, HipStageOp};
use crate::status::{check, HipError};

/// `jolt_rlc` combines at most this many tables in one call (`JOLT_MAX_MEMBER_TABLES`); the bytecode value fold goes in groups above it.
const RLC_GROUP: usize = ffi::JOLT_MAX_MEMBER_TABLES;

/// What a cycle kernel parks for the address slot of relation `R` (`SumcheckKernel::park_residue`): its FINISHED operator.  The device-side twin of
/// `PrecommittedReductionCarry<F, R>` (`precommitted_reduction.rs:225-234`), keyed in the `ProofSession` by the address-phase relation it becomes.
pub struct HipPrecommittedCarry<R>(pub HipStageOp, PhantomData<fn() -> R>);
#[cfg(feature = "allocative")]
impl<R> allocative::Allocative for HipPrecommittedCarry<R> {
    fn visit<'a, 'b: 'a>(&self, visitor: &'a mut allocative::Visitor<'b>) {
        let mut visitor = visitor.enter_self_sized::<Self>();
        visitor.visit_simple(allocative::Key::new("heap"), 0usize); // the tables live in HBM
        visitor.exit();
    }
}

fn park_carry<RA: 'static>(op: HipStageOp, session: &mut ProofSession) {
    session.park(HipPrecommittedCarry::<RA>(op, PhantomData));
}

/// The four stage-6b cycle-phase slots and the stage-4 `advice_opening` slot.
pub struct HipPrecommittedCycle {
    pub ctx: Arc<HipContext>,
}

impl HipPrecommittedCycle {
    pub fn new(ctx: &Arc<HipContext>) -> Self {
        Self { ctx: Arc::clone(ctx) }
    }
}

/// The stage-7 slot of address-phase relation `R`: reclaims the [`HipPrecommittedCarry<R>`] the cycle kernel parked.  `missing_carry`: the reference's diagnostic
/// for a session stage 6b never parked into ("stage 6b parked no ... reduction state for the scheduled address phase").
pub struct HipPrecommittedAddress<R> {
    pub ctx: Arc<HipContext>,
    missing_carry: &'static str,
    _relation: PhantomData<fn() -> R>,
}

impl<R> HipPrecommittedAddress<R> {
    pub fn new(ctx: &Arc<HipContext>, missing_carry: &'static str) -> Self {
        Self { ctx: Arc::clone(ctx), missing_carry, _relation: PhantomData }
    }
}

// ------------------------------------------------------------------------------------------------------------------
// device builders (the prepare side)
// ------------------------------------------------------------------------------------------------------------------
/// `lsb_permutation` (`precommitted_reduction.rs:595-609`): `None` when the relabeling is the identity.
fn lsb_permutation(ctx: &HipContext, perm_be: &[usize]) -> Result<Option<Vec<usize>>, HipError> {
    let mut map = vec![0usize; perm_be.len()];
    let mut same = 0i32;
    // SAFETY: `map` has one entry per variable; plain integers.
    check(unsafe { ffi::jolt_host_precommitted_lsb_permutation(perm_be.as_ptr(), perm_be.len(), map.as_mut_ptr(), &mut same) }, ctx.raw)?;
    Ok((same == 0).then_some(map))
}

/// `permute_challenges` (`:641-652`).
fn permute_challenges(ctx: &HipContext, challenges_be: &[Fr], map: &[usize]) -> Result<Vec<Fr>, HipError> {
    let mut out = vec![Fr::default(); challenges_be.len()];
    // SAFETY: `Fr` has the layout of jolt_fr_t; one map entry and one output per challenge.
    check(unsafe { ffi::jolt_host_precommitted_permute_challenges(challenges_be.as_ptr().cast(), challenges_be.len(), map.as_ptr(), out.as_mut_ptr().cast()) }, ctx.raw)?;
    Ok(out)
}

/// `permute_coefficients` (`:615-636`) into a fresh resident table.
fn permute_bits(table: &HipTable, map: &[usize]) -> Result<HipTable, HipError> {
    let mut raw = ptr::null_mut();
    // SAFETY: live table of 2^map.len() entries (checked by the library); valid out-pointer.
    check(unsafe { ffi::jolt_table_permute_bits(table.ctx.raw, table.raw, map.as_ptr(), map.len(), &mut raw) }, table.ctx.raw)?;
    Ok(HipTable { ctx: Arc::clone(&table.ctx), raw })
}

/// `shifted_eq_slice` (`optimized/precommitted_reduction.rs:337-360`): never the full RAM-domain table.
fn eq_evals_shifted(ctx: &Arc<HipContext>, r: &[Fr], start_index: usize, len: usize) -> Result<HipTable, HipError> {
    let mut raw = ptr::null_mut();
    // SAFETY: layouts as above; valid out-pointer.
    check(unsafe { ffi::jolt_eq_evals_shifted(ctx.raw, r.as_ptr().cast(), r.len(), start_index, len, &mut raw) }, ctx.raw)?;
    Ok(HipTable { ctx: Arc::clone(ctx), raw })
}

/// The bytecode eq template `lane_weights[lane] * eq_cycle[cycle]` (`:419-425`).
fn table_outer(ctx: &Arc<HipContext>, lane_weights: &[Fr], cycle_table: &HipTable, order: TracePolynomialOrder) -> Result<HipTable, HipError> {
    let order = match order {
        TracePolynomialOrder::CycleMajor => ffi::JOLT_TRACE_CYCLE_MAJOR,
        TracePolynomialOrder::AddressMajor => ffi::JOLT_TRACE_ADDRESS_MAJOR,
    };
    let mut raw = ptr::null_mut();
    // SAFETY: `lane_weights.len()` field elements; live cycle table; valid out-pointer.
    check(unsafe { ffi::jolt_table_outer(ctx.raw, lane_weights.as_ptr().cast(), lane_weights.len(), cycle_table.raw, order, &mut raw) }, ctx.raw)?;
    Ok(HipTable { ctx: Arc::clone(ctx), raw })
}

/// The cycle operator over tables already in opening-round order.  The library copies them: the caller's handles are dropped when this returns.
fn cycle_op(ctx: &Arc<HipContext>, reduction: &PrecommittedClaimReduction, value: &HipTable, eq: &HipTable, aux: &[HipTable]) -> Result<HipStageOp, KernelError<Fr>> {
    let expected = 1usize << reduction.poly_opening_round_permutation_be().len();
    for (name, table) in [("value", value), ("eq", eq)].into_iter().chain(aux.iter().map(|t| ("aux", t))) {
        if table.len() != expected {
            return Err(KernelError::TableSizeMismatch { table: format!("precommitted reduction {name}"), expected, got: table.len() });
        }
    }
    let aux_raw: Vec<*const ffi::jolt_table> = aux.iter().map(|t| t.raw.cast_const()).collect();
    let (cycle, address) = (reduction.cycle_phase_rounds(), reduction.address_phase_rounds());
    let mut raw = ptr::null_mut();
    // SAFETY: live tables of one length; the round lists are plain integers that outlive the call.
    check(
        unsafe {
            ffi::jolt_stage_precommitted_cycle_create(
                ctx.raw,
                value.raw,
                eq.raw,
                aux_raw.as_ptr(),
                aux_raw.len(),
                cycle.as_ptr(),
                cycle.len(),
                reduction.cycle_phase_total_rounds(),
                address.as_ptr(),
                address.len(),
                reduction.address_phase_total_rounds(),
                &mut raw,
            )
        },
        ctx.raw,
    )?;
    Ok(HipStageOp::adopt(ctx, raw)?)
}

/// The typed cycle kernel: the operator, the claim extraction, and -- with an address phase scheduled -- the carry parked under `RA`'s key (`park_carry`, `:367-379`).
fn cycle_kernel<RC, RA>(op: HipStageOp, has_address_phase: bool, extract: Extract<RC>) -> Box<dyn SumcheckKernel<Fr, Relation = RC>>
where
    RC: ConcreteSumcheck<Fr> + 'static,
    RA: 'static,
    SumcheckInputClaims<Fr, RC>: InputClaims<Fr>,
    SumcheckOutputClaims<Fr, RC>: OutputClaims<Fr>,
    ConcreteSumcheckChallenges<Fr, RC>: SumcheckChallenges<Fr, JoltChallengeId>,
{
    if has_address_phase {
        kernel_parking(op, Vec::new(), extract, park_carry::<RA>)
    } else {
        kernel(op, Vec::new(), extract)
    }
}

fn advice_table(ctx: &Arc<HipContext>, witness: &dyn JoltWitnessOracle<Fr>, kind: JoltAdviceKind, expected_vars: usize) -> Result<HipTable, KernelError<Fr>> {
    let table = witness.oracle_table(ram_val_check_advice_opening(kind).polynomial_id()).map_err(KernelError::from)?;
    if table.len() != 1usize << expected_vars {
        return Err(KernelError::TableSizeMismatch { table: format!("{kind:?} advice"), expected: 1usize << expected_vars, got: table.len() });
    }
    Ok(ctx.upload(&table)?)
}

/// `for_advice` (`optimized/precommitted_reduction.rs:223-249`): the eq table from the permuted challenges directly, only the advice table pays the permute.
fn advice_op(ctx: &Arc<HipContext>, kind: JoltAdviceKind, reduction: &PrecommittedClaimReduction, r_val: &[Fr], witness: &dyn JoltWitnessPlane<Fr>) -> Result<HipStageOp, KernelError<Fr>> {
    let permutation = reduction.poly_opening_round_permutation_be();
    if r_val.len() != permutation.len() {
        return Err(KernelError::InvalidGeometry { reason: format!("advice reference point has {} variables, schedule expects {}", r_val.len(), permutation.len()) });
    }
    let table = advice_table(ctx, witness, kind, permutation.len())?;
    let (value, eq) = match lsb_permutation(ctx, permutation)? {
        Some(map) => (permute_bits(&table, &map)?, ctx.eq_evals(&permute_challenges(ctx, r_val, &map)?, None)?),
        None => (table, ctx.eq_evals(r_val, None)?),
    };
    cycle_op(ctx, reduction, &value, &eq, &[])
}

// ---------------------------------------------------------------- advice
impl AdviceOpeningEvaluation<Fr> for HipPrecommittedCycle {
    #[tracing::instrument(skip_all, name = "HipAdviceOpeningEvaluation::evaluate", fields(kind = ?kind))]
    fn evaluate(&self, _session: &mut ProofSession, kind: JoltAdviceKind, point: &[Fr], witness: &dyn JoltWitnessOracle<Fr>) -> Result<Fr, KernelError<Fr>> {
        // one eq expansion and one dot product on the device (jolt_table_evaluate)
        Ok(advice_table(&self.ctx, witness, kind, point.len())?.evaluate(point)?)
    }
}

impl PrepareKernel<Fr, TrustedAdviceCyclePhase<Fr>> for HipPrecommittedCycle {
    #[tracing::instrument(skip_all, name = "HipPrecommittedCycle::prepare_trusted_advice")]
    fn prepare(
        &self,
        _session: &mut ProofSession,
        witness: &dyn JoltWitnessPlane<Fr>,
        inputs: ProverInputs<'_, Fr, TrustedAdviceCyclePhase<Fr>>,
    ) -> Result<Box<dyn SumcheckKernel<Fr, Relation = TrustedAdviceCyclePhase<Fr>>>, KernelError<Fr>> {
        let r_val = inputs.relation.reference_opening_point().ok_or(KernelError::InvariantViolation { reason: "trusted-advice cycle phase carries no reference opening point" })?;
        let reduction = inputs.relation.layout().precommitted();
        let op = advice_op(&self.ctx, JoltAdviceKind::Trusted, reduction, r_val, witness)?;
        // output values: the intermediate claim with an address phase scheduled, else the bound advice coefficient (scalar_claim, precommitted_reduction.rs:359-365)
        Ok(cycle_kernel::<_, TrustedAdviceAddressPhase<Fr>>(op, reduction.num_address_phase_rounds() > 0, Box::new(|v, _| {
            short(v, 1)?;
            Ok(TrustedAdviceCyclePhaseOutputClaims { trusted: v[0] })
        })))
    }
}

impl PrepareKernel<Fr, UntrustedAdviceCyclePhase<Fr>> for HipPrecommittedCycle {
    #[tracing::instrument(skip_all, name = "HipPrecommittedCycle::prepare_untrusted_advice")]
    fn prepare(
        &self,
        _session: &mut ProofSession,
        witness: &dyn JoltWitnessPlane<Fr>,
        inputs: ProverInputs<'_, Fr, UntrustedAdviceCyclePhase<Fr>>,
    ) -> Result<Box<dyn SumcheckKernel<Fr, Relation = UntrustedAdviceCyclePhase<Fr>>>, KernelError<Fr>> {
        let r_val = inputs.relation.reference_opening_point().ok_or(KernelError::InvariantViolation { reason: "untrusted-advice cycle phase carries no reference opening point" })?;
        let reduction = inputs.relation.layout().precommitted();
        let op = advice_op(&self.ctx, JoltAdviceKind::Untrusted, reduction, r_val, witness)?;
        Ok(cycle_kernel::<_, UntrustedAdviceAddressPhase<Fr>>(op, reduction.num_address_phase_rounds() > 0, Box::new(|v, _| {
            short(v, 1)?;
            Ok(UntrustedAdviceCyclePhaseOutputClaims { untrusted: v[0] })
        })))
    }
}

// --------------------------------------------------------- program image
impl PrepareKernel<Fr, ProgramImageReductionCyclePhase<Fr>> for HipPrecommittedCycle {
    /// `for_program_image` (`:298-334`): the padded word vector goes up as u64 and is promoted on the device; the shifted eq slice is built there from aligned blocks.
    #[tracing::instrument(skip_all, name = "HipPrecommittedCycle::prepare_program_image")]
    fn prepare(
        &self,
        _session: &mut ProofSession,
        witness: &dyn JoltWitnessPlane<Fr>,
        inputs: ProverInputs<'_, Fr, ProgramImageReductionCyclePhase<Fr>>,
    ) -> Result<Box<dyn SumcheckKernel<Fr, Relation = ProgramImageReductionCyclePhase<Fr>>>, KernelError<Fr>> {
        let ctx = &self.ctx;
        let layout = inputs.relation.layout();
        let reduction = layout.precommitted();
        let (r_addr_rw, start_index) = (inputs.relation.r_addr_rw(), layout.start_index());
        let words = program_image_words_padded(&witness.program_preprocessing().ram.bytecode_words);
        let padded_len = words.len();
        let expected = 1usize << reduction.poly_opening_round_permutation_be().len();
        if padded_len != expected {
            return Err(KernelError::TableSizeMismatch { table: "program image words".to_owned(), expected, got: padded_len });
        }
        let ram_domain = 1usize << r_addr_rw.len();
        if start_index >= ram_domain || padded_len > ram_domain {
            return Err(KernelError::InvalidGeometry { reason: format!("program image block [{start_index}, +{padded_len}) cannot index the RAM domain {ram_domain}") });
        }
        let value = HipInts::from_u64(ctx, &words)?.to_table(0, padded_len)?;
        let eq = eq_evals_shifted(ctx, r_addr_rw, start_index, padded_len)?;
        let (value, eq) = match lsb_permutation(ctx, reduction.poly_opening_round_permutation_be())? {
            Some(map) => (permute_bits(&value, &map)?, permute_bits(&eq, &map)?),
            None => (value, eq),
        };
        let op = cycle_op(ctx, reduction, &value, &eq, &[])?;
        Ok(cycle_kernel::<_, ProgramImageReductionAddressPhase<Fr>>(op, reduction.num_address_phase_rounds() > 0, Box::new(|v, _| {
            short(v, 1)?;
            Ok(ProgramImageReductionCyclePhaseOutputClaims { program_image: v[0] })
        })))
    }
}

// -------------------------------------------------------------- bytecode
impl PrepareKernel<Fr, BytecodeReductionCyclePhase<Fr>> for HipPrecommittedCycle {
    /// `for_bytecode` (`:396-465`): the chunk grids of the public `build_committed_bytecode_chunk_coeffs` (the instruction decoding stays with the reference), uploaded
    /// once; the chunk-weighted value fold (`jolt_rlc`, in groups above 40 chunks), the lane-weight eq template and the permutes run on the device; the raw grids ride
    /// along as passengers -- their fully bound coefficients are the per-chunk openings.
    #[tracing::instrument(skip_all, name = "HipPrecommittedCycle::prepare_bytecode")]
    fn prepare(
        &self,
        _session: &mut ProofSession,
        witness: &dyn JoltWitnessPlane<Fr>,
        inputs: ProverInputs<'_, Fr, BytecodeReductionCyclePhase<Fr>>,
    ) -> Result<Box<dyn SumcheckKernel<Fr, Relation = BytecodeReductionCyclePhase<Fr>>>, KernelError<Fr>> {
        let ctx = &self.ctx;
        let layout = inputs.relation.layout();
        let weights = inputs.relation.weights();
        let reduction = layout.precommitted();
        let program = witness.program_preprocessing();
        let chunk_coeffs: Vec<Vec<Fr>> = build_committed_bytecode_chunk_coeffs(&program.bytecode.bytecode, layout.chunk_count(), layout.trace_order())?;
        if chunk_coeffs.is_empty() {
            return Err(KernelError::InvariantViolation { reason: "committed bytecode grid build produced no grid" });
        }
        let expected = 1usize << reduction.poly_opening_round_permutation_be().len();
        if chunk_coeffs[0].len() != expected {
            return Err(KernelError::TableSizeMismatch { table: "committed bytecode chunk grid".to_owned(), expected, got: chunk_coeffs[0].len() });
        }
        if weights.chunk_rbc_weights.len() != chunk_coeffs.len() {
            return Err(KernelError::TableSizeMismatch { table: "bytecode chunk weights".to_owned(), expected: chunk_coeffs.len(), got: weights.chunk_rbc_weights.len() });
        }
        let chunks: Vec<HipTable> = chunk_coeffs.iter().map(|c| ctx.upload(c)).collect::<Result<_, _>>()?;
        drop(chunk_coeffs);
        // value[index] = sum_c w_c chunk_c[index]
        let value = if chunks.len() <= RLC_GROUP {
            ctx.rlc(&chunks.iter().collect::<Vec<_>>(), &weights.chunk_rbc_weights)?
        } else {
            let parts: Vec<HipTable> = chunks
                .chunks(RLC_GROUP)
                .zip(weights.chunk_rbc_weights.chunks(RLC_GROUP))
                .map(|(tables, scalars)| ctx.rlc(&tables.iter().collect::<Vec<_>>(), scalars))
                .collect::<Result<_, _>>()?;
            ctx.rlc(&parts.iter().collect::<Vec<_>>(), &vec![Fr::from_u64(1); parts.len()])?
        };
        let eq_cycle = ctx.eq_evals(&weights.r_bc, None)?;
        let eq = table_outer(ctx, &weights.lane_weights, &eq_cycle, layout.trace_order())?;
        let (value, eq, chunks) = match lsb_permutation(ctx, reduction.poly_opening_round_permutation_be())? {
            Some(map) => (permute_bits(&value, &map)?, permute_bits(&eq, &map)?, chunks.iter().map(|c| permute_bits(c, &map)).collect::<Result<Vec<_>, _>>()?),
            None => (value, eq, chunks),
        };
        let op = cycle_op(ctx, reduction, &value, &eq, &chunks)?;
        let has_address_phase = reduction.num_address_phase_rounds() > 0;
        // output values: {the intermediate claim} with an address phase scheduled, else {the bound fold, the bound chunk grids} (precommitted_reduction.rs:492-510)
        Ok(cycle_kernel::<_, BytecodeReductionAddressPhase<Fr>>(op, has_address_phase, Box::new(move |v, _| {
            short(v, 1)?;
            Ok(if has_address_phase {
                BytecodeReductionCyclePhaseOutputClaims { intermediate: Some(v[0]), chunks: Vec::new() }
            } else {
                BytecodeReductionCyclePhaseOutputClaims { intermediate: None, chunks: v[1..].to_vec() }
            })
        })))
    }
}

// ------------------------------------------------------ the address phases
/// How an address relation names the operator's output values {the bound value, the bound passengers} on the wire (`precommitted_reduction.rs:536-590`).
pub trait AddressPhaseClaims: ConcreteSumcheck<Fr> + Sized
where
    SumcheckInputClaims<Fr, Self>: InputClaims<Fr>,
    SumcheckOutputClaims<Fr, Self>: OutputClaims<Fr>,
    ConcreteSumcheckChallenges<Fr, Self>: SumcheckChallenges<Fr, JoltChallengeId>,
{
    fn claims(values: &[Fr]) -> SumcheckOutputClaims<Fr, Self>;
}
impl AddressPhaseClaims for TrustedAdviceAddressPhase<Fr> {
    fn claims(values: &[Fr]) -> TrustedAdviceAddressPhaseOutputClaims<Fr> {
        TrustedAdviceAddressPhaseOutputClaims { trusted: values[0] }
    }
}
impl AddressPhaseClaims for UntrustedAdviceAddressPhase<Fr> {
    fn claims(values: &[Fr]) -> UntrustedAdviceAddressPhaseOutputClaims<Fr> {
        UntrustedAdviceAddressPhaseOutputClaims { untrusted: values[0] }
    }
}
impl AddressPhaseClaims for BytecodeReductionAddressPhase<Fr> {
    fn claims(values: &[Fr]) -> BytecodeReductionAddressPhaseOutputClaims<Fr> {
        BytecodeReductionAddressPhaseOutputClaims { chunks: values[1..].to_vec() }
    }
}
impl AddressPhaseClaims for ProgramImageReductionAddressPhase<Fr> {
    fn claims(values: &[Fr]) -> ProgramImageReductionAddressPhaseOutputClaims<Fr> {
        ProgramImageReductionAddressPhaseOutputClaims { program_image: values[0] }
    }
}

impl<R> PrepareKernel<Fr, R> for HipPrecommittedAddress<R>
where
    R: AddressPhaseClaims + 'static,
    SumcheckInputClaims<Fr, R>: InputClaims<Fr>,
    SumcheckOutputClaims<Fr, R>: OutputClaims<Fr>,
    ConcreteSumcheckChallenges<Fr, R>: SumcheckChallenges<Fr, JoltChallengeId>,
{
    #[tracing::instrument(skip_all, name = "HipPrecommittedAddress::prepare")]
    fn prepare(
        &self,
        session: &mut ProofSession,
        _witness: &dyn JoltWitnessPlane<Fr>,
        _inputs: ProverInputs<'_, Fr, R>,
    ) -> Result<Box<dyn SumcheckKernel<Fr, Relation = R>>, KernelError<Fr>> {
        // only a Hip cycle slot parks this carry: a reference-tier stage 6b leaves a PrecommittedReductionCarry this tier cannot open (private fields)
        let HipPrecommittedCarry(cycle, _) = session.take::<HipPrecommittedCarry<R>>().ok_or(KernelError::InvariantViolation { reason: self.missing_carry })?;
        let mut raw = ptr::null_mut();
        // SAFETY: the cycle operator has finished its rounds (the stage driver parks residues after the round loop); valid out-pointer.
        check(unsafe { ffi::jolt_stage_precommitted_address_create(self.ctx.raw, cycle.raw, &mut raw) }, self.ctx.raw)?;
        drop(cycle); // its tables and scale have moved into the address operator
        let op = HipStageOp::adopt(&self.ctx, raw)?;
        Ok(kernel(op, Vec::new(), Box::new(|v, _| {
            short(v, 1)?;
            Ok(R::claims(v))
        })))
    }
}
