//! verify_hip.rs -- verify_proof (prover/src/verifier.rs:27-176) on the GPU: zkm_verify_segments of libzkmhip.so (include/zkm_hip.h)
//! behind the reference's argument list, failing with the reference's `ensure!` messages.
//!
//! Goes into the zkm-prover crate as `prover/src/verify_hip.rs` (it reads the `pub(crate)` field `AllProof::ctl_challenges`,
//! proof.rs:25-29); `prove_root` / `prove_root_with_assumption` (fixed_recursive_verifier.rs:777, 853) call
//! `verify_proof_hip(ctx, all_stark, all_proof.clone(), config)` where they call `verify_proof(..).unwrap()`, and a driver that has K
//! segment proofs at hand verifies them in one set of launches with `verify_proofs_hip`.  The AllStark description ships inside the
//! library, so `all_stark` only fixes the type: the blobs are `proof_blob::stark_proof_to_blob` of the twelve table proofs in
//! Table::all() order, the inverse of what `prove_with_traces_hip` does with the library's output.  The reference items used here are
//! checked by tests/test_rust_verify_names.py.  NOT COMPILED in the build image (no cargo / rustc there).
use std::ffi::CStr;
use std::os::raw::c_char;

use anyhow::{anyhow, ensure, Result};
use plonky2::field::extension::Extendable;
use plonky2::field::types::PrimeField64;
use plonky2::hash::hash_types::{HashOut, RichField};
use plonky2::hip::sys::*;
use plonky2::plonk::config::{GenericConfig, Hasher};

use crate::all_stark::{AllStark, NUM_TABLES};
use crate::config::StarkConfig;
use crate::proof::AllProof;
use crate::proof_blob::stark_proof_to_blob;
use crate::prove_hip::{public_values_words, zkm_config};

/// One segment as zkm_verify_segments takes it: the twelve blobs concatenated, the public values as the transcript observes them, and
/// the claimed CTL challenges.
pub struct SegmentBlobs {
    pub proofs: Vec<u64>,
    pub public_values: Vec<u64>,
    pub ctl_challenges: Vec<u64>,
}

/// AllProof -> the blob layout (the inverse of `stark_proof_from_blob` per table).
pub fn all_proof_to_blobs<F, C, const D: usize>(all_proof: &AllProof<F, C, D>, config: &StarkConfig) -> SegmentBlobs
where
    F: RichField + Extendable<D>,
    C: GenericConfig<D, F = F>,
    C::Hasher: Hasher<F, Hash = HashOut<F>>,
{
    let mut proofs = Vec::new();
    for p in all_proof.stark_proofs.iter() {
        proofs.extend(stark_proof_to_blob::<F, C, D>(p, config));
    }
    let ctl_challenges = all_proof.ctl_challenges.challenges.iter().flat_map(|c| [c.beta.to_canonical_u64(), c.gamma.to_canonical_u64()]).collect();
    SegmentBlobs { proofs, public_values: public_values_words(&all_proof.public_values), ctl_challenges }
}

/// The reference's message for a report (verifier.rs:248-264, plonky2 fri/verifier.rs and hash/merkle_proofs.rs, cross_table_lookup.rs
/// verify_cross_table_lookups), in front of the library's own text, which names segment, table, query and layer.
fn reference_message(report: &zkm_verify_report) -> &'static str {
    match report.code {
        ZKM_VERIFY_SHAPE => "validate_proof_shape failed",
        ZKM_VERIFY_TRANSCRIPT_STATE | ZKM_VERIFY_CTL_CHALLENGES => "Invalid sampling of proof challenges.",
        ZKM_VERIFY_QUOTIENT => "Mismatch between evaluation and opening of quotient polynomial",
        ZKM_VERIFY_POW => "Invalid proof of work witness.",
        ZKM_VERIFY_INITIAL_MERKLE | ZKM_VERIFY_FRI_MERKLE => "Invalid Merkle proof.",
        ZKM_VERIFY_FRI_EVAL => "FRI query evaluation mismatch",
        ZKM_VERIFY_FINAL_POLY => "Final polynomial evaluation is invalid.",
        ZKM_VERIFY_CTL_SUM => "CTL verification failed",
        _ => "the proof could not be verified",
    }
}

/// K segment proofs in one set of launches (zkm_verify_segments): Ok when every proof is accepted, else the first rejection.
pub fn verify_proofs_hip(ctx: *mut zkm_ctx, segments: &[SegmentBlobs], config: &StarkConfig) -> Result<()> {
    ensure!(!segments.is_empty(), "no proof to verify");
    let cfg = zkm_config(config);
    let proofs: Vec<*const u64> = segments.iter().map(|s| s.proofs.as_ptr()).collect();
    let words: Vec<usize> = segments.iter().map(|s| s.proofs.len()).collect();
    let pubs: Vec<*const u64> = segments.iter().map(|s| s.public_values.as_ptr()).collect();
    let npubs: Vec<usize> = segments.iter().map(|s| s.public_values.len()).collect();
    let chals: Vec<*const u64> = segments.iter().map(|s| s.ctl_challenges.as_ptr()).collect();
    for s in segments {
        ensure!(s.ctl_challenges.len() == 2 * config.num_challenges, "a segment claims {} challenge words", s.ctl_challenges.len());
    }
    let mut reports: Vec<zkm_verify_report> = vec![zkm_verify_report::default(); segments.len()];
    let mut err: *mut c_char = std::ptr::null_mut();
    let rc = unsafe {
        zkm_verify_segments(ctx, &cfg, segments.len(), proofs.as_ptr(), words.as_ptr(), pubs.as_ptr(), npubs.as_ptr(), chals.as_ptr(),
                            reports.as_mut_ptr(), &mut err)
    };
    if rc == 0 {
        return Ok(());
    }
    let text = if err.is_null() { format!("zkm_verify_segments: error {rc}") } else { unsafe { CStr::from_ptr(err) }.to_string_lossy().into_owned() };
    if !err.is_null() {
        unsafe { libc::free(err as *mut libc::c_void) };
    }
    let report = reports.iter().find(|r| r.code != ZKM_VERIFY_OK).copied().unwrap_or_default();
    Err(anyhow!("{} ({text}; table {}, query {}, layer {}, lookup {})", reference_message(&report), report.table, report.query, report.layer, report.ctl))
}

/// `verify_proof(all_stark, all_proof, config)` (verifier.rs:27-31) on the GPU of `ctx`.
pub fn verify_proof_hip<F, C, const D: usize>(ctx: *mut zkm_ctx, all_stark: &AllStark<F, D>, all_proof: AllProof<F, C, D>, config: &StarkConfig) -> Result<()>
where
    F: RichField + Extendable<D>,
    C: GenericConfig<D, F = F>,
    C::Hasher: Hasher<F, Hash = HashOut<F>>,
{
    ensure!(all_stark.cross_table_lookups.len() == 15 && all_proof.stark_proofs.len() == NUM_TABLES,
            "libzkmhip verifies the AllStark it ships with (all_stark.rs:136-542)");
    verify_proofs_hip(ctx, &[all_proof_to_blobs(&all_proof, config)], config)
}
