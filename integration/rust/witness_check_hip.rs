//! witness_check_hip.rs -- which row and which constraint of a table's witness fails, on the GPU: zkm_witness_check and
//! zkm_segment_witness_check of libzkmhip.so (include/zkm_hip.h) for the zkm-prover crate.
//!
//! The reference's check_constraints (prover.rs:793-910) panics with "Constraint failed in <Stark>" and nothing else; these calls need
//! the trace alone -- no challenges, no auxiliary columns -- and name the lowest failing row, the lowest nonzero constraint on it (its
//! index in the emission order of the table's eval_packed_generic), its value, and how many rows fail.  The table's own range-check
//! lookups and the cross-table lookups are not table constraints: lookup_check_hip.rs covers the former, check_ctls_hip.rs the latter.
//!
//! Goes into the crate as `prover/src/witness_check_hip.rs` (`#[cfg(feature = "hip")] pub(crate) mod witness_check_hip;`), beside
//! segment_hip.rs, whose `DeviceSegment::tables()` gives the twelve device pointers.  NOT COMPILED in the build image (no cargo / rustc
//! there).
use std::ffi::CStr;
use std::os::raw::{c_char, c_int};

use plonky2::field::polynomial::PolynomialValues;
use plonky2::field::types::PrimeField64;
use plonky2::hip::sys::*;

/// One table's result: `row` is None when every constraint holds on every row.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct WitnessFinding {
    pub row: Option<u64>,
    pub constraint: u64,
    pub value: u64,
    pub failing_rows: u64,
    pub constraints_per_row: u64,
}

impl WitnessFinding {
    fn from_words(w: &[u64]) -> Self {
        WitnessFinding { row: if w[0] == u64::MAX { None } else { Some(w[0]) }, constraint: w[1], value: w[2], failing_rows: w[3],
                         constraints_per_row: w[4] }
    }
}

/// The findings, or -- when the check could not be made (a refusal, a runtime failure) -- the library's message.  A failing witness is
/// a result, not an error: the message that goes with it ("Constraint failed in <Name>Stark: row r, constraint i of N = 0x.. (m of n
/// rows fail)") is returned beside the findings.
fn finish(rc: c_int, err: *mut c_char, words: &[u64]) -> Result<(Vec<WitnessFinding>, Option<String>), String> {
    // (the message is malloc'd by the library; a debugging aid: it is not released)
    let msg = if err.is_null() { None } else { Some(unsafe { CStr::from_ptr(err) }.to_string_lossy().into_owned()) };
    if rc != 0 && !msg.as_deref().map_or(false, |m| m.starts_with("Constraint failed in ")) {
        return Err(msg.unwrap_or_else(|| format!("witness_check: error {rc}")));
    }
    Ok((words.chunks(ZKM_WITNESS_FINDING_WORDS).map(WitnessFinding::from_words).collect(), msg))
}

/// One table from its columns as the witness generator leaves them (`table_id`: ZKM_TABLE_* of include/zkm_hip.h, as
/// prove_hip.rs maps the Table enum): the columns are flattened into one column-major matrix and copied up for the call.
pub fn witness_check_hip<F: PrimeField64>(ctx: *mut zkm_ctx, table_id: c_int, columns: &[PolynomialValues<F>]) -> Result<(WitnessFinding, Option<String>), String> {
    let n = columns[0].len();
    let flat: Vec<u64> = columns.iter().flat_map(|p| p.values.iter().map(|x| x.to_canonical_u64())).collect();
    let mut words = [0u64; ZKM_WITNESS_FINDING_WORDS];
    let mut err: *mut c_char = std::ptr::null_mut();
    let rc = unsafe { zkm_witness_check(ctx, table_id, flat.as_ptr(), columns.len(), n.trailing_zeros(), words.as_mut_ptr(), &mut err) };
    finish(rc, err, &words).map(|(f, msg)| (f[0], msg))
}

/// The twelve tables of a segment (Table::all() order) that are already on the device, e.g. `DeviceSegment::tables()` of segment_hip.rs:
/// one set of launches, one download, nothing else moved.  The message names the first failing table in Table::all() order.
pub fn segment_witness_check_hip(ctx: *mut zkm_ctx, traces: &[*const u64; 12], log_n: &[u32; 12]) -> Result<(Vec<WitnessFinding>, Option<String>), String> {
    let mut words = [0u64; 12 * ZKM_WITNESS_FINDING_WORDS];
    let mut err: *mut c_char = std::ptr::null_mut();
    let rc = unsafe { zkm_segment_witness_check(ctx, traces.as_ptr(), log_n.as_ptr(), words.as_mut_ptr(), &mut err) };
    finish(rc, err, &words)
}
