//! lookup_check_hip.rs -- which value of a table's own range-check lookup fails, on the GPU: zkm_lookup_check and
//! zkm_segment_lookup_check of libzkmhip.so (include/zkm_hip.h) for the zkm-prover crate.
//!
//! The reference has no lookup check at all: a wrong FREQUENCIES cell of MemoryStark or RC_FREQUENCIES cell of ArithmeticStark
//! (Stark::lookups(), memory_stark.rs:476-483, arithmetic_stark.rs:269-276) shows up only as a rejected proof.  These calls need the
//! trace alone -- no challenges, no helper columns, no Z -- and name the smallest value whose looking count differs from its
//! frequency (a field element: the sum over the table rows that hold the value), where it is first looked up and first listed, and
//! how many values fail.  The table constraints are witness_check_hip.rs's, the cross-table lookups check_ctls_hip.rs's.
//!
//! Goes into the crate as `prover/src/lookup_check_hip.rs` (`#[cfg(feature = "hip")] pub(crate) mod lookup_check_hip;`), beside
//! witness_check_hip.rs.  NOT COMPILED in the build image (no cargo / rustc there).
use std::ffi::CStr;
use std::os::raw::{c_char, c_int};

use plonky2::field::polynomial::PolynomialValues;
use plonky2::field::types::PrimeField64;
use plonky2::hip::sys::*;

/// One table's result: `lookup` is None when every lookup of the table holds (and for a table without lookups).
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct LookupFinding {
    pub lookup: Option<u64>,
    pub value: u64,
    pub looking: u64,
    pub frequency: u64,
    pub table_rows: u64,
    /// (trace column, row) of the first looking cell that holds the value
    pub first_cell: Option<(u64, u64)>,
    pub first_table_row: Option<u64>,
    pub failing_values: u64,
}

impl LookupFinding {
    fn from_words(w: &[u64]) -> Self {
        let some = |x: u64| if x == u64::MAX { None } else { Some(x) };
        LookupFinding { lookup: some(w[0]), value: w[1], looking: w[2], frequency: w[3], table_rows: w[4],
                        first_cell: some(w[5]).zip(some(w[6])), first_table_row: some(w[7]), failing_values: w[8] }
    }
}

/// The findings, or -- when the check could not be made (a refusal, a runtime failure) -- the library's message.  A failing lookup is a
/// result, not an error: the message that goes with it ("Lookup failed in <Name>Stark: lookup l: value 0x.. is looked up a times ..")
/// is returned beside the findings.
fn finish(rc: c_int, err: *mut c_char, words: &[u64]) -> Result<(Vec<LookupFinding>, Option<String>), String> {
    // (the message is malloc'd by the library; a debugging aid: it is not released)
    let msg = if err.is_null() { None } else { Some(unsafe { CStr::from_ptr(err) }.to_string_lossy().into_owned()) };
    if rc != 0 && !msg.as_deref().map_or(false, |m| m.starts_with("Lookup failed in ")) {
        return Err(msg.unwrap_or_else(|| format!("lookup_check: error {rc}")));
    }
    Ok((words.chunks(ZKM_LOOKUP_FINDING_WORDS).map(LookupFinding::from_words).collect(), msg))
}

/// One table from its columns as the witness generator leaves them (`table_id`: ZKM_TABLE_* of include/zkm_hip.h, as prove_hip.rs maps
/// the Table enum): the columns are flattened into one column-major matrix and copied up for the call.
pub fn lookup_check_hip<F: PrimeField64>(ctx: *mut zkm_ctx, table_id: c_int, columns: &[PolynomialValues<F>]) -> Result<(LookupFinding, Option<String>), String> {
    let n = columns[0].len();
    let flat: Vec<u64> = columns.iter().flat_map(|p| p.values.iter().map(|x| x.to_canonical_u64())).collect();
    let mut words = [0u64; ZKM_LOOKUP_FINDING_WORDS];
    let mut err: *mut c_char = std::ptr::null_mut();
    let rc = unsafe { zkm_lookup_check(ctx, table_id, flat.as_ptr(), columns.len(), n.trailing_zeros(), words.as_mut_ptr(), &mut err) };
    finish(rc, err, &words).map(|(f, msg)| (f[0], msg))
}

/// The twelve tables of a segment (Table::all() order) that are already on the device, e.g. `DeviceSegment::tables()` of segment_hip.rs:
/// the tables with lookups in one set of launches, one download, nothing else moved.  The message names the first failing table in
/// Table::all() order.
pub fn segment_lookup_check_hip(ctx: *mut zkm_ctx, traces: &[*const u64; 12], log_n: &[u32; 12]) -> Result<(Vec<LookupFinding>, Option<String>), String> {
    let mut words = [0u64; 12 * ZKM_LOOKUP_FINDING_WORDS];
    let mut err: *mut c_char = std::ptr::null_mut();
    let rc = unsafe { zkm_segment_lookup_check(ctx, traces.as_ptr(), log_n.as_ptr(), words.as_mut_ptr(), &mut err) };
    finish(rc, err, &words)
}
