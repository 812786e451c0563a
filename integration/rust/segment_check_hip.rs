//! segment_check_hip.rs -- is every segment's witness consistent, on the GPU: zkm_segments_check and zkm_segment_check of libzkmhip.so
//! (include/zkm_hip.h) for the zkm-prover crate.
//!
//! One call runs the table constraints (witness_check_hip.rs), the range-check lookups (lookup_check_hip.rs) and the cross-table lookups
//! (check_ctls_hip.rs) on K segments whose tables are already on the device -- e.g. `DeviceSegment::tables()` of segment_hip.rs -- in one
//! set of launches and two host waits.  A finding is an `Err` that names the segment: the first finding of the lowest inconsistent segment,
//! in eval_vanishing_poly's order (table constraints, the table's lookups, the cross-table lookups).  The same check stands in front of the
//! prove calls under the tuning key "check_witness".
//!
//! Goes into the crate as `prover/src/segment_check_hip.rs` (`#[cfg(feature = "hip")] pub(crate) mod segment_check_hip;`), beside
//! witness_check_hip.rs.  NOT COMPILED in the build image (no cargo / rustc there).
use std::ffi::CStr;
use std::os::raw::{c_char, c_int};

use plonky2::hip::sys::*;

/// What a segment's first finding is.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum SegmentVerdict {
    Consistent,
    /// position of the lowest failing table in Table::all()
    Constraint(usize),
    /// position of the lowest table with a failing range-check lookup
    Lookup(usize),
    /// index of the lowest failing cross-table lookup
    CrossTableLookup(usize),
}

impl SegmentVerdict {
    fn from_words(w: &[u64]) -> Self {
        match w[0] {
            0 => SegmentVerdict::Consistent,
            1 => SegmentVerdict::Constraint(w[1] as usize),
            2 => SegmentVerdict::Lookup(w[1] as usize),
            _ => SegmentVerdict::CrossTableLookup(w[1] as usize),
        }
    }
}

/// An inconsistent call: the lowest segment with a finding, every segment's verdict, and the library's message
/// ("zkm_segments_check: segment s: Constraint failed in CpuStark: row r, constraint i of N = 0x.. (m of n rows fail)").
#[derive(Debug)]
pub struct SegmentCheckError {
    pub segment: Option<usize>,
    pub verdicts: Vec<SegmentVerdict>,
    pub message: String,
}

/// K segments (Table::all() order each).  Ok: every segment is consistent.  Err: the finding, or -- `segment` None -- the reason the check
/// could not be made (a refusal, a runtime failure).
pub fn segments_check_hip(ctx: *mut zkm_ctx, traces: &[[*const u64; 12]], log_n: &[[u32; 12]]) -> Result<(), SegmentCheckError> {
    assert_eq!(traces.len(), log_n.len());
    let k = traces.len();
    let trace_ptrs: Vec<*const *const u64> = traces.iter().map(|t| t.as_ptr()).collect();
    let log_ptrs: Vec<*const u32> = log_n.iter().map(|l| l.as_ptr()).collect();
    let mut words = vec![0u64; ZKM_SEGMENT_VERDICT_WORDS * k];
    let mut err: *mut c_char = std::ptr::null_mut();
    let rc: c_int = unsafe {
        zkm_segments_check(ctx, k, trace_ptrs.as_ptr(), log_ptrs.as_ptr(), words.as_mut_ptr(), std::ptr::null_mut(), std::ptr::null_mut(),
                           std::ptr::null_mut(), &mut err)
    };
    if rc == 0 {
        return Ok(());
    }
    // (the message is malloc'd by the library; a debugging aid: it is not released)
    let message = if err.is_null() { format!("segments_check: error {rc}") } else { unsafe { CStr::from_ptr(err) }.to_string_lossy().into_owned() };
    let verdicts: Vec<SegmentVerdict> = words.chunks(ZKM_SEGMENT_VERDICT_WORDS).map(SegmentVerdict::from_words).collect();
    let segment = verdicts.iter().position(|v| *v != SegmentVerdict::Consistent);
    Err(SegmentCheckError { segment, verdicts, message })
}

/// One segment, with the cross-table report beside the verdict.
pub fn segment_check_hip(ctx: *mut zkm_ctx, traces: &[*const u64; 12], log_n: &[u32; 12]) -> Result<(), (SegmentVerdict, zkm_ctl_report, String)> {
    let mut words = [0u64; ZKM_SEGMENT_VERDICT_WORDS];
    let mut report: zkm_ctl_report = unsafe { std::mem::zeroed() };
    let mut err: *mut c_char = std::ptr::null_mut();
    let rc = unsafe {
        zkm_segment_check(ctx, traces.as_ptr(), log_n.as_ptr(), words.as_mut_ptr(), std::ptr::null_mut(), std::ptr::null_mut(), &mut report, &mut err)
    };
    if rc == 0 {
        return Ok(());
    }
    let message = if err.is_null() { format!("segment_check: error {rc}") } else { unsafe { CStr::from_ptr(err) }.to_string_lossy().into_owned() };
    Err((SegmentVerdict::from_words(&words), report, message))
}
