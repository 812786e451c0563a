//! sha_calls_hip.rs -- the SHA-256 precompile calls of a segment expanded by libzkmhip.so (include/zkm_hip.h "SHA-256 precompile calls
//! from their inputs") instead of on the host.  `generate_sha_extend` and `generate_sha_compress` (witness/operation.rs:1183-1285,
//! :1298-1458) keep updating the emulator's memory, but push neither their CPU rows (96 a SYSSHAEXTEND, 11 a SYSSHACOMPRESS) nor, through
//! `sha_extend_sponge_log` / `sha_compress_sponge_log` (witness/util.rs:559-694), the sponge's memory reads, the logic operations and the
//! ShaExtend rows: they record the call -- 96 or 352 bytes, the lists the sponge tables need anyway -- and reserve the call's positions
//! in the step list.  `finish` has the library write everything else on the device.
//!
//! How a maintainer hooks it in, on top of cpu_steps_hip.rs:
//!   * `GenerationState` gets a `sha_log: ShaCallLog` beside its `step_log: StepLog`;
//!   * `generate_sha_extend(state, w_ptr, a1)` reads w[0..16] from memory, computes w[16..64] into memory as today and calls
//!     `sha_log.record_sha_extend(&mut step_log, clock, w_ptr, w16)` in place of its loop's row and trace pushes (clock: the clock of
//!     the first row the call would have pushed);
//!   * `generate_sha_compress(state, w_ptr, h_ptr)` likewise calls `record_sha_compress(&mut step_log, clock, w_ptr, h_ptr, hx, w)`;
//!   * at the end of the segment `finish` expands the calls into device memory and patches the reserved steps; the segment is then
//!     proven with `prove_segments_ops_steps_raw`, its `zkm_cpu_steps.raw_rows` and the memory / logic / ShaExtend lists of its
//!     `zkm_segment_ops` pointing at the device blocks `finish` returns.
//! The SYSCALL row in front of a call is logged as today.  SYSKECCAK calls: keccak_calls_hip.rs (the Poseidon sponge has no syscall).
//! A segment that also has calls of another kind does not compose the expansions itself: it hands this log and the others to
//! `calls_hip.rs` (`SegmentCalls`, `prove_segments_ops_calls_raw`: zkm_prove_segments_ops_calls), which expands K segments' calls in one
//! set of launches; `finish` below is the segment whose only calls are SHA calls.
//!
//! Goes into the zkm-prover crate as `prover/src/sha_calls_hip.rs`, beside `cpu_steps_hip.rs`.  NOT COMPILED in the build image (no
//! cargo / rustc there).
use anyhow::{ensure, Result};
use plonky2::hip::sys::*;

use crate::cpu_steps_hip::StepLog;

const CPU_COLS: usize = 259;

/// The SHA calls of one segment: the lists of zkm_segment_ops' two SHA sponge groups, and where each call's steps were reserved.
#[derive(Default)]
pub struct ShaCallLog {
    pub extend_w16: Vec<u32>,    // 16 words a call
    pub extend_meta: Vec<u64>,   // 4 words a call: context, segment, address of w[0], timestamp of round 0's sponge row
    pub compress_hx: Vec<u32>,   // 8 words a call
    pub compress_w: Vec<u32>,    // 64 words a call
    pub compress_meta: Vec<u64>, // 8 words a call: context, segment, address of hx[0], timestamp, address of w[0], segment and context of w, 0
    first_clock: Option<u64>,    // the clock of step 0 of the step list (the bootstrap's row count)
}

/// Device memory `finish` filled: own items in front, generated items behind.  Freed with zkm_dev_free.
pub struct ShaCallBlocks {
    pub raw_rows: *mut u64,
    pub nraw: usize,
    pub memory_ops: *mut u64,
    pub nmemory: usize,
    pub logic_ops: *mut u32,
    pub nlogic: usize,
    pub sha_extend_inputs: *mut u8,
    pub sha_extend_timestamps: *mut u64,
    pub nsha_extend: usize,
}

impl ShaCallLog {
    pub fn nextend(&self) -> usize {
        self.extend_meta.len() / 4
    }

    pub fn ncompress(&self) -> usize {
        self.compress_meta.len() / 8
    }

    fn reserve(&mut self, steps: &mut StepLog, clock: u64, rows: usize) {
        // the step at position i of the list is the row of clock first_clock + i: the call's rows take the next `rows` positions
        let first = *self.first_clock.get_or_insert(clock - steps.steps.len() as u64);
        debug_assert_eq!(first + steps.steps.len() as u64, clock);
        steps.steps.extend((0..rows).map(|_| zkm_cpu_step { kind: ZKM_STEP_RAW, ..Default::default() }));
    }

    /// A SYSSHAEXTEND call: context 0, Segment::Code (0), `w16` = w[0..16] as read from memory.  `clock`: state.traces.clock() at the call.
    pub fn record_sha_extend(&mut self, steps: &mut StepLog, clock: u64, w_ptr: usize, w16: &[u32; 16]) {
        self.extend_w16.extend_from_slice(w16);
        // round 0's read row is at `clock`, its sponge row one later; timestamps are clock * NUM_CHANNELS
        self.extend_meta.extend_from_slice(&[0, 0, w_ptr as u64, (clock + 1) * 10]);
        self.reserve(steps, clock, 96);
    }

    /// A SYSSHACOMPRESS call: `hx` = the eight words at h_ptr before the call, `w` = the 64 schedule words at w_ptr.
    pub fn record_sha_compress(&mut self, steps: &mut StepLog, clock: u64, w_ptr: usize, h_ptr: usize, hx: &[u32; 8], w: &[u32; 64]) {
        self.compress_hx.extend_from_slice(hx);
        self.compress_w.extend_from_slice(w);
        // the hx row is at `clock`, the eight w rows behind it, the sponge row at clock + 9
        self.compress_meta.extend_from_slice(&[0, 0, h_ptr as u64, (clock + 9) * 10, w_ptr as u64, 0, 0, 0]);
        self.reserve(steps, clock, 11);
    }

    /// Expand the calls on the device and patch the reserved steps.  `own_memory` / `own_logic`: the operations left in Traces (6 words /
    /// 3 words each), which go in front of the generated ones; the own RAW rows are `steps.raw_rows`.  The returned blocks hold own +
    /// generated; `steps.list()` must then be given `raw_rows = blocks.raw_rows, nraw = blocks.nraw`.
    pub fn finish(&self, ctx: *mut zkm_ctx, steps: &mut StepLog, own_memory: &[u64], own_logic: &[u32]) -> Result<ShaCallBlocks> {
        let (ne, nc) = (self.nextend(), self.ncompress());
        let (mut rows, mut mem, mut logic, mut ext) = (0usize, 0usize, 0usize, 0usize);
        unsafe { zkm_sha_calls_counts(ne, nc, &mut rows, &mut mem, &mut logic, &mut ext) };
        let own_raw = steps.raw_rows.len() / CPU_COLS;
        // the one statement of masks and positions: the records and the clock each belongs at
        let mut records = vec![zkm_cpu_step::default(); rows];
        let mut clocks = vec![0u64; rows];
        let mut err = std::ptr::null_mut();
        let rc = unsafe {
            zkm_sha_calls_steps(self.extend_meta.as_ptr(), ne, self.compress_meta.as_ptr(), nc, own_raw, records.as_mut_ptr(), clocks.as_mut_ptr(), &mut err)
        };
        check(rc, err)?;
        let first = self.first_clock.unwrap_or(0);
        for (record, clock) in records.iter().zip(&clocks) {
            let at = (clock - first) as usize;
            ensure!(at < steps.steps.len() && steps.steps[at].kind == ZKM_STEP_RAW, "no step was reserved at clock {}", clock);
            steps.steps[at] = *record;
        }
        let alloc = |bytes: usize| -> Result<*mut std::ffi::c_void> {
            let (mut p, mut err) = (std::ptr::null_mut(), std::ptr::null_mut());
            check(unsafe { zkm_dev_alloc(ctx, bytes.max(8), &mut p, &mut err) }, err)?;
            Ok(p)
        };
        let upload = |dst: *mut std::ffi::c_void, src: *const std::ffi::c_void, bytes: usize| -> Result<()> {
            let mut err = std::ptr::null_mut();
            if bytes != 0 {
                check(unsafe { zkm_dev_upload(ctx, dst, src, bytes, &mut err) }, err)?;
            }
            Ok(())
        };
        let blocks = ShaCallBlocks {
            raw_rows: alloc((own_raw + rows) * CPU_COLS * 8)? as *mut u64,
            nraw: own_raw + rows,
            memory_ops: alloc((own_memory.len() + 6 * mem) * 8)? as *mut u64,
            nmemory: own_memory.len() / 6 + mem,
            logic_ops: alloc((own_logic.len() + 3 * logic) * 4)? as *mut u32,
            nlogic: own_logic.len() / 3 + logic,
            sha_extend_inputs: alloc(16 * ext)? as *mut u8,
            sha_extend_timestamps: alloc(8 * ext)? as *mut u64,
            nsha_extend: ext,
        };
        upload(blocks.raw_rows as *mut _, steps.raw_rows.as_ptr() as *const _, steps.raw_rows.len() * 8)?;
        upload(blocks.memory_ops as *mut _, own_memory.as_ptr() as *const _, own_memory.len() * 8)?;
        upload(blocks.logic_ops as *mut _, own_logic.as_ptr() as *const _, own_logic.len() * 4)?;
        let mut err = std::ptr::null_mut();
        let rc = unsafe {
            zkm_sha_calls_witness(ctx, self.extend_w16.as_ptr(), self.extend_meta.as_ptr(), ne, self.compress_hx.as_ptr(), self.compress_w.as_ptr(),
                                  self.compress_meta.as_ptr(), nc, blocks.raw_rows.add(own_raw * CPU_COLS), blocks.memory_ops.add(own_memory.len()),
                                  blocks.logic_ops.add(own_logic.len()), blocks.sha_extend_inputs, blocks.sha_extend_timestamps, &mut err)
        };
        check(rc, err)?;
        Ok(blocks)
    }
}
