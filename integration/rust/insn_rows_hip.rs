//! insn_rows_hip.rs -- the rows of the thirteen instructions `decode` accepts (witness/transition.rs:42-312) and no step kind takes,
//! expanded by libzkmhip.so (include/zkm_hip.h "the instructions the step kinds refuse, as rows") instead of on the host: LUI
//! (`generate_lui`, witness/operation.rs:405-433), MUL MFHI MTHI MFLO MTLO (`generate_binary_arithmetic_op`, :286-318), MULT MULTU DIV
//! DIVU (`generate_binary_arithmetic_hilo_op`, :320-375), SDC1 (`generate_mstore_general`, :1804-1928), SYNC and PREF (`generate_nop`).
//! The generators keep updating the registers and the memory, but push neither their 259-word row nor its arithmetic operation: the
//! recorder logs 48 bytes and a clock and reserves the row's position in the step list.  `finish` has the library write the rows and the
//! arithmetic operations on the device; the rows' memory operations are pushed by their RAW steps, as for any RAW row.
//!
//! How a maintainer hooks it in, on top of cpu_steps_hip.rs:
//!   * `GenerationState` gets an `insn_log: InsnRowLog` beside its `step_log: StepLog`;
//!   * `perform_op` (witness/transition.rs), before it asks `step_log.push`, asks `insn_kind(insn)`; for `Some(kind)` it runs the
//!     generator for its state changes alone and calls, in place of pushing the row (clock: `state.traces.clock()`),
//!       `insn_log.record(&mut state.step_log, clock, kind, &registers, insn)`
//!     which returns false, and records nothing, for a record the library refuses (a division `result()` would panic on): that row is
//!     filled on the host and goes `step_log.push_raw(&row)` as today;
//!   * at the end of the segment `insn_log.finish(ctx, &mut state.step_log)` expands the records into device memory behind the
//!     segment's own RAW rows and patches the reserved steps; the segment is then proven with `prove_segments_ops_steps_raw`, its
//!     `zkm_cpu_steps.raw_rows` pointing at `blocks.raw_rows` and its `zkm_segment_ops.arithmetic_ops` at `blocks.arithmetic_ops`.
//! With this every instruction `decode` accepts has a device path: RAW rows remain for the bootstrap rows a caller hands over and for
//! registers written outside an instruction.  A segment that also has precompile or I/O calls does not compose the
//! expansions itself: it hands this log and the calls' logs to `calls_hip.rs` (`SegmentCalls`, `prove_segments_ops_calls_raw`:
//! zkm_prove_segments_ops_calls), and the library places the records and orders the rows -- the own rows, then the SHA calls', the
//! Keccak calls', the I/O calls', then these -- and puts the arithmetic operations `Traces` still hold in front of the generated ones,
//! for K segments in one set of launches.  `finish` below is the segment without calls and without own operations.
//!
//! Goes into the zkm-prover crate as `prover/src/insn_rows_hip.rs`, beside `cpu_steps_hip.rs`.  NOT COMPILED in the build image (no
//! cargo / rustc there).
use anyhow::{ensure, Result};
use plonky2::hip::sys::*;

use crate::cpu_steps_hip::StepLog;
use crate::witness::state::RegistersState;

const CPU_COLS: usize = 259;

/// The ZKM_INSN_* kind of an instruction word, by the (opcode, func) pairs `decode` matches; None: a step kind takes it, or nothing does.
pub fn insn_kind(insn: u32) -> Option<u32> {
    Some(match (insn >> 26, insn & 0x3F) {
        (0b001111, _) => ZKM_INSN_LUI,
        (0b011100, 0b000010) => ZKM_INSN_MUL,
        (0b000000, 0b011000) => ZKM_INSN_MULT,
        (0b000000, 0b011001) => ZKM_INSN_MULTU,
        (0b000000, 0b011010) => ZKM_INSN_DIV,
        (0b000000, 0b011011) => ZKM_INSN_DIVU,
        (0b000000, 0b010000) => ZKM_INSN_MFHI,
        (0b000000, 0b010001) => ZKM_INSN_MTHI,
        (0b000000, 0b010010) => ZKM_INSN_MFLO,
        (0b000000, 0b010011) => ZKM_INSN_MTLO,
        (0b111101, _) => ZKM_INSN_SDC1,
        (0b000000, 0b001111) => ZKM_INSN_SYNC,
        (0b110011, _) => ZKM_INSN_PREF,
        _ => return None,
    })
}

/// The instruction records of one segment: the two lists of zkm_insn_rows_*, and the first clock.
#[derive(Default)]
pub struct InsnRowLog {
    pub insns: Vec<zkm_cpu_step>, // one record an instruction: pc, next_pc, insn, ZKM_INSN_*, the kernel flag, context, the values read
    pub clocks: Vec<u64>,         // the clock of each record's row
    first_clock: Option<u64>,     // the clock of step 0 of the step list (the bootstrap's row count)
}

/// Device memory `finish` filled.  Freed with zkm_dev_free.
pub struct InsnRowBlocks {
    pub raw_rows: *mut u64,       // own rows in front, generated rows behind
    pub nraw: usize,
    pub arithmetic_ops: *mut u32, // the generated operations, {row filter, in0, in1}; null when there is none
    pub narithmetic: usize,
    pub memory_ops: usize,        // the operations the generated rows' RAW steps push (for sizing the Memory table)
}

impl InsnRowLog {
    /// One instruction, in place of pushing its row.  `registers`: the state BEFORE the step; the values read are the ones `step_log`
    /// collected since the last step.  Whether the library takes the record is the library's statement: it is asked for this record
    /// alone, and a record it refuses (false: nothing recorded, nothing reserved) stays on the host.
    pub fn record(&mut self, steps: &mut StepLog, clock: u64, kind: u32, registers: &RegistersState, insn: u32) -> bool {
        let record = zkm_cpu_step {
            pc: registers.program_counter as u32, next_pc: registers.next_pc as u32, insn, kind,
            flags: if registers.is_kernel { ZKM_STEP_FLAG_KERNEL } else { 0 }, context: registers.context as u32, reads: steps.take_reads(),
        };
        let mut err = std::ptr::null_mut();
        let rc = unsafe { zkm_insn_rows_counts(&record, 1, std::ptr::null_mut(), std::ptr::null_mut(), &mut err) };
        if check(rc, err).is_err() || clock >> 32 != 0 {
            return false;
        }
        // the step at position i of the list is the row of clock first_clock + i: the row takes the next position
        let first = *self.first_clock.get_or_insert(clock - steps.steps.len() as u64);
        debug_assert_eq!(first + steps.steps.len() as u64, clock);
        self.insns.push(record);
        self.clocks.push(clock);
        steps.steps.push(zkm_cpu_step { kind: ZKM_STEP_RAW, ..Default::default() });
        true
    }

    /// Expand the records on the device and patch the reserved steps.  The own RAW rows are `steps.raw_rows`; the returned block holds
    /// own + generated, and `steps.list()` must then be given `raw_rows = blocks.raw_rows, nraw = blocks.nraw`.
    pub fn finish(&self, ctx: *mut zkm_ctx, steps: &mut StepLog) -> Result<InsnRowBlocks> {
        let n = self.insns.len();
        let (mut mem, mut arith) = (0usize, 0usize);
        let mut err = std::ptr::null_mut();
        check(unsafe { zkm_insn_rows_counts(self.insns.as_ptr(), n, &mut mem, &mut arith, &mut err) }, err)?;
        let own_raw = steps.raw_rows.len() / CPU_COLS;
        // the one statement of masks: the RAW records, record k for the position clocks[k] - first_clock
        let mut records = vec![zkm_cpu_step::default(); n];
        let mut err = std::ptr::null_mut();
        check(unsafe { zkm_insn_rows_steps(self.insns.as_ptr(), n, own_raw, records.as_mut_ptr(), &mut err) }, err)?;
        let first = self.first_clock.unwrap_or(0);
        for (record, clock) in records.iter().zip(&self.clocks) {
            let at = (clock - first) as usize;
            ensure!(at < steps.steps.len() && steps.steps[at].kind == ZKM_STEP_RAW, "no step was reserved at clock {}", clock);
            steps.steps[at] = *record;
        }
        let (mut rows, mut ops, mut err) = (std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut());
        check(unsafe { zkm_dev_alloc(ctx, ((own_raw + n) * CPU_COLS * 8).max(8), &mut rows, &mut err) }, err)?;
        if arith != 0 {
            let mut err = std::ptr::null_mut();
            check(unsafe { zkm_dev_alloc(ctx, arith * 12, &mut ops, &mut err) }, err)?;
        }
        let blocks = InsnRowBlocks { raw_rows: rows as *mut u64, nraw: own_raw + n, arithmetic_ops: ops as *mut u32, narithmetic: arith, memory_ops: mem };
        if !steps.raw_rows.is_empty() {
            let mut err = std::ptr::null_mut();
            check(unsafe { zkm_dev_upload(ctx, blocks.raw_rows as *mut _, steps.raw_rows.as_ptr() as *const _, steps.raw_rows.len() * 8, &mut err) }, err)?;
        }
        let mut err = std::ptr::null_mut();
        let rc = unsafe {
            zkm_insn_rows_witness(ctx, self.insns.as_ptr(), self.clocks.as_ptr(), n, blocks.raw_rows.add(own_raw * CPU_COLS), blocks.arithmetic_ops, &mut err)
        };
        check(rc, err)?;
        Ok(blocks)
    }
}
