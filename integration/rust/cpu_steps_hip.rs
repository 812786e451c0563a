//! cpu_steps_hip.rs -- a segment's CPU rows built by libzkmhip.so from a compact step log (include/zkm_hip.h "a segment's CPU table
//! from a compact step log") instead of on the host.  The emulator's fetch, decode and execute stay where they are: `transition`
//! (witness/transition.rs) still decodes the instruction and the `generate_*` functions of witness/operation.rs still update the
//! registers and the memory -- but instead of filling a 259-word `CpuColumnsView` and pushing memory, logic and arithmetic operations
//! into `Traces`, they log 48 bytes: the row's pc / next_pc, the instruction word, the kind and the values they read through the memory
//! channels.  The library derives the row, its channels and every operation the row pushes on the device, in the reference's push order.
//!
//! How a maintainer hooks it in:
//!   * `GenerationState` gets a `step_log: StepLog`;
//!   * `reg_read_with_log` / `mem_read_*_with_log` (witness/util.rs) call `step_log.read(value)` beside what they do today;
//!   * `perform_op` (witness/transition.rs), where it has decoded `op` from `insn`, calls `step_log.push(&registers, insn, &op, sys)`
//!     for a kind the library derives (`step_kind` says which) and skips the row filling; for every other operation -- keccak_general,
//!     the precompiles of operation.rs:1101-1458, get / set context -- it fills the row as today and calls `step_log.push_raw(&row)`;
//!   * the padding loop of `simulate_cpu` (generation/mod.rs:170-185) calls `step_log.pad(..)` instead of pushing rows.
//! What the steps cover leaves `Traces::cpu`, and the memory / logic / arithmetic operations of those rows leave `Traces` too: the
//! library puts them in front of the lists that remain (the precompiles' own operations).  `StagedSteps` stages the next call's steps
//! behind the current proofs (the walk runs on the device); the pool takes a step log as a `SegmentCalls` without
//! calls (`calls_hip.rs` `prove_segments_calls_pool_hip`).
//!
//! Goes into the zkm-prover crate as `prover/src/cpu_steps_hip.rs`, beside `segment_hip.rs`.  The reference items used here are checked
//! by tests/test_rust_cpu_steps_names.py.  NOT COMPILED in the build image (no cargo / rustc there).
use anyhow::{ensure, Result};
use plonky2::field::types::PrimeField64;
use plonky2::hip::sys::*;

use crate::arithmetic::BinaryOperator;
use crate::cpu::columns::CpuColumnsView;
use crate::segment_hip::{size_then_prove, SegmentProofs};
use crate::witness::operation::{BranchCond, MovCond, Operation};
use crate::witness::state::RegistersState;

const CPU_COLS: usize = 259;
const CH0: usize = 205; // first cell of memory channel 0 (cpu/columns/mod.rs); a channel is {used, is_read, context, segment, virt, value}

/// The step list of one segment and the ready-made rows its RAW steps index.  `list()` is valid while `self` lives and is not pushed to.
#[derive(Default)]
pub struct StepLog {
    pub steps: Vec<zkm_cpu_step>,
    pub raw_rows: Vec<u64>,
    reads: [u32; 6],
    nreads: usize,
}

/// The kind of an operation the library derives, or None: such a row is filled on the host and handed over RAW.
pub fn step_kind(op: &Operation) -> Option<u32> {
    use BinaryOperator::*;
    Some(match op {
        Operation::BinaryArithmetic(ADD | ADDU | SUB | SUBU | SLT | SLTU, ..) => ZKM_STEP_BINARY_OP,
        Operation::BinaryArithmeticImm(ADDI | ADDIU | SLTI | SLTIU, ..) => ZKM_STEP_BINARY_IMM_OP,
        Operation::BinaryLogic(..) => ZKM_STEP_LOGIC_OP,
        Operation::BinaryLogicImm(..) => ZKM_STEP_LOGIC_IMM_OP,
        Operation::BinaryArithmetic(SLLV | SRLV | SRAV, ..) => ZKM_STEP_SHIFT,
        Operation::BinaryArithmetic(SLL | SRL | SRA, ..) => ZKM_STEP_SHIFT_IMM,
        Operation::Branch(..) => ZKM_STEP_BRANCH,
        Operation::Jump(..) => ZKM_STEP_JUMPS,
        Operation::Jumpi(..) => ZKM_STEP_JUMPI,
        Operation::JumpDirect(..) => ZKM_STEP_JUMPDIRECT,
        Operation::Nop => ZKM_STEP_NOP,
        Operation::Count(false, ..) => ZKM_STEP_CLZ_OP,
        Operation::Count(true, ..) => ZKM_STEP_CLO_OP,
        Operation::Signext(_, _, 8) => ZKM_STEP_SIGNEXT8,
        Operation::Signext(_, _, 16) => ZKM_STEP_SIGNEXT16,
        Operation::SwapHalf(..) => ZKM_STEP_SWAPHALF,
        Operation::Rdhwr(..) => ZKM_STEP_RDHWR,
        Operation::CondMov(MovCond::EQ, ..) => ZKM_STEP_MOVZ_OP,
        Operation::CondMov(MovCond::NE, ..) => ZKM_STEP_MOVN_OP,
        Operation::Teq(..) => ZKM_STEP_TEQ,
        Operation::Ext(..) => ZKM_STEP_EXT,
        Operation::Ins(..) => ZKM_STEP_INS,
        Operation::Ror(..) => ZKM_STEP_ROR,
        Operation::Maddu(..) => ZKM_STEP_MADDU,
        Operation::Syscall => ZKM_STEP_SYSCALL,
        // loads and stores: the sixteen memio selectors but SDC1, which has no step encoding
        Operation::MloadGeneral(..) => ZKM_STEP_M_OP_LOAD,
        Operation::MstoreGeneral(..) => ZKM_STEP_M_OP_STORE,
        _ => return None,
    })
}

impl StepLog {
    /// A value read through a memory channel (a register, then memory), in the order the generator reads.
    pub fn read(&mut self, value: u32) {
        self.reads[self.nreads] = value;
        self.nreads += 1;
    }

    /// The values read since the last step, handed to a recorder that logs the row elsewhere (insn_rows_hip.rs); the log starts afresh.
    pub fn take_reads(&mut self) -> [u32; 6] {
        self.nreads = 0;
        std::mem::take(&mut self.reads)
    }

    /// The step of an instruction the library derives.  `registers`: the state BEFORE the step (program_counter and next_pc are the
    /// row's).  `syscall`: ZKM_SYSCALL_* for a SYSCALL, 0 otherwise.  Returns false, and logs nothing, for an operation without a kind
    /// (or a word the kind does not take: a NOP that is not word 0, SDC1): the caller fills the row and calls push_raw.
    pub fn push(&mut self, registers: &RegistersState, insn: u32, op: &Operation, syscall: u32) -> bool {
        let reads = std::mem::take(&mut self.reads);
        self.nreads = 0;
        let kind = match step_kind(op) {
            Some(ZKM_STEP_NOP) if insn != 0 => return false,
            Some(ZKM_STEP_M_OP_STORE) if insn >> 26 == 0b111101 => return false,
            Some(kind) => kind,
            None => return false,
        };
        let mut flags = if registers.is_kernel { ZKM_STEP_FLAG_KERNEL } else { 0 } | syscall << 8;
        // decode hands BGEZ, BLTZ, BLEZ and BGTZ register 0 as their second source, whatever the rt field says
        if let Operation::Branch(BranchCond::GE | BranchCond::LT | BranchCond::LE | BranchCond::GT, ..) = op {
            flags |= ZKM_STEP_FLAG_BRANCH_R0;
        }
        self.steps.push(zkm_cpu_step {
            pc: registers.program_counter as u32, next_pc: registers.next_pc as u32, insn, kind, flags, context: registers.context as u32, reads,
        });
        true
    }

    /// A ready-made row: everything the kinds do not cover.  Its used channels become memory operations in ascending channel order;
    /// a row that pushes logic or arithmetic operations keeps pushing them into Traces.
    pub fn push_raw<F: PrimeField64>(&mut self, row: &CpuColumnsView<F>) {
        // CpuColumnsView is #[repr(C)] over F (cpu/columns/mod.rs:66): 259 field words
        let words = unsafe { std::slice::from_raw_parts(row as *const CpuColumnsView<F> as *const F, CPU_COLS) };
        let index = (self.raw_rows.len() / CPU_COLS) as u32;
        let mask = (0..8).filter(|k| words[CH0 + 6 * k].to_canonical_u64() != 0).fold(0u32, |m, k| m | 1 << k);
        self.raw_rows.extend(words.iter().map(|w| w.to_canonical_u64()));
        self.reads = [0; 6];
        self.nreads = 0;
        self.steps.push(zkm_cpu_step { kind: ZKM_STEP_RAW, reads: [index, mask, 0, 0, 0, 0], ..Default::default() });
    }

    /// The padding rows of simulate_cpu (generation/mod.rs:170-185): PAD steps until `rows_before + steps` is a power of two
    /// (rows_before: the bootstrap's rows, zkm_boot_counts).  At least one, as the reference's loop pushes.
    pub fn pad(&mut self, registers: &RegistersState, pc: usize, rows_before: usize) {
        loop {
            self.steps.push(zkm_cpu_step {
                pc: pc as u32, next_pc: registers.next_pc as u32, kind: ZKM_STEP_PAD, context: registers.context as u32, ..Default::default()
            });
            if (rows_before + self.steps.len()).is_power_of_two() {
                break;
            }
        }
    }

    pub fn list(&self) -> zkm_cpu_steps {
        zkm_cpu_steps { steps: self.steps.as_ptr(), nsteps: self.steps.len(), raw_rows: self.raw_rows.as_ptr(), nraw: self.raw_rows.len() / CPU_COLS }
    }

    /// The lengths of the Memory, Logic and Arithmetic lists the steps push (no GPU involved); refuses as the proving call would.
    pub fn counts(&self) -> Result<(usize, usize, usize)> {
        let (mut m, mut l, mut a, mut err) = (0usize, 0usize, 0usize, std::ptr::null_mut());
        let rc = unsafe { zkm_cpu_steps_counts(&self.list(), &mut m, &mut l, &mut a, &mut err) };
        check(rc, err)?;
        Ok((m, l, a))
    }
}

/// K x (bootstrap from the image, CPU rows from the steps, `into_tables`, `prove_with_traces`) in one call.  `segments[s]` holds what
/// is left of Traces (cpu_rows null, ncpu_rows 0); `images` may be empty (no bootstrap).  Results as `prove_segments_ops_hip`.
pub fn prove_segments_ops_steps_raw(ctx: *mut zkm_ctx, images: &[zkm_boot_image], steps: &[zkm_cpu_steps], segments: &[zkm_segment_ops],
                                    config: &zkm_stark_config, public_values: &[&[u64]]) -> Result<SegmentProofs> {
    ensure!(steps.len() == segments.len(), "{} step lists for {} segments", steps.len(), segments.len());
    ensure!(images.is_empty() || images.len() == segments.len(), "{} images for {} segments", images.len(), segments.len());
    ensure!(segments.iter().all(|s| s.cpu_rows.is_null() && s.ncpu_rows == 0), "the steps take the place of cpu_rows");
    let images_ptr = if images.is_empty() { std::ptr::null() } else { images.as_ptr() };
    size_then_prove(segments.len(), public_values, config.num_challenges as usize, |pv, npv, proofs, offs, chal, err| unsafe {
        zkm_prove_segments_ops_steps(ctx, config, segments.len(), images_ptr, steps.as_ptr(), segments.as_ptr(), pv, npv, proofs, offs, chal, err)
    })
}

/// The tables alone: one staged block per segment (zkm_staged_segment_ptrs / zkm_staged_free), heights in Table::all() order.
pub fn segments_tables_steps_raw(ctx: *mut zkm_ctx, images: &[zkm_boot_image], steps: &[zkm_cpu_steps], segments: &[zkm_segment_ops],
                                 config: &zkm_stark_config) -> Result<(Vec<*mut zkm_staged>, Vec<u32>)> {
    ensure!(steps.len() == segments.len() && (images.is_empty() || images.len() == segments.len()), "one step list (and image) per segment");
    let images_ptr = if images.is_empty() { std::ptr::null() } else { images.as_ptr() };
    let (mut handles, mut log_n, mut err) = (vec![std::ptr::null_mut(); segments.len()], vec![0u32; 12 * segments.len()], std::ptr::null_mut());
    let rc = unsafe {
        zkm_segments_tables_steps(ctx, config, segments.len(), images_ptr, steps.as_ptr(), segments.as_ptr(), log_n.as_mut_ptr(), handles.as_mut_ptr(), &mut err)
    };
    check(rc, err)?;
    Ok((handles, log_n))
}

/// K segments' step logs on their way into HBM behind the context's current work, walked on the device behind the upload
/// (zkm_cpu_steps_stage).  `stage` returns at once with no host wait; the lists it was given must stay as they are until `ready`
/// answers true.  `get` is what the `*_steps` calls of the SAME context take for a segment; drop the handle after those calls.
pub struct StagedSteps {
    handle: *mut std::ffi::c_void,
    nseg: usize,
}

impl StagedSteps {
    pub fn stage(ctx: *mut zkm_ctx, steps: &[zkm_cpu_steps]) -> Result<Self> {
        let (mut handle, mut err) = (std::ptr::null_mut(), std::ptr::null_mut());
        let rc = unsafe { zkm_cpu_steps_stage(ctx, steps.len(), steps.as_ptr(), &mut handle, &mut err) };
        check(rc, err)?;
        Ok(StagedSteps { handle, nseg: steps.len() })
    }

    /// True once the uploads, the walk and the download of its verdicts have ended; `wait` blocks until they have.
    pub fn ready(&self, wait: bool) -> Result<bool> {
        let r = unsafe { zkm_staged_steps_ready(self.handle, wait as std::ffi::c_int) };
        ensure!(r >= 0, "zkm_staged_steps_ready: runtime error");
        Ok(r == 1)
    }

    /// Segment `segment` with device pointers and the lengths of the Memory, Logic and Arithmetic lists its steps push; a segment the
    /// walk refused fails with the host walk's message.  One host wait a handle at most.
    pub fn get(&self, segment: usize) -> Result<(zkm_cpu_steps, (usize, usize, usize))> {
        let (mut m, mut l, mut a, mut err) = (0usize, 0usize, 0usize, std::ptr::null_mut());
        let mut steps = zkm_cpu_steps { steps: std::ptr::null(), nsteps: 0, raw_rows: std::ptr::null(), nraw: 0 };
        let rc = unsafe { zkm_staged_steps_get(self.handle, segment, &mut steps, &mut m, &mut l, &mut a, &mut err) };
        check(rc, err)?;
        Ok((steps, (m, l, a)))
    }

    /// Every segment of the handle, for the `*_steps` calls.
    pub fn lists(&self) -> Result<Vec<zkm_cpu_steps>> {
        (0..self.nseg).map(|s| self.get(s).map(|(steps, _)| steps)).collect()
    }
}

impl Drop for StagedSteps {
    fn drop(&mut self) {
        unsafe { zkm_staged_steps_free(self.handle) }
    }
}

/// `prove_segments_ops_steps_raw` on steps staged ahead of the call: no walk on the calling thread, no upload of records or bases.
pub fn prove_segments_ops_steps_staged(ctx: *mut zkm_ctx, images: &[zkm_boot_image], staged: &StagedSteps, segments: &[zkm_segment_ops],
                                       config: &zkm_stark_config, public_values: &[&[u64]]) -> Result<SegmentProofs> {
    prove_segments_ops_steps_raw(ctx, images, &staged.lists()?, segments, config, public_values)
}

/// `segments_tables_steps_raw` on steps staged ahead of the call.
pub fn segments_tables_steps_staged(ctx: *mut zkm_ctx, images: &[zkm_boot_image], staged: &StagedSteps, segments: &[zkm_segment_ops],
                                    config: &zkm_stark_config) -> Result<(Vec<*mut zkm_staged>, Vec<u32>)> {
    segments_tables_steps_raw(ctx, images, &staged.lists()?, segments, config)
}
