//! io_calls_hip.rs -- the rows of a segment's I/O syscalls expanded by libzkmhip.so (include/zkm_hip.h "the I/O syscalls' rows from their
//! bytes") instead of on the host.  The four data-moving helpers that `generate_syscall` calls behind its own row
//! (witness/operation.rs:1660-1673) -- `load_preimage` (:908-989), `load_input` (:1024-1067), `verify` (:991-1022), `commit` (:1069-1099)
//! -- keep reading and writing the emulator's memory, the input stream, the public values stream and the assumptions, but push neither
//! their CPU rows (eight words a row: 32,768 rows for 1 MiB of input) nor the rows' memory operations: each records the call -- its kind,
//! the bytes it moves and four words of meta -- and reserves the call's positions in the step list.  `finish` has the library write the
//! rows on the device; the memory operations are pushed by the rows' RAW steps, as for any RAW row.
//!
//! How a maintainer hooks it in, on top of cpu_steps_hip.rs:
//!   * `GenerationState` gets an `io_log: IoCallLog` beside its `step_log: StepLog`;
//!   * the helpers call, in place of their row and trace pushes (clock: `state.traces.clock()` on entry, the clock after the SYSCALL row):
//!       load_input     `io_log.record_hint_read(&mut step_log, clock, addr, &vec)`
//!       commit         `io_log.record_commit(&mut step_log, clock, addr, &words)`     (the memory words read, as big-endian bytes)
//!       verify         `io_log.record_verify(&mut step_log, clock, addr, &claim_digest)`
//!       load_preimage  `io_log.record_preimage(&mut step_log, clock, &hash_bytes, &content)`
//!   * at the end of the segment `finish` expands the calls into device memory behind the segment's own RAW rows and patches the reserved
//!     steps; the segment is then proven with `prove_segments_ops_steps_raw`, its `zkm_cpu_steps.raw_rows` pointing at the block `finish`
//!     returns.
//! The SYSCALL row in front of a call is logged as today.  A segment that also has calls of another kind does not
//! compose the expansions itself: it hands this log and the others to `calls_hip.rs` (`SegmentCalls`, `prove_segments_ops_calls_raw`:
//! zkm_prove_segments_ops_calls), and the library places the records and orders the rows -- the own rows, then the SHA calls', the
//! Keccak calls', the I/O calls' -- for K segments in one set of launches; `finish` below is the segment whose only calls are I/O calls.
//!
//! Goes into the zkm-prover crate as `prover/src/io_calls_hip.rs`, beside `cpu_steps_hip.rs`.  NOT COMPILED in the build image (no
//! cargo / rustc there).
use anyhow::{ensure, Result};
use plonky2::hip::sys::*;

use crate::cpu_steps_hip::StepLog;

const CPU_COLS: usize = 259;
const PREIMAGE_MAP: u64 = 0x31000000; // where load_preimage writes the length and the content

/// The I/O calls of one segment: the four lists of zkm_io_calls_*, and the first clock.
pub struct IoCallLog {
    pub kinds: Vec<u32>,      // ZKM_IO_* of each call
    pub data: Vec<u8>,        // the calls' bytes, concatenated
    pub data_off: Vec<u64>,   // ncalls + 1 offsets into `data`
    pub meta: Vec<u64>,       // 4 words a call: context, segment, address, the first row's timestamp
    first_clock: Option<u64>, // the clock of step 0 of the step list (the bootstrap's row count)
}

impl Default for IoCallLog {
    fn default() -> Self {
        IoCallLog { kinds: Vec::new(), data: Vec::new(), data_off: vec![0], meta: Vec::new(), first_clock: None }
    }
}

/// Device memory `finish` filled: own rows in front, generated rows behind.  Freed with zkm_dev_free.
pub struct IoCallBlocks {
    pub raw_rows: *mut u64,
    pub nraw: usize,
    pub memory_ops: usize, // the operations the generated rows' RAW steps push (for sizing the Memory table)
}

impl IoCallLog {
    pub fn ncalls(&self) -> usize {
        self.kinds.len()
    }

    /// One call: context 0, Segment::Code (0).  How many rows it takes is the library's statement: it is asked for this call alone,
    /// and a call it refuses (false: nothing recorded) stays on the host.
    fn record(&mut self, steps: &mut StepLog, clock: u64, kind: u32, addr: u64, parts: &[&[u8]]) -> bool {
        let len: usize = parts.iter().map(|p| p.len()).sum();
        let off = [0u64, len as u64];
        let mut rows = 0usize;
        let mut err = std::ptr::null_mut();
        let rc = unsafe { zkm_io_calls_counts(&kind, off.as_ptr(), 1, &mut rows, std::ptr::null_mut(), &mut err) };
        if check(rc, err).is_err() {
            return false;
        }
        self.kinds.push(kind);
        for p in parts {
            self.data.extend_from_slice(p);
        }
        self.data_off.push(self.data.len() as u64);
        self.meta.extend_from_slice(&[0, 0, addr, clock * 10]);
        // the step at position i of the list is the row of clock first_clock + i: the call's rows take the next `rows` positions
        let first = *self.first_clock.get_or_insert(clock - steps.steps.len() as u64);
        debug_assert_eq!(first + steps.steps.len() as u64, clock);
        steps.steps.extend((0..rows).map(|_| zkm_cpu_step { kind: ZKM_STEP_RAW, ..Default::default() }));
        true
    }

    /// SYSHINTREAD: `vec` (the next vector of the input stream, any length) is written from `addr` on.
    pub fn record_hint_read(&mut self, steps: &mut StepLog, clock: u64, addr: usize, vec: &[u8]) -> bool {
        self.record(steps, clock, ZKM_IO_HINT_READ, addr as u64, &[vec])
    }

    /// SYSWRITE to FD_PUBLIC_VALUES: `words` are the ceil(size / 4) memory words read from `addr` on, each as its big-endian bytes.
    pub fn record_commit(&mut self, steps: &mut StepLog, clock: u64, addr: usize, words: &[u8]) -> bool {
        self.record(steps, clock, ZKM_IO_COMMIT, addr as u64, &[words])
    }

    /// SYSVERIFY: the 32 bytes of the claim digest read from `addr` on.
    pub fn record_verify(&mut self, steps: &mut StepLog, clock: u64, addr: usize, claim_digest: &[u8; 32]) -> bool {
        self.record(steps, clock, ZKM_IO_VERIFY, addr as u64, &[&claim_digest[..]])
    }

    /// SYSGETPID: the 32 hash bytes read at 0x30001000 and the file's content, written from 0x31000000 on behind its length.
    pub fn record_preimage(&mut self, steps: &mut StepLog, clock: u64, hash_bytes: &[u8; 32], content: &[u8]) -> bool {
        self.record(steps, clock, ZKM_IO_PREIMAGE, PREIMAGE_MAP, &[&hash_bytes[..], content])
    }

    /// Expand the calls on the device and patch the reserved steps.  The own RAW rows are `steps.raw_rows`; the returned block holds
    /// own + generated, and `steps.list()` must then be given `raw_rows = blocks.raw_rows, nraw = blocks.nraw`.
    pub fn finish(&self, ctx: *mut zkm_ctx, steps: &mut StepLog) -> Result<IoCallBlocks> {
        let n = self.ncalls();
        let (mut rows, mut mem) = (0usize, 0usize);
        let mut err = std::ptr::null_mut();
        check(unsafe { zkm_io_calls_counts(self.kinds.as_ptr(), self.data_off.as_ptr(), n, &mut rows, &mut mem, &mut err) }, err)?;
        let own_raw = steps.raw_rows.len() / CPU_COLS;
        // the one statement of masks and positions: the records and the clock each belongs at
        let mut records = vec![zkm_cpu_step::default(); rows];
        let mut clocks = vec![0u64; rows];
        let mut err = std::ptr::null_mut();
        let rc = unsafe {
            zkm_io_calls_steps(self.kinds.as_ptr(), self.data_off.as_ptr(), self.meta.as_ptr(), n, own_raw, records.as_mut_ptr(), clocks.as_mut_ptr(),
                               &mut err)
        };
        check(rc, err)?;
        let first = self.first_clock.unwrap_or(0);
        for (record, clock) in records.iter().zip(&clocks) {
            let at = (clock - first) as usize;
            ensure!(at < steps.steps.len() && steps.steps[at].kind == ZKM_STEP_RAW, "no step was reserved at clock {}", clock);
            steps.steps[at] = *record;
        }
        let (mut p, mut err) = (std::ptr::null_mut(), std::ptr::null_mut());
        check(unsafe { zkm_dev_alloc(ctx, ((own_raw + rows) * CPU_COLS * 8).max(8), &mut p, &mut err) }, err)?;
        let blocks = IoCallBlocks { raw_rows: p as *mut u64, nraw: own_raw + rows, memory_ops: mem };
        if !steps.raw_rows.is_empty() {
            let mut err = std::ptr::null_mut();
            check(unsafe { zkm_dev_upload(ctx, blocks.raw_rows as *mut _, steps.raw_rows.as_ptr() as *const _, steps.raw_rows.len() * 8, &mut err) }, err)?;
        }
        let mut err = std::ptr::null_mut();
        let rc = unsafe {
            zkm_io_calls_witness(ctx, self.kinds.as_ptr(), self.data.as_ptr(), self.data_off.as_ptr(), self.meta.as_ptr(), n,
                                 blocks.raw_rows.add(own_raw * CPU_COLS), &mut err)
        };
        check(rc, err)?;
        Ok(blocks)
    }
}
