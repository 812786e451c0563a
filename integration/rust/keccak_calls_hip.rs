//! keccak_calls_hip.rs -- the SYSKECCAK precompile calls of a segment expanded by libzkmhip.so (include/zkm_hip.h "SYSKECCAK precompile
//! calls from their input bytes") instead of on the host.  `generate_keccak` (witness/operation.rs:1101-1181) keeps reading the input from
//! and writing the digest to the emulator's memory, but pushes neither its CPU rows (ceil(words / 8) + 2 a call) nor, through
//! `keccak_sponge_log` (witness/util.rs:471-557), the sponge's memory reads, the XORs and the Keccak-f inputs: it records the call -- its
//! input bytes and four words of meta, the lists the KeccakSponge table needs anyway, and the digest's address -- and reserves the call's
//! positions in the step list.  `finish` has the library write everything else on the device.
//!
//! How a maintainer hooks it in, on top of cpu_steps_hip.rs:
//!   * `GenerationState` gets a `keccak_log: KeccakCallLog` beside its `step_log: StepLog`;
//!   * `generate_keccak(state, addr, len, ptr)` reads the input words from memory and writes the digest as today and calls
//!     `keccak_log.record_keccak(&mut step_log, clock, addr, &input, ptr)` in place of its row and trace pushes (clock: the clock of the
//!     first row the call would have pushed; input: the `len` bytes, `keccak_value_byte_be`).  For a length that is not a multiple of
//!     4 it calls `record_keccak_tail` with one more argument, the last memory word its loop read: the only provable value of that word
//!     is the padded message's (the remaining input bytes, 0x01, zeros, 0x80 in the fourth byte of a block's last word -- what the
//!     guest runtime writes, runtime/precompiles/src/io.rs:128-144, and what the sponge's reads carry, witness/util.rs:513-535), and if
//!     the word read is that one the call is recorded with ZKM_SPONGE_PADDED_TAIL.  Either function returns false for a call the
//!     library would refuse (an empty input; a last word that is not the padded one): the generator then pushes its rows and lists
//!     as today -- the KeccakSponge operation it pushes is packed by segment_hip.rs with ZKM_SPONGE_BYTE_ADDRESSED;
//!   * at the end of the segment `finish` expands the calls into device memory and patches the reserved steps; the segment is then
//!     proven with `prove_segments_ops_steps_raw`, its `zkm_cpu_steps.raw_rows` and the memory / logic / Keccak lists of its
//!     `zkm_segment_ops` pointing at the device blocks `finish` returns, and `keccak_sponge_*` at the log's own three lists (with the
//!     operations segment_hip.rs packed for the calls that were not recorded, if any, appended by the caller).
//! The SYSCALL row in front of a call is logged as today.  A segment that also has calls of another kind does not
//! compose the expansions itself: it hands this log and the others to `calls_hip.rs` (`SegmentCalls`, `prove_segments_ops_calls_raw`:
//! zkm_prove_segments_ops_calls), and the library places the records and orders every list -- the own items, then the SHA calls', then
//! the Keccak calls' -- for K segments in one set of launches; `finish` below is the Keccak-only segment.
//!
//! Goes into the zkm-prover crate as `prover/src/keccak_calls_hip.rs`, beside `cpu_steps_hip.rs`.  NOT COMPILED in the build image (no
//! cargo / rustc there).
use anyhow::{ensure, Result};
use plonky2::hip::sys::*;

use crate::cpu_steps_hip::StepLog;

const CPU_COLS: usize = 259;

/// The Keccak calls of one segment: the lists of zkm_segment_ops' KeccakSponge group, the digests' addresses, and the first clock.
pub struct KeccakCallLog {
    pub inputs: Vec<u8>,        // the calls' input bytes, concatenated
    pub input_off: Vec<u64>,    // ncalls + 1 offsets into `inputs`
    pub meta: Vec<u64>,         // 4 words a call: context, segment, address of word 0 | ZKM_SPONGE_BYTE_ADDRESSED (| ZKM_SPONGE_PADDED_TAIL), the sponge row's timestamp
    pub digest_addrs: Vec<u64>, // the address a call's digest is written to
    first_clock: Option<u64>,   // the clock of step 0 of the step list (the bootstrap's row count)
}

impl Default for KeccakCallLog {
    fn default() -> Self {
        KeccakCallLog { inputs: Vec::new(), input_off: vec![0], meta: Vec::new(), digest_addrs: Vec::new(), first_clock: None }
    }
}

/// Device memory `finish` filled: own items in front, generated items behind.  Freed with zkm_dev_free.
pub struct KeccakCallBlocks {
    pub raw_rows: *mut u64,
    pub nraw: usize,
    pub memory_ops: *mut u64,
    pub nmemory: usize,
    pub logic_ops: *mut u32,
    pub nlogic: usize,
    pub keccak_inputs: *mut u64,
    pub keccak_timestamps: *mut u64,
    pub nkeccak: usize,
}

/// The last memory word of a call whose length is no multiple of 4, as the padded message has it: the input's last len % 4 bytes,
/// 0x01, zeros, and 0x80 in the fourth byte when the word is the last of a 136-byte block (0x81 there when len % 136 == 135).
pub fn padded_tail_word(input: &[u8]) -> u32 {
    let rem = &input[input.len() / 4 * 4..];
    let mut bytes = [0u8; 4];
    bytes[..rem.len()].copy_from_slice(rem);
    bytes[rem.len()] = 0x01;
    if input.len() % 136 + 4 > 136 {
        bytes[3] |= 0x80;
    }
    u32::from_be_bytes(bytes)
}

/// What a call of `len` input bytes costs the link host-expanded, in bytes: its CPU rows, the sponge's reads (48 a byte), the XORs and
/// the Keccak-f inputs with their timestamps -- against `len` + 48 recorded (an offset, four meta words, the digest's address).
pub fn call_bytes(len: usize) -> usize {
    let (words, blocks) = ((len + 3) / 4, len / 136 + 1);
    ((words + 7) / 8 + 2) * CPU_COLS * 8 + len * 48 + 34 * blocks * 12 + blocks * 208
}

impl KeccakCallLog {
    pub fn ncalls(&self) -> usize {
        self.digest_addrs.len()
    }

    /// A SYSKECCAK call: context 0, Segment::Code (0), `input` = the bytes read from `addr` on, the digest written to `ptr`.  `clock`:
    /// state.traces.clock() at the call.  false (nothing recorded): the length is 0 or not a multiple of 4 (such a call is recorded
    /// with `record_keccak_tail`), the call stays on the host.
    pub fn record_keccak(&mut self, steps: &mut StepLog, clock: u64, addr: usize, input: &[u8], ptr: usize) -> bool {
        input.len() % 4 == 0 && self.record(steps, clock, addr, input, ptr, 0)
    }

    /// The same for a call of any length: `last_word` is the memory word generate_keccak read last (the one that holds the input's last
    /// byte).  For a length that is no multiple of 4 the call is recorded, flagged, iff that word is the padded message's; for a
    /// multiple of 4 the word is all input and nothing is asked of it.
    pub fn record_keccak_tail(&mut self, steps: &mut StepLog, clock: u64, addr: usize, input: &[u8], ptr: usize, last_word: u32) -> bool {
        if input.len() % 4 == 0 {
            return self.record(steps, clock, addr, input, ptr, 0);
        }
        last_word == padded_tail_word(input) && self.record(steps, clock, addr, input, ptr, ZKM_SPONGE_PADDED_TAIL)
    }

    fn record(&mut self, steps: &mut StepLog, clock: u64, addr: usize, input: &[u8], ptr: usize, tail: u64) -> bool {
        if input.is_empty() {
            return false;
        }
        // how many read rows stand in front of the sponge row is the library's statement: ask it for this call's clocks
        let off = [0u64, input.len() as u64];
        let flags = [0u64, 0, tail, 0];
        let mut rows = 0usize;
        let mut err = std::ptr::null_mut();
        let null = std::ptr::null_mut();
        let rc = unsafe {
            if tail == 0 {
                zkm_keccak_calls_counts(off.as_ptr(), 1, &mut rows, null, null, null, &mut err)
            } else {
                zkm_keccak_calls_counts_meta(off.as_ptr(), flags.as_ptr(), 1, &mut rows, null, null, null, &mut err)
            }
        };
        if check(rc, err).is_err() {
            return false;
        }
        let read_rows = (rows - 2) as u64;               // the sponge row and the write row close the call
        self.inputs.extend_from_slice(input);
        self.input_off.push(self.inputs.len() as u64);
        self.meta.extend_from_slice(&[0, 0, addr as u64 | ZKM_SPONGE_BYTE_ADDRESSED | tail, (clock + read_rows) * 10]);
        self.digest_addrs.push(ptr as u64);
        // the step at position i of the list is the row of clock first_clock + i: the call's rows take the next `rows` positions
        let first = *self.first_clock.get_or_insert(clock - steps.steps.len() as u64);
        debug_assert_eq!(first + steps.steps.len() as u64, clock);
        steps.steps.extend((0..rows).map(|_| zkm_cpu_step { kind: ZKM_STEP_RAW, ..Default::default() }));
        true
    }

    /// Expand the calls on the device and patch the reserved steps.  `own_memory` / `own_logic`: the operations left in Traces (6 words /
    /// 3 words each), which go in front of the generated ones; the own RAW rows are `steps.raw_rows`; the Keccak-f inputs left in Traces
    /// (the calls that stayed on the host) are appended by the caller to a copy of the returned lists if there are any.  The returned
    /// blocks hold own + generated; `steps.list()` must then be given `raw_rows = blocks.raw_rows, nraw = blocks.nraw`.
    pub fn finish(&self, ctx: *mut zkm_ctx, steps: &mut StepLog, own_memory: &[u64], own_logic: &[u32]) -> Result<KeccakCallBlocks> {
        let n = self.ncalls();
        let (mut rows, mut mem, mut logic, mut perms) = (0usize, 0usize, 0usize, 0usize);
        let mut err = std::ptr::null_mut();
        check(unsafe { zkm_keccak_calls_counts_meta(self.input_off.as_ptr(), self.meta.as_ptr(), n, &mut rows, &mut mem, &mut logic, &mut perms, &mut err) }, err)?;
        let own_raw = steps.raw_rows.len() / CPU_COLS;
        // the one statement of masks and positions: the records and the clock each belongs at
        let mut records = vec![zkm_cpu_step::default(); rows];
        let mut clocks = vec![0u64; rows];
        let mut err = std::ptr::null_mut();
        let rc = unsafe {
            zkm_keccak_calls_steps(self.input_off.as_ptr(), self.meta.as_ptr(), n, own_raw, records.as_mut_ptr(), clocks.as_mut_ptr(), &mut err)
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
        let blocks = KeccakCallBlocks {
            raw_rows: alloc((own_raw + rows) * CPU_COLS * 8)? as *mut u64,
            nraw: own_raw + rows,
            memory_ops: alloc((own_memory.len() + 6 * mem) * 8)? as *mut u64,
            nmemory: own_memory.len() / 6 + mem,
            logic_ops: alloc((own_logic.len() + 3 * logic) * 4)? as *mut u32,
            nlogic: own_logic.len() / 3 + logic,
            keccak_inputs: alloc(200 * perms)? as *mut u64,
            keccak_timestamps: alloc(8 * perms)? as *mut u64,
            nkeccak: perms,
        };
        upload(blocks.raw_rows as *mut _, steps.raw_rows.as_ptr() as *const _, steps.raw_rows.len() * 8)?;
        upload(blocks.memory_ops as *mut _, own_memory.as_ptr() as *const _, own_memory.len() * 8)?;
        upload(blocks.logic_ops as *mut _, own_logic.as_ptr() as *const _, own_logic.len() * 4)?;
        let mut err = std::ptr::null_mut();
        let rc = unsafe {
            zkm_keccak_calls_witness(ctx, self.inputs.as_ptr(), self.input_off.as_ptr(), self.meta.as_ptr(), self.digest_addrs.as_ptr(), n,
                                     blocks.raw_rows.add(own_raw * CPU_COLS), blocks.memory_ops.add(own_memory.len()),
                                     blocks.logic_ops.add(own_logic.len()), blocks.keccak_inputs, blocks.keccak_timestamps, &mut err)
        };
        check(rc, err)?;
        Ok(blocks)
    }
}
