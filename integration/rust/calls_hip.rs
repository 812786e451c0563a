//! calls_hip.rs -- K segments' calls expanded by libzkmhip.so in ONE set of launches (include/zkm_hip.h "K segments' calls expanded in one
//! set of launches"), in front of the K-segment builder: the composition of the four recorders -- sha_calls_hip.rs, keccak_calls_hip.rs,
//! io_calls_hip.rs, insn_rows_hip.rs -- that a segment with several kinds needs.  Which RAW index a generated row gets, where its record
//! goes in the step list, the order inside every list (own items, then the SHA calls', the Keccak calls', the I/O calls', the
//! instructions') and which groups of `zkm_segment_ops` the calls set is the library's business: the caller hands over the logs as the
//! recorders filled them and never calls their `finish`.
//!
//! How a maintainer hooks it in, on top of the four recorders:
//!   * `GenerationState` keeps its `step_log: StepLog` and the four logs; the `record_*` calls stay where they are (each reserves its
//!     rows' positions in `step_log`);
//!   * at the end of a segment `SegmentCalls::new(&state.step_log, first_clock, own, &sha, &keccak, &io, &insns)` borrows them -- nothing
//!     is copied; `own` is what is left of `Traces` (cpu_rows null; the memory, logic and arithmetic operations and Keccak permutations
//!     the step kinds do not push; the SHA and Keccak sponge groups empty: the calls own them);
//!   * K of them go to `prove_segments_ops_calls_raw`, in place of K x four `finish` calls and `prove_segments_ops_steps_raw`: per 32
//!     segments the expansion takes one scratch block, at most one launch per kind and one host wait.
//! `segment_calls_steps` is the host half alone (the patched step list and the counts), for a caller that sizes its tables first.
//!   * a caller that records segment k + 1 while segment k is proven stages it instead: `StagedCalls::stage` queues the uploads, the
//!     expansions, the placement of the records and the walk behind the proofs in flight and returns at once;
//!     `prove_segments_ops_calls_staged` then proves from device memory with nothing read per row on the calling thread;
//!   * a caller with several GPUs hands all segments to `prove_segments_calls_pool_hip`: the pool's workers do that staging themselves.
//!
//! Goes into the zkm-prover crate as `prover/src/calls_hip.rs`, beside `cpu_steps_hip.rs`.  NOT COMPILED in the build image (no cargo /
//! rustc there).
use std::marker::PhantomData;
use std::os::raw::c_void;

use anyhow::{ensure, Result};
use plonky2::hip::sys::*;

use crate::cpu_steps_hip::StepLog;
use crate::insn_rows_hip::InsnRowLog;
use crate::io_calls_hip::IoCallLog;
use crate::keccak_calls_hip::KeccakCallLog;
use crate::segment_hip::{size_then_prove, SegmentProofs};
use crate::sha_calls_hip::ShaCallLog;

/// One segment as the recorders logged it: `struct zkm_segment_calls` over borrowed logs.
pub struct SegmentCalls<'a> {
    pub raw: ZkmSegmentCalls,
    logs: PhantomData<&'a StepLog>,
}

impl<'a> SegmentCalls<'a> {
    pub fn new(steps: &'a StepLog, first_clock: u64, own: zkm_segment_ops, sha: &'a ShaCallLog, keccak: &'a KeccakCallLog, io: &'a IoCallLog,
               insns: &'a InsnRowLog) -> Self {
        let raw = ZkmSegmentCalls {
            steps: steps.list(), first_clock, own,
            extend_w16: sha.extend_w16.as_ptr(), extend_meta: sha.extend_meta.as_ptr(), nextend: sha.nextend(),
            compress_hx: sha.compress_hx.as_ptr(), compress_w: sha.compress_w.as_ptr(), compress_meta: sha.compress_meta.as_ptr(), ncompress: sha.ncompress(),
            keccak_inputs: keccak.inputs.as_ptr(), keccak_input_off: keccak.input_off.as_ptr(), keccak_meta: keccak.meta.as_ptr(),
            keccak_digest_addrs: keccak.digest_addrs.as_ptr(), nkeccak: keccak.ncalls(),
            io_kinds: io.kinds.as_ptr(), io_data: io.data.as_ptr(), io_data_off: io.data_off.as_ptr(), io_meta: io.meta.as_ptr(), nio: io.ncalls(),
            insns: insns.insns.as_ptr(), insn_clocks: insns.clocks.as_ptr(), ninsns: insns.insns.len(),
        };
        SegmentCalls { raw, logs: PhantomData }
    }
}

/// What zkm_segment_calls_steps counts, in the header's order.
#[derive(Clone, Copy, Debug, Default)]
pub struct CallsCounts {
    pub sha_rows: usize, pub keccak_rows: usize, pub io_rows: usize, pub insn_rows: usize, pub nraw: usize, pub memory_ops: usize,
    pub logic_ops: usize, pub arithmetic_ops: usize, pub sha_extend_rows: usize, pub keccak_perms: usize, pub row_memory_ops: usize,
}

/// The host half alone: the patched step list (every call's RAW record at clock - first_clock) and the counts.  No GPU is involved;
/// every refusal of the lists is made here as the expansion would make it.
pub fn segment_calls_steps(calls: &SegmentCalls) -> Result<(Vec<zkm_cpu_step>, CallsCounts)> {
    let mut patched = vec![zkm_cpu_step::default(); calls.raw.steps.nsteps];
    let (mut n, mut err) = ([0usize; ZKM_CALLS_COUNTS], std::ptr::null_mut());
    let rc = unsafe { zkm_segment_calls_steps(&calls.raw as *const ZkmSegmentCalls as *const c_void, patched.as_mut_ptr(), n.as_mut_ptr(), &mut err) };
    check(rc, err)?;
    Ok((patched, CallsCounts { sha_rows: n[0], keccak_rows: n[1], io_rows: n[2], insn_rows: n[3], nraw: n[4], memory_ops: n[5], logic_ops: n[6],
                             arithmetic_ops: n[7], sha_extend_rows: n[8], keccak_perms: n[9], row_memory_ops: n[10] }))
}

fn raw_array(segments: &[SegmentCalls]) -> Vec<ZkmSegmentCalls> {
    segments.iter().map(|s| s.raw).collect()
}

/// K x (the calls' expansion, bootstrap from the image, CPU rows from the steps, `into_tables`, `prove_with_traces`) in one call:
/// zkm_prove_segments_ops_calls.  `images` may be empty (no bootstrap).  Results as `prove_segments_ops_steps_raw`, word for word what
/// that gives on the four recorders' `finish`ed blocks.
pub fn prove_segments_ops_calls_raw(ctx: *mut zkm_ctx, images: &[zkm_boot_image], segments: &[SegmentCalls], config: &zkm_stark_config,
                                    public_values: &[&[u64]]) -> Result<SegmentProofs> {
    ensure!(images.is_empty() || images.len() == segments.len(), "{} images for {} segments", images.len(), segments.len());
    let images_ptr = if images.is_empty() { std::ptr::null() } else { images.as_ptr() };
    let raw = raw_array(segments);
    size_then_prove(segments.len(), public_values, config.num_challenges as usize, |pv, npv, proofs, offs, chal, err| unsafe {
        zkm_prove_segments_ops_calls(ctx, config, raw.len(), images_ptr, raw.as_ptr() as *const c_void, pv, npv, proofs, offs, chal, err)
    })
}

/// All segments of a program over the pool's contexts, as the recorders logged them: the groups of `prove_segments_multi_hip`
/// (prove_hip.rs), each proven on its worker's context -- staged one group ahead of the proofs, or expanded in its call
/// (`zkm_pool_set_tuning(pool, "pool_stage_ahead", ..)`).  `pool` is the `*mut zkm_pool` of a `HipPool`; `images` may be empty.  A step
/// log without calls is a `SegmentCalls` over empty logs.  Results word for word those of `prove_segments_ops_calls_raw` on one context.
/// The logs must be host memory unless the pool has one device.
pub fn prove_segments_calls_pool_hip(pool: *mut zkm_pool, images: &[zkm_boot_image], segments: &[SegmentCalls], config: &zkm_stark_config,
                                     max_stack: usize, public_values: &[&[u64]]) -> Result<SegmentProofs> {
    ensure!(images.is_empty() || images.len() == segments.len(), "{} images for {} segments", images.len(), segments.len());
    let images_ptr = if images.is_empty() { std::ptr::null() } else { images.as_ptr() };
    let raw = raw_array(segments);
    size_then_prove(segments.len(), public_values, config.num_challenges as usize, |pv, npv, proofs, offs, chal, err| unsafe {
        zkm_pool_prove_segments_calls(pool, config, raw.len(), max_stack, images_ptr, raw.as_ptr() as *const c_void, pv, npv, proofs, offs, chal, err)
    })
}

/// The tables alone: zkm_segments_tables_calls.  One staged block per segment (zkm_staged_segment_ptrs / zkm_staged_free), heights in
/// Table::all() order.
pub fn segments_tables_calls_raw(ctx: *mut zkm_ctx, images: &[zkm_boot_image], segments: &[SegmentCalls], config: &zkm_stark_config)
                                 -> Result<(Vec<*mut zkm_staged>, Vec<u32>)> {
    ensure!(images.is_empty() || images.len() == segments.len(), "{} images for {} segments", images.len(), segments.len());
    let images_ptr = if images.is_empty() { std::ptr::null() } else { images.as_ptr() };
    let raw = raw_array(segments);
    let (mut handles, mut log_n, mut err) = (vec![std::ptr::null_mut(); raw.len()], vec![0u32; 12 * raw.len()], std::ptr::null_mut());
    let rc = unsafe {
        zkm_segments_tables_calls(ctx, config, raw.len(), images_ptr, raw.as_ptr() as *const c_void, log_n.as_mut_ptr(), handles.as_mut_ptr(), &mut err)
    };
    check(rc, err)?;
    Ok((handles, log_n))
}

/// The expansion alone, for a caller that keeps the expanded segments (to build tables and prove in separate calls): the handle owns the
/// patched step lists and the device blocks; `get(s)` is what zkm_segments_tables_steps / zkm_prove_segments_ops_steps take for segment
/// s.  The logs must outlive the handle: the sponge groups of `get`'s operations point into them.
pub struct ExpandedCalls<'a> {
    handle: *mut c_void,
    nseg: usize,
    logs: PhantomData<&'a StepLog>,
}

impl<'a> ExpandedCalls<'a> {
    pub fn expand(ctx: *mut zkm_ctx, segments: &[SegmentCalls<'a>]) -> Result<Self> {
        let raw = raw_array(segments);
        let (mut handle, mut err) = (std::ptr::null_mut(), std::ptr::null_mut());
        check(unsafe { zkm_segments_calls_expand(ctx, raw.len(), raw.as_ptr() as *const c_void, &mut handle, &mut err) }, err)?;
        Ok(ExpandedCalls { handle, nseg: raw.len(), logs: PhantomData })
    }

    pub fn get(&self, segment: usize) -> Result<(zkm_cpu_steps, zkm_segment_ops)> {
        ensure!(segment < self.nseg, "segment {} of {}", segment, self.nseg);
        let (mut steps, mut ops) = unsafe { (std::mem::zeroed::<zkm_cpu_steps>(), std::mem::zeroed::<zkm_segment_ops>()) };
        ensure!(unsafe { zkm_expanded_calls_get(self.handle, segment, &mut steps, &mut ops) } == 0, "zkm_expanded_calls_get refused segment {}", segment);
        Ok((steps, ops))
    }
}

impl Drop for ExpandedCalls<'_> {
    fn drop(&mut self) {
        unsafe { zkm_expanded_calls_free(self.handle) }
    }
}

/// K segments' calls on their way into HBM behind the context's current work (zkm_segments_calls_stage): expanded, their records placed
/// into the step list and the list walked on the device.  `stage` returns at once with no host wait; the logs (and the images' words)
/// must stay as they are until `ready` answers true.  `get` is what the `*_steps` calls of the SAME context take for a segment; drop
/// the handle after those calls.
pub struct StagedCalls<'a> {
    handle: *mut c_void,
    nseg: usize,
    with_images: bool,
    logs: PhantomData<&'a StepLog>,
}

impl<'a> StagedCalls<'a> {
    pub fn stage(ctx: *mut zkm_ctx, images: &[zkm_boot_image], segments: &[SegmentCalls<'a>]) -> Result<Self> {
        ensure!(images.is_empty() || images.len() == segments.len(), "{} images for {} segments", images.len(), segments.len());
        let images_ptr = if images.is_empty() { std::ptr::null() } else { images.as_ptr() };
        let raw = raw_array(segments);
        let (mut handle, mut err) = (std::ptr::null_mut(), std::ptr::null_mut());
        check(unsafe { zkm_segments_calls_stage(ctx, raw.len(), raw.as_ptr() as *const c_void, images_ptr, &mut handle, &mut err) }, err)?;
        Ok(StagedCalls { handle, nseg: raw.len(), with_images: !images.is_empty(), logs: PhantomData })
    }

    /// True once the uploads, the expansions, the placement, the walk and the downloads have ended; `wait` blocks until they have.
    pub fn ready(&self, wait: bool) -> Result<bool> {
        let r = unsafe { zkm_staged_calls_ready(self.handle, wait as std::os::raw::c_int) };
        ensure!(r >= 0, "zkm_staged_calls_ready: runtime error");
        Ok(r == 1)
    }

    /// Segment `segment` with device pointers; a refused segment fails with the refusal's text.  One host wait a handle at most.
    pub fn get(&self, segment: usize) -> Result<(zkm_cpu_steps, zkm_segment_ops, zkm_boot_image)> {
        let (mut steps, mut ops, mut image) =
            unsafe { (std::mem::zeroed::<zkm_cpu_steps>(), std::mem::zeroed::<zkm_segment_ops>(), std::mem::zeroed::<zkm_boot_image>()) };
        let mut err = std::ptr::null_mut();
        check(unsafe { zkm_staged_calls_get(self.handle, segment, &mut steps, &mut ops, &mut image, &mut err) }, err)?;
        Ok((steps, ops, image))
    }
}

impl Drop for StagedCalls<'_> {
    fn drop(&mut self) {
        unsafe { zkm_staged_calls_free(self.handle) }
    }
}

/// `prove_segments_ops_calls_raw` on calls staged ahead of the call: zkm_prove_segments_ops_steps on the handle's outputs, word for
/// word the same proofs, with its three host waits and nothing of the calls read on the calling thread.
pub fn prove_segments_ops_calls_staged(ctx: *mut zkm_ctx, staged: &StagedCalls, config: &zkm_stark_config, public_values: &[&[u64]])
                                       -> Result<SegmentProofs> {
    let (mut lists, mut ops, mut images) = (Vec::new(), Vec::new(), Vec::new());
    for s in 0..staged.nseg {
        let (st, o, im) = staged.get(s)?;
        lists.push(st);
        ops.push(o);
        images.push(im);
    }
    let images_ptr = if staged.with_images { images.as_ptr() } else { std::ptr::null() };
    size_then_prove(staged.nseg, public_values, config.num_challenges as usize, |pv, npv, proofs, offs, chal, err| unsafe {
        zkm_prove_segments_ops_steps(ctx, config, staged.nseg, images_ptr, lists.as_ptr(), ops.as_ptr(), pv, npv, proofs, offs, chal, err)
    })
}
