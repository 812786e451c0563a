//! memory_hip.rs -- the Memory table's witness (MemoryStark::generate_trace, memory/memory_stark.rs:135-248) built by
//! libzkmhip.so from the segment's raw memory operations (zkm_memory_trace, include/zkm_hip.h).
//!
//! Goes into the zkm-prover crate as `prover/src/memory_hip.rs`, beside `prove_hip.rs`; `Traces::into_tables`
//! (witness/traces.rs:272) calls `memory_trace_hip` instead of `all_stark.memory_stark.generate_trace(&mut memory_ops)` when the
//! `hip` feature is on.  The reference items it uses are checked by tests/test_rust_memory_names.py.
//! NOT COMPILED in the build image (no cargo / rustc there).
use anyhow::Result;
use plonky2::field::polynomial::PolynomialValues;
use plonky2::field::types::PrimeField64;
use plonky2::hip::sys::*;

use crate::witness::memory::{MemoryOp, MemoryOpKind};

/// The operations of a segment in the 6-word layout of zkm_memory_trace: {context, segment, virt, timestamp, is_read, value}.  Only
/// `MemoryOp::new` operations (filter true, witness/memory.rs:79-96) go in: the padding and dummy rows are the kernel's to make.
pub fn memory_op_words(memory_ops: &[MemoryOp]) -> Result<Vec<u64>> {
    let mut w = Vec::with_capacity(6 * memory_ops.len());
    for (i, op) in memory_ops.iter().enumerate() {
        anyhow::ensure!(op.filter, "memory op {} has filter = false: zkm_memory_trace takes the segment's MemoryOp::new operations", i);
        w.extend_from_slice(&[
            op.address.context as u64,
            op.address.segment as u64,
            op.address.virt as u64,
            op.timestamp as u64,
            matches!(op.kind, MemoryOpKind::Read) as u64,
            op.value as u64,
        ]);
    }
    Ok(w)
}

/// A Memory table in HBM (13 x 2^log_n words, column-major), made by zkm_memory_trace; freed on drop.  `ptr()` is what the
/// device-pointer entry points (zkm_prove_segment, zkm_prove_with_traces) take for Table::Memory.
pub struct DeviceMemoryTrace {
    ctx: *mut zkm_ctx,
    ptr: *mut u64,
    pub log_n: u32,
}
impl DeviceMemoryTrace {
    pub fn ptr(&self) -> *const u64 {
        self.ptr
    }
}
impl Drop for DeviceMemoryTrace {
    fn drop(&mut self) {
        unsafe { zkm_dev_free(self.ctx, self.ptr as *mut core::ffi::c_void) };
    }
}

/// `MemoryStark::generate_trace` (memory_stark.rs:135-248) on the GPU, the table left in HBM at the reference's height: the sizing
/// call, then the trace call.
pub fn memory_trace_dev(ctx: *mut zkm_ctx, memory_ops: &[MemoryOp]) -> Result<DeviceMemoryTrace> {
    let words = memory_op_words(memory_ops)?;
    let mut err = std::ptr::null_mut();
    let mut natural = 0usize;
    check(unsafe { zkm_memory_trace(ctx, words.as_ptr(), memory_ops.len(), 0, std::ptr::null_mut(), &mut natural, &mut err) }, err)?;
    let log_n = natural.trailing_zeros();
    let mut p: *mut core::ffi::c_void = std::ptr::null_mut();
    check(unsafe { zkm_dev_alloc(ctx, (ZKM_MEMORY_COLS << log_n) * 8, &mut p, &mut err) }, err)?;
    let t = DeviceMemoryTrace { ctx, ptr: p as *mut u64, log_n };
    check(unsafe { zkm_memory_trace(ctx, words.as_ptr(), memory_ops.len(), log_n, t.ptr, &mut natural, &mut err) }, err)?;
    Ok(t)
}

/// Drop-in for `all_stark.memory_stark.generate_trace(&mut memory_ops)` in `Traces::into_tables` (witness/traces.rs:272): the same
/// thirteen columns, built on the GPU and downloaded.
pub fn memory_trace_hip<F: PrimeField64>(ctx: *mut zkm_ctx, memory_ops: &[MemoryOp]) -> Result<Vec<PolynomialValues<F>>> {
    let t = memory_trace_dev(ctx, memory_ops)?;
    let n = 1usize << t.log_n;
    let mut host = vec![0u64; ZKM_MEMORY_COLS * n];
    let mut err = std::ptr::null_mut();
    check(unsafe { zkm_dev_download(ctx, host.as_mut_ptr() as *mut core::ffi::c_void, t.ptr as *const core::ffi::c_void, host.len() * 8,
                                    &mut err) }, err)?;
    Ok(host.chunks_exact(n).map(|col| PolynomialValues::new(col.iter().map(|&x| F::from_canonical_u64(x)).collect())).collect())
}
