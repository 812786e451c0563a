//! arithmetic_hip.rs -- the Arithmetic table's witness (ArithmeticStark::generate_trace, arithmetic/arithmetic_stark.rs:155-185)
//! built by libzkmhip.so from the segment's arithmetic operations (zkm_arithmetic_trace, include/zkm_hip.h).
//!
//! Goes into the zkm-prover crate as `prover/src/arithmetic_hip.rs`, beside `prove_hip.rs`; `Traces::into_tables`
//! (witness/traces.rs:273) calls `arithmetic_trace_hip` instead of `all_stark.arithmetic_stark.generate_trace(&arithmetic_ops)` when
//! the `hip` feature is on.  The reference items it uses are checked by tests/test_rust_arithmetic_names.py.
//! NOT COMPILED in the build image (no cargo / rustc there).
use anyhow::Result;
use plonky2::field::polynomial::PolynomialValues;
use plonky2::field::types::PrimeField64;
use plonky2::hip::sys::*;

use crate::arithmetic::Operation;

/// The operations of a segment in the 3-word layout of zkm_arithmetic_trace: {row filter, input0, input1}, the arguments
/// `Operation::binary` received.  result0 / result1 are not passed: the kernel computes them as `BinaryOperator::result` does.
pub fn arithmetic_op_words(arithmetic_ops: &[Operation]) -> Vec<u32> {
    let mut w = Vec::with_capacity(3 * arithmetic_ops.len());
    for op in arithmetic_ops {
        match op {
            Operation::BinaryOperation { operator, input0, input1, .. } => w.extend_from_slice(&[
                operator.row_filter() as u32,
                *input0,
                *input1,
            ]),
        }
    }
    w
}

/// An Arithmetic table in HBM (54 x 2^log_n words, column-major), made by zkm_arithmetic_trace; freed on drop.  `ptr()` is what the
/// device-pointer entry points (zkm_prove_segment, zkm_prove_with_traces) take for Table::Arithmetic.
pub struct DeviceArithmeticTrace {
    ctx: *mut zkm_ctx,
    ptr: *mut u64,
    pub log_n: u32,
}
impl DeviceArithmeticTrace {
    pub fn ptr(&self) -> *const u64 {
        self.ptr
    }
}
impl Drop for DeviceArithmeticTrace {
    fn drop(&mut self) {
        unsafe { zkm_dev_free(self.ctx, self.ptr as *mut core::ffi::c_void) };
    }
}

/// `ArithmeticStark::generate_trace` (arithmetic_stark.rs:155-185) on the GPU, the table left in HBM at the reference's height
/// (max(2^16, next_pow2(rows))): the sizing call, then the trace call.
pub fn arithmetic_trace_dev(ctx: *mut zkm_ctx, arithmetic_ops: &[Operation]) -> Result<DeviceArithmeticTrace> {
    let words = arithmetic_op_words(arithmetic_ops);
    let mut err = std::ptr::null_mut();
    let mut natural = 0usize;
    check(unsafe { zkm_arithmetic_trace(ctx, words.as_ptr(), arithmetic_ops.len(), 0, std::ptr::null_mut(), &mut natural, &mut err) }, err)?;
    let log_n = natural.trailing_zeros();
    let mut p: *mut core::ffi::c_void = std::ptr::null_mut();
    check(unsafe { zkm_dev_alloc(ctx, (ZKM_ARITHMETIC_COLS << log_n) * 8, &mut p, &mut err) }, err)?;
    let t = DeviceArithmeticTrace { ctx, ptr: p as *mut u64, log_n };
    check(unsafe { zkm_arithmetic_trace(ctx, words.as_ptr(), arithmetic_ops.len(), log_n, t.ptr, &mut natural, &mut err) }, err)?;
    Ok(t)
}

/// Drop-in for `all_stark.arithmetic_stark.generate_trace(&arithmetic_ops)` in `Traces::into_tables` (witness/traces.rs:273): the
/// same fifty-four columns, built on the GPU and downloaded.
pub fn arithmetic_trace_hip<F: PrimeField64>(ctx: *mut zkm_ctx, arithmetic_ops: &[Operation]) -> Result<Vec<PolynomialValues<F>>> {
    let t = arithmetic_trace_dev(ctx, arithmetic_ops)?;
    let n = 1usize << t.log_n;
    let mut host = vec![0u64; ZKM_ARITHMETIC_COLS * n];
    let mut err = std::ptr::null_mut();
    check(unsafe { zkm_dev_download(ctx, host.as_mut_ptr() as *mut core::ffi::c_void, t.ptr as *const core::ffi::c_void, host.len() * 8,
                                    &mut err) }, err)?;
    Ok(host.chunks_exact(n).map(|col| PolynomialValues::new(col.iter().map(|&x| F::from_canonical_u64(x)).collect())).collect())
}
