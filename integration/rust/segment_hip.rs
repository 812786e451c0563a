//! segment_hip.rs -- a whole segment's tables (Traces::into_tables, witness/traces.rs:230-320) built by libzkmhip.so from the
//! segment's raw operations (zkm_segment_tables / zkm_prove_segment_ops, include/zkm_hip.h), and its proof in one call; K segments
//! built in one set of launches and proven in lock-step (zkm_prove_segments_ops), their lists staged behind the proofs in flight
//! (StagedOps), and a pool's workers taking operations (prove_segments_ops_pool_hip).
//!
//! Goes into the zkm-prover crate as `prover/src/segment_hip.rs`, beside `prove_hip.rs`, `memory_hip.rs` and `arithmetic_hip.rs`;
//! `generate_traces` -> `into_tables` -> `prove_with_traces` (generation/mod.rs:25-76) becomes `prove_segment_ops_hip` when the `hip`
//! feature is on.  One addition to logic.rs is needed, because the fields of logic::Operation are private to that module:
//!
//!     impl Operation { pub(crate) fn hip_words(&self) -> [u32; 3] { [self.operator as u32, self.input0, self.input1] } }
//!
//! With `boot_image_from_segment` (boot_hip.rs) the bootstrap kernel (cpu/bootstrap_kernel.rs:26-306) is not generated on the host at all: the zkm_*_boot
//! calls build its rows from the segment's image, and `generate_traces` then pushes only what `simulate_cpu` does (bootstrap only: the
//! reference's exit kernel has no caller).
//!
//! (Op is And, Or, Xor, Nor in that order: the op codes 0 .. 3 of zkm_logic_trace.)  The reference items used here are checked by
//! tests/test_rust_segment_names.py, tests/test_rust_segments_ops_names.py and tests/test_rust_boot_names.py.  NOT COMPILED in the build image (no cargo / rustc there).
use anyhow::{ensure, Result};
use plonky2::field::types::PrimeField64;
use plonky2::hip::sys::*;

use crate::arithmetic_hip::arithmetic_op_words;
use crate::memory_hip::memory_op_words;
use crate::witness::memory::MemoryAddress;
use crate::witness::traces::Traces;

/// The host arrays behind a zkm_segment_ops: the CPU rows are borrowed from the Traces as they are (CpuColumnsView is #[repr(C)],
/// cpu/columns/mod.rs:66: ncpu_rows x 259 words, row-major), every other list is packed here into the layout of its entry point.
pub struct SegmentOpsHost {
    cpu: *const u64,
    ncpu: usize,
    arithmetic: Vec<u32>,
    logic: Vec<u32>,
    memory: Vec<u64>,
    poseidon_inputs: Vec<u64>,
    poseidon_ts: Vec<u64>,
    poseidon_sponge: (Vec<u8>, Vec<u64>, Vec<u64>),
    keccak_inputs: Vec<u64>,
    keccak_ts: Vec<u64>,
    keccak_sponge: (Vec<u8>, Vec<u64>, Vec<u64>),
    sha_extend_inputs: Vec<u8>,
    sha_extend_ts: Vec<u64>,
    sha_extend_sponge: (Vec<u32>, Vec<u64>),
    sha_compress: (Vec<u32>, Vec<u32>, Vec<u64>),
}

fn addr_words(a: &MemoryAddress) -> (u64, u64, u64) {
    (a.context as u64, a.segment as u64, a.virt as u64)
}

/// One sponge table's operations: bytes, nops + 1 offsets, nops x {context, segment, virt_base, timestamp}.  Word i of an input must be
/// read at virt_base + i (zkm_keccak_sponge_trace's layout): other addresses are an error, not a guess.
fn sponge_lists<'a>(ops: impl Iterator<Item = (&'a [MemoryAddress], usize, &'a [u8])>, what: &str) -> Result<(Vec<u8>, Vec<u64>, Vec<u64>)> {
    let (mut bytes, mut off, mut meta) = (Vec::new(), vec![0u64], Vec::new());
    for (k, (base_address, timestamp, input)) in ops.enumerate() {
        ensure!(!input.is_empty() && !base_address.is_empty(), "{} op {}: empty input (base_address[0] is required)", what, k);
        let (ctx, seg, virt) = addr_words(&base_address[0]);
        // the words sit 1 apart (the bootstrap's operations) or 4 apart (a SYSKECCAK call reads one memory word every 4 bytes: the meta
        // says so with ZKM_SPONGE_BYTE_ADDRESSED); an operation of one word is logged unflagged
        let step = if base_address.len() > 1 { addr_words(&base_address[1]).2.wrapping_sub(virt) } else { 1 };
        ensure!(step == 1 || step == 4, "{} op {}: base addresses are neither 1 nor 4 apart", what, k);
        for (i, a) in base_address.iter().enumerate() {
            ensure!(addr_words(a) == (ctx, seg, virt + step * i as u64), "{} op {}: base addresses are not {} apart throughout", what, k, step);
        }
        bytes.extend_from_slice(input);
        off.push(bytes.len() as u64);
        meta.extend_from_slice(&[ctx, seg, if step == 4 { virt | ZKM_SPONGE_BYTE_ADDRESSED } else { virt }, timestamp as u64]);
    }
    Ok((bytes, off, meta))
}

/// Packs a segment's Traces into the lists of zkm_segment_ops.  Fails where the C layouts cannot express the data: sponge addresses
/// that are neither 1 nor 4 apart throughout an operation, SHA-extend round operations that are not complete 48-round schedules, SHA-compress rows that are not 65
/// per compression (or do not follow their compression's addresses and timestamp).
pub fn segment_ops_host<F: PrimeField64>(traces: &Traces<F>) -> Result<SegmentOpsHost> {
    let le = |b: &[u8]| u32::from_le_bytes([b[0], b[1], b[2], b[3]]);
    let mut poseidon_inputs = Vec::with_capacity(12 * traces.poseidon_inputs.len());
    let mut poseidon_ts = Vec::with_capacity(traces.poseidon_inputs.len());
    for (input, ts) in &traces.poseidon_inputs {
        poseidon_inputs.extend(input.iter().map(|x| x.to_canonical_u64()));
        poseidon_ts.push(*ts as u64);
    }
    let mut keccak_inputs = Vec::with_capacity(25 * traces.keccak_inputs.len());
    let mut keccak_ts = Vec::with_capacity(traces.keccak_inputs.len());
    for (input, ts) in &traces.keccak_inputs {
        keccak_inputs.extend_from_slice(input);
        keccak_ts.push(*ts as u64);
    }
    let mut sha_extend_inputs = Vec::with_capacity(16 * traces.sha_extend_inputs.len());
    let mut sha_extend_ts = Vec::with_capacity(traces.sha_extend_inputs.len());
    for (input, ts) in &traces.sha_extend_inputs {
        sha_extend_inputs.extend_from_slice(input);
        sha_extend_ts.push(*ts as u64);
    }
    // ShaExtendSponge: 48 consecutive round operations are one schedule; w[0 .. 16] are the w_i_minus_16 words of its first 16 rounds,
    // w[j] lives at address(w[0]) + 4 j, round r is stamped timestamp(round 0) + 20 r
    let ext = &traces.sha_extend_sponge_ops;
    ensure!(ext.len() % 48 == 0, "ShaExtendSponge: {} round operations are not complete 48-round schedules", ext.len());
    let (mut w16, mut ext_meta) = (Vec::with_capacity(ext.len() / 3), Vec::with_capacity(ext.len() / 12));
    for (b, rounds) in ext.chunks_exact(48).enumerate() {
        let (ctx, seg, w0) = addr_words(&rounds[0].base_address[2]);
        for (r, op) in rounds.iter().enumerate() {
            let i = r as u64 + 16;
            let want = [i - 15, i - 2, i - 16, i - 7].map(|j| (ctx, seg, w0 + 4 * j));
            ensure!(op.i == rounds[0].i + r && op.timestamp == rounds[0].timestamp + 20 * r && op.base_address.len() == 4
                        && op.base_address.iter().map(addr_words).eq(want.into_iter()) && addr_words(&op.output_address) == (ctx, seg, w0 + 4 * i),
                    "ShaExtendSponge schedule {} round {}: not the round of a complete schedule at contiguous addresses", b, r);
            if r < 16 {
                w16.push(le(&op.input[8..12]));
            }
        }
        ext_meta.extend_from_slice(&[ctx, seg, w0, rounds[0].timestamp as u64]);
    }
    // ShaCompress and ShaCompressSponge from the sponge operations: hx = input (le words), w = w_i_s, meta {context, segment, address of
    // hx[0], timestamp, address of w[0], segment of w, context of w, 0}; the compress table's rows must be the 65 of each operation
    let comp = &traces.sha_compress_sponge_ops;
    ensure!(traces.sha_compress_inputs.len() == 65 * comp.len(), "ShaCompress: {} rows for {} compressions (65 each)",
            traces.sha_compress_inputs.len(), comp.len());
    let (mut hx, mut w, mut comp_meta) = (Vec::with_capacity(8 * comp.len()), Vec::with_capacity(64 * comp.len()), Vec::with_capacity(8 * comp.len()));
    for (k, op) in comp.iter().enumerate() {
        ensure!(op.base_address.len() == 9 && op.input.len() == 32 && op.w_i_s.len() == 64, "ShaCompressSponge op {}: unexpected shape", k);
        let (ctx, seg, h0) = addr_words(&op.base_address[0]);
        let (wctx, wseg, wv) = addr_words(&op.base_address[8]);
        ensure!((0..8).all(|q| addr_words(&op.base_address[q]) == (ctx, seg, h0 + 4 * q as u64)), "ShaCompressSponge op {}: hx not contiguous", k);
        for (rd, (_, addr, ts)) in traces.sha_compress_inputs[65 * k..65 * (k + 1)].iter().enumerate() {
            ensure!(addr_words(addr) == (wctx, wseg, wv + 4 * rd as u64) && *ts == op.timestamp,
                    "ShaCompress row {}: not round {} of compression {}", 65 * k + rd, rd, k);
        }
        hx.extend(op.input.chunks_exact(4).map(le));
        w.extend(op.w_i_s.iter().map(|b| u32::from_le_bytes(*b)));
        comp_meta.extend_from_slice(&[ctx, seg, h0, op.timestamp as u64, wv, wseg, wctx, 0]);
    }
    Ok(SegmentOpsHost {
        cpu: traces.cpu.as_ptr() as *const u64,
        ncpu: traces.cpu.len(),
        arithmetic: arithmetic_op_words(&traces.arithmetic_ops),
        logic: traces.logic_ops.iter().flat_map(|op| op.hip_words()).collect(),
        memory: memory_op_words(&traces.memory_ops)?,
        poseidon_inputs,
        poseidon_ts,
        poseidon_sponge: sponge_lists(traces.poseidon_sponge_ops.iter().map(|o| (&o.base_address[..], o.timestamp, &o.input[..])), "PoseidonSponge")?,
        keccak_inputs,
        keccak_ts,
        keccak_sponge: sponge_lists(traces.keccak_sponge_ops.iter().map(|o| (&o.base_address[..], o.timestamp, &o.input[..])), "KeccakSponge")?,
        sha_extend_inputs,
        sha_extend_ts,
        sha_extend_sponge: (w16, ext_meta),
        sha_compress: (hx, w, comp_meta),
    })
}

impl SegmentOpsHost {
    /// The zkm_segment_ops of these lists (valid while `self` and the Traces it borrows the CPU rows from live).
    pub fn ops(&self) -> zkm_segment_ops {
        let (c_hx, c_w, c_meta) = (&self.sha_compress.0, &self.sha_compress.1, &self.sha_compress.2);
        zkm_segment_ops {
            cpu_rows: self.cpu, ncpu_rows: self.ncpu,
            arithmetic_ops: self.arithmetic.as_ptr(), narithmetic: self.arithmetic.len() / 3,
            logic_ops: self.logic.as_ptr(), nlogic: self.logic.len() / 3,
            memory_ops: self.memory.as_ptr(), nmemory: self.memory.len() / 6,
            poseidon_inputs: self.poseidon_inputs.as_ptr(), poseidon_timestamps: self.poseidon_ts.as_ptr(), nposeidon: self.poseidon_ts.len(),
            poseidon_sponge_inputs: self.poseidon_sponge.0.as_ptr(), poseidon_sponge_off: self.poseidon_sponge.1.as_ptr(),
            poseidon_sponge_meta: self.poseidon_sponge.2.as_ptr(), nposeidon_sponge: self.poseidon_sponge.1.len() - 1,
            keccak_inputs: self.keccak_inputs.as_ptr(), keccak_timestamps: self.keccak_ts.as_ptr(), nkeccak: self.keccak_ts.len(),
            keccak_sponge_inputs: self.keccak_sponge.0.as_ptr(), keccak_sponge_off: self.keccak_sponge.1.as_ptr(),
            keccak_sponge_meta: self.keccak_sponge.2.as_ptr(), nkeccak_sponge: self.keccak_sponge.1.len() - 1,
            sha_extend_inputs: self.sha_extend_inputs.as_ptr(), sha_extend_timestamps: self.sha_extend_ts.as_ptr(), nsha_extend: self.sha_extend_ts.len(),
            sha_extend_sponge_w16: self.sha_extend_sponge.0.as_ptr(), sha_extend_sponge_meta: self.sha_extend_sponge.1.as_ptr(),
            nsha_extend_sponge: self.sha_extend_sponge.1.len() / 4,
            sha_compress_hx: c_hx.as_ptr(), sha_compress_w: c_w.as_ptr(), sha_compress_meta: c_meta.as_ptr(), nsha_compress: c_meta.len() / 8,
            sha_compress_sponge_hx: c_hx.as_ptr(), sha_compress_sponge_w: c_w.as_ptr(), sha_compress_sponge_meta: c_meta.as_ptr(),
            nsha_compress_sponge: c_meta.len() / 8,
        }
    }
}

/// The twelve tables of a segment in ONE device block (a segment-shaped zkm_staged), at the reference's heights; freed on drop.
/// `tables()` gives traces[s] of zkm_prove_segments: K of these prove in lock-step.
pub struct DeviceSegment {
    staged: *mut zkm_staged,
    pub log_n: [u32; 12],
}
impl DeviceSegment {
    pub fn tables(&self) -> Result<[*const u64; 12]> {
        let mut p = [std::ptr::null(); 12];
        ensure!(unsafe { zkm_staged_segment_ptrs(self.staged, p.as_mut_ptr()) } == 0, "zkm_staged_segment_ptrs failed");
        Ok(p)
    }
}
impl Drop for DeviceSegment {
    fn drop(&mut self) {
        unsafe { zkm_staged_free(self.staged) };
    }
}

/// `traces.into_tables(all_stark, config, timing)` (witness/traces.rs:230-320) on the GPU, the tables left in HBM.
pub fn into_tables_dev<F: PrimeField64>(ctx: *mut zkm_ctx, traces: &Traces<F>, config: &zkm_stark_config) -> Result<DeviceSegment> {
    let host = segment_ops_host(traces)?;
    let ops = host.ops();
    let mut seg = DeviceSegment { staged: std::ptr::null_mut(), log_n: [0; 12] };
    let mut err = std::ptr::null_mut();
    check(unsafe { zkm_segment_tables(ctx, config, &ops, seg.log_n.as_mut_ptr(), &mut seg.staged, &mut err) }, err)?;
    Ok(seg)
}

/// `into_tables` + `prove_with_traces` (generation/mod.rs:25-76) in one call: the proof blobs (offsets in the thirteen words of the
/// second element, include/zkm_hip.h layout) and the CTL challenges, word for word zkm_prove_segment's on the same tables.
pub fn prove_segment_ops_hip<F: PrimeField64>(ctx: *mut zkm_ctx, traces: &Traces<F>, config: &zkm_stark_config, public_values: &[u64])
                                              -> Result<(Vec<u64>, [usize; 13], Vec<u64>)> {
    let host = segment_ops_host(traces)?;
    let ops = host.ops();
    let mut offs = [0usize; 13];
    let mut err = std::ptr::null_mut();
    check(unsafe { zkm_prove_segment_ops(ctx, config, &ops, public_values.as_ptr(), public_values.len(), std::ptr::null_mut(),
                                         offs.as_mut_ptr(), std::ptr::null_mut(), &mut err) }, err)?;
    let mut proofs = vec![0u64; offs[12]];
    let mut challenges = vec![0u64; 2 * config.num_challenges as usize];
    check(unsafe { zkm_prove_segment_ops(ctx, config, &ops, public_values.as_ptr(), public_values.len(), proofs.as_mut_ptr(),
                                         offs.as_mut_ptr(), challenges.as_mut_ptr(), &mut err) }, err)?;
    Ok((proofs, offs, challenges))
}

/// One (proof blobs, offsets, CTL challenges) per segment, as `prove_segment_ops_hip` returns them.
pub type SegmentProofs = Vec<(Vec<u64>, [usize; 13], Vec<u64>)>;

/// The two calls of a K-segment entry point -- sizing, then proving into buffers of those sizes -- behind one closure:
/// `call(public_values, npublic, proofs_out, proof_offsets_out, ctl_challenges_out, err)`.
pub(crate) fn size_then_prove(nseg: usize, public_values: &[&[u64]], num_challenges: usize,
                   call: impl Fn(*const *const u64, *const usize, *const *mut u64, *mut usize, *const *mut u64, *mut *mut std::os::raw::c_char) -> i32)
                   -> Result<SegmentProofs> {
    ensure!(public_values.len() == nseg, "{} public value lists for {} segments", public_values.len(), nseg);
    let pub_ptrs: Vec<*const u64> = public_values.iter().map(|p| p.as_ptr()).collect();
    let pub_lens: Vec<usize> = public_values.iter().map(|p| p.len()).collect();
    let mut offs = vec![0usize; 13 * nseg];
    let mut err = std::ptr::null_mut();
    check(call(pub_ptrs.as_ptr(), pub_lens.as_ptr(), std::ptr::null(), offs.as_mut_ptr(), std::ptr::null(), &mut err), err)?;
    let mut proofs: Vec<Vec<u64>> = (0..nseg).map(|s| vec![0u64; offs[13 * s + 12]]).collect();
    let mut challenges: Vec<Vec<u64>> = (0..nseg).map(|_| vec![0u64; 2 * num_challenges]).collect();
    let proof_ptrs: Vec<*mut u64> = proofs.iter_mut().map(|p| p.as_mut_ptr()).collect();
    let chal_ptrs: Vec<*mut u64> = challenges.iter_mut().map(|c| c.as_mut_ptr()).collect();
    check(call(pub_ptrs.as_ptr(), pub_lens.as_ptr(), proof_ptrs.as_ptr(), offs.as_mut_ptr(), chal_ptrs.as_ptr(), &mut err), err)?;
    Ok(proofs.into_iter().zip(challenges).enumerate().map(|(s, (p, c))| {
        let mut seg_offs = [0usize; 13];
        seg_offs.copy_from_slice(&offs[13 * s..13 * s + 13]);
        (p, seg_offs, c)
    }).collect())
}

/// K x (`into_tables` + `prove_with_traces`) in one call: every generation kernel is launched once for all K segments, the call has
/// three host waits whatever K, and the proofs advance in lock-step.  Each result is word for word `prove_segment_ops_hip`'s.
pub fn prove_segments_ops_hip<F: PrimeField64>(ctx: *mut zkm_ctx, segments: &[Traces<F>], config: &zkm_stark_config, public_values: &[&[u64]])
                                               -> Result<SegmentProofs> {
    let hosts = segments.iter().map(segment_ops_host).collect::<Result<Vec<_>>>()?;
    let ops: Vec<zkm_segment_ops> = hosts.iter().map(|h| h.ops()).collect();
    prove_segments_ops_raw(ctx, &ops, config, public_values)
}

/// ... on zkm_segment_ops the caller holds: host lists, or the device lists of `StagedOps::ops` (same context), mixed.
pub fn prove_segments_ops_raw(ctx: *mut zkm_ctx, ops: &[zkm_segment_ops], config: &zkm_stark_config, public_values: &[&[u64]])
                              -> Result<SegmentProofs> {
    size_then_prove(ops.len(), public_values, config.num_challenges as usize, |pv, npv, proofs, offs, chal, err| unsafe {
        zkm_prove_segments_ops(ctx, config, ops.len(), ops.as_ptr(), pv, npv, proofs, offs, chal, err)
    })
}

/// A segment's lists on their way into HBM behind the context's current work (zkm_segment_ops_stage): stage the next call's segments
/// while the current call proves, hand `ops()` to `prove_segments_ops_raw` on the same context, drop after that call has returned.
/// `host` may be dropped or reused once `ready(true)` has returned: the handle keeps its own copy of the two sponge offset arrays.
pub struct StagedOps(*mut zkm_staged_ops);
impl StagedOps {
    pub fn new(ctx: *mut zkm_ctx, host: &SegmentOpsHost) -> Result<Self> {
        let ops = host.ops();
        let mut staged = std::ptr::null_mut();
        let mut err = std::ptr::null_mut();
        check(unsafe { zkm_segment_ops_stage(ctx, &ops, &mut staged, &mut err) }, err)?;
        Ok(Self(staged))
    }
    /// The same segment with device pointers, ordered behind the upload on the device (no host wait).
    pub fn ops(&self) -> Result<zkm_segment_ops> {
        let mut ops = std::mem::MaybeUninit::<zkm_segment_ops>::zeroed();
        ensure!(unsafe { zkm_staged_ops_get(self.0, ops.as_mut_ptr()) } == 0, "zkm_staged_ops_get failed");
        Ok(unsafe { ops.assume_init() })
    }
    /// Have the uploads landed?  `wait` blocks until they have.
    pub fn ready(&self, wait: bool) -> Result<bool> {
        let r = unsafe { zkm_staged_ops_ready(self.0, wait as i32) };
        ensure!(r >= 0, "zkm_staged_ops_ready: runtime error");
        Ok(r == 1)
    }
}
impl Drop for StagedOps {
    fn drop(&mut self) {
        unsafe { zkm_staged_ops_free(self.0) };
    }
}

/// All segments of a program over the pool's contexts, from their raw operations: the groups of `prove_segments_multi_hip`, each ONE
/// zkm_prove_segments_ops call on its worker's context.  `pool` is the `*mut zkm_pool` of a `HipPool` (prove_hip.rs).
pub fn prove_segments_ops_pool_hip<F: PrimeField64>(pool: *mut zkm_pool, segments: &[Traces<F>], config: &zkm_stark_config, max_stack: usize,
                                                    public_values: &[&[u64]]) -> Result<SegmentProofs> {
    let hosts = segments.iter().map(segment_ops_host).collect::<Result<Vec<_>>>()?;
    let ops: Vec<zkm_segment_ops> = hosts.iter().map(|h| h.ops()).collect();
    size_then_prove(ops.len(), public_values, config.num_challenges as usize, |pv, npv, proofs, offs, chal, err| unsafe {
        zkm_pool_prove_segments_ops(pool, config, ops.len(), max_stack, ops.as_ptr(), pv, npv, proofs, offs, chal, err)
    })
}
