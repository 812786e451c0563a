//! boot_hip.rs -- a segment's bootstrap kernel (cpu/bootstrap_kernel.rs:26-306) built by libzkmhip.so from the segment's image
//! (the zkm_*_boot calls, include/zkm_hip.h) instead of on the host: `generate_traces` (generation/mod.rs:25-76) then pushes only what
//! `simulate_cpu` does, with clocks from the bootstrap's row count on (zkm_boot_counts), and the library puts the bootstrap's CPU rows,
//! memory operations, Poseidon inputs and sponge rows in front.  Bootstrap only: `generate_exit_kernel` has no caller in the reference
//! (generation/mod.rs:168).  Images are staged, and taken by the pool, beside a segment's calls
//! (`calls_hip.rs` `StagedCalls`, `prove_segments_calls_pool_hip`).
//!
//! Goes into the zkm-prover crate as `prover/src/boot_hip.rs`, beside `segment_hip.rs`.  The reference items used here are checked by
//! tests/test_rust_boot_names.py.  NOT COMPILED in the build image (no cargo / rustc there).
use anyhow::{ensure, Result};
use plonky2::hip::sys::*;

use crate::cpu::kernel::elf::Program;
use crate::segment_hip::{size_then_prove, SegmentProofs};

/// The image of a segment's Program (cpu/kernel/elf.rs:13-31, filled by load_segment from emulator/src/state.rs:33-43) as the zkm_*_boot
/// calls take it: the BTreeMap's pairs in its own (ascending) order.  `image()` is valid while `self` lives.
pub struct BootImageHost {
    addrs: Vec<u32>,
    values: Vec<u32>,
    entry: u32,
    pre_hash_root: [u8; 32],
    pre_image_id: [u8; 32],
}
pub fn boot_image_from_segment(program: &Program) -> BootImageHost {
    BootImageHost {
        addrs: program.image.keys().copied().collect(),
        values: program.image.values().copied().collect(),
        entry: program.entry,
        pre_hash_root: program.pre_hash_root,
        pre_image_id: program.pre_image_id,
    }
}
impl BootImageHost {
    /// check: refuse a page hash, root hash or image id that does not match (the three assert_eq of the reference's bootstrap)
    pub fn image(&self, check: bool) -> zkm_boot_image {
        zkm_boot_image {
            addrs: self.addrs.as_ptr(), values: self.values.as_ptr(), nwords: self.addrs.len(),
            npages: self.addrs.iter().filter(|addr| *addr & 0xFFF == 0).count(),
            entry: self.entry, check: check as u32, pre_hash_root: self.pre_hash_root, pre_image_id: self.pre_image_id,
        }
    }
}

/// K x (bootstrap from the image + `into_tables` + `prove_with_traces`) in one call.  `segments[s]` holds only what `simulate_cpu`
/// pushed for segment s (CPU rows with clocks from the bootstrap's row count on: zkm_boot_counts); rows of bootstrap and segment
/// together must be a power of two.  Results as `prove_segments_ops_hip`.
pub fn prove_segments_ops_boot_raw(ctx: *mut zkm_ctx, images: &[zkm_boot_image], segments: &[zkm_segment_ops], config: &zkm_stark_config,
                                   public_values: &[&[u64]]) -> Result<SegmentProofs> {
    ensure!(images.len() == segments.len(), "{} images for {} segments", images.len(), segments.len());
    size_then_prove(segments.len(), public_values, config.num_challenges as usize, |pv, npv, proofs, offs, chal, err| unsafe {
        zkm_prove_segments_ops_boot(ctx, config, segments.len(), images.as_ptr(), segments.as_ptr(), pv, npv, proofs, offs, chal, err)
    })
}
