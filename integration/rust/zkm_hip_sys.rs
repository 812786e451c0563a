//! zkm_hip_sys.rs -- `extern "C"` mirror of include/zkm_hip.h (libzkmhip.so), the drop-in boundary of the HIP proving path.
//!
//! Goes into the plonky2 fork as `plonky2/src/hip/sys.rs` (and is re-exported for zkm-prover).  Error convention of the
//! reference's only existing FFI (recursion/src/snark/snarks.rs:7-20, 39-59): `c_int` status, `*mut *mut c_char` message
//! that the caller frees.  `build.rs` links it the way recursion/build.rs:1-31 links the gnark library:
//!     println!("cargo:rustc-link-search=native={}", std::env::var("ZKM_HIP_LIB_DIR").unwrap());
//!     println!("cargo:rustc-link-lib=dylib=zkmhip");
//! NOT COMPILED in the build image (no cargo / rustc there); checked against the header by eye and by
//! tests/test_abi.py (every declaration, struct layout and constant).
#![allow(non_camel_case_types)]
use std::os::raw::{c_char, c_double, c_int, c_uint, c_void};

#[repr(C)] pub struct zkm_ctx { _p: [u8; 0] }
#[repr(C)] pub struct zkm_batch { _p: [u8; 0] }
#[repr(C)] pub struct zkm_pool { _p: [u8; 0] }
#[repr(C)] pub struct zkm_staged { _p: [u8; 0] }
pub enum zkm_staged_ops {}   // opaque: only ever behind a pointer

#[repr(C)] #[derive(Clone, Copy, Debug, Default)]
pub struct zkm_challenger { pub state: [u64; 12], pub in_buf: [u64; 8], pub out_buf: [u64; 8], pub n_in: u32, pub n_out: u32 }

#[repr(C)] #[derive(Clone, Copy, Debug)]
pub struct zkm_stark_config { pub rate_bits: c_uint, pub cap_height: c_uint, pub pow_bits: c_uint, pub num_challenges: c_uint,
                              pub num_queries: c_uint, pub arity_bits: c_uint, pub final_poly_bits: c_uint }

#[repr(C)] #[derive(Clone, Copy, Debug, Default)]
pub struct zkm_proof_layout {
    pub degree_bits: u64, pub trace_cols: u64, pub aux_cols: u64, pub quotient_polys: u64, pub ctl_zs: u64, pub cap_height: u64,
    pub fri_layers: u64, pub final_poly_len: u64, pub num_queries: u64, pub rate_bits: u64, pub arity_bits: u64,
    pub total_words: usize, pub init_challenger_state: usize, pub trace_cap: usize, pub aux_cap: usize, pub quotient_cap: usize,
    pub local_values: usize, pub next_values: usize, pub aux_polys: usize, pub aux_polys_next: usize, pub ctl_zs_first: usize,
    pub quotient_polys_open: usize, pub commit_phase_merkle_caps: usize, pub final_poly: usize, pub pow_witness: usize,
    pub query_round_proofs: usize, pub query_round_words: usize,
}
#[repr(C)] #[derive(Clone, Copy, Debug, Default)]
pub struct zkm_proof_query_layout {
    pub oracle_evals: [usize; 3], pub oracle_cols: [usize; 3], pub oracle_siblings: [usize; 3], pub initial_siblings: usize,
    pub layer_evals: [usize; 16], pub layer_siblings: [usize; 16], pub layer_siblings_count: [usize; 16],
}

#[repr(C)] #[derive(Clone, Copy, Debug, Default)]
pub struct zkm_column { pub n_local: u32, pub n_next: u32, pub term_off: u32, pub _pad: u32, pub constant: u64 }
#[repr(C)] #[derive(Clone, Copy, Debug, Default)]
pub struct zkm_colset { pub ncols: u32, pub col_off: u32, pub has_filter: u32, pub nprod: u32, pub prod_off: u32, pub nconst: u32,
                        pub const_off: u32, pub _pad: u32 }
#[repr(C)] #[derive(Clone, Copy, Debug)]
pub struct zkm_ctl_table { pub columns: *const zkm_column, pub ncolumns: usize, pub term_col: *const u32, pub term_coeff: *const u64,
                           pub nterms: usize, pub colsets: *const zkm_colset, pub ncolsets: usize, pub filter_idx: *const u32,
                           pub nfilter_idx: usize }
#[repr(C)] #[derive(Clone, Copy, Debug, Default)]
pub struct zkm_ctl_z { pub ncolsets: u32, pub colset_off: u32, pub num_helpers: u32, pub _pad: u32, pub beta: u64, pub gamma: u64 }
#[repr(C)] #[derive(Clone, Copy, Debug, Default)]
pub struct zkm_ctl_side { pub table: u32, pub colset: u32 }
#[repr(C)] #[derive(Clone, Copy, Debug, Default)]
pub struct zkm_cross_table_lookup { pub nlooking: u32, pub looking_off: u32, pub looked: zkm_ctl_side }
#[repr(C)] #[derive(Clone, Copy, Debug)]
pub struct zkm_table_input { pub table_id: c_int, pub trace: *const u64, pub ncols: usize, pub log_n: c_uint, pub ctl: *const zkm_ctl_table,
                             pub columns: *const *const u64 }
/// descriptor of one FRI oracle / batch for zkm_prove_openings_fri (FriInstanceInfo, stark.rs:91-148)
#[repr(C)] #[derive(Clone, Copy, Debug)]
pub struct zkm_fri_poly { pub oracle: u32, pub poly: u32 }
#[repr(C)] #[derive(Clone, Copy, Debug)]
pub struct zkm_fri_batch { pub point: [u64; 2], pub polys: *const zkm_fri_poly, pub npolys: usize }
/// a segment's raw operations for zkm_segment_tables / zkm_prove_segment_ops: one group per field of the reference's Traces, in its
/// order (witness/traces.rs:47-62); segment_hip.rs packs a Traces<F> into it
#[repr(C)] #[derive(Clone, Copy, Debug)]
pub struct zkm_segment_ops {
    pub cpu_rows: *const u64, pub ncpu_rows: usize,
    pub arithmetic_ops: *const u32, pub narithmetic: usize,
    pub logic_ops: *const u32, pub nlogic: usize,
    pub memory_ops: *const u64, pub nmemory: usize,
    pub poseidon_inputs: *const u64, pub poseidon_timestamps: *const u64, pub nposeidon: usize,
    pub poseidon_sponge_inputs: *const u8, pub poseidon_sponge_off: *const u64, pub poseidon_sponge_meta: *const u64, pub nposeidon_sponge: usize,
    pub keccak_inputs: *const u64, pub keccak_timestamps: *const u64, pub nkeccak: usize,
    pub keccak_sponge_inputs: *const u8, pub keccak_sponge_off: *const u64, pub keccak_sponge_meta: *const u64, pub nkeccak_sponge: usize,
    pub sha_extend_inputs: *const u8, pub sha_extend_timestamps: *const u64, pub nsha_extend: usize,
    pub sha_extend_sponge_w16: *const u32, pub sha_extend_sponge_meta: *const u64, pub nsha_extend_sponge: usize,
    pub sha_compress_hx: *const u32, pub sha_compress_w: *const u32, pub sha_compress_meta: *const u64, pub nsha_compress: usize,
    pub sha_compress_sponge_hx: *const u32, pub sha_compress_sponge_w: *const u32, pub sha_compress_sponge_meta: *const u64,
    pub nsha_compress_sponge: usize,
}
pub type ZkmSegmentOps = zkm_segment_ops;
// (The structs from here on carry Rust-style names, with the C names as aliases; tests/test_abi.py compares every struct of this file,
// under its C name, with the C compiler's layout of the header.)
/// one occurrence of a tuple zkm_check_ctls reports: side of the lookup (the looked side last), index of the table, row
#[repr(C)] #[derive(Clone, Copy, Debug, Default)]
pub struct ZkmCtlLocation { pub side: u32, pub table: u32, pub row: u64 }
pub type zkm_ctl_location = ZkmCtlLocation;
/// what zkm_check_ctls / zkm_segment_check_ctls found (include/zkm_hip.h): kind 0 consistent, 1 non-binary filter, 2 multisets differ,
/// 3 the check could not be made
#[repr(C)] #[derive(Clone, Copy, Debug)]
pub struct ZkmCtlReport {
    pub kind: u32, pub ctl: u32, pub attempts: u32, pub host_waits: u32,
    pub side: u32, pub table: u32,
    pub row: u64, pub filter_value: u64,
    pub width: u32, pub nwords: u32,
    pub tuple: [u64; 64],
    pub looking_count: u64, pub looked_count: u64,
    pub nlooking_locations: u32, pub nlooked_locations: u32,
    pub looking: [ZkmCtlLocation; 8], pub looked: [ZkmCtlLocation; 8],
}
pub type zkm_ctl_report = ZkmCtlReport;
/// the verdict of zkm_verify_* on one proof (include/zkm_hip.h):
/// code = ZKM_VERIFY_*, the check that failed, in the reference's order of checks
#[repr(C)] #[derive(Clone, Copy, Debug, Default)]
pub struct ZkmVerifyReport {
    pub code: u32, pub table: u32, pub challenge: u32, pub query: u32, pub tree: u32, pub layer: u32, pub ctl: u32, pub host_waits: u32,
}
pub type zkm_verify_report = ZkmVerifyReport;
/// a segment's memory image for the zkm_*_boot calls (include/zkm_hip.h):
/// the bootstrap kernel's part of Traces is built from it on the device
#[repr(C)] #[derive(Clone, Copy, Debug)]
pub struct ZkmBootImage {
    pub addrs: *const u32, pub values: *const u32, pub nwords: usize, pub npages: usize, pub entry: u32, pub check: u32,
    pub pre_hash_root: [u8; 32], pub pre_image_id: [u8; 32],
}
pub type zkm_boot_image = ZkmBootImage;
/// the dirty pages of a split, the hash pages that exist already, pc and the registers for zkm_image[s]_hash (include/zkm_hip.h)
#[repr(C)] #[derive(Clone, Copy, Debug)]
pub struct ZkmImagePages {
    pub dirty_index: *const u32, pub ndirty: usize, pub dirty_words: *const u32, pub known_index: *const u32, pub nknown: usize,
    pub known_words: *const u32, pub pc: u32, pub registers: [u8; 156],
}
pub type zkm_image_pages = ZkmImagePages;
/// one cycle of the compact step log and a segment's step list (include/zkm_hip.h): the CPU rows and the operations they push are built
/// from them on the device
#[repr(C)] #[derive(Clone, Copy, Debug, Default)]
pub struct ZkmCpuStep {
    pub pc: u32, pub next_pc: u32, pub insn: u32, pub kind: u32, pub flags: u32, pub context: u32, pub reads: [u32; 6],
}
pub type zkm_cpu_step = ZkmCpuStep;
#[repr(C)] #[derive(Clone, Copy, Debug)]
pub struct ZkmCpuSteps {
    pub steps: *const zkm_cpu_step, pub nsteps: usize, pub raw_rows: *const u64, pub nraw: usize,
}
pub type zkm_cpu_steps = ZkmCpuSteps;
/// `struct zkm_segment_calls` (include/zkm_hip.h "K segments' calls expanded in one set of launches"): one segment as the emulator records
/// it -- its step list with placeholders, its own operations, and the calls of the four kinds.  The header tags this struct and the
/// handle below instead of typedef'ing them; the extern block passes pointers to them as plain addresses (`*const c_void`)
#[repr(C)] #[derive(Clone, Copy, Debug)]
pub struct ZkmSegmentCalls {
    pub steps: zkm_cpu_steps, pub first_clock: u64, pub own: zkm_segment_ops,
    pub extend_w16: *const u32, pub extend_meta: *const u64, pub nextend: usize,
    pub compress_hx: *const u32, pub compress_w: *const u32, pub compress_meta: *const u64, pub ncompress: usize,
    pub keccak_inputs: *const u8, pub keccak_input_off: *const u64, pub keccak_meta: *const u64, pub keccak_digest_addrs: *const u64,
    pub nkeccak: usize,
    pub io_kinds: *const u32, pub io_data: *const u8, pub io_data_off: *const u64, pub io_meta: *const u64, pub nio: usize,
    pub insns: *const zkm_cpu_step, pub insn_clocks: *const u64, pub ninsns: usize,
}
pub enum ZkmExpandedCalls {}   // `struct zkm_expanded_calls`: opaque, only ever behind a pointer
pub const ZKM_CALLS_COUNTS: usize = 11;
pub const ZKM_STEP_BINARY_OP: u32 = 0; pub const ZKM_STEP_BINARY_IMM_OP: u32 = 1; pub const ZKM_STEP_LOGIC_OP: u32 = 2;
pub const ZKM_STEP_LOGIC_IMM_OP: u32 = 3; pub const ZKM_STEP_SHIFT: u32 = 4; pub const ZKM_STEP_SHIFT_IMM: u32 = 5;
pub const ZKM_STEP_BRANCH: u32 = 6; pub const ZKM_STEP_JUMPS: u32 = 7; pub const ZKM_STEP_JUMPI: u32 = 8; pub const ZKM_STEP_JUMPDIRECT: u32 = 9;
pub const ZKM_STEP_M_OP_LOAD: u32 = 10; pub const ZKM_STEP_M_OP_STORE: u32 = 11; pub const ZKM_STEP_NOP: u32 = 12;
pub const ZKM_STEP_CLZ_OP: u32 = 13; pub const ZKM_STEP_CLO_OP: u32 = 14; pub const ZKM_STEP_SIGNEXT8: u32 = 15;
pub const ZKM_STEP_SIGNEXT16: u32 = 16; pub const ZKM_STEP_SWAPHALF: u32 = 17; pub const ZKM_STEP_RDHWR: u32 = 18;
pub const ZKM_STEP_MOVZ_OP: u32 = 19; pub const ZKM_STEP_MOVN_OP: u32 = 20; pub const ZKM_STEP_TEQ: u32 = 21; pub const ZKM_STEP_EXT: u32 = 22;
pub const ZKM_STEP_INS: u32 = 23; pub const ZKM_STEP_ROR: u32 = 24; pub const ZKM_STEP_MADDU: u32 = 25; pub const ZKM_STEP_SYSCALL: u32 = 26;
pub const ZKM_STEP_PAD: u32 = 27; pub const ZKM_STEP_RAW: u32 = 28;
pub const ZKM_STEP_FLAG_KERNEL: u32 = 1; pub const ZKM_STEP_FLAG_BRANCH_R0: u32 = 2;
pub const ZKM_SYSCALL_OTHER: u32 = 0; pub const ZKM_SYSCALL_MMAP: u32 = 1; pub const ZKM_SYSCALL_BRK: u32 = 2; pub const ZKM_SYSCALL_CLONE: u32 = 3;
pub const ZKM_SYSCALL_READ: u32 = 5; pub const ZKM_SYSCALL_WRITE: u32 = 6; pub const ZKM_SYSCALL_FCNTL: u32 = 7;
pub const ZKM_SYSCALL_SET_THREAD_AREA: u32 = 8;
// a sponge operation's meta word 2 (virt_base) with this bit set: word w of the input is read at (virt_base & !bit) + 4 w
pub const ZKM_SPONGE_BYTE_ADDRESSED: u64 = 0x8000000000000000;
// beside it, on a SYSKECCAK call whose length is no multiple of 4: the call's last memory word is the padded message's
pub const ZKM_SPONGE_PADDED_TAIL: u64 = 0x4000000000000000;
// the kinds of zkm_io_calls_*: the data-moving helper behind generate_syscall's row (load_input, commit, verify, load_preimage)
pub const ZKM_IO_HINT_READ: u32 = 0; pub const ZKM_IO_COMMIT: u32 = 1; pub const ZKM_IO_VERIFY: u32 = 2; pub const ZKM_IO_PREIMAGE: u32 = 3;
// the kinds of zkm_insn_rows_*: the thirteen encodings decode() accepts and no ZKM_STEP_* kind takes
pub const ZKM_INSN_LUI: u32 = 0; pub const ZKM_INSN_MUL: u32 = 1; pub const ZKM_INSN_MULT: u32 = 2; pub const ZKM_INSN_MULTU: u32 = 3;
pub const ZKM_INSN_DIV: u32 = 4; pub const ZKM_INSN_DIVU: u32 = 5; pub const ZKM_INSN_MFHI: u32 = 6; pub const ZKM_INSN_MTHI: u32 = 7;
pub const ZKM_INSN_MFLO: u32 = 8; pub const ZKM_INSN_MTLO: u32 = 9; pub const ZKM_INSN_SDC1: u32 = 10; pub const ZKM_INSN_SYNC: u32 = 11;
pub const ZKM_INSN_PREF: u32 = 12;
pub const ZKM_VERIFY_OK: u32 = 0; pub const ZKM_VERIFY_SHAPE: u32 = 1; pub const ZKM_VERIFY_TRANSCRIPT_STATE: u32 = 2;
pub const ZKM_VERIFY_CTL_CHALLENGES: u32 = 3; pub const ZKM_VERIFY_QUOTIENT: u32 = 4; pub const ZKM_VERIFY_POW: u32 = 5;
pub const ZKM_VERIFY_INITIAL_MERKLE: u32 = 6; pub const ZKM_VERIFY_FRI_EVAL: u32 = 7; pub const ZKM_VERIFY_FRI_MERKLE: u32 = 8;
pub const ZKM_VERIFY_FINAL_POLY: u32 = 9; pub const ZKM_VERIFY_CTL_SUM: u32 = 10; pub const ZKM_VERIFY_FAILED: u32 = 11;

// ZKM_TABLE_* ids (NOT the reference's Table enum order: see zkm_table_enum_index)
// zkm_poseidon_selftest: output modes of a permutation probe, and the probes
pub const ZKM_POSEIDON_OUT_ALL: u32 = 0; pub const ZKM_POSEIDON_OUT_CAPACITY: u32 = 1; pub const ZKM_POSEIDON_OUT_DIGEST: u32 = 2;
pub const ZKM_POSEIDON_PROBE_PERMUTE_LANE: u32 = 0; pub const ZKM_POSEIDON_PROBE_PERMUTE_LANE_MFMA: u32 = 1; pub const ZKM_POSEIDON_PROBE_PERMUTE_QUAD: u32 = 2;
pub const ZKM_POSEIDON_PROBE_PERMUTE_WIDE: u32 = 3; pub const ZKM_POSEIDON_PROBE_MDS_VALU: u32 = 4; pub const ZKM_POSEIDON_PROBE_MDS_MFMA: u32 = 5;
pub const ZKM_POSEIDON_PROBE_MDS_QUAD: u32 = 6; pub const ZKM_POSEIDON_PROBE_MDS_ROWS: u32 = 7; pub const ZKM_POSEIDON_PROBE_GROUP3: u32 = 8;
pub const ZKM_POSEIDON_PROBE_GROUP3_QUAD: u32 = 9; pub const ZKM_POSEIDON_PROBE_GROUP2: u32 = 10; pub const ZKM_POSEIDON_PROBE_FOLD: u32 = 11;
pub const ZKM_POSEIDON_PROBE_FOLD_TY: u32 = 12; pub const ZKM_POSEIDON_PROBE_SBOX7: u32 = 13; pub const ZKM_POSEIDON_PROBE_SBOX_DELTA: u32 = 14;
pub const ZKM_POSEIDON_PROBE_ADD_RC0: u32 = 15; pub const ZKM_POSEIDON_PROBE_GROUP4: u32 = 17; pub const ZKM_POSEIDON_PROBE_FOLD_WIDE: u32 = 18;
pub const ZKM_TABLE_POSEIDON: c_int = 0; pub const ZKM_TABLE_LOGIC: c_int = 1; pub const ZKM_TABLE_KECCAK_SPONGE: c_int = 2;
pub const ZKM_TABLE_KECCAK: c_int = 3; pub const ZKM_TABLE_MEMORY: c_int = 4; pub const ZKM_TABLE_POSEIDON_SPONGE: c_int = 5;
pub const ZKM_TABLE_SHA_EXTEND: c_int = 6; pub const ZKM_TABLE_SHA_EXTEND_SPONGE: c_int = 7; pub const ZKM_TABLE_SHA_COMPRESS: c_int = 8;
pub const ZKM_TABLE_SHA_COMPRESS_SPONGE: c_int = 9; pub const ZKM_TABLE_ARITHMETIC: c_int = 10; pub const ZKM_TABLE_CPU: c_int = 11;
// width of the MemoryStark table zkm_memory_trace writes (memory/columns.rs)
pub const ZKM_MEMORY_COLS: usize = 13;
// width of the ArithmeticStark table zkm_arithmetic_trace writes (arithmetic/columns.rs)
pub const ZKM_ARITHMETIC_COLS: usize = 54;

#[link(name = "zkmhip")]
extern "C" {
    // context / memory
    pub fn zkm_ctx_create(device: c_int, out: *mut *mut zkm_ctx, err: *mut *mut c_char) -> c_int;
    pub fn zkm_ctx_destroy(ctx: *mut zkm_ctx);
    pub fn zkm_ctx_synchronize(ctx: *mut zkm_ctx, err: *mut *mut c_char) -> c_int;
    pub fn zkm_ctx_stream(ctx: *mut zkm_ctx) -> *mut c_void;
    pub fn zkm_ctx_memory(ctx: *const zkm_ctx, live_bytes: *mut usize, cached_bytes: *mut usize);
    pub fn zkm_ctx_resident_bytes(ctx: *const zkm_ctx) -> usize;
    pub fn zkm_ctx_trim(ctx: *mut zkm_ctx);
    pub fn zkm_ctx_set_tuning(ctx: *mut zkm_ctx, key: *const c_char, value: u64, err: *mut *mut c_char) -> c_int;
    pub fn zkm_dev_alloc(ctx: *mut zkm_ctx, bytes: usize, out: *mut *mut c_void, err: *mut *mut c_char) -> c_int;
    pub fn zkm_dev_free(ctx: *mut zkm_ctx, p: *mut c_void) -> c_int;
    pub fn zkm_dev_upload(ctx: *mut zkm_ctx, dst_dev: *mut c_void, src_host: *const c_void, bytes: usize, err: *mut *mut c_char) -> c_int;
    pub fn zkm_dev_download(ctx: *mut zkm_ctx, dst_host: *mut c_void, src_dev: *const c_void, bytes: usize, err: *mut *mut c_char) -> c_int;
    pub fn zkm_host_alloc(ctx: *mut zkm_ctx, bytes: usize, out: *mut *mut c_void, err: *mut *mut c_char) -> c_int;
    pub fn zkm_host_free(ctx: *mut zkm_ctx, p: *mut c_void) -> c_int;
    pub fn zkm_host_register(ctx: *mut zkm_ctx, p: *mut c_void, bytes: usize, err: *mut *mut c_char) -> c_int;
    pub fn zkm_host_unregister(ctx: *mut zkm_ctx, p: *mut c_void) -> c_int;
    // NTT / PolynomialBatch
    pub fn zkm_ntt(ctx: *mut zkm_ctx, cols: *mut u64, ncols: usize, log_n: c_uint, inverse: c_int, coset_shift: u64, err: *mut *mut c_char) -> c_int;
    pub fn zkm_batch_commit_values(ctx: *mut zkm_ctx, values: *const u64, ncols: usize, log_n: c_uint, rate_bits: c_uint, cap_height: c_uint,
                                   out: *mut *mut zkm_batch, err: *mut *mut c_char) -> c_int;
    pub fn zkm_batch_commit_coeffs(ctx: *mut zkm_ctx, coeffs: *const u64, ncols: usize, log_n: c_uint, rate_bits: c_uint, cap_height: c_uint,
                                   out: *mut *mut zkm_batch, err: *mut *mut c_char) -> c_int;
    pub fn zkm_batch_commit_columns(ctx: *mut zkm_ctx, columns: *const *const u64, ncols: usize, log_n: c_uint, columns_are_values: c_int,
                                    rate_bits: c_uint, cap_height: c_uint, out: *mut *mut zkm_batch, err: *mut *mut c_char) -> c_int;
    pub fn zkm_batch_free(b: *mut zkm_batch);
    pub fn zkm_batch_cap(b: *const zkm_batch, out: *mut u64) -> c_int;
    pub fn zkm_batch_coeffs(b: *const zkm_batch, out: *mut u64) -> c_int;
    pub fn zkm_batch_lde_row(b: *const zkm_batch, natural_index: usize, out: *mut u64) -> c_int;
    pub fn zkm_batch_lde_rows(b: *const zkm_batch, index_start: usize, step: usize, count: usize, out: *mut u64) -> c_int;
    pub fn zkm_batch_leaf(b: *const zkm_batch, leaf_index: usize, out: *mut u64) -> c_int;
    pub fn zkm_batch_merkle_path(b: *const zkm_batch, leaf_index: usize, siblings_out: *mut u64) -> c_int;
    pub fn zkm_batch_digest_layer(b: *const zkm_batch, level: c_uint, out: *mut u64) -> c_int;
    // stacked commitments: nstack same-shaped members in one handle (zkm_eval_openings_stack, zkm_fri_prove_stack)
    pub fn zkm_batch_commit_values_stack(ctx: *mut zkm_ctx, values: *const *const u64, nstack: usize, ncols: usize, log_n: c_uint,
                                         rate_bits: c_uint, cap_height: c_uint, out: *mut *mut zkm_batch, err: *mut *mut c_char) -> c_int;
    pub fn zkm_batch_commit_coeffs_stack(ctx: *mut zkm_ctx, coeffs: *const *const u64, nstack: usize, ncols: usize, log_n: c_uint,
                                         rate_bits: c_uint, cap_height: c_uint, out: *mut *mut zkm_batch, err: *mut *mut c_char) -> c_int;
    pub fn zkm_batch_stack_size(b: *const zkm_batch) -> usize;
    pub fn zkm_batch_stack_cap(b: *const zkm_batch, k: usize, out: *mut u64) -> c_int;
    pub fn zkm_batch_stack_coeffs(b: *const zkm_batch, k: usize, out: *mut u64) -> c_int;
    pub fn zkm_batch_stack_merkle_path(b: *const zkm_batch, k: usize, leaf_index: usize, leaf_out: *mut u64, siblings_out: *mut u64) -> c_int;
    pub fn zkm_field_selftest(ctx: *mut zkm_ctx, a: *const u64, b: *const u64, n: usize, out: *mut u64, err: *mut *mut c_char) -> c_int;
    // hash primitives, witness kernels
    pub fn zkm_poseidon_permute_batch(ctx: *mut zkm_ctx, states: *mut u64, k: usize, err: *mut *mut c_char) -> c_int;
    pub fn zkm_keccakf_batch(ctx: *mut zkm_ctx, states: *mut u64, k: usize, err: *mut *mut c_char) -> c_int;
    /// parity / debug: one piece of the device's Poseidon permutation on chosen words (probe: ZKM_POSEIDON_PROBE_*, arg: see the header)
    pub fn zkm_poseidon_selftest(ctx: *mut zkm_ctx, probe: u32, arg: u32, r#in: *const u64, n: usize, out: *mut u64, err: *mut *mut c_char) -> c_int;
    pub fn zkm_consumer_selftest(ctx: *mut zkm_ctx, alphas: *const u64, nalphas: usize, terms: *const u64, K: usize, n: usize, run: u32, out: *mut u64, err: *mut *mut c_char) -> c_int;
    pub fn zkm_poseidon_trace(ctx: *mut zkm_ctx, seed: u64, num_perms: usize, log_n: c_uint, out_dev: *mut u64, err: *mut *mut c_char) -> c_int;
    pub fn zkm_poseidon_trace_inputs(ctx: *mut zkm_ctx, inputs: *const u64, timestamps: *const u64, num_perms: usize, log_n: c_uint,
                                     out_dev: *mut u64, err: *mut *mut c_char) -> c_int;
    pub fn zkm_poseidon_sponge_trace(ctx: *mut zkm_ctx, inputs: *const u8, input_off: *const u64, meta: *const u64, nops: usize, log_n: c_uint,
                                     out_dev: *mut u64, rows_used_out: *mut usize, err: *mut *mut c_char) -> c_int;
    pub fn zkm_keccak_sponge_trace(ctx: *mut zkm_ctx, inputs: *const u8, input_off: *const u64, meta: *const u64, nops: usize, log_n: c_uint,
                                   out_dev: *mut u64, rows_used_out: *mut usize, err: *mut *mut c_char) -> c_int;
    pub fn zkm_keccak_trace(ctx: *mut zkm_ctx, inputs: *const u64, timestamps: *const u64, nperms: usize, log_n: c_uint, out_dev: *mut u64,
                            err: *mut *mut c_char) -> c_int;
    pub fn zkm_sha_extend_trace(ctx: *mut zkm_ctx, inputs: *const u8, timestamps: *const u64, nrows: usize, log_n: c_uint, out_dev: *mut u64,
                                err: *mut *mut c_char) -> c_int;
    pub fn zkm_sha_extend_sponge_trace(ctx: *mut zkm_ctx, w16: *const u32, meta: *const u64, nblocks: usize, log_n: c_uint, out_dev: *mut u64,
                                       err: *mut *mut c_char) -> c_int;
    pub fn zkm_sha_compress_trace(ctx: *mut zkm_ctx, hx: *const u32, w: *const u32, meta: *const u64, ncomp: usize, log_n: c_uint,
                                  out_dev: *mut u64, err: *mut *mut c_char) -> c_int;
    pub fn zkm_sha_compress_sponge_trace(ctx: *mut zkm_ctx, hx: *const u32, w: *const u32, meta: *const u64, ncomp: usize, log_n: c_uint,
                                         out_dev: *mut u64, err: *mut *mut c_char) -> c_int;
    pub fn zkm_logic_trace(ctx: *mut zkm_ctx, ops: *const u32, nops: usize, log_n: c_uint, out_dev: *mut u64, err: *mut *mut c_char) -> c_int;
    pub fn zkm_memory_trace(ctx: *mut zkm_ctx, ops: *const u64, nops: usize, log_n: c_uint, out_dev: *mut u64, natural_rows_out: *mut usize,
                            err: *mut *mut c_char) -> c_int;
    pub fn zkm_arithmetic_trace(ctx: *mut zkm_ctx, ops: *const u32, nops: usize, log_n: c_uint, out_dev: *mut u64,
                                natural_rows_out: *mut usize, err: *mut *mut c_char) -> c_int;
    // Fiat-Shamir
    pub fn zkm_challenger_init(ch: *mut zkm_challenger);
    pub fn zkm_challenger_observe(ch: *mut zkm_challenger, elems: *const u64, n: usize);
    pub fn zkm_challenger_get(ch: *mut zkm_challenger) -> u64;
    pub fn zkm_challenger_compact(ch: *mut zkm_challenger, state_out: *mut u64);
    // STARK
    pub fn zkm_standard_config(cfg: *mut zkm_stark_config);
    pub fn zkm_table_width(table_id: c_int) -> usize;
    pub fn zkm_table_enum_index(table_id: c_int) -> c_int;
    pub fn zkm_num_lookup_columns(table_id: c_int, cfg: *const zkm_stark_config) -> usize;
    pub fn zkm_proof_words(cfg: *const zkm_stark_config, log_n: c_uint, ncols: usize, naux: usize, nctl_zs: usize) -> usize;
    pub fn zkm_proof_get_layout(proof: *const u64, out: *mut zkm_proof_layout) -> c_int;
    pub fn zkm_proof_get_query_layout(proof: *const u64, out: *mut zkm_proof_query_layout) -> c_int;
    pub fn zkm_prove_single_table(ctx: *mut zkm_ctx, table_id: c_int, cfg: *const zkm_stark_config, trace: *const u64, ncols: usize,
                                  log_n: c_uint, trace_batch: *const zkm_batch, aux: *const u64, naux: usize, num_helpers: *const u32,
                                  nctl_zs: usize, challenger: *mut zkm_challenger, proof_out: *mut u64, err: *mut *mut c_char) -> c_int;
    pub fn zkm_prove_single_table_ctl(ctx: *mut zkm_ctx, table_id: c_int, cfg: *const zkm_stark_config, trace: *const u64, ncols: usize,
                                      log_n: c_uint, trace_batch: *const zkm_batch, aux: *const u64, naux: usize, table: *const zkm_ctl_table,
                                      zs: *const zkm_ctl_z, colset_ids: *const u32, nzs: usize, lookup_challenges: *const u64,
                                      challenger: *mut zkm_challenger, proof_out: *mut u64, err: *mut *mut c_char) -> c_int;
    pub fn zkm_ctl_data(ctx: *mut zkm_ctx, table: *const zkm_ctl_table, zs: *const zkm_ctl_z, colset_ids: *const u32, nzs: usize,
                        trace: *const u64, ncols: usize, log_n: c_uint, aux_out: *mut u64, err: *mut *mut c_char) -> c_int;
    pub fn zkm_lookup_helper_columns(ctx: *mut zkm_ctx, table: *const zkm_ctl_table, colset_ids: *const u32, nlookup: usize, table_col: u32,
                                     freq_col: u32, challenge: u64, trace: *const u64, ncols: usize, log_n: c_uint, out: *mut u64,
                                     err: *mut *mut c_char) -> c_int;
    pub fn zkm_all_proof_words(cfg: *const zkm_stark_config, tables: *const zkm_table_input, ntables: usize, ctls: *const zkm_cross_table_lookup,
                               sides: *const zkm_ctl_side, nctls: usize, proof_offsets_out: *mut usize) -> usize;
    pub fn zkm_prove_with_traces(ctx: *mut zkm_ctx, cfg: *const zkm_stark_config, tables: *const zkm_table_input, ntables: usize,
                                 ctls: *const zkm_cross_table_lookup, sides: *const zkm_ctl_side, nctls: usize, public_values: *const u64,
                                 npublic: usize, proofs_out: *mut u64, ctl_challenges_out: *mut u64, err: *mut *mut c_char) -> c_int;
    pub fn zkm_all_stark_ctls(ctls_out: *mut *const zkm_cross_table_lookup, nctls_out: *mut usize, sides_out: *mut *const zkm_ctl_side,
                              nsides_out: *mut usize) -> c_int;
    pub fn zkm_all_stark_ctl_table(table_id: c_int) -> *const zkm_ctl_table;
    pub fn zkm_prove_segment(ctx: *mut zkm_ctx, cfg: *const zkm_stark_config, traces: *const *const u64, log_n: *const c_uint,
                             public_values: *const u64, npublic: usize, proofs_out: *mut u64, proof_offsets_out: *mut usize,
                             ctl_challenges_out: *mut u64, err: *mut *mut c_char) -> c_int;
    pub fn zkm_prove_segment_columns(ctx: *mut zkm_ctx, cfg: *const zkm_stark_config, columns: *const *const *const u64, log_n: *const c_uint,
                                     public_values: *const u64, npublic: usize, proofs_out: *mut u64, proof_offsets_out: *mut usize,
                                     ctl_challenges_out: *mut u64, err: *mut *mut c_char) -> c_int;
    // K independent segments in lock-step (include/zkm_hip.h): traces[s][t] / columns[s][t][i], log_n[s][t], one output buffer per segment
    pub fn zkm_prove_segments(ctx: *mut zkm_ctx, cfg: *const zkm_stark_config, nseg: usize, traces: *const *const *const u64,
                              log_n: *const *const c_uint, public_values: *const *const u64, npublic: *const usize, proofs_out: *const *mut u64,
                              ctl_challenges_out: *const *mut u64, err: *mut *mut c_char) -> c_int;
    pub fn zkm_prove_segments_columns(ctx: *mut zkm_ctx, cfg: *const zkm_stark_config, nseg: usize, columns: *const *const *const *const u64,
                                      log_n: *const *const c_uint, public_values: *const *const u64, npublic: *const usize,
                                      proofs_out: *const *mut u64, ctl_challenges_out: *const *mut u64, err: *mut *mut c_char) -> c_int;
    // staged traces: the next proof's upload behind the current proof (copy streams; returns at once)
    pub fn zkm_trace_stage(ctx: *mut zkm_ctx, values: *const u64, ncols: usize, log_n: c_uint, canonical: c_int, out: *mut *mut zkm_staged,
                           err: *mut *mut c_char) -> c_int;
    pub fn zkm_trace_stage_columns(ctx: *mut zkm_ctx, columns: *const *const u64, ncols: usize, log_n: c_uint, canonical: c_int,
                                   out: *mut *mut zkm_staged, err: *mut *mut c_char) -> c_int;
    pub fn zkm_segment_stage(ctx: *mut zkm_ctx, traces: *const *const u64, log_n: *const c_uint, canonical: c_int, out: *mut *mut zkm_staged,
                             err: *mut *mut c_char) -> c_int;
    pub fn zkm_segment_stage_columns(ctx: *mut zkm_ctx, columns: *const *const *const u64, log_n: *const c_uint, canonical: c_int,
                                     out: *mut *mut zkm_staged, err: *mut *mut c_char) -> c_int;
    pub fn zkm_staged_segment_ptrs(staged: *mut zkm_staged, ptrs_out: *mut *const u64) -> c_int;
    pub fn zkm_staged_ptr(staged: *mut zkm_staged) -> *const u64;
    pub fn zkm_staged_ready(staged: *mut zkm_staged, wait: c_int) -> c_int;
    pub fn zkm_staged_free(staged: *mut zkm_staged);
    // a whole segment from its raw operations: the twelve tables in one device block (Traces::into_tables), or proven at once
    pub fn zkm_segment_tables(ctx: *mut zkm_ctx, cfg: *const zkm_stark_config, ops: *const zkm_segment_ops, log_n_out: *mut c_uint,
                              out: *mut *mut zkm_staged, err: *mut *mut c_char) -> c_int;
    pub fn zkm_prove_segment_ops(ctx: *mut zkm_ctx, cfg: *const zkm_stark_config, ops: *const zkm_segment_ops, public_values: *const u64,
                                 npublic: usize, proofs_out: *mut u64, proof_offsets_out: *mut usize, ctl_challenges_out: *mut u64,
                                 err: *mut *mut c_char) -> c_int;
    // K segments from their raw operations: every generation kernel launched once for all K, three host waits, lock-step proofs
    pub fn zkm_segments_tables(ctx: *mut zkm_ctx, cfg: *const zkm_stark_config, nseg: usize, ops: *const zkm_segment_ops, log_n_out: *mut c_uint,
                               out: *mut *mut zkm_staged, err: *mut *mut c_char) -> c_int;
    pub fn zkm_prove_segments_ops(ctx: *mut zkm_ctx, cfg: *const zkm_stark_config, nseg: usize, ops: *const zkm_segment_ops,
                                  public_values: *const *const u64, npublic: *const usize, proofs_out: *const *mut u64,
                                  proof_offsets_out: *mut usize, ctl_challenges_out: *const *mut u64, err: *mut *mut c_char) -> c_int;
    // the same calls with each segment's bootstrap kernel built from its image in front of the caller's lists
    pub fn zkm_boot_counts(image: *const zkm_boot_image, cpu_rows: *mut usize, memory_ops: *mut usize, poseidon_inputs: *mut usize,
                           sponge_ops: *mut usize, sponge_rows: *mut usize);
    pub fn zkm_segment_tables_boot(ctx: *mut zkm_ctx, cfg: *const zkm_stark_config, image: *const zkm_boot_image, ops: *const zkm_segment_ops,
                                   log_n_out: *mut c_uint, out: *mut *mut zkm_staged, err: *mut *mut c_char) -> c_int;
    pub fn zkm_segments_tables_boot(ctx: *mut zkm_ctx, cfg: *const zkm_stark_config, nseg: usize, images: *const zkm_boot_image,
                                    ops: *const zkm_segment_ops, log_n_out: *mut c_uint, out: *mut *mut zkm_staged, err: *mut *mut c_char) -> c_int;
    pub fn zkm_prove_segment_ops_boot(ctx: *mut zkm_ctx, cfg: *const zkm_stark_config, image: *const zkm_boot_image, ops: *const zkm_segment_ops,
                                      public_values: *const u64, npublic: usize, proofs_out: *mut u64, proof_offsets_out: *mut usize,
                                      ctl_challenges_out: *mut u64, err: *mut *mut c_char) -> c_int;
    pub fn zkm_prove_segments_ops_boot(ctx: *mut zkm_ctx, cfg: *const zkm_stark_config, nseg: usize, images: *const zkm_boot_image,
                                       ops: *const zkm_segment_ops, public_values: *const *const u64, npublic: *const usize,
                                       proofs_out: *const *mut u64, proof_offsets_out: *mut usize, ctl_challenges_out: *const *mut u64,
                                       err: *mut *mut c_char) -> c_int;
    pub fn zkm_boot_witness(ctx: *mut zkm_ctx, image: *const zkm_boot_image, cpu_rows_out: *mut u64, memory_ops_out: *mut u64,
                            poseidon_inputs_out: *mut u64, poseidon_ts_out: *mut u64, digests_out: *mut u64, err: *mut *mut c_char) -> c_int;
    // the same calls with the CPU rows built on the device from a compact step log
    pub fn zkm_cpu_steps_counts(steps: *const zkm_cpu_steps, memory_ops: *mut usize, logic_ops: *mut usize, arithmetic_ops: *mut usize,
                                err: *mut *mut c_char) -> c_int;
    pub fn zkm_cpu_witness(ctx: *mut zkm_ctx, steps: *const zkm_cpu_steps, first_clock: u64, log_n: c_uint, cpu_out_dev: *mut u64,
                           memory_ops_out_dev: *mut u64, logic_ops_out_dev: *mut u32, arithmetic_ops_out_dev: *mut u32,
                           err: *mut *mut c_char) -> c_int;
    pub fn zkm_segments_tables_steps(ctx: *mut zkm_ctx, cfg: *const zkm_stark_config, nseg: usize, images: *const zkm_boot_image,
                                     steps: *const zkm_cpu_steps, ops: *const zkm_segment_ops, log_n_out: *mut c_uint,
                                     out: *mut *mut zkm_staged, err: *mut *mut c_char) -> c_int;
    pub fn zkm_prove_segments_ops_steps(ctx: *mut zkm_ctx, cfg: *const zkm_stark_config, nseg: usize, images: *const zkm_boot_image,
                                        steps: *const zkm_cpu_steps, ops: *const zkm_segment_ops, public_values: *const *const u64,
                                        npublic: *const usize, proofs_out: *const *mut u64, proof_offsets_out: *mut usize,
                                        ctl_challenges_out: *const *mut u64, err: *mut *mut c_char) -> c_int;
    // steps staged ahead of a call and walked on the device (the handle is an address, as the header passes it)
    pub fn zkm_cpu_steps_scan(ctx: *mut zkm_ctx, nseg: usize, steps: *const zkm_cpu_steps, counts_out: *mut usize, base_out: *const *mut u32,
                              err: *mut *mut c_char) -> c_int;
    pub fn zkm_cpu_steps_stage(ctx: *mut zkm_ctx, nseg: usize, steps: *const zkm_cpu_steps, out: *mut *mut c_void, err: *mut *mut c_char) -> c_int;
    pub fn zkm_staged_steps_ready(staged: *mut c_void, wait: c_int) -> c_int;
    pub fn zkm_staged_steps_get(staged: *mut c_void, segment: usize, steps_out: *mut zkm_cpu_steps, memory_ops: *mut usize, logic_ops: *mut usize,
                                arithmetic_ops: *mut usize, err: *mut *mut c_char) -> c_int;
    pub fn zkm_staged_steps_free(staged: *mut c_void);
    // SHA-256 precompile calls expanded on the device from the sponge tables' lists: counts, the RAW records with their clocks, the kernel
    pub fn zkm_sha_calls_counts(nextend: usize, ncompress: usize, cpu_rows: *mut usize, memory_ops: *mut usize, logic_ops: *mut usize,
                                sha_extend_rows: *mut usize);
    pub fn zkm_sha_calls_steps(extend_meta: *const u64, nextend: usize, compress_meta: *const u64, ncompress: usize, raw_base: usize,
                               steps_out: *mut zkm_cpu_step, clocks_out: *mut u64, err: *mut *mut c_char) -> c_int;
    pub fn zkm_sha_calls_witness(ctx: *mut zkm_ctx, extend_w16: *const u32, extend_meta: *const u64, nextend: usize, compress_hx: *const u32,
                                 compress_w: *const u32, compress_meta: *const u64, ncompress: usize, raw_rows_out_dev: *mut u64,
                                 memory_ops_out_dev: *mut u64, logic_ops_out_dev: *mut u32, sha_extend_inputs_out_dev: *mut u8,
                                 sha_extend_timestamps_out_dev: *mut u64, err: *mut *mut c_char) -> c_int;
    // SYSKECCAK precompile calls expanded on the device from the KeccakSponge table's lists (meta flagged ZKM_SPONGE_BYTE_ADDRESSED)
    pub fn zkm_keccak_calls_counts(input_off: *const u64, ncalls: usize, cpu_rows: *mut usize, memory_ops: *mut usize, logic_ops: *mut usize,
                                   keccak_perms: *mut usize, err: *mut *mut c_char) -> c_int;
    pub fn zkm_keccak_calls_counts_meta(input_off: *const u64, meta: *const u64, ncalls: usize, cpu_rows: *mut usize, memory_ops: *mut usize,
                                        logic_ops: *mut usize, keccak_perms: *mut usize, err: *mut *mut c_char) -> c_int;
    pub fn zkm_keccak_calls_steps(input_off: *const u64, meta: *const u64, ncalls: usize, raw_base: usize, steps_out: *mut zkm_cpu_step,
                                  clocks_out: *mut u64, err: *mut *mut c_char) -> c_int;
    pub fn zkm_keccak_calls_witness(ctx: *mut zkm_ctx, inputs: *const u8, input_off: *const u64, meta: *const u64, digest_addrs: *const u64,
                                    ncalls: usize, raw_rows_out_dev: *mut u64, memory_ops_out_dev: *mut u64, logic_ops_out_dev: *mut u32,
                                    keccak_inputs_out_dev: *mut u64, keccak_timestamps_out_dev: *mut u64, err: *mut *mut c_char) -> c_int;
    // the I/O syscalls' rows (hint read, commit, verify, preimage) expanded on the device from the bytes each call moves
    pub fn zkm_io_calls_counts(kinds: *const u32, data_off: *const u64, ncalls: usize, cpu_rows: *mut usize, memory_ops: *mut usize,
                               err: *mut *mut c_char) -> c_int;
    pub fn zkm_io_calls_steps(kinds: *const u32, data_off: *const u64, meta: *const u64, ncalls: usize, raw_base: usize,
                              steps_out: *mut zkm_cpu_step, clocks_out: *mut u64, err: *mut *mut c_char) -> c_int;
    pub fn zkm_io_calls_witness(ctx: *mut zkm_ctx, kinds: *const u32, data: *const u8, data_off: *const u64, meta: *const u64, ncalls: usize,
                                raw_rows_out_dev: *mut u64, err: *mut *mut c_char) -> c_int;
    // the rows of the instructions no step kind takes (LUI, MUL, the hi/lo kinds and moves, SDC1, SYNC, PREF) expanded on the device
    pub fn zkm_insn_rows_counts(insns: *const zkm_cpu_step, ninsns: usize, memory_ops: *mut usize, arithmetic_ops: *mut usize,
                                err: *mut *mut c_char) -> c_int;
    pub fn zkm_insn_rows_steps(insns: *const zkm_cpu_step, ninsns: usize, raw_base: usize, steps_out: *mut zkm_cpu_step,
                               err: *mut *mut c_char) -> c_int;
    pub fn zkm_insn_rows_witness(ctx: *mut zkm_ctx, insns: *const zkm_cpu_step, clocks: *const u64, ninsns: usize, raw_rows_out_dev: *mut u64,
                                 arithmetic_ops_out_dev: *mut u32, err: *mut *mut c_char) -> c_int;
    // K segments' calls expanded in one set of launches: the host half, the expansion with its handle, and the two calls that run the
    // builder behind it (calls: *const ZkmSegmentCalls, nseg of them; expanded / *out: *mut ZkmExpandedCalls)
    pub fn zkm_segment_calls_steps(calls: *const c_void, steps_out: *mut zkm_cpu_step, counts_out: *mut usize, err: *mut *mut c_char) -> c_int;
    pub fn zkm_segments_calls_expand(ctx: *mut zkm_ctx, nseg: usize, calls: *const c_void, out: *mut *mut c_void, err: *mut *mut c_char) -> c_int;
    pub fn zkm_expanded_calls_get(expanded: *const c_void, segment: usize, steps_out: *mut zkm_cpu_steps, ops_out: *mut zkm_segment_ops) -> c_int;
    pub fn zkm_expanded_calls_free(expanded: *mut c_void);
    pub fn zkm_segments_tables_calls(ctx: *mut zkm_ctx, cfg: *const zkm_stark_config, nseg: usize, images: *const zkm_boot_image,
                                     calls: *const c_void, log_n_out: *mut c_uint, out: *mut *mut zkm_staged, err: *mut *mut c_char) -> c_int;
    pub fn zkm_prove_segments_ops_calls(ctx: *mut zkm_ctx, cfg: *const zkm_stark_config, nseg: usize, images: *const zkm_boot_image,
                                        calls: *const c_void, public_values: *const *const u64, npublic: *const usize,
                                        proofs_out: *const *mut u64, proof_offsets_out: *mut usize, ctl_challenges_out: *const *mut u64,
                                        err: *mut *mut c_char) -> c_int;
    // the same calls staged behind the current proofs: expanded, placed and walked on the device (staged / *out: an address)
    pub fn zkm_segments_calls_stage(ctx: *mut zkm_ctx, nseg: usize, calls: *const c_void, images: *const zkm_boot_image, out: *mut *mut c_void,
                                    err: *mut *mut c_char) -> c_int;
    pub fn zkm_staged_calls_ready(staged: *mut c_void, wait: c_int) -> c_int;
    pub fn zkm_staged_calls_get(staged: *mut c_void, segment: usize, steps_out: *mut zkm_cpu_steps, ops_out: *mut zkm_segment_ops,
                                image_out: *mut zkm_boot_image, err: *mut *mut c_char) -> c_int;
    pub fn zkm_staged_calls_free(staged: *mut c_void);
    // what the emulator hashes between two segments: hash pages, root and image id of a memory image
    pub fn zkm_image_hash_plan(dirty_index: *const u32, ndirty: usize, hash_index_out: *mut u32, capacity: usize) -> usize;
    pub fn zkm_image_hash(ctx: *mut zkm_ctx, r#in: *const zkm_image_pages, hash_words_out: *mut u32, page_hash_root_out: *mut u8,
                          image_id_out: *mut u8, err: *mut *mut c_char) -> c_int;
    pub fn zkm_images_hash(ctx: *mut zkm_ctx, nimg: usize, r#in: *const zkm_image_pages, hash_words_out: *const *mut u32,
                           page_hash_roots_out: *mut u8, image_ids_out: *mut u8, err: *mut *mut c_char) -> c_int;
    pub fn zkm_ctx_host_waits(ctx: *const zkm_ctx) -> u64;
    // staged operations: the next call's lists uploaded behind the current proofs
    pub fn zkm_segment_ops_stage(ctx: *mut zkm_ctx, ops: *const zkm_segment_ops, out: *mut *mut zkm_staged_ops, err: *mut *mut c_char) -> c_int;
    pub fn zkm_staged_ops_get(staged: *mut zkm_staged_ops, ops_out: *mut zkm_segment_ops) -> c_int;
    pub fn zkm_staged_ops_ready(staged: *mut zkm_staged_ops, wait: c_int) -> c_int;
    pub fn zkm_staged_ops_free(staged: *mut zkm_staged_ops);
    // one process, many GPUs: contexts_per_device contexts on each device, one worker thread per context, groups of <= max_stack segments
    pub fn zkm_pool_create(devices: *const c_int, ndevices: usize, contexts_per_device: usize, out: *mut *mut zkm_pool, err: *mut *mut c_char) -> c_int;
    pub fn zkm_pool_destroy(pool: *mut zkm_pool);
    pub fn zkm_pool_workers(pool: *const zkm_pool) -> usize;
    pub fn zkm_pool_context(pool: *mut zkm_pool, worker: usize) -> *mut zkm_ctx;
    pub fn zkm_pool_device(pool: *const zkm_pool, worker: usize) -> c_int;
    pub fn zkm_pool_set_tuning(pool: *mut zkm_pool, key: *const c_char, value: u64, err: *mut *mut c_char) -> c_int;
    pub fn zkm_pool_prove_segments(pool: *mut zkm_pool, cfg: *const zkm_stark_config, nseg: usize, max_stack: usize,
                                   traces: *const *const *const u64, log_n: *const *const c_uint, public_values: *const *const u64,
                                   npublic: *const usize, proofs_out: *const *mut u64, ctl_challenges_out: *const *mut u64,
                                   err: *mut *mut c_char) -> c_int;
    pub fn zkm_pool_prove_segments_columns(pool: *mut zkm_pool, cfg: *const zkm_stark_config, nseg: usize, max_stack: usize,
                                           columns: *const *const *const *const u64, log_n: *const *const c_uint,
                                           public_values: *const *const u64, npublic: *const usize, proofs_out: *const *mut u64,
                                           ctl_challenges_out: *const *mut u64, err: *mut *mut c_char) -> c_int;
    pub fn zkm_pool_prove_segments_ops(pool: *mut zkm_pool, cfg: *const zkm_stark_config, nseg: usize, max_stack: usize,
                                       ops: *const zkm_segment_ops, public_values: *const *const u64, npublic: *const usize,
                                       proofs_out: *const *mut u64, proof_offsets_out: *mut usize, ctl_challenges_out: *const *mut u64,
                                       err: *mut *mut c_char) -> c_int;
    pub fn zkm_pool_prove_segments_calls(pool: *mut zkm_pool, cfg: *const zkm_stark_config, nseg: usize, max_stack: usize,
                                         images: *const zkm_boot_image, calls: *const c_void, public_values: *const *const u64,
                                         npublic: *const usize, proofs_out: *const *mut u64, proof_offsets_out: *mut usize,
                                         ctl_challenges_out: *const *mut u64, err: *mut *mut c_char) -> c_int;
    pub fn zkm_pool_plan(nseg: usize, workers: usize, max_stack: usize, group_sizes_out: *mut usize, capacity: usize) -> usize;
    pub fn zkm_pool_last_assignment(pool: *const zkm_pool, segment: usize, worker_out: *mut usize, group_out: *mut usize) -> c_int;
    pub fn zkm_prove_single_tables(ctx: *mut zkm_ctx, table_id: c_int, cfg: *const zkm_stark_config, nproofs: usize, traces: *const *const u64,
                                   ncols: usize, log_n: c_uint, aux: *const *const u64, naux: usize, num_helpers: *const u32, nctl_zs: usize,
                                   challengers: *const *mut zkm_challenger, proofs_out: *const *mut u64, err: *mut *mut c_char) -> c_int;
    pub fn zkm_fri_proof_words(cfg: *const zkm_stark_config, log_n: c_uint, oracle_cols: *const usize, noracles: usize) -> usize;
    pub fn zkm_fri_prove(ctx: *mut zkm_ctx, cfg: *const zkm_stark_config, oracles: *const *const zkm_batch, noracles: usize,
                         batches: *const zkm_fri_batch, nbatches: usize, challenger: *mut zkm_challenger, proof_out: *mut u64,
                         err: *mut *mut c_char) -> c_int;
    pub fn zkm_fri_prove_stack(ctx: *mut zkm_ctx, cfg: *const zkm_stark_config, oracles: *const *const zkm_batch, noracles: usize,
                               batches: *const zkm_fri_batch, nbatches: usize, points: *const u64, challengers: *const *mut zkm_challenger,
                               proofs_out: *const *mut u64, err: *mut *mut c_char) -> c_int;
    pub fn zkm_prove_openings(ctx: *mut zkm_ctx, cfg: *const zkm_stark_config, trace_batch: *const zkm_batch, aux_batch: *const zkm_batch,
                              quot_batch: *const zkm_batch, nctl_zs: usize, challenger: *mut zkm_challenger, proof_out: *mut u64,
                              err: *mut *mut c_char) -> c_int;
    pub fn zkm_segment_image_words(tables: *const zkm_table_input, ntables: usize, ctls: *const zkm_cross_table_lookup, sides: *const zkm_ctl_side,
                                   nctls: usize, npublic: usize) -> usize;
    pub fn zkm_segment_image_write(tables: *const zkm_table_input, ntables: usize, ctls: *const zkm_cross_table_lookup, sides: *const zkm_ctl_side,
                                   nctls: usize, public_values: *const u64, npublic: usize, image_out: *mut u64, err: *mut *mut c_char) -> c_int;
    pub fn zkm_prove_segment_image(ctx: *mut zkm_ctx, cfg: *const zkm_stark_config, image: *const u64, image_words: usize, proofs_out: *mut u64,
                                   proof_words_out: *mut usize, proof_offsets_out: *mut usize, ctl_challenges_out: *mut u64,
                                   err: *mut *mut c_char) -> c_int;
    pub fn zkm_quotient(ctx: *mut zkm_ctx, table_id: c_int, trace: *const zkm_batch, aux: *const zkm_batch, num_helpers: *const u32, nctl_zs: usize,
                        alphas: *const u64, nalphas: usize, out_coeffs: *mut u64, err: *mut *mut c_char) -> c_int;
    pub fn zkm_eval_openings(ctx: *mut zkm_ctx, b: *const zkm_batch, zeta: *const u64, out: *mut u64, err: *mut *mut c_char) -> c_int;
    pub fn zkm_eval_openings_stack(ctx: *mut zkm_ctx, b: *const zkm_batch, zetas: *const u64, out: *mut u64, err: *mut *mut c_char) -> c_int;
    // check_constraints (prover.rs:793-910): debugging aid, rc != 0 + "Constraint failed in <Stark>" and the first failing row
    // check_ctls (cross_table_lookup.rs:1486-1581) on the device: every lookup's looking multiset against its looked multiset
    pub fn zkm_check_ctls(ctx: *mut zkm_ctx, tables: *const zkm_table_input, ntables: usize, ctls: *const zkm_cross_table_lookup,
                          sides: *const zkm_ctl_side, nctls: usize, report: *mut zkm_ctl_report, err: *mut *mut c_char) -> c_int;
    pub fn zkm_segment_check_ctls(ctx: *mut zkm_ctx, traces: *const *const u64, log_n: *const c_uint, report: *mut zkm_ctl_report,
                                  err: *mut *mut c_char) -> c_int;
    // each table's own constraints on every row of the trace, from the trace alone: rc != 0 + "Constraint failed in <Stark>: row r, constraint
    // i of N = 0x.. (m of n rows fail)" and the finding(s), ZKM_WITNESS_FINDING_WORDS words a table (witness_check_hip.rs)
    pub fn zkm_witness_check(ctx: *mut zkm_ctx, table_id: c_int, trace: *const u64, ncols: usize, log_n: c_uint, finding: *mut u64,
                             err: *mut *mut c_char) -> c_int;
    pub fn zkm_segment_witness_check(ctx: *mut zkm_ctx, traces: *const *const u64, log_n: *const c_uint, findings: *mut u64,
                                     err: *mut *mut c_char) -> c_int;
    // each table's own range-check lookups from the trace alone: rc != 0 + "Lookup failed in <Stark>: lookup l: value 0x.. is looked up a
    // times (..) and has frequency 0x.. in k table rows (..); m values fail" and the finding(s), ZKM_LOOKUP_FINDING_WORDS words a table
    // (lookup_check_hip.rs)
    pub fn zkm_lookup_check(ctx: *mut zkm_ctx, table_id: c_int, trace: *const u64, ncols: usize, log_n: c_uint, finding: *mut u64,
                            err: *mut *mut c_char) -> c_int;
    pub fn zkm_segment_lookup_check(ctx: *mut zkm_ctx, traces: *const *const u64, log_n: *const c_uint, findings: *mut u64,
                                    err: *mut *mut c_char) -> c_int;
    // the three checks on nseg segments in one set of launches and two host waits: rc != 0 + "zkm_segments_check: segment s: " and the
    // owning check's message; verdicts ZKM_SEGMENT_VERDICT_WORDS words a segment (segment_check_hip.rs)
    pub fn zkm_segments_check(ctx: *mut zkm_ctx, nseg: usize, traces: *const *const *const u64, log_n: *const *const c_uint, verdicts: *mut u64,
                              witness_findings: *mut u64, lookup_findings: *mut u64, ctl_reports: *mut zkm_ctl_report,
                              err: *mut *mut c_char) -> c_int;
    pub fn zkm_segment_check(ctx: *mut zkm_ctx, traces: *const *const u64, log_n: *const c_uint, verdict: *mut u64, witness_findings: *mut u64,
                             lookup_findings: *mut u64, ctl_report: *mut zkm_ctl_report, err: *mut *mut c_char) -> c_int;
    // verify_proof (verifier.rs:27-176) on the device: the general form, K AllStark segments, and the mirror of zkm_prove_single_table
    pub fn zkm_verify_proofs(ctx: *mut zkm_ctx, cfg: *const zkm_stark_config, tables: *const zkm_table_input, ntables: usize,
                             ctls: *const zkm_cross_table_lookup, sides: *const zkm_ctl_side, nctls: usize, public_values: *const u64,
                             npublic: usize, proofs: *const u64, proof_words: usize, ctl_challenges: *const u64, report: *mut zkm_verify_report,
                             err: *mut *mut c_char) -> c_int;
    pub fn zkm_verify_segments(ctx: *mut zkm_ctx, cfg: *const zkm_stark_config, nseg: usize, proofs: *const *const u64, proof_words: *const usize,
                               public_values: *const *const u64, npublic: *const usize, ctl_challenges: *const *const u64,
                               reports: *mut zkm_verify_report, err: *mut *mut c_char) -> c_int;
    pub fn zkm_verify_single_table(ctx: *mut zkm_ctx, table_id: c_int, cfg: *const zkm_stark_config, proof: *const u64, proof_words: usize,
                                   ncols: usize, naux: usize, num_helpers: *const u32, nctl_zs: usize, challenger: *mut zkm_challenger,
                                   report: *mut zkm_verify_report, err: *mut *mut c_char) -> c_int;
    pub fn zkm_fri_verify(ctx: *mut zkm_ctx, cfg: *const zkm_stark_config, nproofs: usize, proofs: *const *const u64, proof_words: *const usize,
                          log_n: *const c_uint, oracle_cols: *const *const usize, noracles: *const usize, oracle_caps: *const *const *const u64,
                          batches: *const *const zkm_fri_batch, nbatches: *const usize, opened: *const *const *const u64,
                          challengers: *const *mut zkm_challenger, reports: *mut zkm_verify_report, err: *mut *mut c_char) -> c_int;
    pub fn zkm_check_constraints(ctx: *mut zkm_ctx, table_id: c_int, cfg: *const zkm_stark_config, trace: *const u64, ncols: usize, log_n: c_uint,
                                 aux: *const u64, naux: usize, table: *const zkm_ctl_table, zs: *const zkm_ctl_z, colset_ids: *const u32,
                                 nzs: usize, lookup_challenges: *const u64, alphas: *const u64, nalphas: usize, first_failing_row: *mut u64,
                                 err: *mut *mut c_char) -> c_int;
    // profiling
    pub fn zkm_profile_enable(ctx: *mut zkm_ctx, on: c_int);
    pub fn zkm_profile_reset(ctx: *mut zkm_ctx);
    pub fn zkm_profile_count(ctx: *mut zkm_ctx) -> usize;
    pub fn zkm_profile_get(ctx: *mut zkm_ctx, i: usize, name: *mut *const c_char, launches: *mut u64, total_ms: *mut c_double) -> c_int;
    pub fn zkm_version() -> *const c_char;
}

/// words of one finding of zkm_witness_check / zkm_segment_witness_check: row (all ones: every constraint holds), index of the first nonzero
/// constraint on that row, its canonical value, rows with a nonzero constraint, constraints a row emits
pub const ZKM_WITNESS_FINDING_WORDS: usize = 5;
/// words of one finding of zkm_lookup_check / zkm_segment_lookup_check: failing lookup (all ones: every lookup holds), the value, its looking
/// count, its frequency, its table rows, column and row of its first looking cell, its first table row, the unbalanced values
pub const ZKM_LOOKUP_FINDING_WORDS: usize = 9;
/// words of one segment's verdict of zkm_segments_check / zkm_segment_check: the kind of its first finding (0 consistent, 1 a table
/// constraint, 2 a range-check lookup, 3 a cross-table lookup), then the failing table's position in Table::all() or the lookup's index
pub const ZKM_SEGMENT_VERDICT_WORDS: usize = 2;

/// status + message -> anyhow::Error; the message is released with free() like recursion/src/snark/snarks.rs:55-57
pub fn check(rc: c_int, err: *mut c_char) -> anyhow::Result<()> {
    if rc == 0 {
        return Ok(());
    }
    let msg = if err.is_null() { format!("libzkmhip error {rc}") } else { unsafe { std::ffi::CStr::from_ptr(err).to_string_lossy().into_owned() } };
    if !err.is_null() {
        unsafe { libc::free(err as *mut c_void) };
    }
    Err(anyhow::anyhow!(msg))
}
