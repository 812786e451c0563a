/* include/zkm_hip.h -- C ABI of libzkmhip.so: the MI355X (gfx950) STARK/FRI hot path of the zkMIPS prover.
 *
 * This is the drop-in boundary.  The reference (zkMIPS/zkm @ 2025-04-04) has no FFI on this path: the
 * prover calls the un-vendored plonky2 fork (prover/Cargo.toml:17-20) through Rust generics.  Each entry
 * point below names the reference call site / plonky2 item it replaces; INTEGRATION.md shows the
 * `extern "C"` block a patched plonky2 / zkm-prover would bind.  Error convention follows the reference's
 * only existing FFI (recursion/src/snark/snarks.rs:7-20, 39-59): int status (0 = ok) + optional
 * malloc'd message in *err that the caller releases with free().
 * What holds for every export: no C++ exception and no crash from a null handle crosses the boundary.  A
 * null zkm_ctx / zkm_batch / zkm_staged / zkm_pool is status 1 (with "<function>: null argument" where
 * there is an err), a no-op for destroy / free, 0 or NULL for size- and pointer-returning functions;
 * zkm_staged_ready keeps 1 / 0 / -1 and zkm_pool_device -1.  A failed call releases what it allocated,
 * and a failed prove call leaves the caller's challenger untouched.
 *
 * Data conventions
 *   - field element: canonical uint64_t (< p = 2^64 - 2^32 + 1); F2 = F[X]/(X^2-7) as [c0, c1].
 *   - matrices are column-major: element (row r, column c) of an n-row matrix is at c*n + r -- the layout
 *     of Vec<PolynomialValues<F>> flattened (prover/src/util.rs:37-46).
 *   - every data pointer may be a host pointer or a device (HBM) pointer of the context's GPU; the
 *     library detects which (hipPointerGetAttributes).  Output buffers documented "host" must be host.
 *   - a zkm_ctx is single-owner (one per GPU, driven from one thread at a time), like the reference's
 *     `&mut Challenger` / `&mut TimingTree` threading (prover.rs:441-450).
 */
#ifndef ZKM_HIP_H
#define ZKM_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct zkm_ctx zkm_ctx;
typedef struct zkm_batch zkm_batch;

/* ------------------------------------------------------------------ context / memory */
int zkm_ctx_create(int device, zkm_ctx** out, char** err);
void zkm_ctx_destroy(zkm_ctx* ctx);
int zkm_ctx_synchronize(zkm_ctx* ctx, char** err);
/* times a host thread has waited for this context's stream since it was created (the calls that promise a number of waits are
 * checked by the difference around them) */
uint64_t zkm_ctx_host_waits(const zkm_ctx* ctx);
/* the hipStream_t every kernel of this context is launched on (for event timing by the host) */
void* zkm_ctx_stream(zkm_ctx* ctx);
/* Device memory held by the context's caching allocator: bytes in live allocations (DeviceBuffers, batches, scratch of a call in
 * flight) and bytes cached for reuse (freed on zkm_ctx_destroy, or when an allocation would otherwise fail). */
void zkm_ctx_memory(const zkm_ctx* ctx, size_t* live_bytes, size_t* cached_bytes);
/* Of the live bytes: tables the context keeps for reuse (twiddles, coset power tables, block twiddles -- also those of its commit
 * lanes, which build their own on first use).  live - resident == 0 between calls when the caller holds no buffers or batches. */
size_t zkm_ctx_resident_bytes(const zkm_ctx* ctx);
/* Return every cached (not live) block to the device (the free lists are exact-size: a segment of many table shapes leaves one
 * cached block per distinct size behind). */
void zkm_ctx_trim(zkm_ctx* ctx);
/* Size thresholds at which the library switches between two kernels that produce the same words (every switch has a parity test on
 * both sides, tests/test_gpu_prove.py::test_tuning_*).  Keys:
 *   "ingest_chunk_cols"         columns per chunk of the pipelined host ingest (default 32; 0 = one monolithic upload)
 *   "keccak_parts_max_points"   quotient domains of a Keccak table up to this many points use 25 threads per point (default 2^15)
 *   "fri_fused_division_min"    polynomials from this many coefficients on divide by (X - z) with all batches in one workgroup (default: never)
 *   "fri_scan_combine"          the bottom level of the division by (X - z): suffix scan of every opening batch and their weighted sum in ONE
 *                               launch, nothing but the final polynomial written (default 1); 0: a scan launch writing the suffix values of
 *                               every batch and a combine launch reading them again (round 4's form)
 *   "wide_max_hashes"           hashing launches of up to this many hashes give each hash a 16-lane row (default 1024), and
 *   "quad_max_hashes"           up to this many a quad of lanes (default 32768): the latency forms of the Poseidon permutation, at
 *                               4.2x / 1.45x the issue slots of the one-lane form.  0 and 0: one lane per hash for every leaf and
 *                               every tree level of >= 256 parents (the levels below that, a few hundred hashes per tree, keep the
 *                               quad form: the one-lane kernel works on blocks of 256 parents); a GPU shared by many contexts
 *                               proving small segments may prefer throughput -- measured in profiles/r03_hw_queues.txt
 *   "leaf_mfma"                 one-lane-per-leaf hashing (trace / auxiliary leaves, FRI layer leaves) with the dense MDS layers of the FULL
 *                               rounds on the matrix core (v_mfma_i32_32x32x32_i8 with a block-diagonal matrix operand: every lane gets M
 *                               times its own state; csrc/poseidon_mfma_dev.h: 32-bit partial sums, 93 registers, five waves per SIMD) and the
 *                               s-boxes / partial rounds on the vector ALU (default 1: leaf hashing 40.9 -> 39.4 ms at 262 x 2^22, +2 %
 *                               proofs/s and lock-step segments/s); 0: every layer as 32-bit multiply-adds
 *   "small_ntt"                 transforms of 2^9 .. 2^13 points (inverse transforms and coset-LDE blocks of short tables, quotient
 *                               chunks, FRI layers) in ONE launch, a column per workgroup (default 1); 0: two strided passes
 *   "tree_tail"                 Merkle trees of up to 2^15 leaves built in ONE launch that also delivers the cap to the host (default 1);
 *                               0: up to three launches for the levels and a download kernel
 *   "commit_lanes"              trace / auxiliary commitments of one segment built side by side (default 4: the context and three
 *                               lanes, one stream and host thread each; 1 = everything on the context's own stream)
 *   "pow_round_log"             the proof-of-work search tries 2^this candidates per round of its one launch (default 17; 8 .. 22);
 *                               the witness found is the smallest one whatever the value
 *   "max_stack"                 zkm_prove_segments: segments per lock-step group (default and maximum 32; 1 = one segment at a time, the
 *                               path of zkm_prove_segment); a table's group is also bounded by 65535 stacked columns (Keccak: 26 segments)
 *   "segments_memory_budget"    zkm_prove_segments: bytes of HBM the segments proven together may hold (estimated: values, coefficients, 4x LDE
 *                               and digests of every table's three commitments); more segments than that are proven in consecutive waves.
 *                               Default 0 = 80 % of (the blocks this context has cached + free memory) at the call; contexts sharing a GPU
 *                               are sized by the caller (contexts x segments per call x ~1.8 GB for 2^16-cycle segments)
 *   "aux_pipeline"              a segment whose tables are all short (no LDE over 1 GiB), commit_lanes > 1: the lanes build the auxiliary
 *                               commitments of tables 1.. BEHIND the proofs of the earlier tables instead of all of them before the
 *                               first proof (default 1; same transcript, same proofs); 0: all auxiliary commitments first
 *   "throughput_profile"        1: the settings for MANY contexts per GPU proving small segments (commit_lanes 1, wide_max_hashes 256,
 *                               quad_max_hashes 4096, pow_round_log 16: 16 contexts reach 74-75 segments/s of 2^16 cycles against 57-59 for 8 contexts
 *                               with the defaults, profiles/r04_throughput_profile.txt); 0: the defaults again
 *   "block_after_us"            a transcript round trip (cap, opening partials, proof-of-work witness coming down) is waited for by
 *                               polling a flag in pinned memory; after this many microseconds (default 50) a thread of a CROWDED
 *                               process -- more than half as many threads waiting as CPUs the process may run on -- parks on a
 *                               blocking-sync event instead, leaving its core to the other contexts.  0: always park.
 *   "check_ctls"                1: zkm_prove_with_traces, zkm_prove_segment[_columns], zkm_prove_segment_ops, zkm_prove_segments[_columns] and
 *                               zkm_prove_segments_ops run zkm_check_ctls on each segment's tables before they prove -- the reference's `test`
 *                               feature (prover.rs:171-176) -- and fail with "check_ctls: segment <position in the call>: " and that call's
 *                               message; no proof is written.  Default 0: no launch is added and every proof word stays what it is
 *   "check_witness"             1: the same prove calls (with the _ops_boot, _ops_steps and _ops_calls forms and a pool's groups) run
 *                               zkm_segments_check on the segments of each wave before anything is committed -- table constraints, the
 *                               range-check lookups and the cross-table lookups, two host waits a wave whatever its segments -- and fail with
 *                               "check_witness: segment <position in the call>: " and that call's message ("Constraint failed in <Name>Stark:
 *                               ..", "Lookup failed in <Name>Stark: ..", "CTL #j: .."); no proof or challenge word is written.  A
 *                               zkm_prove_with_traces call on tables other than the twelve of the AllStark gets the cross-table part only.
 *                               With "check_ctls" also set the cross-table lookups are checked once, here.  A wave whose checks' scratch
 *                               would not fit beside its tables is checked in consecutive sub-groups.  Default 0: no launch is added and
 *                               every proof word stays what it is
 *   "verify"                    1: the same prove calls verify what they have written (zkm_verify_proofs on every segment's blobs) before they
 *                               return, as prove_root does (fixed_recursive_verifier.rs:777, 853); on a rejection the call fails with
 *                               "verify: segment <position in the call>: " and that call's message, and no proof word is handed out -- of any
 *                               segment of a zkm_prove_segments[_columns] call, all of which are verified in one set of launches after the
 *                               last has been proven.  (zkm_prove_segments_ops builds and proves a call of more than 32 segments, or
 *                               of more than the memory budget holds, in consecutive waves, and a pool deals groups to its workers: there
 *                               each wave / group is verified and handed out on its own.)
 *                               Default 0: no launch is added and every proof word stays what it is
 *   "boot_chain_quad"           1: the sponge chains of the zkm_*_boot calls run their permutation across a quad of lanes (sixteen chains a
 *                               wave) instead of a 16-lane row (four a wave); the words are the same.  Default 0: the row form --
 *                               a chain of 129 permutations took 1.43 ms in the row form and 2.11 ms in the quad form on an MI355X, at
 *                               16, 64 and 256 pages alike (profiles/boot_time.json).  A measurement aid: tools/boot_time.py sets it to
 *                               time both, nothing else should
 *   "image_hash_form"           the lane form of the level launches of zkm_image_hash / zkm_images_hash: 1 a 16-lane row a chain (four chains
 *                               a wave), 2 a quad of lanes a chain (sixteen a wave), 0 (default; so is any value above 2) chosen per level
 *                               from the launch's chain count: the row form up to 8192 chains of a level (all images of the call together),
 *                               the quad form above -- the crossover tools/image_hash_time.py measured on an MI355X (a level of 8192
 *                               chains: 2.12 ms against 2.32; of 10240: 2.70 against 2.35; profiles/image_hash_time.json).  The words are
 *                               the same in every form
 *   "pool_stage_ahead"          zkm_pool_prove_segments_calls, read by each worker from its own context (zkm_pool_set_tuning sets all): 1
 *                               (default) the worker keeps ONE group staged ahead -- it stages the group it claims
 *                               (zkm_segments_calls_stage), claims and stages its next group before it proves the current one
 *                               (zkm_prove_segments_ops_steps on the handle's outputs), so the next group's uploads, expansions, placement
 *                               and walk run behind the current proofs; at most two handles a worker.  0: every group is one expanding
 *                               call, as zkm_prove_segments_ops_calls.  Proofs, offsets and challenges are the same words either way
 *   "debug_verify_flip"         TEST HOOK, accepted only when the process environment holds ZKM_ENABLE_TEST_HOOKS=1 (an unknown key otherwise):
 *                               under "verify", word `value` (0: off) of the blobs of segment 1 of the call (segment 0 of a call of one) is
 *                               increased by one mod p between proving and verifying (tests/test_gpu_verify.py)
 *   "debug_ctl_key_bits"        TEST HOOK, accepted only when the process environment holds ZKM_ENABLE_TEST_HOOKS=1 (an unknown key otherwise):
 *                               the FIRST attempt of every zkm_check_ctls call sorts by keys truncated to `value` bits (0: off), so that the
 *                               collision path -- confirmation fails, the call sorts again with the next seed -- runs; reports are
 *                               unchanged and `attempts` is 2 (tests/test_gpu_check_ctls.py)
 *   "debug_fail_allocs"         TEST HOOK, accepted only when the process environment holds ZKM_ENABLE_TEST_HOOKS=1 (an unknown key otherwise):
 *                               the next `value` device allocations of the context and its lanes fail on their first
 *                               attempt as if out of memory, so the recovery path (trim the caches -- this context's, then the
 *                               parent's and the sibling lanes' -- and retry) runs; proofs are unchanged (tests/test_segment.py)
 * An unknown key is an error.  Applies to the context and its commit lanes. */
int zkm_ctx_set_tuning(zkm_ctx* ctx, const char* key, uint64_t value, char** err);
/* Pinned host memory (N3, trace ingest): host-resident traces (the reference's Vec<PolynomialValues>, prover.rs:144-167) are
 * uploaded in column chunks on a copy stream while earlier chunks are transformed and hashed; that overlap needs page-locked
 * source memory.  Either let the witness generator write into zkm_host_alloc memory, or zkm_host_register its own buffers once.
 * Pageable host pointers are accepted everywhere too (the upload then blocks the calling thread chunk by chunk). */
int zkm_host_alloc(zkm_ctx* ctx, size_t bytes, void** out, char** err);
int zkm_host_free(zkm_ctx* ctx, void* p);
int zkm_host_register(zkm_ctx* ctx, void* p, size_t bytes, char** err);
int zkm_host_unregister(zkm_ctx* ctx, void* p);
int zkm_dev_alloc(zkm_ctx* ctx, size_t bytes, void** out, char** err);
int zkm_dev_free(zkm_ctx* ctx, void* p);
int zkm_dev_upload(zkm_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes, char** err);
int zkm_dev_download(zkm_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes, char** err);

/* ------------------------------------------------------------------ K1/K2/K9: batched Goldilocks NTT
 * Replaces PolynomialValues::{ifft, coset_ifft} / PolynomialCoeffs::{fft, coset_fft}
 * (call sites prover.rs:678-681, 787, 829).  In place over `ncols` columns of 2^log_n elements,
 * natural order in and out.  coset_shift 0 or 1 = plain subgroup; otherwise forward = scale coeff i by
 * shift^i then NTT, inverse = iNTT then scale coeff i by shift^-i (plonky2 conventions). */
int zkm_ntt(zkm_ctx* ctx, uint64_t* cols, size_t ncols, unsigned log_n, int inverse, uint64_t coset_shift, char** err);

/* Parity / debug: the loose-arithmetic field primitives of the butterflies on arbitrary 64-bit words (also >= p), n pairs from host
 * memory: out = 7 x n canonical words: a + b, a - b, a 2^24, a 2^48, a 2^72, a b, and a b again through the branch-free product the
 * quotient / opening kernels use (mod p).  Exercises the corrections of the device arithmetic that field data reaches with probability
 * 2^-32 .. 2^-64 (second wrap of add / subtract, borrow of the Goldilocks reduction with and without the product's middle carry). */
int zkm_field_selftest(zkm_ctx* ctx, const uint64_t* a, const uint64_t* b, size_t n, uint64_t* out, char** err);

/* ------------------------------------------------------------------ K1-K5: PolynomialBatch
 * zkm_batch_commit_values == PolynomialBatch::from_values(values, rate_bits, false, cap_height, ..)
 *   (prover.rs:154-163, 514-521); zkm_batch_commit_coeffs == from_coeffs (prover.rs:579-586).
 * Inputs are borrowed for the call (no clone, cf. prover.rs:155-157); the batch owns device memory:
 * coefficients (ncols x n), the LDE (ncols x 4n, rows in bit-reversed order == merkle_tree.leaves) and
 * all Merkle digest layers. */
int zkm_batch_commit_values(zkm_ctx* ctx, const uint64_t* values, size_t ncols, unsigned log_n, unsigned rate_bits,
                            unsigned cap_height, zkm_batch** out, char** err);
int zkm_batch_commit_coeffs(zkm_ctx* ctx, const uint64_t* coeffs, size_t ncols, unsigned log_n, unsigned rate_bits,
                            unsigned cap_height, zkm_batch** out, char** err);
/* The same two constructors from ONE POINTER PER COLUMN: the reference's argument is a Vec<PolynomialValues<F>> /
 * Vec<PolynomialCoeffs<F>> -- a separate heap allocation per column (prover.rs:154-163 trace_poly_values, :576-587 chunks) -- so the
 * Rust side passes `values.iter().map(|p| p.values.as_ptr())` and nothing is flattened on the host.  columns[i] -> 2^log_n words,
 * host (pageable, pinned or registered) or device; columns_are_values != 0: from_values, 0: from_coeffs.  Wide host-resident
 * matrices take the same pipelined ingest as zkm_batch_commit_values (column chunks on a copy stream). */
int zkm_batch_commit_columns(zkm_ctx* ctx, const uint64_t* const* columns, size_t ncols, unsigned log_n, int columns_are_values,
                             unsigned rate_bits, unsigned cap_height, zkm_batch** out, char** err);
void zkm_batch_free(zkm_batch* b);
/* The accessors from here to zkm_batch_digest_layer take no member: given a STACK (below) every one of them reads member 0 and
 * writes what it writes for a single commitment -- zkm_batch_cap 4 << cap_height words, whatever the stack's size.
 * .merkle_tree.cap (prover.rs:180, 524, 588): 2^cap_height digests x 4 words, host out */
int zkm_batch_cap(const zkm_batch* b, uint64_t* out);
/* .polynomials (proof.rs:311): ncols x n coefficients, natural order; out may be host or device */
int zkm_batch_coeffs(const zkm_batch* b, uint64_t* out);
/* get_lde_values(natural_index, 1) (prover.rs:687): one LDE row, ncols words, host out */
int zkm_batch_lde_row(const zkm_batch* b, size_t natural_index, uint64_t* out);
/* get_lde_values_packed(index_start, step) generalised to `count` consecutive indices (prover.rs:687, 723-748: the quotient
 * loop reads rows i_start .. i_start + P::WIDTH): out[i * ncols + c] = get_lde_values(index_start + i, step)[c], host or device */
int zkm_batch_lde_rows(const zkm_batch* b, size_t index_start, size_t step, size_t count, uint64_t* out);
/* merkle_tree.leaves[leaf_index] and merkle_tree.prove(leaf_index): (lde_bits - cap_height) x 4 words */
int zkm_batch_leaf(const zkm_batch* b, size_t leaf_index, uint64_t* out);
int zkm_batch_merkle_path(const zkm_batch* b, size_t leaf_index, uint64_t* siblings_out);
/* digest layer `level` (0 = leaf digests), (4n >> level) x 4 words, host out -- parity/debug */
int zkm_batch_digest_layer(const zkm_batch* b, unsigned level, uint64_t* out);

/* ------------------------------------------------------------------ stacked commitments
 * A STACK is nstack same-shaped commitments built in one set of launches and held in one handle: what a caller that commits the same
 * oracle once per segment (a PLONK prover proving one circuit K times) hands to zkm_eval_openings_stack / zkm_fri_prove_stack.
 * values[k] / coeffs[k] -> ncols x 2^log_n words of member k, host or device.  Member k is, word for word, what zkm_batch_commit_values /
 * _coeffs gives for the same words: cap, polynomials, leaves and Merkle paths.
 * Refused on the host, before the context: a NULL values or out; nstack outside 1..32; ncols = 0 or nstack x ncols > 65535;
 * log_n + rate_bits > 30; cap_height > log_n + rate_bits; a NULL member pointer (the message names the member).
 * The accessors above read member 0 of a stack (a single commitment is a stack of one: they are the ones below at k = 0); the ones
 * below take the member.  zkm_batch_free frees a stack. */
int zkm_batch_commit_values_stack(zkm_ctx* ctx, const uint64_t* const* values, size_t nstack, size_t ncols, unsigned log_n, unsigned rate_bits,
                                  unsigned cap_height, zkm_batch** out, char** err);
int zkm_batch_commit_coeffs_stack(zkm_ctx* ctx, const uint64_t* const* coeffs, size_t nstack, size_t ncols, unsigned log_n, unsigned rate_bits,
                                  unsigned cap_height, zkm_batch** out, char** err);
/* members of the handle: 1 for every batch of the constructors above the stack's, 0 for NULL */
size_t zkm_batch_stack_size(const zkm_batch* b);
/* member k's cap as zkm_batch_cap, its polynomials as zkm_batch_coeffs (natural order; out host or device), and
 * merkle_tree.leaves[leaf_index] (ncols words) with merkle_tree.prove(leaf_index) ((lde_bits - cap_height) x 4 words) of its tree, host
 * out, either may be NULL.  Status 1: a NULL batch, k or leaf_index out of range, a failed copy. */
int zkm_batch_stack_cap(const zkm_batch* b, size_t k, uint64_t* out);
int zkm_batch_stack_coeffs(const zkm_batch* b, size_t k, uint64_t* out);
int zkm_batch_stack_merkle_path(const zkm_batch* b, size_t k, size_t leaf_index, uint64_t* leaf_out, uint64_t* siblings_out);

/* ------------------------------------------------------------------ hash primitives
 * a13: Poseidon permutation (prover/src/poseidon/poseidon_stark.rs:51-95; == plonky2 PoseidonHash's
 * permutation); k states of 12 words, in place.  K15: Keccak-f[1600] (cpu/kernel/keccak_util.rs:6-31,
 * keccak_sponge_stark.rs:410); k states of 25 words, in place. */
int zkm_poseidon_permute_batch(zkm_ctx* ctx, uint64_t* states, size_t k, char** err);
int zkm_keccakf_batch(zkm_ctx* ctx, uint64_t* states, size_t k, char** err);

/* Parity / debug: ONE piece of the device's Poseidon permutation per call, on words the caller chooses (any uint64: the device code
 * promises "loose" inputs everywhere).  The device has four forms of the permutation -- one lane per hash on the vector ALU, one lane per
 * hash with the full-round MDS layers on the matrix core, one hash per quad of lanes, one hash per 16-lane row -- and leaf hashing only
 * ever feeds them the LDE of field data; this entry point places a chosen state in front of each form, of a single linear layer or fused
 * partial-round group, and of the folds they end in.  `in` and `out` are host memory; a state is 12 words; outputs are the raw words the
 * device code produced (loose unless stated), nothing is canonicalised by the probe.
 *   probe                                  arg                   in -> out
 *   PERMUTE_LANE, PERMUTE_LANE_MFMA,       ZKM_POSEIDON_OUT_*    n states -> n states through the form's permutation.  OUT_ALL: twelve canonical words.
 *   PERMUTE_QUAD, PERMUTE_WIDE                                   OUT_CAPACITY: words 8..11, loose; words 0..7 are garbage.  OUT_DIGEST: words 0..3,
 *                                                                canonical; words 4..11 are garbage.  The quad and 16-lane forms ignore arg and
 *                                                                return twelve canonical words.
 *   MDS_VALU, MDS_MFMA, MDS_QUAD           next: 1, 2, 3, 27,    n states -> n states: M s + the constants of round `next` (30: none) -- the layer
 *                                          28, 29 or 30          of a full round on the vector ALU, on the matrix core, in the quad form
 *   MDS_ROWS                               0 / 1                 n states -> n states: the last layer of OUT_DIGEST (0: rows 0..3 of M s) / of
 *                                                                OUT_CAPACITY (1: rows 8..11); the other rows are unspecified
 *   GROUP3, GROUP3_QUAD                    g = 0..6              n states -> n states: fused group g -- the linear layers of rounds 3g+3 .. 3g+5
 *                                                                with their constants and the word-0 s-boxes of rounds 3g+4, 3g+5
 *   GROUP2                                 0                     n states -> n states: the tail group (linear layers of rounds 24, 25)
 *   FOLD                                   0                     n pairs (al, ah), both < 2^59 -> n words al + 2^32 ah
 *   FOLD_TY                                0                     n pairs (T, Y), T < 2^57, Y < 2^27 in the low half of its word -> n words T + 2^48 Y
 *   SBOX7, SBOX_DELTA, ADD_RC0             0                     n states -> n states, word by word: x^7;  x^7 - x;  x + constant of round 0
 *   GROUP4                                 g = 0..4              n states -> n states: four-round group g of the one-lane permutation -- the linear layers
 *                                                                of rounds 4g+3 .. 4g+6 with their constants and the word-0 s-boxes of rounds 4g+4 .. 4g+6
 *   FOLD_WIDE                              0                     n triples (al, ah, carries), al and ah ANY uint64, carries = cl + 2 ch with cl, ch in {0, 1}
 *                                                                -> n words (al + 2^64 cl) + 2^32 (ah + 2^64 ch): the fold of an M^4 row
 * (all mod p).  An unknown probe, an arg outside its column, n = 0 or n > 2^20 is an error: nothing is launched. */
#define ZKM_POSEIDON_OUT_ALL 0
#define ZKM_POSEIDON_OUT_CAPACITY 1
#define ZKM_POSEIDON_OUT_DIGEST 2
#define ZKM_POSEIDON_PROBE_PERMUTE_LANE 0
#define ZKM_POSEIDON_PROBE_PERMUTE_LANE_MFMA 1
#define ZKM_POSEIDON_PROBE_PERMUTE_QUAD 2
#define ZKM_POSEIDON_PROBE_PERMUTE_WIDE 3
#define ZKM_POSEIDON_PROBE_MDS_VALU 4
#define ZKM_POSEIDON_PROBE_MDS_MFMA 5
#define ZKM_POSEIDON_PROBE_MDS_QUAD 6
#define ZKM_POSEIDON_PROBE_MDS_ROWS 7
#define ZKM_POSEIDON_PROBE_GROUP3 8
#define ZKM_POSEIDON_PROBE_GROUP3_QUAD 9
#define ZKM_POSEIDON_PROBE_GROUP2 10
#define ZKM_POSEIDON_PROBE_FOLD 11
#define ZKM_POSEIDON_PROBE_FOLD_TY 12
#define ZKM_POSEIDON_PROBE_SBOX7 13
#define ZKM_POSEIDON_PROBE_SBOX_DELTA 14
#define ZKM_POSEIDON_PROBE_ADD_RC0 15
#define ZKM_POSEIDON_PROBE_GROUP4 17      /* (16 is not a probe) */
#define ZKM_POSEIDON_PROBE_FOLD_WIDE 18
int zkm_poseidon_selftest(zkm_ctx* ctx, uint32_t probe, uint32_t arg, const uint64_t* in, size_t n, uint64_t* out, char** err);

/* Parity / debug: the constraint consumer of the quotient kernels (the alpha-accumulation of vanishing_poly.rs:30-45,
 * constraint_consumer.rs:57-62) on words the trace never holds.  n lanes each feed their own K terms -- terms[k * n + lane], ANY
 * 64-bit words, also >= p -- to a consumer with the nalphas (1 or 2) challenges `alphas` (any words), `run` terms at a time (1 .. 8;
 * the tail in one shorter run; 1 = the single-constraint path); out[a * n + lane] = sum_k terms[k] alphas[a]^(K-1-k) mod p, canonical.
 * K = 0, n = 0, n > 2^20 or K * n > 2^26 is an error: nothing is launched. */
int zkm_consumer_selftest(zkm_ctx* ctx, const uint64_t* alphas, size_t nalphas, const uint64_t* terms, size_t K, size_t n, uint32_t run,
                          uint64_t* out, char** err);

/* ------------------------------------------------------------------ a13: PoseidonStark witness
 * PoseidonStark::generate_trace (poseidon_stark.rs:104-160): 262 columns x 2^log_n rows, column-major,
 * from `num_perms` seeded 12-element inputs (SplitMix64(seed); timestamp 0, FILTER 1) padded with the
 * default row (permutation of zeros, FILTER 0).  out must be a device pointer. */
#define ZKM_POSEIDON_COLS 262
int zkm_poseidon_trace(zkm_ctx* ctx, uint64_t seed, size_t num_perms, unsigned log_n, uint64_t* out_dev, char** err);

/* PoseidonStark::generate_trace for explicit permutation inputs: inputs = num_perms x 12 field elements, one timestamp each
 * (host or device); rows past num_perms are the default row (FILTER 0).  This is the table the PoseidonSponge rows look up
 * (all_stark.rs:169-195). */
int zkm_poseidon_trace_inputs(zkm_ctx* ctx, const uint64_t* inputs, const uint64_t* timestamps, size_t num_perms, unsigned log_n,
                              uint64_t* out_dev, char** err);

/* ------------------------------------------------------------------ N2: PoseidonSpongeStark witness
 * PoseidonSpongeStark::generate_trace (poseidon_sponge/poseidon_sponge_stark.rs:186-381, column map poseidon_sponge/columns.rs:17-66):
 * 110 columns, one row per 32-byte block (len/32 + 1 rows per operation, pad10*1 on the final row), the block's eight
 * little-endian u32 words overwrite the rate, one Poseidon permutation per row; padding rows all-zero.  Operation
 * arguments as zkm_keccak_sponge_trace. */
#define ZKM_POSEIDON_SPONGE_COLS 110
int zkm_poseidon_sponge_trace(zkm_ctx* ctx, const uint8_t* inputs, const uint64_t* input_off, const uint64_t* meta, size_t nops,
                              unsigned log_n, uint64_t* out_dev, size_t* rows_used_out, char** err);

/* ------------------------------------------------------------------ a12: KeccakSpongeStark witness (BASELINE config 5)
 * KeccakSpongeStark::generate_trace (keccak_sponge/keccak_sponge_stark.rs:222-251, rows :253-438, column map
 * keccak_sponge/columns.rs:19-70): 470 columns, one row per 136-byte block (len/136 + 1 rows per operation, pad10*1 on
 * the final row :334-341), one Keccak-f[1600] per row (:410), padding rows all-zero (:440-444).
 *   inputs        concatenated input bytes of all operations (host or device)
 *   input_off     nops + 1 byte offsets into `inputs` (host)
 *   meta          nops x 4 words (host): context, segment, virt_base, timestamp; word i of the input is read at
 *                 virt_base + i (contiguous base addresses), or, with ZKM_SPONGE_BYTE_ADDRESSED set in virt_base, at
 *                 (virt_base & ~ZKM_SPONGE_BYTE_ADDRESSED) + 4 i: the addresses generate_keccak hands to keccak_sponge_log
 *                 (witness/operation.rs:1118-1134), one memory word every 4 bytes.  The flag is per operation and changes
 *                 nothing else of a row; zkm_poseidon_sponge_trace reads it the same way.  ZKM_SPONGE_PADDED_TAIL, a second
 *                 flag bit of virt_base, is masked off and changes nothing of a row: it speaks to the SYSKECCAK calls'
 *                 expansion (below), which hands its metas on unchanged.
 * Output: 470 x 2^log_n column-major, device pointer.  Fails if the operations need more than 2^log_n rows or if an
 * operation is empty (the reference indexes base_address[0]). */
#define ZKM_SPONGE_BYTE_ADDRESSED 0x8000000000000000ULL
#define ZKM_SPONGE_PADDED_TAIL 0x4000000000000000ULL
#define ZKM_KECCAK_SPONGE_COLS 470
int zkm_keccak_sponge_trace(zkm_ctx* ctx, const uint8_t* inputs, const uint64_t* input_off, const uint64_t* meta, size_t nops,
                            unsigned log_n, uint64_t* out_dev, size_t* rows_used_out, char** err);

/* ------------------------------------------------------------------ a12: KeccakStark witness
 * KeccakStark::generate_trace (keccak/keccak_stark.rs:62-236, register map keccak/columns.rs): 2431 columns, 24 rows per
 * permutation (round flags, timestamp, the round's input limbs A, and the bit-decomposed theta / rho-pi / chi / iota
 * intermediates C, C', A', A'', A'''[0,0]); rows past 24*nperms are zero.
 *   inputs      nperms x 25 u64 permutation inputs, A(x, y) = inputs[p][5y + x] (host or device)
 *   timestamps  nperms u64 (host or device)
 * Output: 2431 x 2^log_n column-major, device pointer.  Fails if 24*nperms > 2^log_n. */
#define ZKM_KECCAK_COLS 2431
int zkm_keccak_trace(zkm_ctx* ctx, const uint64_t* inputs, const uint64_t* timestamps, size_t nperms, unsigned log_n,
                     uint64_t* out_dev, char** err);

/* ------------------------------------------------------------------ N2: SHA-256 message-schedule witnesses
 * ShaExtendStark::generate_trace (sha_extend/sha_extend_stark.rs:121-236): 78 columns, one row per schedule step; inputs =
 * nrows x 16 bytes (w[i-15], w[i-2], w[i-16], w[i-7] as little-endian byte quadruples), one timestamp per row; rows past
 * nrows are zero.
 * ShaExtendSpongeStark::generate_trace (sha_extend_sponge/sha_extend_sponge_stark.rs:131-215) for nblocks complete schedules:
 * 76 columns, 48 rows per block; w16 = nblocks x 16 uint32 words w[0..15]; meta = nblocks x 4 {context, segment, address of
 * w[0], timestamp of round 0}; word j lives at address + 4 j and round r is stamped timestamp + 20 r (2 * NUM_CHANNELS). */
#define ZKM_SHA_EXTEND_COLS 78
#define ZKM_SHA_EXTEND_SPONGE_COLS 76
int zkm_sha_extend_trace(zkm_ctx* ctx, const uint8_t* inputs, const uint64_t* timestamps, size_t nrows, unsigned log_n, uint64_t* out_dev,
                         char** err);
int zkm_sha_extend_sponge_trace(zkm_ctx* ctx, const uint32_t* w16, const uint64_t* meta, size_t nblocks, unsigned log_n, uint64_t* out_dev,
                                char** err);

/* SHA-256 compression witnesses for ncomp compressions: hx = ncomp x 8 words (a..h before the block), w = ncomp x 64 schedule
 * words, meta = ncomp x 8 {context, segment, address of hx[0], timestamp, address of w[0], segment of w, context of w, unused}.
 * ShaCompressStark::generate_trace (sha_compress/sha_compress_stark.rs:227-400; rows as emitted by witness/util.rs:605-690):
 * 224 columns, 65 rows per compression -- rounds 0..63 on the running state with w_i and K_i, then the final state with
 * w_i = k_i = 0.  ShaCompressSpongeStark::generate_trace (sha_compress_sponge/sha_compress_sponge_stark.rs:118-230): 127
 * columns, one row per compression (hx, the compressed state, hx + state with carry flags, addresses). */
#define ZKM_SHA_COMPRESS_COLS 224
#define ZKM_SHA_COMPRESS_SPONGE_COLS 127
int zkm_sha_compress_trace(zkm_ctx* ctx, const uint32_t* hx, const uint32_t* w, const uint64_t* meta, size_t ncomp, unsigned log_n,
                           uint64_t* out_dev, char** err);
int zkm_sha_compress_sponge_trace(zkm_ctx* ctx, const uint32_t* hx, const uint32_t* w, const uint64_t* meta, size_t ncomp, unsigned log_n,
                                  uint64_t* out_dev, char** err);

/* ------------------------------------------------------------------ N2: LogicStark witness
 * LogicStark::generate_trace (logic.rs:150-183) with Operation::into_row (:122-142): 69 columns x 2^log_n rows,
 * column-major; row r < nops holds operation r (flag column, the 32 little-endian bits of each input, the result),
 * the remaining rows are zero.  ops = nops x 3 uint32 words {op (0 and, 1 or, 2 xor, 3 nor), input0, input1}, host or
 * device.  Fails if nops > 2^log_n or an op code is out of range. */
#define ZKM_LOGIC_COLS 69
int zkm_logic_trace(zkm_ctx* ctx, const uint32_t* ops, size_t nops, unsigned log_n, uint64_t* out_dev, char** err);

/* ------------------------------------------------------------------ N3: MemoryStark witness
 * MemoryStark::generate_trace (memory/memory_stark.rs:135-248) on the segment's raw memory operations: sort by (context, segment,
 * virt, timestamp) keeping push order among equal keys, fill_gaps (dummy filter-0 reads bridging virt gaps and timestamp gaps above
 * max_rc = next_pow2(nops) - 1), pad_memory_ops (filter-0 read copies of the last operation pushed), the R0 write rule of into_row,
 * first-change flags, RANGE_CHECK, COUNTER and FREQUENCIES.  13 columns x 2^log_n rows, column-major, canonical; column order of
 * memory/columns.rs (FILTER, TIMESTAMP, IS_READ, CONTEXT, SEGMENT, VIRTUAL, VALUE, three first-change flags, RANGE_CHECK,
 * COUNTER, FREQUENCIES).  Word for word the CPU oracle's zko_memory_trace.
 *   ops                nops x 6 words {context, segment, virt, timestamp, is_read (nonzero: read), value (truncated to 32 bits)},
 *                      host or device; every op has filter 1 (MemoryOp::new)
 *   out_dev            device pointer, or NULL: sizing only -- log_n is ignored and only *natural_rows_out is computed
 *   natural_rows_out   next_pow2(nops + dummy rows), the reference's table height (may be NULL)
 * Fails (nonzero, message in *err; the contents of out_dev are then unspecified) if nops is 0 or 2^32 or more, log_n is above
 * ZKM_MEMORY_MAX_LOG_N, a key word is not below p, the dummy rows overflow (2^62 rows or more), the table needs more than 2^log_n
 * rows (*natural_rows_out is still written), or a context / segment gap gives a range check of 2^log_n or more.  Synchronous on the
 * context's stream. */
#define ZKM_MEMORY_COLS 13
#define ZKM_MEMORY_MAX_LOG_N 28
int zkm_memory_trace(zkm_ctx* ctx, const uint64_t* ops, size_t nops, unsigned log_n, uint64_t* out_dev, size_t* natural_rows_out,
                     char** err);

/* ------------------------------------------------------------------ N3: ArithmeticStark witness
 * ArithmeticStark::generate_trace (arithmetic/arithmetic_stark.rs:155-185) with generate_range_checks (:127-153) on the segment's
 * arithmetic operations: each operation's rows (binary_op_to_rows, arithmetic/mod.rs:237-313; two rows for DIV, DIVU, SRL, SRLV, SRA
 * and SRAV, one for the rest) in push order, zero rows behind them, RANGE_COUNTER (column 44) = min(row, 2^16 - 1) and RC_FREQUENCIES
 * (column 45) += the count of each value over the 18 shared columns 26..43 of all 2^log_n rows, padding included.  54 columns x
 * 2^log_n rows, column-major, canonical; column order of arithmetic/columns.rs.
 *   ops                nops x 3 uint32 words {op, input0, input1} as Operation::binary(operator, input0, input1) receives them, host
 *                      or device; op = the operator's row filter, IS_ADD = 0 .. IS_MTLO = 25 (mod.rs:135-164).  result0 / result1
 *                      are computed on the device (BinaryOperator::result, mod.rs:48-133).  nops = 0 is valid: an all-padding table
 *   out_dev            device pointer, or NULL: sizing only -- log_n is ignored and only *natural_rows_out is computed
 *   natural_rows_out   max(2^16, next_pow2(rows)), the reference's table height (may be NULL)
 * Fails (nonzero, message in *err; the contents of out_dev are then unspecified) if nops is 2^31 or more, log_n is below 16 or above
 * ZKM_ARITHMETIC_MAX_LOG_N, the rows do not fit in 2^log_n (*natural_rows_out is still written), or an operation is outside the
 * reference's domain:
 *   op > 25;
 *   DIV or DIVU with input1 = 0, or DIV of 0x80000000 by 0xFFFFFFFF (result() panics on both, mod.rs:123-127);
 *   ADDI, ADDIU, SLTI or SLTIU with an input1 that is not a sign-extended 16-bit immediate (the emulator sign-extends,
 *   witness/operation.rs:390; for any other input1 the row of addcy.rs / slt.rs and result0, mod.rs:52-60 / 94-109, disagree);
 *   SLL, SRL, SRA or SRAV with a shift amount above 31 (result() gives 0 there, mod.rs:63-69, and sra.rs:52-73 shifts by the full
 *   amount; SLLV and SRLV mask it, mod.rs:72-73, and accept any);
 *   a shared-column value of 2^16 or more (the assert of generate_range_checks, arithmetic_stark.rs:144-149).
 * LUI accepts any input0.  A failure leaves the context usable and its transient memory as it was.  Synchronous on the context's
 * stream. */
#define ZKM_ARITHMETIC_COLS 54
#define ZKM_ARITHMETIC_MAX_LOG_N 28
int zkm_arithmetic_trace(zkm_ctx* ctx, const uint32_t* ops, size_t nops, unsigned log_n, uint64_t* out_dev, size_t* natural_rows_out,
                         char** err);

/* ------------------------------------------------------------------ Fiat-Shamir (host)
 * plonky2 Challenger<F, PoseidonHash> (uses at prover.rs:182-190, 466, 524-527, 588-591, 610). */
typedef struct {
    uint64_t state[12];
    uint64_t in_buf[8];
    uint64_t out_buf[8];
    uint32_t n_in, n_out;
} zkm_challenger;
void zkm_challenger_init(zkm_challenger* ch);
void zkm_challenger_observe(zkm_challenger* ch, const uint64_t* elems, size_t n);
uint64_t zkm_challenger_get(zkm_challenger* ch);
void zkm_challenger_compact(zkm_challenger* ch, uint64_t state_out[12]);

/* ------------------------------------------------------------------ a5: prove_single_table
 * StarkConfig::standard_fast_config (prover/src/config.rs:17-30). */
typedef struct {
    unsigned rate_bits, cap_height, pow_bits, num_challenges, num_queries, arity_bits, final_poly_bits;
} zkm_stark_config;
void zkm_standard_config(zkm_stark_config* cfg);

/* Tables with a constraint kernel (the reference's Table enum, all_stark.rs:96-110, has 12):
 *   POSEIDON       poseidon/poseidon_stark.rs:554-594   262 columns
 *   LOGIC          logic.rs:199-248                       69 columns
 *   KECCAK_SPONGE  keccak_sponge_stark.rs:456-567        470 columns
 *   KECCAK         keccak/keccak_stark.rs:256-413       2431 columns
 *   MEMORY         memory/memory_stark.rs:253-341         13 columns, plus the range-check lookup :476-483
 *   POSEIDON_SPONGE poseidon_sponge/poseidon_sponge_stark.rs:383-478  110 columns
 *   SHA_EXTEND     sha_extend/sha_extend_stark.rs:238-317              78 columns
 *   SHA_EXTEND_SPONGE sha_extend_sponge/sha_extend_sponge_stark.rs:220-330  76 columns
 *   SHA_COMPRESS   sha_compress/sha_compress_stark.rs:402-606         224 columns
 *   SHA_COMPRESS_SPONGE sha_compress_sponge/sha_compress_sponge_stark.rs:233-268  127 columns
 *   ARITHMETIC     arithmetic/arithmetic_stark.rs:214-240 and its nine operation modules, 54 columns, plus the 18-column range-check lookup
 *                  :269-276 (at least 2^16 rows); rows from zkm_arithmetic_trace or the CPU-side witness generator */
#define ZKM_TABLE_POSEIDON 0
#define ZKM_TABLE_LOGIC 1
#define ZKM_TABLE_KECCAK_SPONGE 2
#define ZKM_TABLE_KECCAK 3
#define ZKM_TABLE_MEMORY 4
#define ZKM_TABLE_POSEIDON_SPONGE 5
#define ZKM_TABLE_SHA_EXTEND 6
#define ZKM_TABLE_SHA_EXTEND_SPONGE 7
#define ZKM_TABLE_SHA_COMPRESS 8
#define ZKM_TABLE_SHA_COMPRESS_SPONGE 9
#define ZKM_TABLE_ARITHMETIC 10
#define ZKM_TABLE_CPU 11
/* Position of a table in the reference's Table enum (all_stark.rs:96-110: Arithmetic = 0, Cpu, Poseidon, PoseidonSponge, Keccak,
 * KeccakSponge, ShaExtend, ShaExtendSponge, ShaCompress, ShaCompressSponge, Logic, Memory = 11), or -1 for an unknown id.  The
 * ZKM_TABLE_* ids above are NOT in that order.  prove_with_traces (prover.rs:144-200, 234-438) commits, observes and proves the
 * tables in Table::all() order on one transcript: zkm_prove_with_traces / zkm_prove_segment_image use the caller's array order and
 * reject an array that holds all twelve tables in any other order (sub-segments of fewer tables, as the tests prove them, are the
 * caller's responsibility). */
int zkm_table_enum_index(int table_id);
#define ZKM_ARITHMETIC_COLS 54
#define ZKM_CPU_COLS 259
#define ZKM_MEMORY_COLS 13
size_t zkm_table_width(int table_id); /* 0 for an unknown id */
/* Auxiliary columns the table's own logUp lookups (Stark::lookups(), lookup.rs:22-40) put in front of the CTL columns:
 * per lookup and challenge, ceil(columns / 2) helper columns and one Z (stark.rs:217-223).  0 for tables without lookups.
 * The naux arguments of the prove entry points count the CTL columns only; zkm_proof_words takes the total. */
size_t zkm_num_lookup_columns(int table_id, const zkm_stark_config* cfg);

/* Proof blob (uint64_t words) -- the fields of StarkProofWithMetadata (proof.rs:178-201) flattened:
 *   [0] magic "ZKMPROOF" [1] degree_bits [2] W trace cols [3] A aux cols [4] Q quotient polys [5] Z ctl zs
 *   [6] cap_height [7] L fri layers [8] F final_poly_len [9] num_queries [10] rate_bits [11] arity_bits
 *   [12..15] 0
 *   init_challenger_state[12]
 *   trace_cap[C*4] aux_cap[C*4] quotient_cap[C*4]                    C = 2^cap_height
 *   local_values[2W] next_values[2W] aux[2A] aux_next[2A] ctl_zs_first[Z] quotient[2Q]
 *   commit_phase_merkle_caps[L][C*4]   final_poly[2F]   pow_witness[1]
 *   query_round_proofs[num_queries]:
 *       oracle 0..2: evals[ncols_o], siblings[(lde_bits - cap_height)*4]
 *       layer i in 0..L: evals[2*2^arity_bits], siblings[(lde_bits - arity_bits*(i+1) - cap_height)*4]
 */
#define ZKM_PROOF_MAGIC 0x5a4b4d50524f4f46ULL
size_t zkm_proof_words(const zkm_stark_config* cfg, unsigned log_n, size_t ncols, size_t naux, size_t nctl_zs);

/* N4, proof hand-off: word offsets of every field of a proof blob, read from the blob's own header, so the caller can rebuild
 * StarkProofWithMetadata (proof.rs:178-201), StarkOpeningSet (:281-297) and plonky2's FriProof with plain slice copies.  F2 values
 * are pairs of consecutive words (c0, c1); digests are 4 words.  Returns 0, or nonzero if the header is not a proof header. */
typedef struct {
    uint64_t degree_bits, trace_cols, aux_cols, quotient_polys, ctl_zs, cap_height, fri_layers, final_poly_len, num_queries, rate_bits,
        arity_bits;
    size_t total_words;
    size_t init_challenger_state;                 /* 12 words */
    size_t trace_cap, aux_cap, quotient_cap;      /* 2^cap_height digests each */
    size_t local_values, next_values;             /* trace_cols F2 values each */
    size_t aux_polys, aux_polys_next;             /* aux_cols F2 values each */
    size_t ctl_zs_first;                          /* ctl_zs base-field words */
    size_t quotient_polys_open;                   /* quotient_polys F2 values */
    size_t commit_phase_merkle_caps;              /* fri_layers x 2^cap_height digests */
    size_t final_poly;                            /* final_poly_len F2 coefficients */
    size_t pow_witness;                           /* 1 word */
    size_t query_round_proofs, query_round_words; /* num_queries rounds of query_round_words words, see zkm_proof_query_layout */
} zkm_proof_layout;
int zkm_proof_get_layout(const uint64_t* proof, zkm_proof_layout* out);
/* Offsets inside ONE query round (relative to query_round_proofs + q * query_round_words):
 *   oracle o in {0 trace, 1 aux, 2 quotient}: evals at oracle_evals[o] (oracle_cols[o] base-field words), Merkle siblings at
 *   oracle_siblings[o] (initial_siblings digests) -- FriInitialTreeProof;
 *   layer i < fri_layers: 2^arity_bits F2 evals at layer_evals[i], layer_siblings_count[i] digests at layer_siblings[i] -- FriQueryStep.
 * Arrays are sized for at most 16 layers.  recover_degree_bits (proof.rs:205-212) reads initial_siblings + cap_height - rate_bits. */
typedef struct {
    size_t oracle_evals[3], oracle_cols[3], oracle_siblings[3], initial_siblings;
    size_t layer_evals[16], layer_siblings[16], layer_siblings_count[16];
} zkm_proof_query_layout;
int zkm_proof_get_query_layout(const uint64_t* proof, zkm_proof_query_layout* out);

/* prove_single_table (prover.rs:441-641) for table `table_id`.
 *   trace       ncols x 2^log_n trace values (host or device) -- used only if trace_batch is NULL
 *   trace_batch optional existing commitment of the trace (prover.rs:445); NULL = commit here
 *   aux         naux x 2^log_n auxiliary values = ctl helper columns ++ ctl z columns (prover.rs:497-508)
 *   num_helpers helper-column count of each of the nctl_zs CtlZData (cross_table_lookup.rs:474-481)
 *   challenger  in/out transcript (host)
 *   proof_out   host buffer of zkm_proof_words() words */
int zkm_prove_single_table(zkm_ctx* ctx, int table_id, const zkm_stark_config* cfg, const uint64_t* trace, size_t ncols,
                           unsigned log_n, const zkm_batch* trace_batch, const uint64_t* aux, size_t naux,
                           const uint32_t* num_helpers, size_t nctl_zs, zkm_challenger* challenger, uint64_t* proof_out,
                           char** err);


/* K proofs of the same table at the same height in lock-step (cf. zkm_prove_segments): K calls of zkm_prove_single_table -- traces[k],
 * aux[k], challengers[k], proofs_out[k] as that entry point takes them (trace values required; the benchmark's CtlData shape) -- as one:
 * stacked trace / auxiliary / quotient commitments, one launch per stage and one transcript round trip per stage for all K.  Every
 * blob and every challenger state equals the single call's.  At most 32 proofs per call; tables with lookups of their own (Memory,
 * Arithmetic) go through zkm_prove_segments.  ~14.6 GB of HBM per 262 x 2^20 proof in flight. */
int zkm_prove_single_tables(zkm_ctx* ctx, int table_id, const zkm_stark_config* cfg, size_t nproofs, const uint64_t* const* traces, size_t ncols,
                            unsigned log_n, const uint64_t* const* aux, size_t naux, const uint32_t* num_helpers, size_t nctl_zs,
                            zkm_challenger* const* challengers, uint64_t* const* proofs_out, char** err);

/* ------------------------------------------------------------------ a3/a7: cross-table lookups, data-driven
 * Column / Filter / TableWithColumns / CrossTableLookup (prover/src/cross_table_lookup.rs:31-415) restated as
 * plain arrays so that the same description drives CTL data generation (a3), the CTL constraint checks inside
 * the quotient kernel (a7) and the verifier. */
typedef struct {            /* Column<F>: sum_k coeff_k*local[col_k] + sum_k coeff_k*next[col_k] + constant */
    uint32_t n_local, n_next, term_off, _pad;   /* terms [term_off, +n_local) are local, the next n_next are next-row */
    uint64_t constant;
} zkm_column;
typedef struct {            /* TableWithColumns minus the table id: Vec<Column> + Option<Filter> */
    uint32_t ncols, col_off;                    /* columns[col_off .. col_off+ncols) */
    uint32_t has_filter, nprod, prod_off, nconst, const_off, _pad;
    /* Filter = sum_{k<nprod} columns[filter_idx[prod_off+2k]] * columns[filter_idx[prod_off+2k+1]]
     *        + sum_{k<nconst} columns[filter_idx[const_off+k]]                       (cross_table_lookup.rs:40-103) */
} zkm_colset;
typedef struct {            /* all descriptor arrays of one table (host pointers) */
    const zkm_column* columns; size_t ncolumns;
    const uint32_t* term_col; const uint64_t* term_coeff; size_t nterms;
    const zkm_colset* colsets; size_t ncolsets;
    const uint32_t* filter_idx; size_t nfilter_idx;
} zkm_ctl_table;
typedef struct {            /* CtlZData (cross_table_lookup.rs:424-438) */
    uint32_t ncolsets, colset_off;              /* colset_ids[colset_off .. +ncolsets) index the table's colsets */
    uint32_t num_helpers, _pad;                 /* helper columns of this Z: ceil(ncolsets/2) if ncolsets > 1 else 0
                                                   (the benchmark's fake CTL data has ncolsets == 0, num_helpers == 1) */
    uint64_t beta, gamma;                       /* GrandProductChallenge */
} zkm_ctl_z;
typedef struct { uint32_t table, colset; } zkm_ctl_side;
typedef struct { uint32_t nlooking, looking_off; zkm_ctl_side looked; } zkm_cross_table_lookup;  /* looking sides: sides[looking_off..] */

/* a3: cross_table_lookup_data for one table (get_helper_cols :709-797, partial_sums :841-872): helper columns and
 * the upside-down running-sum Z of every CtlZData.  aux_out = all helper columns (zs order) ++ all Z columns,
 * column-major (sum num_helpers + nzs) x 2^log_n, host or device; trace = ncols x 2^log_n values, host or device. */
int zkm_ctl_data(zkm_ctx* ctx, const zkm_ctl_table* table, const zkm_ctl_z* zs, const uint32_t* colset_ids, size_t nzs,
                 const uint64_t* trace, size_t ncols, unsigned log_n, uint64_t* aux_out, char** err);

/* a4: lookup_helper_columns (lookup.rs:46-124): logUp helper columns of one Lookup for one challenge --
 *   h_j[i] = sum over the (<= 2) looking columns f of chunk j of filter_f[i] / (challenge + f[i]),
 *   Z[0] = 0, Z[i+1] = Z[i] + sum_j h_j[i] - frequencies[i] / (challenge + table[i]).
 * colset_ids: the nlookup looking columns as single-column sets (column + optional filter); table_col / freq_col:
 * column indices of Lookup::table_column / frequencies_column.  out = (ceil(nlookup/2) + 1) x 2^log_n: helpers, then Z
 * (the order prove_single_table appends them, prover.rs:480-493). */
int zkm_lookup_helper_columns(zkm_ctx* ctx, const zkm_ctl_table* table, const uint32_t* colset_ids, size_t nlookup, uint32_t table_col,
                              uint32_t freq_col, uint64_t challenge, const uint64_t* trace, size_t ncols, unsigned log_n,
                              uint64_t* out, char** err);

/* prove_single_table with real CTL data: like zkm_prove_single_table, the CtlZData described by (table, zs, colset_ids).
 * lookup_challenges: for a table with its own lookups (zkm_num_lookup_columns() > 0) the num_challenges lookup challenges --
 * the betas of the CTL challenges (prover.rs:468-474); the helper columns are computed here (prover.rs:475-493) from the
 * trace VALUES, so `trace` is required for such tables even when trace_batch is given.  NULL otherwise. */
int zkm_prove_single_table_ctl(zkm_ctx* ctx, int table_id, const zkm_stark_config* cfg, const uint64_t* trace, size_t ncols,
                               unsigned log_n, const zkm_batch* trace_batch, const uint64_t* aux, size_t naux,
                               const zkm_ctl_table* table, const zkm_ctl_z* zs, const uint32_t* colset_ids, size_t nzs,
                               const uint64_t* lookup_challenges, zkm_challenger* challenger, uint64_t* proof_out, char** err);

/* a1: prove_with_traces (prover.rs:130-232): commit every trace, seed the transcript with all trace caps and the
 * public values, draw the CTL challenges, build every table's CtlData, then prove the tables in order on the shared
 * transcript.  Output: per-table proof blobs concatenated (offsets in proof_offsets_out[ntables+1]) and the
 * num_challenges (beta, gamma) pairs. */
typedef struct {
    int table_id;
    const uint64_t* trace;      /* ncols x 2^log_n in one block, host or device; NULL when `columns` is given */
    size_t ncols;
    unsigned log_n;
    const zkm_ctl_table* ctl;   /* column sets referenced by the cross-table lookups */
    const uint64_t* const* columns;  /* or: one pointer per column (2^log_n words each, host or device) -- the reference's
                                        Vec<PolynomialValues<F>> (prover.rs:130-142) without a host-side flatten; NULL = use `trace` */
} zkm_table_input;
size_t zkm_all_proof_words(const zkm_stark_config* cfg, const zkm_table_input* tables, size_t ntables,
                           const zkm_cross_table_lookup* ctls, const zkm_ctl_side* sides, size_t nctls, size_t* proof_offsets_out);
int zkm_prove_with_traces(zkm_ctx* ctx, const zkm_stark_config* cfg, const zkm_table_input* tables, size_t ntables,
                          const zkm_cross_table_lookup* ctls, const zkm_ctl_side* sides, size_t nctls,
                          const uint64_t* public_values, size_t npublic, uint64_t* proofs_out, uint64_t* ctl_challenges_out,
                          char** err);

/* The AllStark of the reference (all_stark.rs:96-155, 136-542) ships with the library, so a caller proves a whole segment from
 * the twelve traces alone: zkm_all_stark_ctls returns the fifteen cross-table lookups (sides name tables by their position in
 * the Table enum, all_stark.rs:96-110), zkm_all_stark_ctl_table the column sets of one table, and zkm_prove_segment ==
 * prove_with_traces (prover.rs:130-232) on traces[t] / log_n[t] of Table::all()[t] (widths: zkm_table_width).  Pass
 * proofs_out = NULL to size the output first: proof_offsets_out[13] (offsets of the twelve blobs + the total).
 * (csrc/all_stark_ctl.inc is generated from zkm_amd/tables.py by tools/gen_all_stark_ctl.py.) */
int zkm_all_stark_ctls(const zkm_cross_table_lookup** ctls_out, size_t* nctls_out, const zkm_ctl_side** sides_out, size_t* nsides_out);
const zkm_ctl_table* zkm_all_stark_ctl_table(int table_id);
int zkm_prove_segment(zkm_ctx* ctx, const zkm_stark_config* cfg, const uint64_t* const* traces, const unsigned* log_n,
                      const uint64_t* public_values, size_t npublic, uint64_t* proofs_out, size_t* proof_offsets_out,
                      uint64_t* ctl_challenges_out, char** err);
/* zkm_prove_segment with one pointer per column: columns[t][i] -> column i of table t (Table::all() order), 2^log_n[t] words. */
int zkm_prove_segment_columns(zkm_ctx* ctx, const zkm_stark_config* cfg, const uint64_t* const* const* columns, const unsigned* log_n,
                              const uint64_t* public_values, size_t npublic, uint64_t* proofs_out, size_t* proof_offsets_out,
                              uint64_t* ctl_challenges_out, char** err);

/* K INDEPENDENT segments in lock-step: the reference proves the segments of a program one after the other, each a prove_with_traces
 * on its own transcript (prover/examples/utils/src/utils.rs:57-68, 105-133; prover.rs:130-232).  Here the K segments of one call
 * advance through every stage of prove_with_traces TOGETHER: for every table, the segments whose table has the same height form a
 * group (at most "max_stack", see zkm_ctx_set_tuning; heights may differ between segments -- a table's segments of another height form
 * another group), a group's trace / auxiliary / quotient commitments, CTL data, constraint evaluation, openings, FRI layers, proof of
 * work and query gathers are ONE launch (or group of launches) for all its segments, and each of its transcript round trips (caps,
 * opening partials, final polynomial, proof-of-work witness, query rounds) brings the words of all of them down together.  The
 * transcripts stay per segment, on the host; every proof blob and every challenge is word for word what zkm_prove_segment returns
 * for that segment alone (tests/test_segments_batch.py).  A 2^16-cycle segment is mostly tables of 2^6 .. 2^13 rows whose launches
 * cannot fill the GPU one segment at a time: K of them do.
 *   traces[s][t]        table t (Table::all() order) of segment s: zkm_table_width x 2^log_n[s][t] words, host or device
 *   public_values[s]    npublic[s] words (arrays may be NULL when no segment has public values)
 *   proofs_out[s]       zkm_prove_segment(.., proofs_out = NULL, ..) sizes a segment's buffer and gives its thirteen offsets
 *   ctl_challenges_out[s]   2 * num_challenges words
 * Memory: every commitment of every segment of a group is alive until its table has been proven (~1.8 GB of HBM per 2^16-cycle segment);
 * a call with more segments than 80 % of (the blocks this context has cached + the memory that is free) holds is proven in
 * consecutive, equally sized waves (the words are the same; only fewer segments share a launch).
 * A failure leaves every output undefined (no partial results). */
int zkm_prove_segments(zkm_ctx* ctx, const zkm_stark_config* cfg, size_t nseg, const uint64_t* const* const* traces,
                       const unsigned* const* log_n, const uint64_t* const* public_values, const size_t* npublic, uint64_t* const* proofs_out,
                       uint64_t* const* ctl_challenges_out, char** err);
/* zkm_prove_segments with one pointer per column: columns[s][t][i] -> column i of table t of segment s (2^log_n[s][t] words) -- K of the
 * reference's [Vec<PolynomialValues<F>>; NUM_TABLES] (prover.rs:130-142) as they come out of generate_traces, nothing flattened. */
int zkm_prove_segments_columns(zkm_ctx* ctx, const zkm_stark_config* cfg, size_t nseg, const uint64_t* const* const* const* columns,
                               const unsigned* const* log_n, const uint64_t* const* public_values, const size_t* npublic,
                               uint64_t* const* proofs_out, uint64_t* const* ctl_challenges_out, char** err);

/* ------------------------------------------------------------------ staged traces: the NEXT proof's upload behind the CURRENT proof
 * The reference commits from host Vecs (prover.rs:144-167).  A prove call handed a host trace pipelines the upload INSIDE the proof
 * (column chunks absorbed as they arrive: zkm_batch_commit_values); a driver that has the next segment's trace while the current one is
 * being proven -- the witness generator runs ahead of the prover -- stages it instead: zkm_trace_stage[_columns] queues the upload of
 * an ncols x 2^log_n host matrix on the context's two copy streams (alternate pieces of >= 64 MB: 8 columns at 2^20 rows, a short table in one copy) into a block of the context's
 * allocator and RETURNS AT ONCE; zkm_staged_ptr gives the device matrix to pass as `trace` / `traces[k]` of a later prove call ON THE
 * SAME CONTEXT, ordered behind the upload on the context's compute stream (a device-side wait; NULL on a runtime error).  A prove
 * call orders EVERY stream it uses (the context's compute and copy streams, its commit lanes' compute and copy streams) behind what was
 * queued on the context's compute stream before the call -- these waits, the canonicalising pass below, anything the caller wrote on
 * zkm_ctx_stream -- with device-side waits: no stream of the call reads a staged matrix before it has landed.  That call runs the
 * device-resident path at full speed while the copy engines bring in the trace after it.
 *   canonical   nonzero: the caller vouches that every word is < p; 0: the staged copy is canonicalised once when first consumed
 *   host memory pinned (zkm_host_alloc, or a Vec under zkm_host_register): the copies are asynchronous.  Pageable memory works and
 *               makes zkm_trace_stage itself take the time of the upload (the runtime stages it through its own pinned buffer).
 *   The host matrix must stay valid and unchanged until zkm_staged_ready(h, ..) returns 1 or zkm_staged_free(h) has returned.
 * zkm_staged_ready: 1 = uploaded, 0 = in flight (wait = 0 only), -1 = runtime error.  zkm_staged_free waits for the upload and returns
 * the block; call it after the prove call that consumed the matrix has returned. */
typedef struct zkm_staged zkm_staged;
int zkm_trace_stage(zkm_ctx* ctx, const uint64_t* values, size_t ncols, unsigned log_n, int canonical, zkm_staged** out, char** err);
int zkm_trace_stage_columns(zkm_ctx* ctx, const uint64_t* const* columns, size_t ncols, unsigned log_n, int canonical, zkm_staged** out,
                            char** err);
/* All twelve tables of ONE segment in one call (Table::all() order; traces[t]: zkm_table_width x 2^log_n[t] words, or columns[t][i]): one
 * device block, one pair of events; zkm_staged_segment_ptrs gives the twelve device matrices to pass as traces[s] of zkm_prove_segments.
 * A lock-step call of K segments then costs K stage calls instead of 12 K. */
int zkm_segment_stage(zkm_ctx* ctx, const uint64_t* const* traces, const unsigned* log_n, int canonical, zkm_staged** out, char** err);
int zkm_segment_stage_columns(zkm_ctx* ctx, const uint64_t* const* const* columns, const unsigned* log_n, int canonical, zkm_staged** out,
                              char** err);
int zkm_staged_segment_ptrs(zkm_staged* staged, const uint64_t** ptrs_out);
const uint64_t* zkm_staged_ptr(zkm_staged* staged);
int zkm_staged_ready(zkm_staged* staged, int wait);
void zkm_staged_free(zkm_staged* staged);

/* ------------------------------------------------------------------ N3: a whole segment from its raw operations
 * Traces::into_tables (witness/traces.rs:230-320) on the device: the reference's Traces, one group of fields per field of it in its
 * order.  Every list keeps the layout of the entry point named beside it; pointers are host (pageable or pinned) or device memory,
 * except the two sponge offset arrays, which must be host memory.  A count may be 0 (its pointers may then be NULL): the table is
 * padding only, min_rows high.
 *   cpu_rows    Vec<CpuColumnsView<F>> as it is: ncpu_rows x ZKM_CPU_COLS words, row-major; ncpu_rows a power of two, at most 2^28
 *               (simulate_cpu pads to one, generation/mod.rs:170-185).  Words may be non-canonical: column c of row r of the table is
 *               cpu_rows[r * ZKM_CPU_COLS + c] mod p.
 *   every other list   as its zkm_*_trace entry point; sha_extend_sponge_* are complete 48-round schedules (w16, meta), sha_compress_* and
 *               sha_compress_sponge_* one {hx, w, meta} per compression. */
typedef struct {
    const uint64_t* cpu_rows; size_t ncpu_rows;
    const uint32_t* arithmetic_ops; size_t narithmetic;                                      /* zkm_arithmetic_trace */
    const uint32_t* logic_ops; size_t nlogic;                                                /* zkm_logic_trace */
    const uint64_t* memory_ops; size_t nmemory;                                              /* zkm_memory_trace */
    const uint64_t* poseidon_inputs; const uint64_t* poseidon_timestamps; size_t nposeidon;  /* zkm_poseidon_trace_inputs */
    const uint8_t* poseidon_sponge_inputs; const uint64_t* poseidon_sponge_off; const uint64_t* poseidon_sponge_meta;
    size_t nposeidon_sponge;                                                                 /* zkm_poseidon_sponge_trace */
    const uint64_t* keccak_inputs; const uint64_t* keccak_timestamps; size_t nkeccak;        /* zkm_keccak_trace */
    const uint8_t* keccak_sponge_inputs; const uint64_t* keccak_sponge_off; const uint64_t* keccak_sponge_meta;
    size_t nkeccak_sponge;                                                                   /* zkm_keccak_sponge_trace */
    const uint8_t* sha_extend_inputs; const uint64_t* sha_extend_timestamps; size_t nsha_extend;   /* zkm_sha_extend_trace (rows) */
    const uint32_t* sha_extend_sponge_w16; const uint64_t* sha_extend_sponge_meta; size_t nsha_extend_sponge;   /* zkm_sha_extend_sponge_trace */
    const uint32_t* sha_compress_hx; const uint32_t* sha_compress_w; const uint64_t* sha_compress_meta; size_t nsha_compress;   /* zkm_sha_compress_trace */
    const uint32_t* sha_compress_sponge_hx; const uint32_t* sha_compress_sponge_w; const uint64_t* sha_compress_sponge_meta;
    size_t nsha_compress_sponge;                                                             /* zkm_sha_compress_sponge_trace */
} zkm_segment_ops;

/* zkm_segment_tables: the twelve tables of the segment (Table::all() order) in ONE block of the context's allocator.
 *   log_n_out[12]   the reference's heights, min_rows = max(2^cfg->cap_height, 64) (traces.rs:246-247, MIN_TRACE_LEN all_stark.rs:115):
 *                   Arithmetic max(2^16, next_pow2(rows)); Cpu ncpu_rows; Poseidon pow2(max(nposeidon, min_rows)); PoseidonSponge
 *                   pow2(max(sum(len / 32 + 1), min_rows)); Keccak pow2(max(24 nkeccak, min_rows)); KeccakSponge pow2(max(sum(len / 136 + 1),
 *                   min_rows)); ShaExtend pow2(max(nsha_extend, min_rows)); ShaExtendSponge pow2(max(48 nsha_extend_sponge, min_rows));
 *                   ShaCompress pow2(max(65 nsha_compress, min_rows)); ShaCompressSponge pow2(max(nsha_compress_sponge, min_rows)); Logic
 *                   pow2(max(nlogic, min_rows)); Memory zkm_memory_trace's natural height.  Each table is word for word what its entry
 *                   point writes at that height (the Poseidon padding row is the permutation of zero).
 *   out             a segment-shaped zkm_staged (zkm_staged_segment_ptrs / _ready / _free; traces[s] of zkm_prove_segments).  The call
 *                   returns once the tables are complete: the handle is never an upload in flight.  NULL: sizing only -- log_n_out is
 *                   filled (the device still finds the Memory and Arithmetic heights) and nothing is allocated.
 * Fails (nonzero, a message naming the table) on every refusal of the per-table entry points, on CPU rows that are not a power of two
 * or more than 2^28, a NULL pointer with a nonzero count, zero memory operations, and a table of more than 2^28 rows.  A failure leaves
 * the context usable and its live memory as it was.  At most three host waits: the Memory key widths with the Arithmetic row count and
 * flags, the Memory row count, the writers' validation flags.  CPU rows in host memory are copied in row pieces on the context's copy
 * streams (asynchronous from pinned memory) while the other tables are generated. */
int zkm_segment_tables(zkm_ctx* ctx, const zkm_stark_config* cfg, const zkm_segment_ops* ops, unsigned* log_n_out, zkm_staged** out,
                       char** err);
/* zkm_segment_tables, zkm_prove_segment on the block, the block freed: into_tables + prove_with_traces (generation/mod.rs:25-76) in
 * one call.  Outputs as zkm_prove_segment; proofs_out = NULL sizes them (proof_offsets_out[13]) -- unlike zkm_prove_segment's sizing
 * pass this one needs the context, for the Memory and Arithmetic heights. */
int zkm_prove_segment_ops(zkm_ctx* ctx, const zkm_stark_config* cfg, const zkm_segment_ops* ops, const uint64_t* public_values, size_t npublic,
                          uint64_t* proofs_out, size_t* proof_offsets_out, uint64_t* ctl_challenges_out, char** err);

/* K segments' tables in one call: K x Traces::into_tables with the segment as a grid dimension -- every generation kernel is launched
 * ONCE for all K (heights may differ: the grid is the largest segment's), and the call has the THREE host waits of zkm_segment_tables
 * whatever K (one download each of all K key widths and Arithmetic counts, all K Memory row counts, all K validation flag triples).
 *   ops         nseg zkm_segment_ops, each as zkm_segment_tables takes it (any mix of pageable, pinned and device memory, or the
 *               pointers of zkm_staged_ops_get); more than 32 segments are built in consecutive groups
 *   log_n_out   log_n_out[12 * s + t]: height of table t (Table::all() order) of segment s
 *   out         out[s]: a segment-shaped zkm_staged each (one block per segment: free each on its own), word for word what
 *               zkm_segment_tables gives for that segment alone.  NULL: sizing only.
 * Every refusal of zkm_segment_tables applies per segment; the message names the segment's position in the call before the table
 * ("zkm_segments_tables: segment 1: Logic: ...").  nseg = 0 and NULL ops are refused.  A failure leaves the context usable, its live
 * memory as it was, and no handle behind. */
int zkm_segments_tables(zkm_ctx* ctx, const zkm_stark_config* cfg, size_t nseg, const zkm_segment_ops* ops, unsigned* log_n_out,
                        zkm_staged** out, char** err);
/* zkm_segments_tables, zkm_prove_segments on the blocks (lock-step: one launch per stage for all of them), the blocks freed: K x
 * (into_tables + prove_with_traces) in one call.  public_values / npublic / proofs_out / ctl_challenges_out as zkm_prove_segments;
 * every blob and every challenge is word for word what zkm_prove_segment_ops returns for that segment alone.
 *   proof_offsets_out   proof_offsets_out[13 * s + i] as zkm_prove_segment_ops gives them for segment s (may be NULL when proving)
 *   proofs_out = NULL   sizing: only the heights are found (two host waits per 32 segments) and proof_offsets_out is filled
 * More than 32 segments, or more than the context's "segments_memory_budget" holds -- estimated as for zkm_prove_segments, plus the
 * built tables and the staging block -- are built and proven in consecutive, equally sized waves; the words do not depend on the
 * waves.  Refusals and failures as zkm_segments_tables and zkm_prove_segments (positions are those in the call). */
int zkm_prove_segments_ops(zkm_ctx* ctx, const zkm_stark_config* cfg, size_t nseg, const zkm_segment_ops* ops,
                           const uint64_t* const* public_values, const size_t* npublic, uint64_t* const* proofs_out, size_t* proof_offsets_out,
                           uint64_t* const* ctl_challenges_out, char** err);

/* Staged operations: the NEXT call's lists behind the CURRENT proofs (the counterpart of zkm_segment_stage for operations).  Every
 * byte count of a segment's lists is known on the host, so zkm_segment_ops_stage queues the uploads -- one block of the context's
 * allocator for the CPU rows and every list, alternate pieces on the context's two copy streams, behind what the compute stream has
 * queued -- and RETURNS AT ONCE.  The checks that need no device (NULL pointers, the CPU row count, the sponge offsets, zero memory
 * operations) run here and refuse here.
 *   zkm_staged_ops_get     the same segment with device pointers, for zkm_segment[s]_tables / zkm_prove_segment[s]_ops ON THE SAME
 *                          CONTEXT (another context is refused): that call is ordered behind the upload on the device -- the compute
 *                          stream waits for the copies, every other stream of the call waits for the compute stream -- with no host
 *                          wait.  The two sponge offset arrays, which the builder reads on the host, point at the handle's own copy.
 *   zkm_staged_ops_ready   1: the uploads have landed -- every list of the caller, offsets included, may be reused; 0: in flight;
 *                          -1: a runtime error.  wait != 0 blocks until they have.
 *   zkm_staged_ops_free    after the call that consumed the handle has returned (waits for the uploads, releases the block). */
typedef struct zkm_staged_ops zkm_staged_ops;
int zkm_segment_ops_stage(zkm_ctx* ctx, const zkm_segment_ops* ops, zkm_staged_ops** out, char** err);
int zkm_staged_ops_get(zkm_staged_ops* staged, zkm_segment_ops* ops_out);
int zkm_staged_ops_ready(zkm_staged_ops* staged, int wait);
void zkm_staged_ops_free(zkm_staged_ops* staged);

/* ------------------------------------------------------------------ a segment's bootstrap kernel from its image
 * generate_bootstrap_kernel (prover/src/cpu/bootstrap_kernel.rs:26-306, the first thing generate_traces does) on the device: the rows
 * that write the segment's memory image into (context 0, Segment::Code) eight words a row, the Poseidon sponge over each 4 KiB page
 * with the check of its digest against the image's hash words (the root page against pre_hash_root), and the image id over the root
 * and the entry pc.  Everything it pushes into Traces is a function of the image, so the caller hands over 8 bytes a word instead of
 * the CPU rows, memory operations, Poseidon inputs and sponge operations made from them (about 530 KB a page).  Bootstrap only: the
 * reference's exit kernel has no caller and is not built.
 *   addrs / values   the image as nwords pairs in BTreeMap order: addrs strictly ascending multiples of 4; host or device memory
 *   npages           addresses with addr & 0xFFF == 0 (checked on the device); each is hashed as a page, absent words reading as 0
 *   check            nonzero: the three assert_eq of the reference (page hash, root hash, image id) refuse the call
 * With R = ceil(nwords / 8) and P = npages the bootstrap gives R + P + 3 CPU rows, nwords + 4096 P + 45 memory operations, 129 P + 2
 * Poseidon inputs and P + 1 sponge operations of 129 P + 2 rows (zkm_boot_counts; pure, any pointer may be NULL), all of them BEFORE
 * what simulate_cpu pushes. */
typedef struct zkm_boot_image {
    const uint32_t* addrs; const uint32_t* values; size_t nwords;
    size_t npages;
    uint32_t entry, check;
    uint8_t pre_hash_root[32], pre_image_id[32];
} zkm_boot_image;
void zkm_boot_counts(const zkm_boot_image* image, size_t* cpu_rows, size_t* memory_ops, size_t* poseidon_inputs, size_t* sponge_ops,
                     size_t* sponge_rows);
/* zkm_segment[s]_tables / zkm_prove_segment[s]_ops with the bootstrap built from `image` (one per segment) in front of `ops`:
 *   ops   what simulate_cpu pushed only; its CPU rows carry clocks from R + P + 3 on and are transposed behind the bootstrap's rows, its
 *         Poseidon inputs, sponge operations and memory operations follow the bootstrap's.  (R + P + 3) + ops->ncpu_rows must be a power
 *         of two; nmemory may be 0.  The device pointers of zkm_staged_ops_get are accepted as ops; images themselves are not staged,
 *         and the pool takes them beside a segment's steps and calls (zkm_pool_prove_segments_calls).
 * Heights are those of into_tables on the joined lists; "check_ctls", "verify", waves, memory budget and sizing mode as in the calls
 * without an image, and so are the three host waits whatever K: the sponge chains run on a second stream beside the Memory, Arithmetic
 * and Logic tables, and the digest checks ride on the third wait (sizing mode therefore makes the first two kinds of refusal only).
 * Refused (nonzero; the message names the segment's position in calls of several, the table "Cpu" and the address):
 *   an address that is not a multiple of 4 above the one before it; npages that is not the image's count; a page whose hash words at
 *   0x80000000 + ((addr >> 12) << 5) are not all in the image; with `check`, a page hash, root hash or image id mismatch; a row count
 *   that is not a power of two.
 * A refusal leaves the context usable and its live memory as it was. */
int zkm_segment_tables_boot(zkm_ctx* ctx, const zkm_stark_config* cfg, const zkm_boot_image* image, const zkm_segment_ops* ops, unsigned* log_n_out,
                            zkm_staged** out, char** err);
int zkm_segments_tables_boot(zkm_ctx* ctx, const zkm_stark_config* cfg, size_t nseg, const zkm_boot_image* images, const zkm_segment_ops* ops,
                             unsigned* log_n_out, zkm_staged** out, char** err);
int zkm_prove_segment_ops_boot(zkm_ctx* ctx, const zkm_stark_config* cfg, const zkm_boot_image* image, const zkm_segment_ops* ops,
                               const uint64_t* public_values, size_t npublic, uint64_t* proofs_out, size_t* proof_offsets_out,
                               uint64_t* ctl_challenges_out, char** err);
int zkm_prove_segments_ops_boot(zkm_ctx* ctx, const zkm_stark_config* cfg, size_t nseg, const zkm_boot_image* images, const zkm_segment_ops* ops,
                                const uint64_t* const* public_values, const size_t* npublic, uint64_t* const* proofs_out,
                                size_t* proof_offsets_out, uint64_t* const* ctl_challenges_out, char** err);
/* The bootstrap's kernels alone (tests and tools): device outputs sized by zkm_boot_counts -- cpu_rows_out cpu_rows x ZKM_CPU_COLS words
 * row-major, memory_ops_out memory_ops x 6 words (zkm_memory_trace's layout), poseidon_inputs_out n x 12 with poseidon_ts_out n,
 * digests_out sponge_ops x 4.  Refusals as above.  Two host waits. */
int zkm_boot_witness(zkm_ctx* ctx, const zkm_boot_image* image, uint64_t* cpu_rows_out, uint64_t* memory_ops_out, uint64_t* poseidon_inputs_out,
                     uint64_t* poseidon_ts_out, uint64_t* digests_out, char** err);

/* ------------------------------------------------------------------ a segment's CPU table from a compact step log
 * The row filling of witness/operation.rs (the generate_* functions that turn the values an instruction read into columns) on the
 * device.  The emulator's fetch, decode and execute stay on the host: instead of a 259-word CpuColumnsView a cycle it records one
 * zkm_cpu_step, 48 bytes, and the step at position i of the list becomes
 *   row first_clock + i of the CPU table, written column-major straight into the table (clock = first_clock + i);
 *   its memory operations (zkm_memory_trace's 6 words, context 0 for registers and the shift table, timestamp clock * 10), its logic
 *   operation and its arithmetic operation ({op, in0, in1} as zkm_logic_trace / zkm_arithmetic_trace take them; results are computed
 *   on the device), each list in the order the reference pushes: per row the order of the generator's reg_read / reg_write /
 *   mem_read / mem_write calls, which is not channel order (binary_imm writes rt on channels 1 and 2; syscall uses channels 0-3, then
 *   6 and 7, then 4 and 5).  A write to register 0 fills its channel with used = 0 and pushes nothing (witness/util.rs:198-204).
 *   pc, next_pc   program_counter and next_program_counter of the row, both from before the step (next_pc is the delay-slot value)
 *   insn          the instruction word; its 32 bits fill the six bit fields of the row
 *   kind          ZKM_STEP_*, below
 *   flags         bit 0: kernel mode; bit 1 (ZKM_STEP_FLAG_BRANCH_R0), BRANCH against zero only: channel 1 reads register 0 whatever the
 *                 rt field (the reference decodes BGEZ so); bits 8-11, SYSCALL only: ZKM_SYSCALL_* (the branch of generate_syscall taken)
 *   context       the row's context, and the context of a load's / store's memory channels
 *   reads         the values the step reads through the memory channels, in the order the generator reads them: register reads, then
 *                 memory reads (RDHWR of register 29: the one read follows the write)
 * Kinds, one per op flag that has a witness model (tests/cpu_fixtures.py Machine), each with exactly these encodings:
 *   BINARY_OP ADD ADDU SUB SUBU SLT SLTU; BINARY_IMM_OP ADDI ADDIU SLTI SLTIU; LOGIC_OP AND OR XOR NOR; LOGIC_IMM_OP ANDI ORI XORI
 *   (pushes no logic operation, as the reference); SHIFT SLLV SRLV SRAV;
 *   SHIFT_IMM SLL SRL SRA (rs = 0); BRANCH BEQ BNE BLEZ BGTZ BLTZ BGEZ (channel 1 reads the register the rt field names, see flags);
 *   JUMPS JR JALR; JUMPI J JAL; JUMPDIRECT BAL; M_OP_LOAD LB LH LWL LW LBU LHU LWR LL; M_OP_STORE SB SH SWL SW SWR SC; NOP (word 0);
 *   CLZ_OP; CLO_OP; SIGNEXT8 SEB; SIGNEXT16 SEH; SWAPHALF WSBH; RDHWR; MOVZ_OP; MOVN_OP; TEQ (operands that differ); EXT; INS; ROR;
 *   MADDU; SYSCALL (mmap, brk, clone, read, write, fcntl, set_thread_area, other).  Every other encoding is refused.
 *   PAD   the padding row of simulate_cpu (generation/mod.rs:170-185): clock, context, pc, next_pc and is_exit_kernel = 1
 *   RAW   reads[0] indexes a ready-made row in raw_rows (nraw x ZKM_CPU_COLS words row-major, any representative mod p, host or device
 *         memory); reads[1] has bit k set for each of the eight channels k whose `used` cell is 1 -- the counts and the operations
 *         follow this mask.  Rows in host memory are held to it on the walk (a mismatch is refused), and so is every row, in host or
 *         device memory, on the device walk (zkm_cpu_steps_scan, zkm_cpu_steps_stage, below); only the host walk of an unstaged
 *         call leaves rows in device memory unread: there a mismatch is not detected, and a used channel the mask leaves out
 *         pushes nothing.  The row is copied canonical and the masked
 *         channels become memory operations in ascending channel order, timestamped from the row's OWN clock cell (every other
 *         kind: first_clock + position); no logic or arithmetic operation.  The escape for everything the kinds do not cover: keccak_general and the precompile rows, a bootstrap row
 *         handed over by the caller, a register written outside an instruction.
 * `steps` is host memory (pageable or pinned), or what zkm_staged_steps_get hands out; the library walks host memory once on the host, and every refusal -- an unknown kind, an encoding
 * the kind does not take, a RAW index >= nraw, a RAW mask that is not its host row's, a NULL pointer with a nonzero count -- is made
 * on that walk, before any device work, and names the step's index.  The counts of a step are a function of its record alone
 * (csrc/cpu_steps_dev.h, one __host__ __device__ function for the walk and the kernels).
 *   zkm_cpu_steps_counts   the three list lengths of a step list; needs no GPU
 *   zkm_cpu_witness        the kernels alone (tests and tools): cpu_out_dev ZKM_CPU_COLS x 2^log_n words column-major, zero outside rows
 *                          [first_clock, first_clock + nsteps), which must fit; memory_ops_out_dev n x 6 words, logic_ops_out_dev and
 *                          arithmetic_ops_out_dev n x 3 uint32, sized by zkm_cpu_steps_counts (a list of count 0 may be NULL).
 *                          Returns once the outputs are complete (one host wait).
 *   zkm_segments_tables_steps / zkm_prove_segments_ops_steps   zkm_segments_tables[_boot] / zkm_prove_segments_ops[_boot] with the CPU
 *                          rows built from steps[s]: ops[s].cpu_rows must be NULL with ncpu_rows 0; images may be NULL (no bootstrap);
 *                          first_clock is the bootstrap's row count.  The joined Memory, Logic and Arithmetic lists are the
 *                          bootstrap's, then the steps', then ops[s]'s own (the Memory sort is stable).  (bootstrap rows) + nsteps
 *                          must be a power of two: the caller appends PAD steps as simulate_cpu does.  Heights are those of
 *                          into_tables on the joined lists; "check_ctls", "verify", waves, memory budget and sizing mode as in the
 *                          calls without steps, and so are the three host waits whatever K: the step path adds none.  Every table,
 *                          blob and challenge is word for word what the calls without steps give for the expanded rows and lists.
 * Steps are staged by zkm_cpu_steps_stage (below; zkm_segment_ops_stage takes none), the pool takes them as
 * zkm_segment_calls without calls (zkm_pool_prove_segments_calls), kinds outside the list go RAW (the thirteen other
 * encodings decode() accepts as rows expanded on the device: zkm_insn_rows_* below), and there is no exit
 * kernel.  Profile scopes cpu_steps/lists and cpu_steps/rows (zkm_cpu_witness: cpu_steps/rows_lists). */
#define ZKM_STEP_BINARY_OP 0
#define ZKM_STEP_BINARY_IMM_OP 1
#define ZKM_STEP_LOGIC_OP 2
#define ZKM_STEP_LOGIC_IMM_OP 3
#define ZKM_STEP_SHIFT 4
#define ZKM_STEP_SHIFT_IMM 5
#define ZKM_STEP_BRANCH 6
#define ZKM_STEP_JUMPS 7
#define ZKM_STEP_JUMPI 8
#define ZKM_STEP_JUMPDIRECT 9
#define ZKM_STEP_M_OP_LOAD 10
#define ZKM_STEP_M_OP_STORE 11
#define ZKM_STEP_NOP 12
#define ZKM_STEP_CLZ_OP 13
#define ZKM_STEP_CLO_OP 14
#define ZKM_STEP_SIGNEXT8 15
#define ZKM_STEP_SIGNEXT16 16
#define ZKM_STEP_SWAPHALF 17
#define ZKM_STEP_RDHWR 18
#define ZKM_STEP_MOVZ_OP 19
#define ZKM_STEP_MOVN_OP 20
#define ZKM_STEP_TEQ 21
#define ZKM_STEP_EXT 22
#define ZKM_STEP_INS 23
#define ZKM_STEP_ROR 24
#define ZKM_STEP_MADDU 25
#define ZKM_STEP_SYSCALL 26
#define ZKM_STEP_PAD 27
#define ZKM_STEP_RAW 28
#define ZKM_STEP_FLAG_KERNEL 1u
#define ZKM_STEP_FLAG_BRANCH_R0 2u
#define ZKM_SYSCALL_OTHER 0
#define ZKM_SYSCALL_MMAP 1
#define ZKM_SYSCALL_BRK 2
#define ZKM_SYSCALL_CLONE 3
#define ZKM_SYSCALL_READ 5
#define ZKM_SYSCALL_WRITE 6
#define ZKM_SYSCALL_FCNTL 7
#define ZKM_SYSCALL_SET_THREAD_AREA 8
/* (Layout lock: tests/test_abi.py compares these two structs, like every struct of this header, as the C compiler lays them out with
 * the numpy, ctypes and Rust mirrors.) */
typedef struct zkm_cpu_step { uint32_t pc, next_pc, insn, kind, flags, context; uint32_t reads[6]; } zkm_cpu_step;   /* 48 bytes */
typedef struct zkm_cpu_steps { const zkm_cpu_step* steps; size_t nsteps; const uint64_t* raw_rows; size_t nraw; } zkm_cpu_steps;
int zkm_cpu_steps_counts(const zkm_cpu_steps* steps, size_t* memory_ops, size_t* logic_ops, size_t* arithmetic_ops, char** err);
int zkm_cpu_witness(zkm_ctx* ctx, const zkm_cpu_steps* steps, uint64_t first_clock, unsigned log_n, uint64_t* cpu_out_dev,
                    uint64_t* memory_ops_out_dev, uint32_t* logic_ops_out_dev, uint32_t* arithmetic_ops_out_dev, char** err);
int zkm_segments_tables_steps(zkm_ctx* ctx, const zkm_stark_config* cfg, size_t nseg, const zkm_boot_image* images, const zkm_cpu_steps* steps,
                              const zkm_segment_ops* ops, unsigned* log_n_out, zkm_staged** out, char** err);
int zkm_prove_segments_ops_steps(zkm_ctx* ctx, const zkm_stark_config* cfg, size_t nseg, const zkm_boot_image* images, const zkm_cpu_steps* steps,
                                 const zkm_segment_ops* ops, const uint64_t* const* public_values, const size_t* npublic,
                                 uint64_t* const* proofs_out, size_t* proof_offsets_out, uint64_t* const* ctl_challenges_out, char** err);

/* Staged steps: the NEXT call's step logs behind the CURRENT proofs, walked on the device.  The walk of an unstaged call runs on the
 * calling thread before any device work; here it is two kernels behind the upload (csrc/cpu_steps_walk.hip): a thread per step takes
 * the same counts from the same function, finds the step's first refusal in the host walk's order -- a RAW index >= nraw, an unknown
 * kind, operands or an encoding the kind does not take, a RAW mask that is not the `used` cells of its row -- and a scan over the
 * workgroups' sums gives the three list lengths and the base triples, word for word the host walk's.  The rows of RAW steps are in
 * device memory by then whichever memory the caller had them in, so the mask check covers them all.  Of a refused segment the device
 * keeps the lowest refused step, its record and the mask found, and the message is the host walk's, character for character.
 *   zkm_cpu_steps_scan     the walk alone (tests and tools), for nseg segments in one set of launches: steps[s].steps and raw_rows may be
 *                          host or device memory; counts_out takes 3 words a segment (memory, logic, arithmetic); base_out, which may be
 *                          NULL and whose entries may be NULL, takes segment s's 3 words per 256 steps into HOST memory.  One host
 *                          wait.  A refusal reads "zkm_cpu_steps_scan: segment <s>: step <i>: ...", of the lowest such segment.
 *   zkm_cpu_steps_stage    reads nothing of the lists on the host: one block of the context's allocator for all segments, and, on the
 *                          context's two copy streams behind what the compute stream has queued, the records, the RAW rows that lie in
 *                          host memory, the walk's kernels behind them and the download of the verdicts into pinned memory of the
 *                          handle.  RETURNS AT ONCE, with no host wait.  RAW rows in device memory are referenced, not copied: they
 *                          must live until the handle is freed.  The caller's host lists must stay as they are until
 *                          zkm_staged_steps_ready returns 1.  *out is the handle, which the functions below take (an address to the
 *                          bindings, as every handle is).
 *   zkm_staged_steps_ready 1: uploads, walk and download have ended -- the caller's lists may be reused; 0: in flight; -1: a runtime
 *                          error.  wait != 0 blocks until they have.
 *   zkm_staged_steps_get   waits on the host for the handle's events (long fired when the stage ran behind the previous call; one host
 *                          wait a handle at most), then, for a segment that passed: steps_out with `steps` and `raw_rows` in device
 *                          memory, and the three list lengths (each pointer may be NULL); the compute stream is ordered behind the
 *                          events with a device-side wait, once per handle.  For a refused segment it fails with
 *                          "zkm_staged_steps_get: segment <s>: step <i>: ..."; the other segments of the handle stay usable.
 *   zkm_staged_steps_free  waits for the events, then releases the block (NULL is allowed); after the calls that consumed the handle
 *                          have returned.
 * zkm_segments_tables_steps and zkm_prove_segments_ops_steps ON THE SAME CONTEXT take steps_out as steps[s]: for such a segment the
 * builder does not walk, uploads neither records nor bases and orders its compute stream behind the handle's events itself, and
 * everything else is as for an unstaged segment -- the three host waits, waves, "check_ctls", "check_witness", "verify", and every
 * table, blob and challenge word for word.  Staged and unstaged segments, images and the lists of zkm_staged_ops_get mix in one call.
 * steps_out is taken as it was handed out (a changed count or raw_rows is refused), a handle of another context is refused, and so is
 * a `steps` pointer in device memory that no handle owns.  Refused on the host before any device work, here and in zkm_cpu_steps_scan:
 * NULL with a nonzero count, nseg = 0, nsteps above 2^28 (the builder's own limit: 8 memory operations a step stay below 2^32), a
 * NULL argument.  A refusal leaves the context usable, its live memory as it was and no handle behind.
 * The pool still takes no steps; images and calls (zkm_segments_calls_expand) are still not staged -- in THIS form and by THESE entry
 * points, that is: a pool call takes neither a zkm_cpu_steps list nor a handle of zkm_cpu_steps_stage (a handle is its context's).
 * zkm_segments_calls_stage ("Staged calls", below) stages images and calls, on top of this walk, and the pool takes a step log as a
 * zkm_segment_calls without calls, which its workers stage themselves (zkm_pool_prove_segments_calls).  Profile scope cpu_steps/walk
 * (zkm_cpu_steps_scan only: the staged walk runs on a copy stream). */
int zkm_cpu_steps_scan(zkm_ctx* ctx, size_t nseg, const zkm_cpu_steps* steps, size_t* counts_out, uint32_t* const* base_out, char** err);
int zkm_cpu_steps_stage(zkm_ctx* ctx, size_t nseg, const zkm_cpu_steps* steps, void** out, char** err);
int zkm_staged_steps_ready(void* staged, int wait);
int zkm_staged_steps_get(void* staged, size_t segment, zkm_cpu_steps* steps_out, size_t* memory_ops, size_t* logic_ops, size_t* arithmetic_ops,
                         char** err);
void zkm_staged_steps_free(void* staged);

/* ------------------------------------------------------------------ SHA-256 precompile calls from their inputs
 * What generate_sha_extend and generate_sha_compress (witness/operation.rs:1183-1285, :1298-1458) and their helpers sha_extend_sponge_log
 * and sha_compress_sponge_log (witness/util.rs:559-694) turn one SYSSHAEXTEND / SYSSHACOMPRESS call into, on the device, from the lists
 * the caller hands over for the sponge tables anyway: sha_extend_sponge_w16 / _meta and sha_compress_sponge_hx / _w / _meta of
 * zkm_segment_ops, in the layouts of zkm_sha_extend_sponge_trace and zkm_sha_compress_trace.  With E extend and C compress calls:
 *   cpu_rows          96 E + 11 C   ready-made CpuColumnsView rows for RAW steps.  Extend call e: rows 96 e + 2 r (the read row of round r:
 *                                   channels 0-3 read w[i-15], w[i-2], w[i-16], w[i-7], channel 4 writes w[i], i = r + 16; mask 0x1F) and
 *                                   96 e + 2 r + 1 (its sponge row; mask 0).  Compress call c: rows 96 E + 11 c + 0 .. 10 -- the hx row (eight
 *                                   reads), eight w rows (eight reads each), the sponge row (mask 0), the write row (eight writes of
 *                                   hx[q] + state[q]); mask 0xFF but for the sponge row
 *   memory_ops        768 E + 288 C the SPONGE's reads only (four of each input word, at the sponge row's timestamp), zkm_memory_trace's six
 *                                   words; the operations of the rows' channels are pushed by their RAW steps, as for any RAW row
 *   logic_ops         192 E + 768 C {op, in0, in1}: a round's four XORs / twelve operations, from xor(e ror 6, e ror 11) through
 *                                   xor(maj_inter, b & c), in the generators' push order
 *   sha_extend_rows   48 E          the ShaExtend table's inputs (16 bytes: w[i-15], w[i-2], w[i-16], w[i-7] little-endian) and timestamps
 * Every list holds all extend calls in list order, round by round, then all compress calls in list order, round by round.
 * A row holds exactly what the generators put into a CpuColumnsView::default(): clock; the six cells of each used channel (context, segment
 * and address from the meta -- w's own context and segment for the w rows of a compress call; is_read; value); on a sponge row
 * is_sha_extend_sponge / is_sha_compress_sponge, the values of channels 0-2 with used = 0 (context, segment, and the address of w[i] /
 * of hx[0]) and general.element.value = w[i] / general.shash.value[q] = hx[q] + state[q].  Every other cell is 0.
 * Clocks follow from the meta's timestamp, the sponge row's: S = timestamp / 10 (NUM_CHANNELS).  Extend: round r's sponge row at S + 2 r
 * (the meta's timestamp is round 0's; zkm_sha_extend_sponge_trace stamps round r timestamp + 20 r), its read row one clock before.
 * Compress: the hx row at S - 9, w row k at S - 8 + k, the sponge row at S, the write row at S + 1.
 *   zkm_sha_calls_counts    the four counts above (any out pointer may be NULL); pure: no context, no GPU
 *   zkm_sha_calls_steps     pure.  The cpu_rows RAW records (reads[0] = raw_base + j for row j: raw_base is where the generated rows start in
 *                           the caller's raw_rows block; reads[1] = the row's channel mask; every other field 0) into steps_out, and the clock
 *                           each belongs at into clocks_out: the caller puts record j at position clocks_out[j] - first_clock of its step
 *                           list.  THE statement of masks and positions: the binding, the Rust recorder and the kernel's indexing follow it.
 *                           The meta lists are host memory here (device memory is refused), and raw_base + cpu_rows must fit in 32 bits.
 *   zkm_sha_calls_witness   the kernel (one launch for all calls of both kinds, one workgroup a call).  The five lists may be host or device
 *                           memory; the five outputs are plain device pointers, so each may aim into the middle of a larger block (own RAW
 *                           rows, own operations in front): raw_rows_out_dev cpu_rows x ZKM_CPU_COLS words row-major, canonical;
 *                           memory_ops_out_dev memory_ops x 6 words; logic_ops_out_dev logic_ops x 3 uint32; sha_extend_inputs_out_dev
 *                           48 E x 16 bytes; sha_extend_timestamps_out_dev 48 E words (8-byte aligned; 4 for the logic operations and the
 *                           inputs).  Returns once the outputs are complete: one host wait.  Profile scope sha_calls/rows_lists.
 * Refused by both, on the host before any device work, the message naming the list (extend_meta, compress_meta, extend_w16, compress_hx,
 * compress_w) and the call's position in it: a NULL list with a nonzero count; a timestamp that is not a multiple of 10 or too small for
 * the call's first row to have a clock >= 0; an address whose last word (w[63], hx[7], the 65th round's dummy address w + 256) does not fit
 * in 32 bits; a context or segment of 2^32 or more.  zkm_sha_calls_witness also refuses a NULL output with a nonzero count, and makes every
 * refusal before it reports a missing context; a refusal leaves the context usable.  A meta list in DEVICE memory is not read by the host
 * and so not held to these rules: its words go into the rows and lists as they are (no store's address depends on them).
 * Out of scope: the Keccak calls have their own expansion (the next section), and the Poseidon sponge has no syscall in the reference (only
 * the bootstrap produces such operations); the SYSCALL row in front of a
 * call stays whatever the caller logs today; nothing is staged by THIS entry point (zkm_segments_calls_stage does, and the pool takes
 * calls: zkm_pool_prove_segments_calls), and nothing is fused into the segment builder -- the
 * expansion is a call of its own with its own host wait, and its outputs go into zkm_cpu_steps.raw_rows and the lists of zkm_segment_ops,
 * all of which may be device memory. */
void zkm_sha_calls_counts(size_t nextend, size_t ncompress, size_t* cpu_rows, size_t* memory_ops, size_t* logic_ops, size_t* sha_extend_rows);
int zkm_sha_calls_steps(const uint64_t* extend_meta, size_t nextend, const uint64_t* compress_meta, size_t ncompress, size_t raw_base,
                        zkm_cpu_step* steps_out, uint64_t* clocks_out, char** err);
int zkm_sha_calls_witness(zkm_ctx* ctx, const uint32_t* extend_w16, const uint64_t* extend_meta, size_t nextend, const uint32_t* compress_hx,
                          const uint32_t* compress_w, const uint64_t* compress_meta, size_t ncompress, uint64_t* raw_rows_out_dev,
                          uint64_t* memory_ops_out_dev, uint32_t* logic_ops_out_dev, uint8_t* sha_extend_inputs_out_dev,
                          uint64_t* sha_extend_timestamps_out_dev, char** err);

/* ------------------------------------------------------------------ SYSKECCAK precompile calls from their input bytes
 * What generate_keccak (witness/operation.rs:1101-1181) and its helper keccak_sponge_log (witness/util.rs:471-557, with xor_into_sponge,
 * :724-741) turn one SYSKECCAK call into, on the device, from the lists the caller hands over for the KeccakSponge table anyway:
 * keccak_sponge_inputs / _off / _meta of zkm_segment_ops, in the layout of zkm_keccak_sponge_trace, with ZKM_SPONGE_BYTE_ADDRESSED set in
 * every meta's virt_base (a call reads one memory word every 4 bytes), and one more word a call: digest_addrs, the address the digest is
 * written to (a2).  For a call of L input bytes in W = ceil(L / 4) memory words, with R = ceil(W / 8) and B = L / 136 + 1:
 *   cpu_rows      R + 2    ready-made CpuColumnsView rows for RAW steps: read row j (channels 0 .. min(8, W - 8 j) - 1 read word 8 j + i at
 *                          base + 4 (8 j + i), the value the big-endian reading of the word's four bytes in the padded message -- the
 *                          input bytes, and in the last word of a length that is no multiple of 4 the padding behind them, see
 *                          ZKM_SPONGE_PADDED_TAIL below; mask = that many low bits), the sponge row (mask 0: is_keccak_sponge; the values of channels 0-3 with used = 0 are context, segment,
 *                          the address of word (L / 136) * 34 -- 0 if the input has no such word -- and L; general.khash.value[i] the
 *                          big-endian reading of digest bytes 4 (7 - i) ..), the write row (mask 0xFF: channel i writes the big-endian
 *                          reading of digest bytes 4 i .. to digest_addr + 4 i).  Every other cell is 0
 *   memory_ops    L        the SPONGE's reads only, zkm_memory_trace's six words: one a byte, of the word that holds it, in byte order, at
 *                          the sponge row's timestamp; the operations of the rows' channels are pushed by their RAW steps
 *   logic_ops     34 B     {XOR, lhs, rhs}, block by block: lhs the state's 32-bit word before the absorption, rhs the padded block's word,
 *                          both little-endian; the last block carries pad10*1
 *   keccak_perms  B        the KeccakStark inputs (25 words: the state after the XOR, before the permutation) and timestamps (the sponge
 *                          row's)
 * Every list holds the calls in list order; call k's items start at the sum of the earlier calls' counts.  Context and segment come from
 * the meta (the reference hard-codes 0 and Segment::Code: for its callers the rows are identical).  Clocks follow from the meta's
 * timestamp, the sponge row's: S = timestamp / 10 (NUM_CHANNELS); read row j at S - R + j, the sponge row at S, the write row at S + 1.
 *   zkm_keccak_calls_counts   the four totals (any out pointer may be NULL); pure: no context, no GPU.  Without metas it takes lengths that
 *                             are multiples of 4 only
 *   zkm_keccak_calls_counts_meta   the same totals for calls of any length: meta as below (host memory; a list in device memory is
 *                             not read) says which calls carry ZKM_SPONGE_PADDED_TAIL.  With meta NULL it is zkm_keccak_calls_counts,
 *                             and its refusals are that function's, under that function's name.  Pure
 *   zkm_keccak_calls_steps    pure.  The cpu_rows RAW records (reads[0] = raw_base + j, reads[1] = the row's channel mask, every other field
 *                             0) into steps_out and the clock each belongs at into clocks_out, as zkm_sha_calls_steps does.  THE statement
 *                             of masks and positions: the binding, the Rust recorder and the kernel's indexing follow it.  meta is host
 *                             memory here, and raw_base + cpu_rows must fit in 32 bits.
 *   zkm_keccak_calls_witness  the kernel (one launch, one workgroup a call).  input_off is host memory; inputs, meta and digest_addrs may be
 *                             host or device memory; the five outputs are plain device pointers, so each may aim into the middle of a
 *                             larger block: raw_rows_out_dev cpu_rows x ZKM_CPU_COLS words row-major, canonical; memory_ops_out_dev
 *                             memory_ops x 6 words; logic_ops_out_dev logic_ops x 3 uint32 (4-byte aligned, the others 8);
 *                             keccak_inputs_out_dev keccak_perms x 25 words; keccak_timestamps_out_dev keccak_perms words.  Returns once
 *                             the outputs are complete: one host wait.  Profile scope keccak_calls/rows_lists.
 * Refused, on the host before any device work and before a missing context is reported, the message naming the list (input_off, meta,
 * digest_addrs, inputs, or the output) and the call's position: a NULL list or output with a nonzero count; input_off in device memory;
 * offsets that do not increase; a length that is 0, or not a multiple of 4 in a call without ZKM_SPONGE_PADDED_TAIL; a meta without
 * ZKM_SPONGE_BYTE_ADDRESSED; a timestamp that is
 * not a multiple of 10 or too small for the first read row's clock to be >= 0; base + 4 (W - 1) or digest_addr + 28 that does not fit in
 * 32 bits; a context or segment of 2^32 or more; raw_base + cpu_rows that does not fit in 32 bits; an output that is not aligned to its
 * words.  A refusal leaves the context usable.  meta or digest_addrs in DEVICE memory is not read by the host and so not held to these
 * rules (no store's address depends on them); such a list takes lengths that are multiples of 4 only.
 * Lengths that are not a multiple of 4: the last memory word then holds more than input bytes, and only one value of it can be proven.
 * The guest runtime writes it as the remaining 1-3 input bytes, 0x01, then zeros, with 0x80 in its fourth byte when the word is the last
 * of a 136-byte block (runtime/precompiles/src/io.rs:128-144); the sponge's reads of the remainder carry exactly that word (rem_data,
 * witness/util.rs:513-535), the KeccakSponge table looks the final block's bytes up in memory with the padding in them
 * (keccak_sponge_stark.rs:88-124, :319-347), and the Memory table makes every read of one address agree -- so the word is the padded
 * message's, a function of the input bytes and L (0x81 in the fourth byte when L % 136 == 135).  The caller that has seen the call read
 * that word sets ZKM_SPONGE_PADDED_TAIL in the meta's virt_base, beside ZKM_SPONGE_BYTE_ADDRESSED: the call is then expanded with the
 * padded word in its last read channel and in the sponge's reads of the last 1-3 bytes, and nothing else of a call depends on L % 4.
 * Without the flag (or with meta in device memory, which the host does not read) such a length is refused as before; the call can
 * still travel as RAW rows and the caller's own lists beside a flagged sponge operation.  For a multiple of 4 the flag changes nothing.
 * Every entry point that takes these lists with their metas -- zkm_keccak_calls_steps, zkm_keccak_calls_witness and the segment entry
 * points built on them (zkm_segment_calls_steps, zkm_segments_calls_expand, zkm_segments_tables_calls, zkm_prove_segments_ops_calls,
 * zkm_segments_calls_stage, zkm_pool_prove_segments_calls) -- takes flagged calls of any length. */
int zkm_keccak_calls_counts(const uint64_t* input_off, size_t ncalls, size_t* cpu_rows, size_t* memory_ops, size_t* logic_ops,
                            size_t* keccak_perms, char** err);
int zkm_keccak_calls_counts_meta(const uint64_t* input_off, const uint64_t* meta, size_t ncalls, size_t* cpu_rows, size_t* memory_ops,
                                 size_t* logic_ops, size_t* keccak_perms, char** err);
int zkm_keccak_calls_steps(const uint64_t* input_off, const uint64_t* meta, size_t ncalls, size_t raw_base, zkm_cpu_step* steps_out,
                           uint64_t* clocks_out, char** err);
int zkm_keccak_calls_witness(zkm_ctx* ctx, const uint8_t* inputs, const uint64_t* input_off, const uint64_t* meta,
                             const uint64_t* digest_addrs, size_t ncalls, uint64_t* raw_rows_out_dev, uint64_t* memory_ops_out_dev,
                             uint32_t* logic_ops_out_dev, uint64_t* keccak_inputs_out_dev, uint64_t* keccak_timestamps_out_dev, char** err);

/* ------------------------------------------------------------------ the I/O syscalls' rows from their bytes
 * What the four data-moving helpers that generate_syscall calls behind its own row (witness/operation.rs:1660-1673) push, on the device,
 * from the bytes each moves: load_input (:1024-1067, SYSHINTREAD), commit (:1069-1099, SYSWRITE to FD_PUBLIC_VALUES), verify (:991-1022,
 * SYSVERIFY) and load_preimage (:908-989, SYSGETPID).  A row is a CpuColumnsView::default() with clock set and, for every used channel,
 * used = 1, is_read, the three address cells and the value (witness/util.rs:304-349); every other cell is 0.  The lists:
 *   kinds     ncalls uint32, one of the four constants below; host memory
 *   data_off  ncalls + 1 words: call k's bytes are data[data_off[k] .. data_off[k + 1]); host memory
 *   data      the calls' bytes, host or device memory (may be NULL when the calls hold no byte)
 *   meta      ncalls x 4 words {context, segment, address, timestamp}; timestamp = the first row's clock x 10 (NUM_CHANNELS), the clock
 *             after the SYSCALL row.  Context and segment come from here (the reference hard-codes 0 and Segment::Code: for its callers
 *             the rows are identical)
 * What a call's L bytes are, and the rows they make (a word's value is the big-endian reading of its four bytes unless said otherwise):
 *   HINT_READ  the input-stream vector, any L >= 0: W = ceil(L / 4) words, the last right-padded with 0.  max(1, ceil(W / 8)) rows (a call
 *              of 0 bytes still pushes one row, with no channel used); row j, channel i WRITES word 8 j + i to address + 4 (8 j + i)
 *   COMMIT     the W = L / 4 memory words the call reads (the reference reads whole words whatever `size` is); rows and addresses as for
 *              the hint read, the channels READ
 *   VERIFY     the 32 bytes of the claim digest: one row, channels 0-7 read at address + 4 i
 *   PREIMAGE   the 32 hash bytes, then the content of C = L - 32 bytes; address must be 0x31000000.  Row 0: channels 0-7 read the hash
 *              words at 0x30001000 + 4 i.  Then Q = 1 + ceil(C / 4) write words in ceil(Q / 8) rows, word q in row 1 + q / 8, channel
 *              q % 8, at address + 4 q: word 0 is C, word 1 + k content word k.  A last content word of n < 4 bytes is those bytes read
 *              little-endian, | 1 << 8 n, | 0x80 << 24 if C % 32 + 4 > 32, byte-swapped (:960-980)
 * Rows are canonical and row-major, calls in list order; the clock of a call's row j is timestamp / 10 + j; the channel mask of a row is
 * its used channels (always the low ones).  memory_ops counts the used channels: the operations themselves are pushed by the rows' RAW
 * steps, as for any RAW row -- this expansion writes no operation list of its own.
 *   zkm_io_calls_counts   the two totals (any out pointer may be NULL); pure: no context, no GPU
 *   zkm_io_calls_steps    pure.  The cpu_rows RAW records (reads[0] = raw_base + j, reads[1] = the row's channel mask, every other field 0)
 *                         into steps_out and the clock each belongs at into clocks_out, as zkm_keccak_calls_steps does.  THE statement of
 *                         masks and positions: the binding, the Rust recorder and the kernel's indexing follow it.  meta is host memory
 *                         here, and raw_base + cpu_rows must fit in 32 bits.
 *   zkm_io_calls_witness  the kernel: one launch for all calls, the work divided by ROW (one call may be half a segment, the next one
 *                         row): the host's walk uploads the calls' row offsets and a workgroup finds the call of each of its rows by a
 *                         search over them.  Every word of the block is written (zeros, clocks, channel cells): nothing is zeroed in
 *                         front.  meta may be host or device memory; raw_rows_out_dev is a plain device pointer (8-byte aligned), so it may
 *                         aim into the middle of a larger block, cpu_rows x ZKM_CPU_COLS words.  Returns once the rows are complete: one
 *                         host wait.  Profile scope io_calls/rows.
 * Refused, on the host before any device work and before a missing context is reported, the message naming the list (kinds, data_off,
 * meta, data, or the output) and the call's position: a NULL list or output with a nonzero count; kinds or data_off in device memory; an
 * unknown kind; offsets that decrease; a verify call that is not 32 bytes; a commit length that is not a multiple of 4; a preimage
 * shorter than 32 bytes or with another address; an address that is not 4-aligned; a last word whose address does not fit in 32 bits; a
 * context or segment of 2^32 or more; a timestamp that is not a multiple of 10; raw_base + cpu_rows that does not fit in 32 bits; a
 * misaligned output.  A refusal leaves the context usable.  A meta in DEVICE memory is not read by the host and so not held to these
 * rules (no store's address depends on it).
 * Out of scope: the SYSCALL row in front of a call stays whatever the caller logs today; commit and verify READ memory, so the caller
 * supplies the words; nothing is staged by THIS entry point (zkm_segments_calls_stage does, and the pool takes calls:
 * zkm_pool_prove_segments_calls), and nothing is fused into the segment builder. */
#define ZKM_IO_HINT_READ 0
#define ZKM_IO_COMMIT 1
#define ZKM_IO_VERIFY 2
#define ZKM_IO_PREIMAGE 3
int zkm_io_calls_counts(const uint32_t* kinds, const uint64_t* data_off, size_t ncalls, size_t* cpu_rows, size_t* memory_ops, char** err);
int zkm_io_calls_steps(const uint32_t* kinds, const uint64_t* data_off, const uint64_t* meta, size_t ncalls, size_t raw_base,
                       zkm_cpu_step* steps_out, uint64_t* clocks_out, char** err);
int zkm_io_calls_witness(zkm_ctx* ctx, const uint32_t* kinds, const uint8_t* data, const uint64_t* data_off, const uint64_t* meta,
                         size_t ncalls, uint64_t* raw_rows_out_dev, char** err);

/* ------------------------------------------------------------------ the instructions the step kinds refuse, as rows
 * decode() (witness/transition.rs:42-312) accepts thirteen encodings that no ZKM_STEP_* kind takes.  Their rows are expanded here, on the
 * device, as ready-made rows for RAW steps, and the arithmetic operations they push go into a device list for zkm_segment_ops -- the
 * route the calls above take; the step kinds, their refusals and their messages stay as they are.  A record is a zkm_cpu_step in host
 * memory: pc, next_pc, insn, flags bit 0 (kernel mode) and context as in the step log; kind one of the constants below; reads the values
 * read, in the generator's order; clocks[k] is the clock of record k's row.  Each kind takes exactly the (opcode, func) pair decode
 * matches for it; the other fields are free: they go into the row's bits and, where decode uses them, into the operands.
 *   MUL (0x1C, 0x02)  generate_binary_arithmetic_op (witness/operation.rs:286-318): channels 0 and 1 read rs and rt (reads[0], reads[1]),
 *                     channel 2 writes the product's low word to rd; pushes {IS_MUL, in0, in1}
 *   MFHI MTHI MFLO MTLO (0, 0x10 .. 0x13)  the same generator with decode's operands: MFHI reads register 33 and register 0 and writes
 *                     rd, MTHI reads rs and register 0 and writes register 33, MFLO reads 32 and 0 and writes rd, MTLO reads rs and 0 and
 *                     writes 32; the value written is reads[0]; reads[1], the value of register 0, must be 0; pushes {IS_M*, in0, 0}
 *   MULT MULTU DIV DIVU (0, 0x18 .. 0x1B)  generate_binary_arithmetic_hilo_op (:320-375): channels 0 and 1 read rs and rt, channel 2
 *                     writes lo to register 32, channel 3 hi to register 33 (DIV: quotient and remainder as Rust's / and %); pushes one
 *   LUI (0x0F)        generate_lui (:405-433): no read; channel 0 is a write of sext(imm) to register rs, channel 1 a write of 1 << 16 to
 *                     rt, channel 2 the write of imm << 16 to rt; pushes {IS_LUI, sext(imm), 1 << 16}
 *   SDC1 (0x3D)       generate_mstore_general with MemOp::SDC1 (:1804-1928): channels 0 and 1 read base and rt, channel 2 reads the word
 *                     at (base + sext(imm)) & ~3 in the record's context (reads[0 .. 2]), channel 3 stores 0 there; the three bit
 *                     decompositions, aux_filter and is_sdc1 are set, aux_rs0_mul_rs1 is 0; pushes nothing
 *   SYNC (0, 0x0F), PREF (0x33)  generate_nop: the op flag alone; no channel, no operation
 * A row is the whole CpuColumnsView: clock, context, pc, next_pc, the kernel flag, the 32 instruction bits, one op flag (binary_op,
 * binary_imm_op for LUI, m_op_store, nop), the channels, the kind's own cells, every other cell 0, all words canonical.  A write to
 * register 0 fills its channel with used = 0 and pushes nothing (witness/util.rs:198-204).  Results are computed on the device as
 * BinaryOperator::result does (arithmetic/mod.rs:48-133).  The arithmetic operations are {row filter, in0, in1} triples of uint32 as
 * zkm_arithmetic_trace takes them, in record order; a record that pushes none takes no slot.  The rows' memory operations are pushed by
 * their RAW steps, as for any RAW row (all thirteen generators push them in channel order).
 * What a record produces is one __host__ __device__ function (csrc/insn_rows.hip zkm_insn::expand) for the host walk and the kernel.
 *   zkm_insn_rows_counts    the used channels and the operations of the records (any out pointer may be NULL); pure: no context, no GPU
 *   zkm_insn_rows_steps     pure.  The RAW records (kind ZKM_STEP_RAW, reads[0] = raw_base + k, reads[1] = the row's mask of used channels,
 *                           every other field 0) into steps_out; the caller places record k at clocks[k] - first_clock of its step list.
 *                           THE statement of masks: MUL and the four moves 3 | (dest != 0) << 2; the hi/lo kinds and SDC1 0xF; LUI
 *                           (rs != 0) | (rt != 0) << 1 | (rt != 0) << 2; SYNC and PREF 0.  raw_base + ninsns must fit in 32 bits.
 *   zkm_insn_rows_witness   the kernel: one launch for all records; a workgroup builds a fixed number of rows in LDS, one lane a row, then
 *                           all its lanes stream the block out, adjacent lanes on adjacent words.  Every word of the ninsns x ZKM_CPU_COLS
 *                           block is written exactly once: nothing is zeroed in front.  raw_rows_out_dev is a plain device pointer (8-byte
 *                           aligned), so it may aim into the middle of a larger block; arithmetic_ops_out_dev (4-byte aligned) takes
 *                           arithmetic_ops x 3 uint32 and may be NULL when no record pushes an operation.  The host walk uploads each
 *                           workgroup's base in the arithmetic list.  Returns once both outputs are complete: one host wait.  Profile
 *                           scope insn_rows/rows.
 * Refused, on the host walk before any device work and before a missing context is reported, the message naming the function and
 * `record k`: an unknown kind; an encoding the kind does not take; DIV or DIVU with a zero divisor and DIV of 0x80000000 by 0xFFFFFFFF
 * (result() panics on all three); MFHI, MFLO, MTHI or MTLO whose reads[1] is not 0; a clock of 2^32 or more; raw_base + ninsns that does
 * not fit in 32 bits; a NULL list or output with a nonzero count; records or clocks in device memory; a misaligned output.  A refusal
 * leaves the context usable and its live memory as it was.
 * Out of scope: new step kinds; the records are not staged by THIS entry point (zkm_segments_calls_stage does, and the pool
 * takes them: zkm_pool_prove_segments_calls); nothing is fused into the segment builder;
 * keccak_general, Pc and GetContext / SetContext (decode never produces them); the exit kernel. */
#define ZKM_INSN_LUI 0
#define ZKM_INSN_MUL 1
#define ZKM_INSN_MULT 2
#define ZKM_INSN_MULTU 3
#define ZKM_INSN_DIV 4
#define ZKM_INSN_DIVU 5
#define ZKM_INSN_MFHI 6
#define ZKM_INSN_MTHI 7
#define ZKM_INSN_MFLO 8
#define ZKM_INSN_MTLO 9
#define ZKM_INSN_SDC1 10
#define ZKM_INSN_SYNC 11
#define ZKM_INSN_PREF 12
int zkm_insn_rows_counts(const zkm_cpu_step* insns, size_t ninsns, size_t* memory_ops, size_t* arithmetic_ops, char** err);
int zkm_insn_rows_steps(const zkm_cpu_step* insns, size_t ninsns, size_t raw_base, zkm_cpu_step* steps_out, char** err);
int zkm_insn_rows_witness(zkm_ctx* ctx, const zkm_cpu_step* insns, const uint64_t* clocks, size_t ninsns, uint64_t* raw_rows_out_dev,
                          uint32_t* arithmetic_ops_out_dev, char** err);

/* ------------------------------------------------------------------ K segments' calls expanded in one set of launches
 * The four expansions above, composed: which RAW index each generated row gets, where its record goes in the step list, one device
 * block per list with the segment's own items in front, and which groups of zkm_segment_ops the calls set -- for K segments at once,
 * in front of zkm_segments_tables_steps / zkm_prove_segments_ops_steps, whose inputs it produces.  A segment as the emulator records
 * it is one zkm_segment_calls:
 *   steps         the segment's own step list with a placeholder record (any record: it is overwritten) at the position of every row of
 *                 a call and of every `insns` record; raw_rows: the segment's own ready-made rows, HOST memory
 *   first_clock   the clock of steps.steps[0] (the bootstrap's row count, or 0)
 *   own           the segment's own operations, and the groups that are passed on untouched.  cpu_rows must be NULL; memory_ops,
 *                 logic_ops, arithmetic_ops, keccak_* (the segment's own permutations), poseidon_* and poseidon_sponge_* may be set;
 *                 sha_extend_*, sha_extend_sponge_*, sha_compress_*, sha_compress_sponge_* and keccak_sponge_* must be empty: the
 *                 calls own them
 *   extend_* compress_*   the SHA calls as zkm_sha_calls_witness takes them       } every list the host reads -- the metas, the offsets, the
 *   keccak_*              the SYSKECCAK calls as zkm_keccak_calls_witness does   } kinds, the records, the clocks -- is HOST memory here; the
 *   io_*                  the I/O calls as zkm_io_calls_witness does             } payloads (w16, hx, w, the input bytes, the data bytes,
 *   insns, insn_clocks    the records of zkm_insn_rows_witness and their clocks  } the digest addresses) are host or device memory
 * RAW indices continue steps.nraw in the order own, SHA, Keccak, I/O, instructions; every list holds the segment's own items in front and
 * the generated ones behind in that order.
 *   zkm_segment_calls_steps     pure (no context, no GPU): the host half, built from the four zkm_*_steps / zkm_*_counts above.  Writes the
 *                               patched list (steps.nsteps records: the segment's own with every call's RAW record at clock - first_clock)
 *                               into steps_out, and counts_out[ZKM_CALLS_COUNTS]: [0..3] the rows of the SHA, Keccak, I/O calls and the
 *                               instructions; [4] the total nraw (steps.nraw + those); the items GENERATED into the lists: [5] memory
 *                               operations (the SHA and Keccak sponges' reads), [6] logic operations, [7] arithmetic operations, [8]
 *                               ShaExtend rows, [9] Keccak permutations; [10] the memory operations the I/O and instruction rows' RAW
 *                               steps will push (no list item).  Either output may be NULL.
 *   zkm_segments_calls_expand   the calls of all nseg segments.  A group of up to 32 segments takes ONE scratch block (every list the
 *                               host holds, of every kind and segment, and the kernels' descriptors), at most ONE launch per kind
 *                               (none for a kind no segment of the group uses; profile scopes as the four entry points) and ONE host
 *                               wait; more segments are expanded in consecutive groups.  *out holds the results:
 *   zkm_expanded_calls_get      for segment `segment`: steps_out = the patched list (held by the handle) with raw_rows in device memory --
 *                               own rows, then the SHA calls', the Keccak calls', the I/O calls', the instructions' -- and ops_out = `own`
 *                               with memory_ops, logic_ops, keccak_* and sha_extend_* in device memory (arithmetic_ops too when the
 *                               segment has instruction records; otherwise it is passed on), sha_extend_sponge_*, sha_compress_*,
 *                               sha_compress_sponge_* and keccak_sponge_* pointing at the CALLER's call lists, which therefore stay
 *                               as they are until the handle is freed.  A segment with no calls at all passes through unchanged, its own
 *                               rows and lists uploaded.  Every word is what the four entry points write when composed by hand.
 *   zkm_expanded_calls_free     releases the handle and its device blocks (NULL is allowed)
 *   zkm_segments_tables_calls / zkm_prove_segments_ops_calls   the expansion, zkm_segments_tables_steps / zkm_prove_segments_ops_steps on
 *                               its outputs, the free.  Arguments as those take them with `calls` in place of steps and ops; images may be
 *                               NULL; sizing mode, waves, "check_ctls" and "verify" are the inner call's, and so are its three host waits:
 *                               the expansion in front adds one per 32 segments.
 * Refused by all of them, on the host before any device work, the message naming the function and the segment's position in the call and
 * then what the kind's entry point says ("zkm_segments_calls_expand: segment 1: zkm_io_calls_counts: kinds: call 2: ..."): every refusal of the four
 * entry points that concerns the lists (a NULL pointer with a nonzero count, a Keccak length that is not a positive multiple of 4, an
 * unknown I/O kind, an instruction record outside the thirteen, ...); a meta, offset, kind, record or clock list in device memory; a
 * call row whose clock lies outside the step list; two records on one clock; a group of `own` that the calls own; own.cpu_rows; raw_rows
 * in device memory; nseg = 0 or NULL calls.  A refusal leaves the context usable, its live memory as it was, and no handle behind.
 * Out of scope: nothing is fused into the builder (its kernels and its three host waits are untouched); the pool takes the same lists
 * (zkm_pool_prove_segments_calls); THESE
 * entry points place the records into the step list on the host (the builder walks it there): zkm_segments_calls_stage, below, does
 * both on the device, ahead of the call.
 * (The struct and the handle are tagged, not typedef'd: to the header-driven bindings a pointer to either is a plain address.) */
#define ZKM_CALLS_COUNTS 11
struct zkm_segment_calls {
    zkm_cpu_steps steps;
    uint64_t first_clock;
    zkm_segment_ops own;
    const uint32_t* extend_w16; const uint64_t* extend_meta; size_t nextend;                                /* zkm_sha_calls_witness */
    const uint32_t* compress_hx; const uint32_t* compress_w; const uint64_t* compress_meta; size_t ncompress;
    const uint8_t* keccak_inputs; const uint64_t* keccak_input_off; const uint64_t* keccak_meta; const uint64_t* keccak_digest_addrs;
    size_t nkeccak;                                                                                         /* zkm_keccak_calls_witness */
    const uint32_t* io_kinds; const uint8_t* io_data; const uint64_t* io_data_off; const uint64_t* io_meta; size_t nio;   /* zkm_io_calls_witness */
    const zkm_cpu_step* insns; const uint64_t* insn_clocks; size_t ninsns;                                  /* zkm_insn_rows_witness */
};
struct zkm_expanded_calls;
int zkm_segment_calls_steps(const struct zkm_segment_calls* calls, zkm_cpu_step* steps_out, size_t* counts_out, char** err);
int zkm_segments_calls_expand(zkm_ctx* ctx, size_t nseg, const struct zkm_segment_calls* calls, struct zkm_expanded_calls** out, char** err);
int zkm_expanded_calls_get(const struct zkm_expanded_calls* expanded, size_t segment, zkm_cpu_steps* steps_out, zkm_segment_ops* ops_out);
void zkm_expanded_calls_free(struct zkm_expanded_calls* expanded);
int zkm_segments_tables_calls(zkm_ctx* ctx, const zkm_stark_config* cfg, size_t nseg, const zkm_boot_image* images,
                              const struct zkm_segment_calls* calls, unsigned* log_n_out, zkm_staged** out, char** err);
int zkm_prove_segments_ops_calls(zkm_ctx* ctx, const zkm_stark_config* cfg, size_t nseg, const zkm_boot_image* images,
                                 const struct zkm_segment_calls* calls, const uint64_t* const* public_values, const size_t* npublic,
                                 uint64_t* const* proofs_out, size_t* proof_offsets_out, uint64_t* const* ctl_challenges_out, char** err);

/* Staged calls: the NEXT call's zkm_segment_calls behind the CURRENT proofs -- the form the emulator records, staged as steps, tables
 * and operations are.  zkm_segments_calls_expand builds one record and one clock per generated ROW on the calling thread, checks and
 * patches the step list there, and waits on the host once per 32 segments; the builder then walks the patched list on the host again.
 * zkm_segments_calls_stage reads the lists on the host per CALL only -- the counts, and every refusal of zkm_segments_calls_expand that
 * needs no row's clock, word for word under this function's name, before any device work and leaving no handle -- and queues the rest
 * on the context's two copy streams, behind what the compute stream has queued (as zkm_cpu_steps_stage orders them): the segment's own
 * step records, ready-made rows and lists, every payload and meta list of the calls, the images' addrs / values where they lie in host
 * memory, the four expansion launches, a placement kernel (a thread per generated row: the row's record -- the same statement
 * zkm_*_calls_steps write on the host -- stored at clock - first_clock of the device's step list), the walk of zkm_cpu_steps_stage
 * over the patched list, whose mask check therefore covers the generated rows too, and the download of both sets of verdicts into
 * pinned memory of the handle.  It RETURNS AT ONCE, with no host wait; more than 32 segments queue consecutive sets of launches in the
 * same call.  images may be NULL (no segment stands behind a bootstrap); otherwise nseg images, as the builder's `images`.
 * The two refusals that need a row's clock are found by the placement kernel: a row whose clock lies outside the step list (it touches
 * nothing), and two records on one clock; the row named is the one zkm_segments_calls_expand names.
 *   zkm_staged_calls_ready   1: uploads, expansions, placement, walk and downloads have ended -- every list of the caller may be reused;
 *                            0: in flight (wait = 0 only); -1: a runtime error.  NULL: 1.
 *   zkm_staged_calls_get     waits on the host for the handle's events the first time it is called (at most one host wait a handle),
 *                            and orders the compute stream behind them once.  steps_out: the patched list and all ready-made rows --
 *                            own, SHA, Keccak, I/O, instructions -- in device memory, staged steps to the builder (counts and bases
 *                            from the handle, nothing uploaded; pass it as it is handed out).  ops_out: as zkm_expanded_calls_get's,
 *                            with every list the builder accepts in device memory pointing into the handle's blocks -- the joined
 *                            lists, and the calls' groups (sha_extend_sponge_*, sha_compress_*, sha_compress_sponge_*,
 *                            keccak_sponge_inputs / _meta) at the copies the expansions read; keccak_sponge_off, which the builder
 *                            reads on the host, points at the handle's own copy.  A payload list the caller had in device memory is
 *                            referenced, not copied, and stays the caller's until the handle is freed, as do own.poseidon_* and
 *                            own.poseidon_sponge_* (passed on untouched; poseidon_sponge_off is read on the host), and
 *                            own.arithmetic_ops of a segment without instruction records.  image_out (may be NULL): the segment's
 *                            image with addrs / values in device memory (zeroed when the stage had no images).
 *                            A refused segment fails with "zkm_staged_calls_get: segment <s>: " and the placement's refusal in
 *                            zkm_segments_calls_expand's words ("instruction record row 7 (clock 96): two records on one clock"), else
 *                            the walk's in the host walk's ("step <i>: ..."); the other segments of the handle stay usable.
 *   zkm_staged_calls_free    waits for the events, then releases everything (NULL is allowed); after the calls that consumed the
 *                            handle have returned.
 * zkm_segments_tables_steps / zkm_prove_segments_ops_steps, with `images`, take these outputs ON THE SAME CONTEXT and keep their three
 * host waits; tables, blobs and challenges are word for word those of zkm_segments_tables_calls / zkm_prove_segments_ops_calls on the
 * same input.  They refuse the outputs of a handle of another context, and steps whose nsteps, raw_rows or nraw were changed on the way.
 * Refused by the stage, beside the lists' refusals: NULL `out`, NULL calls or nseg = 0, a segment of more than 2^28 steps, an image
 * whose addrs or values is NULL with a nonzero nwords, a NULL context (last).  A refusal leaves the context usable and its live memory as it was.
 * A handle is its context's, so of a caller's handles the pool takes none: its workers stage their own groups this way
 * (zkm_pool_prove_segments_calls, "pool_stage_ahead").
 * (The handle is passed as an address, as zkm_cpu_steps_stage's is.) */
int zkm_segments_calls_stage(zkm_ctx* ctx, size_t nseg, const struct zkm_segment_calls* calls, const zkm_boot_image* images, void** out,
                             char** err);
int zkm_staged_calls_ready(void* staged, int wait);
int zkm_staged_calls_get(void* staged, size_t segment, zkm_cpu_steps* steps_out, zkm_segment_ops* ops_out, zkm_boot_image* image_out,
                         char** err);
void zkm_staged_calls_free(void* staged);

/* ------------------------------------------------------------------ a memory image's hash pages, root and image id
 * What the emulator does at every segment split -- Memory::update_page_hash and Memory::compute_image_id (emulator/src/memory.rs:388-471,
 * with poseidon / hash_page / CONST_HASH_PAGES, :43-118, and alloc_hash_page, :378-386; called from split_segment, state.rs:1477-1530) --
 * as one device call: the producer of the hash words, pre_hash_root and pre_image_id that the bootstrap above checks.  Page q
 * (q = addr >> 12) is hashed into the eight words at 0x80000000 + (q << 5): a dirty page p into its L1 page 0x80000 + (p >> 7), that
 * into its L2 page 0x81000 + (p >> 14), that into the root page 0x81020.
 *   zkm_image_hash_plan   pure (no context): the ascending list of hash pages update_page_hash writes for these (ascending) dirty
 *                         pages -- the L1 pages, the L2 pages, then the root, which is always there (ndirty = 0 gives the root alone).
 *                         Returns the count and writes min(count, capacity) entries; hash_index_out may be NULL.
 *   zkm_image_hash        A plan page listed in `known` starts from the given words, every other as alloc_hash_page makes it (128
 *                         copies of the digest of the level below's fresh page; the zero page's digest at the bottom).  Every dirty
 *                         page is hashed into its L1 slot, every plan L1 page into its L2 slot, every plan L2 page into its root slot;
 *                         `registers` go to byte 0x400 of the root page; the root page's hash is page_hash_root_out; the image id is the
 *                         sponge over the root's eight words byte-swapped and pc.  The sponge is overwrite-mode over from_canonical_u32
 *                         of the little-endian words with pad10*1 (a 129th block for a page); a digest is four canonical words, word j
 *                         stored as page words 2j (low half) and 2j + 1.  hash_words_out: nplan x 1024 words in plan order, host or
 *                         device memory -- the pages as the emulator leaves them, the root page with the registers in it; passed as the
 *                         next call's `known` (device pointers), the hash pages stay on the device between splits.
 *                         Refused (nonzero; the message names the position and the index), on the host before any device work: a NULL
 *                         pointer with a nonzero count; indices not strictly ascending; a dirty index >= 0x80000; a known index that is
 *                         not in the plan; ndirty == 0 without the root among the known pages (the reference panics with "compute image
 *                         ID fail").  A refusal leaves the context usable and its live memory as it was.  One host wait, for the outputs.
 *   zkm_images_hash       nimg independent memories in ONE set of launches (the image is a grid dimension, the chains of a level run
 *                         side by side: K images cost about one image's latency).  hash_words_out[m] as above for image m; roots and
 *                         ids 32 bytes an image; every word is what zkm_image_hash gives for that image alone, and zkm_image_hash is
 *                         the nimg = 1 case of the same code.  A refusal names the image's position.
 * The lane form of the level launches: "image_hash_form" (zkm_ctx_set_tuning).  Profile scopes image_hash/init and image_hash/level. */
typedef struct zkm_image_pages {
    const uint32_t* dirty_index; size_t ndirty;  /* HOST memory: page indices (addr >> 12) below 0x80000, strictly ascending (wtrace[0]) */
    const uint32_t* dirty_words;                 /* ndirty x 1024 LE words, host or device memory */
    const uint32_t* known_index; size_t nknown;  /* HOST memory: hash pages that exist already, strictly ascending, each one in the plan */
    const uint32_t* known_words;                 /* nknown x 1024, host or device memory */
    uint32_t pc;                                 /* compute_image_id's pc */
    uint8_t registers[156];                      /* get_registers_bytes(), copied to the root page at 0x400 */
} zkm_image_pages;
size_t zkm_image_hash_plan(const uint32_t* dirty_index, size_t ndirty, uint32_t* hash_index_out, size_t capacity);
int zkm_image_hash(zkm_ctx* ctx, const zkm_image_pages* in, uint32_t* hash_words_out, uint8_t page_hash_root_out[32], uint8_t image_id_out[32],
                   char** err);
int zkm_images_hash(zkm_ctx* ctx, size_t nimg, const zkm_image_pages* in, uint32_t* const* hash_words_out, uint8_t* page_hash_roots_out,
                    uint8_t* image_ids_out, char** err);

/* ------------------------------------------------------------------ one process, many GPUs: a pool of contexts
 * The reference drives all segments of a program from ONE process (prover/examples/utils/src/utils.rs:57-68 prove_single_seg_common,
 * :105-133 prove_multi_seg_common: a loop of prove_with_traces calls); segments are independent proofs, so N GPUs take them
 * side by side with no data-path collective.  A pool owns `contexts_per_device` contexts on each of `devices[0 .. ndevices)` (a device
 * may be listed once only) and, per call, one worker thread per context: the nseg segments of a call are cut into consecutive groups of
 * at most `max_stack` segments (every worker the same number of groups, sizes as even as the count allows), the workers pull groups
 * from one queue, and a group is ONE lock-step call (zkm_prove_segments[_columns]) on the worker's context.  Every proof blob and
 * every challenge is word for word what zkm_prove_segment returns for that segment alone, whatever the device count.
 *   traces / columns / log_n / public_values / npublic / proofs_out / ctl_challenges_out   as zkm_prove_segments[_columns]
 *   max_stack   segments per lock-step call, 1 .. 32 (0 = 8; also bounded by the contexts' "max_stack" tuning)
 * The inputs must be readable from every device of the pool: HOST memory (pageable, zkm_host_alloc'ed or zkm_host_register'ed -- what a
 * Rust Vec is), or device memory when the pool has one device.  The first failing group stops the queue; its message names the worker,
 * the device and the positions of its segments in the call.  A failure leaves every output undefined.  A pool is single-owner like
 * a context: one call at a time.  zkm_pool_context hands out worker w's context (0 <= w < zkm_pool_workers) for zkm_ctx_set_tuning,
 * zkm_ctx_memory, zkm_profile_*; zkm_pool_set_tuning applies one key to all of them. */
typedef struct zkm_pool zkm_pool;
int zkm_pool_create(const int* devices, size_t ndevices, size_t contexts_per_device, zkm_pool** out, char** err);
void zkm_pool_destroy(zkm_pool* pool);
size_t zkm_pool_workers(const zkm_pool* pool);
zkm_ctx* zkm_pool_context(zkm_pool* pool, size_t worker);
int zkm_pool_device(const zkm_pool* pool, size_t worker);
int zkm_pool_set_tuning(zkm_pool* pool, const char* key, uint64_t value, char** err);
int zkm_pool_prove_segments(zkm_pool* pool, const zkm_stark_config* cfg, size_t nseg, size_t max_stack, const uint64_t* const* const* traces,
                            const unsigned* const* log_n, const uint64_t* const* public_values, const size_t* npublic,
                            uint64_t* const* proofs_out, uint64_t* const* ctl_challenges_out, char** err);
int zkm_pool_prove_segments_columns(zkm_pool* pool, const zkm_stark_config* cfg, size_t nseg, size_t max_stack,
                                    const uint64_t* const* const* const* columns, const unsigned* const* log_n,
                                    const uint64_t* const* public_values, const size_t* npublic, uint64_t* const* proofs_out,
                                    uint64_t* const* ctl_challenges_out, char** err);
/* The pool takes operations: the same groups, each ONE zkm_prove_segments_ops call on its worker's context (tables built and proven
 * there).  ops / proof_offsets_out as zkm_prove_segments_ops; the lists must be host memory unless the pool has one device.
 * proofs_out = NULL sizes (the groups spread over the workers as in a proving call).  zkm_pool_last_assignment works after it. */
int zkm_pool_prove_segments_ops(zkm_pool* pool, const zkm_stark_config* cfg, size_t nseg, size_t max_stack, const zkm_segment_ops* ops,
                                const uint64_t* const* public_values, const size_t* npublic, uint64_t* const* proofs_out,
                                size_t* proof_offsets_out, uint64_t* const* ctl_challenges_out, char** err);
/* The pool takes segments as the emulator records them: the same groups, each a list of zkm_segment_calls -- a step log, the SHA /
 * Keccak / I/O calls and the instruction records ("Calls", above), behind a boot image where `images` is not NULL (then nseg of them).
 * A zkm_segment_calls without calls is a plain step log: this is also how the pool takes steps.  Every blob, offset and challenge is
 * word for word what zkm_prove_segments_ops_calls gives on one context for the same list, whatever the worker count, max_stack or
 * "pool_stage_ahead" (zkm_ctx_set_tuning), which chooses how a worker serves its groups: staged one group ahead (default), or one
 * expanding call a group.  proofs_out = NULL sizes (proof_offsets_out as zkm_pool_prove_segments_ops; the groups are served in the
 * same way, so a refusal reads the same in both calls).  Every list must be host memory unless the pool has one device.
 * Refused on the host, in this order: a NULL pool, cfg or calls (or proofs_out without ctl_challenges_out, or neither proofs_out nor
 * proof_offsets_out), nseg = 0, max_stack beyond 32.  A failing group's message names the worker, the device and the group's
 * segments, then what zkm_prove_segments_ops_calls (one call a group; under this entry point's name) or zkm_segments_calls_stage /
 * zkm_staged_calls_get (staged ahead) say, with the segment's position in THIS call.  A failure frees every handle a worker holds --
 * the group staged ahead and never proven too, whose segments stay unassigned -- and leaves every worker context's live memory as it
 * was and the pool usable.  zkm_pool_last_assignment works after it.  Measured: profiles/pool_calls_time.json. */
int zkm_pool_prove_segments_calls(zkm_pool* pool, const zkm_stark_config* cfg, size_t nseg, size_t max_stack, const zkm_boot_image* images,
                                  const struct zkm_segment_calls* calls, const uint64_t* const* public_values, const size_t* npublic,
                                  uint64_t* const* proofs_out, size_t* proof_offsets_out, uint64_t* const* ctl_challenges_out, char** err);
/* The groups a pool call of nseg segments is cut into for `workers` workers (a pure function: no pool, no GPU): returns their number and
 * writes the first min(capacity, number) sizes, in segment order.  20 segments, 2 workers, max_stack 4 -> 4, 4, 3, 3, 3, 3. */
size_t zkm_pool_plan(size_t nseg, size_t workers, size_t max_stack, size_t* group_sizes_out, size_t capacity);
/* which worker proved segment s of the pool's LAST call, and in which group (diagnostics / tests): 0 on success */
int zkm_pool_last_assignment(const zkm_pool* pool, size_t segment, size_t* worker_out, size_t* group_out);

/* a10 alone (BASELINE config 4): PolynomialBatch::prove_openings (call site prover.rs:618-628) for the STARK FRI
 * instance (stark.rs:91-148: batches at zeta, g*zeta and 1 over the trace / auxiliary / quotient oracles) on three
 * existing commitments.  Transcript: compact, zeta <- challenger, openings observed (proof.rs:336-367), prove_openings.
 * The last nctl_zs auxiliary polynomials are the ones opened at 1.  Output: the usual proof blob. */
int zkm_prove_openings(zkm_ctx* ctx, const zkm_stark_config* cfg, const zkm_batch* trace_batch, const zkm_batch* aux_batch,
                       const zkm_batch* quot_batch, size_t nctl_zs, zkm_challenger* challenger, uint64_t* proof_out, char** err);

/* PolynomialBatch::prove_openings (plonky2 fri/oracle.rs) for an ARBITRARY FriInstanceInfo: `noracles` (<= 8) commitments of equal
 * degree, `nbatches` FriBatchInfo { point, polynomials: (oracle_index, polynomial_index)... } in instance order.  Transcript as in
 * plonky2: alpha <- challenger; per batch the alpha-reduced polynomial divided by (X - point), batches chained with
 * ReducingFactor::shift_poly; commit phase with one cap + beta per reduction arity; final polynomial; proof of work; query rounds.
 * (The openings themselves are the caller's: observe them before the call, as StarkOpeningSet / OpeningSet do.)  With the three
 * STARK oracles and the three batches of stark.rs:91-148 the output equals the FRI part of zkm_prove_openings' blob.
 * cfg->rate_bits may be 2 or 3 here and in zkm_fri_verify (3: plonky2's standard_recursion_config; the oracles are committed at the
 * same rate); the STARK entry points take 2 only.
 * The call is zkm_fri_prove_stack (below) at ONE claim -- one body, one combination launch for all batches -- on single commitments:
 * it refuses a stack ("zkm_fri_prove: stacked batches are internal"), takes the claim's points from the batches, and every refusal
 * leaves the challenger, the context and its live memory as they were.
 * FRI proof blob: [0] magic "ZKMFRIPF" [1] degree_bits [2] noracles [3] cap_height [4] L fri layers [5] F final_poly_len
 *   [6] num_queries [7] rate_bits [8] arity_bits [9..15] 0 [16..23] columns of each oracle
 *   commit_phase_merkle_caps[L][C*4]  final_poly[2F]  pow_witness[1]
 *   query_round_proofs[num_queries]: per oracle evals[cols] + siblings[(lde_bits - cap_height)*4]; per layer evals[2*2^arity_bits] +
 *   siblings[(lde_bits - arity_bits*(i+1) - cap_height)*4] */
#define ZKM_FRI_PROOF_MAGIC 0x46504952464d4b5aULL
typedef struct { uint32_t oracle, poly; } zkm_fri_poly;
typedef struct { uint64_t point[2]; const zkm_fri_poly* polys; size_t npolys; } zkm_fri_batch;
size_t zkm_fri_proof_words(const zkm_stark_config* cfg, unsigned log_n, const size_t* oracle_cols, size_t noracles);
int zkm_fri_prove(zkm_ctx* ctx, const zkm_stark_config* cfg, const zkm_batch* const* oracles, size_t noracles, const zkm_fri_batch* batches,
                  size_t nbatches, zkm_challenger* challenger, uint64_t* proof_out, char** err);
/* K opening proofs of ONE instance in lock-step: every oracle is a stack of the same size K (zkm_batch_commit_values_stack /
 * _coeffs_stack; K = zkm_batch_stack_size), the batches' polynomial lists are shared by the K claims, and
 *   points          K x nbatches x 2 words: claim k's point of batch b (the `point` fields inside `batches` are ignored)
 *   challengers[k]  in/out as zkm_fri_prove's        proofs_out[k]   zkm_fri_proof_words words, host
 * Claim k is zkm_fri_prove on member k of every oracle -- the two entry points are one body, zkm_fri_prove its case K = 1 -- so every
 * blob and every challenger state equals that call's on single commitments of the same data, word for word, and zkm_fri_verify takes
 * the K blobs as K claims.  The K proofs share every launch --
 * one combination launch for all batches and claims, then the division, the commit phase, the proof of work and the query gather of
 * the lock-step STARK proofs -- and every transcript round trip: the call waits for the device as often as ONE zkm_fri_prove does.
 * Refused on the host before any device work, leaving every challenger, the context and its live memory as they were: a NULL
 * argument; more than 8 oracles or batches; oracles whose stack sizes, degree, rate, cap height or coefficient layout differ (or
 * differ from cfg); a stack of more than 32; an empty batch; a polynomial index out of range; a NULL challenger or blob, or a point
 * word >= p, of a claim ("zkm_fri_prove_stack: claim 2: non-canonical opening point").  A call that fails later leaves the challengers
 * untouched too.  Out of scope: claims of different shapes in one call (group them, as segments are grouped by height); the pool.
 * Measured: profiles/fri_stack_time.json; the single call before and after it became this body: profiles/fri_single_path_time.json. */
int zkm_fri_prove_stack(zkm_ctx* ctx, const zkm_stark_config* cfg, const zkm_batch* const* oracles, size_t noracles, const zkm_fri_batch* batches,
                        size_t nbatches, const uint64_t* points, zkm_challenger* const* challengers, uint64_t* const* proofs_out, char** err);

/* ------------------------------------------------------------------ stage entry points (parity / reuse)
 * a6: compute_quotient_polys (prover.rs:645-789): nalphas polys of 2n coefficients, natural order;
 * out host or device. */
/* ------------------------------------------------------------------ N3: trace ingest
 * A segment's traces as one file / memory image, the hand-off from the CPU-side witness generator (generate_traces,
 * witness/traces.rs:230-320 returns [Vec<PolynomialValues<F>>; 12]; each table is written column-major as util.rs:37-46 lays it
 * out).  All integers little-endian uint64 unless noted:
 *   [0] magic "ZKMTRACE"  [1] version 1  [2] ntables  [3] npublic  [4] nctls  [5] nsides  [6..7] 0
 *   public values[npublic]
 *   per table (8 words): table_id, ncols, log_n, data offset (words from file start), ncolumns, nterms, ncolsets, nfilter_idx
 *   per table, its column-set description: columns[ncolumns] (zkm_column, 3 words each), term_col[nterms] (uint32, padded to 8 B),
 *       term_coeff[nterms], colsets[ncolsets] (zkm_colset, 4 words each), filter_idx[nfilter_idx] (uint32, padded to 8 B)
 *   cross-table lookups[nctls] (zkm_cross_table_lookup, 2 words each), sides[nsides] (zkm_ctl_side, 1 word each)
 *   trace data: per table ncols x 2^log_n canonical field elements
 * zkm_segment_image_words sizes an image; zkm_segment_image_write fills one from the in-memory description (traces must be host
 * pointers); zkm_prove_segment_image proves straight from an image (e.g. an mmap of the file): the traces are uploaded table by
 * table, never copied on the host. */
size_t zkm_segment_image_words(const zkm_table_input* tables, size_t ntables, const zkm_cross_table_lookup* ctls, const zkm_ctl_side* sides,
                               size_t nctls, size_t npublic);
int zkm_segment_image_write(const zkm_table_input* tables, size_t ntables, const zkm_cross_table_lookup* ctls, const zkm_ctl_side* sides,
                            size_t nctls, const uint64_t* public_values, size_t npublic, uint64_t* image_out, char** err);
/* proofs_out / ctl_challenges_out as zkm_prove_with_traces; *proof_words_out receives the total; pass proofs_out = NULL to query
 * the size first (returns 0 and only fills *proof_words_out and proof_offsets_out[ntables + 1] if non-NULL). */
int zkm_prove_segment_image(zkm_ctx* ctx, const zkm_stark_config* cfg, const uint64_t* image, size_t image_words, uint64_t* proofs_out,
                            size_t* proof_words_out, size_t* proof_offsets_out, uint64_t* ctl_challenges_out, char** err);

int zkm_quotient(zkm_ctx* ctx, int table_id, const zkm_batch* trace, const zkm_batch* aux, const uint32_t* num_helpers,
                 size_t nctl_zs, const uint64_t* alphas, size_t nalphas, uint64_t* out_coeffs, char** err);
/* check_constraints (prover.rs:793-910; the reference calls it under debug assertions, :529-541): evaluate the table's whole vanishing
 * polynomial -- table constraints, the table's lookups, the cross-table-lookup checks, in eval_vanishing_poly's order
 * (vanishing_poly.rs:17-46) -- on every row of the TRACE DOMAIN (rate_bits = 0: row i with next row i + 1 mod n, the Lagrange selectors
 * are the indicators of the first / last row) with the given constraint challenges, and report whether every accumulator vanishes.
 *   trace   ncols x 2^log_n trace values          aux   naux x 2^log_n auxiliary values: the table's lookup helper columns (zkm_num_lookup_columns,
 *           as zkm_lookup_helper_columns makes them per challenge), then the CTL helper columns and Zs (zkm_ctl_data) -- prover.rs:497-508 order
 *   table / zs / colset_ids / nzs, lookup_challenges   as zkm_prove_single_table_ctl
 * Returns 0 and *first_failing_row = ~0 when all constraints hold; nonzero with the reference's message "Constraint failed in <Stark>"
 * and the first failing row otherwise.  A debugging aid: not on the proving path. */
int zkm_check_constraints(zkm_ctx* ctx, int table_id, const zkm_stark_config* cfg, const uint64_t* trace, size_t ncols, unsigned log_n,
                          const uint64_t* aux, size_t naux, const zkm_ctl_table* table, const zkm_ctl_z* zs, const uint32_t* colset_ids, size_t nzs,
                          const uint64_t* lookup_challenges, const uint64_t* alphas, size_t nalphas, uint64_t* first_failing_row, char** err);
/* The table's OWN constraints on every row of the trace domain, from the trace alone -- no challenges, no auxiliary columns -- naming the
 * first one that fails: what zkm_check_constraints answers with one row, answered with the row, the constraint and its value.  The
 * constraints are those of the table's eval_packed_generic in emission order (the order of the alpha powers, constraint_consumer.rs:57-62):
 * row r is paired with row (r + 1) mod n, transition constraints are switched off on the last row, first-row and last-row constraints
 * are switched on only on their row.  NOT covered, because they are not table constraints: the range-check lookups of Memory and
 * Arithmetic (Stark::lookups(); zkm_check_constraints evaluates them with their helper columns) and the cross-table lookups
 * (zkm_check_ctls); zkm_lookup_check below checks those lookups from the trace alone.
 *   trace     ncols x 2^log_n canonical words, column-major, host or device (a host table is copied up for the call); ncols must be
 *             zkm_table_width(table_id), log_n at most 30
 *   finding   ZKM_WITNESS_FINDING_WORDS words (host): the row (all ones when every constraint holds), the index of the first nonzero
 *             constraint on that row, its canonical value, the number of rows with at least one nonzero constraint, the number of
 *             constraints a row emits
 * Returns 0 when every constraint holds on every row.  Otherwise nonzero, with the finding filled and *err =
 *   Constraint failed in <Name>Stark: row r, constraint i of N = 0x.. (m of n rows fail)        (the prefix: prover.rs:903-908)
 * WHICH finding is reported is fixed: the lowest failing row, and within it the lowest constraint index.  A refusal -- a null argument, an
 * unknown table id, ncols that is not the table's width, log_n out of range -- names its argument and is made on the host before any
 * device work.
 * zkm_segment_witness_check: the same for the twelve tables of a segment, traces[t] / log_n[t] of Table::all()[t] as
 * zkm_segment_check_ctls takes them (the twelve pointers of zkm_staged_segment_ptrs, for one), in ONE set of launches with one download
 * and one host wait whatever the tables (zkm_ctx_host_waits).  findings = 12 x ZKM_WITNESS_FINDING_WORDS words, every table's own
 * result; *err names the lowest failing table in Table::all() order.
 * Both run on the context's stream, behind what is queued there.  On the proving path only under "check_witness" (zkm_segments_check). */
#define ZKM_WITNESS_FINDING_WORDS 5
int zkm_witness_check(zkm_ctx* ctx, int table_id, const uint64_t* trace, size_t ncols, unsigned log_n, uint64_t* finding, char** err);
int zkm_segment_witness_check(zkm_ctx* ctx, const uint64_t* const* traces, const unsigned* log_n, uint64_t* findings, char** err);
/* The table's own range-check LOOKUPS (Stark::lookups(): Memory looks RANGE_CHECK up in COUNTER with FREQUENCIES, memory_stark.rs:476-483;
 * Arithmetic its 18 shared columns in RANGE_COUNTER with RC_FREQUENCIES, arithmetic_stark.rs:269-276) from the trace alone -- no
 * challenges, no helper columns, no Z -- naming the value that fails.  For a lookup with looking columns cols[], table_col and freq_col,
 * and a value v (words are read as field elements: a word >= p counts as its residue):
 *   looking(v)   = the number of cells (c in cols, row r) with trace[c][r] == v                            (an integer)
 *   frequency(v) = the sum over the rows r with trace[table_col][r] == v of trace[freq_col][r]             (mod p)
 * The lookup holds iff looking(v) == frequency(v) (mod p) for every v: exactly what the logUp argument enforces for every challenge
 * (lookup.rs:106-121, 183-194).  The table column need not be 0 .. n - 1: rows that share a value add their frequencies; frequencies are
 * field elements (p - 1 and looking + 1 on two rows of one value balance; p - 1 on a value nobody looks up does not).
 *   trace, ncols, log_n   as zkm_witness_check; also refused: a lookup of more than 2^30 records, rows x (looking columns + 1)
 *   finding   ZKM_LOOKUP_FINDING_WORDS words (host):
 *             0     index of the failing lookup among the table's lookups; all ones when every lookup holds, and for a table without lookups
 *             1     the value: the smallest unbalanced canonical value of that lookup (the lowest failing lookup)
 *             2     looking(value)                        3     frequency(value), canonical
 *             4     the number of rows whose table column holds the value
 *             5, 6  trace column and row of the first looking cell that holds it, in (the lookup's column order, then row) order; all ones
 *                   in both when there is none
 *             7     the lowest row whose table column holds it; all ones when there is none
 *             8     the number of unbalanced values of that lookup
 *             (words 1 .. 8 are 0 when every lookup holds)
 * Returns 0 when every lookup holds.  Otherwise nonzero, with the finding filled and *err =
 *   Lookup failed in <Name>Stark: lookup l: value 0x.. is looked up a times (first: column c, row r) and has frequency 0x.. in k table
 *   rows (first: row t); m values fail                                   ("first: none" for a location that does not exist)
 * Refusals are made on the host before any device work and write nothing to `finding`.  A table without lookups costs no launch and no
 * host wait.
 * zkm_segment_lookup_check: the same for the twelve tables of a segment, as zkm_segment_witness_check takes them: the tables with lookups
 * share ONE set of launches, one download and one host wait (zkm_ctx_host_waits).  findings = 12 x ZKM_LOOKUP_FINDING_WORDS words in
 * Table::all() order, every table's own result; *err names the lowest failing table in that order.
 * Both run on the context's stream, behind what is queued there; a finding or a failure leaves the context usable.  On the proving path
 * only under "check_witness" (zkm_segments_check).  With zkm_witness_check and zkm_check_ctls this covers what eval_vanishing_poly and verify_cross_table_lookups ask
 * of a witness. */
#define ZKM_LOOKUP_FINDING_WORDS 9
int zkm_lookup_check(zkm_ctx* ctx, int table_id, const uint64_t* trace, size_t ncols, unsigned log_n, uint64_t* finding, char** err);
int zkm_segment_lookup_check(zkm_ctx* ctx, const uint64_t* const* traces, const unsigned* log_n, uint64_t* findings, char** err);
/* check_ctls (cross_table_lookup.rs:1486-1581 testutils::check_ctls; prove_with_traces calls it under the `test` feature, prover.rs:171-176):
 * for each CrossTableLookup, the multiset of the rows of the looking tables whose filter is 1 (check_ctl :1505-1536, process_table
 * :1538-1563) must equal that of the looked table -- on the device, nothing downloaded.  tables / ctls / sides / nctls as
 * zkm_prove_with_traces takes them (`trace` or `columns`, host or device pointers; host tables are copied up for the call).
 * Tuples are compared as canonical field elements; Columns with next-row terms follow eval_table (:266-285: on the last row the next-row
 * part is zero); a filter value other than 0 or 1 is the reference's "Non-binary filter?" (:1560).
 * Returns 0 when every lookup holds.  Otherwise nonzero, with `report` filled (it may be NULL) and *err =
 *   "CTL #i: Row [..] is present a times in the looking tables, but b times in the looked table. Looking locations (Table, Row index):
 *    [(Cpu, 5), ..]. Looked locations (Table, Row index): []."   (check_locations :1565-1581), or
 *   "CTL #i: Non-binary filter? (side s, table T, row r: the filter is v)".
 * WHICH finding is reported is fixed: the lowest failing lookup; within it a non-binary filter wins over a multiset difference, and the
 * row named is the smallest in (side, row) order -- side = position among the lookup's looking sides, the looked side counting last;
 * among unbalanced tuples the one whose first occurrence comes first in (side, row) order; locations are listed in that order.
 *   kind          0 consistent; 1 non-binary filter; 2 multisets differ; 3 the check could not be made (bad arguments, column sets of
 *                 unequal width on the two sides of a lookup, a runtime failure): the message says why
 *   ctl           the reported lookup (kind 1, 2)
 *   attempts      rows are matched by sorting 128-bit keys of their tuples; every match is confirmed word for word, and keys of different
 *                 tuples that collide make the call sort again with other keys: the number of sorts (1 in practice; kind 3 after 4)
 *   host_waits    times the call waited for the device: the same whatever the number of lookups and sides
 *   side, table, row, filter_value   kind 1: the row (table = index into `tables`) and its filter's value
 *   width, nwords, tuple             kind 2: the tuple's columns, and the first nwords = min(width, 64) canonical words
 *   looking_count, looked_count      kind 2: its occurrences on either side
 *   looking, looked                  kind 2: the first n*_locations = min(count, 8) locations of either side
 * zkm_segment_check_ctls: the same for the AllStark that ships with the library, traces[t] / log_n[t] of Table::all()[t] as
 * zkm_prove_segment takes them -- e.g. the twelve device pointers of zkm_staged_segment_ptrs for a block zkm_segment_tables built.
 * Both run on the context's stream, behind what is queued there.  A debugging aid: on the proving path only under "check_ctls". */
/* (Layout lock: tests/test_abi.py compares these two structs, like every struct of this header, as the C compiler lays them out with
 * the ctypes and Rust mirrors.) */
#define ZKM_CTL_REPORT_WORDS 64
#define ZKM_CTL_REPORT_LOCATIONS 8
typedef struct zkm_ctl_location { uint32_t side, table; uint64_t row; } zkm_ctl_location;
typedef struct zkm_ctl_report {
    uint32_t kind, ctl, attempts, host_waits;
    uint32_t side, table;
    uint64_t row, filter_value;
    uint32_t width, nwords;
    uint64_t tuple[ZKM_CTL_REPORT_WORDS];
    uint64_t looking_count, looked_count;
    uint32_t nlooking_locations, nlooked_locations;
    zkm_ctl_location looking[ZKM_CTL_REPORT_LOCATIONS], looked[ZKM_CTL_REPORT_LOCATIONS];
} zkm_ctl_report;
int zkm_check_ctls(zkm_ctx* ctx, const zkm_table_input* tables, size_t ntables, const zkm_cross_table_lookup* ctls, const zkm_ctl_side* sides,
                   size_t nctls, zkm_ctl_report* report, char** err);
int zkm_segment_check_ctls(zkm_ctx* ctx, const uint64_t* const* traces, const unsigned* log_n, zkm_ctl_report* report, char** err);
/* The three checks -- zkm_segment_witness_check, zkm_segment_lookup_check and zkm_segment_check_ctls -- on nseg segments in ONE
 * call: everything eval_vanishing_poly and verify_cross_table_lookups ask of a witness, in ONE set of launches for all segments (the
 * tables of a kind share a launch, the lookups' jobs share theirs 32 at a time) and TWO host waits whatever nseg when every segment is
 * consistent: the cross-table record counts, then one download of the cross-table verdicts with the witness and lookup findings.
 * A key collision adds one wait per extra attempt, failing cross-table lookups add one for all their reports, failing constraints or
 * range-check lookups add none (zkm_ctx_host_waits).
 *   traces[s][t], log_n[s][t]   table t of segment s in Table::all() order, column-major, host or device memory (the two may be mixed:
 *                      host tables are copied up for the call) -- e.g. the twelve pointers of zkm_staged_segment_ptrs for each segment
 *   verdicts           nseg x ZKM_SEGMENT_VERDICT_WORDS words, or NULL: [2 s] the kind of segment s's FIRST finding in the order of
 *                      eval_vanishing_poly (vanishing_poly.rs:17-46) -- 0 consistent; 1 a table constraint, [2 s + 1] the position of the
 *                      lowest failing table in Table::all(); 2 a range-check lookup, [2 s + 1] likewise; 3 a cross-table lookup,
 *                      [2 s + 1] the lookup's index
 *   witness_findings   nseg x 12 x ZKM_WITNESS_FINDING_WORDS words, or NULL: what zkm_segment_witness_check writes for each segment alone
 *   lookup_findings    nseg x 12 x ZKM_LOOKUP_FINDING_WORDS words, or NULL: what zkm_segment_lookup_check writes for each segment alone
 *   ctl_reports        nseg reports, or NULL: what zkm_segment_check_ctls writes for each segment alone, except `attempts` and
 *                      `host_waits`, which are the CALL's in every report
 * All three checks always run to the end on every segment, and the outputs are filled whatever they find.  Returns 0 when every segment
 * is consistent; otherwise nonzero with *err = "zkm_segments_check: segment <s>: <message>": s the lowest segment with a finding, the
 * message the one the owning per-segment check gives for that segment's first finding ("Constraint failed in <Name>Stark: ..",
 * "Lookup failed in <Name>Stark: ..", "CTL #j: ..").  Refusals -- nseg = 0, a NULL traces, log_n, traces[s], log_n[s] or table, a log_n
 * above 30, a lookup of more than 2^30 records -- are made on the host before any device work and before the context is needed, and
 * name the function, the segment and the table ("zkm_segments_check: segment 1: Logic: trace: null argument"); they leave the context
 * usable.  Everything runs on the context's stream, and all scratch is back in the context's cache when the call returns.  Segments
 * whose scratch would not fit in device memory together are checked in consecutive sub-groups, each with its own waits.
 * zkm_segment_check: the call for one segment (messages name zkm_segment_check).  In front of the prove calls under "check_witness". */
#define ZKM_SEGMENT_VERDICT_WORDS 2
int zkm_segments_check(zkm_ctx* ctx, size_t nseg, const uint64_t* const* const* traces, const unsigned* const* log_n, uint64_t* verdicts,
                       uint64_t* witness_findings, uint64_t* lookup_findings, zkm_ctl_report* ctl_reports, char** err);
int zkm_segment_check(zkm_ctx* ctx, const uint64_t* const* traces, const unsigned* log_n, uint64_t* verdict, uint64_t* witness_findings,
                      uint64_t* lookup_findings, zkm_ctl_report* ctl_report, char** err);
/* ------------------------------------------------------------------ verify_proof on the device
 * verify_proof (verifier.rs:27-176) with verify_stark_proof_with_challenges (:178-292) per table and verify_cross_table_lookups, for the
 * proof blobs this library writes, from the blobs alone -- what prove_root / prove_root_with_assumption run on every segment proof
 * before it enters the recursion (fixed_recursive_verifier.rs:777, 853).  The transcript is replayed on the host (every word of it is
 * in the blob); the constraints at zeta, the Merkle paths and the FRI arithmetic of all tables of all segments run in one set of
 * launches, and one download brings the verdicts back.  A rejected proof is a normal result: nothing is asserted on the device.
 *   code        ZKM_VERIFY_*: the check that failed, in the reference's order of checks
 *                 OK; SHAPE (magic, header against cfg and the table -- validate_proof_shape :294-342 -- the FRI proof's shape,
 *                 proof_words too short, a field word >= p: found on the host, such a blob never reaches a kernel); TRANSCRIPT_STATE (the
 *                 recorded init_challenger_state is not where the transcript stands); CTL_CHALLENGES (the claimed challenges are not the
 *                 transcript's); QUOTIENT ("Mismatch between evaluation and opening of quotient polynomial" :248-264); POW; INITIAL_MERKLE;
 *                 FRI_EVAL; FRI_MERKLE; FINAL_POLY; CTL_SUM (verify_cross_table_lookups); FAILED (the check could not be made: bad
 *                 arguments, a runtime failure)
 *   table       index into `tables` / Table::all()        challenge   the constraint challenge (QUOTIENT) or CTL challenge (CTL_SUM)
 *   query, tree (initial oracle 0 trace, 1 auxiliary, 2 quotient), layer      where in the query phase
 *   ctl         the lookup (CTL_SUM)                       host_waits  times the call waited for the device (counted where the context waits):
 *                                                          1 whatever the segments; 0 for a segment refused on the host
 * WHICH finding is reported is fixed: CTL_CHALLENGES first; then the lowest table, and within it TRANSCRIPT_STATE, QUOTIENT (lowest
 * challenge), POW, then the lowest query and inside it trace tree, auxiliary tree, quotient tree, per layer evaluation before Merkle
 * path, the final polynomial; CTL_SUM (lowest lookup, lowest challenge) only when every table passes.  A blob with a SHAPE finding in
 * any table is reported as SHAPE at that table and nothing of its segment is launched.
 * (Layout lock: tests/test_abi.py compares the struct, like every struct of this header, with the ctypes and Rust mirrors.) */
#define ZKM_VERIFY_OK 0
#define ZKM_VERIFY_SHAPE 1
#define ZKM_VERIFY_TRANSCRIPT_STATE 2
#define ZKM_VERIFY_CTL_CHALLENGES 3
#define ZKM_VERIFY_QUOTIENT 4
#define ZKM_VERIFY_POW 5
#define ZKM_VERIFY_INITIAL_MERKLE 6
#define ZKM_VERIFY_FRI_EVAL 7
#define ZKM_VERIFY_FRI_MERKLE 8
#define ZKM_VERIFY_FINAL_POLY 9
#define ZKM_VERIFY_CTL_SUM 10
#define ZKM_VERIFY_FAILED 11
typedef struct zkm_verify_report {
    uint32_t code, table, challenge, query, tree, layer, ctl, host_waits;
} zkm_verify_report;
/* The general form, the mirror of zkm_prove_with_traces: tables / ctls / sides / nctls / public values as that call takes them (`trace` and
 * `columns` of a table are ignored; its log_n must be the blob's), proofs = the per-table blobs concatenated as it writes them,
 * proof_words their total, ctl_challenges = the claimed challenges (2 * num_challenges words) or NULL.  Returns 0 when the proof is
 * accepted; nonzero otherwise with *err naming table and check; `report` (may be NULL) is filled either way. */
int zkm_verify_proofs(zkm_ctx* ctx, const zkm_stark_config* cfg, const zkm_table_input* tables, size_t ntables,
                      const zkm_cross_table_lookup* ctls, const zkm_ctl_side* sides, size_t nctls, const uint64_t* public_values,
                      size_t npublic, const uint64_t* proofs, size_t proof_words, const uint64_t* ctl_challenges, zkm_verify_report* report,
                      char** err);
/* verify_proof for nseg segments proven with the AllStark that ships with the library (zkm_all_stark_ctls): proofs[s] = the twelve
 * blobs of segment s in Table::all() order as zkm_prove_segment* writes them, in HOST memory (the transcript is replayed there; a
 * device pointer is FAILED), proof_words[s] their total.  The heights are read from the blobs (recover_degree_bits, proof.rs:205-212), so segments of different heights share a call.  public_values / npublic /
 * ctl_challenges may be NULL, and so may each ctl_challenges[s]; reports = nseg entries (may be NULL).  Returns 0 when every proof is
 * accepted; nonzero otherwise, *err naming the first rejected segment, its table (the reference's name) and the check. */
int zkm_verify_segments(zkm_ctx* ctx, const zkm_stark_config* cfg, size_t nseg, const uint64_t* const* proofs, const size_t* proof_words,
                        const uint64_t* const* public_values, const size_t* npublic, const uint64_t* const* ctl_challenges,
                        zkm_verify_report* reports, char** err);
/* The mirror of zkm_prove_single_table (the benchmark's fake CtlData shape): verify_stark_proof_with_challenges (verifier.rs:178-292)
 * on one blob, `challenger` in/out like the prove call (left untouched unless the proof is accepted).  naux counts the CTL columns. */
int zkm_verify_single_table(zkm_ctx* ctx, int table_id, const zkm_stark_config* cfg, const uint64_t* proof, size_t proof_words, size_t ncols,
                            size_t naux, const uint32_t* num_helpers, size_t nctl_zs, zkm_challenger* challenger, zkm_verify_report* report,
                            char** err);
/* The mirror of zkm_fri_prove: plonky2's verify_fri_proof (fri/verifier.rs; call sites verifier.rs:276-289, and in circuit form
 * recursive_verifier.rs:426) for ANY FriInstanceInfo, on nproofs FRI proof blobs (magic "ZKMFRIPF") in one set of launches behind one
 * upload and before one download: one host wait whatever nproofs.  Claims of different heights and instances share a call.  Claim i:
 *   proofs[i], proof_words[i]   the blob zkm_fri_prove wrote, HOST memory            log_n[i]   degree bits of the instance
 *   oracle_cols[i], noracles[i] columns of each initial oracle, 1..8 oracles
 *   oracle_caps[i]              noracles[i] pointers: each oracle's cap, 2^cap_height digests (zkm_batch_cap), host
 *   batches[i], nbatches[i]     the instance exactly as zkm_fri_prove takes it, 1..8 batches
 *   opened[i]                   nbatches[i] pointers: opened[i][b] = batches[i][b].npolys F2 values (2 words each), the claimed p(point) in
 *                               the batch's polynomial order, e.g. from zkm_eval_openings; host
 *   challengers[i]              in/out: the state zkm_fri_prove was entered with; advanced to the state zkm_fri_prove leaves only when
 *                               claim i is accepted, untouched otherwise (as in zkm_verify_single_table)
 * (The claims travel as parallel arrays, as zkm_verify_segments' segments do.)
 * Transcript: the one zkm_fri_prove writes, replayed on the host from the blob alone: alpha is drawn; per layer the cap is observed and
 * beta drawn; the final polynomial is observed; the proof-of-work witness is applied; the query indices are drawn.
 * reports (nproofs entries, may be NULL): code is one of OK, SHAPE, POW, INITIAL_MERKLE, FRI_EVAL, FRI_MERKLE, FINAL_POLY, FAILED;
 * table = 0, tree = the oracle's index, query / layer / host_waits as above (host_waits 1 for a claim that was launched, 0 for one
 * refused on the host).  WHICH finding is reported follows plonky2's order: POW; then the lowest query, and inside it the oracles'
 * Merkle proofs in ascending order, per layer the evaluation check before the Merkle proof, then the final polynomial.
 * Returns 0 iff every claim is accepted; otherwise *err names the first rejected claim
 * ("zkm_fri_verify: proof 3: query 5: Invalid Merkle proof. (initial oracle 2) [INITIAL_MERKLE]").
 * SHAPE (found on the host: such a claim reaches no kernel): wrong magic; header words [1..8] and [16..23] that are not what cfg, log_n,
 * oracle_cols and noracles give; proof_words below the blob's size; a word of the blob, an opened value, a cap word or a point >= p.
 * FAILED (the call could not be made, every report says so): a NULL pointer or nproofs == 0; a polynomial index out of range, an empty
 * batch, more than 8 oracles or batches; a base-field point on the LDE coset ((z / g)^(2^lde_bits) == 1: plonky2 would divide by
 * zero); a device pointer; a configuration zkm_blob_describe refuses.  A refusal or a rejection leaves the context usable and its
 * live memory as it was.
 * Out of scope: PLONK's own checks (vanishing polynomial, partial products, public inputs); deriving the openings; compressed FRI
 * proofs; the pool; running this check under the "verify" tuning key behind zkm_fri_prove, which has neither caps nor openings at hand. */
int zkm_fri_verify(zkm_ctx* ctx, const zkm_stark_config* cfg, size_t nproofs, const uint64_t* const* proofs, const size_t* proof_words,
                   const unsigned* log_n, const size_t* const* oracle_cols, const size_t* noracles, const uint64_t* const* const* oracle_caps,
                   const zkm_fri_batch* const* batches, const size_t* nbatches, const uint64_t* const* const* opened,
                   zkm_challenger* const* challengers, zkm_verify_report* reports, char** err);

/* a9: StarkOpeningSet::new building block (proof.rs:299-334): p(zeta) in F2 for every polynomial of the
 * batch; out = ncols x 2 words, host. */
int zkm_eval_openings(zkm_ctx* ctx, const zkm_batch* b, const uint64_t zeta[2], uint64_t* out, char** err);
/* ... of a stack (zkm_batch_commit_values_stack), each member at its own point: zetas = nstack x 2 words, out = nstack x ncols x 2 words,
 * host; member k's words are zkm_eval_openings' on member k's single commitment.  One set of launches, one host wait. */
int zkm_eval_openings_stack(zkm_ctx* ctx, const zkm_batch* b, const uint64_t* zetas, uint64_t* out, char** err);

/* ------------------------------------------------------------------ profiling (HIP events on the ctx stream) */
void zkm_profile_enable(zkm_ctx* ctx, int on);
void zkm_profile_reset(zkm_ctx* ctx);
/* number of distinct kernel names recorded since reset */
size_t zkm_profile_count(zkm_ctx* ctx);
/* i-th record: name (static string), number of launches, summed device milliseconds */
int zkm_profile_get(zkm_ctx* ctx, size_t i, const char** name, uint64_t* launches, double* total_ms);

const char* zkm_version(void);

#ifdef __cplusplus
}
#endif
#endif
