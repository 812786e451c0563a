// zkm_internal.h -- shared host-side declarations of libzkmhip.so (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <exception>
#include <map>
#include <memory>
#include <mutex>
#include <tuple>
#include <type_traits>
#include <stdexcept>
#include <string>
#include <initializer_list>
#include <vector>

#include "../../include/zkm_hip.h"
#include "gl_dev.h"
#include "proof_blob.h"
#include "tables.h"

#define ZKM_HIP_CHECK(expr)                                                                                  \
    do {                                                                                                     \
        hipError_t _e = (expr);                                                                              \
        if (_e != hipSuccess)                                                                                \
            throw std::runtime_error(std::string(#expr) + ": " + hipGetErrorString(_e) + " (" + __FILE__ + ":" + \
                                     std::to_string(__LINE__) + ")");                                        \
    } while (0)

// an error that belongs to ONE segment of a stacked launch (position in the stack); what() is the reference's message
struct zkm_segment_error : std::runtime_error {
    size_t seg;
    zkm_segment_error(size_t s, const char* msg) : std::runtime_error(msg), seg(s) {}
};

struct zkm_prof_rec {
    const char* name;
    hipEvent_t start, stop;
};

#ifndef ZKM_MAX_SEG
#define ZKM_MAX_SEG 32       // segments one lock-step group may hold (per-segment challenges travel in kernel-argument arrays of this size)
#endif
struct seg_gl { gl_t v[ZKM_MAX_SEG]; };          // one base-field word per segment
struct seg_gl2 { gl_t v[2 * ZKM_MAX_SEG]; };     // two per segment (an F2 element, or the <= 2 constraint challenges)

#ifndef ZKM_COMMIT_LANES
#define ZKM_COMMIT_LANES 4   // trace commitments in flight per context (the context itself + 3 lanes)
#endif
#ifndef ZKM_LEAF_MFMA_DEFAULT
#define ZKM_LEAF_MFMA_DEFAULT 1
#endif

// K segments served by ONE launch (the witness generators; the prover's kernels use the same idiom, zkm_batch): descriptor s sits in
// kernel-argument slot s, the kernel takes its segment from blockIdx.z -- a uniform read, so the descriptor lives in scalar registers --
// and the grid's x extent is the largest segment's; workgroups beyond a segment's own extent leave at once.
template <class A> struct zkm_seg_args { A v[ZKM_MAX_SEG]; };
// Descriptors that travel in device memory instead (the calls' expansions'): zkm_seg_desc is segment blockIdx.z's, read through the
// constant address space -- the descriptors went up before the launch and no kernel writes them -- so the read is scalar, and the
// pointers it holds are known to be global as kernel-argument pointers are (read as generic pointers they would make every access a
// flat one and no second-level load a scalar one).
#ifdef __HIPCC__
template <class A> __device__ __forceinline__ A zkm_seg_desc(const A* segs) {
    A a;
    __builtin_memcpy(&a, (const __attribute__((address_space(4))) A*)segs + blockIdx.z, sizeof(A));
    return a;
}
#endif

struct zkm_twiddles {
    gl_t* fwd = nullptr;  // per-stage tables concatenated: entry (1<<s) + j = w_{2^(s+1)}^j, j < 2^s
    gl_t* inv = nullptr;  // same with inverse roots
    unsigned log_max = 0;
};

struct zkm_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t copy_stream = nullptr;  // host -> device ingest, overlapped with the compute stream (created on first use)
    hipStream_t copy_stream2 = nullptr; // second upload stream of staged traces (zkm_trace_stage: alternate pieces, two copy engines)
    hipStream_t side_stream = nullptr;  // the bootstrap's sponge chains beside the other tables' generation (created on first use)
    int boot_chain_quad = 0;            // the chains' permutation across a quad of lanes instead of a 16-lane row (tools/boot_time.py times both)   } zkm_ctx_set_tuning
    int image_hash_form = 0;            // the level launches of zkm_image[s]_hash: 0 by chain count, 1 the 16-lane row form, 2 the quad form   } zkm_ctx_set_tuning
    size_t image_hash_row_max = 8192;   // ... by chain count: the row form up to this many chains of a level in one launch -- two waves on each of the
                                        // 1024 SIMDs -- the quad form above (profiles/image_hash_time.json: 2.12 against 2.32 ms at 8192 chains, 2.70 against 2.35 at 10240)
    size_t ingest_chunk_cols = 32;     // columns per ingest chunk (0 = monolithic upload)           } zkm_ctx_set_tuning
    size_t keccak_parts_max_points = (size_t)1 << 15;   // k_quotient_keccak_parts up to this many points  }
    size_t fri_fused_division_min = ~(size_t)0;         // k_seg_scan_final from this many coefficients (default: never -- since the
                                                        // LDS-tiled kernels of round 4 the per-batch scans are faster at every size)  }
    int fri_scan_combine = 1;           // bottom level of the division by (X - z): scan and weighted sum in one launch (0: two launches)   } zkm_ctx_set_tuning
    size_t small_ntt = 1;               // transforms of 2^9 .. 2^13 points in one launch (k_ntt_small); 0: the two-pass plan          } zkm_ctx_set_tuning
    unsigned pow_round_log = 17;        // proof-of-work search: 2^this candidates per round of the search launch                          } zkm_ctx_set_tuning
    int aux_pipeline = 1;               // segments of short tables: lanes build later tables' auxiliary commitments behind the proofs      } zkm_ctx_set_tuning
    size_t commit_lanes = ZKM_COMMIT_LANES;   // trace / auxiliary commitments of one segment in flight (this context + lanes)   } zkm_ctx_set_tuning
    size_t segments_memory_budget = 0;  // bytes one wave of a zkm_prove_segments call may hold (0: 80 % of cached + free HBM, shared out over the contexts of the process that are inside such a call)   } zkm_ctx_set_tuning
    int pool_stage_ahead = 1;           // a pool worker of zkm_pool_prove_segments_calls keeps its next group staged behind the current proofs (0: each group one expanding call)   } zkm_ctx_set_tuning
    size_t last_stack = 0;             // segments of the previous prove_with_traces call of this context (0: none yet)
    size_t prev_stack = 0;              // ... and the other height whose blocks may still be cached (two heights are kept: ctl.hip prove_segments_impl)
    size_t max_stack = ZKM_MAX_SEG;     // segments of one lock-step group (zkm_prove_segments): 1 .. ZKM_MAX_SEG               } zkm_ctx_set_tuning
    int leaf_mfma = ZKM_LEAF_MFMA_DEFAULT;   // one-lane-per-leaf hashing: MDS layers of the full rounds on the matrix core (poseidon_mfma_dev.h)   } zkm_ctx_set_tuning
    size_t wide_max_hashes = 1024;      // launches of up to this many hashes use 16 lanes per hash (latency form)   } 0 / 0: one lane
    size_t quad_max_hashes = 32768;     // ... and up to this many four lanes per hash                                } per hash always
    int num_cus = 256;
    int cu_part_k = -1, cu_part_n = 0;   // measurement aid (ZKM_CU_MASK_PART): the streams of this context are confined to one part of the CUs
    // profiling
    bool profiling = false;
    std::vector<zkm_prof_rec> prof;
    std::vector<hipEvent_t> event_pool;
    struct agg { const char* name; uint64_t launches; double ms; };
    std::vector<agg> prof_agg;
    bool prof_agg_valid = false;
    // caching allocator: exact-size free lists
    std::multimap<size_t, void*> free_blocks;
    std::map<void*, size_t> live_blocks;
    std::mutex alloc_mu;                // guards the two maps (the out-of-memory path of a relative trims this cache from its thread)
    zkm_ctx* parent = nullptr;          // of a commit lane: the context that owns it
    std::atomic<int> debug_fail_allocs{0};   // test hook (root context only): pretend the next k hipMalloc first attempts fail
    int check_ctls = 0;                 // the prove drivers run check_ctls on each segment's tables before they prove (ctl_check.hip)   } zkm_ctx_set_tuning
    int check_witness = 0;              // the prove drivers run the three witness checks on each wave's segments before they commit (segment_check.hip)   } zkm_ctx_set_tuning
    unsigned debug_ctl_key_bits = 0;    // test hook: the FIRST attempt of a check_ctls call sorts by keys truncated to this many bits (0: off)
    int verify = 0;                     // the prove drivers verify every segment's blobs before they hand them out (verify.hip)   } zkm_ctx_set_tuning
    uint64_t debug_verify_flip = 0;     // test hook: under `verify`, this word of one segment's blobs is changed before it is verified (0: off)
    // twiddles
    zkm_twiddles tw;
    // power tables for coset scaling: key (shift, log_n) -> device ptr [lo table 2^h | hi table 2^(log_n-h)]
    std::map<std::pair<uint64_t, unsigned>, gl_t*> pow_tables;
    // block twiddles of the coset-split LDE's upper stages: key (shift, log_n, stages) -> device ptr [4 cosets][2^stages]
    std::map<std::tuple<uint64_t, unsigned, unsigned>, gl_t*> lde_ct_tables;
    size_t resident_bytes = 0;  // of the live blocks: tables kept for reuse (twiddles, power tables, block twiddles)
    // pinned host staging
    uint64_t* h_staging = nullptr;
    size_t h_staging_words = 0;
    // commit lanes (ctl.hip zkm_prove_with_traces): sub-contexts -- own stream, allocator, twiddle / power tables, profiler records --
    // on which the independent trace commitments of one segment are built side by side, one host thread each.  Owned by this
    // context (created on first use, destroyed with it); a lane has no lanes of its own.  A batch remembers the (sub-)context
    // that built it and returns its memory there.
    std::vector<zkm_ctx*> lanes;
    void ensure_lanes(size_t k);

    void* alloc(size_t bytes);
    void release(void* p);
    void trim_self();  // hipFree every cached (not live) block of THIS allocator (any thread: used by a relative's out-of-memory retry)
    void trim();       // ... and of the lanes; only between calls
    void drop_copy_streams();   // trim(): the idle upload streams and the side stream give their hardware queues back
    hipStream_t ensure_copy_stream(int k = 0);   // upload stream k (0: copy_stream, 1: copy_stream2), created on first use
    hipStream_t ensure_side_stream();            // side_stream, created on first use
    void shrink_down();   // the pinned download area back to its base size (trim(): between calls, owner's thread)
    void ensure_twiddles(unsigned log_n);
    const gl_t* pow_table(uint64_t shift, unsigned log_n);  // lo: 2^ceil(log_n/2) entries, then hi
    uint64_t* staging(size_t words);
    // Small transfers of the transcript round trips (caps, opening partials, FRI final polynomial, proof-of-work witness, query rounds
    // down; challenge powers, query indices, descriptors up) go through pinned memory: a copy from / to pageable memory is staged by the
    // runtime inside the call (a blit into its own pinned buffer, a host copy, and both of them behind the runtime's locks).
    struct xfer { void* dst; const void* src; size_t bytes; };
    void download(std::initializer_list<xfer> xs);               // all device -> host, then ONE stream synchronisation
    void download(void* dst, const void* src, size_t bytes) { download({xfer{dst, src, bytes}}); }
    void upload(void* dst, const void* src, size_t bytes);       // host -> device on the stream; `src` may be reused on return
    char* h_xfer = nullptr;                                      // [0, XFER_UP): upload ring,
                                                                 // then one cache line for the completion flag of k_download
    uint64_t down_seq = 0;
    void wait_flag(const uint64_t* flag, uint64_t seq);          // spin, then (crowded process) block: core.hip
    uint64_t block_after_us = 50;                                // } zkm_ctx_set_tuning "block_after_us" (0: always block)
    hipEvent_t block_event = nullptr;
    uint64_t blocked_waits = 0;                                  // round trips that ended in the blocking wait (diagnostic)
    void ensure_xfer();
    // a kernel that delivers a small result to the host ITSELF (hash.hip k_merkle_tail): xfer_begin hands out the pinned slot, the flag,
    // a zeroed device word for "last workgroup publishes" and the sequence number to publish; xfer_finish waits for it and copies out
    uint64_t xfer_begin(size_t bytes, uint64_t** host_slot, uint64_t** flag, unsigned** counter);
    void xfer_finish(uint64_t seq, void* dst, size_t bytes);
    unsigned* d_counter = nullptr;
    unsigned long long* d_pow_best = nullptr;                    // the proof-of-work search's result word: all ones between searches
    unsigned long long* pow_best();
    size_t tree_tail = 1;               // trees of <= 2^15 leaves in one launch incl. the cap's trip to the host; 0: levels + download      } zkm_ctx_set_tuning
    size_t up_off = 0;
    char* h_down = nullptr;                                      // pinned download area, down_cap bytes (grows: ensure_down)
    size_t down_cap = 0;
    void ensure_down(size_t bytes);
    static constexpr size_t XFER_DOWN = (size_t)1 << 20, XFER_DOWN_MAX = (size_t)1 << 28, XFER_UP = (size_t)1 << 18;
    hipEvent_t get_event();
    size_t prof_begin(const char* name);   // returns the record's index (scopes nest: a stage scope holds kernel scopes)
    void prof_end(size_t idx);
    uint64_t host_waits = 0;            // times a thread waited for this context's stream (sync, wait_flag, ensure_down): callers that report their waits read the difference
    void sync() { host_waits++; ZKM_HIP_CHECK(hipStreamSynchronize(stream)); up_off = 0; }
};


// ---- the C ABI's error boundary (include/zkm_hip.h "Error convention"): the one writer of *err, and the one place an exception becomes
// a status.  zkm_api runs an entry point's body: 0 when it returns (or the int it returns, for a body that delegates to another entry
// point), 1 and the message when it throws.  The context form rejects a null context and makes the context's device current.
inline int zkm_fail(char** err, const char* msg, const char* suffix = "") noexcept {
    if (err) {
        const size_t a = strlen(msg), b = strlen(suffix);
        *err = (char*)malloc(a + b + 1);
        if (*err) { memcpy(*err, msg, a); memcpy(*err + a, suffix, b + 1); }
    }
    return 1;
}
template <class F> int zkm_api(const char* what, char** err, F&& body) noexcept {
    try {
        if constexpr (std::is_void_v<decltype(body())>) {
            body();
            return 0;
        } else {
            return body();
        }
    } catch (const std::exception& e) {
        return zkm_fail(err, e.what());
    } catch (...) {
        return zkm_fail(err, what, ": unknown error");
    }
}
template <class F> int zkm_api(const char* what, const zkm_ctx* c, char** err, F&& body) noexcept {
    return zkm_api(what, err, [&] {
        if (!c) throw std::runtime_error(std::string(what) + ": null argument");
        ZKM_HIP_CHECK(hipSetDevice(c->device));
        return body();
    });
}

// RAII owner of scratch blocks from the context's allocator, released on every exit path.  Blocks released while an exception unwinds
// may still be in use by work queued on the context's stream: the owner waits for the stream first (a normal exit adds no wait).
struct zkm_scratch_list {
    zkm_ctx* c;
    std::vector<void*> ps;
    const int unwinding = std::uncaught_exceptions();
    explicit zkm_scratch_list(zkm_ctx* ctx) : c(ctx) {}
    zkm_scratch_list(const zkm_scratch_list&) = delete;
    zkm_scratch_list& operator=(const zkm_scratch_list&) = delete;
    ~zkm_scratch_list() {
        if (std::uncaught_exceptions() > unwinding) (void)hipStreamSynchronize(c->stream);
        for (void* p : ps) c->release(p);
    }
    template <class T = void> T* alloc(size_t bytes) {
        ps.reserve(ps.size() + 1);   // (push_back cannot throw once the block exists)
        ps.push_back(c->alloc(bytes));
        return (T*)ps.back();
    }
};
// ... of one block, movable: it goes back to the allocator that made it (a block of commit lane w to w's, whichever thread drops it),
// on the same terms -- reset() or the destructor; take() hands the block out of the owner.
struct zkm_scratch {
    zkm_ctx* c = nullptr;
    void* p = nullptr;
    int unwinding = std::uncaught_exceptions();
    zkm_scratch() = default;
    zkm_scratch(zkm_ctx* ctx, size_t bytes) : c(ctx), p(ctx->alloc(bytes)) {}
    zkm_scratch(zkm_scratch&& o) noexcept : c(o.c), p(o.take()) {}
    zkm_scratch& operator=(zkm_scratch&& o) noexcept {
        reset();
        c = o.c;
        p = o.take();
        return *this;
    }
    ~zkm_scratch() { reset(); }
    void reset() noexcept {
        if (!p) return;
        if (std::uncaught_exceptions() > unwinding) (void)hipStreamSynchronize(c->stream);
        c->release(take());
    }
    void* take() noexcept {
        void* q = p;
        p = nullptr;
        return q;
    }
    template <class T> T* as() const { return (T*)p; }
};

// Owner of one pooled event (zkm_ctx::get_event), movable: it goes back to the pool of the context that issued it.  The pools are not
// thread-safe: the owner of a commit lane's event is destroyed on the thread that drives that lane, or on the caller's thread after the
// lanes have been joined -- never while the lane's thread may still take events from the same pool.
struct zkm_event {
    zkm_ctx* c = nullptr;
    hipEvent_t e = nullptr;
    zkm_event() = default;
    explicit zkm_event(zkm_ctx* ctx) : c(ctx), e(ctx->get_event()) {}
    zkm_event(zkm_event&& o) noexcept : c(o.c), e(o.e) { o.e = nullptr; }
    zkm_event& operator=(zkm_event&& o) noexcept {
        reset();
        c = o.c;
        e = o.e;
        o.e = nullptr;
        return *this;
    }
    ~zkm_event() { reset(); }
    void reset() noexcept {
        if (e) c->event_pool.push_back(e);
        e = nullptr;
    }
    void record(hipStream_t st) const { ZKM_HIP_CHECK(hipEventRecord(e, st)); }
};

// Owner of pinned host words that a queued copy writes (a staged handle's verdicts).
template <class T> struct zkm_pinned {
    T* p = nullptr;
    zkm_pinned() = default;
    zkm_pinned(const zkm_pinned&) = delete;
    zkm_pinned& operator=(const zkm_pinned&) = delete;
    ~zkm_pinned() {
        if (p) (void)hipHostFree(p);
    }
    void alloc(size_t n) { ZKM_HIP_CHECK(hipHostMalloc((void**)&p, n * sizeof(T), hipHostMallocDefault)); }
};

// The ONE statement of how input is put into HBM behind the context's current work (the staged traces, operations, steps and calls;
// DESIGN.md 3, "Input staged behind the current work").  The work goes onto the context's two copy streams, and the fence sees to the
// orderings that make that safe:
//   begin   the copy streams go behind what the compute stream has queued -- the block being filled may be one a finished call of
//           this context released -- and the fence is ARMED: destroyed now (an exception unwinds the stage), it waits on the host for
//           both copy streams, so that what is in flight lands before the block and the host memory it reads go away
//   end     one event behind the work on each copy stream; the fence is ENDED and stands for that work from here on: ready / wait
//           look at the events from the host, join puts the compute stream behind them (once, a device-side wait), and the
//           destructor waits for them before the handle's block goes back to an allocator whose blocks later work of the compute
//           stream reuses
// A handle declares its fence BEHIND the blocks and the host memory that the queued work uses: members go in reverse order, so the fence
// has waited by the time they do.  The events are pooled ones: a fence is destroyed on the thread that drives its context (zkm_event).
struct zkm_copy_fence {
    zkm_copy_fence() = default;
    zkm_copy_fence(const zkm_copy_fence&) = delete;
    zkm_copy_fence& operator=(const zkm_copy_fence&) = delete;
    ~zkm_copy_fence() {
        if (armed) {
            (void)hipSetDevice(c->device);
            (void)hipStreamSynchronize(c->copy_stream);
            (void)hipStreamSynchronize(c->copy_stream2);
        } else if (done[0].e) {
            wait();
        }
    }
    void begin(zkm_ctx* ctx) {
        c = ctx;
        const hipStream_t up[2] = {c->ensure_copy_stream(0), c->ensure_copy_stream(1)};
        const zkm_event e(c);
        e.record(c->stream);
        for (const hipStream_t st : up) ZKM_HIP_CHECK(hipStreamWaitEvent(st, e.e, 0));
        armed = true;
    }
    void end() { record(c->copy_stream, c->copy_stream2); }
    // ... without a begin, for a block that work already queued on the compute stream fills (zkm_staged_from_segment): both events on
    // that stream, and nothing left to join
    void end_on_compute(zkm_ctx* ctx) {
        c = ctx;
        record(c->stream, c->stream);
        joined = true;
    }
    void disarm() { armed = false; }   // a stage that records no events of its own (calls_stage.hip: its staged steps' stand for it)
    // 1: the work has ended, 0: it is in flight (wait: block until it has ended instead), -1: the runtime reports an error.  (A fence
    // that never began stands for no work: ready, and nothing to wait for)
    int ready(bool wait) const {
        if (!c) return 1;
        (void)hipSetDevice(c->device);
        for (const zkm_event& e : done) {
            if (wait) {
                if (hipEventSynchronize(e.e) != hipSuccess) return -1;
            } else {
                const hipError_t q = hipEventQuery(e.e);
                if (q == hipErrorNotReady) return 0;
                if (q != hipSuccess) return -1;
            }
        }
        return 1;
    }
    void wait() const noexcept {
        if (!c) return;
        (void)hipSetDevice(c->device);
        (void)hipEventSynchronize(done[0].e);
        (void)hipEventSynchronize(done[1].e);
    }
    void join() {
        if (joined) return;
        for (const zkm_event& e : done) ZKM_HIP_CHECK(hipStreamWaitEvent(c->stream, e.e, 0));
        joined = true;
    }
    bool is_joined() const { return joined; }
    hipEvent_t event(int k) const { return done[k].e; }

private:
    zkm_ctx* c = nullptr;
    zkm_event done[2];
    bool armed = false, joined = false;
    void record(hipStream_t s0, hipStream_t s1) {
        done[0] = zkm_event(c);
        done[1] = zkm_event(c);
        done[0].record(s0);
        done[1].record(s1);
        armed = false;
    }
};

// hipFuncSetAttribute is per device: `done` remembers the devices on which `kernel`'s dynamic-LDS limit has been raised (one bit per
// device; a process may hold contexts on several GPUs, and several host threads may get here at once -- setting it twice is harmless).
// The limit goes to a fixed maximum, never to what the current launch needs: a later, larger launch finds it raised.  Returns the
// runtime's answer: a caller with a smaller launch to fall back on checks it, the others wrap the call in ZKM_HIP_CHECK.
inline hipError_t zkm_allow_big_lds(const zkm_ctx* c, const void* kernel, std::atomic<uint64_t>& done, int limit = 160 * 1024) noexcept {
    const uint64_t bit = (uint64_t)1 << (c->device & 63);
    if (done.load(std::memory_order_acquire) & bit) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, limit);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return e;
    }
    done.fetch_or(bit, std::memory_order_release);
    return hipSuccess;
}

// RAII profiling scope around one kernel launch (or a small group).  Names starting with "stage/" are the reference's timed!
// scopes (prover.rs:146-153, 193, 204, 479, 513, 545, 578, 620): event pairs at the stage boundaries, reported beside the kernel
// records (consumers separate the two by the prefix; a stage's time includes its transcript round trips and launch gaps).
struct zkm_prof_scope {
    zkm_ctx* c;
    size_t idx = 0;
    bool on;
    zkm_prof_scope(zkm_ctx* ctx, const char* name) : c(ctx), on(ctx->profiling) {
        if (on) idx = c->prof_begin(name);
    }
    zkm_prof_scope(const zkm_prof_scope&) = delete;
    zkm_prof_scope& operator=(const zkm_prof_scope&) = delete;
    ~zkm_prof_scope() {
        if (on) c->prof_end(idx);
    }
};

// A batch may hold the SAME-SHAPED polynomials of `nseg` independent segments (zkm_prove_segments: K segments advance through every
// stage of prove_with_traces in lock-step, one launch per stage): segment s owns columns [s ncols, (s + 1) ncols) of the coefficient and
// LDE matrices (column strides n and N as ever, so the transforms see nseg * ncols columns), its own block of dig_words digest words
// (level_off is relative to the block) and cap words [s capw, (s + 1) capw).  Kernels take the segment from blockIdx.z.
struct zkm_batch {
    zkm_ctx* ctx = nullptr;
    size_t ncols = 0;         // per segment
    size_t nseg = 1;
    unsigned log_n = 0, rate_bits = 0, cap_height = 0;
    gl_t* coeffs = nullptr;   // nseg x ncols x n; position P of a column = coefficient of X^zkm_coeff_exponent(P, coeff_s1)
    unsigned coeff_s1 = 0;    // 0: natural order; else the digit layout of the two-pass inverse transform (2^18 .. 2^20 rows)
    gl_t* lde = nullptr;      // nseg x ncols x N, rows bit-reversed
    gl_t* digests = nullptr;  // per segment: levels 0..top concatenated, 4 words per node
    size_t dig_words = 0;     // digest words of one segment's tree
    std::vector<size_t> level_off;  // word offsets (within a segment's block)
    std::vector<uint64_t> cap;      // host copy, nseg x (4 << cap_height) words
    size_t coeff_seg() const { return ncols << log_n; }
    size_t lde_seg() const { return ncols << (log_n + rate_bits); }
    size_t n() const { return (size_t)1 << log_n; }
    size_t N() const { return (size_t)1 << (log_n + rate_bits); }
    unsigned lde_bits() const { return log_n + rate_bits; }
    unsigned top() const { return lde_bits() - cap_height; }
};

// owner of a batch until it is handed out (zkm_batch_free: waits for the streams, releases the blocks)
struct zkm_batch_deleter {
    void operator()(zkm_batch* b) const { zkm_batch_free(b); }
};
using zkm_batch_ptr = std::unique_ptr<zkm_batch, zkm_batch_deleter>;
// an empty batch of this shape (zkm_batch_build fills it in); core.hip
zkm_batch_ptr zkm_batch_new(zkm_ctx* c, size_t ncols, size_t nseg, unsigned log_n, unsigned rate_bits, unsigned cap_height);

// Copies of the callers' transcripts for a prove call to advance (chs: what the stages take); commit() hands them back once the whole
// proof exists.  A call that fails on the way -- the reference's prove_openings cannot fail half way; a C ABI call can -- never gets
// there, and leaves every caller's challenger where it was.
struct zkm_transcripts {
    std::vector<zkm_challenger*> callers;
    std::vector<zkm_challenger> local;
    std::vector<zkm_challenger*> chs;
    zkm_transcripts(zkm_challenger* const* callers_, size_t n) : callers(callers_, callers_ + n), local(n), chs(n) {
        for (size_t k = 0; k < n; k++) { local[k] = *callers[k]; chs[k] = &local[k]; }
    }
    explicit zkm_transcripts(zkm_challenger* caller) : zkm_transcripts(&caller, 1) {}
    zkm_transcripts(const zkm_transcripts&) = delete;   // (chs points into local)
    void commit() {
        for (size_t k = 0; k < callers.size(); k++) *callers[k] = local[k];
    }
};

inline bool zkm_is_device_ptr(const void* p) {
    hipPointerAttribute_t a;
    hipError_t e = hipPointerGetAttributes(&a, p);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return a.type == hipMemoryTypeDevice;
}

template <class A, class... X>
void zkm_launch_segs(hipStream_t stream, void (*kernel)(zkm_seg_args<A>, X...), const A* segs, size_t nseg, size_t grid_x, unsigned threads, X... x) {
    static_assert(sizeof(zkm_seg_args<A>) + sizeof...(X) * 8 <= 3840, "the descriptors travel as kernel arguments (4 KiB)");
    if (nseg == 0 || nseg > ZKM_MAX_SEG) throw std::runtime_error("zkm_launch_segs: segment count out of range");
    if (!grid_x) return;
    zkm_seg_args<A> S{};
    std::copy(segs, segs + nseg, S.v);
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid_x, 1, (unsigned)nseg), dim3(threads), 0, stream, S, x...);
    ZKM_HIP_CHECK(hipGetLastError());
}

// ---- hash.hip
void zkm_launch_poseidon_permute(zkm_ctx*, gl_t* states, size_t k);
void zkm_launch_mul_selftest_branchfree(zkm_ctx*, const uint64_t* a, const uint64_t* b, size_t n, uint64_t* out);  // stark.hip
void zkm_launch_keccakf(zkm_ctx*, uint64_t* states, size_t k);
// leaf digests of a column-major matrix (row j across ncols columns of stride `col_stride` words)
// nseg > 1: segment s reads lde + s * lde_seg and writes digests + s * dig_seg (blockIdx.z)
void zkm_launch_merkle_leaves(zkm_ctx*, const gl_t* lde, size_t nrows, size_t ncols, size_t col_stride, gl_t* digests, size_t nseg = 1,
                              size_t lde_seg = 0, size_t dig_seg = 0);
// the same digests from column chunks: state = 12 x nrows words kept between the chunks of one matrix (see hash.hip)
void zkm_launch_merkle_leaves_chunk(zkm_ctx*, const gl_t* lde, size_t nrows, size_t nc, size_t col_stride, gl_t* state, bool first,
                                    bool last, gl_t* digests);
void zkm_ntt_natural_ex(zkm_ctx* c, const gl_t* in, size_t cs_in, gl_t* scratch, size_t cs_s, gl_t* out, size_t cs_out, size_t ncols,
                        unsigned log_n, bool inverse, uint64_t shift);
// leaf digests of row-major leaves formed from F2 SoA arrays: leaf k = 16 consecutive (c0,c1) pairs
// (nseg > 1: segment s reads c0 / c1 + s * val_seg and writes digests + s * dig_seg)
void zkm_launch_merkle_leaves_ext(zkm_ctx*, const gl_t* c0, const gl_t* c1, size_t nleaves, unsigned arity, gl_t* digests, size_t nseg = 1,
                                  size_t val_seg = 0, size_t dig_seg = 0);
// build all digest layers above level 0; fills level_off and returns total words needed (call with digests==nullptr to size)
size_t zkm_merkle_layout(unsigned log_leaves, unsigned cap_height, std::vector<size_t>& level_off);
// (nseg trees of the same shape, dig_seg words apart: one launch per group of levels for all of them)
void zkm_merkle_build_inner(zkm_ctx*, gl_t* digests, const std::vector<size_t>& level_off, unsigned log_leaves, unsigned cap_height,
                            size_t nseg = 1, size_t dig_seg = 0);
// ... and the caps into cap_out (host, nseg x (4 << cap_height) words): one launch for small trees (zkm_merkle_tail), levels + download otherwise
void zkm_merkle_build_inner_cap(zkm_ctx*, gl_t* digests, const std::vector<size_t>& level_off, unsigned log_leaves, unsigned cap_height,
                                uint64_t* cap_out, size_t nseg = 1, size_t dig_seg = 0);
bool zkm_merkle_tail(zkm_ctx*, gl_t* digests, const std::vector<size_t>& level_off, unsigned log_leaves, unsigned cap_height, uint64_t* cap_out,
                     unsigned l0, size_t nseg = 1, size_t dig_seg = 0);

// ---- ntt.hip
// in-place, natural -> bit-reversed order, forward or inverse roots, no scaling
void zkm_ntt_dif_bitrev(zkm_ctx*, gl_t* data, size_t ncols, size_t col_stride, unsigned log_n, bool inverse);
// natural -> natural into `out` (may not alias `in`), using `in` as scratch (destroyed).
//   inverse: out = iNTT(in) * shift^-i ; forward: out = NTT(in * shift^i)   (shift 0/1 = none)
void zkm_ntt_natural(zkm_ctx*, gl_t* in_scratch, gl_t* out, size_t ncols, size_t col_stride_in, size_t col_stride_out,
                     unsigned log_n, bool inverse, uint64_t shift);
// out[c][i] = in[c][i] * shift^i for i < n_in, 0 for n_in <= i < n_out  (columns strided)
void zkm_launch_scale_pad(zkm_ctx*, const gl_t* in, size_t col_stride_in, gl_t* out, size_t col_stride_out, size_t ncols,
                          unsigned log_n_in, unsigned log_n_out, uint64_t shift);
// coset LDE of coefficients (natural order, or the digit layout when coeff_s1 != 0) into bit-reversed evaluations: out (ncols x 2^(log_n+rate_bits))
void zkm_lde_bitrev(zkm_ctx*, const gl_t* coeffs, gl_t* out, size_t ncols, unsigned log_n, unsigned rate_bits, uint64_t shift,
                    unsigned coeff_s1 = 0);
// ---- coefficient layout of a batch (ntt.hip zkm_intt_digit): position P of a column holds the coefficient of X^zkm_coeff_exponent(P).
// s1 = 0: natural order.  s1 = log_n - 12 for 2^18 .. 2^20 rows: what the two-pass inverse transform leaves (see ntt.hip).
inline unsigned zkm_coeff_layout_s1(unsigned log_n) { return (log_n >= 18 && log_n <= 20) ? log_n - 12 : 0; }
GL_HD uint32_t zkm_coeff_exponent(uint32_t P, unsigned s1) {
    if (!s1) return P;
    const uint32_t t_hi = P & ((1u << s1) - 1), cc = (P >> s1) & ((1u << (12 - s1)) - 1), blk = P >> 12;
    return (t_hi << 12) | (cc << s1) | bitrev32(blk, s1);
}
// values (natural, read-only) -> coefficients in the digit layout, two passes; coefficient columns to / from natural order (in != out)
void zkm_intt_digit(zkm_ctx*, const gl_t* values, size_t cs_in, gl_t* coeffs, size_t cs_out, size_t ncols, unsigned log_n);
void zkm_coeff_layout_convert(zkm_ctx*, const gl_t* in, size_t cs_in, gl_t* out, size_t cs_out, size_t ncols, unsigned log_n, bool to_natural);

// ---- core.hip
int zkm_live_contexts();   // contexts of this process that exist right now (zkm_ctx_create .. zkm_ctx_destroy; lanes not counted)
// dev_values (optional, ncols x n words of device memory): host values are uploaded THERE and stay (the caller reuses them, e.g. for
// the CTL columns of prove_with_traces) instead of being staged inside the batch's LDE buffer.
// src_cols (optional, instead of src): one pointer per column (each n words, host or device).
void zkm_batch_build(zkm_batch* b, const uint64_t* src, bool src_is_values, gl_t* dev_values = nullptr,
                     const uint64_t* const* src_cols = nullptr, const uint64_t* const* seg_srcs = nullptr);
// a new batch of nseg members committed to srcs[0 .. nseg) (values, or coefficients in natural order; host or device): the one place that
// chooses between zkm_batch_build's single form (nseg == 1: srcs[0]) and its per-member sources (throws)
zkm_batch_ptr zkm_batch_commit(zkm_ctx* c, const uint64_t* const* srcs, size_t nseg, size_t ncols, unsigned log_n, unsigned rate_bits,
                               unsigned cap_height, bool are_values);
zkm_batch* zkm_batch_commit_values_keep(zkm_ctx* c, const uint64_t* values, size_t ncols, unsigned log_n, unsigned rate_bits,
                                        unsigned cap_height, gl_t* dev_values, const uint64_t* const* columns = nullptr);
// stark.hip: prove_single_table from existing (stacked) trace and auxiliary commitments, for chs.size() proofs in lock-step (throws)
void zkm_prove_table_from_commitments(zkm_ctx* c, int table_id, const zkm_stark_config* cfg, size_t ncols, unsigned log_n, const zkm_batch* trace_batch,
                                      const zkm_batch* aux_batch, size_t naux_ctl, const zkm_ctl_table* table, const zkm_ctl_z* zs,
                                      const uint32_t* colset_ids, size_t nzs, const uint64_t* lookup_challenges, const std::vector<zkm_challenger*>& chs,
                                      const std::vector<uint64_t*>& proofs);
void zkm_launch_canon(zkm_ctx* c, gl_t* v, size_t total);   // v[i] = canonical representative of v[i], in place
void zkm_host_poseidon_permute(uint64_t st[12]);
void zkm_host_poseidon_permute_reference(uint64_t st[12]);   // poseidon_dev.h compiled for the host (cross-check)
// ---- hash.hip (LogicStark witness)
// ---- tables' own logUp lookups (tables.h: definitions; ctl.hip: helper columns)
const zkm_table_lookup* zkm_table_lookups(int table_id, size_t* n);
void zkm_table_lookup_columns_device(zkm_ctx* c, int table_id, const uint64_t* challenges, size_t nch, const gl_t* d_trace, size_t n,
                                     gl_t* d_out, size_t nseg = 1, size_t trace_seg = 0, size_t out_seg = 0);
// ---- witness.hip: the data-parallel writers, K segments a launch.  One descriptor serves every table: `in` are the table's input lists
// in the order of its description (tables.h zkm_writer; a sponge: the bytes, their offsets, the meta words, the first row of each
// operation), k the operations, n the table's rows, aux the Poseidon seed or the KeccakSponge rows in use, bad the Logic flag; tmp is
// the KeccakSponge scratch (filled in by the launcher).
struct zkm_writer_seg {
    const void* in[4];
    size_t k, n, aux;
    gl_t* out;
    int* bad;
    void* tmp[2];
};
void zkm_launch_writers(zkm_ctx* c, int table_id, const zkm_writer_seg* segs, size_t nseg);

// ---- the two witnesses whose heights need the device, in phases: zkm_memory_trace / zkm_arithmetic_trace run each one's phases back
// to back with a host wait between them; segment_ops.hip runs the phases of both side by side, so that one wait serves both.  A phase
// throws with `what` in front of its message; the job owns its scratch blocks until it goes.
// memory_trace.hip: widths (queues the OR of the key fields into d_acc[0..5)) -> the host reads d_acc -> sort (sort, gaps, scan: the row
// count before padding lands at start[nops]) -> the host reads it -> height -> write (rows and neighbours; *d_bad set on a range check
// of 2^log_n or more)
struct zkm_memory_job {
    zkm_ctx* c;
    const char* what;
    const uint64_t* d_ops;       // nops x 6 words, device
    size_t nops;
    zkm_scratch small, keys_a, keys_b, idx_a, idx_b, start;
    // [0, 5) OR of the key fields and the >= p flag, [5] last op with dummies; d_count: where the row count lands beside start[nops].
    // Null: in `small` ([6] free), which widths then allocates; a caller of several jobs points them into one block, for one download.
    unsigned long long* d_acc = nullptr;
    uint64_t* d_count = nullptr;
    const uint32_t* idx = nullptr;         // sorted order
    uint64_t M = 0, count = 0;
    zkm_memory_job(zkm_ctx* ctx, const char* w, const uint64_t* ops, size_t n) : c(ctx), what(w), d_ops(ops), nops(n) {}
};
// (the launching phases take nseg <= ZKM_MAX_SEG jobs of one context and serve them with ONE launch per kernel)
void zkm_memory_widths(zkm_memory_job* j, size_t nseg);
void zkm_memory_sort(zkm_memory_job* j, size_t nseg, const uint64_t* acc, size_t acc_stride);   // job s: acc[s * acc_stride + (0..5)]
size_t zkm_memory_height(zkm_memory_job& j, uint64_t count, size_t* natural_rows_out);   // next_pow2(count); throws if it saturated
void zkm_memory_write(zkm_memory_job* j, size_t nseg, const unsigned* log_n, gl_t* const* out_dev, int* const* d_bad);
// arithmetic_trace.hip: count (validation flags and the scan of the row counts: rows at start[nops], flags at start[nops + 1]) -> the
// host reads both -> height -> write (rows, RC_FREQUENCIES; *d_bad set on a shared-column value of 2^16 or more)
struct zkm_arith_job {
    zkm_ctx* c;
    const char* what;
    const uint32_t* d_ops;       // nops x 3 words, device (may be null when nops = 0)
    size_t nops;
    zkm_scratch start, hist;
    uint64_t rows = 0;
    zkm_arith_job(zkm_ctx* ctx, const char* w, const uint32_t* ops, size_t n) : c(ctx), what(w), d_ops(ops), nops(n) {}
    uint64_t* d_counts = nullptr;   // {rows, flags}: the two words the host reads.  Null: start[nops], start[nops + 1]
    uint64_t* counts() const { return d_counts ? d_counts : start.as<uint64_t>() + nops; }
};
void zkm_arithmetic_count(zkm_arith_job* j, size_t nseg);
size_t zkm_arithmetic_height(zkm_arith_job& j, const uint64_t got[2], size_t* natural_rows_out);   // max(2^16, next_pow2(rows)); throws on a flag
void zkm_arithmetic_write(zkm_arith_job* j, size_t nseg, const unsigned* log_n, gl_t* const* out_dev, unsigned* const* d_bad);

// ---- bootstrap.hip: a segment's bootstrap-kernel witness from its image, in phases (the file's head lists them).  One descriptor per
// segment, in device memory; a job owns the scratch block the descriptor points into.
struct zkm_boot_seg {
    const uint32_t *addrs, *values;              // the image, device
    uint32_t nwords, npages, rows_image, check;  // rows_image = ceil(nwords / 8)
    uint32_t id_words[9], want_root[8], want_id[8];   // check_image_id's nine words; the expected digests as LE words
    uint64_t *post, *digests;                    // state after each permutation (as po_in); (npages + 1) x 4
    uint32_t *pagew, *blk_count, *page_addr, *page_idx;   // (npages + 1) x 1024 message words; pages per 256 image words; the pages
    unsigned long long* flags;                   // [0] order / alignment, [1] page count, [2] missing hash word, [3] digest mismatch
    uint64_t *mem, *po_in, *po_ts;               // outputs: the boot's first memory operation / Poseidon input / timestamp
    gl_t *cpu, *ps;                              // cell (row r, column k) of the CPU rows at cpu[r cpu_rs + k cpu_cs]; ps likewise, or null
    size_t cpu_rs, cpu_cs, ps_rs, ps_cs;
};
struct zkm_boot_counts_t { size_t rows_image, cpu_rows, memory_ops, poseidon, sponge_ops; };   // poseidon: inputs = sponge rows
void zkm_boot_sizes(const zkm_boot_image* im, zkm_boot_counts_t* n);
size_t zkm_boot_scratch_bytes(const zkm_boot_image* im);   // what a job of this image holds beside the joined lists (0 for null)
struct zkm_boot_job {
    zkm_ctx* c;
    const zkm_boot_image* im;                    // null: a segment without a bootstrap (every phase passes it over)
    zkm_boot_counts_t n{};
    zkm_scratch scratch;
    zkm_boot_seg d{};
    zkm_boot_job(zkm_ctx* ctx, const zkm_boot_image* image);   // the host checks: throws the bare message
    void prepare();                              // scratch, the image's upload, `d` without flags and outputs (the caller sets those)
};
// (nseg <= ZKM_MAX_SEG jobs of one context, ONE launch per kernel; d_desc: room for nseg descriptors, a different one for late than
// the one the chain may still be reading)
void zkm_boot_early(zkm_ctx* c, zkm_boot_job* j, size_t nseg, zkm_boot_seg* d_desc);   // needs flags, mem
void zkm_boot_chain(zkm_ctx* c, zkm_boot_job* j, size_t nseg, const zkm_boot_seg* d_desc, hipStream_t st);   // needs po_in; early's descriptors
void zkm_boot_late(zkm_ctx* c, zkm_boot_job* j, size_t nseg, zkm_boot_seg* d_desc);    // needs po_ts, cpu, ps
std::string zkm_boot_refusal_early(const zkm_boot_job& j, const uint64_t flags[4]);    // "" or the message (flags 0, 1: known after early)
std::string zkm_boot_refusal_late(const zkm_boot_job& j, const uint64_t flags[4]);     // flags 2, 3: known after late

// ---- cpu_steps.hip: CPU rows and the operations they push from the compact step log.  The host walk makes every refusal (throws the
// bare message, "step <i>: ..."), counts the three lists and gives the base of each workgroup of ZKM_CPU_STEPS_BLOCK steps in them (three
// words a workgroup; `base` may be null); one descriptor per segment for the launch.
struct zkm_steps_counts_t { size_t mem = 0, logic = 0, arith = 0; };
void zkm_cpu_steps_walk(const zkm_cpu_steps* steps, zkm_steps_counts_t* n, std::vector<uint32_t>* base);
struct zkm_steps_seg {
    const zkm_cpu_step* steps;   // device
    const uint32_t* base;        // device: the walk's base triples
    const uint64_t* raw;         // device: the ready-made rows of the RAW steps
    size_t nsteps, n, row0;      // step i is row row0 + i of the n-row column-major table at `out` ...
    uint64_t clock0;             // ... with clock clock0 + i
    gl_t* out;                   // (rows = false: unused)
    uint64_t* mem;               // where the steps' first operation of each list goes (a null list is not written; lists = false: unused)
    uint32_t *logic, *arith;
};
// nseg <= ZKM_MAX_SEG segments of one context, ONE launch: the rows (over a zeroed table), the lists, or both
void zkm_cpu_steps_launch(zkm_ctx* c, const zkm_steps_seg* segs, size_t nseg, bool rows, bool lists);
// the text of a step's refusal ("step <i>: ..."): `code` is zkm_step's (cpu_steps_dev.h), `used` the channels a RAW row uses (BAD_MASK)
std::string zkm_cpu_step_refusal(size_t i, const zkm_cpu_step& t, size_t nraw, int code, uint32_t used);

// ---- cpu_steps_walk.hip: the same walk on the device, for steps staged ahead of a call (zkm_cpu_steps_stage).  What the builder
// (segment_ops.hip) needs of a segment whose `steps` pointer a staged handle owns: the handle's context, what the segment was staged
// with, the walk's counts and base triples, its refusal ("" when it passed) and the events every reader of the block is ordered behind.
// zkm_staged_steps_find waits on the host for the handle's events the first time anyone asks (zkm_staged_steps_get has, as a rule).
struct zkm_staged_steps_ref {
    zkm_ctx* ctx = nullptr;
    zkm_cpu_steps dev{};           // steps and raw_rows in device memory, as zkm_staged_steps_get hands them out
    zkm_steps_counts_t n;
    const uint32_t* base = nullptr;   // device
    std::string refusal;
    hipEvent_t done[2] = {nullptr, nullptr};
};
bool zkm_staged_steps_find(const void* d_steps, zkm_staged_steps_ref* out);
// The body of zkm_cpu_steps_stage behind its refusals (throws): the copies, the walk and the verdicts' download queued on the two copy
// streams, the handle registered.  own_steps: the records are copied into the handle's block wherever they lie; false: records in device
// memory are walked IN PLACE and handed out as they came (calls_stage.hip: the list it has patched on the device, queued on the first
// copy stream in front of this call -- the caller keeps that list alive for as long as the handle).  zkm_staged_steps_at: what
// zkm_staged_steps_find gives, for segment s of a handle the caller holds (a segment without steps is in no registry).
// zkm_staged_steps_join: the compute stream behind the handle's fence, once (what zkm_staged_steps_get does for a good segment).
struct zkm_staged_steps;
zkm_staged_steps* zkm_steps_stage_queue(zkm_ctx* c, size_t nseg, const zkm_cpu_steps* steps, bool own_steps);
void zkm_staged_steps_at(zkm_staged_steps* h, size_t s, zkm_staged_steps_ref* out);
void zkm_staged_steps_join(zkm_staged_steps* h);

// ---- the calls' expansions (sha_calls.hip, keccak_calls.hip, io_calls.hip, insn_rows.hip): K segments served by ONE launch a kind.
// A job is one segment's calls of one kind: the caller's lists (host or device memory as the kind's entry point says), where the
// outputs go (device) and what the host walk found.
//   check    the ONE statement of the kind's refusals about its lists (throws the bare message; the kind's own entry point and
//            calls_entry.hip both call it), the counts and the host walk's vectors
//   scratch  the bytes a launch of these jobs puts up: the K descriptors and the lists the host holds (zkm_calls_layout)
//   launch   queues the uploads into `scratch` and ONE launch for nseg <= ZKM_MAX_SEG checked jobs (zkm_calls_queue).  The SHA and
//            Keccak kernels store only the cells a row sets: zero_rows queues a memset of each job's rows in front (false: the caller
//            has zeroed them).  `stream`: where everything is queued; null is the context's compute stream (a staged call passes a copy
//            stream: calls_stage.hip).
// scratch and launch are the kinds' instantiations of the one launcher in calls_launch.h, where the block's layout and what is in use
// until the stream has been waited for are stated.  The per-kind entry points are the nseg = 1 case (zkm_calls_one).
struct zkm_calls_hold;   // the descriptors' host copy (calls_launch.h)
struct zkm_sha_job {
    const uint32_t* w16 = nullptr; const uint64_t* emeta = nullptr; size_t E = 0;
    const uint32_t *hx = nullptr, *w = nullptr; const uint64_t* cmeta = nullptr; size_t C = 0;
    uint64_t *rows = nullptr, *mem = nullptr, *ext_ts = nullptr;
    uint32_t *logic = nullptr, *ext_in = nullptr;
    size_t nrows = 0, nmem = 0, nlogic = 0, next = 0;
};
void zkm_sha_calls_check(zkm_sha_job& j);
size_t zkm_sha_calls_scratch(const zkm_sha_job* j, size_t nseg);
void zkm_sha_calls_launch(zkm_ctx* c, const zkm_sha_job* j, size_t nseg, char* scratch, zkm_calls_hold& hold, bool zero_rows, hipStream_t stream = nullptr);
struct zkm_keccak_base { uint64_t row, mem, logic, perm; };   // where a call starts in each list: the sums of the earlier calls' counts
struct zkm_keccak_job {
    const uint8_t* inputs = nullptr; const uint64_t *off = nullptr, *meta = nullptr, *digest_addrs = nullptr; size_t n = 0;
    uint64_t *rows = nullptr, *mem = nullptr, *perm_in = nullptr, *perm_ts = nullptr;
    uint32_t* logic = nullptr;
    size_t nrows = 0, nmem = 0, nlogic = 0, nperm = 0;
    std::vector<zkm_keccak_base> bases;
    std::vector<uint64_t> off_up;   // the offsets as they go up: from the first call's on, where the bytes go up
};
void zkm_keccak_calls_check(zkm_keccak_job& j);
size_t zkm_keccak_calls_scratch(const zkm_keccak_job* j, size_t nseg);
void zkm_keccak_calls_launch(zkm_ctx* c, const zkm_keccak_job* j, size_t nseg, char* scratch, zkm_calls_hold& hold, bool zero_rows, hipStream_t stream = nullptr);
struct zkm_io_job {
    const uint32_t* kinds = nullptr; const uint8_t* data = nullptr; const uint64_t *off = nullptr, *meta = nullptr; size_t n = 0;
    uint64_t* rows = nullptr;
    size_t nrows = 0, nmem = 0;
    std::vector<uint64_t> row_off, off_up;
};
void zkm_io_calls_check(zkm_io_job& j);
size_t zkm_io_calls_scratch(const zkm_io_job* j, size_t nseg);
void zkm_io_calls_launch(zkm_ctx* c, const zkm_io_job* j, size_t nseg, char* scratch, zkm_calls_hold& hold, hipStream_t stream = nullptr);
struct zkm_insn_job {
    const zkm_cpu_step* insns = nullptr; const uint64_t* clocks = nullptr; size_t n = 0;
    uint64_t* rows = nullptr;
    uint32_t* arith = nullptr;
    size_t nmem = 0, narith = 0;
    std::vector<uint32_t> base;     // one per workgroup: the operations the records in front of it push
};
void zkm_insn_rows_check(zkm_insn_job& j);
size_t zkm_insn_rows_scratch(const zkm_insn_job* j, size_t nseg);
void zkm_insn_rows_launch(zkm_ctx* c, const zkm_insn_job* j, size_t nseg, char* scratch, zkm_calls_hold& hold, hipStream_t stream = nullptr);

// ---- the three witness checks (witness_check.hip, lookup_check.hip, ctl_check.hip), each in two parts so that segment_check.hip can put
// them behind ONE pair of host waits: a part that QUEUES its launches on the context's stream into result words the caller names, and a
// part that READS those words once they are on the host.  A table of a check: registry id, column-major trace, height.
struct zkm_check_table {
    int id;
    const uint64_t* trace;
    unsigned log_n;
};
// the table's trace on the device: in place, or a copy of host memory queued on the stream and owned by `copies`
inline const uint64_t* zkm_check_table_on_device(zkm_ctx* c, const zkm_check_table& t, std::vector<zkm_scratch>& copies) {
    if (zkm_is_device_ptr(t.trace)) return t.trace;
    const size_t bytes = (zkm_table(t.id)->width << t.log_n) * sizeof(gl_t);
    copies.emplace_back(c, bytes);
    ZKM_HIP_CHECK(hipMemcpyAsync(copies.back().p, t.trace, bytes, hipMemcpyHostToDevice, c->stream));
    return copies.back().as<uint64_t>();
}
// witness_check.hip: ntab tables (device memory, any segments' in any order), d_find = ntab x ZKM_WITNESS_FINDING_WORDS device words; per
// table kind one `rows` and one `name` launch per ZKM_MAX_SEG tables of that kind.  read: the first table with a failing row (ntab: none)
// and its message
void zkm_witness_check_queue(zkm_ctx* c, const zkm_check_table* tabs, size_t ntab, uint64_t* d_find);
size_t zkm_witness_check_read(const char* what, const zkm_check_table* tabs, size_t ntab, const uint64_t* findings, std::string* msg);
// lookup_check.hip: one job per (table, lookup) of the ntab tables (device memory), every launch serves ZKM_MAX_SEG jobs; d_out =
// zkm_lookup_check_jobs x ZKM_LOOKUP_FINDING_WORDS device words (none queued when there is no job).  `queued` owns the jobs' scratch until
// the stream has been waited for.  read: findings = ntab x ZKM_LOOKUP_FINDING_WORDS (every table's own result) from the downloaded job
// words; the first table with a failing lookup (ntab: none) and its message
struct zkm_lookup_queued {
    std::vector<zkm_scratch> store;
    std::vector<size_t> job_table;   // the table of each job
};
size_t zkm_lookup_check_jobs(const zkm_check_table* tabs, size_t ntab);
void zkm_lookup_check_queue(zkm_ctx* c, const zkm_check_table* tabs, size_t ntab, uint64_t* d_out, zkm_lookup_queued* queued);
size_t zkm_lookup_check_read(const zkm_check_table* tabs, size_t ntab, const zkm_lookup_queued& queued, const uint64_t* job_words, uint64_t* findings,
                             std::string* msg);
// ctl_check.hip: check_ctls on the tables of nseg segments (tables[s]: ntables inputs) in ONE set of launches: nseg x nctls jobs over one
// descriptor block, ZKM_MAX_SEG jobs a launch; one download for the record counts, one per attempt for the verdicts, one for the reports
// of all failing segments.  reps[s] / msgs[s]: segment s's report and the reference's message (kind 0: consistent, message empty);
// attempts and host_waits are the CALL's in every report.  `ride` (may be null): a download of the caller's that travels with the FIRST
// attempt's verdicts -- the words of checks queued in front of this call cost no wait of their own.  Returns the lowest failing segment
// (nseg: none); throws when the check cannot be made
size_t zkm_check_ctls_run_segments(zkm_ctx* c, size_t nseg, const zkm_table_input* const* tables, size_t ntables, const zkm_cross_table_lookup* ctls,
                                   const zkm_ctl_side* sides, size_t nctls, zkm_ctl_report* reps, std::string* msgs, const zkm_ctx::xfer* ride = nullptr);
// ... on one segment's tables.  Returns the report's kind (0 consistent, 1 non-binary filter, 2 multisets differ) with the reference's
// message in *msg; throws when the check cannot be made
int zkm_check_ctls_run(zkm_ctx* c, const zkm_table_input* tables, size_t ntables, const zkm_cross_table_lookup* ctls, const zkm_ctl_side* sides,
                       size_t nctls, zkm_ctl_report* rep, std::string* msg);
// segment_check.hip: the three checks on nseg AllStark segments behind two host waits (the body of zkm_segments_check).  tables[s]: the
// twelve inputs in Table::all() order, `trace` set (host or device).  Outputs as zkm_segments_check's (any may be null).  Returns the lowest
// segment with a finding (nseg: none) and its message; throws when the check cannot be made
size_t zkm_segments_check_run(zkm_ctx* c, size_t nseg, const zkm_table_input* const* tables, uint64_t* verdicts, uint64_t* witness_findings,
                              uint64_t* lookup_findings, zkm_ctl_report* ctl_reports, std::string* msg);
// ---- the verifier (verify.hip; the constraint evaluation on the line through the opening lives beside k_quotient in stark.hip)
// per-table CtlZData lists in cross_table_lookup_data order (ctl.hip): the prover's derivation, which the verifier replays
struct table_zs {
    std::vector<zkm_ctl_z> zs;
    std::vector<uint32_t> ids;
    size_t naux = 0;
};
std::vector<table_zs> zkm_derive_zs(size_t ntables, const zkm_cross_table_lookup* ctls, const zkm_ctl_side* sides, size_t nctls, size_t nch,
                                    const uint64_t* challenges);
void zkm_all_stark_table_inputs(zkm_table_input out[ZKM_NUM_TABLES]);   // ctl.hip: the twelve tables of the built-in AllStark (no traces, log_n 0)
// One (segment, table) of a verify call as the kernels see it: where its blob lies in the call's device block, the blob's validated
// description (proof_blob.h: every offset follows from it), and what the transcript replay gave.
#define ZKM_VERIFY_LINE_POINTS 5      // constraints are evaluated on the rows v0 + t v1, t = 0 .. 4 (degree <= 3, one point to spare)
#define ZKM_VERIFY_LINE_THREADS (4 * ZKM_VERIFY_LINE_POINTS)
// What the Merkle chains and the reduction know of one entry of a verify call, a (segment, table) of zkm_verify_* or a claim of
// zkm_fri_verify alike: where the blob and the caps of its initial trees lie in the call's device block, the blob's FRI part
// (proof_blob.h: noracles initial trees and L layer trees, every offset follows from it) and the entry's query indices and verdicts.
// A query has noracles + 2 L + 1 verdict words, in the order of the findings: the initial trees' Merkle paths, per layer the evaluation
// check then the Merkle path, the final polynomial.  The STARK blob is the case of three initial trees whose caps lie in the blob.
struct zkm_verify_chains {
    uint64_t blob;                    // word offset of the blob
    uint64_t caps;                    // word offset of initial tree 0's cap; tree k's lies k * fri.cap_words further
    zkm_fri_part fri;
    uint32_t xs, verdicts;            // first of its fri.nq query indices / of its fri.nq * slots() verdict words
    GL_HD uint32_t trees() const { return (uint32_t)(fri.round.noracles + fri.round.L); }
    GL_HD uint32_t slots() const { return (uint32_t)(fri.round.noracles + 2 * fri.round.L + 1); }
    GL_HD uint32_t slot_layer_eval(uint32_t l) const { return (uint32_t)fri.round.noracles + 2 * l; }
    GL_HD uint32_t slot_final() const { return slot_layer_eval((uint32_t)fri.round.L); }
};
struct zkm_verify_table {
    uint64_t blob;                    // word offset of the blob
    uint64_t rows;                    // word offset of its line rows: [t][column][local, next], trace columns then auxiliary columns
    zkm_blob_desc d;
    uint32_t slots, xs, verdicts;     // verdict words per query = 4 + 2 L; first of its nq query indices / of its nq * slots verdict words
    gl_t zeta[2], zeta_next[2], fri_alpha[2], apow_wa[2], apow_z[2], red_open[3][2], betas[ZKM_FRI_HEADER_LAYERS][2];
};
// stark.hip: all constraints of `table_id` on the line rows of nseg <= ZKM_MAX_SEG (segment, table) entries, ONE launch; entry s reads
// d_rows + rows_off[s] and writes its 20 x 2 accumulators (thread = 4 t + setting, then challenge) to d_acc + acc_off[s].  `own` holds
// nseg lists of CtlZData (device pointers) for `naux` CTL columns; alphas / lookup_challenges: nseg x nalphas
struct ctl_dev;
void zkm_verify_line_constraints(zkm_ctx* c, int table_id, size_t nalphas, const ctl_dev& own, size_t naux, const uint64_t* lookup_challenges,
                                 const gl_t* alphas, const gl_t* d_rows, const uint64_t* rows_off, gl_t* d_acc, const uint64_t* acc_off,
                                 size_t W, size_t A, size_t nseg);
// verify.hip: verify_proof on nseg segments' blobs in ONE set of launches (the body of zkm_verify_segments; the prove drivers call it
// under "verify"): tables[s] = segment s's table list, proofs[s] / proof_words[s] its blobs, challenges[s] the claimed CTL challenges.
// Returns the index of the first rejected segment (its report's message in *msg) or nseg when all are accepted; throws when the check
// cannot be made
size_t zkm_verify_run(zkm_ctx* c, const zkm_stark_config* cfg, size_t nseg, const zkm_table_input* const* tables, size_t ntables,
                      const zkm_cross_table_lookup* ctls, const zkm_ctl_side* sides, size_t nctls, const uint64_t* const* pub, const size_t* npub,
                      const uint64_t* const* proofs, const size_t* proof_words, const uint64_t* const* challenges, std::string* msg);
// ctl.hip: the body of zkm_prove_segments[_columns] (exactly one of traces / columns non-null); seg_base = position of segment 0 in the
// caller's larger call (csrc/pool.hip deals groups of one pool call to its workers) -- used in error messages only
extern "C" int zkm_prove_segments_entry(const char* what, zkm_ctx* c, const zkm_stark_config* cfg, size_t nseg, const uint64_t* const* const* traces,
                                        const uint64_t* const* const* const* columns, const unsigned* const* log_n, const uint64_t* const* pub,
                                        const size_t* npub, uint64_t* const* proofs, uint64_t* const* challenges, char** err, size_t seg_base);
double zkm_segment_footprint(const zkm_stark_config* cfg, const unsigned log_n[ZKM_NUM_TABLES]);   // ctl.hip: estimated bytes of one segment in a proving wave
// segment_ops.hip: the body of zkm_prove_segments_ops, seg_base as above (the pool's workers)
extern "C" int zkm_prove_segments_ops_entry(const char* what, zkm_ctx* c, const zkm_stark_config* cfg, size_t nseg, const zkm_segment_ops* ops,
                                            const uint64_t* const* pub, const size_t* npub, uint64_t* const* proofs, size_t* offsets_out,
                                            uint64_t* const* challenges, char** err, size_t seg_base);
// The pool's workers for a segment as the emulator records it (zkm_pool_prove_segments_calls), seg_base as above.  C++ linkage: these
// are no part of the library's exported names.
// segment_ops.hip: the body of zkm_prove_segments_ops_steps with a context (images: or null)
int zkm_prove_segments_ops_steps_entry(const char* what, zkm_ctx* c, const zkm_stark_config* cfg, size_t nseg, const zkm_boot_image* images,
                                       const zkm_cpu_steps* steps, const zkm_segment_ops* ops, const uint64_t* const* pub, const size_t* npub,
                                       uint64_t* const* proofs, size_t* offsets_out, uint64_t* const* challenges, char** err, size_t seg_base);
// calls_entry.hip: the body of zkm_prove_segments_ops_calls
int zkm_prove_segments_ops_calls_entry(const char* what, zkm_ctx* c, const zkm_stark_config* cfg, size_t nseg, const zkm_boot_image* images,
                                       const struct zkm_segment_calls* calls, const uint64_t* const* pub, const size_t* npub,
                                       uint64_t* const* proofs, size_t* offsets_out, uint64_t* const* challenges, char** err, size_t seg_base);
// calls_stage.hip: the bodies of zkm_segments_calls_stage and zkm_staged_calls_get, under their own names; a refusal names segment
// seg_base + s
int zkm_segments_calls_stage_entry(zkm_ctx* c, size_t nseg, const struct zkm_segment_calls* calls, const zkm_boot_image* images, void** out,
                                   char** err, size_t seg_base);
int zkm_staged_calls_get_entry(void* staged, size_t segment, zkm_cpu_steps* steps_out, zkm_segment_ops* ops_out, zkm_boot_image* image_out,
                               char** err, size_t seg_base);
