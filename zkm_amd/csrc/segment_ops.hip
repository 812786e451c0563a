// segment_ops.hip -- whole segments' twelve tables built on the device from their raw operations (the reference's Traces::into_tables,
// witness/traces.rs:230-320), and the proofs of those segments in the same call.
//
//   zkm_segments_tables      K segments: every height (Table::all() order), ONE output block per segment from the context's allocator,
//                            every table written into it, each handed out as a segment-shaped zkm_staged;
//   zkm_prove_segments_ops   zkm_segments_tables, zkm_prove_segments on the blocks (lock-step), the blocks freed; in waves when the
//                            call holds more than ZKM_MAX_SEG segments or more than the memory budget;
//   zkm_segment_tables, zkm_prove_segment_ops   the one-segment forms (the same builder, K = 1; zkm_prove_segment proves);
//   zkm_segment_ops_stage    a segment's lists uploaded behind the work in flight, for a later call of the above;
//   zkm_*_boot               the same calls with each segment's bootstrap kernel built from its image (bootstrap.hip) in front of the
//                            caller's lists: the boot's rows are the first of the CPU, Poseidon and PoseidonSponge tables and its
//                            memory operations the first of the joined list.  Its sponge chains run on the context's side stream
//                            beside the Memory, Arithmetic and Logic tables; its flags ride on waits (1) and (3).
//   zkm_*_steps              the same calls with each segment's CPU rows built from its compact step log (cpu_steps.hip) behind the
//                            bootstrap's rows: the steps' memory, logic and arithmetic operations are written into the joined lists
//                            in the early phase (Memory and Arithmetic are sized on them), the rows into the zeroed table once the
//                            output block exists.  No host wait is added; k_cpu_rows_to_cols is not launched for such a segment.
//
// The one kernel here, k_cpu_rows_to_cols, turns the emulator's CPU rows (Vec<CpuColumnsView<F>>: 259 words a row, row-major) into the
// column-major table of trace_rows_to_poly_values (util.rs:37-46), canonical.  Every other table comes from its existing launcher;
// every launcher serves the K segments of a wave with ONE launch per kernel (the segment is blockIdx.z), and the Memory and
// Arithmetic witnesses run in phases (zkm_internal.h zkm_memory_job / zkm_arith_job) so that they share host waits.
//
// Host waits per wave, whatever K, each ONE download of the wave's sync words (16 per segment, zkm_ctx::download):
//   (1) the Memory key widths, with the Arithmetic row counts and validation flags;
//   (2) the Memory row counts after the sort and the gap scan: every height is then known, and the output blocks are allocated;
//   (3) the validation flags of every writer (Logic op codes, Memory range checks, Arithmetic shared-column values), a triple a segment.
// Sizing mode ends after (2).  Inputs in host memory go through one staging block for the wave; CPU rows in host memory are copied in
// row pieces on the context's two copy streams, each piece transposed on the compute stream behind its own copy, so that the largest
// transfer overlaps the other tables' generation.
#include <algorithm>
#include <cmath>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "zkm_internal.h"

extern "C" zkm_staged* zkm_staged_from_segment(zkm_ctx* c, void* block, const size_t off[ZKM_NUM_TABLES + 1]);   // core.hip

namespace {

constexpr int CPU_W = ZKM_CPU_COLS;        // 259 words a row
constexpr int TR_ROWS = 32;                // rows per tile
constexpr int TR_THREADS = 256;
constexpr unsigned SEG_MAX_LOG_N = 28;     // every table, as ZKM_MEMORY_MAX_LOG_N / ZKM_ARITHMETIC_MAX_LOG_N

// ---- CPU rows -> columns.  A workgroup stages TR_ROWS consecutive rows -- one contiguous run of TR_ROWS x 2072 B -- in LDS at their own
// stride with 16-byte loads, then writes them column by column: lanes 0..31 of a wave take column c, lanes 32..63 column c + 1, so every
// store instruction is two runs of 256 B down two columns.  The tile needs no padding: a row is 518 dwords, so lane l of a ds_read_b64
// down a column reads bank (518 l + 2 c) mod 64 = (6 l + 2 c) mod 64, a different pair of banks for each of the 32 lanes of a group.
// 66,304 B of LDS: two workgroups per CU.  Words >= p are reduced on the way (GoldilocksField words may be non-canonical).
// One launch serves K segments (zkm_seg_args): rows [0, nrows) at `rows` become rows [row0, row0 + nrows) of the n-row table at `out`.
struct cpu_seg {
    const uint64_t* rows;
    size_t nrows, row0, n;
    gl_t* out;
};
__global__ __launch_bounds__(TR_THREADS) void k_cpu_rows_to_cols(zkm_seg_args<cpu_seg> S) {
    __shared__ __attribute__((aligned(16))) uint64_t t[TR_ROWS * CPU_W];
    const cpu_seg& A = S.v[blockIdx.z];
    const size_t nrows = A.nrows, n = A.n;
    const size_t pr = (size_t)blockIdx.x * TR_ROWS;
    if (pr >= nrows) return;
    const unsigned here = (unsigned)(nrows - pr < (size_t)TR_ROWS ? nrows - pr : TR_ROWS);
    const uint64_t* src = A.rows + pr * CPU_W;
    const unsigned nw = here * CPU_W;
    if (here == TR_ROWS && (((uintptr_t)src) & 15) == 0) {
        // a full tile: every load in flight before the first LDS store (17 x 16 B per lane)
        constexpr unsigned NV = TR_ROWS * CPU_W / 2, PER = NV / TR_THREADS;
        const uint4* s4 = (const uint4*)src;
        uint4* t4 = (uint4*)t;
        const bool tail = threadIdx.x < NV - PER * TR_THREADS;
        uint4 v[PER], w = {};
#pragma unroll
        for (unsigned k = 0; k < PER; k++) v[k] = s4[k * TR_THREADS + threadIdx.x];
        if (tail) w = s4[PER * TR_THREADS + threadIdx.x];
#pragma unroll
        for (unsigned k = 0; k < PER; k++) t4[k * TR_THREADS + threadIdx.x] = v[k];
        if (tail) t4[PER * TR_THREADS + threadIdx.x] = w;
    } else if ((((uintptr_t)src) & 15) == 0) {
        const uint4* s4 = (const uint4*)src;
        uint4* t4 = (uint4*)t;
        for (unsigned i = threadIdx.x; i < nw / 2; i += TR_THREADS) t4[i] = s4[i];
        if ((nw & 1) && threadIdx.x == 0) t[nw - 1] = src[nw - 1];
    } else {
        for (unsigned i = threadIdx.x; i < nw; i += TR_THREADS) t[i] = src[i];
    }
    __syncthreads();
    const unsigned lane = threadIdx.x & 63, r = lane & 31;
    if (r >= here) return;
    gl_t* o = A.out + A.row0 + pr + r;
#pragma unroll 4
    for (unsigned c = 2 * (threadIdx.x >> 6) + (lane >> 5); c < (unsigned)CPU_W; c += 2 * (TR_THREADS / 64)) {
        const uint64_t v = t[r * CPU_W + c];
        o[(size_t)c * n] = v >= GL_P ? v - GL_P : v;
    }
}

void launch_cpu_rows_to_cols(zkm_ctx* c, const cpu_seg* segs, size_t nseg) {
    size_t max_rows = 0;
    for (size_t s = 0; s < nseg; s++) max_rows = std::max(max_rows, segs[s].nrows);
    zkm_prof_scope ps(c, "segment_ops/cpu_rows_to_cols");
    zkm_launch_segs(c->stream, k_cpu_rows_to_cols, segs, nseg, (max_rows + TR_ROWS - 1) / TR_ROWS, TR_THREADS);
}

// names for positions in Table::all() (tables.h: zkm_table_at)
enum { AR, CPU, PO, PS, KK, KS, SE, SES, SC, SCS, LO, ME, NTAB };
static_assert(NTAB == ZKM_NUM_TABLES && zkm_table_at(ME)->id == ZKM_TABLE_MEMORY, "the positions are the registry's");

unsigned log2_of(size_t pow2) { return pow2 ? 63 - __builtin_clzll(pow2) : 0; }
size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }

// the output of one build: the block (empty in sizing mode), the word offset of each table in it, and the heights
struct segment_block {
    zkm_scratch block;
    size_t off[NTAB + 1] = {};
    unsigned lg[NTAB] = {};
};

// ---- lists staged ahead of a call (zkm_segment_ops_stage): the block of each handle alive in this process and the context it belongs
// to.  A build handed such a block's pointers on another context is refused -- nothing would order that context behind the upload.
std::mutex g_staged_mu;
std::map<const void*, const zkm_ctx*> g_staged_ops;   // block -> its context
const zkm_ctx* staged_ops_context(const void* p) {
    std::lock_guard<std::mutex> lk(g_staged_mu);
    const auto it = g_staged_ops.find(p);
    return it == g_staged_ops.end() ? nullptr : it->second;
}

// one list of a zkm_segment_ops: the address of its pointer field (fields differ in type: read and written as bytes) and its size
struct list_ref {
    void* field;
    size_t bytes;
    bool sizing;   // read before the heights are known (Arithmetic, Memory)
    const void* get() const {
        const void* p;
        memcpy(&p, field, sizeof p);
        return p;
    }
    void set(const void* p) const { memcpy(field, &p, sizeof p); }
};
// Where the lists of a data-parallel writer (tables.h zkm_writer, in its order) lie in a zkm_segment_ops: the count, the pointers and,
// for a sponge, its host offsets.  In the order the lists take in a staging block.
struct ops_fields {
    int t;
    size_t count, list[3], off;
    size_t k(const zkm_segment_ops& o) const { return *(const size_t*)((const char*)&o + count); }
    const void* ptr(const zkm_segment_ops& o, size_t field) const {
        const void* p;
        memcpy(&p, (const char*)&o + field, sizeof p);
        return p;
    }
    // bytes of list i (a sponge's byte list: where its last operation ends -- the offsets are host memory, builder::sponge_rows checks it)
    size_t bytes(const zkm_segment_ops& o, uint32_t i) const {
        const uint32_t per = zkm_table_at(t)->writer.list_bytes[i];
        return per ? k(o) * per : k(o) ? ((const uint64_t*)ptr(o, off))[k(o)] : 0;
    }
};
#define F(m) offsetof(zkm_segment_ops, m)
const ops_fields FIELDS[] = {
    {LO, F(nlogic), {F(logic_ops)}},
    {PO, F(nposeidon), {F(poseidon_inputs), F(poseidon_timestamps)}},
    {PS, F(nposeidon_sponge), {F(poseidon_sponge_inputs), F(poseidon_sponge_meta)}, F(poseidon_sponge_off)},
    {KK, F(nkeccak), {F(keccak_inputs), F(keccak_timestamps)}},
    {KS, F(nkeccak_sponge), {F(keccak_sponge_inputs), F(keccak_sponge_meta)}, F(keccak_sponge_off)},
    {SE, F(nsha_extend), {F(sha_extend_inputs), F(sha_extend_timestamps)}},
    {SES, F(nsha_extend_sponge), {F(sha_extend_sponge_w16), F(sha_extend_sponge_meta)}},
    {SC, F(nsha_compress), {F(sha_compress_hx), F(sha_compress_w), F(sha_compress_meta)}},
    {SCS, F(nsha_compress_sponge), {F(sha_compress_sponge_hx), F(sha_compress_sponge_w), F(sha_compress_sponge_meta)}},
};
#undef F
const ops_fields& fields_of(int t) {
    for (const ops_fields& f : FIELDS)
        if (f.t == t) return f;
    throw std::runtime_error("segment_ops: no data-parallel writer for table " + std::string(zkm_table_at(t)->name));
}

// every list of `o` except the CPU rows and the two sponge offset arrays (which stay host memory)
std::vector<list_ref> lists_of(zkm_segment_ops& o) {
    std::vector<list_ref> ls = {{&o.arithmetic_ops, o.narithmetic * 12, true}, {&o.memory_ops, o.nmemory * 48, true}};
    for (const ops_fields& f : FIELDS)
        for (uint32_t i = 0; i < zkm_table_at(f.t)->writer.nlists; i++) ls.push_back({(char*)&o + f.list[i], f.bytes(o, i), false});
    return ls;
}

// One segment of a wave.  The phases below are driven for the K builders of a wave side by side (build_wave), so that every launch and
// every host wait serves all of them.
struct builder {
    std::string what;             // "<entry point>", or "<entry point>: segment <position in the call>" in a call of several
    zkm_ctx* c;
    const zkm_segment_ops* o;     // the caller's lists
    const zkm_boot_image* im;     // the image whose bootstrap goes in front of them, or null
    zkm_boot_counts_t bn{};       // ... and what it adds to each list (zeros without an image)
    const zkm_cpu_steps* st;      // the step log the CPU rows are built from (behind the bootstrap's, in place of the caller's), or null
    zkm_steps_counts_t sn{};      // ... and what it adds to the Memory, Logic and Arithmetic lists, behind the bootstrap's part
    std::vector<uint32_t> step_base;   // ... where each workgroup of steps starts in them (cpu_steps.hip)
    const void *d_steps = nullptr, *d_step_base = nullptr, *d_raw = nullptr;   // device copies of the steps, the bases and the RAW rows
    zkm_staged_steps_ref staged;  // steps a zkm_cpu_steps_stage handle owns (staged.ctx != null): walked on the device, nothing of them goes up
    zkm_segment_ops d{};          // ... and where the device reads them: the caller's device pointers, or places in the staging block
    unsigned lg[NTAB] = {};
    std::vector<uint64_t> ps_row, ks_row;   // first row of each sponge operation
    size_t ps_rows = 0, ks_rows = 0;
    const void *d_pso = nullptr, *d_psr = nullptr, *d_kso = nullptr, *d_ksr = nullptr;   // device copies of the offsets and the row offsets
    std::string me_what, ar_what;
    // staging
    struct upload { list_ref dst; const void* src; size_t off, skip; };   // skip: bytes of the bootstrap's part in front (joined lists)
    std::vector<upload> ups;
    bool cpu_host = false;
    size_t cpu_off = 0, piece_rows = 0;
    std::vector<zkm_event> piece_done;

    builder(const char* entry, zkm_ctx* ctx, const zkm_segment_ops* ops, size_t pos, bool label, const zkm_boot_image* image = nullptr,
            const zkm_cpu_steps* steps = nullptr)
        : what(label ? std::string(entry) + ": segment " + std::to_string(pos) : std::string(entry)), c(ctx), o(ops), im(image), st(steps) {}
    size_t nmemory() const { return bn.memory_ops + sn.mem + o->nmemory; }
    size_t nlogic() const { return sn.logic + o->nlogic; }
    size_t narithmetic() const { return sn.arith + o->narithmetic; }
    size_t nposeidon() const { return bn.poseidon + o->nposeidon; }
    size_t nsteps() const { return st ? st->nsteps : 0; }
    size_t ncpu_rows() const { return bn.cpu_rows + nsteps() + o->ncpu_rows; }

    [[noreturn]] void refuse(int t, const std::string& msg) const { throw std::runtime_error(what + ": " + zkm_table_at(t)->name + ": " + msg); }
    // a height of max(rows, min_rows) rounded up to a power of two; rows = count x per, refused above 2^SEG_MAX_LOG_N
    unsigned height(int t, size_t count, size_t per, size_t min_rows) const {
        const size_t cap = (size_t)1 << SEG_MAX_LOG_N;
        if (count > cap / per) refuse(t, "the operations need more than 2^" + std::to_string(SEG_MAX_LOG_N) + " rows");
        size_t h = 1;
        while (h < std::max(count * per, min_rows)) h <<= 1;
        return log2_of(h);
    }
    void need(int t, size_t count, std::initializer_list<const void*> ps) const {
        if (!count) return;
        for (const void* p : ps)
            if (!p) refuse(t, "null pointer with a nonzero count");
    }
    // rows of a sponge table: sum over the operations of len / rate + 1; the offsets must be host memory
    size_t sponge_rows(int t, const uint64_t* off, size_t nops, size_t rate, std::vector<uint64_t>& row_off) const {
        if (nops && zkm_is_device_ptr(off)) refuse(t, "the offsets must be host memory");
        row_off.assign(nops + 1, 0);
        const size_t cap = (size_t)1 << SEG_MAX_LOG_N;
        for (size_t i = 0; i < nops; i++) {
            if (off[i + 1] <= off[i]) refuse(t, "empty operation (base_address[0] is required)");
            const uint64_t len = off[i + 1] - off[i];
            if (len / rate + 1 > cap - row_off[i]) refuse(t, "the operations need more than 2^" + std::to_string(SEG_MAX_LOG_N) + " rows");
            row_off[i + 1] = row_off[i] + len / rate + 1;
        }
        return row_off[nops];
    }

    // ---- phase: every check that needs no device (zkm_segment_ops_stage runs it too).  This phase and heights() never use `c`: the
    // *_steps calls run both without a context (steps_without_context), so that the host's refusals can be made where there is no GPU
    void check_host() {
        const zkm_segment_ops& o = *this->o;
        need(CPU, o.ncpu_rows, {o.cpu_rows});
        need(AR, o.narithmetic, {o.arithmetic_ops});
        need(ME, o.nmemory, {o.memory_ops});
        for (const ops_fields& f : FIELDS) {   // (a sponge: the offsets here, the bytes once the offsets have been read)
            const zkm_writer& w = zkm_table_at(f.t)->writer;
            for (uint32_t i = 0; i < w.nlists; i++) need(f.t, f.k(o), {f.ptr(o, w.list_bytes[i] ? f.list[i] : f.off)});
        }
        if (im) {
            try {
                bn = zkm_boot_job(c, im).n;
            } catch (const std::exception& e) {
                refuse(CPU, std::string("bootstrap image: ") + e.what());
            }
        }
        if (st) {
            if (o.cpu_rows || o.ncpu_rows) refuse(CPU, "cpu_rows must be NULL with ncpu_rows 0: the steps take their place");
            if (st->nsteps && zkm_staged_steps_find(st->steps, &staged)) {
                // staged steps: the device has walked them; the handle knows the counts, the bases and the verdict
                if (staged.ctx != c) refuse(CPU, "the steps were staged on another context");
                if (st->nsteps != staged.dev.nsteps || st->raw_rows != staged.dev.raw_rows || st->nraw != staged.dev.nraw)
                    refuse(CPU, "staged steps are taken as zkm_staged_steps_get hands them out");
                if (!staged.refusal.empty()) refuse(CPU, staged.refusal);
                sn = staged.n;
            } else {
                staged = zkm_staged_steps_ref{};
                if (st->nsteps && st->steps && zkm_is_device_ptr(st->steps)) refuse(CPU, "steps in device memory that no staged handle owns");
                try {
                    zkm_cpu_steps_walk(st, &sn, &step_base);
                } catch (const std::exception& e) {
                    refuse(CPU, e.what());
                }
            }
        }
        const size_t rows = ncpu_rows();
        if ((st ? st->nsteps : o.ncpu_rows) == 0 || (rows & (rows - 1)) || rows > ((size_t)1 << SEG_MAX_LOG_N))
            refuse(CPU, std::to_string(rows) + " rows" + (im ? " (" + std::to_string(bn.cpu_rows) + " of the bootstrap)" : std::string()) +
                            ": not a power of two of at most 2^" + std::to_string(SEG_MAX_LOG_N));
        if (nmemory() == 0) refuse(ME, "No memory ops?");
        if (nmemory() >= ((size_t)1 << 32)) refuse(ME, "2^32 or more memory ops");
        if (narithmetic() >= ((size_t)1 << 31)) refuse(AR, "2^31 or more arithmetic ops");
        ps_rows = sponge_rows(PS, o.poseidon_sponge_off, o.nposeidon_sponge, 32, ps_row) + bn.poseidon;
        for (uint64_t& r : ps_row) r += bn.poseidon;      // the bootstrap's sponge rows come first
        ks_rows = sponge_rows(KS, o.keccak_sponge_off, o.nkeccak_sponge, 136, ks_row);
        need(PS, fields_of(PS).bytes(o, 0), {o.poseidon_sponge_inputs});
        need(KS, fields_of(KS).bytes(o, 0), {o.keccak_sponge_inputs});
        const zkm_ctx* owner = staged_ops_context(o.cpu_rows);
        if (owner && owner != c) refuse(CPU, "the lists were staged on another context");
    }
    // ---- phase: the heights the host knows (Arithmetic and Memory: the least they can be, for the memory estimate of a wave)
    void heights(const zkm_stark_config* cfg) {
        const zkm_segment_ops& o = *this->o;
        const size_t min_rows = std::max<size_t>((size_t)1 << cfg->cap_height, 64);   // max(num_cap_elements, MIN_TRACE_LEN), traces.rs:246-247
        for (const ops_fields& f : FIELDS) lg[f.t] = height(f.t, f.k(o), zkm_table_at(f.t)->writer.rows_per_op, min_rows);
        // ... except where the rows are not the caller's count: the sponges' lengths, the bootstrap's permutations in front
        lg[PO] = height(PO, nposeidon(), 1, min_rows);
        lg[PS] = height(PS, ps_rows, 1, min_rows);
        lg[KS] = height(KS, ks_rows, 1, min_rows);
        lg[LO] = height(LO, nlogic(), 1, min_rows);
        lg[AR] = height(AR, narithmetic(), 1, (size_t)1 << 16);
        lg[CPU] = log2_of(ncpu_rows());
        lg[ME] = height(ME, nmemory(), 1, 1);
    }
    // ---- phase: the segment's part of the staging block, from byte `base`: the CPU rows (host rows only), then every list in host memory.
    // Returns the bytes it takes.
    size_t plan(bool write, size_t base) {
        const zkm_segment_ops& o = *this->o;
        d = o;
        d_pso = d_psr = d_kso = d_ksr = d_steps = d_step_base = d_raw = nullptr;
        ups.clear();
        cpu_host = write && o.ncpu_rows && !zkm_is_device_ptr(o.cpu_rows);
        cpu_off = base;
        size_t at = base + align_up(cpu_host ? o.ncpu_rows * CPU_W * 8 : 0);
        auto add = [&](const list_ref& l, const void* src, size_t skip = 0) {
            if (!(l.bytes + skip) || (!write && !l.sizing)) return;
            ups.push_back(upload{l, src, at, skip});
            at += align_up(l.bytes + skip);
        };
        // the lists the bootstrap and the steps write the head of are joined in the staging block, wherever the caller's part lies
        for (const list_ref& l : lists_of(d)) {
            const size_t skip = l.field == (void*)&d.memory_ops ? (bn.memory_ops + sn.mem) * 48
                                : l.field == (void*)&d.arithmetic_ops ? sn.arith * 12
                                : l.field == (void*)&d.logic_ops ? sn.logic * 12
                                : l.field == (void*)&d.poseidon_inputs ? bn.poseidon * 96
                                : l.field == (void*)&d.poseidon_timestamps ? bn.poseidon * 8 : 0;
            if (skip || !zkm_is_device_ptr(l.get())) add(l, l.get(), skip);
        }
        // the steps, their workgroups' bases and the RAW rows that lie in host memory: read by the launch that sizes Memory and Arithmetic
        if (st && staged.ctx) {
            d_steps = st->steps;
            d_step_base = staged.base;
            d_raw = st->raw_rows;
        } else if (st) {
            add(list_ref{&d_steps, st->nsteps * sizeof(zkm_cpu_step), true}, st->steps);
            add(list_ref{&d_step_base, step_base.size() * 4, true}, step_base.data());
            d_raw = st->raw_rows;
            if (st->nraw && !zkm_is_device_ptr(st->raw_rows)) add(list_ref{&d_raw, st->nraw * CPU_W * 8, true}, st->raw_rows);
        }
        const size_t nps = o.nposeidon_sponge ? (o.nposeidon_sponge + 1) * 8 : 0, nks = o.nkeccak_sponge ? (o.nkeccak_sponge + 1) * 8 : 0;
        add(list_ref{&d_pso, nps, false}, o.poseidon_sponge_off);
        add(list_ref{&d_psr, nps, false}, ps_row.data());
        add(list_ref{&d_kso, nks, false}, o.keccak_sponge_off);
        add(list_ref{&d_ksr, nks, false}, ks_row.data());
        return at - base;
    }
    // ---- phase: the copies of the CPU rows in pieces of >= 8192 rows (17 MB), at most 16 of them, on alternate copy streams (`turn` runs
    // on through the segments of a wave), an event behind each
    void copy_cpu_rows(char* sb, size_t& turn) {
        const zkm_segment_ops& o = *this->o;
        piece_rows = o.ncpu_rows;
        if (!cpu_host) return;
        d.cpu_rows = (const uint64_t*)(sb + cpu_off);
        piece_rows = std::min<size_t>(o.ncpu_rows, std::max<size_t>(8192, o.ncpu_rows / 16));
        for (size_t r0 = 0; r0 < o.ncpu_rows; r0 += piece_rows, turn++) {
            const hipStream_t up = (turn & 1) ? c->copy_stream2 : c->copy_stream;
            const size_t here = std::min(piece_rows, o.ncpu_rows - r0);   // (behind a bootstrap the caller's rows are no power of two)
            ZKM_HIP_CHECK(hipMemcpyAsync((void*)(d.cpu_rows + r0 * CPU_W), o.cpu_rows + r0 * CPU_W, here * CPU_W * 8, hipMemcpyHostToDevice, up));
            piece_done.emplace_back(c);
            piece_done.back().record(up);
        }
    }
    // ---- phase: the uploads of the lists on the compute stream (sizing: the two that the heights need; then the others)
    void put(char* sb, bool sizing) {
        for (const upload& u : ups) {
            if (u.dst.sizing != sizing) continue;
            if (u.dst.bytes) ZKM_HIP_CHECK(hipMemcpyAsync(sb + u.off + u.skip, u.src, u.dst.bytes, u.skip ? hipMemcpyDefault : hipMemcpyHostToDevice, c->stream));
            u.dst.set(sb + u.off);
        }
    }
    // where a joined list will lie (put sets the same pointer when it queues the caller's part)
    void point_joined(char* sb) {
        for (const upload& u : ups)
            if (u.skip) u.dst.set(sb + u.off);
    }
    size_t n(int t) const { return (size_t)1 << lg[t]; }
    // the steps' descriptor: their operations lie behind the bootstrap's in the joined lists (`logic`: null where the list is not staged)
    zkm_steps_seg steps_seg(gl_t* cpu, bool logic) const {
        return zkm_steps_seg{(const zkm_cpu_step*)d_steps, (const uint32_t*)d_step_base, (const uint64_t*)d_raw, st->nsteps, n(CPU), bn.cpu_rows,
                             bn.cpu_rows, cpu, (uint64_t*)d.memory_ops + 6 * bn.memory_ops, logic ? (uint32_t*)d.logic_ops : nullptr,
                             (uint32_t*)d.arithmetic_ops};
    }
};

constexpr size_t SYNC_WORDS = 16;   // per segment: [0, 5) Memory key widths and >= p flag, [5] Memory last op with dummies, [6] Memory row count,
                                    // [7] Arithmetic rows, [8] Arithmetic flags, [9, 11) three 32-bit validation flags (Logic, Memory, Arithmetic),
                                    // [11, 15) the bootstrap's flags (zkm_boot_seg::flags)

// a failure while the sponge chains run on the side stream: they end before their blocks go back to the allocator
struct side_join {
    hipStream_t st = nullptr;
    ~side_join() {
        if (st) (void)hipStreamSynchronize(st);
    }
};

// K <= ZKM_MAX_SEG checked builders of one context, phase by phase: one staging block, three host waits, one launch per kernel.
// write = false: sizing only (the heights; the blocks stay empty).
std::vector<segment_block> build_wave(zkm_ctx* c, builder* b, size_t K, bool write) {
    // ---- the staging block: the sync words of every segment, then each segment's part
    size_t stage_bytes = align_up(K * SYNC_WORDS * 8), nboot = 0;
    for (size_t s = 0; s < K; s++) nboot += b[s].im != nullptr;
    const size_t desc_off = stage_bytes;     // the bootstraps' descriptors: one set for the early phase and the chains, one for the late phase
    stage_bytes += align_up(2 * nboot * sizeof(zkm_boot_seg));
    for (size_t s = 0; s < K; s++) stage_bytes += b[s].plan(write, stage_bytes);
    zkm_scratch stage(c, stage_bytes);
    char* sb = stage.as<char>();
    uint64_t* d_sync = (uint64_t*)sb;
    std::vector<uint64_t> sync(K * SYNC_WORDS);
    // staged steps: the compute stream goes behind their uploads and their walk before anything of this wave is queued (every other stream
    // of the call starts behind the compute stream; zkm_staged_steps_get has queued the same waits, as a rule)
    for (size_t s = 0; s < K; s++)
        for (const hipEvent_t e : b[s].staged.done)
            if (b[s].staged.ctx) ZKM_HIP_CHECK(hipStreamWaitEvent(c->stream, e, 0));
    // host rows go up on the copy streams, each piece with an event of its own: of the fence only the start and the guard, which stays
    // armed -- the copy streams are waited for before the staging block goes back, however the wave ends.  A wave of device-resident
    // rows leaves the copy streams alone
    zkm_copy_fence copies;
    bool any_host_rows = false;
    for (size_t s = 0; s < K; s++) any_host_rows = any_host_rows || b[s].cpu_host;
    if (any_host_rows) copies.begin(c);
    size_t turn = 0;
    for (size_t s = 0; s < K; s++) b[s].copy_cpu_rows(sb, turn);
    ZKM_HIP_CHECK(hipMemsetAsync(d_sync, 0, K * SYNC_WORDS * 8, c->stream));
    for (size_t s = 0; s < K; s++) b[s].put(sb, true);
    // ---- the bootstraps: every memory operation of theirs (Memory is sized on the joined list), then the sponge chains on the side
    // stream, joined before the writers that need the states
    std::vector<zkm_boot_job> bj;
    zkm_boot_seg* d_desc = (zkm_boot_seg*)(sb + desc_off);
    side_join side;
    zkm_event chains_done;
    bj.reserve(K);
    for (size_t s = 0; s < K; s++) {
        bj.emplace_back(c, b[s].im);
        if (b[s].im || b[s].st) b[s].point_joined(sb);
        if (!b[s].im) continue;
        bj[s].prepare();
        bj[s].d.flags = (unsigned long long*)(d_sync + s * SYNC_WORDS + 11);
        bj[s].d.mem = (uint64_t*)b[s].d.memory_ops;
        bj[s].d.po_in = write ? (uint64_t*)b[s].d.poseidon_inputs : nullptr;
    }
    zkm_boot_early(c, bj.data(), K, d_desc);
    if (nboot && write) {
        // (a profiled context keeps the chains on the compute stream: the scopes are event pairs on that stream, so "bootstrap/chain_*"
        // measures the chains only there, and the call then costs the serial sum -- tools/boot_time.py reads the overlap from the difference)
        const hipStream_t st = c->profiling ? c->stream : c->ensure_side_stream();
        const zkm_event e(c);
        e.record(c->stream);
        ZKM_HIP_CHECK(hipStreamWaitEvent(st, e.e, 0));
        side.st = st;
        zkm_boot_chain(c, bj.data(), K, d_desc, st);
        chains_done = zkm_event(c);
        chains_done.record(st);
    }

    // ---- the steps' memory, logic and arithmetic operations, behind the bootstrap's in the joined lists (Memory and Arithmetic are sized
    // on them); the rows follow once the table exists
    size_t nstep = 0;
    {
        zkm_steps_seg ss[ZKM_MAX_SEG];
        for (size_t s = 0; s < K; s++)
            if (b[s].st) ss[nstep++] = b[s].steps_seg(nullptr, write);
        if (nstep) zkm_cpu_steps_launch(c, ss, nstep, false, true);
    }
    // ---- Memory and Arithmetic sizing phases; waits (1) and (2)
    std::vector<zkm_memory_job> mj;
    std::vector<zkm_arith_job> aj;
    mj.reserve(K);
    aj.reserve(K);
    for (size_t s = 0; s < K; s++) {
        b[s].me_what = b[s].what + ": " + zkm_table_at(ME)->name;
        b[s].ar_what = b[s].what + ": " + zkm_table_at(AR)->name;
        mj.emplace_back(c, b[s].me_what.c_str(), b[s].d.memory_ops, b[s].nmemory());
        aj.emplace_back(c, b[s].ar_what.c_str(), b[s].d.arithmetic_ops, b[s].narithmetic());
        mj[s].d_acc = (unsigned long long*)(d_sync + s * SYNC_WORDS);
        mj[s].d_count = d_sync + s * SYNC_WORDS + 6;
        aj[s].d_counts = d_sync + s * SYNC_WORDS + 7;
    }
    zkm_memory_widths(mj.data(), K);
    zkm_arithmetic_count(aj.data(), K);
    c->download(sync.data(), d_sync, K * SYNC_WORDS * 8);                                                               // wait (1)
    std::vector<segment_block> out(K);
    const size_t cap = (size_t)1 << SEG_MAX_LOG_N;
    for (size_t s = 0; s < K; s++)
        if (b[s].im)
            if (const std::string m = zkm_boot_refusal_early(bj[s], &sync[s * SYNC_WORDS + 11]); !m.empty()) b[s].refuse(CPU, m);
    for (size_t s = 0; s < K; s++) {
        const size_t ar_n = zkm_arithmetic_height(aj[s], &sync[s * SYNC_WORDS + 7], nullptr);
        if (ar_n > cap) b[s].refuse(AR, "the table needs " + std::to_string(ar_n) + " rows, more than 2^" + std::to_string(SEG_MAX_LOG_N));
        b[s].lg[AR] = log2_of(ar_n);
    }
    zkm_memory_sort(mj.data(), K, sync.data(), SYNC_WORDS);
    c->download(sync.data(), d_sync, K * SYNC_WORDS * 8);                                                               // wait (2)
    for (size_t s = 0; s < K; s++) {
        const size_t me_n = zkm_memory_height(mj[s], sync[s * SYNC_WORDS + 6], nullptr);
        if (me_n > cap) b[s].refuse(ME, "the table needs " + std::to_string(me_n) + " rows, more than 2^" + std::to_string(SEG_MAX_LOG_N));
        b[s].lg[ME] = log2_of(me_n);
        for (int t = 0; t < NTAB; t++) {
            out[s].lg[t] = b[s].lg[t];
            out[s].off[t + 1] = out[s].off[t] + (zkm_table_at(t)->width << b[s].lg[t]);
        }
    }
    if (!write) return out;

    // ---- one output block per segment (each handle is freed on its own) and every writer, a launch per kernel for the wave; wait (3)
    for (size_t s = 0; s < K; s++) {
        b[s].put(sb, false);
        out[s].block = zkm_scratch(c, out[s].off[NTAB] * sizeof(gl_t));
        // (a CPU table built from steps: the kinds store the cells they set over zeros)
        if (b[s].st)
            ZKM_HIP_CHECK(hipMemsetAsync(out[s].block.as<gl_t>() + out[s].off[CPU], 0, (out[s].off[CPU + 1] - out[s].off[CPU]) * sizeof(gl_t), c->stream));
    }
    auto T = [&](size_t s, int t) { return out[s].block.as<gl_t>() + out[s].off[t]; };
    auto flag = [&](size_t s, int k) { return (unsigned*)(d_sync + s * SYNC_WORDS + 9) + k; };   // 0 Logic, 1 Memory, 2 Arithmetic
    {
        unsigned lg[ZKM_MAX_SEG];
        gl_t* o[ZKM_MAX_SEG];
        unsigned* bad[ZKM_MAX_SEG];
        for (size_t s = 0; s < K; s++) { lg[s] = b[s].lg[AR]; o[s] = T(s, AR); bad[s] = flag(s, 2); }
        zkm_arithmetic_write(aj.data(), K, lg, o, bad);
    }
    // the data-parallel writers: table t's descriptor for segment s from the table's description and its fields, then what only this
    // table has (`more`)
    auto writers = [&](int t, auto&& more) {
        const ops_fields& f = fields_of(t);
        const zkm_writer& d = zkm_table_at(t)->writer;
        zkm_writer_seg w[ZKM_MAX_SEG];
        for (size_t s = 0; s < K; s++) {
            w[s] = zkm_writer_seg{{}, f.k(*b[s].o), b[s].n(t), 0, T(s, t)};
            for (uint32_t i = 0; i < d.nlists; i++) w[s].in[d.variable ? 2 * i : i] = f.ptr(b[s].d, f.list[i]);
            more(s, w[s]);
        }
        zkm_launch_writers(c, zkm_table_at(t)->id, w, K);
    };
    using W = zkm_writer_seg&;
    // (PoseidonSponge first: its writer zero-fills the table, the bootstrap's rows go in behind it; the bootstrap's timestamps in front of
    // the Poseidon writer)
    writers(PS, [&](size_t s, W w) { w.in[1] = b[s].d_pso; w.in[3] = b[s].d_psr; });
    if (nboot) {
        for (size_t s = 0; s < K; s++) {
            if (!b[s].im) continue;
            bj[s].d.po_ts = (uint64_t*)b[s].d.poseidon_timestamps;
            bj[s].d.cpu = T(s, CPU);
            bj[s].d.cpu_rs = 1;
            bj[s].d.cpu_cs = b[s].n(CPU);
            bj[s].d.ps = T(s, PS);
            bj[s].d.ps_rs = 1;
            bj[s].d.ps_cs = b[s].n(PS);
        }
        ZKM_HIP_CHECK(hipStreamWaitEvent(c->stream, chains_done.e, 0));
        side.st = nullptr;                      // (from here on the compute stream is behind the chains)
        zkm_boot_late(c, bj.data(), K, d_desc + nboot);
    }
    // (the bootstrap's permutations come first; a Poseidon table without permutations is seed 0 with no inputs: every row is the padding row)
    writers(PO, [&](size_t s, W w) {
        w.k = b[s].nposeidon();
        if (!w.k) w.in[0] = w.in[1] = nullptr;
    });
    writers(KK, [](size_t, W) {});
    writers(KS, [&](size_t s, W w) { w.in[1] = b[s].d_kso; w.in[3] = b[s].d_ksr; w.aux = b[s].ks_rows; });
    for (const int t : {SE, SES, SC, SCS}) writers(t, [](size_t, W) {});
    writers(LO, [&](size_t s, W w) { w.k = b[s].nlogic(); w.bad = (int*)flag(s, 0); });
    {
        unsigned lg[ZKM_MAX_SEG];
        gl_t* o[ZKM_MAX_SEG];
        int* bad[ZKM_MAX_SEG];
        for (size_t s = 0; s < K; s++) { lg[s] = b[s].lg[ME]; o[s] = T(s, ME); bad[s] = (int*)flag(s, 1); }
        zkm_memory_write(mj.data(), K, lg, o, bad);
    }
    // the CPU table: device-resident rows of every segment in one launch; host rows piece by piece, each behind its own copy (last: the
    // copies overlap everything above)
    if (nstep) {
        zkm_steps_seg ss[ZKM_MAX_SEG];
        size_t k = 0;
        for (size_t s = 0; s < K; s++)
            if (b[s].st) ss[k++] = b[s].steps_seg(T(s, CPU), false);
        zkm_cpu_steps_launch(c, ss, k, true, false);
    }
    {
        cpu_seg cs[ZKM_MAX_SEG];
        size_t nd = 0;
        for (size_t s = 0; s < K; s++)
            if (!b[s].cpu_host && !b[s].st) cs[nd++] = cpu_seg{b[s].d.cpu_rows, b[s].o->ncpu_rows, b[s].bn.cpu_rows, b[s].n(CPU), T(s, CPU)};
        if (nd) launch_cpu_rows_to_cols(c, cs, nd);
        for (size_t s = 0; s < K; s++) {
            if (!b[s].cpu_host) continue;
            for (size_t r0 = 0, k = 0; r0 < b[s].o->ncpu_rows; r0 += b[s].piece_rows, k++) {
                ZKM_HIP_CHECK(hipStreamWaitEvent(c->stream, b[s].piece_done[k].e, 0));
                const cpu_seg piece{b[s].d.cpu_rows + r0 * CPU_W, std::min(b[s].piece_rows, b[s].o->ncpu_rows - r0), b[s].bn.cpu_rows + r0, b[s].n(CPU),
                                    T(s, CPU)};
                launch_cpu_rows_to_cols(c, &piece, 1);
            }
        }
    }
    c->download(sync.data(), d_sync, K * SYNC_WORDS * 8);                                                               // wait (3)
    for (size_t s = 0; s < K; s++) {
        const unsigned* f = (const unsigned*)&sync[s * SYNC_WORDS + 9];
        if (f[0]) b[s].refuse(LO, zkm_table_at(LO)->writer.bad);
        if (f[1]) b[s].refuse(ME, "a range check is 2^log_n or more (a context or segment gap)");
        if (f[2]) b[s].refuse(AR, "a shared-column value is 2^16 or more");
        if (b[s].im)
            if (const std::string m = zkm_boot_refusal_late(bj[s], &sync[s * SYNC_WORDS + 11]); !m.empty()) b[s].refuse(CPU, m);
    }
    return out;
}

// the builders of a call: argument checks, every host check of every segment, the host-known heights.  A call of one segment through
// the one-segment entry points names no position (label = false).
std::vector<builder> make_builders(const char* what, zkm_ctx* c, const zkm_stark_config* cfg, const zkm_segment_ops* ops, size_t nseg, size_t seg_base,
                                   bool label, const zkm_boot_image* images = nullptr, const zkm_cpu_steps* steps = nullptr) {
    if (!cfg || !ops) throw std::runtime_error(std::string(what) + ": null argument");
    if (nseg == 0) throw std::runtime_error(std::string(what) + ": no segments");
    if (cfg->cap_height > SEG_MAX_LOG_N) throw std::runtime_error(std::string(what) + ": cap_height out of range");
    std::vector<builder> b;
    b.reserve(nseg);
    for (size_t s = 0; s < nseg; s++) {
        b.emplace_back(what, c, ops + s, seg_base + s, label, images ? images + s : nullptr, steps ? steps + s : nullptr);
        b.back().check_host();
        b.back().heights(cfg);
    }
    return b;
}

// a call of nseg segments in at least `nwaves` waves of at most ZKM_MAX_SEG: even sizes (two stack heights at most, as the prover's own waves)
std::vector<size_t> even_waves(size_t nseg, size_t nwaves) {
    nwaves = std::min(nseg, std::max<size_t>(nwaves, (nseg + ZKM_MAX_SEG - 1) / ZKM_MAX_SEG));
    std::vector<size_t> k(nwaves, nseg / nwaves);
    for (size_t w = 0; w < nseg % nwaves; w++) k[w]++;
    return k;
}

}  // namespace

struct zkm_staged_ops {
    zkm_ctx* ctx = nullptr;
    zkm_scratch block;                   // the CPU rows and every list
    zkm_segment_ops dev{};               // the segment with device pointers; the two offset arrays point at the copies below
    std::vector<uint64_t> ps_off, ks_off;
    zkm_copy_fence fence;                // the uploads on the two copy streams (behind the block: it has waited when the block goes back)
    ~zkm_staged_ops() {
        if (!block.p) return;
        std::lock_guard<std::mutex> lk(g_staged_mu);
        g_staged_ops.erase(block.p);
    }
};

extern "C" {

// the body of zkm_segments_tables[_boot] (images: one per segment, or null)
static int segments_tables(const char* what, zkm_ctx* c, const zkm_stark_config* cfg, size_t nseg, const zkm_boot_image* images,
                           const zkm_segment_ops* ops, unsigned* log_n_out, zkm_staged** out, char** err, const zkm_cpu_steps* steps = nullptr) {
    return zkm_api(what, c, err, [&] {
        if (!log_n_out) throw std::runtime_error(std::string(what) + ": null argument");
        std::vector<builder> b = make_builders(what, c, cfg, ops, nseg, 0, true, images, steps);
        std::vector<segment_block> blocks;   // (a failure in a later wave releases the earlier waves' blocks: no handle is left behind)
        size_t s0 = 0;
        for (const size_t k : even_waves(nseg, 1)) {
            for (segment_block& sb : build_wave(c, b.data() + s0, k, out != nullptr)) blocks.push_back(std::move(sb));
            s0 += k;
        }
        for (size_t s = 0; s < nseg; s++)
            for (int t = 0; t < NTAB; t++) log_n_out[NTAB * s + t] = blocks[s].lg[t];
        if (!out) return;
        std::vector<zkm_staged*> handles;
        try {
            for (size_t s = 0; s < nseg; s++) {
                handles.push_back(zkm_staged_from_segment(c, blocks[s].block.p, blocks[s].off));
                blocks[s].block.take();
            }
        } catch (...) {
            for (zkm_staged* h : handles) zkm_staged_free(h);
            throw;
        }
        std::copy(handles.begin(), handles.end(), out);
    });
}
int zkm_segments_tables(zkm_ctx* c, const zkm_stark_config* cfg, size_t nseg, const zkm_segment_ops* ops, unsigned* log_n_out, zkm_staged** out,
                        char** err) {
    return segments_tables("zkm_segments_tables", c, cfg, nseg, nullptr, ops, log_n_out, out, err);
}
int zkm_segments_tables_boot(zkm_ctx* c, const zkm_stark_config* cfg, size_t nseg, const zkm_boot_image* images, const zkm_segment_ops* ops,
                             unsigned* log_n_out, zkm_staged** out, char** err) {
    if (!images) return zkm_fail(err, "zkm_segments_tables_boot: null argument");
    return segments_tables("zkm_segments_tables_boot", c, cfg, nseg, images, ops, log_n_out, out, err);
}

// A *_steps call without a context still makes every refusal that needs no device -- the walk over the steps among them -- before it
// reports the missing context: what the host decides can be checked where there is no GPU.
static int steps_without_context(const char* what, const zkm_stark_config* cfg, size_t nseg, const zkm_boot_image* images, const zkm_cpu_steps* steps,
                                 const zkm_segment_ops* ops, char** err) {
    return zkm_api(what, err, [&] {
        make_builders(what, nullptr, cfg, ops, nseg, 0, true, images, steps);
        throw std::runtime_error(std::string(what) + ": null argument");
    });
}
int zkm_segments_tables_steps(zkm_ctx* c, const zkm_stark_config* cfg, size_t nseg, const zkm_boot_image* images, const zkm_cpu_steps* steps,
                              const zkm_segment_ops* ops, unsigned* log_n_out, zkm_staged** out, char** err) {
    if (!steps) return zkm_fail(err, "zkm_segments_tables_steps: null argument");
    if (!c) return steps_without_context("zkm_segments_tables_steps", cfg, nseg, images, steps, ops, err);
    return segments_tables("zkm_segments_tables_steps", c, cfg, nseg, images, ops, log_n_out, out, err, steps);
}

// the body of zkm_prove_segments_ops[_boot | _steps] and of the pool's workers (images, steps: one per segment, or null)
static int prove_segments_ops(const char* what, zkm_ctx* c, const zkm_stark_config* cfg, size_t nseg, const zkm_boot_image* images,
                              const zkm_segment_ops* ops, const uint64_t* const* pub, const size_t* npub, uint64_t* const* proofs,
                              size_t* offsets_out, uint64_t* const* challenges, char** err, size_t seg_base, const zkm_cpu_steps* steps = nullptr) {
    return zkm_api(what, c, err, [&]() -> int {
        if (proofs && !challenges) throw std::runtime_error(std::string(what) + ": null argument");
        if (!proofs && !offsets_out) throw std::runtime_error(std::string(what) + ": null argument");
        std::vector<builder> b = make_builders(what, c, cfg, ops, nseg, seg_base, true, images, steps);
        // ---- the waves: what a segment holds while it is proven (the prover's estimate at the heights the host knows), its tables,
        // its part of the staging block and its bootstrap's scratch, against the budget of zkm_prove_segments
        size_t nwaves = 1;
        if (proofs && nseg > 1) {
            size_t free_b = 0, total_b = 0, live = 0, cached = 0;
            ZKM_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
            zkm_ctx_memory(c, &live, &cached);
            const double budget = c->segments_memory_budget ? (double)c->segments_memory_budget : 0.8 * ((double)cached + (double)free_b);
            double total = 0;
            for (size_t s = 0; s < nseg; s++) {
                double tables = 0;
                for (int t = 0; t < NTAB; t++) tables += 8.0 * (double)(zkm_table_at(t)->width << b[s].lg[t]);
                total += zkm_segment_footprint(cfg, b[s].lg) + tables + (double)b[s].plan(true, 0) + (double)zkm_boot_scratch_bytes(b[s].im);
            }
            nwaves = (size_t)std::min<double>((double)nseg, std::max(1.0, std::ceil(total / std::max(budget, 1.0))));
        }
        size_t s0 = 0;
        for (const size_t k : even_waves(nseg, nwaves)) {
            std::vector<segment_block> blocks = build_wave(c, b.data() + s0, k, proofs != nullptr);
            const uint64_t* traces[ZKM_MAX_SEG][NTAB] = {};
            const uint64_t* const* tr[ZKM_MAX_SEG];
            const unsigned* lg[ZKM_MAX_SEG];
            for (size_t s = 0; s < k; s++) {
                for (int t = 0; t < NTAB && proofs; t++) traces[s][t] = blocks[s].block.as<const uint64_t>() + blocks[s].off[t];
                tr[s] = traces[s];
                lg[s] = blocks[s].lg;
                if (offsets_out)
                    if (const int rc = zkm_prove_segment(nullptr, cfg, traces[s], lg[s], nullptr, 0, nullptr, offsets_out + (NTAB + 1) * (s0 + s), nullptr, err))
                        return rc;
            }
            if (proofs)
                if (const int rc = zkm_prove_segments_entry(what, c, cfg, k, tr, nullptr, lg, pub ? pub + s0 : nullptr, npub ? npub + s0 : nullptr,
                                                            proofs + s0, challenges + s0, err, seg_base + s0))
                    return rc;
            s0 += k;
        }
        return 0;
    });
}

int zkm_prove_segments_ops_entry(const char* what, zkm_ctx* c, const zkm_stark_config* cfg, size_t nseg, const zkm_segment_ops* ops,
                                 const uint64_t* const* pub, const size_t* npub, uint64_t* const* proofs, size_t* offsets_out,
                                 uint64_t* const* challenges, char** err, size_t seg_base) {
    return prove_segments_ops(what, c, cfg, nseg, nullptr, ops, pub, npub, proofs, offsets_out, challenges, err, seg_base);
}
int zkm_prove_segments_ops(zkm_ctx* c, const zkm_stark_config* cfg, size_t nseg, const zkm_segment_ops* ops, const uint64_t* const* pub,
                           const size_t* npub, uint64_t* const* proofs, size_t* offsets_out, uint64_t* const* challenges, char** err) {
    return prove_segments_ops("zkm_prove_segments_ops", c, cfg, nseg, nullptr, ops, pub, npub, proofs, offsets_out, challenges, err, 0);
}
int zkm_prove_segments_ops_boot(zkm_ctx* c, const zkm_stark_config* cfg, size_t nseg, const zkm_boot_image* images, const zkm_segment_ops* ops,
                                const uint64_t* const* pub, const size_t* npub, uint64_t* const* proofs, size_t* offsets_out,
                                uint64_t* const* challenges, char** err) {
    if (!images) return zkm_fail(err, "zkm_prove_segments_ops_boot: null argument");
    return prove_segments_ops("zkm_prove_segments_ops_boot", c, cfg, nseg, images, ops, pub, npub, proofs, offsets_out, challenges, err, 0);
}

int zkm_prove_segments_ops_steps(zkm_ctx* c, const zkm_stark_config* cfg, size_t nseg, const zkm_boot_image* images, const zkm_cpu_steps* steps,
                                 const zkm_segment_ops* ops, const uint64_t* const* pub, const size_t* npub, uint64_t* const* proofs,
                                 size_t* offsets_out, uint64_t* const* challenges, char** err) {
    if (!steps) return zkm_fail(err, "zkm_prove_segments_ops_steps: null argument");
    if (!c) return steps_without_context("zkm_prove_segments_ops_steps", cfg, nseg, images, steps, ops, err);
    return prove_segments_ops("zkm_prove_segments_ops_steps", c, cfg, nseg, images, ops, pub, npub, proofs, offsets_out, challenges, err, 0, steps);
}
// (zkm_internal.h: the pool's workers, on the outputs of a staged or expanded group)
extern "C++" int zkm_prove_segments_ops_steps_entry(const char* what, zkm_ctx* c, const zkm_stark_config* cfg, size_t nseg, const zkm_boot_image* images,
                                                    const zkm_cpu_steps* steps, const zkm_segment_ops* ops, const uint64_t* const* pub,
                                                    const size_t* npub, uint64_t* const* proofs, size_t* offsets_out, uint64_t* const* challenges,
                                                    char** err, size_t seg_base) {
    if (!steps) return zkm_fail(err, what, ": null argument");
    return prove_segments_ops(what, c, cfg, nseg, images, ops, pub, npub, proofs, offsets_out, challenges, err, seg_base, steps);
}

// the body of zkm_segment_tables[_boot] (image: or null)
static int segment_tables(const char* what, zkm_ctx* c, const zkm_stark_config* cfg, const zkm_boot_image* image, const zkm_segment_ops* ops,
                          unsigned* log_n_out, zkm_staged** out, char** err) {
    return zkm_api(what, c, err, [&] {
        if (!ops || !log_n_out) throw std::runtime_error(std::string(what) + ": null argument");
        std::vector<builder> b = make_builders(what, c, cfg, ops, 1, 0, false, image);
        segment_block sb = std::move(build_wave(c, b.data(), 1, out != nullptr)[0]);
        for (int t = 0; t < NTAB; t++) log_n_out[t] = sb.lg[t];
        if (!out) return;
        *out = zkm_staged_from_segment(c, sb.block.p, sb.off);
        sb.block.take();
    });
}
int zkm_segment_tables(zkm_ctx* c, const zkm_stark_config* cfg, const zkm_segment_ops* ops, unsigned* log_n_out, zkm_staged** out, char** err) {
    return segment_tables("zkm_segment_tables", c, cfg, nullptr, ops, log_n_out, out, err);
}
int zkm_segment_tables_boot(zkm_ctx* c, const zkm_stark_config* cfg, const zkm_boot_image* image, const zkm_segment_ops* ops, unsigned* log_n_out,
                            zkm_staged** out, char** err) {
    if (!image) return zkm_fail(err, "zkm_segment_tables_boot: null argument");
    return segment_tables("zkm_segment_tables_boot", c, cfg, image, ops, log_n_out, out, err);
}

// the body of zkm_prove_segment_ops[_boot] (image: or null)
static int prove_segment_ops(const char* what, zkm_ctx* c, const zkm_stark_config* cfg, const zkm_boot_image* image, const zkm_segment_ops* ops,
                             const uint64_t* pub, size_t npub, uint64_t* proofs, size_t* offsets_out, uint64_t* challenges, char** err) {
    return zkm_api(what, c, err, [&] {
        if (!ops) throw std::runtime_error(std::string(what) + ": null argument");
        std::vector<builder> b = make_builders(what, c, cfg, ops, 1, 0, false, image);
        segment_block sb = std::move(build_wave(c, b.data(), 1, proofs != nullptr)[0]);
        const uint64_t* traces[NTAB] = {};
        for (int t = 0; t < NTAB; t++) traces[t] = proofs ? sb.block.as<const uint64_t>() + sb.off[t] : nullptr;
        return zkm_prove_segment(proofs ? c : nullptr, cfg, traces, sb.lg, pub, npub, proofs, offsets_out, challenges, err);
    });
}
int zkm_prove_segment_ops(zkm_ctx* c, const zkm_stark_config* cfg, const zkm_segment_ops* ops, const uint64_t* pub, size_t npub,
                          uint64_t* proofs, size_t* offsets_out, uint64_t* challenges, char** err) {
    return prove_segment_ops("zkm_prove_segment_ops", c, cfg, nullptr, ops, pub, npub, proofs, offsets_out, challenges, err);
}
int zkm_prove_segment_ops_boot(zkm_ctx* c, const zkm_stark_config* cfg, const zkm_boot_image* image, const zkm_segment_ops* ops, const uint64_t* pub,
                               size_t npub, uint64_t* proofs, size_t* offsets_out, uint64_t* challenges, char** err) {
    if (!image) return zkm_fail(err, "zkm_prove_segment_ops_boot: null argument");
    return prove_segment_ops("zkm_prove_segment_ops_boot", c, cfg, image, ops, pub, npub, proofs, offsets_out, challenges, err);
}

// ---- staged operations: the next call's lists behind the current proofs.  Every byte count is known on the host, so the uploads are
// queued on the two copy streams (behind what the compute stream has queued: the block may be one a finished call released) and the
// call returns; zkm_staged_ops_get orders the compute stream behind them with a device-side wait.
int zkm_segment_ops_stage(zkm_ctx* c, const zkm_segment_ops* ops, zkm_staged_ops** out, char** err) {
    return zkm_api("zkm_segment_ops_stage", c, err, [&] {
        if (!ops || !out) throw std::runtime_error("zkm_segment_ops_stage: null argument");
        builder b("zkm_segment_ops_stage", c, ops, 0, false);
        b.check_host();
        std::unique_ptr<zkm_staged_ops> h(new zkm_staged_ops());
        h->ctx = c;
        h->dev = *ops;
        if (ops->nposeidon_sponge) h->ps_off.assign(ops->poseidon_sponge_off, ops->poseidon_sponge_off + ops->nposeidon_sponge + 1);
        if (ops->nkeccak_sponge) h->ks_off.assign(ops->keccak_sponge_off, ops->keccak_sponge_off + ops->nkeccak_sponge + 1);
        h->dev.poseidon_sponge_off = h->ps_off.data();
        h->dev.keccak_sponge_off = h->ks_off.data();
        const size_t cpu_bytes = ops->ncpu_rows * CPU_W * 8;
        std::vector<list_ref> lists = lists_of(h->dev);
        size_t bytes = align_up(cpu_bytes);
        for (const list_ref& l : lists) bytes += align_up(l.bytes);
        h->block = zkm_scratch(c, bytes);
        char* base = h->block.as<char>();
        h->fence.begin(c);   // (a copy that fails to queue: the ones before it land before the block goes back)
        // alternate streams: the CPU rows in pieces of >= 16 MB, every other list in one copy (device-resident lists are copied too: the
        // handle owns all it hands out)
        size_t turn = 0, at = 0;
        auto copy = [&](void* dst, const void* src, size_t n) {
            ZKM_HIP_CHECK(hipMemcpyAsync(dst, src, n, hipMemcpyDefault, (turn++ & 1) ? c->copy_stream2 : c->copy_stream));
        };
        const size_t piece = std::max<size_t>((size_t)16 << 20, cpu_bytes / 16);
        for (size_t o0 = 0; o0 < cpu_bytes; o0 += piece) copy(base + o0, (const char*)ops->cpu_rows + o0, std::min(piece, cpu_bytes - o0));
        h->dev.cpu_rows = (const uint64_t*)base;
        at = align_up(cpu_bytes);
        for (const list_ref& l : lists) {
            if (!l.bytes) continue;
            copy(base + at, l.get(), l.bytes);
            l.set(base + at);
            at += align_up(l.bytes);
        }
        h->fence.end();
        {
            std::lock_guard<std::mutex> lk(g_staged_mu);
            g_staged_ops[h->block.p] = c;
        }
        *out = h.release();
    });
}

int zkm_staged_ops_get(zkm_staged_ops* h, zkm_segment_ops* ops_out) {
    if (!h || !ops_out) return 1;
    zkm_ctx* c = h->ctx;
    if (!h->fence.is_joined() && zkm_api("zkm_staged_ops_get", c, nullptr, [&] { h->fence.join(); })) return 1;
    *ops_out = h->dev;
    return 0;
}

int zkm_staged_ops_ready(zkm_staged_ops* h, int wait) { return h ? h->fence.ready(wait != 0) : 1; }

void zkm_staged_ops_free(zkm_staged_ops* h) { delete h; }   // (the fence waits for the uploads before the block goes back)

}  // extern "C"
