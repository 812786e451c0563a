// segment_ops.hip -- a whole segment's twelve tables built on the device from its raw operations (the reference's Traces::into_tables,
// witness/traces.rs:230-320), and the proof of that segment in one call.
//
//   zkm_segment_tables      every height (Table::all() order), ONE output block from the context's allocator, every table written
//                           into it, handed out as a segment-shaped zkm_staged;
//   zkm_prove_segment_ops   zkm_segment_tables, zkm_prove_segment on the block, the block freed.
//
// The one new kernel, k_cpu_rows_to_cols, turns the emulator's CPU rows (Vec<CpuColumnsView<F>>: 259 words a row, row-major) into the
// column-major table of trace_rows_to_poly_values (util.rs:37-46), canonical.  Every other table comes from its existing launcher;
// the Memory and Arithmetic witnesses run in phases (zkm_internal.h zkm_memory_job / zkm_arith_job) so that they share host waits.
//
// Host waits per call, each ONE download of a few words (zkm_ctx::download):
//   (1) the Memory key widths, with the Arithmetic row count and validation flags;
//   (2) the Memory row count after the sort and the gap scan: every height is then known, and the output block is allocated;
//   (3) the validation flags of every writer (Logic op codes, Memory range checks, Arithmetic shared-column values), one device array.
// Sizing mode (out == NULL) ends after (2).  Inputs in host memory go through one staging block; CPU rows in host memory are copied in
// row pieces on the context's two copy streams, each piece transposed on the compute stream behind its own copy, so that the largest
// transfer overlaps the other tables' generation.
#include <algorithm>
#include <string>
#include <vector>

#include "zkm_internal.h"

extern "C" zkm_staged* zkm_staged_from_segment(zkm_ctx* c, void* block, const size_t off[13]);   // core.hip

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
__global__ __launch_bounds__(TR_THREADS) void k_cpu_rows_to_cols(const uint64_t* __restrict__ rows, size_t nrows, size_t row0, size_t n,
                                                                  gl_t* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint64_t t[TR_ROWS * CPU_W];
    const size_t pr = (size_t)blockIdx.x * TR_ROWS;
    const unsigned here = (unsigned)(nrows - pr < (size_t)TR_ROWS ? nrows - pr : TR_ROWS);
    const uint64_t* src = rows + pr * CPU_W;
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
    gl_t* o = out + row0 + pr + r;
#pragma unroll 4
    for (unsigned c = 2 * (threadIdx.x >> 6) + (lane >> 5); c < (unsigned)CPU_W; c += 2 * (TR_THREADS / 64)) {
        const uint64_t v = t[r * CPU_W + c];
        o[(size_t)c * n] = v >= GL_P ? v - GL_P : v;
    }
}

void launch_cpu_rows_to_cols(zkm_ctx* c, const uint64_t* rows, size_t nrows, size_t row0, size_t n, gl_t* out) {
    zkm_prof_scope ps(c, "segment_ops/cpu_rows_to_cols");
    hipLaunchKernelGGL(k_cpu_rows_to_cols, dim3((unsigned)((nrows + TR_ROWS - 1) / TR_ROWS)), dim3(TR_THREADS), 0, c->stream, rows, nrows, row0,
                       n, out);
    ZKM_HIP_CHECK(hipGetLastError());
}

// Table::all() (all_stark.rs:117-134) and the reference's names of the tables, for messages
enum { AR, CPU, PO, PS, KK, KS, SE, SES, SC, SCS, LO, ME, NTAB };
const char* const NAME[NTAB] = {"Arithmetic", "Cpu", "Poseidon", "PoseidonSponge", "Keccak", "KeccakSponge", "ShaExtend", "ShaExtendSponge",
                                "ShaCompress", "ShaCompressSponge", "Logic", "Memory"};
const int TABLE_ID[NTAB] = {ZKM_TABLE_ARITHMETIC, ZKM_TABLE_CPU, ZKM_TABLE_POSEIDON, ZKM_TABLE_POSEIDON_SPONGE, ZKM_TABLE_KECCAK,
                            ZKM_TABLE_KECCAK_SPONGE, ZKM_TABLE_SHA_EXTEND, ZKM_TABLE_SHA_EXTEND_SPONGE, ZKM_TABLE_SHA_COMPRESS,
                            ZKM_TABLE_SHA_COMPRESS_SPONGE, ZKM_TABLE_LOGIC, ZKM_TABLE_MEMORY};

unsigned log2_of(size_t pow2) { return pow2 ? 63 - __builtin_clzll(pow2) : 0; }
size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }

// after a failure the copy streams may still be writing into the staging block: wait for them before it goes back to the allocator
struct copy_join {
    zkm_ctx* c = nullptr;
    ~copy_join() {
        if (!c) return;
        (void)hipStreamSynchronize(c->copy_stream);
        (void)hipStreamSynchronize(c->copy_stream2);
    }
};

// the output of one build: the block (empty in sizing mode) and the word offset of each table in it
struct segment_block {
    zkm_scratch block;
    size_t off[13] = {};
};

struct builder {
    const char* what;
    zkm_ctx* c;
    const zkm_segment_ops& o;
    unsigned lg[NTAB] = {};

    [[noreturn]] void refuse(int t, const std::string& msg) const { throw std::runtime_error(std::string(what) + ": " + NAME[t] + ": " + msg); }
    std::string name(int t) const { return std::string(what) + ": " + NAME[t]; }
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

    segment_block run(const zkm_stark_config* cfg, bool write) {
        if (!cfg) throw std::runtime_error(std::string(what) + ": null argument");
        if (cfg->cap_height > SEG_MAX_LOG_N) throw std::runtime_error(std::string(what) + ": cap_height out of range");
        const size_t min_rows = std::max<size_t>((size_t)1 << cfg->cap_height, 64);   // max(num_cap_elements, MIN_TRACE_LEN), traces.rs:246-247
        // ---- every check that needs no device
        need(CPU, o.ncpu_rows, {o.cpu_rows});
        need(AR, o.narithmetic, {o.arithmetic_ops});
        need(LO, o.nlogic, {o.logic_ops});
        need(ME, o.nmemory, {o.memory_ops});
        need(PO, o.nposeidon, {o.poseidon_inputs, o.poseidon_timestamps});
        need(PS, o.nposeidon_sponge, {o.poseidon_sponge_off, o.poseidon_sponge_meta});
        need(KK, o.nkeccak, {o.keccak_inputs, o.keccak_timestamps});
        need(KS, o.nkeccak_sponge, {o.keccak_sponge_off, o.keccak_sponge_meta});
        need(SE, o.nsha_extend, {o.sha_extend_inputs, o.sha_extend_timestamps});
        need(SES, o.nsha_extend_sponge, {o.sha_extend_sponge_w16, o.sha_extend_sponge_meta});
        need(SC, o.nsha_compress, {o.sha_compress_hx, o.sha_compress_w, o.sha_compress_meta});
        need(SCS, o.nsha_compress_sponge, {o.sha_compress_sponge_hx, o.sha_compress_sponge_w, o.sha_compress_sponge_meta});
        if (o.ncpu_rows == 0 || (o.ncpu_rows & (o.ncpu_rows - 1)) || o.ncpu_rows > ((size_t)1 << SEG_MAX_LOG_N))
            refuse(CPU, std::to_string(o.ncpu_rows) + " rows: not a power of two of at most 2^" + std::to_string(SEG_MAX_LOG_N));
        if (o.nmemory == 0) refuse(ME, "No memory ops?");
        if (o.nmemory >= ((size_t)1 << 32)) refuse(ME, "2^32 or more memory ops");
        if (o.narithmetic >= ((size_t)1 << 31)) refuse(AR, "2^31 or more arithmetic ops");
        std::vector<uint64_t> ps_row, ks_row;
        const size_t ps_rows = sponge_rows(PS, o.poseidon_sponge_off, o.nposeidon_sponge, 32, ps_row);
        const size_t ks_rows = sponge_rows(KS, o.keccak_sponge_off, o.nkeccak_sponge, 136, ks_row);
        const size_t ps_bytes = o.nposeidon_sponge ? o.poseidon_sponge_off[o.nposeidon_sponge] : 0;
        const size_t ks_bytes = o.nkeccak_sponge ? o.keccak_sponge_off[o.nkeccak_sponge] : 0;
        need(PS, ps_bytes, {o.poseidon_sponge_inputs});
        need(KS, ks_bytes, {o.keccak_sponge_inputs});
        lg[CPU] = log2_of(o.ncpu_rows);
        lg[PO] = height(PO, o.nposeidon, 1, min_rows);
        lg[PS] = height(PS, ps_rows, 1, min_rows);
        lg[KK] = height(KK, o.nkeccak, 24, min_rows);
        lg[KS] = height(KS, ks_rows, 1, min_rows);
        lg[SE] = height(SE, o.nsha_extend, 1, min_rows);
        lg[SES] = height(SES, o.nsha_extend_sponge, 48, min_rows);
        lg[SC] = height(SC, o.nsha_compress, 65, min_rows);
        lg[SCS] = height(SCS, o.nsha_compress_sponge, 1, min_rows);
        lg[LO] = height(LO, o.nlogic, 1, min_rows);

        // ---- the staging block: [0, 64) the writers' flags, then the CPU rows (host rows only), then every input list in host memory
        struct upload { const void* src; size_t bytes; const void** dev; };
        std::vector<upload> ups;
        const void *d_ar = o.arithmetic_ops, *d_me = o.memory_ops, *d_lo = o.logic_ops, *d_poi = o.poseidon_inputs, *d_pot = o.poseidon_timestamps,
                   *d_psi = o.poseidon_sponge_inputs, *d_pso = o.poseidon_sponge_off, *d_psm = o.poseidon_sponge_meta,
                   *d_psr = ps_row.data(), *d_kki = o.keccak_inputs, *d_kkt = o.keccak_timestamps, *d_ksi = o.keccak_sponge_inputs,
                   *d_kso = o.keccak_sponge_off, *d_ksm = o.keccak_sponge_meta, *d_ksr = ks_row.data(), *d_sei = o.sha_extend_inputs,
                   *d_set = o.sha_extend_timestamps, *d_sew = o.sha_extend_sponge_w16, *d_sem = o.sha_extend_sponge_meta,
                   *d_sch = o.sha_compress_hx, *d_scw = o.sha_compress_w, *d_scm = o.sha_compress_meta, *d_ssh = o.sha_compress_sponge_hx,
                   *d_ssw = o.sha_compress_sponge_w, *d_ssm = o.sha_compress_sponge_meta;
        auto add = [&](const void** p, size_t bytes, bool host_only) {
            if (bytes && (host_only || !zkm_is_device_ptr(*p))) ups.push_back(upload{*p, bytes, p});
        };
        add(&d_ar, o.narithmetic * 12, false);
        add(&d_me, o.nmemory * 48, false);
        const size_t nsizing = ups.size();
        if (write) {
            add(&d_lo, o.nlogic * 12, false);
            add(&d_poi, o.nposeidon * 96, false);
            add(&d_pot, o.nposeidon * 8, false);
            add(&d_psi, ps_bytes, false);
            add(&d_pso, o.nposeidon_sponge ? (o.nposeidon_sponge + 1) * 8 : 0, true);
            add(&d_psm, o.nposeidon_sponge * 32, false);
            add(&d_psr, o.nposeidon_sponge ? (o.nposeidon_sponge + 1) * 8 : 0, true);
            add(&d_kki, o.nkeccak * 200, false);
            add(&d_kkt, o.nkeccak * 8, false);
            add(&d_ksi, ks_bytes, false);
            add(&d_kso, o.nkeccak_sponge ? (o.nkeccak_sponge + 1) * 8 : 0, true);
            add(&d_ksm, o.nkeccak_sponge * 32, false);
            add(&d_ksr, o.nkeccak_sponge ? (o.nkeccak_sponge + 1) * 8 : 0, true);
            add(&d_sei, o.nsha_extend * 16, false);
            add(&d_set, o.nsha_extend * 8, false);
            add(&d_sew, o.nsha_extend_sponge * 64, false);
            add(&d_sem, o.nsha_extend_sponge * 32, false);
            add(&d_sch, o.nsha_compress * 32, false);
            add(&d_scw, o.nsha_compress * 256, false);
            add(&d_scm, o.nsha_compress * 64, false);
            add(&d_ssh, o.nsha_compress_sponge * 32, false);
            add(&d_ssw, o.nsha_compress_sponge * 256, false);
            add(&d_ssm, o.nsha_compress_sponge * 64, false);
        }
        const bool cpu_host = write && !zkm_is_device_ptr(o.cpu_rows);
        const size_t cpu_bytes = cpu_host ? o.ncpu_rows * CPU_W * 8 : 0;
        size_t stage_bytes = 64 + align_up(cpu_bytes);
        std::vector<size_t> up_off(ups.size());
        for (size_t i = 0; i < ups.size(); i++) {
            up_off[i] = stage_bytes;
            stage_bytes += align_up(ups[i].bytes);
        }
        zkm_scratch stage(c, stage_bytes);
        char* sb = stage.as<char>();
        unsigned* d_flags = (unsigned*)sb;   // [0] Logic op code, [1] Memory range check, [2] Arithmetic shared-column value
        std::vector<zkm_event> piece_done;
        copy_join join;
        const uint64_t* cpu_src = o.cpu_rows;
        size_t piece_rows = o.ncpu_rows;
        if (cpu_host) {
            // pieces of >= 8192 rows (17 MB), at most 16 of them; alternate copy streams, each behind what the compute stream has queued
            c->ensure_copy_stream(0);
            c->ensure_copy_stream(1);
            const zkm_event e(c);
            e.record(c->stream);
            ZKM_HIP_CHECK(hipStreamWaitEvent(c->copy_stream, e.e, 0));
            ZKM_HIP_CHECK(hipStreamWaitEvent(c->copy_stream2, e.e, 0));
            join.c = c;
            cpu_src = (const uint64_t*)(sb + 64);
            piece_rows = std::min<size_t>(o.ncpu_rows, std::max<size_t>(8192, o.ncpu_rows / 16));
            for (size_t r0 = 0, k = 0; r0 < o.ncpu_rows; r0 += piece_rows, k++) {
                hipStream_t st = (k & 1) ? c->copy_stream2 : c->copy_stream;
                ZKM_HIP_CHECK(hipMemcpyAsync((void*)(cpu_src + r0 * CPU_W), o.cpu_rows + r0 * CPU_W, piece_rows * CPU_W * 8, hipMemcpyHostToDevice, st));
                piece_done.emplace_back(c);
                piece_done.back().record(st);
            }
        }
        ZKM_HIP_CHECK(hipMemsetAsync(d_flags, 0, 64, c->stream));
        auto put = [&](size_t i) {
            ZKM_HIP_CHECK(hipMemcpyAsync(sb + up_off[i], ups[i].src, ups[i].bytes, hipMemcpyHostToDevice, c->stream));
            *ups[i].dev = sb + up_off[i];
        };
        for (size_t i = 0; i < nsizing; i++) put(i);

        // ---- Memory and Arithmetic sizing phases; waits (1) and (2)
        const std::string me_what = name(ME), ar_what = name(AR);
        zkm_memory_job mj(c, me_what.c_str(), (const uint64_t*)d_me, o.nmemory);
        zkm_arith_job aj(c, ar_what.c_str(), (const uint32_t*)d_ar, o.narithmetic);
        zkm_memory_widths(mj);
        zkm_arithmetic_count(aj);
        uint64_t acc[5], got[2];
        c->download({{acc, mj.d_acc, sizeof acc}, {got, aj.counts(), sizeof got}});                               // wait (1)
        const size_t ar_n = zkm_arithmetic_height(aj, got, nullptr);
        zkm_memory_sort(mj, acc);
        uint64_t count = 0;
        c->download(&count, mj.start.as<uint64_t>() + o.nmemory, 8);                                                    // wait (2)
        const size_t me_n = zkm_memory_height(mj, count, nullptr);
        if (me_n > ((size_t)1 << SEG_MAX_LOG_N)) refuse(ME, "the table needs " + std::to_string(me_n) + " rows, more than 2^" + std::to_string(SEG_MAX_LOG_N));
        if (ar_n > ((size_t)1 << SEG_MAX_LOG_N)) refuse(AR, "the table needs " + std::to_string(ar_n) + " rows, more than 2^" + std::to_string(SEG_MAX_LOG_N));
        lg[AR] = log2_of(ar_n);
        lg[ME] = log2_of(me_n);
        segment_block out;
        for (int t = 0; t < NTAB; t++) out.off[t + 1] = out.off[t] + (zkm_table_width(TABLE_ID[t]) << lg[t]);
        if (!write) return out;

        // ---- the one output block and every writer; wait (3)
        for (size_t i = nsizing; i < ups.size(); i++) put(i);
        out.block = zkm_scratch(c, out.off[12] * sizeof(gl_t));
        gl_t* base = out.block.as<gl_t>();
        auto T = [&](int t) { return base + out.off[t]; };
        auto N = [&](int t) { return (size_t)1 << lg[t]; };
        zkm_arithmetic_write(aj, lg[AR], T(AR), d_flags + 2);
        zkm_launch_poseidon_trace(c, 0, o.nposeidon ? (const uint64_t*)d_poi : nullptr, o.nposeidon ? (const uint64_t*)d_pot : nullptr, o.nposeidon,
                                  lg[PO], T(PO));
        zkm_launch_poseidon_sponge_trace(c, (const uint8_t*)d_psi, (const uint64_t*)d_pso, (const uint64_t*)d_psm, (const uint64_t*)d_psr,
                                         o.nposeidon_sponge, lg[PS], T(PS));
        zkm_launch_keccak_trace(c, (const uint64_t*)d_kki, (const uint64_t*)d_kkt, o.nkeccak, N(KK), T(KK));
        zkm_launch_keccak_sponge_trace(c, (const uint8_t*)d_ksi, (const uint64_t*)d_kso, (const uint64_t*)d_ksm, (const uint64_t*)d_ksr,
                                       o.nkeccak_sponge, ks_rows, lg[KS], T(KS));
        zkm_launch_sha_extend_trace(c, (const uint8_t*)d_sei, (const uint64_t*)d_set, o.nsha_extend, N(SE), T(SE));
        zkm_launch_sha_extend_sponge_trace(c, (const uint32_t*)d_sew, (const uint64_t*)d_sem, o.nsha_extend_sponge, N(SES), T(SES));
        zkm_launch_sha_compress_trace(c, false, (const uint32_t*)d_sch, (const uint32_t*)d_scw, (const uint64_t*)d_scm, o.nsha_compress, N(SC),
                                      T(SC));
        zkm_launch_sha_compress_trace(c, true, (const uint32_t*)d_ssh, (const uint32_t*)d_ssw, (const uint64_t*)d_ssm, o.nsha_compress_sponge,
                                      N(SCS), T(SCS));
        zkm_launch_logic_trace(c, (const uint32_t*)d_lo, o.nlogic, N(LO), T(LO), (int*)d_flags);
        zkm_memory_write(mj, lg[ME], T(ME), (int*)d_flags + 1);
        for (size_t r0 = 0, k = 0; r0 < o.ncpu_rows; r0 += piece_rows, k++) {   // (last: the copies overlap everything above)
            if (cpu_host) ZKM_HIP_CHECK(hipStreamWaitEvent(c->stream, piece_done[k].e, 0));
            launch_cpu_rows_to_cols(c, cpu_src + r0 * CPU_W, piece_rows, r0, N(CPU), T(CPU));
        }
        unsigned flags[3];
        c->download(flags, d_flags, sizeof flags);                                                                       // wait (3)
        if (flags[0]) refuse(LO, "op code out of range (0 and, 1 or, 2 xor, 3 nor)");
        if (flags[1]) refuse(ME, "a range check is 2^log_n or more (a context or segment gap)");
        if (flags[2]) refuse(AR, "a shared-column value is 2^16 or more");
        return out;
    }
};

}  // namespace

extern "C" {

int zkm_segment_tables(zkm_ctx* c, const zkm_stark_config* cfg, const zkm_segment_ops* ops, unsigned* log_n_out, zkm_staged** out, char** err) {
    return zkm_api("zkm_segment_tables", c, err, [&] {
        if (!ops || !log_n_out) throw std::runtime_error("zkm_segment_tables: null argument");
        builder b{"zkm_segment_tables", c, *ops};
        segment_block sb = b.run(cfg, out != nullptr);
        for (int t = 0; t < NTAB; t++) log_n_out[t] = b.lg[t];
        if (!out) return;
        *out = zkm_staged_from_segment(c, sb.block.p, sb.off);
        sb.block.take();
    });
}

int zkm_prove_segment_ops(zkm_ctx* c, const zkm_stark_config* cfg, const zkm_segment_ops* ops, const uint64_t* pub, size_t npub,
                          uint64_t* proofs, size_t* offsets_out, uint64_t* challenges, char** err) {
    return zkm_api("zkm_prove_segment_ops", c, err, [&] {
        if (!ops) throw std::runtime_error("zkm_prove_segment_ops: null argument");
        builder b{"zkm_prove_segment_ops", c, *ops};
        segment_block sb = b.run(cfg, proofs != nullptr);
        const uint64_t* traces[NTAB] = {};
        for (int t = 0; t < NTAB; t++) traces[t] = proofs ? sb.block.as<const uint64_t>() + sb.off[t] : nullptr;
        return zkm_prove_segment(proofs ? c : nullptr, cfg, traces, b.lg, pub, npub, proofs, offsets_out, challenges, err);
    });
}

}  // extern "C"
