// io_calls.hip -- the rows of a segment's I/O syscalls expanded on the device from the bytes each call moves (include/zkm_hip.h "the I/O
// syscalls' rows from their bytes"): what the four data-moving helpers behind generate_syscall's own row push -- load_input
// (witness/operation.rs:1024-1067), commit (:1069-1099), verify (:991-1022) and load_preimage (:908-989) -- as ready-made rows for RAW
// steps.  A row holds its clock and up to eight channels of six cells; every cell is a function of the call's bytes, address and clock.
//
// Where a call's rows go and what each channel holds is stated once, in `place` below: zkm_io_calls_counts, zkm_io_calls_steps (masks,
// clocks, RAW indices) and the kernel all read it.  A call's length varies (one call may be half a segment, the next one row), so the work
// is divided by ROW: the host's walk computes the calls' row offsets and uploads them, and a workgroup finds the call of each of its rows
// by a search over them.
//
// k_io_calls: ONE launch for the calls of K segments (the segment is blockIdx.z; its descriptor is read from device memory, where it went
// up with the lists as the bootstrap's do -- a uniform read; zkm_io_calls_witness is the K = 1 case), a workgroup of 256 threads for
// ROWS_PER_WG consecutive rows of one segment.  The first ROWS_PER_WG lanes search the row offsets and put what their row needs (the
// call's kind, bytes, meta; the row's position, clock and channel count) into LDS.  Then all lanes walk the workgroup's span of the
// row-major block word by word, adjacent lanes on adjacent words with 8-byte stores: zeros, the clock, and the channel cells computed in
// place.  Every word is written, so no zero-fill pass comes in front; the kernel is write-only but for the calls' bytes, and its floor is
// the 2,072 bytes a row it has to write.
#include "calls_launch.h"
#include "calls_place_dev.h"

namespace {

using zkm_step::C_CH0;
using zkm_step::C_CLOCK;
using namespace zkm_calls;
constexpr unsigned CPU_W = ZKM_CPU_COLS, THREADS = 256, ROWS_PER_WG = 8;
static_assert(C_CLOCK + 1 == C_CH0 && C_CH0 + 48 <= CPU_W, "a row's clock and its 48 channel cells are 49 contiguous words");

// ---- the one statement of where things go, for a call of kind `kind` with L bytes (the host has refused the lengths a kind does not take)
namespace place = zkm_io_place;   // (calls_place_dev.h)

struct io_calls_args {
    const uint32_t* kinds;      // ncalls
    const uint8_t* data;
    const uint64_t* off;        // ncalls + 1
    const uint64_t* meta;       // ncalls x 4 {context, segment, address, timestamp of the first row}
    const uint64_t* row_off;    // ncalls + 1: where a call's rows start; strictly increasing (every call has a row)
    uint64_t* rows;
    uint64_t nrows;
    uint32_t ncalls;
    uint32_t nwg;               // the segment's own extent of the grid
};

// what a row needs of its call
struct row_info {
    const uint8_t* bytes;       // the call's bytes
    uint64_t L, ctx, seg, address, clock, j;
    uint32_t kind, channels;
};

// byte p of a call, 0 behind its end
__device__ __forceinline__ uint32_t byte_or_0(const uint8_t* __restrict__ b, uint64_t L, uint64_t p) { return p < L ? b[p] : 0u; }
// memory word w of the bytes from `at` on as the CPU holds it: the big-endian reading of its four bytes, right-padded with 0
__device__ __forceinline__ uint32_t be_word(const uint8_t* __restrict__ b, uint64_t L, uint64_t at) {
    return byte_or_0(b, L, at) << 24 | byte_or_0(b, L, at + 1) << 16 | byte_or_0(b, L, at + 2) << 8 | byte_or_0(b, L, at + 3);
}
// write word q of a preimage call: the content's length, then the content's words; a last word of n < 4 bytes as load_preimage builds it
// (:960-980): the bytes little-endian, | 1 << 8 n, | 0x80 << 24 if C % 32 + 4 > 32, byte-swapped -- which is the big-endian reading of the
// zero-padded bytes with 0x01 in byte n and 0x80 in byte 3
__device__ __forceinline__ uint32_t preimage_word(const uint8_t* __restrict__ b, uint64_t L, uint64_t q) {
    const uint64_t C = L - 32;
    if (q == 0) return (uint32_t)C;
    const uint64_t at = 4 * (q - 1), n = C - at;
    uint32_t v = be_word(b, L, 32 + at);
    if (n < 4) v |= (1u << (8 * (3 - n))) | (C % place::POSEIDON_RATE_BYTES + 4 > place::POSEIDON_RATE_BYTES ? 0x80u : 0u);
    return v;
}

// cell f of channel i of a row (cpu/columns/mod.rs MemoryChannelView: used, is_read, addr_context, addr_segment, addr_virtual, value)
__device__ __forceinline__ uint64_t chan_cell(const row_info& r, unsigned i, unsigned f) {
    if (f == 0) return 1;
    if (f == 2) return r.ctx;
    if (f == 3) return r.seg;
    const bool hash_row = r.kind == ZKM_IO_PREIMAGE && r.j == 0;
    if (f == 1) return r.kind != ZKM_IO_HINT_READ && (r.kind != ZKM_IO_PREIMAGE || hash_row);
    const uint64_t w = 8 * (r.j - place::lead_rows(r.kind)) + i;                  // the word among the call's (the hash row: i itself)
    if (f == 4) return hash_row ? place::PREIMAGE_HASH + 4 * i : r.address + 4 * w;
    if (r.kind == ZKM_IO_PREIMAGE) return hash_row ? be_word(r.bytes, r.L, 4 * i) : preimage_word(r.bytes, r.L, w);
    return be_word(r.bytes, r.L, 4 * w);
}

__global__ __launch_bounds__(THREADS) void k_io_calls(const io_calls_args* __restrict__ segs) {
    __shared__ row_info info[ROWS_PER_WG];
    const io_calls_args A = zkm_seg_desc(segs);   // (uniform: scalar loads)
    if (blockIdx.x >= A.nwg) return;
    const unsigned t = threadIdx.x;
    const uint64_t row0 = (uint64_t)blockIdx.x * ROWS_PER_WG;
    const unsigned nrows = A.nrows - row0 < ROWS_PER_WG ? (unsigned)(A.nrows - row0) : ROWS_PER_WG;
    if (t < nrows) {
        // the call k with row_off[k] <= row < row_off[k + 1]
        const uint64_t row = row0 + t;
        uint32_t lo = 0, hi = A.ncalls;   // the answer lies in [lo, hi)
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (A.row_off[mid] <= row) lo = mid;
            else hi = mid;
        }
        const uint32_t k = lo;
        row_info r;
        r.kind = A.kinds[k];
        r.bytes = A.data + A.off[k];
        r.L = A.off[k + 1] - A.off[k];
        r.ctx = A.meta[4 * k];
        r.seg = A.meta[4 * k + 1];
        r.address = A.meta[4 * k + 2];
        r.j = row - A.row_off[k];
        r.clock = place::row_clock(A.meta[4 * k + 3], r.j);
        r.channels = place::channels(r.kind, r.L, r.j);
        info[t] = r;
    }
    __syncthreads();
    // the workgroup's span of the block, word by word: adjacent lanes store adjacent words
    uint64_t* __restrict__ out = A.rows + row0 * CPU_W;
    for (unsigned w = t; w < nrows * CPU_W; w += THREADS) {
        const unsigned r = w / CPU_W, col = w % CPU_W;
        uint64_t v = 0;
        if (col == C_CLOCK) v = info[r].clock;
        else if (col >= C_CH0 && col < C_CH0 + 48) {
            const unsigned ch = (col - C_CH0) / 6, f = (col - C_CH0) % 6;
            if (ch < info[r].channels) v = chan_cell(info[r], ch, f);
        }
        out[w] = v;
    }
}

// ---- the host's refusals, naming the list and the call's position (they throw the bare message)
const char* const KIND_NAME[place::NKINDS] = {"hint read", "commit", "verify", "preimage"};

struct totals { uint64_t rows, mem; };

// kinds and offsets: host memory, known kinds, offsets that do not decrease, the lengths each kind takes.  Returns the totals, and where
// each call's rows start (ncalls + 1 entries) if asked.
totals check_calls(const uint32_t* kinds, const uint64_t* off, size_t n, std::vector<uint64_t>* row_off) {
    totals sum{0, 0};
    if (n && !kinds) throw std::runtime_error("kinds: NULL with a count of " + dec(n));
    if (n && !off) throw std::runtime_error("data_off: NULL with a count of " + dec(n));
    if (n && zkm_is_device_ptr(kinds)) throw std::runtime_error("kinds: device memory (the kinds size the output: they must be host memory)");
    if (n && zkm_is_device_ptr(off)) throw std::runtime_error("data_off: device memory (the offsets size the output: they must be host memory)");
    if (row_off) row_off->assign(n + 1, 0);
    for (size_t k = 0; k < n; k++) {
        if (kinds[k] >= place::NKINDS)
            throw std::runtime_error("kinds: call " + dec(k) + ": unknown kind " + dec(kinds[k]) + " (ZKM_IO_HINT_READ, _COMMIT, _VERIFY and _PREIMAGE are 0 to 3)");
        const std::string at = "data_off: call " + dec(k) + ": ";
        if (off[k + 1] < off[k]) throw std::runtime_error(at + "the offsets decrease (" + dec(off[k]) + " then " + dec(off[k + 1]) + ")");
        const uint64_t L = off[k + 1] - off[k];
        if (kinds[k] == ZKM_IO_VERIFY && L != 32) throw std::runtime_error(at + "a verify call of " + dec(L) + " bytes (the claim digest is 32)");
        if (kinds[k] == ZKM_IO_COMMIT && L % 4)
            throw std::runtime_error(at + "a commit call of " + dec(L) + " bytes is not a multiple of 4 (the call reads whole memory words: hand over the words)");
        if (kinds[k] == ZKM_IO_PREIMAGE && L < 32) throw std::runtime_error(at + "a preimage call of " + dec(L) + " bytes is shorter than its 32 hash bytes");
        sum.rows += place::rows(kinds[k], L);
        sum.mem += place::mem(kinds[k], L);
        if (row_off) (*row_off)[k + 1] = sum.rows;
    }
    return sum;
}

void check_meta(const uint32_t* kinds, const uint64_t* off, const uint64_t* meta, size_t n) {
    if (n && !meta) throw std::runtime_error("meta: NULL with a count of " + dec(n));
    // (a list in device memory is not read by the host: see the header)
    for (size_t k = 0; k < n && !zkm_is_device_ptr(meta); k++) {
        const uint64_t* m = meta + 4 * k;
        const uint64_t L = off[k + 1] - off[k];
        const std::string at = "meta: call " + dec(k) + ": ";
        if (m[0] >= LIM) throw std::runtime_error(at + "context " + dec(m[0]) + " does not fit in 32 bits");
        if (m[1] >= LIM) throw std::runtime_error(at + "segment " + dec(m[1]) + " does not fit in 32 bits");
        if (kinds[k] == ZKM_IO_PREIMAGE && m[2] != place::PREIMAGE_MAP)
            throw std::runtime_error(at + "address " + hex(m[2]) + " of a preimage call is not 0x31000000");
        if (m[2] % 4) throw std::runtime_error(at + "address " + hex(m[2]) + " is not aligned to 4 bytes");
        if (m[2] >= LIM || place::last_address(kinds[k], L, m[2]) >= LIM)
            throw std::runtime_error(at + "address " + hex(m[2]) + ": the last word of the " + KIND_NAME[kinds[k]] + " (" + dec(place::words(kinds[k], L)) +
                                     " words) does not fit in 32 bits");
        if (m[3] % 10) throw std::runtime_error(at + "timestamp " + dec(m[3]) + " is not a multiple of 10 (NUM_CHANNELS)");
    }
}

// the bytes go up from the first call's offset on, so the offsets that go up count from there
void rebase_offsets(zkm_io_job& j) {
    j.off_up.assign(j.off, j.off + j.n + 1);
    if (!zkm_is_device_ptr(j.data))
        for (uint64_t& o : j.off_up) o -= j.off[0];
}

// what the K-segment launcher takes of this kind (calls_launch.h)
struct io_kind {
    using job = zkm_io_job;
    using args = io_calls_args;
    static constexpr const char *name = "zkm_io_calls_launch", *scope = "io_calls/rows";
    static constexpr auto kernel = k_io_calls;
    static constexpr unsigned threads = THREADS;
    // a job's five lists: the kinds, the bytes, the offsets, the meta, the row offsets; which of them go up
    static std::array<zkm_calls_list, 5> lists(const job& j) {
        const size_t n = j.n, first = n ? j.off[0] : 0, nbytes = n ? j.off[n] - first : 0;
        const bool data_up = !zkm_is_device_ptr(j.data);
        return {{{j.kinds, 4 * n, !zkm_is_device_ptr(j.kinds)},
                 {data_up && j.data ? j.data + first : j.data, nbytes, data_up},
                 {j.off_up.data(), n ? 8 * (n + 1) : 0, true},
                 {j.meta, 32 * n, !zkm_is_device_ptr(j.meta)},
                 {j.row_off.data(), n ? 8 * (n + 1) : 0, true}}};
    }
    static args make(const job& j, const void* const* dev) {
        return {(const uint32_t*)dev[0], (const uint8_t*)dev[1], (const uint64_t*)dev[2], (const uint64_t*)dev[3], (const uint64_t*)dev[4],
                j.rows, j.nrows, (uint32_t)j.n, (uint32_t)extent(j)};
    }
    static size_t extent(const job& j) { return (j.nrows + ROWS_PER_WG - 1) / ROWS_PER_WG; }   // a workgroup for ROWS_PER_WG rows
    static size_t sparse_rows(const job&) { return 0; }   // (the kernel writes every word)
};

}  // namespace

void zkm_io_calls_check(zkm_io_job& j) {
    const totals sum = check_calls(j.kinds, j.off, j.n, &j.row_off);
    check_meta(j.kinds, j.off, j.meta, j.n);
    j.nrows = sum.rows, j.nmem = sum.mem;
    j.off_up.clear();
    if (j.n == 0) return;
    const size_t first = j.off[0], nbytes = j.off[j.n] - first;
    if (nbytes && !j.data) throw std::runtime_error("data: NULL with " + dec(nbytes) + " bytes to read");
    if (sum.rows > LIM) throw std::runtime_error(dec(sum.rows) + " rows: a RAW index does not fit in 32 bits");
    if (j.n > 0x7FFFFFFF) throw std::runtime_error("2^31 or more calls");
    rebase_offsets(j);
}
size_t zkm_io_calls_scratch(const zkm_io_job* j, size_t nseg) { return zkm_calls_layout<io_kind>(j, nseg, nullptr); }
void zkm_io_calls_launch(zkm_ctx* c, const zkm_io_job* j, size_t nseg, char* sb, zkm_calls_hold& hold, hipStream_t stream) {
    zkm_calls_queue<io_kind>(c, stream ? stream : c->stream, j, nseg, sb, hold, false);
}

extern "C" {

int zkm_io_calls_counts(const uint32_t* kinds, const uint64_t* data_off, size_t ncalls, size_t* cpu_rows, size_t* memory_ops, char** err) {
    return zkm_api("zkm_io_calls_counts", err, [&] {
        totals sum;
        try {
            sum = check_calls(kinds, data_off, ncalls, nullptr);
        } catch (const std::exception& e) {
            throw std::runtime_error(std::string("zkm_io_calls_counts: ") + e.what());
        }
        if (cpu_rows) *cpu_rows = sum.rows;
        if (memory_ops) *memory_ops = sum.mem;
    });
}

int zkm_io_calls_steps(const uint32_t* kinds, const uint64_t* data_off, const uint64_t* meta, size_t ncalls, size_t raw_base,
                       zkm_cpu_step* steps_out, uint64_t* clocks_out, char** err) {
    return zkm_api("zkm_io_calls_steps", err, [&] {
        auto refuse = [](const std::string& m) { throw std::runtime_error("zkm_io_calls_steps: " + m); };
        std::vector<uint64_t> row_off;
        totals sum;
        try {
            sum = check_calls(kinds, data_off, ncalls, &row_off);
            check_meta(kinds, data_off, meta, ncalls);
        } catch (const std::exception& e) {
            refuse(e.what());
        }
        if (ncalls && zkm_is_device_ptr(meta)) refuse("meta: device memory (the clocks are read on the host)");
        if (sum.rows && (!steps_out || !clocks_out)) refuse("null argument");
        if (raw_base >= LIM || raw_base + sum.rows > LIM) refuse("raw_base " + dec(raw_base) + ": a RAW index does not fit in 32 bits");
        for (size_t k = 0; k < ncalls; k++) {
            const uint64_t L = data_off[k + 1] - data_off[k];
            for (size_t j = 0; j < place::rows(kinds[k], L); j++) {
                const zkm_row_rec r = place::row_rec(kinds, data_off, meta, k, j);
                steps_out[row_off[k] + j] = raw_step(raw_base + row_off[k] + j, r.mask);
                clocks_out[row_off[k] + j] = r.clock;
            }
        }
    });
}

int zkm_io_calls_witness(zkm_ctx* c, const uint32_t* kinds, const uint8_t* data, const uint64_t* data_off, const uint64_t* meta, size_t ncalls,
                         uint64_t* raw_rows_out_dev, char** err) {
    return zkm_api("zkm_io_calls_witness", err, [&] {
        auto refuse = [](const std::string& m) { throw std::runtime_error("zkm_io_calls_witness: " + m); };
        // every refusal first, on the host: the lists, the output, then the context
        zkm_io_job j;
        j.kinds = kinds, j.data = data, j.off = data_off, j.meta = meta, j.n = ncalls, j.rows = raw_rows_out_dev;
        try {
            zkm_io_calls_check(j);
        } catch (const std::exception& e) {
            refuse(e.what());
        }
        if (ncalls == 0) {
            if (!c) refuse("null argument");
            return;
        }
        if (!raw_rows_out_dev) refuse("raw_rows_out_dev: NULL with " + dec(j.nrows) + " rows to write");
        if ((uintptr_t)raw_rows_out_dev & 7) refuse("raw_rows_out_dev is not aligned to its words (8 bytes)");
        if (!c) refuse("null argument");
        ZKM_HIP_CHECK(hipSetDevice(c->device));
        zkm_calls_one<io_kind>(c, j);
    });
}

}  // extern "C"
