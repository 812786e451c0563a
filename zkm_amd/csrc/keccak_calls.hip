// keccak_calls.hip -- the SYSKECCAK precompile calls of a segment expanded on the device from the lists the caller already hands over for
// the KeccakSponge table (include/zkm_hip.h "SYSKECCAK precompile calls from their input bytes"): the CPU rows of generate_keccak
// (witness/operation.rs:1101-1181) as ready-made rows for RAW steps, and what keccak_sponge_log (witness/util.rs:471-557, with
// xor_into_sponge, :724-741) pushes -- the sponge's memory reads, the XORs of every absorption, the Keccak-f inputs and timestamps.
//
// Where a call's rows and operations go is stated once, in `place` below: zkm_keccak_calls_counts, zkm_keccak_calls_steps (masks, clocks,
// RAW indices) and the kernel's indexing all read it.  A call's length varies, so where call k starts in each list is a prefix sum over the
// earlier calls; the host computes the four sums a call from input_off and uploads them with the lists.
//
// k_keccak_calls: ONE launch for the calls of K segments (the segment is blockIdx.z; its descriptor is read from device memory, where it
// went up with the lists as the bootstrap's do -- a uniform read; zkm_keccak_calls_witness is the K = 1 case), one workgroup of 256
// threads a call.  The sequential part -- B absorptions and permutations -- is run by one lane, block by block: all lanes stage the
// padded 136-byte block in LDS, lane 0 XORs it into the state, stores the state (the Keccak-f input, an output anyway) and permutes.  The
// digest goes into LDS.  After the barrier all lanes write: the 49 contiguous clock and channel cells of a row by adjacent lanes, every
// list by adjacent lanes on adjacent words; an XOR's lhs is the stored state word ^ the block word.  The row block is zeroed by one
// memset before the launch, so only the cells a row sets are stored.
#include "calls_launch.h"
#include "calls_place_dev.h"
#include "hash_constants_dev.h"

namespace {

using zkm_step::C_CH0;
using zkm_step::C_CLOCK;
using zkm_step::C_GEN;
using zkm_step::C_IS_KECCAK_SPONGE;
using zkm_step::chan_cell;
using zkm_step::read_word;
using namespace zkm_calls;
constexpr unsigned CPU_W = ZKM_CPU_COLS, THREADS = 256;
constexpr uint32_t OP_XOR = 2;   // zkm_logic_trace's code
constexpr uint64_t FLAG = ZKM_SPONGE_BYTE_ADDRESSED, TAIL = ZKM_SPONGE_PADDED_TAIL;

// ---- the one statement of where things go, for a call of L >= 1 input bytes
namespace place = zkm_keccak_place;   // (calls_place_dev.h)

using call_base = zkm_keccak_base;   // where a call starts in each list: the sums of the earlier calls' counts

struct keccak_calls_args {
    const uint8_t* inputs;
    const uint64_t* off;         // ncalls + 1
    const uint64_t* meta;        // ncalls x 4 {context, segment, address of word 0 | FLAG (| TAIL), timestamp of the sponge row}
    const uint64_t* digest_addr; // ncalls
    const call_base* base;       // ncalls
    uint64_t *rows, *mem, *perm_in, *perm_ts;
    uint32_t* logic;
    uint32_t ncalls;             // the segment's own extent of the grid
};

// byte `pos` of the padded message: the input, then pad10*1 up to the end of the last block
__device__ __forceinline__ uint32_t padded_byte(const uint8_t* __restrict__ msg, size_t L, size_t pos) {
    if (pos < L) return msg[pos];
    return (pos == L ? 0x01u : 0u) | (pos == place::RATE * place::blocks(L) - 1 ? 0x80u : 0u);
}
// memory word w < W of the call as the CPU reads it: the big-endian reading of its four bytes in the padded message.  A word that
// lies inside the input is loaded as it is; the last word of a length that is no multiple of 4 goes byte by byte through padded_byte,
// so no lane loads a byte at or beyond msg + L (the next call's bytes, or the end of the buffer, lie there)
__device__ __forceinline__ uint32_t be_word(const uint8_t* __restrict__ msg, size_t L, size_t w) {
    if (4 * w + 4 <= L) return (uint32_t)msg[4 * w] << 24 | (uint32_t)msg[4 * w + 1] << 16 | (uint32_t)msg[4 * w + 2] << 8 | msg[4 * w + 3];
    return padded_byte(msg, L, 4 * w) << 24 | padded_byte(msg, L, 4 * w + 1) << 16 | padded_byte(msg, L, 4 * w + 2) << 8 | padded_byte(msg, L, 4 * w + 3);
}
__device__ __forceinline__ uint32_t bswap(uint32_t x) { return __builtin_bswap32(x); }

__global__ __launch_bounds__(THREADS) void k_keccak_calls(const keccak_calls_args* __restrict__ segs) {
    __shared__ uint64_t block[place::RATE / 8];   // the padded block being absorbed
    __shared__ uint32_t digest[8];                // the digest's bytes as little-endian words
    const keccak_calls_args A = zkm_seg_desc(segs);   // (uniform: scalar loads)
    if (blockIdx.x >= A.ncalls) return;
    const unsigned t = threadIdx.x;
    const size_t k = blockIdx.x;
    const uint8_t* __restrict__ msg = A.inputs + A.off[k];
    const size_t L = A.off[k + 1] - A.off[k], W = place::words(L), R = place::read_rows(L), B = place::blocks(L);
    const call_base at = A.base[k];
    const uint64_t ctx = A.meta[4 * k], seg = A.meta[4 * k + 1], addr = A.meta[4 * k + 2] & ~(FLAG | TAIL), ts = A.meta[4 * k + 3], S = ts / 10;
    const uint64_t daddr = A.digest_addr[k];
    uint64_t* __restrict__ perm_in = A.perm_in + place::STATE * at.perm;

    // ---- the sponge, block by block: lane 0 holds the state
    uint64_t st[place::STATE];
#pragma unroll
    for (unsigned i = 0; i < place::STATE; i++) st[i] = 0;
    for (size_t b = 0; b < B; b++) {
        if (t < place::RATE) ((uint8_t*)block)[t] = (uint8_t)padded_byte(msg, L, place::RATE * b + t);
        __syncthreads();
        if (t == 0) {
#pragma unroll
            for (unsigned i = 0; i < place::RATE / 8; i++) st[i] ^= block[i];
#pragma unroll
            for (unsigned i = 0; i < place::STATE; i++) perm_in[place::STATE * b + i] = st[i];
            keccakf_dev(st);
        }
        __syncthreads();
    }
    if (t == 0) {
#pragma unroll
        for (unsigned i = 0; i < 4; i++) {
            digest[2 * i] = (uint32_t)st[i];
            digest[2 * i + 1] = (uint32_t)(st[i] >> 32);
        }
    }
    __syncthreads();

    // ---- the read rows: the clock, then the six cells of every channel that reads a word (64 slots a row, 49 cells)
    for (size_t j = t; j < R * 64; j += THREADS) {
        const size_t r = j >> 6;
        const unsigned cell = j & 63;
        if (cell > 48) continue;
        uint64_t v = place::row_clock(S, L, r);
        if (cell) {
            const unsigned ch = (cell - 1) / 6, f = (cell - 1) % 6;
            if (ch >= place::read_channels(L, r)) continue;
            const size_t w = 8 * r + ch;
            v = chan_cell(f, true, ctx, seg, addr + 4 * w, be_word(msg, L, w));
        }
        A.rows[(at.row + r) * CPU_W + C_CLOCK + cell] = v;
    }
    // the sponge row: the flag, the clock, context / segment / address of the final block's first word / length in the values of
    // channels 0-3, general.khash.value = the digest's words in reverse
    if (t < 14) {
        uint64_t* row = A.rows + (at.row + place::sponge_row(L)) * CPU_W;
        const size_t fw = place::final_word(L);
        if (t < 8) row[C_GEN + t] = bswap(digest[7 - t]);
        else if (t == 8) row[C_IS_KECCAK_SPONGE] = 1;
        else if (t == 9) row[C_CLOCK] = place::row_clock(S, L, place::sponge_row(L));
        else row[C_CH0 + 6 * (t - 10) + 5] = t == 10 ? ctx : t == 11 ? seg : t == 12 ? (fw < W ? addr + 4 * fw : 0) : (uint64_t)L;
    }
    // the write row: eight writes of the digest's words
    if (t >= 64 && t < 64 + 49) {
        const unsigned cell = t - 64;
        uint64_t v = place::row_clock(S, L, place::write_row(L));
        if (cell) {
            const unsigned ch = (cell - 1) / 6, f = (cell - 1) % 6;
            v = chan_cell(f, false, ctx, seg, daddr + 4 * ch, bswap(digest[ch]));
        }
        A.rows[(at.row + place::write_row(L)) * CPU_W + C_CLOCK + cell] = v;
    }
    // the sponge's reads: one a byte, of the word that holds it (keccak_sponge_log), six words a read
    uint64_t* __restrict__ mem = A.mem + 6 * at.mem;
    for (size_t j = t; j < 6 * place::mem(L); j += THREADS) {
        const size_t w = j / 24;
        mem[j] = read_word((unsigned)(j % 6), ctx, seg, addr + 4 * w, ts, be_word(msg, L, w));
    }
    // the 34 XORs of every absorption (xor_into_sponge), three words an operation: the state before = the stored state ^ the block
    uint32_t* __restrict__ logic = A.logic + 3 * at.logic;
    for (size_t j = t; j < 3 * place::logic(L); j += THREADS) {
        const size_t op = j / 3, b = op / place::RATE_U32;
        const unsigned f = (unsigned)(j % 3), i = (unsigned)(op % place::RATE_U32);
        uint32_t rhs = 0;
#pragma unroll
        for (unsigned q = 0; q < 4; q++) rhs |= padded_byte(msg, L, place::RATE * b + 4 * i + q) << (8 * q);
        const uint32_t after = (uint32_t)(perm_in[place::STATE * b + i / 2] >> (32 * (i & 1)));
        logic[j] = f == 0 ? OP_XOR : f == 1 ? after ^ rhs : rhs;
    }
    for (size_t b = t; b < B; b += THREADS) A.perm_ts[at.perm + b] = ts;
}

// ---- the host's refusals, naming the list and the call's position (they throw the bare message)
// the offsets: host memory, increasing, every length positive, and a multiple of 4 unless the call's meta carries TAIL (`meta`: the
// metas if the host may read them, else null -- then no call is flagged).  Returns the totals, and the sums a call if asked.
call_base check_offsets(const uint64_t* off, const uint64_t* meta, size_t n, std::vector<call_base>* bases) {
    call_base sum{0, 0, 0, 0};
    if (n && !off) throw std::runtime_error("input_off: NULL with a count of " + dec(n));
    if (n && zkm_is_device_ptr(off)) throw std::runtime_error("input_off: device memory (the offsets size the outputs: they must be host memory)");
    if (n && meta && zkm_is_device_ptr(meta)) meta = nullptr;
    if (bases) bases->resize(n);
    for (size_t k = 0; k < n; k++) {
        const std::string at = "input_off: call " + dec(k) + ": ";
        if (off[k + 1] < off[k]) throw std::runtime_error(at + "the offsets do not increase (" + dec(off[k]) + " then " + dec(off[k + 1]) + ")");
        const uint64_t L = off[k + 1] - off[k];
        if (L == 0 || (L % 4 && !(meta && meta[4 * k + 2] & TAIL)))
            throw std::runtime_error(at + "length " + dec(L) + " is not a positive multiple of 4 (the other bytes of the last memory word follow from no list: "
                                          "such a call travels as RAW rows beside a sponge operation with ZKM_SPONGE_BYTE_ADDRESSED)");
        if (bases) (*bases)[k] = sum;
        sum.row += place::rows(L);
        sum.mem += place::mem(L);
        sum.logic += place::logic(L);
        sum.perm += place::blocks(L);
    }
    return sum;
}

void check_meta(const uint64_t* off, const uint64_t* meta, size_t n) {
    if (n && !meta) throw std::runtime_error("meta: NULL with a count of " + dec(n));
    // (a list in device memory is not read by the host: see the header)
    for (size_t k = 0; k < n && !zkm_is_device_ptr(meta); k++) {
        const uint64_t* m = meta + 4 * k;
        const uint64_t L = off[k + 1] - off[k], W = place::words(L), base = m[2] & ~(FLAG | TAIL);
        const std::string at = "meta: call " + dec(k) + ": ";
        if (m[0] >= LIM) throw std::runtime_error(at + "context " + dec(m[0]) + " does not fit in 32 bits");
        if (m[1] >= LIM) throw std::runtime_error(at + "segment " + dec(m[1]) + " does not fit in 32 bits");
        if (!(m[2] & FLAG)) throw std::runtime_error(at + "virt_base " + hex(m[2]) + " lacks ZKM_SPONGE_BYTE_ADDRESSED (a call reads one memory word every 4 bytes)");
        if (base >= LIM || base + 4 * (W - 1) >= LIM) throw std::runtime_error(at + "address of word 0 " + hex(base) + ": word " + dec(W - 1) + " does not fit in 32 bits");
        if (m[3] % 10) throw std::runtime_error(at + "timestamp " + dec(m[3]) + " is not a multiple of 10 (NUM_CHANNELS)");
        if (m[3] / 10 < place::read_rows(L)) throw std::runtime_error(at + "timestamp " + dec(m[3]) + " puts the first read row before clock 0");
    }
}

void check_digest_addrs(const uint64_t* addrs, size_t n) {
    if (n && !addrs) throw std::runtime_error("digest_addrs: NULL with a count of " + dec(n));
    for (size_t k = 0; k < n && !zkm_is_device_ptr(addrs); k++)
        if (addrs[k] >= LIM || addrs[k] + 28 >= LIM)
            throw std::runtime_error("digest_addrs: call " + dec(k) + ": address " + hex(addrs[k]) + ": the digest's eighth word does not fit in 32 bits");
}

// the input bytes go up from the first call's offset on, so the offsets that go up count from there
void rebase_offsets(zkm_keccak_job& j) {
    j.off_up.assign(j.off, j.off + j.n + 1);
    if (!zkm_is_device_ptr(j.inputs))
        for (uint64_t& o : j.off_up) o -= j.off[0];
}

// what the K-segment launcher takes of this kind (calls_launch.h)
struct keccak_kind {
    using job = zkm_keccak_job;
    using args = keccak_calls_args;
    static constexpr const char *name = "zkm_keccak_calls_launch", *scope = "keccak_calls/rows_lists";
    static constexpr auto kernel = k_keccak_calls;
    static constexpr unsigned threads = THREADS;
    // a job's five lists: the bytes, the offsets, the meta, the digest addresses, the sums a call; which of them go up
    static std::array<zkm_calls_list, 5> lists(const job& j) {
        const size_t n = j.n, first = n ? j.off[0] : 0, nbytes = n ? j.off[n] - first : 0;
        const bool inputs_up = !zkm_is_device_ptr(j.inputs);
        return {{{inputs_up && j.inputs ? j.inputs + first : j.inputs, nbytes, inputs_up},
                 {j.off_up.data(), n ? 8 * (n + 1) : 0, true},
                 {j.meta, 32 * n, !zkm_is_device_ptr(j.meta)},
                 {j.digest_addrs, 8 * n, !zkm_is_device_ptr(j.digest_addrs)},
                 {j.bases.data(), sizeof(call_base) * n, true}}};
    }
    static args make(const job& j, const void* const* dev) {
        return {(const uint8_t*)dev[0], (const uint64_t*)dev[1], (const uint64_t*)dev[2], (const uint64_t*)dev[3], (const call_base*)dev[4],
                j.rows, j.mem, j.perm_in, j.perm_ts, j.logic, (uint32_t)j.n};
    }
    static size_t extent(const job& j) { return j.n; }   // a workgroup a call
    static size_t sparse_rows(const job& j) { return j.nrows; }
};

// the four totals, for zkm_keccak_calls_counts (no metas) and zkm_keccak_calls_counts_meta: one set of refusals under the first's name,
// which the segment entry points pass on as it is
void counts(const uint64_t* off, const uint64_t* meta, size_t n, size_t* cpu_rows, size_t* memory_ops, size_t* logic_ops, size_t* keccak_perms) {
    call_base sum;
    try {
        sum = check_offsets(off, meta, n, nullptr);
    } catch (const std::exception& e) {
        throw std::runtime_error(std::string("zkm_keccak_calls_counts: ") + e.what());
    }
    if (cpu_rows) *cpu_rows = sum.row;
    if (memory_ops) *memory_ops = sum.mem;
    if (logic_ops) *logic_ops = sum.logic;
    if (keccak_perms) *keccak_perms = sum.perm;
}

}  // namespace

void zkm_keccak_calls_check(zkm_keccak_job& j) {
    const call_base sum = check_offsets(j.off, j.meta, j.n, &j.bases);
    check_meta(j.off, j.meta, j.n);
    check_digest_addrs(j.digest_addrs, j.n);
    if (j.n && !j.inputs) throw std::runtime_error("inputs: NULL with a count of " + dec(j.n));
    if (j.n > 0x7FFFFFFF) throw std::runtime_error("2^31 or more calls");
    j.nrows = sum.row, j.nmem = sum.mem, j.nlogic = sum.logic, j.nperm = sum.perm;
    j.off_up.clear();
    if (j.n) rebase_offsets(j);
}
size_t zkm_keccak_calls_scratch(const zkm_keccak_job* j, size_t nseg) { return zkm_calls_layout<keccak_kind>(j, nseg, nullptr); }
void zkm_keccak_calls_launch(zkm_ctx* c, const zkm_keccak_job* j, size_t nseg, char* sb, zkm_calls_hold& hold, bool zero_rows, hipStream_t stream) {
    zkm_calls_queue<keccak_kind>(c, stream ? stream : c->stream, j, nseg, sb, hold, zero_rows);
}

extern "C" {

int zkm_keccak_calls_counts(const uint64_t* input_off, size_t ncalls, size_t* cpu_rows, size_t* memory_ops, size_t* logic_ops,
                            size_t* keccak_perms, char** err) {
    return zkm_api("zkm_keccak_calls_counts", err, [&] { counts(input_off, nullptr, ncalls, cpu_rows, memory_ops, logic_ops, keccak_perms); });
}

int zkm_keccak_calls_counts_meta(const uint64_t* input_off, const uint64_t* meta, size_t ncalls, size_t* cpu_rows, size_t* memory_ops,
                                 size_t* logic_ops, size_t* keccak_perms, char** err) {
    return zkm_api("zkm_keccak_calls_counts_meta", err, [&] { counts(input_off, meta, ncalls, cpu_rows, memory_ops, logic_ops, keccak_perms); });
}

int zkm_keccak_calls_steps(const uint64_t* input_off, const uint64_t* meta, size_t ncalls, size_t raw_base, zkm_cpu_step* steps_out,
                           uint64_t* clocks_out, char** err) {
    return zkm_api("zkm_keccak_calls_steps", err, [&] {
        auto refuse = [](const std::string& m) { throw std::runtime_error("zkm_keccak_calls_steps: " + m); };
        std::vector<call_base> bases;
        call_base sum;
        try {
            sum = check_offsets(input_off, meta, ncalls, &bases);
            check_meta(input_off, meta, ncalls);
        } catch (const std::exception& e) {
            refuse(e.what());
        }
        if (ncalls && zkm_is_device_ptr(meta)) refuse("meta: device memory (the clocks are read on the host)");
        if (sum.row && (!steps_out || !clocks_out)) refuse("null argument");
        if (raw_base >= LIM || raw_base + sum.row > LIM) refuse("raw_base " + dec(raw_base) + ": a RAW index does not fit in 32 bits");
        for (size_t k = 0; k < ncalls; k++) {
            const uint64_t L = input_off[k + 1] - input_off[k];
            for (size_t j = 0; j < place::rows(L); j++) {
                const zkm_row_rec r = place::row_rec(input_off, meta, k, j);
                steps_out[bases[k].row + j] = raw_step(raw_base + bases[k].row + j, r.mask);
                clocks_out[bases[k].row + j] = r.clock;
            }
        }
    });
}

int zkm_keccak_calls_witness(zkm_ctx* c, const uint8_t* inputs, const uint64_t* input_off, const uint64_t* meta, const uint64_t* digest_addrs,
                             size_t ncalls, uint64_t* raw_rows_out_dev, uint64_t* memory_ops_out_dev, uint32_t* logic_ops_out_dev,
                             uint64_t* keccak_inputs_out_dev, uint64_t* keccak_timestamps_out_dev, char** err) {
    return zkm_api("zkm_keccak_calls_witness", err, [&] {
        auto refuse = [](const std::string& m) { throw std::runtime_error("zkm_keccak_calls_witness: " + m); };
        // every refusal first, on the host: the lists, the outputs, then the context
        zkm_keccak_job j;
        j.inputs = inputs, j.off = input_off, j.meta = meta, j.digest_addrs = digest_addrs, j.n = ncalls;
        j.rows = raw_rows_out_dev, j.mem = memory_ops_out_dev, j.logic = logic_ops_out_dev, j.perm_in = keccak_inputs_out_dev, j.perm_ts = keccak_timestamps_out_dev;
        try {
            zkm_keccak_calls_check(j);
        } catch (const std::exception& e) {
            refuse(e.what());
        }
        if (ncalls == 0) {
            if (!c) refuse("null argument");
            return;
        }
        if (!raw_rows_out_dev) refuse("raw_rows_out_dev: NULL with " + dec(j.nrows) + " rows to write");
        if (!memory_ops_out_dev) refuse("memory_ops_out_dev: NULL with " + dec(j.nmem) + " operations to write");
        if (!logic_ops_out_dev) refuse("logic_ops_out_dev: NULL with " + dec(j.nlogic) + " operations to write");
        if (!keccak_inputs_out_dev) refuse("keccak_inputs_out_dev: NULL with " + dec(j.nperm) + " permutations to write");
        if (!keccak_timestamps_out_dev) refuse("keccak_timestamps_out_dev: NULL with " + dec(j.nperm) + " permutations to write");
        if (((uintptr_t)raw_rows_out_dev | (uintptr_t)memory_ops_out_dev | (uintptr_t)keccak_inputs_out_dev | (uintptr_t)keccak_timestamps_out_dev) & 7 ||
            (uintptr_t)logic_ops_out_dev & 3)
            refuse("an output is not aligned to its words (8 bytes; 4 for the logic operations)");
        if (!c) refuse("null argument");
        ZKM_HIP_CHECK(hipSetDevice(c->device));
        zkm_calls_one<keccak_kind>(c, j);
    });
}

}  // extern "C"
