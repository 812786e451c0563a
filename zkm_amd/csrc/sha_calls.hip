// sha_calls.hip -- the SHA-256 precompile calls of a segment expanded on the device from the lists the caller already hands over for the
// sponge tables (include/zkm_hip.h "SHA-256 precompile calls from their inputs"): the CPU rows of generate_sha_extend /
// generate_sha_compress (witness/operation.rs:1183-1285, :1298-1458) as ready-made rows for RAW steps, and what sha_extend_sponge_log /
// sha_compress_sponge_log (witness/util.rs:559-694) push -- the sponge's memory reads, the logic operations, the ShaExtend inputs and
// timestamps.
//
// Where a call's rows and operations go is stated once, in `place` below: zkm_sha_calls_counts, zkm_sha_calls_steps (masks, clocks, RAW
// indices) and the kernel's indexing all read it.
//
// k_sha_calls: ONE launch for all calls of both kinds of K segments (the segment is blockIdx.z; its descriptor is read from device
// memory, where it went up with the lists as the bootstrap's do -- a uniform read; zkm_sha_calls_witness is the K = 1 case), one
// workgroup of 256 threads a call (workgroups [0, E) extend, [E, E + C) compress: the branch is uniform in a workgroup, the calls are
// independent, and a second launch would only add its gap).  The sequential part -- 48 schedule steps, or 64 rounds of eight words -- is
// run once by one lane into LDS; after the barrier all lanes write from LDS: the 49 contiguous clock and channel cells of a row by
// adjacent lanes, every list by adjacent lanes on adjacent words. The row block is zeroed by one memset before the launch, so only the
// cells a row sets are stored.
#include "calls_launch.h"
#include "calls_place_dev.h"
#include "hash_constants_dev.h"

namespace {

using zkm_step::C_CH0;
using zkm_step::C_CLOCK;
using zkm_step::C_GEN;
using zkm_step::C_IS_SHA_COMPRESS_SPONGE;
using zkm_step::C_IS_SHA_EXTEND_SPONGE;
using zkm_step::chan_cell;
using zkm_step::read_word;
using namespace zkm_calls;
constexpr unsigned CPU_W = ZKM_CPU_COLS, THREADS = 256;
constexpr uint32_t OP_AND = 0, OP_XOR = 2;   // zkm_logic_trace's codes

// ---- the one statement of where things go.  E extend calls, then C compress calls, in every list.
namespace place = zkm_sha_place;   // (calls_place_dev.h)

struct sha_calls_args {
    const uint32_t* w16;     // E x 16
    const uint64_t* emeta;   // E x 4 {context, segment, address of w[0], timestamp of round 0's sponge row}
    const uint32_t *hx, *w;  // C x 8, C x 64
    const uint64_t* cmeta;   // C x 8 {context, segment, address of hx[0], timestamp, address of w[0], segment of w, context of w, unused}
    size_t E, C;
    uint64_t *rows, *mem, *ext_ts;
    uint32_t *logic, *ext_in;
};

__device__ __forceinline__ uint32_t ror(uint32_t x, unsigned r) { return (x >> r) | (x << (32 - r)); }

// schedule word indices a round i reads, in the generator's order: w[i-15], w[i-2], w[i-16], w[i-7]
__device__ __forceinline__ unsigned ext_src(unsigned i, unsigned q) { return i - (q == 0 ? 15 : q == 1 ? 2 : q == 2 ? 16 : 7); }

__device__ void extend_call(const sha_calls_args& A, size_t e, uint32_t* w) {
    const unsigned t = threadIdx.x;
    if (t < 16) w[t] = A.w16[16 * e + t];
    __syncthreads();
    if (t == 0)
        for (unsigned i = 16; i < 64; i++) {
            const uint32_t w15 = w[i - 15], w2 = w[i - 2];
            w[i] = (ror(w2, 17) ^ ror(w2, 19) ^ (w2 >> 10)) + w[i - 16] + (ror(w15, 7) ^ ror(w15, 18) ^ (w15 >> 3)) + w[i - 7];
        }
    __syncthreads();
    const uint64_t ctx = A.emeta[4 * e], seg = A.emeta[4 * e + 1], addr = A.emeta[4 * e + 2], ts = A.emeta[4 * e + 3], S = ts / 10;
    // the read rows: clock, then channels 0-3 reading w[i-15], w[i-2], w[i-16], w[i-7] and channel 4 writing w[i] (31 contiguous cells)
    for (unsigned j = t; j < place::EXT_ROUNDS * 32; j += THREADS) {
        const unsigned r = j >> 5, cell = j & 31, i = r + 16;
        if (cell > 30) continue;
        uint64_t v = place::ext_clock(S, r, 0);
        if (cell) {
            const unsigned ch = (cell - 1) / 6, f = (cell - 1) % 6, idx = ch < 4 ? ext_src(i, ch) : i;
            v = chan_cell(f, ch < 4, ctx, seg, addr + 4 * idx, w[idx]);
        }
        A.rows[place::ext_row(e, r, 0) * CPU_W + C_CLOCK + cell] = v;
    }
    // the sponge rows: the flag, element.value = w_i, the clock, and context / segment / address of w[i] in the values of channels 0-2
    for (unsigned j = t; j < place::EXT_ROUNDS * 8; j += THREADS) {
        const unsigned r = j >> 3, cell = j & 7, i = r + 16;
        if (cell > 5) continue;
        uint64_t* row = A.rows + place::ext_row(e, r, 1) * CPU_W;
        if (cell == 0) row[C_IS_SHA_EXTEND_SPONGE] = 1;
        else if (cell == 1) row[C_GEN] = w[i];
        else if (cell == 2) row[C_CLOCK] = place::ext_clock(S, r, 1);
        else row[C_CH0 + 6 * (cell - 3) + 5] = cell == 3 ? ctx : cell == 4 ? seg : addr + 4 * i;
    }
    // the sponge's reads: four of each of the round's four input words (sha_extend_sponge_log), six words a read
    uint64_t* mem = A.mem + 6 * place::mem_base(A.E, e, false);
    for (unsigned j = t; j < 6 * place::EXT_MEM; j += THREADS) {
        const unsigned op = j / 6, f = j % 6, r = op >> 4, idx = ext_src(r + 16, (op >> 2) & 3);
        mem[j] = read_word(f, ctx, seg, addr + 4 * idx, ts + 20 * r, w[idx]);
    }
    // the four XORs of a round (generate_sha_extend), three words an operation
    uint32_t* logic = A.logic + 3 * place::logic_base(A.E, e, false);
    for (unsigned j = t; j < 3 * place::EXT_LOGIC; j += THREADS) {
        const unsigned op = j / 3, f = j % 3, r = op >> 2, k = op & 3, i = r + 16;
        const uint32_t x = w[k < 2 ? i - 15 : i - 2];
        const uint32_t a = k == 0 ? ror(x, 7) : k == 1 ? ror(x, 7) ^ ror(x, 18) : k == 2 ? ror(x, 17) : ror(x, 17) ^ ror(x, 19);
        const uint32_t b = k == 0 ? ror(x, 18) : k == 1 ? x >> 3 : k == 2 ? ror(x, 19) : x >> 10;
        logic[j] = f == 0 ? OP_XOR : f == 1 ? a : b;
    }
    // the ShaExtend table's inputs (the four words as little-endian bytes) and timestamps
    for (unsigned j = t; j < 4 * place::EXT_ROUNDS; j += THREADS) A.ext_in[4 * place::EXT_ROUNDS * e + j] = w[ext_src((j >> 2) + 16, j & 3)];
    if (t < place::EXT_ROUNDS) A.ext_ts[place::EXT_ROUNDS * e + t] = ts + 20 * t;
}

__device__ void compress_call(const sha_calls_args& A, size_t c, uint32_t* w, uint32_t* st) {
    const unsigned t = threadIdx.x;
    if (t < 64) w[t] = A.w[64 * c + t];
    if (t < 8) st[t] = A.hx[8 * c + t];
    __syncthreads();
    if (t == 0)   // st[8 i + q]: the state before round i; st[512 ..]: the compressed state
        for (unsigned i = 0; i < 64; i++) {
            const uint32_t* s = st + 8 * i;
            const uint32_t a = s[0], b = s[1], cc = s[2], d = s[3], e = s[4], f = s[5], g = s[6], h = s[7];
            const uint32_t t1 = h + (ror(e, 6) ^ ror(e, 11) ^ ror(e, 25)) + ((e & f) ^ (~e & g)) + SHA256_K_DEV[i] + w[i];
            const uint32_t t2 = (ror(a, 2) ^ ror(a, 13) ^ ror(a, 22)) + ((a & b) ^ (a & cc) ^ (b & cc));
            uint32_t* n = st + 8 * (i + 1);
            n[0] = t1 + t2; n[1] = a; n[2] = b; n[3] = cc; n[4] = d + t1; n[5] = e; n[6] = f; n[7] = g;
        }
    __syncthreads();
    const uint64_t* m = A.cmeta + 8 * c;
    const uint64_t hctx = m[0], hseg = m[1], haddr = m[2], ts = m[3], waddr = m[4], wseg = m[5], wctx = m[6], S = ts / 10;
    // the ten rows that use all eight channels: hx row (reads), eight w rows (reads), write row (hx + state); clock + 48 channel cells each
    for (unsigned j = t; j < 10 * 64; j += THREADS) {
        const unsigned kk = j >> 6, cell = j & 63, k = kk < 9 ? kk : place::CMP_WRITE;
        if (cell > 48) continue;
        uint64_t v = place::cmp_clock(S, k);
        if (cell) {
            const unsigned ch = (cell - 1) / 6, f = (cell - 1) % 6;
            if (k == place::CMP_HX) v = chan_cell(f, true, hctx, hseg, haddr + 4 * ch, st[ch]);
            else if (k == place::CMP_WRITE) v = chan_cell(f, false, hctx, hseg, haddr + 4 * ch, st[ch] + st[512 + ch]);
            else v = chan_cell(f, true, wctx, wseg, waddr + 4 * (8 * (k - place::CMP_W0) + ch), w[8 * (k - place::CMP_W0) + ch]);
        }
        A.rows[place::cmp_row(A.E, c, k) * CPU_W + C_CLOCK + cell] = v;
    }
    // the sponge row: the flag, shash.value[q] = hx[q] + state[q], the clock, context / segment / address of hx[0] in channels 0-2
    if (t < 13) {
        uint64_t* row = A.rows + place::cmp_row(A.E, c, place::CMP_SPONGE) * CPU_W;
        if (t < 8) row[C_GEN + t] = (uint32_t)(st[t] + st[512 + t]);
        else if (t == 8) row[C_IS_SHA_COMPRESS_SPONGE] = 1;
        else if (t == 9) row[C_CLOCK] = place::cmp_clock(S, place::CMP_SPONGE);
        else row[C_CH0 + 6 * (t - 10) + 5] = t == 10 ? hctx : t == 11 ? hseg : haddr;
    }
    // the sponge's reads: four of each hx word, then four of each w_i (sha_compress_sponge_log)
    uint64_t* mem = A.mem + 6 * place::mem_base(A.E, c, true);
    for (unsigned j = t; j < 6 * place::CMP_MEM; j += THREADS) {
        const unsigned op = j / 6, f = j % 6, q = op >> 2;
        mem[j] = q < 8 ? read_word(f, hctx, hseg, haddr + 4 * q, ts, st[q]) : read_word(f, wctx, wseg, waddr + 4 * (q - 8), ts, w[q - 8]);
    }
    // the twelve operations of a round (generate_sha_compress), from xor(e ror 6, e ror 11) through xor(maj_inter, b & c)
    uint32_t* logic = A.logic + 3 * place::logic_base(A.E, c, true);
    for (unsigned j = t; j < 3 * place::CMP_LOGIC; j += THREADS) {
        const unsigned op = j / 3, f = j % 3, i = op / 12, k = op % 12;
        const uint32_t* s = st + 8 * i;
        const uint32_t a = s[0], b = s[1], cc = s[2], e = s[4], ff = s[5], g = s[6];
        uint32_t code = OP_XOR, x, y;
        switch (k) {
        case 0: x = ror(e, 6); y = ror(e, 11); break;
        case 1: x = ror(e, 6) ^ ror(e, 11); y = ror(e, 25); break;
        case 2: code = OP_AND; x = e; y = ff; break;
        case 3: code = OP_AND; x = ~e; y = g; break;
        case 4: x = e & ff; y = ~e & g; break;
        case 5: x = ror(a, 2); y = ror(a, 13); break;
        case 6: x = ror(a, 2) ^ ror(a, 13); y = ror(a, 22); break;
        case 7: code = OP_AND; x = a; y = b; break;
        case 8: code = OP_AND; x = a; y = cc; break;
        case 9: code = OP_AND; x = b; y = cc; break;
        case 10: x = a & b; y = a & cc; break;
        default: x = (a & b) ^ (a & cc); y = b & cc; break;
        }
        logic[j] = f == 0 ? code : f == 1 ? x : y;
    }
}

__global__ __launch_bounds__(THREADS) void k_sha_calls(const sha_calls_args* __restrict__ segs) {
    __shared__ uint32_t w[64], st[8 * 65];
    const sha_calls_args A = zkm_seg_desc(segs);   // (uniform: scalar loads)
    if (blockIdx.x < A.E) extend_call(A, blockIdx.x, w);
    else if (blockIdx.x < A.E + A.C) compress_call(A, blockIdx.x - A.E, w, st);
}

// ---- the host's refusals: one walk over the two meta lists, naming the list and the call's position (throws the bare message)

void check_meta(const uint64_t* emeta, size_t E, const uint64_t* cmeta, size_t C) {
    if (E >= LIM / place::EXT_MEM || C >= LIM / place::CMP_LOGIC) throw std::runtime_error("2^32 or more operations");
    auto timestamp = [](const std::string& at, uint64_t ts, uint64_t before, const char* first) {
        if (ts % 10) throw std::runtime_error(at + "timestamp " + dec(ts) + " is not a multiple of 10 (NUM_CHANNELS)");
        if (ts / 10 < before) throw std::runtime_error(at + "timestamp " + dec(ts) + " puts " + first + " before clock 0");
    };
    auto fits = [&](const std::string& at, const char* what, uint64_t v) {
        if (v >= LIM) throw std::runtime_error(at + what + " " + dec(v) + " does not fit in 32 bits");
    };
    auto address = [&](const std::string& at, const char* base, uint64_t v, uint64_t span, const char* last) {
        if (v >= LIM || v + span >= LIM) throw std::runtime_error(at + "address of " + base + " " + hex(v) + ": " + last + " does not fit in 32 bits");
    };
    if (E && !emeta) throw std::runtime_error("extend_meta: NULL with a count of " + dec(E));
    if (C && !cmeta) throw std::runtime_error("compress_meta: NULL with a count of " + dec(C));
    // (a list in device memory is not read by the host: see the header)
    for (size_t e = 0; e < E && !zkm_is_device_ptr(emeta); e++) {
        const uint64_t* m = emeta + 4 * e;
        const std::string at = "extend_meta: call " + dec(e) + ": ";
        fits(at, "context", m[0]);
        fits(at, "segment", m[1]);
        address(at, "w[0]", m[2], 4 * 63, "w[63]");
        timestamp(at, m[3], 1, "the first read row");
    }
    for (size_t c = 0; c < C && !zkm_is_device_ptr(cmeta); c++) {
        const uint64_t* m = cmeta + 8 * c;
        const std::string at = "compress_meta: call " + dec(c) + ": ";
        fits(at, "context", m[0]);
        fits(at, "segment", m[1]);
        fits(at, "segment of w", m[5]);
        fits(at, "context of w", m[6]);
        address(at, "hx[0]", m[2], 4 * 7, "hx[7]");
        address(at, "w[0]", m[4], 4 * 64, "the 65th round's dummy address w + 256");
        timestamp(at, m[3], 9, "the hx row");
    }
}

// what the K-segment launcher takes of this kind (calls_launch.h)
struct sha_kind {
    using job = zkm_sha_job;
    using args = sha_calls_args;
    static constexpr const char *name = "zkm_sha_calls_launch", *scope = "sha_calls/rows_lists";
    static constexpr auto kernel = k_sha_calls;
    static constexpr unsigned threads = THREADS;
    // a job's five lists: the ones the host holds go up
    static std::array<zkm_calls_list, 5> lists(const job& j) {
        auto list = [](const void* p, size_t bytes) { return zkm_calls_list{p, bytes, bytes && !zkm_is_device_ptr(p)}; };
        return {{list(j.w16, 64 * j.E), list(j.emeta, 32 * j.E), list(j.hx, 32 * j.C), list(j.w, 256 * j.C), list(j.cmeta, 64 * j.C)}};
    }
    static args make(const job& j, const void* const* dev) {
        return {(const uint32_t*)dev[0], (const uint64_t*)dev[1], (const uint32_t*)dev[2], (const uint32_t*)dev[3], (const uint64_t*)dev[4],
                j.E, j.C, j.rows, j.mem, j.ext_ts, j.logic, j.ext_in};
    }
    static size_t extent(const job& j) { return j.E + j.C; }   // a workgroup a call
    static size_t sparse_rows(const job& j) { return place::cmp_row(j.E, j.C, 0); }
};

}  // namespace

void zkm_sha_calls_check(zkm_sha_job& j) {
    check_meta(j.emeta, j.E, j.cmeta, j.C);
    if (j.E && !j.w16) throw std::runtime_error("extend_w16: NULL with a count of " + dec(j.E));
    if (j.C && !j.hx) throw std::runtime_error("compress_hx: NULL with a count of " + dec(j.C));
    if (j.C && !j.w) throw std::runtime_error("compress_w: NULL with a count of " + dec(j.C));
    if (j.E + j.C > 0x7FFFFFFF) throw std::runtime_error("2^31 or more calls");
    j.nrows = place::cmp_row(j.E, j.C, 0), j.nmem = place::mem_base(j.E, j.C, true), j.nlogic = place::logic_base(j.E, j.C, true);
    j.next = place::EXT_ROUNDS * j.E;
}
size_t zkm_sha_calls_scratch(const zkm_sha_job* j, size_t nseg) { return zkm_calls_layout<sha_kind>(j, nseg, nullptr); }
void zkm_sha_calls_launch(zkm_ctx* c, const zkm_sha_job* j, size_t nseg, char* sb, zkm_calls_hold& hold, bool zero_rows, hipStream_t stream) {
    zkm_calls_queue<sha_kind>(c, stream ? stream : c->stream, j, nseg, sb, hold, zero_rows);
}

extern "C" {

void zkm_sha_calls_counts(size_t E, size_t C, size_t* cpu_rows, size_t* memory_ops, size_t* logic_ops, size_t* sha_extend_rows) {
    if (cpu_rows) *cpu_rows = place::cmp_row(E, C, 0);
    if (memory_ops) *memory_ops = place::mem_base(E, C, true);
    if (logic_ops) *logic_ops = place::logic_base(E, C, true);
    if (sha_extend_rows) *sha_extend_rows = place::EXT_ROUNDS * E;
}

int zkm_sha_calls_steps(const uint64_t* extend_meta, size_t nextend, const uint64_t* compress_meta, size_t ncompress, size_t raw_base,
                        zkm_cpu_step* steps_out, uint64_t* clocks_out, char** err) {
    return zkm_api("zkm_sha_calls_steps", err, [&] {
        auto refuse = [](const std::string& m) { throw std::runtime_error("zkm_sha_calls_steps: " + m); };
        try {
            check_meta(extend_meta, nextend, compress_meta, ncompress);
        } catch (const std::exception& e) {
            refuse(e.what());
        }
        if ((nextend && zkm_is_device_ptr(extend_meta)) || (ncompress && zkm_is_device_ptr(compress_meta))) refuse("the meta lists must be host memory");
        const size_t rows = place::cmp_row(nextend, ncompress, 0);
        if (rows && (!steps_out || !clocks_out)) refuse("null argument");
        if (raw_base >= LIM || raw_base + rows > LIM) refuse("raw_base " + dec(raw_base) + ": a RAW index does not fit in 32 bits");
        for (size_t j = 0; j < rows; j++) {
            const zkm_row_rec r = place::row_rec(extend_meta, nextend, compress_meta, j);
            steps_out[j] = raw_step(raw_base + j, r.mask);
            clocks_out[j] = r.clock;
        }
    });
}

int zkm_sha_calls_witness(zkm_ctx* c, const uint32_t* extend_w16, const uint64_t* extend_meta, size_t nextend, const uint32_t* compress_hx,
                          const uint32_t* compress_w, const uint64_t* compress_meta, size_t ncompress, uint64_t* raw_rows_out_dev,
                          uint64_t* memory_ops_out_dev, uint32_t* logic_ops_out_dev, uint8_t* sha_extend_inputs_out_dev,
                          uint64_t* sha_extend_timestamps_out_dev, char** err) {
    return zkm_api("zkm_sha_calls_witness", err, [&] {
        auto refuse = [](const std::string& m) { throw std::runtime_error("zkm_sha_calls_witness: " + m); };
        // every refusal first, on the host: the lists, the outputs, then the context
        zkm_sha_job j;
        j.w16 = extend_w16, j.emeta = extend_meta, j.E = nextend, j.hx = compress_hx, j.w = compress_w, j.cmeta = compress_meta, j.C = ncompress;
        j.rows = raw_rows_out_dev, j.mem = memory_ops_out_dev, j.ext_ts = sha_extend_timestamps_out_dev, j.logic = logic_ops_out_dev;
        j.ext_in = (uint32_t*)sha_extend_inputs_out_dev;
        try {
            zkm_sha_calls_check(j);
        } catch (const std::exception& e) {
            refuse(e.what());
        }
        if (j.E + j.C == 0) {
            if (!c) refuse("null argument");
            return;
        }
        if (!raw_rows_out_dev) refuse("raw_rows_out_dev: NULL with " + dec(j.nrows) + " rows to write");
        if (!memory_ops_out_dev) refuse("memory_ops_out_dev: NULL with " + dec(j.nmem) + " operations to write");
        if (!logic_ops_out_dev) refuse("logic_ops_out_dev: NULL with " + dec(j.nlogic) + " operations to write");
        if (j.E && !sha_extend_inputs_out_dev) refuse("sha_extend_inputs_out_dev: NULL with " + dec(j.next) + " rows to write");
        if (j.E && !sha_extend_timestamps_out_dev) refuse("sha_extend_timestamps_out_dev: NULL with " + dec(j.next) + " rows to write");
        if (((uintptr_t)raw_rows_out_dev | (uintptr_t)memory_ops_out_dev | (uintptr_t)sha_extend_timestamps_out_dev) & 7 ||
            ((uintptr_t)logic_ops_out_dev | (uintptr_t)sha_extend_inputs_out_dev) & 3)
            refuse("an output is not aligned to its words (8 bytes; 4 for the logic operations and the ShaExtend inputs)");
        if (!c) refuse("null argument");
        ZKM_HIP_CHECK(hipSetDevice(c->device));
        zkm_calls_one<sha_kind>(c, j);
    });
}

}  // extern "C"
