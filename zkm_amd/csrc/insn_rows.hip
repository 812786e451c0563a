// insn_rows.hip -- the rows of the thirteen instructions decode() accepts (witness/transition.rs:42-312) and no step kind takes, expanded
// on the device as ready-made rows for RAW steps, with the arithmetic operations they push (include/zkm_hip.h "the instructions the step
// kinds refuse, as rows"): LUI (generate_lui, witness/operation.rs:405-433), MUL MFHI MTHI MFLO MTLO (generate_binary_arithmetic_op,
// :286-318), MULT MULTU DIV DIVU (generate_binary_arithmetic_hilo_op, :320-375), SDC1 (generate_mstore_general, :1804-1928) and SYNC / PREF
// (generate_nop).
//
// What a record produces is stated once, in zkm_insn::expand below: a __host__ __device__ function that drives a sink, as zkm_step::walk
// does for the step kinds (cpu_steps_dev.h).  The host walk runs it with a counting sink (the refusals, the channel mask of
// zkm_insn_rows_steps, the two counts, each workgroup's base in the arithmetic list); the kernel runs it with a sink that writes an LDS
// row and the operation -- so masks, offsets and cells agree by construction.
//
// k_insn_rows: ONE launch for the records of K segments (the segment is blockIdx.z; its descriptor is read from device memory, where it
// went up with the lists as the bootstrap's do -- a uniform read; zkm_insn_rows_witness is the K = 1 case), a workgroup of 256 threads
// for ROWS_PER_WG consecutive records of one segment.  All lanes zero the workgroup's LDS block (2,072 bytes a row); the first
// ROWS_PER_WG lanes load their record (three 16-byte loads), find their slot in the arithmetic list (the workgroup's uploaded base + a
// ballot over the lanes in front) and build their row in LDS through expand; then all lanes stream the block out word by word, adjacent
// lanes on adjacent words with 8-byte stores.  Every word is written exactly once, so no zero-fill pass comes in front; the kernel's
// floor is the 2,072 bytes a row it has to write.
#include "calls_launch.h"
#include "calls_place_dev.h"   // zkm_insn: one record as a whole row (expand), and the record the step list gets for it

namespace {

using namespace zkm_insn;
using namespace zkm_calls;
constexpr unsigned CPU_W = ZKM_CPU_COLS, THREADS = 256, ROWS_PER_WG = 16;
static_assert(ROWS_PER_WG <= 64, "the rows' lanes are one wave: the arithmetic slots come from a ballot");
static_assert(ROWS_PER_WG * CPU_W * 8 <= 48 * 1024, "the workgroup's rows fit in LDS");

struct insn_rows_args {
    const zkm_cpu_step* insns;   // ninsns
    const uint64_t* clocks;      // ninsns
    const uint32_t* arith_base;  // one per workgroup: the operations the records in front of it push
    uint64_t* rows;
    uint32_t* arith;             // null: no record pushes an operation
    uint64_t ninsns;
    uint32_t nwg;                // the segment's own extent of the grid
};

// the writing sink: a row in LDS (zeroed in front) and the record's slot in the arithmetic list
struct lds_sink {
    uint64_t* row;
    uint32_t* ar;
    __device__ __forceinline__ void cell(unsigned col, uint64_t v) { row[col] = v; }
    __device__ __forceinline__ void chan(unsigned i, bool used, bool is_read, uint32_t ctx, uint32_t seg, uint32_t virt, uint32_t value) {
        uint64_t* p = row + C_CH0 + 6 * i;
        p[0] = used; p[1] = is_read; p[2] = ctx; p[3] = seg; p[4] = virt; p[5] = value;
    }
    __device__ __forceinline__ void arith(uint32_t op, uint32_t a, uint32_t b) {
        if (ar) { ar[0] = op; ar[1] = a; ar[2] = b; }
    }
};

__global__ __launch_bounds__(THREADS) void k_insn_rows(const insn_rows_args* __restrict__ segs) {
    __shared__ uint64_t block[ROWS_PER_WG * CPU_W];
    const insn_rows_args A = zkm_seg_desc(segs);   // (uniform: scalar loads)
    if (blockIdx.x >= A.nwg) return;
    const unsigned t = threadIdx.x;
    const uint64_t row0 = (uint64_t)blockIdx.x * ROWS_PER_WG;
    const unsigned nrows = A.ninsns - row0 < ROWS_PER_WG ? (unsigned)(A.ninsns - row0) : ROWS_PER_WG;
    for (unsigned w = t; w < nrows * CPU_W; w += THREADS) block[w] = 0;
    __syncthreads();
    if (t < 64) {   // the wave that holds the rows' lanes (whole, for the ballot)
        const bool live = t < nrows;
        zkm_cpu_step r{};
        r.kind = NKINDS;   // (a lane without a record: expand drives nothing)
        uint64_t clock = 0;
        if (live) {
            const uint4* p = (const uint4*)(A.insns + row0 + t);
            const uint4 a = p[0], b = p[1], c = p[2];
            r.pc = a.x; r.next_pc = a.y; r.insn = a.z; r.kind = a.w;
            r.flags = b.x; r.context = b.y; r.reads[0] = b.z; r.reads[1] = b.w;
            r.reads[2] = c.x; r.reads[3] = c.y; r.reads[4] = c.z; r.reads[5] = c.w;
            clock = A.clocks[row0 + t];
        }
        shape k;
        if (expand(r, clock, k) != OK) k = shape{};   // (the host walk has refused such a record)
        const uint64_t pushing = __ballot(k.narith != 0);
        const unsigned before = __popcll(pushing & (((uint64_t)1 << t) - 1));
        if (live) {
            lds_sink s{block + t * CPU_W, A.arith && k.narith ? A.arith + 3 * ((size_t)A.arith_base[blockIdx.x] + before) : nullptr};
            (void)expand(r, clock, s);
        }
    }
    __syncthreads();
    // the workgroup's span of the output, word by word: adjacent lanes store adjacent words
    uint64_t* __restrict__ out = A.rows + row0 * CPU_W;
    for (unsigned w = t; w < nrows * CPU_W; w += THREADS) out[w] = block[w];
}

// ---- the host walk: every refusal, naming the record; the counts, the masks, the workgroups' bases
const char* const KIND_NAME[NKINDS] = {"LUI", "MUL", "MULT", "MULTU", "DIV", "DIVU", "MFHI", "MTHI", "MFLO", "MTLO", "SDC1", "SYNC", "PREF"};

struct totals { uint64_t mem = 0, arith = 0; };

// Returns the totals; masks (one per record) and base (one per workgroup) if asked.  Throws the bare message.
totals check_insns(const zkm_cpu_step* insns, size_t n, std::vector<uint32_t>* masks, std::vector<uint32_t>* base) {
    totals sum;
    if (n && !insns) throw std::runtime_error("insns: NULL with a count of " + dec(n));
    if (n && zkm_is_device_ptr(insns)) throw std::runtime_error("insns: device memory (the records size the outputs: they must be host memory)");
    if (masks) masks->assign(n, 0);
    if (base) base->assign((n + ROWS_PER_WG - 1) / ROWS_PER_WG, 0);
    for (size_t k = 0; k < n; k++) {
        const zkm_cpu_step& t = insns[k];
        if (base && k % ROWS_PER_WG == 0) (*base)[k / ROWS_PER_WG] = (uint32_t)sum.arith;
        shape s;
        const int verdict = expand(t, 0, s);
        if (verdict != OK) {
            const std::string at = "record " + dec(k) + ": ";
            switch (verdict) {
            case BAD_KIND: throw std::runtime_error(at + "unknown kind " + dec(t.kind) + " (ZKM_INSN_LUI to ZKM_INSN_PREF are 0 to 12)");
            case BAD_ENCODING: throw std::runtime_error(at + KIND_NAME[t.kind] + " does not take the encoding " + hex8(t.insn));
            case DIV_BY_ZERO: throw std::runtime_error(at + KIND_NAME[t.kind] + " by zero (reads[1] is 0: the reference's result() panics)");
            case DIV_OVERFLOW: throw std::runtime_error(at + "DIV of 0x80000000 by 0xffffffff overflows (the reference's result() panics)");
            default:
                throw std::runtime_error(at + KIND_NAME[t.kind] + " reads register 0 on channel 1: reads[1] is " + hex8(t.reads[1]) + ", not 0");
            }
        }
        if (masks) (*masks)[k] = s.mask;
        sum.mem += __builtin_popcount(s.mask);
        sum.arith += s.narith;
    }
    return sum;
}

void check_clocks(const uint64_t* clocks, size_t n) {
    if (n && !clocks) throw std::runtime_error("clocks: NULL with a count of " + dec(n));
    if (n && zkm_is_device_ptr(clocks)) throw std::runtime_error("clocks: device memory (they are read on the host)");
    for (size_t k = 0; k < n; k++)
        if (clocks[k] >= LIM) throw std::runtime_error("record " + dec(k) + ": clock " + dec(clocks[k]) + " does not fit in 32 bits");
}

// what the K-segment launcher takes of this kind (calls_launch.h)
struct insn_kind {
    using job = zkm_insn_job;
    using args = insn_rows_args;
    static constexpr const char *name = "zkm_insn_rows_launch", *scope = "insn_rows/rows";
    static constexpr auto kernel = k_insn_rows;
    static constexpr unsigned threads = THREADS;
    // a job's three lists: the records, the clocks, the workgroups' bases; the records and clocks go up unless a staged call has them up already
    static std::array<zkm_calls_list, 3> lists(const job& j) {
        return {{{j.insns, j.n * sizeof(zkm_cpu_step), !zkm_is_device_ptr(j.insns)}, {j.clocks, j.n * 8, !zkm_is_device_ptr(j.clocks)},
                 {j.base.data(), j.base.size() * 4, true}}};
    }
    static args make(const job& j, const void* const* dev) {
        return {(const zkm_cpu_step*)dev[0], (const uint64_t*)dev[1], (const uint32_t*)dev[2], j.rows, j.narith ? j.arith : nullptr, j.n, (uint32_t)extent(j)};
    }
    static size_t extent(const job& j) { return (j.n + ROWS_PER_WG - 1) / ROWS_PER_WG; }   // a workgroup for ROWS_PER_WG records
    static size_t sparse_rows(const job&) { return 0; }   // (the kernel writes every word)
};

}  // namespace

void zkm_insn_rows_check(zkm_insn_job& j) {
    const totals sum = check_insns(j.insns, j.n, nullptr, &j.base);
    check_clocks(j.clocks, j.n);
    if (j.n > LIM) throw std::runtime_error(dec(j.n) + " rows: a RAW index does not fit in 32 bits");
    j.nmem = sum.mem;
    j.narith = sum.arith;
}
size_t zkm_insn_rows_scratch(const zkm_insn_job* j, size_t nseg) { return zkm_calls_layout<insn_kind>(j, nseg, nullptr); }
void zkm_insn_rows_launch(zkm_ctx* c, const zkm_insn_job* j, size_t nseg, char* sb, zkm_calls_hold& hold, hipStream_t stream) {
    zkm_calls_queue<insn_kind>(c, stream ? stream : c->stream, j, nseg, sb, hold, false);
}

extern "C" {

int zkm_insn_rows_counts(const zkm_cpu_step* insns, size_t ninsns, size_t* memory_ops, size_t* arithmetic_ops, char** err) {
    return zkm_api("zkm_insn_rows_counts", err, [&] {
        totals sum;
        try {
            sum = check_insns(insns, ninsns, nullptr, nullptr);
        } catch (const std::exception& e) {
            throw std::runtime_error(std::string("zkm_insn_rows_counts: ") + e.what());
        }
        if (memory_ops) *memory_ops = sum.mem;
        if (arithmetic_ops) *arithmetic_ops = sum.arith;
    });
}

int zkm_insn_rows_steps(const zkm_cpu_step* insns, size_t ninsns, size_t raw_base, zkm_cpu_step* steps_out, char** err) {
    return zkm_api("zkm_insn_rows_steps", err, [&] {
        auto refuse = [](const std::string& m) { throw std::runtime_error("zkm_insn_rows_steps: " + m); };
        std::vector<uint32_t> masks;
        try {
            check_insns(insns, ninsns, &masks, nullptr);
        } catch (const std::exception& e) {
            refuse(e.what());
        }
        if (ninsns && !steps_out) refuse("steps_out: NULL with " + dec(ninsns) + " records to write");
        if (raw_base >= LIM || raw_base + ninsns > LIM) refuse("raw_base " + dec(raw_base) + ": a RAW index does not fit in 32 bits");
        for (size_t k = 0; k < ninsns; k++) steps_out[k] = raw_step(raw_base + k, masks[k]);
    });
}

int zkm_insn_rows_witness(zkm_ctx* c, const zkm_cpu_step* insns, const uint64_t* clocks, size_t ninsns, uint64_t* raw_rows_out_dev,
                          uint32_t* arithmetic_ops_out_dev, char** err) {
    return zkm_api("zkm_insn_rows_witness", err, [&] {
        auto refuse = [](const std::string& m) { throw std::runtime_error("zkm_insn_rows_witness: " + m); };
        // every refusal first, on the host: the records, the clocks, the outputs, then the context
        zkm_insn_job j;
        j.insns = insns, j.clocks = clocks, j.n = ninsns, j.rows = raw_rows_out_dev, j.arith = arithmetic_ops_out_dev;
        try {
            zkm_insn_rows_check(j);
        } catch (const std::exception& e) {
            refuse(e.what());
        }
        if (ninsns == 0) {
            if (!c) refuse("null argument");
            return;
        }
        if (!raw_rows_out_dev) refuse("raw_rows_out_dev: NULL with " + dec(ninsns) + " rows to write");
        if ((uintptr_t)raw_rows_out_dev & 7) refuse("raw_rows_out_dev is not aligned to its words (8 bytes)");
        if (j.narith && !arithmetic_ops_out_dev) refuse("arithmetic_ops_out_dev: NULL with " + dec(j.narith) + " operations to write");
        if ((uintptr_t)arithmetic_ops_out_dev & 3) refuse("arithmetic_ops_out_dev is not aligned to its words (4 bytes)");
        if (!c) refuse("null argument");
        ZKM_HIP_CHECK(hipSetDevice(c->device));
        zkm_calls_one<insn_kind>(c, j);
    });
}

}  // extern "C"
