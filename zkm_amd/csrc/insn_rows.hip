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
#include "cpu_steps_dev.h"

namespace zkm_insn {

using zkm_step::bits32;
using zkm_step::reg_read;
using zkm_step::reg_write;
using zkm_step::sext;
using zkm_step::C_BITS;
using zkm_step::C_CH0;
using zkm_step::C_CLOCK;
using zkm_step::C_CONTEXT;
using zkm_step::C_GEN;
using zkm_step::C_KERNEL;
using zkm_step::C_MEMIO;
using zkm_step::C_NEXT_PC;
using zkm_step::C_PC;
using zkm_step::F_BINARY;
using zkm_step::F_BINARY_IMM;
using zkm_step::F_NOP;
using zkm_step::F_STORE;
using zkm_step::IO_AUX;
using zkm_step::IO_SDC1;
using zkm_step::SEG_CODE;
constexpr uint32_t NKINDS = 13;
// row filters of the arithmetic operators the step kinds leave out (arithmetic/mod.rs:135-164)
enum : uint32_t { A_MULT = 6, A_MULTU = 7, A_MUL = 8, A_DIV = 9, A_DIVU = 10, A_LUI = 21, A_MFHI = 22, A_MTHI = 23, A_MFLO = 24, A_MTLO = 25 };
constexpr uint32_t REG_LO = 32, REG_HI = 33;
// what expand returns
enum : int { OK = 0, BAD_KIND, BAD_ENCODING, DIV_BY_ZERO, DIV_OVERFLOW, R0_NOT_ZERO };

// does `kind` take this instruction word?  Exactly the (opcode, func) pair decode matches for it; the other fields are free.
GL_HD bool takes(uint32_t kind, uint32_t insn) {
    const uint32_t op = insn >> 26, fn = insn & 63;
    switch (kind) {
    case ZKM_INSN_LUI: return op == 0x0F;
    case ZKM_INSN_MUL: return op == 0x1C && fn == 0x02;
    case ZKM_INSN_MULT: return op == 0 && fn == 0x18;
    case ZKM_INSN_MULTU: return op == 0 && fn == 0x19;
    case ZKM_INSN_DIV: return op == 0 && fn == 0x1A;
    case ZKM_INSN_DIVU: return op == 0 && fn == 0x1B;
    case ZKM_INSN_MFHI: return op == 0 && fn == 0x10;
    case ZKM_INSN_MTHI: return op == 0 && fn == 0x11;
    case ZKM_INSN_MFLO: return op == 0 && fn == 0x12;
    case ZKM_INSN_MTLO: return op == 0 && fn == 0x13;
    case ZKM_INSN_SDC1: return op == 0x3D;
    case ZKM_INSN_SYNC: return op == 0 && fn == 0x0F;
    case ZKM_INSN_PREF: return op == 0x33;
    default: return false;
    }
}

// One record: the whole CpuColumnsView row (through s.cell / s.chan), and the arithmetic operation it pushes (s.arith).  Results are
// BinaryOperator::result's (arithmetic/mod.rs:48-133).  Nothing is driven unless the verdict is OK.
template <class S> GL_HD int expand(const zkm_cpu_step& t, uint64_t clock, S& s) {
    if (t.kind >= NKINDS) return BAD_KIND;
    if (!takes(t.kind, t.insn)) return BAD_ENCODING;
    const uint32_t w = t.insn, rs = (w >> 21) & 31, rt = (w >> 16) & 31, rd = (w >> 11) & 31, imm = w & 0xFFFF;
    const uint32_t a = t.reads[0], b = t.reads[1];
    const bool div = t.kind == ZKM_INSN_DIV || t.kind == ZKM_INSN_DIVU;
    const bool move = t.kind >= ZKM_INSN_MFHI && t.kind <= ZKM_INSN_MTLO;
    if (div && b == 0) return DIV_BY_ZERO;
    if (t.kind == ZKM_INSN_DIV && a == 0x80000000u && b == 0xFFFFFFFFu) return DIV_OVERFLOW;
    if (move && b != 0) return R0_NOT_ZERO;
    // the fixed part: clock, context, pc, next_pc, the kernel flag and the six bit fields in column order, each from its low bit
    s.cell(C_CLOCK, clock);
    if (t.context) s.cell(C_CONTEXT, t.context);
    if (t.pc) s.cell(C_PC, t.pc);
    if (t.next_pc) s.cell(C_NEXT_PC, t.next_pc);
    if (t.flags & ZKM_STEP_FLAG_KERNEL) s.cell(C_KERNEL, 1);
    bits32(s, C_BITS, (w >> 26) | (rs << 6) | (rt << 11) | (rd << 16) | (((w >> 6) & 31) << 21) | ((w & 63) << 26));
    switch (t.kind) {
    case ZKM_INSN_LUI: {   // channel 0 writes sext(imm) to rs, channel 1 writes 1 << 16 to rt, channel 2 the result to rt
        const uint32_t in0 = sext(imm, 16), in1 = 1u << 16;
        s.cell(F_BINARY_IMM, 1);
        reg_write(s, 0, rs, in0);
        reg_write(s, 1, rt, in1);
        reg_write(s, 2, rt, in0 << 16);
        s.arith(A_LUI, in0, in1);
        return OK;
    }
    case ZKM_INSN_MUL:
    case ZKM_INSN_MFHI:
    case ZKM_INSN_MTHI:
    case ZKM_INSN_MFLO:
    case ZKM_INSN_MTLO: {   // channels 0 and 1 read, channel 2 writes; decode's operands: MFHI (33, 0, rd), MTHI (rs, 0, 33), MFLO (32, 0, rd), MTLO (rs, 0, 32)
        const bool mul = t.kind == ZKM_INSN_MUL, from = t.kind == ZKM_INSN_MFHI || t.kind == ZKM_INSN_MFLO;
        const bool hi = t.kind == ZKM_INSN_MFHI || t.kind == ZKM_INSN_MTHI;
        const uint32_t r0 = mul ? rs : from ? (hi ? REG_HI : REG_LO) : rs, r1 = mul ? rt : 0, dest = mul || from ? rd : hi ? REG_HI : REG_LO;
        const uint32_t f = mul ? A_MUL : t.kind == ZKM_INSN_MFHI ? A_MFHI : t.kind == ZKM_INSN_MTHI ? A_MTHI : t.kind == ZKM_INSN_MFLO ? A_MFLO : A_MTLO;
        s.cell(F_BINARY, 1);
        reg_read(s, 0, r0, a);
        reg_read(s, 1, r1, b);
        reg_write(s, 2, dest, mul ? a * b : a);
        s.arith(f, a, b);
        return OK;
    }
    case ZKM_INSN_MULT:
    case ZKM_INSN_MULTU:
    case ZKM_INSN_DIV:
    case ZKM_INSN_DIVU: {   // channels 0 and 1 read rs and rt, channel 2 writes lo to register 32, channel 3 hi to register 33
        uint32_t lo, hi, f;
        if (t.kind == ZKM_INSN_MULT) {
            const uint64_t p = (uint64_t)((int64_t)(int32_t)a * (int64_t)(int32_t)b);
            f = A_MULT; lo = (uint32_t)p; hi = (uint32_t)(p >> 32);
        } else if (t.kind == ZKM_INSN_MULTU) {
            const uint64_t p = (uint64_t)a * b;
            f = A_MULTU; lo = (uint32_t)p; hi = (uint32_t)(p >> 32);
        } else if (t.kind == ZKM_INSN_DIV) {
            f = A_DIV; lo = (uint32_t)((int32_t)a / (int32_t)b); hi = (uint32_t)((int32_t)a % (int32_t)b);
        } else {
            f = A_DIVU; lo = a / b; hi = a % b;
        }
        s.cell(F_BINARY, 1);
        reg_read(s, 0, rs, a);
        reg_read(s, 1, rt, b);
        reg_write(s, 2, REG_LO, lo);
        reg_write(s, 3, REG_HI, hi);
        s.arith(f, a, b);
        return OK;
    }
    case ZKM_INSN_SDC1: {   // channels 0 and 1 read base and rt, channel 2 reads the word, channel 3 stores 0; aux_rs0_mul_rs1 stays 0
        const uint32_t m = t.reads[2], raw = a + sext(imm, 16), virt = raw & ~3u;
        s.cell(F_STORE, 1);
        s.cell(C_MEMIO + IO_SDC1, 1);
        s.cell(C_MEMIO + IO_AUX, 1);   // aux_filter = m_op_store * opcode_bits[5]: 0x3D has the bit
        reg_read(s, 0, rs, a);
        reg_read(s, 1, rt, b);
        s.chan(2, 1, 1, t.context, SEG_CODE, virt, m);
        s.chan(3, 1, 0, t.context, SEG_CODE, virt, 0);
        bits32(s, C_GEN, raw);
        bits32(s, C_GEN + 32, b);
        bits32(s, C_GEN + 64, m);
        return OK;
    }
    default:   // SYNC, PREF: decode makes them Nop
        s.cell(F_NOP, 1);
        return OK;
    }
}

// the counting sink: the mask of used channels and whether an operation is pushed
struct shape {
    uint32_t mask = 0, narith = 0;
    GL_HD void cell(unsigned, uint64_t) {}
    GL_HD void chan(unsigned i, bool used, bool, uint32_t, uint32_t, uint32_t, uint32_t) { mask |= (uint32_t)used << i; }
    GL_HD void arith(uint32_t, uint32_t, uint32_t) { narith++; }
};

}  // namespace zkm_insn

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
    // a job's three lists: the records, the clocks, the workgroups' bases; the host holds them all
    static std::array<zkm_calls_list, 3> lists(const job& j) {
        return {{{j.insns, j.n * sizeof(zkm_cpu_step), true}, {j.clocks, j.n * 8, true}, {j.base.data(), j.base.size() * 4, true}}};
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
void zkm_insn_rows_launch(zkm_ctx* c, const zkm_insn_job* j, size_t nseg, char* sb, zkm_calls_hold& hold) {
    zkm_calls_queue<insn_kind>(c, j, nseg, sb, hold, false);
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
