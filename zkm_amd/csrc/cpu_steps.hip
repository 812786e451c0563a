// cpu_steps.hip -- a segment's CPU rows, and the memory, logic and arithmetic operations they push, built on the device from the compact
// step log (include/zkm_hip.h zkm_cpu_step; what a step produces: cpu_steps_dev.h).
//
// The steps are walked once before k_cpu_steps runs: every refusal is made on that walk, and since a step's counts are a function of
// its record, the walk also knows the three list lengths and where each workgroup of ZKM_CPU_STEPS_BLOCK steps starts in the lists --
// one base triple per workgroup, and the kernel scans inside the workgroup.  An unstaged call walks on the host (zkm_cpu_steps_walk:
// the bases go up with the steps, no host wait); steps staged ahead of the call are walked on the device (cpu_steps_walk.hip), word
// for word the same bases.
//
// k_cpu_steps: one thread per step, the segment is blockIdx.z.  The record comes in as three 16-byte loads; adjacent lanes are adjacent
// rows, so a column's stores are coalesced with no LDS staging.  The row is never held: the table is zeroed by one memset before the
// launch and a thread stores the cells its kind sets, each straight to its column.  ROWS / LISTS choose what a launch writes: the segment
// builder needs the lists before the heights are known and the table after them (segment_ops.hip), the standalone entry both at once.
#include "cpu_steps_dev.h"
#include "zkm_internal.h"

namespace {

using namespace zkm_step;
constexpr unsigned CPU_W = ZKM_CPU_COLS, BLOCK = ZKM_CPU_STEPS_BLOCK;

template <bool ROWS, bool LISTS> struct row_sink {
    gl_t* o;          // the row's cell in column 0
    size_t n;         // the column stride
    uint64_t* mem;    // where the next operation of each list goes (null: the list is not written)
    uint32_t *lo, *ar;
    uint64_t ts;
    __device__ __forceinline__ void cell(unsigned col, uint64_t v) {
        if (ROWS) o[(size_t)col * n] = v;
    }
    __device__ __forceinline__ void inv(unsigned col, gl_t x) {
        if (ROWS && x) o[(size_t)col * n] = gl_inv(x);
    }
    __device__ __forceinline__ void chan(unsigned i, bool used, bool is_read, uint32_t ctx, uint32_t seg, uint32_t virt, uint32_t value) {
        if (ROWS) {
            gl_t* p = o + (size_t)(C_CH0 + 6 * i) * n;
            p[0] = used; p[n] = is_read; p[2 * n] = ctx; p[3 * n] = seg; p[4 * n] = virt; p[5 * n] = value;
        }
        if (LISTS && used && mem) {
            mem[0] = ctx; mem[1] = seg; mem[2] = virt; mem[3] = ts; mem[4] = is_read; mem[5] = value;
            mem += 6;
        }
    }
    __device__ __forceinline__ void logic(uint32_t op, uint32_t a, uint32_t b) {
        if (LISTS && lo) { lo[0] = op; lo[1] = a; lo[2] = b; }
    }
    __device__ __forceinline__ void arith(uint32_t op, uint32_t a, uint32_t b) {
        if (LISTS && ar) { ar[0] = op; ar[1] = a; ar[2] = b; }
    }
};

template <bool ROWS, bool LISTS> __global__ __launch_bounds__(BLOCK) void k_cpu_steps(zkm_seg_args<zkm_steps_seg> S) {
    __shared__ uint32_t wave_sum[BLOCK / 64];
    const zkm_steps_seg& A = S.v[blockIdx.z];
    if ((size_t)blockIdx.x * BLOCK >= A.nsteps) return;
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool live = i < A.nsteps;
    zkm_cpu_step t{};
    t.kind = ZKM_STEP_PAD;
    if (live) {
        const uint4* p = (const uint4*)(A.steps + i);
        const uint4 a = p[0], b = p[1], c = p[2];
        t.pc = a.x; t.next_pc = a.y; t.insn = a.z; t.kind = a.w;
        t.flags = b.x; t.context = b.y; t.reads[0] = b.z; t.reads[1] = b.w;
        t.reads[2] = c.x; t.reads[3] = c.y; t.reads[4] = c.z; t.reads[5] = c.w;
    }
    row_sink<ROWS, LISTS> s{};
    if (LISTS) {
        // where this step's operations start: the workgroup's base (the host walk's) + the steps before it in the workgroup
        counts k;
        if (live && count(t, k) != OK) k = counts{};
        const uint32_t packed = k.nmem | (k.nlogic << 12) | (k.narith << 22);   // 256 steps: at most 2048, 256, 256
        const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        uint32_t x = packed;
#pragma unroll
        for (unsigned d = 1; d < 64; d <<= 1) {
            const uint32_t y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        if (lane == 63) wave_sum[wave] = x;
        __syncthreads();
        x -= packed;
        for (unsigned w = 0; w < wave; w++) x += wave_sum[w];
        const uint32_t* base = A.base + 3 * (size_t)blockIdx.x;
        s.mem = A.mem ? A.mem + 6 * ((size_t)base[0] + (x & 0xFFF)) : nullptr;
        s.lo = A.logic ? A.logic + 3 * ((size_t)base[1] + ((x >> 12) & 0x3FF)) : nullptr;
        s.ar = A.arith ? A.arith + 3 * ((size_t)base[2] + (x >> 22)) : nullptr;
    }
    if (!live) return;
    const uint64_t clock = A.clock0 + i;
    s.o = A.out + A.row0 + i;
    s.n = A.n;
    s.ts = clock * 10;    // timestamp = clock * NUM_CHANNELS (witness/memory.rs:79-95)
    if (t.kind == ZKM_STEP_RAW) {
        // a ready-made row: copied canonical; its used channels are memory operations in ascending channel order, at the row's own clock
        const uint64_t* src = A.raw + (size_t)t.reads[0] * CPU_W;
        if (ROWS)
            for (unsigned c = 0; c < CPU_W; c++) s.o[(size_t)c * s.n] = gl_canon(src[c]);
        if (LISTS && s.mem) {
            const uint64_t ts = gl_canon(src[C_CLOCK]) * 10;
            for (unsigned k = 0; k < NUM_GP_CHANNELS; k++) {
                if (!((t.reads[1] >> k) & 1)) continue;
                const uint64_t* ch = src + C_CH0 + 6 * k;
                s.mem[0] = gl_canon(ch[2]); s.mem[1] = gl_canon(ch[3]); s.mem[2] = gl_canon(ch[4]); s.mem[3] = ts;
                s.mem[4] = gl_canon(ch[1]) != 0; s.mem[5] = (uint32_t)gl_canon(ch[5]);
                s.mem += 6;
            }
        }
        return;
    }
    s.cell(C_CLOCK, clock);
    if (t.context) s.cell(C_CONTEXT, t.context);
    s.cell(C_PC, t.pc);
    s.cell(C_NEXT_PC, t.next_pc);
    if (t.kind == ZKM_STEP_PAD) {   // generation/mod.rs:171-176
        s.cell(C_IS_EXIT, 1);
        return;
    }
    if (t.flags & 1) s.cell(C_KERNEL, 1);
    // the six bit fields in column order: opcode, rs, rt, rd, shamt, func, each from its low bit
    const uint32_t w = t.insn;
    bits32(s, C_BITS, (w >> 26) | (((w >> 21) & 31) << 6) | (((w >> 16) & 31) << 11) | (((w >> 11) & 31) << 16) | (((w >> 6) & 31) << 21) | ((w & 63) << 26));
    (void)walk(t, s);
}

const char* const KIND_NAMES[] = {"BINARY_OP", "BINARY_IMM_OP", "LOGIC_OP", "LOGIC_IMM_OP", "SHIFT", "SHIFT_IMM", "BRANCH", "JUMPS", "JUMPI", "JUMPDIRECT",
                                  "M_OP_LOAD", "M_OP_STORE", "NOP", "CLZ_OP", "CLO_OP", "SIGNEXT8", "SIGNEXT16", "SWAPHALF", "RDHWR", "MOVZ_OP", "MOVN_OP",
                                  "TEQ", "EXT", "INS", "ROR", "MADDU", "SYSCALL", "PAD", "RAW"};
static_assert(sizeof KIND_NAMES / sizeof *KIND_NAMES == ZKM_STEP_RAW + 1, "one name per kind");

std::string hex8(uint32_t v) {
    char buf[16];
    snprintf(buf, sizeof buf, "0x%08x", v);
    return buf;
}

size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

// The message of a step's refusal, without the entry point's prefix: the one statement of these texts, for the host walk below and for
// the verdict records of the device walk (cpu_steps_walk.hip).  `used`: the channels a RAW step's row uses (BAD_MASK only).
std::string zkm_cpu_step_refusal(size_t i, const zkm_cpu_step& t, size_t nraw, int code, uint32_t used) {
    const std::string at = "step " + std::to_string(i) + ": ";
    if (t.kind > ZKM_STEP_RAW) code = BAD_KIND;   // (no name to print: what count() says of such a record anyway)
    switch (code) {
    case BAD_INDEX: return at + "RAW index " + std::to_string(t.reads[0]) + ", raw_rows holds " + std::to_string(nraw);
    case BAD_KIND: return at + "unknown kind " + std::to_string(t.kind);
    case BAD_OPERANDS: return at + KIND_NAMES[t.kind] + " does not take these operands (TEQ of equal values traps)";
    case BAD_MASK:
        return at + "RAW row " + std::to_string(t.reads[0]) + " uses the channels " + hex8(used) + ", the step's mask is " + hex8(t.reads[1]);
    default:
        return at + KIND_NAMES[t.kind] + " does not take the encoding " + hex8(t.insn) +
               (t.kind == ZKM_STEP_SYSCALL ? " with flags " + hex8(t.flags)
                : t.kind == ZKM_STEP_RAW   ? " with the channel mask " + hex8(t.reads[1])
                                           : std::string());
    }
}

void zkm_cpu_steps_walk(const zkm_cpu_steps* st, zkm_steps_counts_t* n, std::vector<uint32_t>* base) {
    if (!st) throw std::runtime_error("null argument");
    if ((st->nsteps && !st->steps) || (st->nraw && !st->raw_rows)) throw std::runtime_error("null pointer with a nonzero count");
    // (the records are read here, on the host: the device pointers a staged handle hands out go to the builder, which does not walk them)
    if (st->nsteps && zkm_is_device_ptr(st->steps)) throw std::runtime_error("steps in device memory: this walk reads them on the host");
    *n = zkm_steps_counts_t{};
    // ready-made rows the host can read are held to their records: a RAW step's mask must name exactly the row's used channels
    const bool raw_host = st->nraw && !zkm_is_device_ptr(st->raw_rows);
    if (base) base->assign(3 * ((st->nsteps + BLOCK - 1) / BLOCK), 0);
    for (size_t i = 0; i < st->nsteps; i++) {
        const zkm_cpu_step& t = st->steps[i];
        if (n->mem >= ((uint64_t)1 << 32) - 16) throw std::runtime_error("step " + std::to_string(i) + ": 2^32 or more memory operations");
        if (base && i % BLOCK == 0) {
            uint32_t* b = base->data() + 3 * (i / BLOCK);
            b[0] = (uint32_t)n->mem; b[1] = (uint32_t)n->logic; b[2] = (uint32_t)n->arith;
        }
        if (t.kind == ZKM_STEP_RAW && t.reads[0] >= st->nraw) throw std::runtime_error(zkm_cpu_step_refusal(i, t, st->nraw, BAD_INDEX, 0));
        counts k;
        if (const int code = count(t, k); code != OK) throw std::runtime_error(zkm_cpu_step_refusal(i, t, st->nraw, code, 0));
        if (t.kind == ZKM_STEP_RAW && raw_host) {
            const uint64_t* ch = st->raw_rows + (size_t)t.reads[0] * CPU_W + C_CH0;
            uint32_t used = 0;
            for (unsigned c = 0; c < NUM_GP_CHANNELS; c++) used |= (uint32_t)(gl_canon(ch[6 * c]) != 0) << c;
            if (used != t.reads[1]) throw std::runtime_error(zkm_cpu_step_refusal(i, t, st->nraw, BAD_MASK, used));
        }
        n->mem += k.nmem;
        n->logic += k.nlogic;
        n->arith += k.narith;
    }
}

void zkm_cpu_steps_launch(zkm_ctx* c, const zkm_steps_seg* segs, size_t nseg, bool rows, bool lists) {
    size_t most = 0;
    for (size_t s = 0; s < nseg; s++) most = std::max(most, segs[s].nsteps);
    const size_t grid = (most + BLOCK - 1) / BLOCK;
    zkm_prof_scope ps(c, rows && lists ? "cpu_steps/rows_lists" : rows ? "cpu_steps/rows" : "cpu_steps/lists");
    if (rows && lists) zkm_launch_segs(c->stream, k_cpu_steps<true, true>, segs, nseg, grid, BLOCK);
    else if (rows) zkm_launch_segs(c->stream, k_cpu_steps<true, false>, segs, nseg, grid, BLOCK);
    else zkm_launch_segs(c->stream, k_cpu_steps<false, true>, segs, nseg, grid, BLOCK);
}

extern "C" {

int zkm_cpu_steps_counts(const zkm_cpu_steps* st, size_t* memory_ops, size_t* logic_ops, size_t* arithmetic_ops, char** err) {
    return zkm_api("zkm_cpu_steps_counts", err, [&] {
        zkm_steps_counts_t n;
        try {
            zkm_cpu_steps_walk(st, &n, nullptr);
        } catch (const std::exception& e) {
            throw std::runtime_error(std::string("zkm_cpu_steps_counts: ") + e.what());
        }
        if (memory_ops) *memory_ops = n.mem;
        if (logic_ops) *logic_ops = n.logic;
        if (arithmetic_ops) *arithmetic_ops = n.arith;
    });
}

int zkm_cpu_witness(zkm_ctx* c, const zkm_cpu_steps* st, uint64_t first_clock, unsigned log_n, uint64_t* cpu_out, uint64_t* mem_out,
                    uint32_t* logic_out, uint32_t* arith_out, char** err) {
    return zkm_api("zkm_cpu_witness", c, err, [&] {
        auto refuse = [](const std::string& m) { throw std::runtime_error("zkm_cpu_witness: " + m); };
        zkm_steps_counts_t k;
        std::vector<uint32_t> base;
        try {
            zkm_cpu_steps_walk(st, &k, &base);
        } catch (const std::exception& e) {
            refuse(e.what());
        }
        if (!cpu_out || (k.mem && !mem_out) || (k.logic && !logic_out) || (k.arith && !arith_out)) refuse("null argument");
        if (log_n > 28) refuse("log_n above 28");
        const size_t n = (size_t)1 << log_n;
        if (first_clock > n || st->nsteps > n - first_clock)
            refuse("rows [" + std::to_string(first_clock) + ", " + std::to_string(first_clock + st->nsteps) + ") do not fit in 2^" + std::to_string(log_n));
        ZKM_HIP_CHECK(hipMemsetAsync(cpu_out, 0, (size_t)CPU_W * n * sizeof(gl_t), c->stream));
        if (st->nsteps) {
            const bool raw_host = st->nraw && !zkm_is_device_ptr(st->raw_rows);
            const size_t o_base = up256(st->nsteps * sizeof(zkm_cpu_step)), o_raw = o_base + up256(base.size() * 4);
            zkm_scratch block(c, o_raw + (raw_host ? st->nraw * CPU_W * 8 : 0));
            char* sb = block.as<char>();
            ZKM_HIP_CHECK(hipMemcpyAsync(sb, st->steps, st->nsteps * sizeof(zkm_cpu_step), hipMemcpyHostToDevice, c->stream));
            ZKM_HIP_CHECK(hipMemcpyAsync(sb + o_base, base.data(), base.size() * 4, hipMemcpyHostToDevice, c->stream));
            if (raw_host) ZKM_HIP_CHECK(hipMemcpyAsync(sb + o_raw, st->raw_rows, st->nraw * CPU_W * 8, hipMemcpyHostToDevice, c->stream));
            const zkm_steps_seg seg{(const zkm_cpu_step*)sb, (const uint32_t*)(sb + o_base), raw_host ? (const uint64_t*)(sb + o_raw) : st->raw_rows,
                                    st->nsteps, n, (size_t)first_clock, first_clock, cpu_out, mem_out, logic_out, arith_out};
            zkm_cpu_steps_launch(c, &seg, 1, true, true);
            c->sync();   // (the block, `base` and the caller's steps are in use until here)
        } else {
            c->sync();
        }
    });
}

}  // extern "C"
