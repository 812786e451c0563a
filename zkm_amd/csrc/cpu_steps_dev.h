// cpu_steps_dev.h -- what one step of the compact step log (include/zkm_hip.h zkm_cpu_step) puts into a segment: the cells of its CPU row,
// its memory channels, and the logic and arithmetic operations it pushes, in push order (the reference's witness/operation.rs generate_*
// and witness/util.rs, as tests/cpu_fixtures.py Machine restates them).
//
// zkm_step::walk is the ONE statement of that: a __host__ __device__ function that drives a sink.  The host walk (validation, the three
// counts, the base of each workgroup in the lists) runs it with a counting sink, the kernels of cpu_steps.hip run it with the same
// counting sink for the offsets inside a workgroup and with a writing sink for the cells -- so sizes, offsets and writes agree by
// construction.  A sink has
//   cell(col, v)                                   a kind-specific cell of the row (canonical v)
//   inv(col, x)                                    ... the cell x^-1 (0 for 0), x canonical
//   chan(i, used, is_read, ctx, seg, virt, value)  memory channel i; used: the row pushes it as a memory operation
//   logic(op, a, b) / arith(op, a, b)              the operation pushed ({op, in0, in1} of zkm_logic_trace / zkm_arithmetic_trace)
// The row's fixed part (clock, context, pc, next_pc, kernel flag, the 32 instruction bits) is the caller's.
#pragma once
#include "../../include/zkm_hip.h"
#include "gl_dev.h"

#define ZKM_CPU_STEPS_BLOCK 256   // steps a workgroup takes: the host walk uploads one base triple per this many steps

namespace zkm_step {

// column map (cpu/columns/mod.rs:62-96, ops.rs, general.rs)
constexpr unsigned C_IS_BOOT = 0, C_IS_EXIT = 1, C_CONTEXT = 2, C_PC = 4, C_NEXT_PC = 5, C_KERNEL = 6, C_OP = 7, C_BR = 40, C_BITS = 50, C_GEN = 86,
                   C_MEMIO = 188, C_CLOCK = 204, C_CH0 = 205, NUM_GP_CHANNELS = 8;
constexpr unsigned C_IS_KECCAK_SPONGE = 83, C_IS_SHA_EXTEND_SPONGE = 84, C_IS_SHA_COMPRESS_SPONGE = 85;   // the sponge flags behind the bit fields
static_assert(C_CLOCK + 1 == C_CH0, "a row's clock and its 48 channel cells are 49 contiguous words");
constexpr uint32_t SEG_CODE = 0, SEG_SHIFT = 3, SEG_REG = 4;
// op flags, in the order of cpu/columns/ops.rs
enum : unsigned {
    F_BINARY = 7, F_BINARY_IMM, F_EQ_ISZERO, F_LOGIC, F_LOGIC_IMM, F_MOVZ, F_MOVN, F_CLZ, F_CLO, F_SHIFT, F_SHIFT_IMM, F_KECCAK_GENERAL, F_JUMPS,
    F_JUMPI, F_JUMPDIRECT, F_BRANCH, F_PC, F_GET_CONTEXT, F_SET_CONTEXT, F_EXIT_KERNEL, F_LOAD, F_STORE, F_NOP, F_EXT, F_INS, F_MADDU, F_RDHWR,
    F_SIGNEXT8, F_SIGNEXT16, F_SWAPHALF, F_TEQ, F_ROR, F_SYSCALL
};
static_assert(F_SYSCALL == 39, "33 op flags from column 7");
enum : unsigned { BR_SHOULD_JUMP = 40, BR_GT, BR_LT, BR_EQ, BR_IS_GT, BR_IS_LT, BR_IS_EQ, BR_IS_GE, BR_IS_LE, BR_IS_NE };
// memio selectors from C_MEMIO
enum : unsigned { IO_LH, IO_LWL, IO_LW, IO_LBU, IO_LHU, IO_LWR, IO_SB, IO_SH, IO_SWL, IO_SW, IO_SWR, IO_LL, IO_SC, IO_SDC1, IO_LB, IO_AUX };
// row filters of the arithmetic operators (arithmetic/mod.rs:135-164)
enum : uint32_t { A_ADD = 0, A_ADDU = 1, A_ADDI = 2, A_ADDIU = 3, A_SUB = 4, A_SUBU = 5, A_SLLV = 11, A_SRLV = 12, A_SRAV = 13, A_SLL = 14, A_SRL = 15,
                  A_SRA = 16, A_SLT = 17, A_SLTU = 18, A_SLTI = 19, A_SLTIU = 20 };

GL_HD uint32_t sext(uint32_t v, unsigned n) { return (v >> (n - 1)) & 1 ? v | (0xFFFFFFFFu << n) : v & ((n < 32 ? 1u << n : 0u) - 1u); }
GL_HD uint32_t low_mask(unsigned n) { return n >= 32 ? 0xFFFFFFFFu : (1u << n) - 1u; }   // n low bits

#ifdef __HIPCC__
// what the kernels that write a row's channels cell by cell compute (sha_calls.hip, keccak_calls.hip):
// the cell `f` of a used channel (cpu/columns/mod.rs MemoryChannelView: used, is_read, addr_context, addr_segment, addr_virtual, value)
__device__ __forceinline__ uint64_t chan_cell(unsigned f, bool is_read, uint64_t ctx, uint64_t seg, uint64_t virt, uint32_t value) {
    return f == 0 ? 1 : f == 1 ? (uint64_t)is_read : f == 2 ? ctx : f == 3 ? seg : f == 4 ? virt : (uint64_t)value;
}
// the word `f` of a memory read of the sponge (zkm_memory_trace's six words)
__device__ __forceinline__ uint64_t read_word(unsigned f, uint64_t ctx, uint64_t seg, uint64_t virt, uint64_t ts, uint32_t value) {
    return f == 0 ? ctx : f == 1 ? seg : f == 2 ? virt : f == 3 ? ts : f == 4 ? 1 : (uint64_t)value;
}
#endif

// what a walk returns, and the two refusals of a RAW step that need more than its record: its index against nraw, its mask against its row
enum : int { OK = 0, BAD_KIND = 1, BAD_ENCODING = 2, BAD_OPERANDS = 3, BAD_INDEX = 4, BAD_MASK = 5 };

template <class S> GL_HD void reg_read(S& s, unsigned i, uint32_t reg, uint32_t v) { s.chan(i, 1, 1, 0, SEG_REG, reg, v); }
// a write to register 0 fills the channel with used = 0 and pushes nothing (witness/util.rs:198-204)
template <class S> GL_HD void reg_write(S& s, unsigned i, uint32_t reg, uint32_t v) { s.chan(i, reg != 0, 0, 0, SEG_REG, reg, v); }
template <class S> GL_HD void bits32(S& s, unsigned col, uint32_t v) {
    for (unsigned i = 0; i < 32; i++)
        if ((v >> i) & 1) s.cell(col + i, 1);
}

// One step of a kind that has a witness model (everything but PAD and RAW, which the callers treat themselves).
template <class S> GL_HD int walk(const zkm_cpu_step& t, S& s) {
    const uint32_t insn = t.insn, op = insn >> 26, rs = (insn >> 21) & 31, rt = (insn >> 16) & 31, rd = (insn >> 11) & 31, sa = (insn >> 6) & 31,
                   fn = insn & 63, imm = insn & 0xFFFF, pc = t.pc;
    const uint32_t* R = t.reads;
    switch (t.kind) {
    case ZKM_STEP_BINARY_OP: {   // generate_binary_arithmetic_op: channels 0, 1 read rs, rt; channel 2 writes rd
        if (op || sa) return BAD_ENCODING;
        const uint32_t a = R[0], b = R[1];
        uint32_t f, out;
        switch (fn) {
        case 0x20: f = A_ADD; out = a + b; break;
        case 0x21: f = A_ADDU; out = a + b; break;
        case 0x22: f = A_SUB; out = a - b; break;
        case 0x23: f = A_SUBU; out = a - b; break;
        case 0x2A: f = A_SLT; out = (int32_t)a < (int32_t)b; break;
        case 0x2B: f = A_SLTU; out = a < b; break;
        default: return BAD_ENCODING;
        }
        s.cell(F_BINARY, 1);
        reg_read(s, 0, rs, a);
        reg_read(s, 1, rt, b);
        reg_write(s, 2, rd, out);
        s.arith(f, a, b);
        return OK;
    }
    case ZKM_STEP_BINARY_IMM_OP: {   // generate_binary_arithmetic_imm_op: channel 1 holds the sign-extended immediate as a write to rt
        const uint32_t a = R[0], b = sext(imm, 16);
        uint32_t f, out;
        switch (op) {
        case 0x08: f = A_ADDI; out = a + b; break;
        case 0x09: f = A_ADDIU; out = a + b; break;
        case 0x0A: f = A_SLTI; out = (int32_t)a < (int32_t)b; break;
        case 0x0B: f = A_SLTIU; out = a < b; break;
        default: return BAD_ENCODING;
        }
        s.cell(F_BINARY_IMM, 1);
        reg_read(s, 0, rs, a);
        reg_write(s, 1, rt, b);
        reg_write(s, 2, rt, out);
        s.arith(f, a, b);
        return OK;
    }
    case ZKM_STEP_LOGIC_OP: {   // generate_binary_logic_op
        if (op || sa || fn < 0x24 || fn > 0x27) return BAD_ENCODING;
        const uint32_t a = R[0], b = R[1];
        const uint32_t out = fn == 0x24 ? a & b : fn == 0x25 ? a | b : fn == 0x26 ? a ^ b : ~(a | b);
        s.cell(F_LOGIC, 1);
        reg_read(s, 0, rs, a);
        reg_read(s, 1, rt, b);
        reg_write(s, 2, rd, out);
        s.logic(fn - 0x24, a, b);
        return OK;
    }
    case ZKM_STEP_LOGIC_IMM_OP: {   // ANDI ORI XORI (generate_binary_logic_imm_op, operation.rs:260-284): channel 0 reads rs, channel 2 writes
                                    // rt; the immediate is zero-extended and no logic operation is pushed (the reference's push is commented out)
        if (op < 0x0C || op > 0x0E) return BAD_ENCODING;
        const uint32_t a = R[0];
        s.cell(F_LOGIC_IMM, 1);
        reg_read(s, 0, rs, a);
        reg_write(s, 2, rt, op == 0x0C ? a & imm : op == 0x0D ? a | imm : a ^ imm);
        return OK;
    }
    case ZKM_STEP_SHIFT: {   // generate_sllv / srlv / srav: channel 0 reads rs (the displacement), 1 rt, 3 the shift table, 2 writes rd
        if (op || sa || (fn != 4 && fn != 6 && fn != 7)) return BAD_ENCODING;
        const uint32_t d = R[0], a = R[1], n = d & 31;
        const uint32_t out = fn == 4 ? a << n : fn == 6 ? a >> n : (uint32_t)((int32_t)a >> n);
        s.cell(F_SHIFT, 1);
        reg_read(s, 0, rs, d);
        reg_read(s, 1, rt, a);
        s.chan(3, 1, 1, 0, SEG_SHIFT, d, R[2]);
        reg_write(s, 2, rd, out);
        s.arith(fn == 4 ? A_SLLV : fn == 6 ? A_SRLV : A_SRAV, a, d);
        return OK;
    }
    case ZKM_STEP_SHIFT_IMM: {   // generate_shift_imm: channel 1 reads rt, channel 0 carries the amount, 3 reads 2^sa, 2 writes rd
        if (op || rs || (fn != 0 && fn != 2 && fn != 3)) return BAD_ENCODING;
        const uint32_t a = R[0];
        const uint32_t out = fn == 0 ? a << sa : fn == 2 ? a >> sa : (uint32_t)((int32_t)a >> sa);
        s.cell(F_SHIFT_IMM, 1);
        reg_read(s, 1, rt, a);
        s.chan(0, 0, 0, 0, 0, 0, sa);
        s.chan(3, 1, 1, 0, SEG_SHIFT, sa, R[1]);
        reg_write(s, 2, rd, out);
        s.arith(fn == 0 ? A_SLL : fn == 2 ? A_SRL : A_SRA, a, sa);
        return OK;
    }
    case ZKM_STEP_BRANCH: {   // generate_branch (operation.rs:501-568); a compare against zero reads the register the rt field names, or
                              // register 0 under ZKM_STEP_FLAG_BRANCH_R0 (the reference decodes BGEZ's second source as register 0)
        unsigned flag;
        if (op == 4) flag = BR_IS_EQ;
        else if (op == 5) flag = BR_IS_NE;
        else if (op == 6 && rt == 0) flag = BR_IS_LE;
        else if (op == 7 && rt == 0) flag = BR_IS_GT;
        else if (op == 1 && rt == 0) flag = BR_IS_LT;
        else if (op == 1 && rt == 1) flag = BR_IS_GE;
        else return BAD_ENCODING;
        const bool r0 = (t.flags & ZKM_STEP_FLAG_BRANCH_R0) != 0;
        if (r0 && (op == 4 || op == 5)) return BAD_ENCODING;
        const uint32_t s1 = R[0], s2 = R[1];
        const int32_t i1 = (int32_t)s1, i2 = (int32_t)s2;
        const bool taken = flag == BR_IS_EQ ? i1 == i2 : flag == BR_IS_NE ? i1 != i2 : flag == BR_IS_LE ? i1 <= i2 : flag == BR_IS_GT ? i1 > i2
                           : flag == BR_IS_LT ? i1 < i2 : i1 >= i2;
        s.cell(F_BRANCH, 1);
        s.cell(flag, 1);
        reg_read(s, 0, rs, s1);
        reg_read(s, 1, r0 ? 0 : rt, s2);
        if (s1 == s2) s.cell(BR_EQ, 1);
        if (s1 > s2) s.cell(BR_GT, 1);
        if (s1 < s2) s.cell(BR_LT, 1);
        reg_write(s, 2, 0, s1 - s2);
        reg_write(s, 3, 0, s2 - s1);
        reg_write(s, 4, 0, ((s1 ^ s2) & 0x80000000u) != 0);
        reg_write(s, 5, 0, sext(imm, 16) << 2);
        if (taken) s.cell(BR_SHOULD_JUMP, 1);
        return OK;
    }
    case ZKM_STEP_JUMPS: {   // JR / JALR (generate_jump)
        if (op || rt || sa || (fn != 8 && fn != 9) || (fn == 8 && rd)) return BAD_ENCODING;
        s.cell(F_JUMPS, 1);
        reg_read(s, 0, rs, R[0]);
        if (fn == 9) reg_write(s, 1, rd, pc + 8);
        return OK;
    }
    case ZKM_STEP_JUMPI: {   // J / JAL (generate_jumpi): channel 2 carries next_pc[31:28] << 28
        if (op != 2 && op != 3) return BAD_ENCODING;
        s.cell(F_JUMPI, 1);
        s.chan(2, 0, 0, 0, 0, 0, t.next_pc & 0xF0000000u);
        if (op == 3) reg_write(s, 1, 31, pc + 8);
        return OK;
    }
    case ZKM_STEP_JUMPDIRECT: {   // BAL (generate_jumpdirect): channel 2 carries the sign-extended offset << 2; $31 <- pc + 8
        if (op != 1 || rs || rt != 0x11) return BAD_ENCODING;
        s.cell(F_JUMPDIRECT, 1);
        s.chan(2, 0, 0, 0, 0, 0, sext(imm, 16) << 2);
        reg_write(s, 1, 31, pc + 8);
        return OK;
    }
    case ZKM_STEP_M_OP_LOAD:
    case ZKM_STEP_M_OP_STORE: {   // generate_mload_general / generate_mstore_general: 0, 1 read rs, rt; 2 reads the word; 3 writes rt / the word
        const bool load = t.kind == ZKM_STEP_M_OP_LOAD;
        const uint32_t a = R[0], b = R[1], m = R[2], raw = a + sext(imm, 16), virt = raw & ~3u, k = raw & 3;
        unsigned io;
        uint32_t v;
        if (load) {
            switch (op) {
            case 0x20: io = IO_LB; v = sext((m >> (24 - 8 * k)) & 0xFF, 8); break;
            case 0x21: io = IO_LH; v = sext((m >> (16 - 8 * (k & 2))) & 0xFFFF, 16); break;
            case 0x22: io = IO_LWL; v = (b & ~(0xFFFFFFFFu << (8 * k))) | (m << (8 * k)); break;
            case 0x23: io = IO_LW; v = m; break;
            case 0x24: io = IO_LBU; v = (m >> (24 - 8 * k)) & 0xFF; break;
            case 0x25: io = IO_LHU; v = (m >> (16 - 8 * (k & 2))) & 0xFFFF; break;
            case 0x26: io = IO_LWR; v = (b & ~(0xFFFFFFFFu >> (24 - 8 * k))) | (m >> (24 - 8 * k)); break;
            case 0x30: io = IO_LL; v = m; break;
            default: return BAD_ENCODING;
            }
        } else {
            switch (op) {
            case 0x28: io = IO_SB; v = (m & ~(0xFFu << (24 - 8 * k))) | ((b & 0xFF) << (24 - 8 * k)); break;
            case 0x29: io = IO_SH; v = (m & ~(0xFFFFu << (16 - 8 * (k & 2)))) | ((b & 0xFFFF) << (16 - 8 * (k & 2))); break;
            case 0x2A: io = IO_SWL; v = (m & ~(0xFFFFFFFFu >> (8 * k))) | (b >> (8 * k)); break;
            case 0x2B: io = IO_SW; v = b; break;
            case 0x2E: io = IO_SWR; v = (m & ~(0xFFFFFFFFu << (24 - 8 * k))) | (b << (24 - 8 * k)); break;
            case 0x38: io = IO_SC; v = b; break;
            default: return BAD_ENCODING;
            }
        }
        s.cell(load ? F_LOAD : F_STORE, 1);
        s.cell(C_MEMIO + io, 1);
        s.cell(C_MEMIO + IO_AUX, 1);
        reg_read(s, 0, rs, a);
        reg_read(s, 1, rt, b);
        s.chan(2, 1, 1, t.context, SEG_CODE, virt, m);
        if (load) reg_write(s, 3, rt, v);
        else s.chan(3, 1, 0, t.context, SEG_CODE, virt, v);
        bits32(s, C_GEN, raw);
        bits32(s, C_GEN + 32, b);
        bits32(s, C_GEN + 64, m);
        if ((raw & 3) == 3) s.cell(C_GEN + 96, 1);
        return OK;
    }
    case ZKM_STEP_NOP:
        if (insn) return BAD_ENCODING;
        s.cell(F_NOP, 1);
        return OK;
    case ZKM_STEP_CLZ_OP:
    case ZKM_STEP_CLO_OP: {   // generate_count_op (count.rs): the bits, "the prefix is 1" flags and the inverses of prefix - 1
        const bool clz = t.kind == ZKM_STEP_CLZ_OP;
        if (op != 0x1C || rt || sa || fn != (clz ? 0x20u : 0x21u)) return BAD_ENCODING;
        const uint32_t a = R[0], x = clz ? a : ~a;
        uint32_t lz = 0;
        while (lz < 32 && !((x >> (31 - lz)) & 1)) lz++;
        s.cell(clz ? F_CLZ : F_CLO, 1);
        reg_read(s, 0, rs, a);
        reg_write(s, 1, rd, lz);
        bits32(s, C_GEN, x);
        for (unsigned j = 0; j < 31; j++) {
            const uint32_t partial = x >> (30 - j);
            if (partial == 1) s.cell(C_GEN + 32 + j, 1);
            s.inv(C_GEN + 64 + j, partial ? (gl_t)(partial - 1) : GL_P - 1);
        }
        if (x == 0) s.cell(C_GEN + 32 + 31, 1);
        s.inv(C_GEN + 64 + 31, x);
        return OK;
    }
    case ZKM_STEP_SIGNEXT8:
    case ZKM_STEP_SIGNEXT16:
    case ZKM_STEP_SWAPHALF: {   // SEB SEH WSBH (generate_signext, generate_swaphalf)
        const uint32_t want = t.kind == ZKM_STEP_SIGNEXT8 ? 0x10 : t.kind == ZKM_STEP_SIGNEXT16 ? 0x18 : 0x02;
        if (op != 0x1F || rs || fn != 0x20 || sa != want) return BAD_ENCODING;
        const uint32_t a = R[0];
        const uint32_t out = sa == 0x10 ? sext(a & 0xFF, 8) : sa == 0x18 ? sext(a & 0xFFFF, 16) : ((a & 0xFF00FF00u) >> 8) | ((a & 0x00FF00FFu) << 8);
        s.cell(sa == 0x10 ? F_SIGNEXT8 : sa == 0x18 ? F_SIGNEXT16 : F_SWAPHALF, 1);
        reg_read(s, 0, rt, a);
        reg_write(s, 1, rd, out);
        bits32(s, C_GEN + 32, a);
        return OK;
    }
    case ZKM_STEP_RDHWR: {   // generate_rdhwr: rt is written first, register 38 (local_user) is read for rd = 29
        if (op != 0x1F || rs || sa || fn != 0x3B) return BAD_ENCODING;
        const uint32_t out = rd == 0 ? 1 : rd == 29 ? R[0] : 0;
        s.cell(F_RDHWR, 1);
        reg_write(s, 0, rt, out);
        if (rd == 29) reg_read(s, 1, 38, R[0]);
        if (rd) s.cell(C_GEN + 99, rd);
        if (rd == 0) s.cell(C_GEN + 100, 1);
        if (rd == 29) s.cell(C_GEN + 101, 1);
        return OK;
    }
    case ZKM_STEP_MOVZ_OP:
    case ZKM_STEP_MOVN_OP: {   // generate_cond_mov_op
        const bool movn = t.kind == ZKM_STEP_MOVN_OP;
        if (op || sa || fn != (movn ? 0x0Bu : 0x0Au)) return BAD_ENCODING;
        const uint32_t a = R[0], b = R[1], c = R[2];
        const bool mov = movn ? b != 0 : b == 0;
        s.cell(movn ? F_MOVN : F_MOVZ, 1);
        reg_read(s, 0, rs, a);
        reg_read(s, 1, rt, b);
        reg_read(s, 2, rd, c);
        reg_write(s, 3, rd, mov ? a : c);
        s.chan(4, 0, 0, 0, 0, 0, mov);
        s.inv(C_GEN, b);
        return OK;
    }
    case ZKM_STEP_TEQ: {   // generate_teq: the operands differ (equal ones trap)
        if (op || rd || sa || fn != 0x34) return BAD_ENCODING;
        const uint32_t a = R[0], b = R[1];
        if (a == b) return BAD_OPERANDS;
        s.cell(F_TEQ, 1);
        reg_read(s, 0, rs, a);
        reg_read(s, 1, rt, b);
        s.inv(C_GEN, gl_sub(a, b));
        return OK;
    }
    case ZKM_STEP_EXT: {   // EXT rt, rs, lsb, size (generate_extract): rd = size - 1, sa = lsb
        const uint32_t lsb = sa, msb = sa + rd;
        if (op != 0x1F || fn != 0 || msb > 31) return BAD_ENCODING;
        const uint32_t a = R[0];
        s.cell(F_EXT, 1);
        reg_read(s, 0, rs, a);
        reg_write(s, 1, rt, (a >> lsb) & low_mask(rd + 1));
        bits32(s, C_GEN, a);
        s.cell(C_GEN + 32 + msb, 1);
        s.cell(C_GEN + 64 + lsb, 1);
        s.cell(C_GEN + 96, a & low_mask(msb + 1));
        s.cell(C_GEN + 97, a & low_mask(lsb));
        s.cell(C_GEN + 98, (uint64_t)1 << lsb);
        return OK;
    }
    case ZKM_STEP_INS: {   // INS rt, rs, lsb, size (generate_insert): rd = msb, sa = lsb
        const uint32_t lsb = sa, msb = rd;
        if (op != 0x1F || fn != 4 || msb < lsb) return BAD_ENCODING;
        const uint32_t a = R[0], b = R[1], size = msb - lsb + 1, mask = low_mask(size), keep = b & ~(mask << lsb);
        s.cell(F_INS, 1);
        reg_read(s, 0, rs, a);
        reg_read(s, 1, rt, b);
        reg_write(s, 2, rt, keep | ((a & mask) << lsb));
        bits32(s, C_GEN, a);
        s.cell(C_GEN + 32 + size - 1, 1);
        s.cell(C_GEN + 64 + lsb, 1);
        s.cell(C_GEN + 96, keep);
        s.cell(C_GEN + 97, a & mask);
        s.cell(C_GEN + 98, (uint64_t)1 << lsb);
        return OK;
    }
    case ZKM_STEP_ROR: {   // ROTR rd, rt, sa (generate_ror)
        if (op || rs != 1 || fn != 2) return BAD_ENCODING;
        const uint32_t a = R[0];
        s.cell(F_ROR, 1);
        reg_read(s, 0, rt, a);
        reg_write(s, 1, rd, sa ? (a >> sa) | (a << (32 - sa)) : a);
        bits32(s, C_GEN, a);
        s.cell(C_GEN + 64 + sa, 1);
        return OK;
    }
    case ZKM_STEP_MADDU: {   // generate_maddu: (hi, lo) += rs * rt; the carry out of 64 bits goes to the general columns
        if (op != 0x1C || rd || sa || fn != 1) return BAD_ENCODING;
        const uint32_t a = R[0], b = R[1], hi = R[2], lo = R[3];
        const uint64_t prod = (uint64_t)a * b, acc = ((uint64_t)hi << 32) | lo, sum = prod + acc;
        s.cell(F_MADDU, 1);
        reg_read(s, 0, rs, a);
        reg_read(s, 1, rt, b);
        reg_read(s, 2, 33, hi);
        reg_read(s, 3, 32, lo);
        reg_write(s, 4, 33, (uint32_t)(sum >> 32));
        reg_write(s, 5, 32, (uint32_t)sum);
        if (sum < prod) s.cell(C_GEN + 96, (uint64_t)1 << 32);
        return OK;
    }
    case ZKM_STEP_SYSCALL: {   // generate_syscall (syscall.rs:12-232); channels 0-3, then 6 and 7, then 4 and 5
        const uint32_t sub = (t.flags >> 8) & 15;
        if (insn != 0xC || sub == 4 || sub > 8) return BAD_ENCODING;
        const uint32_t a0 = R[1], a1 = R[2], a2 = R[3];
        constexpr unsigned cond = C_GEN, sysnum = C_GEN + 12, a0f = C_GEN + 24, a1f = C_GEN + 27;
        const bool zero = a0 == 0, std12 = a0 == 1 || a0 == 2;
        uint32_t v0 = 0, v1 = 0;
        bool other = !(zero || std12);
        s.cell(F_SYSCALL, 1);
        reg_read(s, 0, 2, R[0]);
        reg_read(s, 1, 4, a0);
        reg_read(s, 2, 5, a1);
        reg_read(s, 3, 6, a2);
        if (zero) s.cell(a0f, 1);
        if (std12) s.cell(a0f + 1, 1);
        if (sub) s.cell(sysnum + sub, 1);
        if (sub == ZKM_SYSCALL_MMAP) {
            const uint32_t heap = R[4];
            reg_read(s, 6, 34, heap);
            other = !zero;
            if (zero) {
                const uint32_t mid = a1 & 0xFFF, size = mid ? a1 + 0x1000 - mid : a1;
                s.cell(cond + 0, 1);
                s.cell(mid ? a1f : sysnum + 10, 1);
                if (mid && size) s.cell(sysnum + 9, size);
                s.cell(mid ? cond + 1 : cond + 2, 1);
                v0 = heap;
                reg_write(s, 7, 34, heap + size);
            } else {
                s.cell(cond + 3, 1);
                v0 = a0;
            }
        } else if (sub == ZKM_SYSCALL_BRK) {
            const uint32_t brk = R[4];
            reg_read(s, 6, 37, brk);
            s.cell(a0 > brk ? cond + 10 : cond + 11, 1);
            v0 = a0 > brk ? a0 : brk;
        } else if (sub == ZKM_SYSCALL_CLONE) {
            v0 = 1;
        } else if (sub == ZKM_SYSCALL_READ) {
            other = !zero;
            s.cell(zero ? cond + 5 : cond + 4, 1);
            if (!zero) { v0 = 0xFFFFFFFFu; v1 = 9; }
        } else if (sub == ZKM_SYSCALL_WRITE) {
            other = !std12;
            s.cell(std12 ? cond + 7 : cond + 6, 1);
            if (std12) v0 = a2;
            else { v0 = 0xFFFFFFFFu; v1 = 9; }
        } else if (sub == ZKM_SYSCALL_FCNTL) {
            if (zero) s.cell(cond + 8, 1);
            if (std12) s.cell(cond + 9, 1);
            if (std12) v0 = 1;
            else if (!zero) { v0 = 0xFFFFFFFFu; v1 = 9; }
        } else if (sub == ZKM_SYSCALL_SET_THREAD_AREA) {
            reg_write(s, 6, 38, a0);
        }
        if (other) s.cell(a0f + 2, 1);
        reg_write(s, 4, 2, v0);
        reg_write(s, 5, 7, v1);
        return OK;
    }
    default:
        return BAD_KIND;
    }
}

// the counting sink: what the host walk sums and the kernels scan
struct counts {
    uint32_t nmem = 0, nlogic = 0, narith = 0;
    GL_HD void cell(unsigned, uint64_t) {}
    GL_HD void inv(unsigned, gl_t) {}
    GL_HD void chan(unsigned, bool used, bool, uint32_t, uint32_t, uint32_t, uint32_t) { nmem += used; }
    GL_HD void logic(uint32_t, uint32_t, uint32_t) { nlogic++; }
    GL_HD void arith(uint32_t, uint32_t, uint32_t) { narith++; }
};

// the counts of any step (a RAW step names its used channels in reads[1]; a PAD step pushes nothing) and the walk's verdict
GL_HD int count(const zkm_cpu_step& t, counts& n) {
    if (t.kind == ZKM_STEP_PAD) return OK;
    if (t.kind == ZKM_STEP_RAW) {
        if (t.reads[1] >> NUM_GP_CHANNELS) return BAD_ENCODING;
        for (unsigned i = 0; i < NUM_GP_CHANNELS; i++) n.nmem += (t.reads[1] >> i) & 1;
        return OK;
    }
    return walk(t, n);
}

}  // namespace zkm_step
