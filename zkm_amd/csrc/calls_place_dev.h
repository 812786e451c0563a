// calls_place_dev.h -- where the rows of a segment's calls go and what the step list gets for each of them, stated once for host and
// device: the `place` statements of sha_calls.hip, keccak_calls.hip and io_calls.hip and the instruction records' expansion of
// insn_rows.hip (each file reads its own under the name it always had), and on top of them ONE statement per kind of a generated row's
// record -- its RAW mask and its clock (zkm_row_rec).  The host functions zkm_*_calls_steps / zkm_insn_rows_steps and the placement
// kernel of calls_stage.hip both read that statement, so a record placed on the device is the record the host would have placed.
#pragma once
#include "cpu_steps_dev.h"

// what the step list gets for one generated row: raw_step(raw_base + row, mask) at `clock`
struct zkm_row_rec {
    uint32_t mask;
    uint64_t clock;
};

// ---- sha_calls.hip: the one statement of where things go.  E extend calls, then C compress calls, in every list.
namespace zkm_sha_place {
constexpr unsigned EXT_ROUNDS = 48, EXT_ROWS = 2 * EXT_ROUNDS, EXT_MEM = 16 * EXT_ROUNDS, EXT_LOGIC = 4 * EXT_ROUNDS;
constexpr unsigned CMP_ROWS = 11, CMP_MEM = 4 * 8 + 4 * 64, CMP_LOGIC = 12 * 64;
constexpr unsigned CMP_HX = 0, CMP_W0 = 1, CMP_SPONGE = 9, CMP_WRITE = 10;       // a compress call's rows
constexpr uint32_t MASK_EXT_READ = 0x1F, MASK_CMP = 0xFF, MASK_SPONGE = 0;       // the channels a row uses
// rows: extend call e owns 96 e + 2 r (read row of round r) and 96 e + 2 r + 1 (its sponge row); compress call c owns 96 E + 11 c + 0..10
GL_HD size_t ext_row(size_t e, unsigned r, unsigned sponge) { return EXT_ROWS * e + 2 * r + sponge; }
GL_HD size_t cmp_row(size_t E, size_t c, unsigned k) { return EXT_ROWS * E + CMP_ROWS * c + k; }
// clocks, counted from the sponge row's S = timestamp / NUM_CHANNELS: an extend round's read row is one clock before its sponge row at
// S + 2 r; a compress call's hx row is at S - 9, w row k at S - 8 + k, the sponge row at S, the write row at S + 1
GL_HD uint64_t ext_clock(uint64_t S, unsigned r, unsigned sponge) { return S + 2 * r - 1 + sponge; }
GL_HD uint64_t cmp_clock(uint64_t S, unsigned k) { return S - 9 + k; }
GL_HD uint32_t cmp_mask(unsigned k) { return k == CMP_SPONGE ? MASK_SPONGE : MASK_CMP; }
GL_HD size_t mem_base(size_t E, size_t e_or_c, bool compress) { return compress ? EXT_MEM * E + CMP_MEM * e_or_c : EXT_MEM * e_or_c; }
GL_HD size_t logic_base(size_t E, size_t e_or_c, bool compress) { return compress ? EXT_LOGIC * E + CMP_LOGIC * e_or_c : EXT_LOGIC * e_or_c; }
// the record of row j of the calls' rows: an extend call's 48 (read row, sponge row) pairs, then a compress call's eleven rows
GL_HD zkm_row_rec row_rec(const uint64_t* emeta, size_t E, const uint64_t* cmeta, size_t j) {
    if (j < EXT_ROWS * E) {
        const size_t e = j / EXT_ROWS;
        const unsigned r = (unsigned)(j % EXT_ROWS) / 2, sponge = (unsigned)(j & 1);
        return {sponge ? MASK_SPONGE : MASK_EXT_READ, ext_clock(emeta[4 * e + 3] / 10, r, sponge)};
    }
    const size_t c = (j - EXT_ROWS * E) / CMP_ROWS;
    const unsigned k = (unsigned)((j - EXT_ROWS * E) % CMP_ROWS);
    return {cmp_mask(k), cmp_clock(cmeta[8 * c + 3] / 10, k)};
}
}  // namespace zkm_sha_place

// ---- keccak_calls.hip: the one statement of where things go, for a call of L >= 1 input bytes (the host has refused a length that is
// no multiple of 4 in a call without ZKM_SPONGE_PADDED_TAIL)
namespace zkm_keccak_place {
constexpr unsigned RATE = 136, RATE_U32 = 34, STATE = 25;                         // KECCAK_RATE_BYTES, KECCAK_RATE_U32S, the state's u64 words
constexpr uint32_t MASK_SPONGE = 0, MASK_WRITE = 0xFF;
GL_HD size_t words(size_t L) { return (L + 3) / 4; }                              // W: the memory words read, the last one maybe in part
GL_HD size_t read_rows(size_t L) { return (words(L) + 7) / 8; }                   // R: eight words a row
GL_HD size_t blocks(size_t L) { return L / RATE + 1; }                            // B: the last one carries pad10*1 (it may hold nothing else)
// what a call adds to each list
GL_HD size_t rows(size_t L) { return read_rows(L) + 2; }
GL_HD size_t mem(size_t L) { return L; }
GL_HD size_t logic(size_t L) { return RATE_U32 * blocks(L); }
// a call's rows: read rows 0 .. R - 1, the sponge row, the write row
GL_HD size_t sponge_row(size_t L) { return read_rows(L); }
GL_HD size_t write_row(size_t L) { return read_rows(L) + 1; }
// clocks, counted from the sponge row's S = timestamp / NUM_CHANNELS: read row j at S - R + j, the write row at S + 1
GL_HD uint64_t row_clock(uint64_t S, size_t L, size_t j) { return S - read_rows(L) + j; }
GL_HD unsigned read_channels(size_t L, size_t j) { return words(L) - 8 * j < 8 ? (unsigned)(words(L) - 8 * j) : 8; }
GL_HD uint32_t row_mask(size_t L, size_t j) { return j < read_rows(L) ? (1u << read_channels(L, j)) - 1 : j == sponge_row(L) ? MASK_SPONGE : MASK_WRITE; }
// the word whose address the sponge row carries: the first of the final block (0 where the input ends before it)
GL_HD size_t final_word(size_t L) { return L / RATE * RATE_U32; }
// the record of row j of call k
GL_HD zkm_row_rec row_rec(const uint64_t* off, const uint64_t* meta, size_t k, size_t j) {
    const size_t L = off[k + 1] - off[k];
    return {row_mask(L, j), row_clock(meta[4 * k + 3] / 10, L, j)};
}
}  // namespace zkm_keccak_place

// ---- io_calls.hip: the one statement of where things go, for a call of kind `kind` with L bytes (the host has refused the lengths a
// kind does not take)
namespace zkm_io_place {
constexpr uint32_t NKINDS = 4;
constexpr uint64_t PREIMAGE_HASH = 0x30001000, PREIMAGE_MAP = 0x31000000;   // load_preimage's two addresses
constexpr unsigned POSEIDON_RATE_BYTES = 32;
GL_HD size_t ceil_div(size_t a, size_t b) { return (a + b - 1) / b; }
// the words a call moves through channels beyond its first row's fixed part: hint read / commit W, verify 8, preimage Q = 1 + ceil(C / 4)
GL_HD size_t words(uint32_t kind, size_t L) {
    return kind == ZKM_IO_HINT_READ ? ceil_div(L, 4) : kind == ZKM_IO_COMMIT ? L / 4 : kind == ZKM_IO_VERIFY ? 8 : 1 + ceil_div(L - 32, 4);
}
// a preimage call's hash row stands in front of its write rows
GL_HD size_t lead_rows(uint32_t kind) { return kind == ZKM_IO_PREIMAGE ? 1 : 0; }
// what a call adds: rows (a hint read or commit of no word still pushes one row) and used channels
GL_HD size_t rows(uint32_t kind, size_t L) {
    const size_t r = ceil_div(words(kind, L), 8);
    return lead_rows(kind) + (r ? r : 1);
}
GL_HD size_t mem(uint32_t kind, size_t L) { return 8 * lead_rows(kind) + words(kind, L); }
GL_HD uint64_t row_clock(uint64_t timestamp, size_t j) { return timestamp / 10 + j; }
// the used channels of a call's row j: always the low ones
GL_HD unsigned channels(uint32_t kind, size_t L, size_t j) {
    if (j < lead_rows(kind)) return 8;
    const size_t left = words(kind, L) - 8 * (j - lead_rows(kind));
    return left < 8 ? (unsigned)left : 8;
}
GL_HD uint32_t row_mask(uint32_t kind, size_t L, size_t j) { return (1u << channels(kind, L, j)) - 1; }
// the address of the last word a call touches, given its meta's address (the hash row's are constants)
GL_HD uint64_t last_address(uint32_t kind, size_t L, uint64_t address) {
    const size_t w = words(kind, L);
    return address + 4 * (w ? w - 1 : 0);
}
// the record of row j of call k
GL_HD zkm_row_rec row_rec(const uint32_t* kinds, const uint64_t* off, const uint64_t* meta, size_t k, size_t j) {
    const size_t L = off[k + 1] - off[k];
    return {row_mask(kinds[k], L, j), row_clock(meta[4 * k + 3], j)};
}
}  // namespace zkm_io_place

// ---- insn_rows.hip: one record of the thirteen instructions no step kind takes, as a whole row
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

// the record of an instruction row: the channels its expansion uses (0 for a record expand refuses: the host walk has refused it)
GL_HD zkm_row_rec row_rec(const zkm_cpu_step& t, uint64_t clock) {
    shape s;
    if (expand(t, 0, s) != OK) s = shape{};
    return {s.mask, clock};
}

}  // namespace zkm_insn
