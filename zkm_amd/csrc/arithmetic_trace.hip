// arithmetic_trace.hip -- ArithmeticStark witness from the raw arithmetic operations (arithmetic_stark.rs:127-185,
// tests/arith_fixtures.py generate_trace).
//
// The reference turns each Operation into one or two rows (binary_op_to_rows, mod.rs:237-313), pads with zero rows to
// max(2^16, next_pow2(rows)), then fills RANGE_COUNTER and counts every value of the 18 shared columns into RC_FREQUENCIES.  Here:
//   (1) k_arith_count  validation flags (one atomicOr per wave) and the row count of each operation (1 or 2);
//   (2) scan           exclusive scan of those counts (scan_dev.h): each operation's first row; the total is the row count;
//   (3) k_arith_rows   one thread per operation writes its rows, every column; the same persistent workgroups then write the zero
//                      rows.  The shared-column values go from registers into an LDS histogram of 2^16 16-bit counters (two per
//                      word, 128 KiB: one 512-thread workgroup per CU); zeros are counted in registers, the padding rows' zeros in
//                      closed form.  The LDS counters are added into a 2^16-bin uint64 histogram in global memory before any of them
//                      could pass 2^16 - 1;
//   (4) k_arith_freq   RC_FREQUENCIES rows 0 .. 2^16 - 1 from that histogram (the rows below write the column's other rows).
// Only the row count and the flags come back to the host before the output is written.
// Every kernel serves K segments in one launch (zkm_seg_args: its segment's descriptor from blockIdx.z); a lone table is K = 1.
#include <algorithm>
#include <vector>

#include "scan_dev.h"
#include "zkm_internal.h"

#undef ZKM_CONST
#define ZKM_CONST static __device__ const
#include "arith_constants.inc"
#undef ZKM_CONST

namespace {

constexpr int AT_THREADS = SCAN_THREADS;             // count kernel
constexpr int AR_THREADS = 512;                      // row kernel: one operation per thread and iteration
constexpr int AR_HIST_WORDS = 1 << 15;               // 2^16 16-bit counters, two per word
constexpr uint32_t RANGE_MAX = 1u << 16;
constexpr int NSHARED = 18;                          // columns 26 .. 43
// Per iteration a workgroup adds at most 2 rows x 18 values per thread to its counters; they go to global memory whenever the adds
// since the last flush may exceed this, so no 16-bit counter can pass 2^16 - 1.
constexpr uint32_t AR_FLUSH_AT = (RANGE_MAX - 1) - 2 * NSHARED * AR_THREADS;
constexpr unsigned AT_MAX_LOG_N = ZKM_ARITHMETIC_MAX_LOG_N;

// row filters (arithmetic/columns.rs; tests/arith_fixtures.py IS_*)
enum : uint32_t {
    IS_ADD, IS_ADDU, IS_ADDI, IS_ADDIU, IS_SUB, IS_SUBU, IS_MULT, IS_MULTU, IS_MUL, IS_DIV, IS_DIVU, IS_SLLV, IS_SRLV, IS_SRAV, IS_SLL,
    IS_SRL, IS_SRA, IS_SLT, IS_SLTU, IS_SLTI, IS_SLTIU, IS_LUI, IS_MFHI, IS_MTHI, IS_MFLO, IS_MTLO, NUM_OPS
};
// shared columns, as offsets into s[18] (column - 26)
enum : int { IN0 = 0, IN1 = 2, IN2 = 4, OUT = 6, AUX0 = 8, AUX1 = 10, AUX2 = 12, QUOT_ABS = 14, REM_ABS = 16,
             OUT_LO = 6, OUT_HI = 8, MULT_AUX_LO = 10, MULT_AUX_HI = 14,
             NV_OUT_AUX_RED = 0, NV_AUX_LO = 3, NV_AUX_HI = 6, NV_SUM = 10, NV_NEG_BORROW = 14 };
constexpr int COL_RC_FREQ = 45;   // (the row store walks the columns in order: 26 filters, 18 shared, RANGE_COUNTER, RC_FREQUENCIES, 8 AUX_EXTRA)
constexpr int64_t ABS_MAX = 1 << 20;

// failure flags (bit -> message in the host code)
enum : uint32_t { BAD_OP = 1, BAD_DIV_ZERO = 2, BAD_DIV_OVERFLOW = 4, BAD_IMM = 8, BAD_SHIFT = 16 };

__device__ __forceinline__ bool two_rows(uint32_t op) {
    return op == IS_DIV || op == IS_DIVU || op == IS_SRL || op == IS_SRLV || op == IS_SRA || op == IS_SRAV;
}

// ---- (1) flags and row counts
struct count_seg {
    const uint32_t* ops;
    uint64_t* cnt;
    unsigned* flags;
    uint32_t nops;
};
__global__ __launch_bounds__(AT_THREADS) void k_arith_count(zkm_seg_args<count_seg> S) {
    const count_seg& A = S.v[blockIdx.z];
    const uint32_t* __restrict__ ops = A.ops;
    uint64_t* __restrict__ cnt = A.cnt;
    unsigned* __restrict__ flags = A.flags;
    const uint32_t nops = A.nops;
    const size_t i = (size_t)blockIdx.x * AT_THREADS + threadIdx.x;
    uint32_t bad = 0;
    if (i < nops) {
        const uint32_t op = ops[3 * i], a = ops[3 * i + 1], b = ops[3 * i + 2];
        if (op >= NUM_OPS) bad |= BAD_OP;
        if ((op == IS_DIV || op == IS_DIVU) && b == 0) bad |= BAD_DIV_ZERO;
        if (op == IS_DIV && a == 0x80000000u && b == 0xFFFFFFFFu) bad |= BAD_DIV_OVERFLOW;
        if ((op == IS_ADDI || op == IS_ADDIU || op == IS_SLTI || op == IS_SLTIU) && (uint32_t)(int32_t)(int16_t)b != b) bad |= BAD_IMM;
        if ((op == IS_SLL || op == IS_SRL || op == IS_SRA || op == IS_SRAV) && b > 31) bad |= BAD_SHIFT;
        cnt[i] = two_rows(op) ? 2 : 1;
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) bad |= __shfl_xor(bad, o);
    if ((threadIdx.x & 63) == 0 && bad) atomicOr(flags, bad);
}

// ---- (3) the row generators of arith_fixtures.rows_for, in 16-bit limbs and int64 intermediates.  A row is its 18 shared values
// s[0..17] (columns 26 .. 43) and its 8 AUX_EXTRA words x[0..7] (columns 46 .. 53); the filter column is set at the store.
__device__ __forceinline__ void put(uint32_t* s, int c, uint32_t v) {
    s[c] = v & 0xFFFF;
    s[c + 1] = v >> 16;
}
__device__ __forceinline__ uint32_t lo16(int64_t v) { return (uint32_t)(v & 0xFFFF); }
__device__ __forceinline__ uint32_t hi16(int64_t v) { return (uint32_t)((v >> 16) & 0xFFFF); }
__device__ __forceinline__ uint32_t abs32(uint32_t x) { return x >> 31 ? 0u - x : x; }

// mul.rs:62-96 with two limbs: OUT, AUX0 (low halves of the carries + 2^20), AUX1 (high halves)
__device__ __forceinline__ void gen_mul(uint32_t* s, int64_t a0, int64_t a1, int64_t b0, int64_t b1) {
    const int64_t u0 = a0 * b0, u1 = a0 * b1 + a1 * b0;
    const int64_t o0 = u0 & 0xFFFF, t = u1 + (u0 >> 16), o1 = t & 0xFFFF, cy = t >> 16;
    const int64_t c0 = -((u0 - o0) >> 16) + ABS_MAX, c1 = -cy + ABS_MAX;
    s[OUT] = (uint32_t)o0;
    s[OUT + 1] = (uint32_t)o1;
    s[AUX0] = lo16(c0);
    s[AUX0 + 1] = lo16(c1);
    s[AUX1] = hi16(c0);
    s[AUX1 + 1] = hi16(c1);
}

// mult.rs:70-113 with four limbs: OUT_LO, MULT_AUX_LO, MULT_AUX_HI
__device__ __forceinline__ void gen_mult(uint32_t* s, const int64_t* l, const int64_t* r) {
    int64_t un[4], out[4], cy = 0;
#pragma unroll
    for (int d = 0; d < 4; d++) {
        int64_t acc = 0;
#pragma unroll
        for (int i = 0; i <= d; i++) acc += l[i] * r[d - i];
        const int64_t t = acc + cy;
        out[d] = t & 0xFFFF;
        cy = t >> 16;
        un[d] = acc - out[d];
    }
    int64_t q[4];
    q[0] = -(un[0] >> 16);
    q[1] = (q[0] - un[1]) >> 16;
    q[2] = (q[1] - un[2]) >> 16;
    q[3] = -cy;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        s[OUT_LO + i] = (uint32_t)out[i];
        s[MULT_AUX_LO + i] = lo16(q[i] + ABS_MAX);
        s[MULT_AUX_HI + i] = hi16(q[i] + ABS_MAX);
    }
}

// div.rs:182-262 (generate_modular_op) for a 32-bit input and a nonzero modulus below 2^32 (every valid operation's case: the
// modulus-zero branch needs a zero divisor or 1 << shift = 0), into the second row: OUT_AUX_RED, AUX_LO, AUX_HI (MODULUS_IS_ZERO and
// DENOM_IS_ZERO stay 0).  Returns the remainder.
__device__ __forceinline__ uint32_t gen_modular(uint32_t* s, uint32_t inp, uint32_t modulus) {
    const uint32_t out = inp % modulus, quot = inp / modulus;
    put(s, NV_OUT_AUX_RED, (uint32_t)(((1ull << 32) - modulus) + out));
    const int64_t p0 = inp & 0xFFFF, p1 = inp >> 16, m0 = modulus & 0xFFFF, m1 = modulus >> 16;
    const int64_t o0 = out & 0xFFFF, o1 = out >> 16, q0 = quot & 0xFFFF, q1 = quot >> 16;
    const int64_t c0 = p0 - o0 - q0 * m0, c1 = p1 - o1 - q0 * m1 - q1 * m0, c2 = -q1 * m1;
    int64_t r[3];
    r[0] = -(c0 >> 16);
    r[1] = (r[0] - c1) >> 16;
    r[2] = (r[1] - c2) >> 16;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        s[NV_AUX_LO + i] = lo16(r[i] + ABS_MAX);
        s[NV_AUX_HI + i] = hi16(r[i] + ABS_MAX);
    }
    return out;
}

// eval_aux_sign_extend (sra.rs:284-300) of shift sh: Horner pairs of ZKM_ARITH_SIGN_EXTEND_POLY from the top, the 16 partial sums;
// words 0..7 go to SRA's first row, 8..15 to its second.  One table per workgroup in LDS (a loop-invariant copy of the polynomial
// would sit in registers).
__device__ __forceinline__ void sign_extend_table(uint64_t (*sext)[16]) {
    if (threadIdx.x < 32) {
        const uint64_t sh = threadIdx.x, sh2 = sh * sh;
        uint64_t acc = 0;
        for (int k = 0; k < 16; k++) {
            const int i = 15 - k;
            acc = gl_add(gl_add(ZKM_ARITH_SIGN_EXTEND_POLY[2 * i], gl_mul(ZKM_ARITH_SIGN_EXTEND_POLY[2 * i + 1], sh)), gl_mul(acc, sh2));
            sext[sh][k] = acc;
        }
    }
}

// row j (0 or 1) of Operation::binary(op, a, b) (op valid; j = 1 only for two_rows(op)).  s and x arrive zeroed.
__device__ __forceinline__ void gen_row(uint32_t op, uint32_t a, uint32_t b, int j, const uint64_t (*sext)[16], uint32_t* s, uint64_t* x) {
    switch (op) {
    case IS_ADD: case IS_ADDU: case IS_ADDI: case IS_ADDIU: case IS_SUB: case IS_SUBU: {   // addcy.rs:12-39
        put(s, IN0, a);
        put(s, IN1, b);
        const bool sub = op == IS_SUB || op == IS_SUBU;
        const uint64_t res = sub ? (uint64_t)a - b : (uint64_t)a + b;
        s[AUX0] = sub ? a < b : res >> 32;
        put(s, OUT, (uint32_t)res);
        break;
    }
    case IS_MUL:                                                                            // mul.rs:98-107
        put(s, IN0, a);
        put(s, IN1, b);
        gen_mul(s, a & 0xFFFF, a >> 16, b & 0xFFFF, b >> 16);
        break;
    case IS_SLT: case IS_SLTU: case IS_SLTI: case IS_SLTIU: {                                // slt.rs:13-46
        put(s, IN0, a);
        put(s, IN1, b);
        const uint32_t cy = a < b;
        const bool sgn = op == IS_SLT || op == IS_SLTI;
        const uint32_t rd = sgn ? (int32_t)a < (int32_t)b : cy;
        const uint32_t cy_val = sgn && ((a ^ b) >> 31) ? (1u << 16) | (1 - cy) : cy;
        put(s, AUX0, a - b);
        put(s, AUX1, cy_val);
        put(s, OUT, rd);
        break;
    }
    case IS_MULT: case IS_MULTU: {                                                          // mult.rs:12-68
        put(s, IN0, a);
        put(s, IN1, b);
        int64_t l[4] = {a & 0xFFFF, a >> 16, 0, 0}, r[4] = {b & 0xFFFF, b >> 16, 0, 0};
        if (op == IS_MULT) {
            x[0] = a >> 31;
            x[1] = b >> 31;
            s[IN2] = (a >> 16) ^ 0x8000;
            s[IN2 + 1] = (b >> 16) ^ 0x8000;
            l[2] = l[3] = 0xFFFF * (int64_t)(a >> 31);
            r[2] = r[3] = 0xFFFF * (int64_t)(b >> 31);
        }
        gen_mult(s, l, r);
        break;
    }
    case IS_DIVU: {                                                                         // div.rs:21-137, 139-180
        if (j == 0) {
            put(s, IN0, a);
            put(s, IN1, b);
            put(s, OUT_LO, a / b);
            put(s, OUT_HI, a % b);
        } else {
            gen_modular(s, a, b);
        }
        break;
    }
    case IS_DIV: {
        const uint32_t quot = (uint32_t)((int32_t)a / (int32_t)b), rem = (uint32_t)((int32_t)a % (int32_t)b);
        if (j == 0) {
            put(s, IN0, a);
            put(s, IN1, b);
            put(s, IN2, abs32(a));
            put(s, OUT_LO, quot);
            put(s, OUT_HI, rem);
            put(s, AUX2, abs32(b));
            put(s, QUOT_ABS, abs32(quot));
            put(s, REM_ABS, abs32(rem));
        } else {
            s[NV_SUM + 0] = (a >> 16) ^ 0x8000;
            s[NV_SUM + 1] = (b >> 16) ^ 0x8000;
            s[NV_SUM + 2] = (quot >> 16) ^ 0x8000;
            s[NV_SUM + 3] = (rem >> 16) ^ 0x8000;
            s[NV_NEG_BORROW + 0] = a >> 31;
            s[NV_NEG_BORROW + 1] = (a & 0xFFFF) != 0;
            s[NV_NEG_BORROW + 2] = b >> 31;
            s[NV_NEG_BORROW + 3] = (b & 0xFFFF) != 0;
            x[0] = quot >> 31;
            x[1] = (quot & 0xFFFF) != 0;
            x[2] = rem >> 31;
            x[3] = (rem & 0xFFFF) != 0;
            x[4] = (a ^ b) >> 31;
            gen_modular(s, abs32(a), abs32(b));
        }
        break;
    }
    case IS_LUI:                                                                            // lui.rs:14-29
        put(s, IN0, a);
        put(s, IN1, 1u << 16);
        gen_mul(s, a & 0xFFFF, a >> 16, 0, 1);
        break;
    case IS_SLL: case IS_SLLV: case IS_SRL: case IS_SRLV: {                                 // shift.rs:42-90
        const uint32_t sh = b & 31;
        if (op == IS_SLL || op == IS_SLLV) {
            put(s, IN0, b);
            put(s, IN1, a);
            put(s, IN2, 1u << sh);
            gen_mul(s, a & 0xFFFF, a >> 16, (1u << sh) & 0xFFFF, (1u << sh) >> 16);
        } else if (j == 0) {
            put(s, IN0, b);
            put(s, IN1, a);
            put(s, IN2, 1u << sh);
            put(s, OUT, a >> sh);
            put(s, AUX0, a & ((1u << sh) - 1));
        } else {
            gen_modular(s, a, 1u << sh);
        }
        break;
    }
    case IS_SRA: case IS_SRAV: {                                                            // sra.rs:31-90, shift < 32
        const uint32_t sh = b;
#pragma unroll
        for (int k = 0; k < 8; k++) x[k] = sext[sh][8 * j + k];
        if (j == 0) {
            put(s, IN0, sh);
            put(s, IN1, a);
            put(s, IN2, 1u << sh);
            put(s, OUT, (uint32_t)((int32_t)a >> sh));
            put(s, AUX0, a & ((1u << sh) - 1));
            put(s, AUX2, a >> sh);
            s[AUX2 + 2] = (a >> 16) ^ 0x8000;
            s[AUX2 + 3] = a >> 31;
        } else {
            put(s, AUX2, (uint32_t)((((1ull << sh) - 1) << ((32 - sh) % 32)) & 0xFFFFFFFFull));
            s[AUX2 + 2] = sh * sh;
            gen_modular(s, a, 1u << sh);
        }
        break;
    }
    default:                                                                                // lo_hi.rs:13-22
        put(s, IN0, a);
        put(s, OUT, a);
        break;
    }
}

struct rows_args {
    const uint32_t* ops;
    const uint64_t* start;      // first row of each operation; start[nops] = rows
    uint32_t nops;
    uint64_t rows;
    size_t n;
    unsigned long long* hist;   // 2^16 bins (RC_FREQUENCIES before the padding zeros)
    unsigned* bad;              // a shared value of 2^16 or more
    gl_t* out;
};

// every column of row r; RC_FREQUENCIES rows below 2^16 belong to k_arith_freq.  One address register pair walks the columns (the
// empty asm keeps the compiler from holding 54 column bases in scalar registers, which it then spills).
__device__ __forceinline__ void store_row(gl_t* __restrict__ out, size_t n, size_t r, uint32_t filt, const uint32_t* s, const uint64_t* x) {
    gl_t* p = out + r;
#define AT_NEXT(v)                 \
    do {                           \
        *p = (v);                  \
        p += n;                    \
        asm volatile("" : "+v"(p)); \
    } while (0)
#pragma unroll
    for (int c = 0; c < NUM_OPS; c++) AT_NEXT(c == (int)filt);
#pragma unroll
    for (int c = 0; c < NSHARED; c++) AT_NEXT(s[c]);
    AT_NEXT(r < RANGE_MAX ? r : RANGE_MAX - 1);
    if (r >= RANGE_MAX) *p = 0;
    p += n;
#pragma unroll
    for (int c = 0; c < 8; c++) AT_NEXT(x[c]);
#undef AT_NEXT
}

// one row's shared values into the counters: zeros in a register, the rest into the 16-bit LDS counters; returns how many went there
__device__ __forceinline__ uint32_t count_row(const uint32_t* s, uint32_t* h, uint64_t& zeros, unsigned* bad) {
    uint32_t added = 0;
#pragma unroll
    for (int c = 0; c < NSHARED; c++) {
        const uint32_t v = s[c];
        if (v == 0) {
            zeros++;
        } else if (v < RANGE_MAX) {
            atomicAdd(&h[v >> 1], 1u << ((v & 1) * 16));
            added++;
        } else {
            atomicOr(bad, 1u);
        }
    }
    return added;
}

// every LDS counter into the global bins, and back to zero
__device__ __forceinline__ void flush(uint32_t* h, unsigned long long* hist) {
    for (int w = threadIdx.x; w < AR_HIST_WORDS; w += AR_THREADS) {
        const uint32_t v = h[w];
        if (v) {
            if (v & 0xFFFF) atomicAdd(&hist[2 * w], (unsigned long long)(v & 0xFFFF));
            if (v >> 16) atomicAdd(&hist[2 * w + 1], (unsigned long long)(v >> 16));
            h[w] = 0;
        }
    }
}

__global__ __launch_bounds__(AR_THREADS) void k_arith_rows(zkm_seg_args<rows_args> S) {
    __shared__ uint32_t h[AR_HIST_WORDS];
    __shared__ uint32_t added;
    __shared__ uint64_t sext[32][16];
    const rows_args& A = S.v[blockIdx.z];
    gl_t* __restrict__ out = A.out;
    // (a workgroup with neither operations nor zero rows of its segment leaves before it clears 128 KiB of counters)
    if ((size_t)blockIdx.x * AR_THREADS >= A.nops && A.rows + (size_t)blockIdx.x * AR_THREADS >= A.n) return;
    for (int w = threadIdx.x; w < AR_HIST_WORDS; w += AR_THREADS) h[w] = 0;
    sign_extend_table(sext);
    if (threadIdx.x == 0) added = 0;
    __syncthreads();
    const size_t n = A.n;
    uint64_t zeros = 0;
    // operations: the loop bound is uniform, so every thread reaches every barrier
    for (size_t base = (size_t)blockIdx.x * AR_THREADS; base < A.nops; base += (size_t)gridDim.x * AR_THREADS) {
        const size_t i = base + threadIdx.x;
        uint32_t mine = 0;
        if (i < A.nops) {
            const uint32_t op = A.ops[3 * i], a = A.ops[3 * i + 1], b = A.ops[3 * i + 2];
            const size_t r = A.start[i];
            for (int j = 0; j < 1 + two_rows(op); j++) {
                uint32_t s[NSHARED] = {};
                uint64_t x[8] = {};
                gen_row(op, a, b, j, sext, s, x);
                store_row(out, n, r + j, j == 0 ? op : NUM_OPS, s, x);
                mine += count_row(s, h, zeros, A.bad);
            }
        }
#pragma unroll
        for (int o = 32; o; o >>= 1) mine += __shfl_xor(mine, o);
        if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&added, mine);
        __syncthreads();
        const bool full = added > AR_FLUSH_AT;
        __syncthreads();   // (every thread has read `added` before it changes: the branch is uniform)
        if (full) {
            if (threadIdx.x == 0) added = 0;
            flush(h, A.hist);
            __syncthreads();
        }
    }
    // zero rows (their 18 zeros per row are added by k_arith_freq)
    for (size_t r = A.rows + (size_t)blockIdx.x * AR_THREADS + threadIdx.x; r < n; r += (size_t)gridDim.x * AR_THREADS) {
        const uint32_t s[NSHARED] = {};
        const uint64_t x[8] = {};
        store_row(out, n, r, NUM_OPS, s, x);
    }
    __syncthreads();
    flush(h, A.hist);
#pragma unroll
    for (int o = 32; o; o >>= 1) zeros += __shfl_xor(zeros, o);
    if ((threadIdx.x & 63) == 0 && zeros) atomicAdd(&A.hist[0], (unsigned long long)zeros);
}

// ---- (4) RC_FREQUENCIES rows 0 .. 2^16 - 1 (n >= 2^16)
struct freq_seg {
    const unsigned long long* hist;
    uint64_t pad_zeros;
    size_t n;
    gl_t* out;
};
__global__ __launch_bounds__(AT_THREADS) void k_arith_freq(zkm_seg_args<freq_seg> S) {
    const freq_seg& A = S.v[blockIdx.z];
    const uint32_t v = blockIdx.x * AT_THREADS + threadIdx.x;
    if (v < RANGE_MAX) A.out[COL_RC_FREQ * A.n + v] = A.hist[v] + (v == 0 ? A.pad_zeros : 0);
}

size_t next_pow2(size_t v) {
    size_t p = 1;
    while (p < v) p <<= 1;
    return p;
}
size_t blocks_for(size_t items, size_t per) { return (items + per - 1) / per; }

}  // namespace

// ---- host phases (zkm_internal.h zkm_arith_job): zkm_arithmetic_trace runs them back to back for one table, segment_ops.hip for the
// K segments of a call beside the Memory witness's
void zkm_arithmetic_count(zkm_arith_job* j, size_t nseg) {
    zkm_ctx* c = j->c;
    count_seg cs[ZKM_MAX_SEG];
    scan_seg sc[ZKM_MAX_SEG];
    std::vector<zkm_scratch> part;
    size_t live = 0, max_ops = 0;   // (a segment without operations takes no part: its counts stay zero)
    for (size_t s = 0; s < nseg; s++) {
        const size_t nops = j[s].nops;
        if (nops >= ((size_t)1 << 31)) throw std::runtime_error(std::string(j[s].what) + ": 2^31 or more arithmetic ops");
        if (nops && !j[s].d_ops) throw std::runtime_error(std::string(j[s].what) + ": null ops");
        // start[0, nops] the scan (start[nops] = rows, also counts()[0]); counts()[1] the failure flags (start[nops + 1] unless the caller
        // gave the two words a home, which it zeroes)
        j[s].start = zkm_scratch(c, (nops + 2) * 8);
        uint64_t* d_start = j[s].start.as<uint64_t>();
        ZKM_HIP_CHECK(hipMemsetAsync(d_start + nops, 0, 16, c->stream));
        if (!nops) continue;
        part.emplace_back(c, blocks_for(nops + 1, SCAN_TILE) * 8);
        cs[live] = count_seg{j[s].d_ops, d_start, (unsigned*)(j[s].counts() + 1), (uint32_t)nops};
        sc[live] = scan_seg{d_start, nops + 1, part.back().as<uint64_t>(), j[s].d_counts};
        max_ops = std::max(max_ops, nops);
        live++;
    }
    if (!live) return;
    zkm_prof_scope ps(c, "arithmetic_trace/count");
    zkm_launch_segs(c->stream, k_arith_count, cs, live, blocks_for(max_ops, AT_THREADS), AT_THREADS);
    scan_launch(c->stream, sc, live);
}

size_t zkm_arithmetic_height(zkm_arith_job& j, const uint64_t got[2], size_t* natural_rows_out) {
    const std::string w(j.what);
    const unsigned flags = (unsigned)got[1];
    if (flags & BAD_OP) throw std::runtime_error(w + ": an op code is above 25 (IS_MTLO)");
    if (flags & BAD_DIV_ZERO) throw std::runtime_error(w + ": DIV or DIVU by zero");
    if (flags & BAD_DIV_OVERFLOW) throw std::runtime_error(w + ": DIV of 0x80000000 by 0xFFFFFFFF overflows");
    if (flags & BAD_IMM) throw std::runtime_error(w + ": ADDI, ADDIU, SLTI or SLTIU with an input1 that is not a sign-extended 16-bit immediate");
    if (flags & BAD_SHIFT) throw std::runtime_error(w + ": SLL, SRL, SRA or SRAV with a shift amount above 31");
    j.rows = got[0];
    const size_t natural = std::max<size_t>(RANGE_MAX, next_pow2(j.rows));
    if (natural_rows_out) *natural_rows_out = natural;
    return natural;
}

void zkm_arithmetic_write(zkm_arith_job* j, size_t nseg, const unsigned* log_n, gl_t* const* out_dev, unsigned* const* d_bad) {
    zkm_ctx* c = j->c;
    rows_args ra[ZKM_MAX_SEG];
    freq_seg fs[ZKM_MAX_SEG];
    size_t grid = 0;
    for (size_t s = 0; s < nseg; s++) {
        const size_t n = (size_t)1 << log_n[s], nops = j[s].nops, rows = j[s].rows;
        // hist[0, 2^16) the RC_FREQUENCIES bins (hist[2^16]: zero, where the wrapper keeps its range-check flag)
        j[s].hist = zkm_scratch(c, (RANGE_MAX + 1) * 8);
        unsigned long long* d_hist = j[s].hist.as<unsigned long long>();
        ZKM_HIP_CHECK(hipMemsetAsync(d_hist, 0, (RANGE_MAX + 1) * 8, c->stream));
        ra[s] = rows_args{j[s].d_ops, j[s].start.as<uint64_t>(), (uint32_t)nops, rows, n, d_hist,
                          d_bad && d_bad[s] ? d_bad[s] : (unsigned*)(d_hist + RANGE_MAX), out_dev[s]};
        fs[s] = freq_seg{d_hist, (uint64_t)NSHARED * (n - rows), n, out_dev[s]};
        const size_t work = std::max<size_t>(nops, n - rows);
        grid = std::max(grid, std::min<size_t>(blocks_for(work, AR_THREADS), (size_t)std::max(c->num_cus, 1)));
    }
    {
        zkm_prof_scope ps(c, "arithmetic_trace/rows");
        zkm_launch_segs(c->stream, k_arith_rows, ra, nseg, grid, AR_THREADS);
    }
    {
        zkm_prof_scope ps(c, "arithmetic_trace/freq");
        zkm_launch_segs(c->stream, k_arith_freq, fs, nseg, RANGE_MAX / AT_THREADS, AT_THREADS);
    }
}

extern "C" int zkm_arithmetic_trace(zkm_ctx* c, const uint32_t* ops, size_t nops, unsigned log_n, uint64_t* out_dev,
                                    size_t* natural_rows_out, char** err) {
    return zkm_api("zkm_arithmetic_trace", c, err, [&] {
        if (nops >= ((size_t)1 << 31)) throw std::runtime_error("zkm_arithmetic_trace: 2^31 or more arithmetic ops");
        if (nops && !ops) throw std::runtime_error("zkm_arithmetic_trace: null ops");
        if (out_dev) {
            if (log_n < 16 || log_n > AT_MAX_LOG_N)
                throw std::runtime_error("zkm_arithmetic_trace: log_n " + std::to_string(log_n) + " outside [16, " +
                                         std::to_string(AT_MAX_LOG_N) + "] (the range-check table needs 2^16 rows)");
            if (!zkm_is_device_ptr(out_dev)) throw std::runtime_error("zkm_arithmetic_trace: out must be a device pointer");
        }
        zkm_scratch_list host_copy(c);
        const uint32_t* d_ops = ops;
        if (nops && !zkm_is_device_ptr(ops)) {
            d_ops = host_copy.alloc<uint32_t>(nops * 12);
            ZKM_HIP_CHECK(hipMemcpyAsync((void*)d_ops, ops, nops * 12, hipMemcpyHostToDevice, c->stream));
        }
        zkm_arith_job j(c, "zkm_arithmetic_trace", d_ops, nops);
        zkm_arithmetic_count(&j, 1);
        uint64_t got[2];
        c->download(got, j.counts(), 16);
        const size_t natural = zkm_arithmetic_height(j, got, natural_rows_out);
        if (!out_dev) return;
        const size_t n = (size_t)1 << log_n;
        if (natural > n)
            throw std::runtime_error("zkm_arithmetic_trace: the table needs " + std::to_string(natural) + " rows, more than 2^" + std::to_string(log_n));
        gl_t* const out = out_dev;
        zkm_arithmetic_write(&j, 1, &log_n, &out, nullptr);
        uint64_t bad = 0;
        c->download(&bad, j.hist.as<unsigned long long>() + RANGE_MAX, 8);
        if (bad) throw std::runtime_error("zkm_arithmetic_trace: a shared-column value is 2^16 or more");
    });
}
