// poseidon_dev.h -- Goldilocks Poseidon permutation (width 12, 4 + 22 + 4 rounds, x^7), device + host.
//
// Same function as the reference's in-tree permutation prover/src/poseidon/poseidon_stark.rs:51-95
// (constant_layer :164-169, sbox_monomial :239-251, mds_layer :310-345), which is also plonky2
// PoseidonHash's permutation (Merkle hasher, Challenger).  One permutation per lane: the 12-word state
// lives in 24 VGPRs, round constants are wave-uniform and come from the scalar (constant) cache.
// No MFMA: this is 64-bit modular integer work.
//
// Formulation.  On gfx950 a 32x32->64 multiply-add (v_mad_u64_u32) issues at nearly the rate of an add
// (profiles/r01_ubench_valu_rates.txt), so the cost of a round is its instruction count, and a full
// 64x64 modular multiply (4 mads + ~15 carry/reduction instructions) is ~25x the price of a multiply by
// a 6-bit MDS entry.  The reference's "fast partial round" form (sparse matrices with 64-bit entries,
// poseidon_stark.rs:463-487) therefore LOSES here: every partial round is done in the textbook form
// -- s-box on lane 0, dense circulant MDS with 6-bit entries -- and the next round's constants are
// folded into the MDS accumulators before the single reduction.  Algebraically identical, so outputs are
// bit-exact (pinned by the plonky2 test vectors and by naive == fast in the oracle).
//
// Partial rounds, fused.  Between two lane-0 s-boxes the state only goes through linear maps, and the integer powers of
// the MDS matrix stay small: the entries of M^3 are < 2^21 and its row sums < 2^25, so a row of M^3 applied to 32-bit
// halves still fits the same pair of 64-bit accumulators (24 multiply-adds) as a row of M.  With
// delta_k = sbox(a_k[0]) - a_k[0] the three rounds
//     a1 = M x + K1,   a2 = M (a1 + e0 delta1) + K2,   a3 = M (a2 + e0 delta2) + K3
// become  a1[0] = M[0,:] x + c1,   a2[0] = M^2[0,:] x + M[0,0] delta1 + c2,
//         a3 = M^3 x + M^2[:,0] delta1 + M[:,0] delta2 + c3          (c1, c2, c3 precomputed from the round constants)
// i.e. two single-row products and ONE dense product instead of three dense products (poseidon_partial_group_t<3>; tables:
// tools/gen_poseidon_constants.py derive_fused, which also asserts the no-overflow bound).
//
// Four rounds per dense product (poseidon_partial_group_t<4>, what the one-lane permutation runs).  What limits the depth is the
// 32-bit multiplier of a multiply-add, not the accumulator: the entries of M^4 are 29-bit numbers (357,057,728 .. 381,558,488), so a
// row of M^4 is still 24 multiply-adds with scalar multipliers; the entries of M^5 have 37 bits and are not.  The row sums of M^4 are
// 2^32 * 1.04, so a half-sum of a row can pass 2^64 -- by less than 2^60, and only in its LAST multiply-add (bounds (a)-(c) of
// poseidon_group4.inc, asserted by the generator and by static_assert there).  That multiply-add's carry-out is the instruction's
// own scalar result, and the row is folded by poseidon_fold_wide, which takes al, ah < 2^64 and the two carries.
//     a4 = M^4 x + M^3[:,0] delta1 + M^2[:,0] delta2 + M[:,0] delta3 + c4,   a3[0] = M^3[0,:] x + M^2[0,0] delta1 + M[0,0] delta2 + c3
// The 23 linear layers (round 3's MDS and the 22 partial rounds) are five four-round groups and one three-round group: 6 dense
// products and 17 single rows (tables: derive_group4).  Algebraically identical to the reference's rounds, so outputs are bit-exact.
//
// The state is kept "loose" (any uint64 representing its residue) between rounds and canonicalised once
// on exit -- see gl_dev.h for the overflow arguments of every loose primitive.
#pragma once
#include "gl_dev.h"

#undef ZKM_CONSTEXPR
#define ZKM_CONSTEXPR static constexpr
namespace pc_host {
#undef ZKM_CONST
#define ZKM_CONST static const
#include "poseidon_constants.inc"
#include "poseidon_group4.inc"
ZKM_CONST uint64_t ZKM_POSEIDON_ZERO12[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // "constants" after the last round
}  // namespace pc_host
#if defined(__HIPCC__)
namespace pc_dev {
#undef ZKM_CONST
#define ZKM_CONST static __device__ __constant__ const
#include "poseidon_constants.inc"
#include "poseidon_group4.inc"
ZKM_CONST uint64_t ZKM_POSEIDON_ZERO12[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
}  // namespace pc_dev
#endif
#undef ZKM_CONST
#undef ZKM_CONSTEXPR

#if defined(__HIP_DEVICE_COMPILE__)
#define PC pc_dev
#define POSEIDON_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
// region markers for tools/isa_histogram.py (comments in the assembly; no instructions): the permutation's control flow has parts
// that run 8, 5 and 1 times per permutation, which loop trip counts alone cannot express
#define POSEIDON_REGION(name) asm volatile("; ZKM_REGION " name)
#else
#define PC pc_host
#define POSEIDON_SCHED_FENCE() ((void)0)
#define POSEIDON_REGION(name) ((void)0)
#endif

// Hide a small multiplier from the optimiser (it stays in an SGPR).  Left to itself the compiler turns the MDS entries that are
// powers of two (2, 8, 16) into v_lshl_add_u64, which needs the 32-bit word zero-extended into a register pair first (a v_mov per
// term) and issues no faster than the v_mad_u64_u32 that takes the word directly.
#if defined(__HIP_DEVICE_COMPILE__)
#define POSEIDON_OPAQUE(c) asm("" : "+s"(c))
// A table pointer the optimiser cannot see through and cannot move: the constants behind it are (re)loaded with scalar loads where
// they are used.  Without it the loop-invariant ones (first-round constants, the last fused group's) are hoisted out of the sponge
// loop as ~100 SGPRs, spilled to VGPR lanes and read back with v_readlane -- 150 vector instructions per permutation for values the
// scalar cache delivers for free.
#define POSEIDON_OPAQUE_PTR(p) asm volatile("" : "+s"(p))
#else
#define POSEIDON_OPAQUE(c) ((void)0)
#define POSEIDON_OPAQUE_PTR(p) ((void)0)
#endif

// x^7 on a loose value -> loose
GL_HD uint64_t poseidon_sbox7(uint64_t x) {
    uint64_t x2 = gl_mul_loose(x, x);
    uint64_t x4 = gl_mul_loose(x2, x2);
    uint64_t x3 = gl_mul_loose(x, x2);
    return gl_mul_loose(x3, x4);
}

// al + 2^32 ah -> loose, for al, ah < 2^59.  No compares: the carries are produced as VALUES.
//   2^32 ah = 2^64 ah_hi + 2^32 ah_lo == EPS ah_hi + 2^32 ah_lo;   s1 = al + EPS ah_hi < 2^60 (one multiply-add);
//   hs = s1_hi + ah_lo is a 33-bit number whose top bit c again weighs 2^64 == EPS;  result = (hs_lo32 : s1_lo) + EPS c,
//   which cannot wrap (c = 1 implies hs_lo32 < 2^28).
// Additive constants are folded in by starting the accumulators at (const_lo, const_hi).
GL_HD uint64_t poseidon_fold(uint64_t al, uint64_t ah) {
#if defined(__HIP_DEVICE_COMPILE__)
    // t = al + EPS ah_hi < 2^60; adding 2^32 ah_lo only touches the high word, and its carry-out (an SGPR pair) selects the EPS
    // correction: multiply-add, add, select, add.  t < 2^60 means the corrected sum cannot wrap again.
    const uint64_t t = (uint64_t)(uint32_t)(ah >> 32) * 0xFFFFFFFFu + al;
    uint32_t rhi, wrap;
    uint64_t carry;
    asm("v_add_co_u32_e64 %0, %1, %3, %4\n\ts_nop 1\n\tv_cndmask_b32 %2, 0, -1, %1"
        : "=&v"(rhi), "=&s"(carry), "=v"(wrap)
        : "v"((uint32_t)(t >> 32)), "v"((uint32_t)ah));
    return (((uint64_t)rhi << 32) | (uint32_t)t) + wrap;
#endif
    uint64_t s1 = (uint64_t)(uint32_t)(ah >> 32) * 0xFFFFFFFFu + al;
    uint64_t hs = (uint64_t)(uint32_t)ah + (s1 >> 32);
    uint64_t base = (hs << 32) | (uint32_t)s1;
    return (uint64_t)(uint32_t)(hs >> 32) * 0xFFFFFFFFu + base;
}

// x * m + c (mod 2^64) with the multiplier in a scalar register, and the carry-out of the 64-bit add: the instruction's own scalar
// result, no compare.  Device: `carry` is the wave's lane mask (bit l = lane l carried); host: 0 or 1.
GL_HD uint64_t gl_mad_s_co(uint32_t x, uint32_t m, uint64_t c, uint64_t& carry) {
#if defined(__HIP_DEVICE_COMPILE__)
    uint64_t r;
    asm("v_mad_u64_u32 %0, %1, %2, %3, %4" : "=v"(r), "=s"(carry) : "v"(x), "s"(m), "v"(c));
    return r;
#else
    const uint64_t r = (uint64_t)x * m + c;
    carry = r < c;
    return r;
#endif
}

// (al + 2^64 cl) + 2^32 (ah + 2^64 ch) -> loose, for ANY al, ah < 2^64 and any carries cl, ch (device: lane masks, host: 0 / 1).
// The fold of an M^4 row, whose half-sums can pass 2^64 once.  2^64 == EPS and 2^96 == -1, so the value is
//     al + 2^32 ah_lo + EPS ah_hi  +  EPS cl - ch.
//   t  = al + EPS ah_hi <= (2^64 - 1) + (2^32 - 1)^2 < 2^65: one multiply-add whose carry-out w1 again weighs EPS.  If w1 = 1 the
//        wrapped t is <= 2^64 - 2^33, so t' = t + EPS w1 <= 2^64 - 2^32 - 1 does not wrap.
//   hs = t'_hi + ah_lo is a 33-bit number whose top bit w2 weighs 2^64 == EPS.  If w2 = 1 then hs_lo32 <= 2^32 - 2, so
//        r = (hs_lo32 : t'_lo) + EPS w2 <= 2^64 - 2 does not wrap.            r == al + 2^32 ah for every al, ah.
//   cl, ch: a half-sum carries about once in 10^8 rows of uniformly distributed words (its mean is 0.52 * 2^64, its deviation
//        0.09 * 2^64) and at the all-ones state on every row; the two corrections sit behind one wave-uniform branch on the masks.
//        r + EPS cl is loose + canonical (gl_add_lc: after a wrap the sum is < EPS, and EPS more cannot wrap); r - ch borrows only at
//        r = 0, where the result is p - 1.
//        Correct whether or not the branch is rare.
GL_HD uint64_t poseidon_fold_wide(uint64_t al, uint64_t ah, uint64_t cl, uint64_t ch) {
    uint64_t r;
#if defined(__HIP_DEVICE_COMPILE__)
    // (the carries travel in vcc from each instruction to the next: written out, so that no 64-bit add needs a zero-extended pair)
    uint64_t t;
    uint32_t e, rlo, rhi;
    asm("v_mad_u64_u32 %0, vcc, %2, -1, %3\n\tv_cndmask_b32 %1, 0, -1, vcc" : "=&v"(t), "=&v"(e) : "v"((uint32_t)(ah >> 32)), "v"(al) : "vcc");
    asm("v_add_co_u32 %0, vcc, %3, %2\n\t"            // t' = t + EPS w1
        "v_addc_co_u32 %1, vcc, 0, %4, vcc\n\t"
        "v_add_co_u32 %1, vcc, %1, %5\n\t"            // hs = t'_hi + ah_lo, w2 in vcc
        "v_cndmask_b32 %2, 0, -1, vcc\n\t"
        "v_add_co_u32 %0, vcc, %0, %2\n\t"            // r = (hs_lo32 : t'_lo) + EPS w2
        "v_addc_co_u32 %1, vcc, 0, %1, vcc"
        : "=&v"(rlo), "=&v"(rhi), "+&v"(e)
        : "v"((uint32_t)t), "v"((uint32_t)(t >> 32)), "v"((uint32_t)ah)
        : "vcc");
    r = ((uint64_t)rhi << 32) | rlo;
    if (__builtin_expect((cl | ch) != 0, 0)) {          // the wave's carry masks: a scalar branch
        asm volatile("; ZKM_COLD");
        const unsigned lane = __lane_id() & 63;
        if ((cl >> lane) & 1) r = gl_add_lc(r, GL_EPS);
        if ((ch >> lane) & 1) r = r ? r - 1 : GL_P - 1;
    }
#else
    const uint64_t p1 = (uint64_t)(uint32_t)(ah >> 32) * 0xFFFFFFFFu;
    uint64_t t = p1 + al;
    if (t < al) t += GL_EPS;
    const uint64_t hs = (t >> 32) + (uint32_t)ah;
    r = (hs << 32) | (uint32_t)t;
    if (hs >> 32) r += GL_EPS;
    if (cl) r = gl_add_lc(r, GL_EPS);
    if (ch) r = r ? r - 1 : GL_P - 1;
#endif
    return r;
}

// Circulant MDS (first row CIRC = {17,15,41,16,2,28,13,13,39,18,34,20}, plus 8 on the (0,0) entry):
//   out[r] = sum_i CIRC[i] * s[(i+r)%12] + [r==0] 8 s[0] + add[r]
// Each state word is split into 32-bit halves, the halves are accumulated in two 64-bit sums that start at the halves of
// the additive constant (next round's constant) and stay < 2^32 * 265 < 2^41, and the pair is folded once (poseidon_fold).
// Inputs loose, outputs loose.
template <bool ADD, int ROW0 = 0, int ROW1 = 12>
GL_HD void poseidon_mds_add(uint64_t s[12], const uint64_t* add) {
    uint32_t lo[12], hi[12];
#pragma unroll
    for (int i = 0; i < 12; i++) {
        lo[i] = (uint32_t)s[i];
        hi[i] = (uint32_t)(s[i] >> 32);
    }
    uint32_t C[12] = {17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20}, diag = 8;
#pragma unroll
    for (int i = 0; i < 12; i++) POSEIDON_OPAQUE(C[i]);
    POSEIDON_OPAQUE(diag);
#pragma unroll
    for (int r = ROW0; r < ROW1; r++) {   // (rows outside [ROW0, ROW1) keep their input word: callers treat them as dead)
        // ADD: the constant is the addend of the row's first multiply-add, whose multiplier C[0] = 17 is then an inline constant and not
        // the opaque SGPR (gl_mad_imm_sc: an instruction reads one scalar operand) -- no 64-bit add of its own per half-sum
        uint64_t al = ADD ? gl_mad_imm_sc<17>(lo[r], (uint64_t)(uint32_t)add[r]) : 0, ah = ADD ? gl_mad_imm_sc<17>(hi[r], add[r] >> 32) : 0;
#pragma unroll
        for (int i = ADD ? 1 : 0; i < 12; i++) {
            al += (uint64_t)lo[(i + r) % 12] * C[i];
            ah += (uint64_t)hi[(i + r) % 12] * C[i];
        }
        if (r == 0) {
            al += (uint64_t)lo[0] * diag;
            ah += (uint64_t)hi[0] * diag;
        }
        s[r] = poseidon_fold(al, ah);
        if ((r & 3) == 3) POSEIDON_SCHED_FENCE();
    }
}
GL_HD void poseidon_mds(uint64_t s[12]) { poseidon_mds_add<false>(s, nullptr); }

// sbox(a) - a mod p, loose -> loose
GL_HD uint64_t poseidon_sbox_delta(uint64_t a) { return gl_sub_rr(poseidon_sbox7(a), a); }
GL_HD constexpr uint32_t poseidon_m1(int i, int j) {
    constexpr uint32_t C[12] = {17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20};
    return C[(j - i + 12) % 12] + ((i == 0 && j == 0) ? 8u : 0u);
}

// Row 0 of M on the halves, from term J on: every multiplier is an inline constant, so every term is one multiply-add (gl_mad_imm)
template <int J>
GL_HD void poseidon_m_row0(const uint32_t lo[12], const uint32_t hi[12], uint64_t& al, uint64_t& ah) {
    if constexpr (J < 12) {
        al = gl_mad_imm<poseidon_m1(0, J)>(lo[J], al);
        ah = gl_mad_imm<poseidon_m1(0, J)>(hi[J], ah);
        poseidon_m_row0<J + 1>(lo, hi, al, ah);
    }
}
// Rows I .. 11 of the dense layer that closes a fused group (M^3 for T = 3, M^2 for T = 2).  The constant c3[i] opens both half-sums as
// the addend of the term with the inline multiplier M[i][0] (<= 41): d2 M[i][0] for T = 3, d1 M[i][0] for T = 2.
template <int T, int I>
GL_HD void poseidon_group_rows(uint64_t s[12], const uint32_t lo[12], const uint32_t hi[12], uint32_t d1l, uint32_t d1h, uint32_t d2l, uint32_t d2h,
                               const uint64_t* c3) {
    if constexpr (I < 12) {
        uint64_t al, ah;
        if (T == 3) {
            al = gl_mad_s(d1l, PC::ZKM_POSEIDON_M2[I][0], gl_mad_imm_sc<poseidon_m1(I, 0)>(d2l, (uint64_t)(uint32_t)c3[I]));
            ah = gl_mad_s(d1h, PC::ZKM_POSEIDON_M2[I][0], gl_mad_imm_sc<poseidon_m1(I, 0)>(d2h, c3[I] >> 32));
#pragma unroll
            for (int j = 0; j < 12; j++) {
                al = gl_mad_s(lo[j], PC::ZKM_POSEIDON_M3[I][j], al);
                ah = gl_mad_s(hi[j], PC::ZKM_POSEIDON_M3[I][j], ah);
            }
        } else {
            al = gl_mad_imm_sc<poseidon_m1(I, 0)>(d1l, (uint64_t)(uint32_t)c3[I]);
            ah = gl_mad_imm_sc<poseidon_m1(I, 0)>(d1h, c3[I] >> 32);
#pragma unroll
            for (int j = 0; j < 12; j++) {
                al = gl_mad_s(lo[j], PC::ZKM_POSEIDON_M2[I][j], al);
                ah = gl_mad_s(hi[j], PC::ZKM_POSEIDON_M2[I][j], ah);
            }
        }
        s[I] = poseidon_fold(al, ah);
        if ((I & 1) == 1) POSEIDON_SCHED_FENCE();
        poseidon_group_rows<T, I + 1>(s, lo, hi, d1l, d1h, d2l, d2h, c3);
    }
}

// Rows I .. 11 of the M^4 layer that closes a four-round group.  The constant c4[i] opens both half-sums as the addend of the term with
// the inline multiplier M[i][0] (delta3's); each half-sum ends on the M^4 term of column 11, whose carry-out goes to the fold: every
// partial sum before it is exact (bound (b) of poseidon_group4.inc) and the complete sum carries at most once (bound (c)).
template <int I>
GL_HD void poseidon_group4_rows(uint64_t s[12], const uint32_t lo[12], const uint32_t hi[12], uint32_t d1l, uint32_t d1h, uint32_t d2l, uint32_t d2h,
                                uint32_t d3l, uint32_t d3h, const uint64_t* c4) {
    if constexpr (I < 12) {
        static_assert(PC::ZKM_POSEIDON_G4_DCOL[0][I] == poseidon_m1(I, 0) && PC::ZKM_POSEIDON_G4_DCOL[1][I] == PC::ZKM_POSEIDON_M2[I][0] &&
                      PC::ZKM_POSEIDON_G4_DCOL[2][I] == PC::ZKM_POSEIDON_M3[I][0], "first columns of M, M^2, M^3");
        uint64_t al = gl_mad_imm_sc<poseidon_m1(I, 0)>(d3l, (uint64_t)(uint32_t)c4[I]), ah = gl_mad_imm_sc<poseidon_m1(I, 0)>(d3h, c4[I] >> 32);
        al = gl_mad_s(d2l, PC::ZKM_POSEIDON_G4_DCOL[1][I], al);
        ah = gl_mad_s(d2h, PC::ZKM_POSEIDON_G4_DCOL[1][I], ah);
        al = gl_mad_s(d1l, PC::ZKM_POSEIDON_G4_DCOL[2][I], al);
        ah = gl_mad_s(d1h, PC::ZKM_POSEIDON_G4_DCOL[2][I], ah);
#pragma unroll
        for (int j = 0; j < 11; j++) {
            al = gl_mad_s(lo[j], PC::ZKM_POSEIDON_M4[I][j], al);
            ah = gl_mad_s(hi[j], PC::ZKM_POSEIDON_M4[I][j], ah);
        }
        uint64_t cl, ch;
        al = gl_mad_s_co(lo[11], PC::ZKM_POSEIDON_M4[I][11], al, cl);
        ah = gl_mad_s_co(hi[11], PC::ZKM_POSEIDON_M4[I][11], ah, ch);
        s[I] = poseidon_fold_wide(al, ah, cl, ch);
        if ((I & 1) == 1) POSEIDON_SCHED_FENCE();
        poseidon_group4_rows<I + 1>(s, lo, hi, d1l, d1h, d2l, d2h, d3l, d3h, c4);
    }
}

// T linear layers (T = 4, 3 or 2) with the T - 1 lane-0 s-boxes between them; c3 = constants after the last layer (T = 4: of word 0
// after the third layer, with c4 = constants after the last).
// delta(k, a) = what lane 0 gains at s-box k = 0, 1 (T = 4: and 2) of the group on its input a: sbox(a) - a in the permutation; the constraint
// evaluator (constraints_dev.h) takes the s-box output from a witness cell instead.
// c1, c2, c3[] are wave-uniform on the device: their halves are the scalar addends of each sum's first multiply-add (gl_mad_imm_sc).
// ROW0_ASM: the first single row (M, inline multipliers) written out term by term (poseidon_m_row0).  The sponge kernels want it: left to
// the compiler the row's shifts and shared multipliers need zero-extended register pairs, and with those gone it keeps ONE zeroed
// scratch pair for the whole kernel.  The constraint evaluator does not: k_quotient<POSEIDON, 1> needs 93 registers with it, 69 without.
template <int T, bool ROW0_ASM = true, class DELTA>
GL_HD void poseidon_partial_group_t(uint64_t s[12], uint64_t c1, uint64_t c2, const uint64_t* c3, DELTA&& delta, const uint64_t* c4 = nullptr) {
    static_assert(T == 2 || T == 3 || T == 4, "groups of two, three or four layers");
    uint32_t lo[12], hi[12];
#pragma unroll
    for (int i = 0; i < 12; i++) {
        lo[i] = (uint32_t)s[i];
        hi[i] = (uint32_t)(s[i] >> 32);
    }
    uint64_t al = gl_mad_imm_sc<poseidon_m1(0, 0)>(lo[0], (uint64_t)(uint32_t)c1), ah = gl_mad_imm_sc<poseidon_m1(0, 0)>(hi[0], c1 >> 32);
    if constexpr (ROW0_ASM) {
        poseidon_m_row0<1>(lo, hi, al, ah);
    } else {
#pragma unroll
        for (int j = 1; j < 12; j++) {
            al += (uint64_t)lo[j] * poseidon_m1(0, j);
            ah += (uint64_t)hi[j] * poseidon_m1(0, j);
        }
    }
    const uint64_t d1 = delta(0, poseidon_fold(al, ah));
    const uint32_t d1l = (uint32_t)d1, d1h = (uint32_t)(d1 >> 32);
    uint32_t d2l = 0, d2h = 0;
    POSEIDON_SCHED_FENCE();
    if (T >= 3) {
        al = gl_mad_imm_sc<poseidon_m1(0, 0)>(d1l, (uint64_t)(uint32_t)c2);
        ah = gl_mad_imm_sc<poseidon_m1(0, 0)>(d1h, c2 >> 32);
#pragma unroll
        for (int j = 0; j < 12; j++) {
            al = gl_mad_s(lo[j], PC::ZKM_POSEIDON_M2[0][j], al);
            ah = gl_mad_s(hi[j], PC::ZKM_POSEIDON_M2[0][j], ah);
        }
        const uint64_t d2 = delta(1, poseidon_fold(al, ah));
        d2l = (uint32_t)d2;
        d2h = (uint32_t)(d2 >> 32);
        POSEIDON_SCHED_FENCE();
    }
    if constexpr (T == 4) {
        // word 0 after the third layer: row 0 of the three-round group's dense layer, c3[0] its constant
        al = gl_mad_s(d1l, PC::ZKM_POSEIDON_M2[0][0], gl_mad_imm_sc<poseidon_m1(0, 0)>(d2l, (uint64_t)(uint32_t)c3[0]));
        ah = gl_mad_s(d1h, PC::ZKM_POSEIDON_M2[0][0], gl_mad_imm_sc<poseidon_m1(0, 0)>(d2h, c3[0] >> 32));
#pragma unroll
        for (int j = 0; j < 12; j++) {
            al = gl_mad_s(lo[j], PC::ZKM_POSEIDON_M3[0][j], al);
            ah = gl_mad_s(hi[j], PC::ZKM_POSEIDON_M3[0][j], ah);
        }
        const uint64_t d3 = delta(2, poseidon_fold(al, ah));
        POSEIDON_SCHED_FENCE();
        poseidon_group4_rows<0>(s, lo, hi, d1l, d1h, d2l, d2h, (uint32_t)d3, (uint32_t)(d3 >> 32), c4);
    } else {
        poseidon_group_rows<T, 0>(s, lo, hi, d1l, d1h, d2l, d2h, c3);
    }
}
// one four-round group: c3 = &(constant of word 0 after the third layer), c4 = constants after the fourth
GL_HD void poseidon_partial_group4(uint64_t s[12], uint64_t c1, uint64_t c2, const uint64_t* c3, const uint64_t* c4) {
    poseidon_partial_group_t<4>(s, c1, c2, c3, [](int, uint64_t a) { return poseidon_sbox_delta(a); }, c4);
}
template <int T>
GL_HD void poseidon_partial_group(uint64_t s[12], uint64_t c1, uint64_t c2, const uint64_t* c3) {
    poseidon_partial_group_t<T>(s, c1, c2, c3, [](int, uint64_t a) { return poseidon_sbox_delta(a); });
}

// One loop over the eight full rounds with the partial-round section hanging off round 3: every piece of round code exists
// once, so the hot loop of the leaf kernel (33 absorb steps per row) is ~30 KB of instructions instead of ~57 KB (the second
// block of full rounds, two inline s-box layers and the last MDS used to be separate copies) and stays inside the 64 KB
// instruction cache two CUs share.
//
// What the caller reads of the result.  A sponge in overwrite mode (plonky2 hash_n_to_m_no_pad: the next input chunk REPLACES the rate
// words) only carries the four capacity words from one permutation to the next, and a digest is the first four words: the last MDS
// layer then needs 4 of its 12 rows (8 x (24 multiply-adds + fold) less) and only what leaves the sponge is canonicalised.
//   ALL: twelve canonical words.   CAPACITY: words 8..11, loose (they go straight into the next permutation); words 0..7 are garbage.
//   DIGEST: words 0..3, canonical; words 4..11 are garbage.
enum { POSEIDON_OUT_ALL = 0, POSEIDON_OUT_CAPACITY = 1, POSEIDON_OUT_DIGEST = 2 };

// The MDS layer of a full round: s <- M s + constants of round `next` (30 = none).  poseidon_mfma_dev.h has the matrix-core form.
struct poseidon_mds_valu {
    GL_HD void layer(uint64_t s[12], int next) const {
        poseidon_mds_add<true>(s, next < 30 ? &PC::ZKM_POSEIDON_RC[next * 12] : PC::ZKM_POSEIDON_ZERO12);
    }
};

// In: any uint64 words (loose).  `out` must be wave-uniform on the device (it selects code, not lanes).
template <class MDS>
GL_HD void poseidon_permute_out_t(uint64_t s[12], int out, const MDS& mds) {
    POSEIDON_REGION("entry");
    const uint64_t* rc0 = PC::ZKM_POSEIDON_RC;
    POSEIDON_OPAQUE_PTR(rc0);
#pragma unroll
    for (int i = 0; i < 12; i++) s[i] = gl_add_lc(s[i], rc0[i]);   // loose + CANONICAL round constant (tests/test_oracle_primitives.py
                                                                   // checks every table entry < p): one correction, not two (gl_dev.h)
#pragma unroll 1
    for (int r = 0; r < 8; r++) {
        POSEIDON_REGION("full_sbox");
#pragma unroll
        for (int i = 0; i < 12; i++) {
            s[i] = poseidon_sbox7(s[i]);
            if ((i & 1) == 1) POSEIDON_SCHED_FENCE();
        }
        if (r == 3) {
            POSEIDON_REGION("partial_head");
            // round 3's MDS opens the first fused group; the groups cover the MDS of rounds 3 .. 25 and the s-boxes of rounds 4 .. 25
#pragma unroll 1
            for (int g = 0; g < 5; g++) {  // MDS of rounds 4g+3 .. 4g+6 and the s-boxes of rounds 4g+4 .. 4g+6; then round 4g+7's
                POSEIDON_REGION("partial_group4");
                poseidon_partial_group4(s, PC::ZKM_POSEIDON_G4_C1[g], PC::ZKM_POSEIDON_G4_C2[g], &PC::ZKM_POSEIDON_G4_C3[g], PC::ZKM_POSEIDON_G4_C4[g]);
                s[0] = poseidon_sbox7(s[0]);
            }
            POSEIDON_REGION("partial_tail");
            const uint64_t* tc12 = PC::ZKM_POSEIDON_G4_TAIL_C12;
            const uint64_t* tc3 = PC::ZKM_POSEIDON_G4_TAIL_C3;
            POSEIDON_OPAQUE_PTR(tc12);
            POSEIDON_OPAQUE_PTR(tc3);
            poseidon_partial_group<3>(s, tc12[0], tc12[1], tc3);  // MDS of rounds 23, 24, 25 and the s-boxes of rounds 24, 25
        } else if (r == 7 && out != POSEIDON_OUT_ALL) {
            POSEIDON_REGION("last_mds_rows");
            if (out == POSEIDON_OUT_CAPACITY) poseidon_mds_add<false, 8, 12>(s, nullptr);
            else poseidon_mds_add<false, 0, 4>(s, nullptr);
        } else {
            POSEIDON_REGION("full_mds");
            // full round r < 3 is round r, r > 3 is round 22 + r; the constants added are those of the NEXT round (none after the last)
            const int next = (r < 3 ? r : 22 + r) + 1;
            mds.layer(s, next);
        }
    }
    POSEIDON_REGION("exit");
    if (out == POSEIDON_OUT_ALL) {
#pragma unroll
        for (int i = 0; i < 12; i++) s[i] = gl_canon(s[i]);
    } else if (out == POSEIDON_OUT_DIGEST) {
#pragma unroll
        for (int i = 0; i < 4; i++) s[i] = gl_canon(s[i]);
    }
}

GL_HD void poseidon_permute_out(uint64_t s[12], int out) { poseidon_permute_out_t(s, out, poseidon_mds_valu{}); }

// In: any uint64 words (loose).  Out: canonical.
GL_HD void poseidon_permute(uint64_t s[12]) { poseidon_permute_out(s, POSEIDON_OUT_ALL); }
