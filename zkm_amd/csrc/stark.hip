// stark.hip -- prove_single_table on the GPU: quotient (K7-K9), openings (K10), FRI (K11-K14), queries.
//
// Host orchestration restates the reference's prover/src/prover.rs:441-641 (stage and transcript order) as stages over one state, the
// table_proof (a proof_stack: the transcripts, blobs and scratch of a stack of proofs in flight): commit_trace -> commit_aux ->
// commit_quotient (alphas, quotient_device) -> draw_zeta, write_openings -> prove_openings (FRI alpha, combination, then fri_finish:
// composites to natural order, divide_accumulate_all, fri_commit_phase, fri_proof_of_work, fri_query_rounds).  Three drivers enter
// that line: from values (zkm_prove_single_table[_ctl]), from the trace and auxiliary commitments (zkm_prove_table_from_commitments:
// zkm_prove_single_tables, ctl.hip) and from all three commitments (zkm_prove_openings).
// The kernels replace the rayon loops of compute_quotient_polys (:700-782), StarkOpeningSet::new
// (proof.rs:299-334) and plonky2's PolynomialBatch::prove_openings / fri_proof.
// The Challenger stays on the host (a few hundred field elements per table); only caps, openings,
// the final polynomial and the query openings cross PCIe.
#define GL_REDUCE_BRANCHFREE 1   // (gl_dev.h: these kernels interleave independent products at low occupancy)
#include "constraints_dev.h"
#include "ctl_dev.h"

// ------------------------------------------------------------------ proof blob: its description for a configuration (proof_blob.h)
// FriReductionStrategy::ConstantArityBits(arity_bits, final_poly_bits) (config.rs:25)
static unsigned fri_num_layers(const zkm_stark_config* c, unsigned degree_bits) {
    unsigned l = 0, d = degree_bits;
    // (d >= arity_bits keeps the subtraction from wrapping when final_poly_bits < arity_bits)
    while (d > c->final_poly_bits && d >= c->arity_bits && d + c->rate_bits - c->arity_bits >= c->cap_height) { d -= c->arity_bits; l++; }
    return l;
}

// Every field of the caller's config is checked once, here, before any allocation or transcript mutation (zkm_blob_describe is the
// first thing every prove entry point and zkm_proof_words call).  The quotient kernels carry at most two alpha accumulators
// (StarkConfig::num_challenges = 2 in standard_fast_config, config.rs:17-30).
// fri_only: the FRI-only entry points (zkm_fri_prove, zkm_fri_verify) also take rate_bits = 3, the rate of plonky2's
// standard_recursion_config: nothing behind them -- commitments, LDEs, folding, query rounds -- is tied to the quotient domain's rate.
static void validate_config(const zkm_stark_config* c, unsigned log_n, bool fri_only = false) {
    if (!c) throw std::runtime_error("stark config: null");
    if (log_n == 0 || log_n > 32) throw std::runtime_error("stark config: degree_bits out of range");
    if (fri_only && c->rate_bits != 2 && c->rate_bits != 3) throw std::runtime_error("stark config: rate_bits must be 2 or 3 for a FRI proof of its own");
    if (!fri_only && c->rate_bits != 2) throw std::runtime_error("stark config: only rate_bits = 2 is supported");
    if (c->arity_bits < 2 || c->arity_bits > 6) throw std::runtime_error("stark config: arity_bits must be in 2..6");
    if (c->pow_bits == 0 || c->pow_bits > 32) throw std::runtime_error("stark config: proof_of_work_bits must be in 1..32");
    if (c->num_challenges < 1 || c->num_challenges > 2) throw std::runtime_error("stark config: num_challenges must be 1 or 2");
    if (c->num_queries == 0 || c->num_queries > 4096) throw std::runtime_error("stark config: num_query_rounds must be in 1..4096");
    if (c->cap_height > log_n + c->rate_bits) throw std::runtime_error("stark config: cap_height exceeds the height of the Merkle tree");
    if (c->final_poly_bits > 32) throw std::runtime_error("stark config: final_poly_bits out of range");
}

zkm_blob_desc zkm_blob_describe(const zkm_stark_config* c, unsigned log_n, size_t W, size_t A, size_t Z) {
    validate_config(c, log_n);
    const unsigned L = fri_num_layers(c, log_n);
    return zkm_blob_desc{log_n, W, A, (size_t)c->num_challenges * 2, Z, c->cap_height, L, (size_t)1 << (log_n - L * c->arity_bits), c->num_queries,
                         c->rate_bits, c->arity_bits};
}

// ------------------------------------------------------------------ K7: quotient evaluation
// Table constraints live in constraints_dev.h; constraint order = alpha-power order (constraint_consumer.rs:57-62): table
// constraints, then the table's lookups, then the CTL checks (vanishing_poly.rs:17-46).
// CTL checks driven by the column-set description (eval_helper_columns cross_table_lookup.rs:1006-1058,
// eval_cross_table_lookup_checks :1067-1150).  The benchmark's fake CTL data (helper columns, no column sets)
// is the ncolsets == 0 case: only the last-row / transition checks on Z are emitted.
// Constraints of CtlZData `i`: helper-column checks q0 <= q < q1, then (if `closing`) the last-row / transition checks on Z.
// `start` = index of the z's first helper column among the auxiliary columns.
template <int NA>
__device__ void eval_ctl_z(const ctl_dev& d, uint32_t i, uint32_t start, uint32_t q0, uint32_t q1, bool closing, const gl_t* __restrict__ tl,
                           size_t N, ptrdiff_t dnext, const gl_t* __restrict__ aux, size_t j, size_t jn, consumer_t<NA>& k) {
    const zkm_ctl_z z = d.zs[i];
    const uint32_t* ids = d.colset_ids + z.colset_off;
    if (z.num_helpers) {
        for (uint32_t q = q0; q < q1; q++) {
            gl_t h = aux[(size_t)(start + q) * N + j];
            const zkm_colset c0 = d.colsets[ids[2 * q]];
            gl_t combin0 = ctl_combine(d, c0, z.beta, z.gamma, tl, N, dnext, true), f0 = ctl_eval_filter(d, c0, tl, N, dnext, true);
            if (2 * q + 1 < z.ncolsets) {
                const zkm_colset c1 = d.colsets[ids[2 * q + 1]];
                gl_t combin1 = ctl_combine(d, c1, z.beta, z.gamma, tl, N, dnext, true), f1 = ctl_eval_filter(d, c1, tl, N, dnext, true);
                k.constraint(gl_sub(gl_sub(gl_mul(gl_mul(combin1, combin0), h), gl_mul(f0, combin1)), gl_mul(f1, combin0)));
            } else {
                k.constraint(gl_sub(gl_mul(combin0, h), f0));
            }
        }
    }
    if (!closing) return;
    gl_t local_z = aux[(size_t)(d.total_helpers + i) * N + j], next_z = aux[(size_t)(d.total_helpers + i) * N + jn];
    if (z.num_helpers) {
        gl_t h_sum = 0;
        for (uint32_t q = 0; q < z.num_helpers; q++) h_sum = gl_add(h_sum, aux[(size_t)(start + q) * N + j]);
        k.last_row(gl_sub(local_z, h_sum));
        k.transition(gl_sub(gl_sub(local_z, next_z), h_sum));
    } else if (z.ncolsets > 1) {
        const zkm_colset c0 = d.colsets[ids[0]], c1 = d.colsets[ids[1]];
        gl_t combin0 = ctl_combine(d, c0, z.beta, z.gamma, tl, N, dnext, true), combin1 = ctl_combine(d, c1, z.beta, z.gamma, tl, N, dnext, true);
        gl_t f0 = ctl_eval_filter(d, c0, tl, N, dnext, true), f1 = ctl_eval_filter(d, c1, tl, N, dnext, true);
        gl_t cc = gl_mul(combin0, combin1), rhs = gl_add(gl_mul(f0, combin1), gl_mul(f1, combin0));
        k.last_row(gl_sub(gl_mul(cc, local_z), rhs));
        k.transition(gl_sub(gl_mul(cc, gl_sub(local_z, next_z)), rhs));
    } else {
        const zkm_colset c0 = d.colsets[ids[0]];
        gl_t combin0 = ctl_combine(d, c0, z.beta, z.gamma, tl, N, dnext, true), f0 = ctl_eval_filter(d, c0, tl, N, dnext, true);
        k.last_row(gl_sub(gl_mul(combin0, local_z), f0));
        k.transition(gl_sub(gl_mul(combin0, gl_sub(local_z, next_z)), f0));
    }
}
template <int NA>
__device__ void eval_ctl_constraints(const ctl_dev& d, const gl_t* __restrict__ tl, size_t N, ptrdiff_t dnext,
                                     const gl_t* __restrict__ aux, size_t j, size_t jn, consumer_t<NA>& k) {
    uint32_t start = 0;
    for (uint32_t i = 0; i < d.nzs; i++) {
        const zkm_ctl_z z = d.zs[i];
        eval_ctl_z<NA>(d, i, start, 0, z.num_helpers ? (z.ncolsets + 1) / 2 : 0, true, tl, N, dnext, aux, j, jn, k);
        start += z.num_helpers;
    }
}

// One thread per point of the quotient domain g<w_2n>, visited in LDE storage order: storage row j < 2n
// of the 4n-row LDE is natural quotient index i = bitrev_{L-1}(j) (every `step` = 2nd natural LDE row,
// prover.rs:668-675); "next" is natural +2 in the 2n domain (prover.rs:704) = +4 in the 4n domain.
// Per-point setup shared by the quotient kernels.
struct quotient_point {
    size_t j, jn;
    uint32_t i;
};
// the (<= 2) constraint challenges of every segment of a stack travel in the kernel-argument segment (seg_gl2: v[2 s + a]): no device
// copy, no upload per table.  Every quotient kernel takes its segment from blockIdx.z: the segment's columns start W N (trace) / A N
// (auxiliary) words after the previous segment's, its outputs NA * size words.
typedef seg_gl2 alpha_args;
// check mode (zkm_check_constraints == check_constraints, prover.rs:793-910, rate_bits = 0): the "LDE" is the trace itself, N = n rows in
// natural order, point j = w_n^j (wpow: the table of w_n), next row j + 1 mod n, and the Lagrange selectors are the indicator values
// of rows 0 and n - 1 -- signalled by gn == 0 (g^n is never 0 on the coset).
template <int NA>
__device__ __forceinline__ quotient_point quotient_setup(size_t j, unsigned lde_bits, const gl_t* __restrict__ alphas, const gl_t* __restrict__ wpow,
                                                         gl_t gn, gl_t last, gl_t w_n, gl_t n_inv, consumer_t<NA>& k) {
    const size_t N = (size_t)1 << lde_bits;
    if (gn == 0) {
        const unsigned h = (lde_bits + 1) / 2;
        const gl_t x = gl_mul_loose(wpow[j & ((1u << h) - 1)], wpow[((size_t)1 << h) + (j >> h)]);
#pragma unroll
        for (int a = 0; a < NA; a++) { k.set_alpha(a, alphas[a]); k.acc[a] = 0; }
        k.z_last = gl_sub(x, last);
        k.l_first = j == 0 ? 1 : 0;
        k.l_last = j == N - 1 ? 1 : 0;
        return quotient_point{j, (j + 1) & (N - 1), (uint32_t)j};
    }
    uint32_t t = bitrev32((uint32_t)j, lde_bits);  // natural index in the 4n domain (even)
    uint32_t i = t >> 1;                           // natural index in the 2n quotient domain
    uint32_t tn = (t + 4) & (uint32_t)(N - 1);
    // x = g * w_{4n}^t
    unsigned h = (lde_bits + 1) / 2;
    gl_t x = gl_mul(GL_GENERATOR, gl_mul_loose(wpow[t & ((1u << h) - 1)], wpow[((size_t)1 << h) + (t >> h)]));
#pragma unroll
    for (int a = 0; a < NA; a++) { k.set_alpha(a, alphas[a]); k.acc[a] = 0; }
    k.z_last = gl_sub(x, last);
    // Z_H(x) = x^n - 1 = g^n (-1)^i - 1;  L_first = Z_H / (n (x - 1)),  L_last = Z_H / (n (w x - 1))
    gl_t zh = gl_sub((i & 1) ? gl_neg(gn) : gn, 1);
    gl_t d0 = gl_sub(x, 1), d1 = gl_sub(gl_mul(w_n, x), 1);
    gl_t dinv = gl_inv(gl_mul(d0, d1));
    gl_t zn = gl_mul(zh, n_inv);
    k.l_first = gl_mul(zn, gl_mul(dinv, d1));
    k.l_last = gl_mul(zn, gl_mul(dinv, d0));
    return quotient_point{j, (size_t)bitrev32(tn, lde_bits), i};
}

// The vanishing polynomial is accumulated by separate launches (vanishing_poly.rs:30-45 order: table constraints, the table's
// lookups, then the cross-table lookup checks): k_quotient<TABLE> stores the running accumulators after the table's own
// constraints; the table-independent CTL kernels continue the same Horner recurrence acc = acc * alpha + c through the CTL checks
// and multiply by Z_H^-1.  The descriptor interpreter stays out of the per-table kernels' register budgets, and a table with few
// rows and hundreds of looking column sets (KeccakSponge) can spread its CTL checks over many workgroups:
//   k_quotient_ctl          all CTL constraints of a point in one thread (large tables: already enough parallelism)
//   k_quotient_ctl_chunk    blockIdx.y = a chunk of consecutive constraints [k_begin, k_end); Horner from 0 within the chunk,
//                           scaled by alpha^(K - k_end) (K = number of CTL constraints) into tmp[chunk]
//   k_quotient_ctl_sum      acc * alpha^K + sum of the chunks, times Z_H^-1
// -- the same polynomial in alpha, so the values are identical.
template <int TABLE, int NA>
__global__ __launch_bounds__(256, (TABLE == ZKM_TABLE_CPU || TABLE == ZKM_TABLE_POSEIDON || TABLE == ZKM_TABLE_ARITHMETIC ? 4 : 1)) void k_quotient(const gl_t* __restrict__ trace, const gl_t* __restrict__ aux,
                                                           unsigned log_n, unsigned lde_bits, lookup_dev lookups, alpha_args alphas_v,
                                                           seg_gl2 lookup_ch,
                                                           const gl_t* __restrict__ wpow /* w_{4n}^t two-level table */,
                                                           gl_t gn, gl_t last, gl_t w_n, gl_t n_inv, gl_t* __restrict__ out, size_t trace_seg,
                                                           size_t aux_seg) {
    const gl_t* const alphas = alphas_v.v + 2 * blockIdx.z;
    size_t N = (size_t)1 << lde_bits;
    size_t size = gn == 0 ? N : N >> 1;       // (check mode: every row of the trace)
    size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= size) return;
    trace += (size_t)blockIdx.z * trace_seg;
    aux += (size_t)blockIdx.z * aux_seg;
    out += (size_t)blockIdx.z * NA * size;
    consumer_t<NA> k;
    const quotient_point q = quotient_setup<NA>(j, lde_bits, alphas, wpow, gn, last, w_n, n_inv, k);
    eval_table_constraints<TABLE, NA>(trace + j, N, (ptrdiff_t)q.jn - (ptrdiff_t)j, k);
    // auxiliary columns: the table's lookup helper columns first, then the CTL helper columns and Zs (prover.rs:495-508)
    if constexpr (TABLE == ZKM_TABLE_MEMORY || TABLE == ZKM_TABLE_ARITHMETIC)
        eval_lookup_constraints<NA>(lookups, lookup_ch.v + 2 * blockIdx.z, trace + j, N, aux, j, q.jn, k);
#pragma unroll
    for (int a = 0; a < NA; a++) out[(size_t)a * size + q.i] = k.value(a);
}

// Short Keccak tables: KECCAK_CONSTRAINT_PARTS threads per point (constraints_dev.h, eval_keccak_constraints_part); blockIdx.y = part.
template <int NA>
__global__ __launch_bounds__(256) void k_quotient_keccak_parts(const gl_t* __restrict__ trace, unsigned lde_bits, alpha_args alphas_v,
                                                               const gl_t* __restrict__ wpow, gl_t gn, gl_t last, gl_t w_n, gl_t n_inv,
                                                               const gl_t* __restrict__ apw /* [segment][NA][K + 1] */,
                                                               gl_t* __restrict__ tmp /* [segment][part][NA][size] */, size_t trace_seg) {
    const gl_t* const alphas = alphas_v.v + 2 * blockIdx.z;
    size_t N = (size_t)1 << lde_bits;
    size_t size = N >> 1;
    size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= size) return;
    trace += (size_t)blockIdx.z * trace_seg;
    apw += (size_t)blockIdx.z * NA * (KECCAK_NUM_CONSTRAINTS + 1);
    tmp += (size_t)blockIdx.z * gridDim.y * NA * size;
    consumer_t<NA> k;
    const quotient_point q = quotient_setup<NA>(j, lde_bits, alphas, wpow, gn, last, w_n, n_inv, k);
    eval_keccak_constraints_part<NA>(trace + j, N, (ptrdiff_t)q.jn - (ptrdiff_t)j, k, (int)blockIdx.y, apw);
#pragma unroll
    for (int a = 0; a < NA; a++) tmp[((size_t)blockIdx.y * NA + a) * size + q.i] = k.value(a);
}
__global__ __launch_bounds__(256) void k_sum_parts(const gl_t* __restrict__ tmp, unsigned nparts, size_t words, gl_t* __restrict__ out) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= words) return;
    tmp += (size_t)blockIdx.z * nparts * words;
    out += (size_t)blockIdx.z * words;
    gl_t acc = 0;
    for (unsigned p = 0; p < nparts; p++) acc = gl_add(acc, tmp[(size_t)p * words + i]);
    out[i] = acc;
}

template <int NA>
__global__ __launch_bounds__(256) void k_quotient_ctl(const gl_t* __restrict__ trace, const gl_t* __restrict__ aux, unsigned lde_bits, ctl_dev ctl,
                                                      uint32_t num_lookup_cols, alpha_args alphas_v, const gl_t* __restrict__ wpow, gl_t gn,
                                                      gl_t zh_inv0, gl_t zh_inv1, gl_t last, gl_t w_n, gl_t n_inv, gl_t* __restrict__ out,
                                                      size_t trace_seg, size_t aux_seg) {
    const gl_t* const alphas = alphas_v.v + 2 * blockIdx.z;
    size_t N = (size_t)1 << lde_bits;
    size_t size = gn == 0 ? N : N >> 1;
    size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= size) return;
    trace += (size_t)blockIdx.z * trace_seg;
    aux += (size_t)blockIdx.z * aux_seg;
    out += (size_t)blockIdx.z * NA * size;
    ctl.zs += (size_t)blockIdx.z * ctl.nzs;
    consumer_t<NA> k;
    const quotient_point q = quotient_setup<NA>(j, lde_bits, alphas, wpow, gn, last, w_n, n_inv, k);
#pragma unroll
    for (int a = 0; a < NA; a++) k.acc[a] = out[(size_t)a * size + q.i];
    eval_ctl_constraints<NA>(ctl, trace + j, N, (ptrdiff_t)q.jn - (ptrdiff_t)j, aux + (size_t)num_lookup_cols * N, j, q.jn, k);
    gl_t zi = (q.i & 1) ? zh_inv1 : zh_inv0;
#pragma unroll
    for (int a = 0; a < NA; a++) out[(size_t)a * size + q.i] = gl_mul(k.acc[a], zi);
}

struct ctl_chunk {
    uint32_t z, helper_start, q0, q1, closing, tail;  // tail = K - k_end: constraints that follow the chunk
};
template <int NA>
__global__ __launch_bounds__(256) void k_quotient_ctl_chunk(const gl_t* __restrict__ trace, const gl_t* __restrict__ aux, unsigned lde_bits, ctl_dev ctl,
                                                            const ctl_chunk* __restrict__ chunks, uint32_t num_lookup_cols, alpha_args alphas_v,
                                                            const gl_t* __restrict__ wpow, gl_t gn, gl_t last, gl_t w_n, gl_t n_inv,
                                                            gl_t* __restrict__ tmp /* [segment][chunk][NA][size] */, size_t trace_seg, size_t aux_seg) {
    const gl_t* const alphas = alphas_v.v + 2 * blockIdx.z;
    size_t N = (size_t)1 << lde_bits;
    size_t size = N >> 1;
    size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= size) return;
    trace += (size_t)blockIdx.z * trace_seg;
    aux += (size_t)blockIdx.z * aux_seg;
    tmp += (size_t)blockIdx.z * gridDim.y * NA * size;
    ctl.zs += (size_t)blockIdx.z * ctl.nzs;
    const ctl_chunk ch = chunks[blockIdx.y];
    consumer_t<NA> k;
    const quotient_point q = quotient_setup<NA>(j, lde_bits, alphas, wpow, gn, last, w_n, n_inv, k);
    eval_ctl_z<NA>(ctl, ch.z, ch.helper_start, ch.q0, ch.q1, ch.closing != 0, trace + j, N, (ptrdiff_t)q.jn - (ptrdiff_t)j,
                   aux + (size_t)num_lookup_cols * N, j, q.jn, k);
#pragma unroll
    for (int a = 0; a < NA; a++)
        tmp[((size_t)blockIdx.y * NA + a) * size + q.i] = gl_mul(k.acc[a], gl_pow(k.alpha[a], ch.tail));
}
template <int NA>
__global__ __launch_bounds__(256) void k_quotient_ctl_sum(const gl_t* __restrict__ tmp, uint32_t nchunks, uint32_t nconstraints, alpha_args alphas_v,
                                                          gl_t zh_inv0, gl_t zh_inv1, size_t size, gl_t* __restrict__ out) {
    const gl_t* const alphas = alphas_v.v + 2 * blockIdx.z;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= size) return;
    tmp += (size_t)blockIdx.z * nchunks * NA * size;
    out += (size_t)blockIdx.z * NA * size;
    gl_t zi = (i & 1) ? zh_inv1 : zh_inv0;
#pragma unroll
    for (int a = 0; a < NA; a++) {
        gl_t acc = gl_mul(out[(size_t)a * size + i], gl_pow(alphas[a], nconstraints));
        for (uint32_t c = 0; c < nchunks; c++) acc = gl_add(acc, tmp[((size_t)c * NA + a) * size + i]);
        out[(size_t)a * size + i] = gl_mul(acc, zi);
    }
}

// the table's own lookups as the constraint kernels take them (lookup_dev, and the nseg x nalphas lookup challenges in kernel-argument
// form); returns the number of lookup columns in front of the CTL columns
static uint32_t table_lookup_args(int table_id, size_t nalphas, const uint64_t* lookup_challenges, size_t nseg, lookup_dev& lookups,
                                  seg_gl2& lookup_ch) {
    uint32_t NL = 0;
    size_t nl = 0;
    const zkm_table_lookup* defs = zkm_table_lookups(table_id, &nl);
    if (nl && !lookup_challenges) throw std::runtime_error("zkm_quotient: this table has lookups; lookup challenges are required");
    if (nl > 2) throw std::runtime_error("zkm_quotient: too many lookups");
    lookups.nlookups = (uint32_t)nl;
    lookups.nch = (uint32_t)nalphas;
    uint32_t off = 0;
    for (size_t l = 0; l < nl; l++) {
        if (off + defs[l].ncols > 24) throw std::runtime_error("zkm_quotient: too many lookup columns");
        lookups.lk[l] = {defs[l].ncols, off, defs[l].table_col, defs[l].freq_col};
        for (uint32_t i = 0; i < defs[l].ncols; i++) lookups.cols[off + i] = defs[l].cols[i];
        off += defs[l].ncols;
        NL += ((defs[l].ncols + 1) / 2 + 1) * (uint32_t)nalphas;
    }
    for (size_t sg = 0; nl && sg < nseg; sg++)
        for (size_t i = 0; i < nalphas; i++) lookup_ch.v[2 * sg + i] = lookup_challenges[sg * nalphas + i];
    return NL;
}

// f(std::integral_constant<int, NA>) for a run-time number of constraint challenges: the one way from it to a template argument
// (tables.h zkm_with_table does the same for the table id)
template <class F> decltype(auto) with_nalphas(size_t nalphas, F&& f) {
    switch (nalphas) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        default: throw std::runtime_error("1 or 2 challenges supported");
    }
}

// what every quotient launch of one table takes beside the columns: the two-level table of w_{4n}^t, g^n (0: the kernels' check mode,
// quotient_setup), 1 / Z_H on the even and odd points, w_n^-1 (the last row), w_n, 1 / n
struct quotient_consts {
    const gl_t* wpow;
    gl_t gn, zh0, zh1, last, w_n, n_inv;
};
// points of the quotient domain per segment (check mode, rate_bits = 0: every row of the trace)
static size_t quotient_points(const zkm_batch* trace) { return trace->rate_bits ? trace->N() >> 1 : trace->N(); }

// the table's own constraints and lookups: d_vals = the running accumulators, nseg x nalphas x points
static void launch_table_constraints(zkm_ctx* c, int table_id, const zkm_batch* trace, const zkm_batch* aux, const lookup_dev& lookups,
                                     const seg_gl2& lookup_ch, const alpha_args& alphas, size_t nalphas, const quotient_consts& q, gl_t* d_vals) {
    const size_t nseg = trace->nseg, size = quotient_points(trace), trace_seg = trace->lde_seg(), aux_seg = aux->lde_seg();
    const unsigned z = (unsigned)nseg, log_n = trace->log_n, lde_bits = trace->lde_bits();
    zkm_prof_scope ps(c, zkm_table(table_id)->quotient_scope);
    dim3 grid((size + 255) / 256, 1, z), block(256);
    if (table_id == ZKM_TABLE_KECCAK && size * nseg <= c->keccak_parts_max_points && q.gn != 0) {
        // short table: 25 threads per point, then the sum of the parts (constraints_dev.h)
        const size_t per = nalphas * (KECCAK_NUM_CONSTRAINTS + 1);
        std::vector<gl_t> apw(nseg * per);
        for (size_t sg = 0; sg < nseg; sg++)
            for (size_t a = 0; a < nalphas; a++) {
                gl_t p = 1;
                for (size_t e = 0; e <= KECCAK_NUM_CONSTRAINTS; e++) {
                    apw[sg * per + a * (KECCAK_NUM_CONSTRAINTS + 1) + e] = p;
                    p = gl_mul(p, gl_canon(alphas.v[2 * sg + a]));
                }
            }
        zkm_scratch d_apw(c, apw.size() * sizeof(gl_t)), d_tmp(c, nseg * (size_t)KECCAK_CONSTRAINT_PARTS * nalphas * size * sizeof(gl_t));
        c->upload(d_apw.p, apw.data(), apw.size() * sizeof(gl_t));
        dim3 gridp((unsigned)((size + 255) / 256), KECCAK_CONSTRAINT_PARTS, z);
        with_nalphas(nalphas, [&](auto NA) {
            hipLaunchKernelGGL((k_quotient_keccak_parts<decltype(NA)::value>), gridp, block, 0, c->stream, trace->lde, lde_bits, alphas, q.wpow, q.gn, q.last,
                               q.w_n, q.n_inv, d_apw.as<gl_t>(), d_tmp.as<gl_t>(), trace_seg);
        });
        hipLaunchKernelGGL(k_sum_parts, dim3((unsigned)((nalphas * size + 255) / 256), 1, z), block, 0, c->stream, d_tmp.as<gl_t>(),
                           (unsigned)KECCAK_CONSTRAINT_PARTS, nalphas * size, d_vals);
    } else
        zkm_with_table(table_id, [&](auto T) {
            with_nalphas(nalphas, [&](auto NA) {
                hipLaunchKernelGGL((k_quotient<decltype(T)::value, decltype(NA)::value>), grid, block, 0, c->stream, trace->lde, aux->lde, log_n, lde_bits,
                                   lookups, alphas, lookup_ch, q.wpow, q.gn, q.last, q.w_n, q.n_inv, d_vals, trace_seg, aux_seg);
            });
        });
    ZKM_HIP_CHECK(hipGetLastError());
}

// the CTL checks behind NL lookup columns, continuing the accumulators in d_vals, and the division by Z_H
static void launch_ctl_checks(zkm_ctx* c, const zkm_batch* trace, const zkm_batch* aux, const ctl_dev_owner& own, uint32_t NL, const alpha_args& alphas,
                              size_t nalphas, const quotient_consts& q, gl_t* d_vals) {
    const size_t nseg = trace->nseg, size = quotient_points(trace), trace_seg = trace->lde_seg(), aux_seg = aux->lde_seg();
    const unsigned z = (unsigned)nseg, lde_bits = trace->lde_bits();
    zkm_prof_scope ps(c, "quotient_ctl");
    dim3 grid((size + 255) / 256, 1, z), block(256);
    // chunk plan: at most CHUNK helper checks per chunk, the closing checks with the last chunk of their Z.  A thread's work is a
    // chain of column-combination evaluations whatever the table's height: on short tables (a launch cannot fill the GPU anyway)
    // one helper check per chunk -- four times the workgroups, a quarter of the chain (KeccakSponge at 2^8 rows: 340 us per launch)
    const bool short_table = size * nseg <= ((size_t)1 << 15);
    const uint32_t CHUNK = short_table ? 1 : 4;
    std::vector<ctl_chunk> plan;
    uint32_t K = 0, hstart = 0;
    for (uint32_t zi = 0; zi < own.h_zs.size(); zi++) {
        // helper checks exist only for real column sets (the benchmark's fake CTL data has helper columns but no sets)
        const uint32_t np = own.h_zs[zi].num_helpers ? (own.h_zs[zi].ncolsets + 1) / 2 : 0;
        uint32_t q0 = 0;
        do {
            const uint32_t q1 = np - q0 > CHUNK ? q0 + CHUNK : np;
            const bool closing = q1 == np;
            K += (q1 - q0) + (closing ? 2 : 0);
            plan.push_back(ctl_chunk{zi, hstart, q0, q1, closing ? 1u : 0u, K});   // (tail: k_end until the count K is known)
            q0 = q1;
        } while (q0 < np);
        hstart += own.h_zs[zi].num_helpers;
    }
    for (ctl_chunk& ch : plan) ch.tail = K - ch.tail;
    const bool chunked = plan.size() >= (short_table ? 2u : 8u) && size * nseg <= ((size_t)1 << 18) && q.gn != 0;
    if (!chunked) {
        with_nalphas(nalphas, [&](auto NA) {
            hipLaunchKernelGGL((k_quotient_ctl<decltype(NA)::value>), grid, block, 0, c->stream, trace->lde, aux->lde, lde_bits, own.d, NL, alphas, q.wpow, q.gn,
                               q.zh0, q.zh1, q.last, q.w_n, q.n_inv, d_vals, trace_seg, aux_seg);
        });
    } else {
        zkm_scratch_list tmp(c);
        ctl_chunk* d_plan = tmp.alloc<ctl_chunk>(plan.size() * sizeof(ctl_chunk));
        gl_t* d_tmp = tmp.alloc<gl_t>(nseg * plan.size() * nalphas * size * sizeof(gl_t));
        c->upload(d_plan, plan.data(), plan.size() * sizeof(ctl_chunk));
        dim3 grid2((unsigned)((size + 255) / 256), (unsigned)plan.size(), z);
        with_nalphas(nalphas, [&](auto NA) {
            hipLaunchKernelGGL((k_quotient_ctl_chunk<decltype(NA)::value>), grid2, block, 0, c->stream, trace->lde, aux->lde, lde_bits, own.d, d_plan, NL, alphas,
                               q.wpow, q.gn, q.last, q.w_n, q.n_inv, d_tmp, trace_seg, aux_seg);
            hipLaunchKernelGGL((k_quotient_ctl_sum<decltype(NA)::value>), grid, block, 0, c->stream, d_tmp, (uint32_t)plan.size(), K, alphas, q.zh0, q.zh1,
                               size, d_vals);
        });
        ZKM_HIP_CHECK(hipGetLastError());
        // (no host sync: upload() has copied `plan` into the pinned ring -- or waited itself if it was too large for it -- and the
        // blocks released here are only reused by later work on this stream)
    }
    ZKM_HIP_CHECK(hipGetLastError());
}

// quotient polys: d_out = nalphas x 2n natural-order coefficients (device) -- per segment of the stack (trace / aux: stacked batches of
// the same nseg; alphas_host: nseg x nalphas; lookup_challenges: nseg x nalphas; own: a description with nseg lists of CtlZData)
// check = true (zkm_check_constraints): trace / aux describe the VALUES (lde = ncols x n values, rate_bits 0) and d_out receives the
// alpha-accumulated constraint values of every row, nalphas x n, instead of quotient coefficients.
static void quotient_device(zkm_ctx* c, int table_id, const zkm_batch* trace, const zkm_batch* aux, const ctl_dev_owner& own,
                            const uint64_t* lookup_challenges, const gl_t* alphas_host, size_t nalphas, gl_t* d_out, bool check = false) {
    lookup_dev lookups{};
    seg_gl2 lookup_ch{};
    const size_t nseg = trace->nseg;
    if (aux->nseg != nseg || nseg == 0 || nseg > ZKM_MAX_SEG) throw std::runtime_error("zkm_quotient: batches of different stacks");
    const uint32_t NL = table_lookup_args(table_id, nalphas, lookup_challenges, nseg, lookups, lookup_ch);
    if (zkm_table_width(table_id) == 0 || trace->ncols != zkm_table_width(table_id))
        throw std::runtime_error("zkm_quotient: unknown table id, or the trace width does not match the table");
    if (trace->rate_bits != (check ? 0u : 2u) || aux->rate_bits != trace->rate_bits || trace->log_n != aux->log_n)
        throw std::runtime_error("zkm_quotient: rate_bits must be 2 and the batches must have equal degree");
    if (nalphas < 1 || nalphas > 2) throw std::runtime_error("zkm_quotient: 1 or 2 challenges supported");
    if (own.naux + NL != aux->ncols) throw std::runtime_error("zkm_quotient: aux column count does not match the CTL description");
    const unsigned log_n = trace->log_n, lde_bits = trace->lde_bits(), log_q = check ? log_n : log_n + 1;
    const size_t size = quotient_points(trace);
    const gl_t gn = check ? 0 : gl_exp_pow2(GL_GENERATOR, log_n), w_n = gl_root_of_unity(log_n);
    const quotient_consts q{c->pow_table(gl_root_of_unity(lde_bits), lde_bits), gn, check ? 1 : gl_inv(gl_sub(gn, 1)), check ? 1 : gl_inv(gl_sub(gl_neg(gn), 1)),
                            gl_inv(w_n), w_n, gl_inv((gl_t)(((uint64_t)1 << log_n) % GL_P))};
    alpha_args d_alphas{};
    for (size_t sg = 0; sg < nseg; sg++)
        for (size_t a = 0; a < nalphas; a++) d_alphas.v[2 * sg + a] = alphas_host[sg * nalphas + a];
    zkm_scratch vals(c, nseg * nalphas * size * sizeof(gl_t));
    gl_t* const d_vals = vals.as<gl_t>();
    launch_table_constraints(c, table_id, trace, aux, lookups, lookup_ch, d_alphas, nalphas, q, d_vals);
    launch_ctl_checks(c, trace, aux, own, NL, d_alphas, nalphas, q, d_vals);
    if (check) {
        ZKM_HIP_CHECK(hipMemcpyAsync(d_out, d_vals, nseg * nalphas * size * sizeof(gl_t), hipMemcpyDeviceToDevice, c->stream));
        return;
    }
    // coset_ifft(g) of each challenge's evaluations (prover.rs:784-788)
    zkm_ntt_natural(c, d_vals, d_out, nseg * nalphas, size, size, log_q, true, GL_GENERATOR);
}   // (`vals` goes back: stream-ordered reuse, no host sync needed)

// ------------------------------------------------------------------ the verifier's constraint check at zeta (verifier.rs:205-264)
// The functions above evaluate the constraints over the base field; the verifier needs them at the opened values v = v0 + v1 X in
// F2 = F[X] / (X^2 - 7).  Every constraint is a polynomial with base-field coefficients (the constraint, CTL and lookup challenges are
// base-field) of degree <= 3 in the opened values, so c(v0 + t v1) is a polynomial of degree <= 3 in t: it is evaluated at the
// BASE-FIELD rows v0 + t v1 for t = 0 .. 4 with the same code k_quotient runs, interpolated, and t replaced by X on the host
// (verify.hip).  The Lagrange / last-row multipliers are F2 values too, and not linear in t: the accumulator is linear in
// (1, z_last, l_first, l_last), so four consumer settings -- (0,0,0), (1,0,0), (0,1,0), (0,0,1) -- separate the plain, transition,
// first-row and last-row classes, and the true multipliers are applied after the interpolation.  Thread 4 t + setting of workgroup z
// handles point t of (segment, table) entry z; the rows are a two-row buffer per point: column c at [2 c] (local) and [2 c + 1] (next).
struct seg_off { uint64_t v[ZKM_MAX_SEG]; };
template <int TABLE>
__global__ __launch_bounds__(64) void k_verify_line(const gl_t* __restrict__ rows, seg_off rows_off, gl_t* __restrict__ acc, seg_off acc_off, uint32_t W,
                                                    uint32_t A, uint32_t NL, lookup_dev lookups, alpha_args alphas_v, seg_gl2 lookup_ch, ctl_dev ctl) {
    const unsigned tid = threadIdx.x;
    if (tid >= ZKM_VERIFY_LINE_THREADS) return;
    const unsigned t = tid >> 2, setting = tid & 3;
    const gl_t* const tl = rows + rows_off.v[blockIdx.z] + (size_t)t * 2 * (W + A);
    const gl_t* const aux = tl + 2 * (size_t)W;
    consumer_t<2> k;
#pragma unroll
    for (int a = 0; a < 2; a++) { k.set_alpha(a, alphas_v.v[2 * blockIdx.z + a]); k.acc[a] = 0; }
    k.z_last = setting == 1 ? 1 : 0;
    k.l_first = setting == 2 ? 1 : 0;
    k.l_last = setting == 3 ? 1 : 0;
    eval_table_constraints<TABLE, 2>(tl, 2, 1, k);
    if constexpr (TABLE == ZKM_TABLE_MEMORY || TABLE == ZKM_TABLE_ARITHMETIC)
        eval_lookup_constraints<2>(lookups, lookup_ch.v + 2 * blockIdx.z, tl, 2, aux, 0, 1, k);
    ctl.zs += (size_t)blockIdx.z * ctl.nzs;
    eval_ctl_constraints<2>(ctl, tl, 2, 1, aux + 2 * (size_t)NL, 0, 1, k);
    gl_t* const o = acc + acc_off.v[blockIdx.z] + 2 * tid;
    o[0] = k.value(0);
    o[1] = k.value(1);
}

void zkm_verify_line_constraints(zkm_ctx* c, int table_id, size_t nalphas, const ctl_dev& own, size_t naux, const uint64_t* lookup_challenges,
                                 const gl_t* alphas, const gl_t* d_rows, const uint64_t* rows_off, gl_t* d_acc, const uint64_t* acc_off,
                                 size_t W, size_t A, size_t nseg) {
    if (nseg == 0 || nseg > ZKM_MAX_SEG) throw std::runtime_error("verify: segment count of a constraint launch out of range");
    if (nalphas < 1 || nalphas > 2) throw std::runtime_error("verify: 1 or 2 challenges supported");
    if (!zkm_table(table_id) || zkm_table_width(table_id) != W) throw std::runtime_error("verify: unknown table id, or the width does not match the table");
    lookup_dev lookups{};
    seg_gl2 lookup_ch{};
    const uint32_t NL = table_lookup_args(table_id, nalphas, lookup_challenges, nseg, lookups, lookup_ch);
    if (naux + NL != A) throw std::runtime_error("verify: aux column count does not match the CTL description");
    alpha_args d_alphas{};   // (one challenge: the second accumulator runs with alpha 0 and is ignored)
    seg_off ro{}, ao{};
    for (size_t sg = 0; sg < nseg; sg++) {
        for (size_t a = 0; a < nalphas; a++) d_alphas.v[2 * sg + a] = alphas[sg * nalphas + a];
        ro.v[sg] = rows_off[sg];
        ao.v[sg] = acc_off[sg];
    }
    zkm_prof_scope ps(c, zkm_table(table_id)->line_scope);
    const dim3 grid(1, 1, (unsigned)nseg), block(64);
    zkm_with_table(table_id, [&](auto T) {
        hipLaunchKernelGGL((k_verify_line<decltype(T)::value>), grid, block, 0, c->stream, d_rows, ro, d_acc, ao, (uint32_t)W, (uint32_t)A, NL, lookups, d_alphas, lookup_ch,
                           own);
    });
    ZKM_HIP_CHECK(hipGetLastError());
}

// ------------------------------------------------------------------ K10: openings
// partial[col][chunk] = sum_{k in chunk} c_k z^(k - chunk_start) for z in {zeta, g*zeta}, plus the plain sum (evaluation
// at 1).  The coefficients are base-field elements, so with a table of the powers z^k = (a_k, b_k) of the chunk (shared by
// every column and chunk; 4 x 2^14 words, L2-resident) each coefficient costs four BASE multiplications -- sum c_k a_k,
// sum c_k b_k for the two points -- instead of two extension-field Horner steps, and the sums are accumulated lazily
// (64-bit wrapping adds with a wrap counter, 2^64 == EPS applied once at the end).  A workgroup handles OPEN_CPB columns
// of one chunk so a power is loaded once per OPEN_CPB coefficients; all loads are coalesced.
#define OPEN_CHUNK_LOG 14
#define OPEN_CPB 4
// pw[.][k] = z^(exponent of position k of a column): the batch's coefficient layout (zkm_coeff_exponent) is a permutation of the BITS
// of the position, so the exponent of position chunk * chunk_len + k is e(k) + e(chunk * chunk_len) and the table of one chunk serves all.
// (blockIdx.z = segment of a stack: its own two points, its own table)
__global__ __launch_bounds__(256) void k_open_powers(seg_gl2 z0s, seg_gl2 z1s, unsigned chunk_len, unsigned coeff_s1,
                                                     gl_t* __restrict__ pw /* [segment][4][chunk_len] */) {
    unsigned k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= chunk_len) return;
    const gl2_t z0{z0s.v[2 * blockIdx.z], z0s.v[2 * blockIdx.z + 1]}, z1{z1s.v[2 * blockIdx.z], z1s.v[2 * blockIdx.z + 1]};
    pw += (size_t)blockIdx.z * 4 * chunk_len;
    const uint64_t e = zkm_coeff_exponent(k, coeff_s1);
    gl2_t p0 = gl2_pow(z0, e), p1 = gl2_pow(z1, e);
    pw[k] = p0.c0; pw[chunk_len + k] = p0.c1; pw[2 * chunk_len + k] = p1.c0; pw[3 * chunk_len + k] = p1.c1;
}
struct lazy_sum {
    uint64_t lo;
    uint32_t wraps;
    __device__ __forceinline__ void add(uint64_t v) {
        lo += v;
        wraps += lo < v;
    }
    __device__ __forceinline__ gl_t value() const {  // lo + wraps 2^64 == lo + wraps EPS (wraps < 2^32: one multiply-add)
        uint64_t r = (uint64_t)wraps * 0xFFFFFFFFu + lo;
        r += (r < lo) ? GL_EPS : 0;
        return gl_canon(r);
    }
};
// (CPB columns per workgroup: 4 amortises the power loads when the launch fills the machine anyway; 1 when it would be a few hundred
// workgroups -- tables of 2^16 / 2^17 rows: four times the waves for the same work)
template <int CPB>
__global__ __launch_bounds__(256) void k_open_partials(const gl_t* __restrict__ coeffs, unsigned log_n, size_t ncols,
                                                       const gl_t* __restrict__ pw, gl_t* __restrict__ partial /* [col][chunk][5] */,
                                                       size_t coeff_seg, size_t partial_seg) {
    __shared__ gl_t red[256 * 5];
    const unsigned chunk_log = log_n < OPEN_CHUNK_LOG ? log_n : OPEN_CHUNK_LOG;
    const size_t chunk_len = (size_t)1 << chunk_log, nchunks = (size_t)1 << (log_n - chunk_log);
    coeffs += (size_t)blockIdx.z * coeff_seg;
    pw += (size_t)blockIdx.z * 4 * chunk_len;
    partial += (size_t)blockIdx.z * partial_seg;
    const size_t col0 = (size_t)blockIdx.y * CPB, chunk = blockIdx.x;
    const unsigned t = threadIdx.x;
    lazy_sum acc[CPB][5];
#pragma unroll
    for (int c = 0; c < CPB; c++)
#pragma unroll
        for (int q = 0; q < 5; q++) acc[c][q] = lazy_sum{0, 0};
    // (software-pipelined by hand: the loads of step k + 1 -- four powers, CPB coefficients -- are issued before the 4 CPB products of step
    // k; with one load-use pair per iteration every one of the 64 steps of a chunk exposed a trip to L2 / HBM at four waves per SIMD)
    gl_t np[4], ncv[CPB];
    auto fetch = [&](size_t idx) {
#pragma unroll
        for (int q = 0; q < 4; q++) np[q] = pw[(size_t)q * chunk_len + idx];
#pragma unroll
        for (int c = 0; c < CPB; c++) {
            // (columns past the end of the batch read column ncols - 1 again; their sums are never stored)
            const size_t col = col0 + c < ncols ? col0 + c : ncols - 1;
            ncv[c] = coeffs[(col << log_n) + chunk * chunk_len + idx];
        }
    };
    if (t < chunk_len) fetch(t);
    for (size_t idx = t; idx < chunk_len; idx += 256) {
        gl_t p[4], cvs[CPB];
#pragma unroll
        for (int q = 0; q < 4; q++) p[q] = np[q];
#pragma unroll
        for (int c = 0; c < CPB; c++) cvs[c] = ncv[c];
        if (idx + 256 < chunk_len) fetch(idx + 256);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int c = 0; c < CPB; c++) {
            const gl_t cv = cvs[c];
#pragma unroll
            for (int q = 0; q < 4; q++) acc[c][q].add(gl_mul_loose(cv, p[q]));
            acc[c][4].add(cv);
        }
    }
#pragma unroll
    for (int c = 0; c < CPB; c++) {
#pragma unroll
        for (int q = 0; q < 5; q++) red[t * 5 + q] = acc[c][q].value();
        __syncthreads();
        for (unsigned s = 128; s > 0; s >>= 1) {
            if (t < s)
                for (int q = 0; q < 5; q++) red[t * 5 + q] = gl_add(red[t * 5 + q], red[(t + s) * 5 + q]);
            __syncthreads();
        }
        if (t < 5 && col0 + c < ncols) partial[((col0 + c) * nchunks + chunk) * 5 + t] = red[t];
        __syncthreads();
    }
}

struct open_vals { gl2_t at_z0, at_z1; gl_t at_one; };

// evaluate every polynomial of the batches (same height, same coefficient layout) at z0, z1 (F2) and 1: one power table, one launch
// per batch, one download.  Stacked batches (nseg segments each): z0 / z1 hold one point per segment, out[s][batch][poly].
static std::vector<std::vector<std::vector<open_vals>>> eval_batches(zkm_ctx* c, const std::vector<const zkm_batch*>& bs, const gl2_t* z0,
                                                                     const gl2_t* z1) {
    const zkm_batch* b0 = bs.at(0);
    const size_t nseg = b0->nseg;
    const unsigned log_n = b0->log_n, chunk_log = log_n < OPEN_CHUNK_LOG ? log_n : OPEN_CHUNK_LOG, chunk_len = 1u << chunk_log;
    const size_t nchunks = (size_t)1 << (log_n - chunk_log);
    size_t total_cols = 0;
    for (const zkm_batch* b : bs) {
        if (b->log_n != log_n || b->coeff_s1 != b0->coeff_s1 || b->nseg != nseg) throw std::runtime_error("internal: openings of batches with different shapes");
        total_cols += b->ncols;
    }
    if (nseg == 0 || nseg > ZKM_MAX_SEG) throw std::runtime_error("internal: openings of a stack of unsupported size");
    const unsigned z = (unsigned)nseg;
    const size_t words_seg = total_cols * nchunks * 5, words = nseg * words_seg;
    zkm_scratch d_part(c, words * sizeof(gl_t)), d_pw(c, nseg * 4 * chunk_len * sizeof(gl_t));
    {
        zkm_prof_scope ps(c, "open_partials");
        seg_gl2 z0s{}, z1s{};
        for (size_t sg = 0; sg < nseg; sg++) { z0s.v[2 * sg] = z0[sg].c0; z0s.v[2 * sg + 1] = z0[sg].c1; z1s.v[2 * sg] = z1[sg].c0; z1s.v[2 * sg + 1] = z1[sg].c1; }
        hipLaunchKernelGGL(k_open_powers, dim3((chunk_len + 255) / 256, 1, z), dim3(256), 0, c->stream, z0s, z1s, chunk_len, b0->coeff_s1, d_pw.as<gl_t>());
        size_t col0 = 0;
        for (const zkm_batch* b : bs) {
            if (nseg * nchunks * ((b->ncols + OPEN_CPB - 1) / OPEN_CPB) < 1024)
                hipLaunchKernelGGL(k_open_partials<1>, dim3(nchunks, b->ncols, z), dim3(256), 0, c->stream, b->coeffs, log_n, b->ncols, d_pw.as<gl_t>(),
                                   d_part.as<gl_t>() + col0 * nchunks * 5, b->coeff_seg(), words_seg);
            else
                hipLaunchKernelGGL(k_open_partials<OPEN_CPB>, dim3(nchunks, (b->ncols + OPEN_CPB - 1) / OPEN_CPB, z), dim3(256), 0, c->stream, b->coeffs,
                                   log_n, b->ncols, d_pw.as<gl_t>(), d_part.as<gl_t>() + col0 * nchunks * 5, b->coeff_seg(), words_seg);
            col0 += b->ncols;
        }
        ZKM_HIP_CHECK(hipGetLastError());
    }
    std::vector<gl_t> part(words);
    c->download(part.data(), d_part.p, words * sizeof(gl_t));
    std::vector<std::vector<std::vector<open_vals>>> all(nseg);
    std::vector<gl2_t> f0(nchunks), f1(nchunks);
    for (size_t sg = 0; sg < nseg; sg++) {
        // chunk ch contributes z^(exponent of its first position) * partial (natural order: z^(ch * chunk_len), i.e. Horner over the chunks)
        for (size_t ch = 0; ch < nchunks; ch++) {
            const uint64_t e = zkm_coeff_exponent((uint32_t)(ch << chunk_log), b0->coeff_s1);
            f0[ch] = gl2_pow(z0[sg], e);
            f1[ch] = gl2_pow(z1[sg], e);
        }
        size_t col0 = 0;
        for (const zkm_batch* b : bs) {
            std::vector<open_vals> o(b->ncols);
            for (size_t col = 0; col < b->ncols; col++) {
                gl2_t a0{0, 0}, a1{0, 0};
                gl_t sum = 0;
                for (size_t ch = 0; ch < nchunks; ch++) {
                    const gl_t* q = &part[sg * words_seg + ((col0 + col) * nchunks + ch) * 5];
                    a0 = gl2_add(a0, gl2_mul(f0[ch], gl2_t{q[0], q[1]}));
                    a1 = gl2_add(a1, gl2_mul(f1[ch], gl2_t{q[2], q[3]}));
                    sum = gl_add(sum, q[4]);
                }
                o[col] = open_vals{a0, a1, sum};
            }
            all[sg].push_back(std::move(o));
            col0 += b->ncols;
        }
    }
    return all;
}

// ------------------------------------------------------------------ K11: FRI batch combination
// comp1 = sum_{j < W+A} alpha^j p_j (g*zeta batch), comp0 = comp1 + sum_q alpha^(W+A+q) quot_q (zeta batch),
// comp2 = sum_k alpha^k ctl_z_k (batch at 1)   -- polynomial order of stark.rs:127-148.  One pass over all
// coefficient polynomials; alpha powers are wave-uniform.
__global__ __launch_bounds__(256) void k_fri_combine(const gl_t* __restrict__ tc, size_t W, const gl_t* __restrict__ ac, size_t A,
                                                     const gl_t* __restrict__ qc, size_t Q, size_t ctl_start,
                                                     const gl_t* __restrict__ apow /* [(W+A+Q)][2] */, size_t n,
                                                     gl_t* __restrict__ comp /* [3][2][n] */, size_t apow_seg) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    // (blockIdx.z = segment of a stack: its coefficient columns follow the previous segment's, its own powers of its own alpha)
    tc += (size_t)blockIdx.z * W * n; ac += (size_t)blockIdx.z * A * n; qc += (size_t)blockIdx.z * Q * n;
    apow += (size_t)blockIdx.z * apow_seg;
    comp += (size_t)blockIdx.z * 6 * n;
    gl_t a0 = 0, a1 = 0, z0 = 0, z1 = 0;
    size_t j = 0;
    for (size_t cidx = 0; cidx < W; cidx++, j++) {
        gl_t v = tc[cidx * n + i];
        a0 = gl_add(a0, gl_mul(v, apow[2 * j]));
        a1 = gl_add(a1, gl_mul(v, apow[2 * j + 1]));
    }
    for (size_t cidx = 0; cidx < A; cidx++, j++) {
        gl_t v = ac[cidx * n + i];
        a0 = gl_add(a0, gl_mul(v, apow[2 * j]));
        a1 = gl_add(a1, gl_mul(v, apow[2 * j + 1]));
        if (cidx >= ctl_start) {
            size_t k = cidx - ctl_start;
            z0 = gl_add(z0, gl_mul(v, apow[2 * k]));
            z1 = gl_add(z1, gl_mul(v, apow[2 * k + 1]));
        }
    }
    comp[2 * n + i] = a0;
    comp[3 * n + i] = a1;
    for (size_t cidx = 0; cidx < Q; cidx++, j++) {
        gl_t v = qc[cidx * n + i];
        a0 = gl_add(a0, gl_mul(v, apow[2 * j]));
        a1 = gl_add(a1, gl_mul(v, apow[2 * j + 1]));
    }
    comp[i] = a0;
    comp[n + i] = a1;
    comp[4 * n + i] = z0;
    comp[5 * n + i] = z1;
}

// Short, wide tables (Keccak: 2431 columns x 2^11 rows): one thread per coefficient index leaves the machine empty and walks thousands
// of columns serially (1 ms for that table).  Here blockIdx.y takes a slice of the W + A + Q polynomials and writes its partial sums
// (trace + aux part, quotient part, CTL part) to part[slice][6][n]; k_fri_combine_sum adds the slices.  Field addition is exact, so the
// result is the same words as k_fri_combine's.
__global__ __launch_bounds__(256) void k_fri_combine_slice(const gl_t* __restrict__ tc, size_t W, const gl_t* __restrict__ ac, size_t A,
                                                           const gl_t* __restrict__ qc, size_t Q, size_t ctl_start,
                                                           const gl_t* __restrict__ apow, size_t n, size_t per_slice,
                                                           gl_t* __restrict__ part /* [segment][slices][6][n] */, size_t apow_seg) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    tc += (size_t)blockIdx.z * W * n; ac += (size_t)blockIdx.z * A * n; qc += (size_t)blockIdx.z * Q * n;
    apow += (size_t)blockIdx.z * apow_seg;
    part += (size_t)blockIdx.z * gridDim.y * 6 * n;
    const size_t j0 = (size_t)blockIdx.y * per_slice, total = W + A + Q;
    const size_t j1 = j0 + per_slice < total ? j0 + per_slice : total;
    gl_t a0 = 0, a1 = 0, q0 = 0, q1 = 0, z0 = 0, z1 = 0;
    for (size_t j = j0; j < j1; j++) {
        if (j < W + A) {
            const gl_t v = j < W ? tc[j * n + i] : ac[(j - W) * n + i];
            a0 = gl_add(a0, gl_mul(v, apow[2 * j]));
            a1 = gl_add(a1, gl_mul(v, apow[2 * j + 1]));
            if (j >= W + ctl_start) {
                const size_t k = j - W - ctl_start;
                z0 = gl_add(z0, gl_mul(v, apow[2 * k]));
                z1 = gl_add(z1, gl_mul(v, apow[2 * k + 1]));
            }
        } else {
            const gl_t v = qc[(j - W - A) * n + i];
            q0 = gl_add(q0, gl_mul(v, apow[2 * j]));
            q1 = gl_add(q1, gl_mul(v, apow[2 * j + 1]));
        }
    }
    gl_t* o = part + (size_t)blockIdx.y * 6 * n + i;
    o[0] = a0; o[n] = a1; o[2 * n] = q0; o[3 * n] = q1; o[4 * n] = z0; o[5 * n] = z1;
}
__global__ __launch_bounds__(256) void k_fri_combine_sum(const gl_t* __restrict__ part, unsigned slices, size_t n, gl_t* __restrict__ comp) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    part += (size_t)blockIdx.z * slices * 6 * n;
    comp += (size_t)blockIdx.z * 6 * n;
    gl_t t[6] = {0, 0, 0, 0, 0, 0};
    for (unsigned s = 0; s < slices; s++)
#pragma unroll
        for (int k = 0; k < 6; k++) t[k] = gl_add(t[k], part[((size_t)s * 6 + k) * n + i]);
    comp[2 * n + i] = t[0];
    comp[3 * n + i] = t[1];
    comp[i] = gl_add(t[0], t[2]);
    comp[n + i] = gl_add(t[1], t[3]);
    comp[4 * n + i] = t[4];
    comp[5 * n + i] = t[5];
}

// divide_by_linear as a hierarchical suffix scan with segments of FRI_SEG (profiles/HISTORY.md), for ALL batches of the instance in one set of
// launches (blockIdx.y = batch; the STARK instance has three: zeta, g zeta, 1).  Per batch b: q_b = (comp_b(X) - comp_b(z_b)) / (X - z_b),
// q_b[k - 1] = S_b[k] with S_b[k] = a_b[k] + z_b S_b[k + 1]; the final polynomial is sum_b w_b q_b, w_b = prod_{b' > b} shift_b'
// (plonky2 accumulates final = final * alpha^(#polys of the batch) + quotient, batch by batch: the same sum, regrouped).
// A thread walks ONE segment of ONE batch -- a chain of FRI_SEG dependent extension-field multiply-adds; the weighted sum over the
// batches is a separate element-wise launch.  (Until round 3: segments of 64 and the bottom level walking all batches in one
// thread, 192 dependent steps: 158 us per table in a 2^16-cycle segment, whatever its size.)
#define FRI_MAX_BATCHES 8
// (segment length: the chain a thread walks.  With the LDS tiles the kernels are chains of dependent extension-field steps at low
// occupancy, so shorter segments -- more, cheaper levels -- win: 2^22 coefficients, three batches: 0.70 ms at 32, 0.46 at 16, 0.36 at 8)
#ifndef FRI_SEG
#define FRI_SEG 8
#endif
struct seg_batches {
    uint32_t nb;
    const gl_t* a0[FRI_MAX_BATCHES];   // this level's arrays of every batch (level 0: the composite polynomials)
    const gl_t* a1[FRI_MAX_BATCHES];
    // Stacked proofs (blockIdx.z = segment): every array of segment s starts a_seg words after segment s - 1's, and the points / weights
    // are per segment: zw[(s * nb + b) * 2] = z_b^(FRI_SEG^level), [.. + 1] = weight of the batch in the final sum
    size_t a_seg;
    const gl2_t* zw;
};
__device__ __forceinline__ gl2_t seg_point(const seg_batches& p, unsigned b) { return p.zw[((size_t)blockIdx.z * p.nb + b) * 2]; }
__device__ __forceinline__ gl2_t seg_weight(const seg_batches& p, unsigned b) { return p.zw[((size_t)blockIdx.z * p.nb + b) * 2 + 1]; }
// A thread's segment is FRI_SEG consecutive words of each array, and the walk over it is a dependent chain: with one 8-byte load per
// step the lanes of a wave sit 256 B apart and every step fetched a whole line from HBM for 8 bytes of it (config 4: 6.4 GB of traffic
// for 0.27 GB of data, profiles/r04_e).  All three kernels therefore work on LDS TILES: the 64 segments of a 64-thread workgroup
// (64 x FRI_SEG consecutive words) are loaded with lane-contiguous accesses into rows of FRI_SEG + 1 words (a thread walking its own row is
// bank-conflict free), results that are arrays over k go back the same way.  Words past the end of the array read as zero -- the
// carry into the last segment is zero, so the chain stays zero there.
#define SEG_TILE (64 * FRI_SEG)
#define SEG_ROW (FRI_SEG + 1)
// (a wave's own LDS accesses execute in order: a wave that reads back what only IT wrote needs no workgroup barrier)
#define ZKM_WAVE_SYNC_LDS()                                  \
    do {                                                     \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); \
        __builtin_amdgcn_wave_barrier();                     \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); \
    } while (0)
__device__ __forceinline__ void seg_tile_load(gl_t* __restrict__ t, const gl_t* __restrict__ a, size_t base, size_t m) {
    for (unsigned e = threadIdx.x; e < SEG_TILE; e += 64) {
        const size_t k = base + e;
        t[(e / FRI_SEG) * SEG_ROW + e % FRI_SEG] = k < m ? a[k] : 0;
    }
}
// totals:  out_b[s] = sum_{k<FRI_SEG} a_b[FRI_SEG s + k] z_b^k          (out: [batch][2][nseg])
__global__ __launch_bounds__(64) void k_seg_totals(seg_batches p, size_t m, gl_t* __restrict__ out) {
    __shared__ gl_t t0[64 * SEG_ROW], t1[64 * SEG_ROW];
    const size_t s = (size_t)blockIdx.x * 64 + threadIdx.x, nseg = (m + FRI_SEG - 1) / FRI_SEG;
    const unsigned b = blockIdx.y;
    seg_tile_load(t0, p.a0[b] + (size_t)blockIdx.z * p.a_seg, (size_t)blockIdx.x * SEG_TILE, m);
    seg_tile_load(t1, p.a1[b] + (size_t)blockIdx.z * p.a_seg, (size_t)blockIdx.x * SEG_TILE, m);
    __syncthreads();
    if (s >= nseg) return;
    out += (size_t)blockIdx.z * 2 * gridDim.y * nseg;
    const gl2_t z = seg_point(p, b);
    gl2_t acc{0, 0};
    const gl_t *r0 = t0 + threadIdx.x * SEG_ROW, *r1 = t1 + threadIdx.x * SEG_ROW;
    for (unsigned k = FRI_SEG; k-- > 0;) acc = gl2_add(gl2_mul(acc, z), gl2_t{r0[k], r1[k]});
    out[(2 * b) * nseg + s] = acc.c0;
    out[(2 * b + 1) * nseg + s] = acc.c1;
}
// scan of a level:  S_b[k] = a_b[k] + z_b S_b[k+1] inside each segment, carry-in = upper_b[s+1] (0 past the end)
// (upper: [batch][2][nupper] suffix values of the level above, or null at the top; out: [batch][2][m])
__global__ __launch_bounds__(64) void k_seg_scan(seg_batches p, size_t m, const gl_t* __restrict__ upper, size_t nupper, gl_t* __restrict__ out) {
    __shared__ gl_t t0[64 * SEG_ROW], t1[64 * SEG_ROW];
    const size_t s = (size_t)blockIdx.x * 64 + threadIdx.x, base = (size_t)blockIdx.x * SEG_TILE;
    const unsigned b = blockIdx.y;
    seg_tile_load(t0, p.a0[b] + (size_t)blockIdx.z * p.a_seg, base, m);
    seg_tile_load(t1, p.a1[b] + (size_t)blockIdx.z * p.a_seg, base, m);
    __syncthreads();
    if (upper) upper += (size_t)blockIdx.z * 2 * gridDim.y * nupper;
    out += (size_t)blockIdx.z * 2 * gridDim.y * m;
    {
        const gl2_t z = seg_point(p, b);
        gl2_t acc{0, 0};
        if (upper && s + 1 < nupper) acc = gl2_t{upper[(2 * b) * nupper + s + 1], upper[(2 * b + 1) * nupper + s + 1]};
        gl_t *r0 = t0 + threadIdx.x * SEG_ROW, *r1 = t1 + threadIdx.x * SEG_ROW;
        for (unsigned k = FRI_SEG; k-- > 0;) {                 // (a segment past the end: zeros in, zero carry, zeros out -- never stored)
            acc = gl2_add(gl2_mul(acc, z), gl2_t{r0[k], r1[k]});
            r0[k] = acc.c0;
            r1[k] = acc.c1;
        }
    }
    __syncthreads();
    for (unsigned e = threadIdx.x; e < SEG_TILE; e += 64) {
        const size_t k = base + e;
        if (k < m) {
            out[(2 * b) * m + k] = t0[(e / FRI_SEG) * SEG_ROW + e % FRI_SEG];
            out[(2 * b + 1) * m + k] = t1[(e / FRI_SEG) * SEG_ROW + e % FRI_SEG];
        }
    }
}
// bottom level of LONG polynomials (>= 2^21 coefficients: enough segments to fill the machine, and the suffix values of every batch
// would be 6 n words written and read again): all batches in one workgroup, one after the other through the same input tile, with
// fin[k - 1] = sum_b w_b S_b[k] accumulated in an output tile
__global__ __launch_bounds__(64) void k_seg_scan_final(seg_batches p, size_t m, const gl_t* __restrict__ upper, size_t nupper, gl_t* __restrict__ f0,
                                                       gl_t* __restrict__ f1) {
    extern __shared__ __attribute__((aligned(16))) gl_t seg_lds[];   // four tiles of 64 rows x (FRI_SEG + 1) words: 18 KB at FRI_SEG = 8 (the dynamic-LDS limit is only raised for builds with longer segments)
    gl_t *const t0 = seg_lds, *const t1 = t0 + 64 * SEG_ROW, *const g0 = t1 + 64 * SEG_ROW, *const g1 = g0 + 64 * SEG_ROW;
    const size_t s = (size_t)blockIdx.x * 64 + threadIdx.x, base = (size_t)blockIdx.x * SEG_TILE;
    gl_t *r0 = t0 + threadIdx.x * SEG_ROW, *r1 = t1 + threadIdx.x * SEG_ROW, *q0 = g0 + threadIdx.x * SEG_ROW, *q1 = g1 + threadIdx.x * SEG_ROW;
    if (upper) upper += (size_t)blockIdx.z * 2 * p.nb * nupper;
    f0 += (size_t)blockIdx.z * 2 * m;
    f1 += (size_t)blockIdx.z * 2 * m;
    for (unsigned b = 0; b < p.nb; b++) {
        if (b) __syncthreads();                                // everyone is done with the previous batch's tile
        seg_tile_load(t0, p.a0[b] + (size_t)blockIdx.z * p.a_seg, base, m);
        seg_tile_load(t1, p.a1[b] + (size_t)blockIdx.z * p.a_seg, base, m);
        __syncthreads();
        const gl2_t z = seg_point(p, b), w = seg_weight(p, b);
        gl2_t acc{0, 0};
        if (upper && s + 1 < nupper) acc = gl2_t{upper[(2 * b) * nupper + s + 1], upper[(2 * b + 1) * nupper + s + 1]};
        for (unsigned k = FRI_SEG; k-- > 0;) {
            acc = gl2_add(gl2_mul(acc, z), gl2_t{r0[k], r1[k]});
            gl2_t f = gl2_mul(acc, w);
            if (b) f = gl2_add(f, gl2_t{q0[k], q1[k]});
            q0[k] = f.c0;
            q1[k] = f.c1;
        }
    }
    __syncthreads();
    for (unsigned e = threadIdx.x; e < SEG_TILE; e += 64) {   // word k of the tile is fin[k - 1]
        const size_t k = base + e;
        if (k > 0 && k < m) {
            f0[k - 1] = g0[(e / FRI_SEG) * SEG_ROW + e % FRI_SEG];
            f1[k - 1] = g1[(e / FRI_SEG) * SEG_ROW + e % FRI_SEG];
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { f0[m - 1] = 0; f1[m - 1] = 0; }
}
// Bottom level, scan and weighted sum in ONE launch (round 5): wave b of the workgroup scans batch b's 64 segments into its own LDS
// tile (the same 8-step chains as k_seg_scan, the batches side by side instead of one after the other as in k_seg_scan_final), then
// all waves add the tiles up: fin[k - 1] = sum_b w_b S_b[k].  The suffix values of the bottom level never go to HBM: the division
// reads the composites twice (totals, then here) and writes fin once -- 1.75x its algorithmic bytes instead of 3.9x (k_seg_scan writing
// 6 n words that k_seg_combine read again).  Field sums are exact, so the words are those of k_seg_scan + k_seg_combine.
__global__ __launch_bounds__(512) void k_seg_scan_combine(seg_batches p, size_t m, const gl_t* __restrict__ upper, size_t nupper, gl_t* __restrict__ f0,
                                                          gl_t* __restrict__ f1) {
    extern __shared__ __attribute__((aligned(16))) gl_t sc_lds[];        // [batch][2][64 * SEG_ROW]
    const unsigned b = threadIdx.x >> 6, lane = threadIdx.x & 63;
    gl_t *const t0 = sc_lds + (size_t)(2 * b) * 64 * SEG_ROW, *const t1 = t0 + 64 * SEG_ROW;
    const size_t s = (size_t)blockIdx.x * 64 + lane, base = (size_t)blockIdx.x * SEG_TILE;
    {
        const gl_t* a0 = p.a0[b] + (size_t)blockIdx.z * p.a_seg;
        const gl_t* a1 = p.a1[b] + (size_t)blockIdx.z * p.a_seg;
        for (unsigned e = lane; e < SEG_TILE; e += 64) {
            const size_t k = base + e;
            const unsigned at = (e / FRI_SEG) * SEG_ROW + e % FRI_SEG;
            t0[at] = k < m ? a0[k] : 0;
            t1[at] = k < m ? a1[k] : 0;
        }
    }
    ZKM_WAVE_SYNC_LDS();
    {
        if (upper) upper += (size_t)blockIdx.z * 2 * p.nb * nupper;
        const gl2_t z = seg_point(p, b);
        gl2_t acc{0, 0};
        if (upper && s + 1 < nupper) acc = gl2_t{upper[(2 * b) * nupper + s + 1], upper[(2 * b + 1) * nupper + s + 1]};
        gl_t *r0 = t0 + lane * SEG_ROW, *r1 = t1 + lane * SEG_ROW;
        const gl2_t w = seg_weight(p, b);
        for (unsigned k = FRI_SEG; k-- > 0;) {
            acc = gl2_add(gl2_mul(acc, z), gl2_t{r0[k], r1[k]});
            const gl2_t f = gl2_mul(acc, w);                   // (the weight goes in here: the sum below is plain additions)
            r0[k] = f.c0;
            r1[k] = f.c1;
        }
    }
    __syncthreads();
    f0 += (size_t)blockIdx.z * 2 * m;
    f1 += (size_t)blockIdx.z * 2 * m;
    for (unsigned e = threadIdx.x; e < SEG_TILE; e += blockDim.x) {       // word k of the tiles is fin[k - 1]
        const size_t k = base + e;
        if (k > 0 && k < m) {
            const unsigned at = (e / FRI_SEG) * SEG_ROW + e % FRI_SEG;
            gl_t x0 = 0, x1 = 0;
            for (unsigned q = 0; q < p.nb; q++) {
                x0 = gl_add(x0, sc_lds[(size_t)(2 * q) * 64 * SEG_ROW + at]);
                x1 = gl_add(x1, sc_lds[(size_t)(2 * q + 1) * 64 * SEG_ROW + at]);
            }
            f0[k - 1] = x0;
            f1[k - 1] = x1;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { f0[m - 1] = 0; f1[m - 1] = 0; }
}
// fin[k - 1] = sum_b w_b S_b[k] (the dropped remainders are the S_b[0]), fin[m - 1] = 0      (suf: [batch][2][m], bottom level)
__global__ __launch_bounds__(256) void k_seg_combine(seg_batches p, size_t m, const gl_t* __restrict__ suf, gl_t* __restrict__ f0,
                                                     gl_t* __restrict__ f1) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    suf += (size_t)blockIdx.z * 2 * p.nb * m;
    f0 += (size_t)blockIdx.z * 2 * m;
    f1 += (size_t)blockIdx.z * 2 * m;
    gl2_t f{0, 0};
    if (i + 1 < m)
        for (unsigned b = 0; b < p.nb; b++) f = gl2_add(f, gl2_mul(gl2_t{suf[(2 * b) * m + i + 1], suf[(2 * b + 1) * m + i + 1]}, seg_weight(p, b)));
    f0[i] = f.c0;
    f1[i] = f.c1;
}

// ------------------------------------------------------------------ K13: FRI fold
// c'_j = sum_{i < arity} beta^i c_{arity j + i}   (reduce_with_powers per chunk)
// A thread's 16 coefficients are one 128-byte line of each array: read with one 8-byte load per step they were fetched from HBM again
// and again (lanes 128 B apart, the lines evicted between steps: 850 MB of traffic for 76 MB of data in config 4, profiles/r04_e).  The
// workgroup's 64 x arity coefficients therefore come in with lane-contiguous loads into an LDS tile (row stride arity + 1: the walk
// over one's own row is bank-conflict free) and are read from there.
// (tile rows of arity + 1 words in dynamic LDS: any arity_bits the config check admits, 2 .. 6 -- ADVICE r04)
// (blockIdx.z = segment of a stack: its own beta; its arrays [2][total] in, [2][nout] out follow the previous segment's)
__global__ __launch_bounds__(64) void k_fri_fold(const gl_t* __restrict__ c0, const gl_t* __restrict__ c1, size_t nout, unsigned arity,
                                                 seg_gl2 betas, gl_t* __restrict__ o0, gl_t* __restrict__ o1) {
    extern __shared__ __attribute__((aligned(16))) gl_t fold_lds[];   // two tiles of 64 rows of arity + 1 words
    gl_t *const t0 = fold_lds, *const t1 = fold_lds + 64 * (arity + 1);
    const gl2_t beta{betas.v[2 * blockIdx.z], betas.v[2 * blockIdx.z + 1]};
    const size_t j0 = (size_t)blockIdx.x * 64, total = nout * arity, base = j0 * arity;
    c0 += (size_t)blockIdx.z * 2 * total; c1 += (size_t)blockIdx.z * 2 * total;
    o0 += (size_t)blockIdx.z * 2 * nout; o1 += (size_t)blockIdx.z * 2 * nout;
    const unsigned tid = threadIdx.x, rs = arity + 1;
    for (unsigned e = tid; e < 64 * arity; e += 64) {
        const size_t k = base + e;
        const unsigned at = (e / arity) * rs + e % arity;
        t0[at] = k < total ? c0[k] : 0;
        t1[at] = k < total ? c1[k] : 0;
    }
    __syncthreads();
    const size_t j = j0 + tid;
    if (j >= nout) return;
    gl2_t acc{0, 0};
    for (unsigned i = arity; i-- > 0;) acc = gl2_add(gl2_mul(acc, beta), gl2_t{t0[tid * rs + i], t1[tid * rs + i]});
    o0[j] = acc.c0;
    o1[j] = acc.c1;
}

// ------------------------------------------------------------------ K14: proof of work
// Smallest candidate w such that Poseidon(state with w written at `pos`)[7] has >= pow_bits leading zeros.  One launch: thread t tries
// base + t, base + t + stride, ... below `limit` and stops as soon as a smaller hit is known (device-scope atomic on `best`), so a
// launch costs about one permutation's latency per 2^pow_bits / stride-th of the expected number of trials -- no host round trip
// between the rounds, no candidates tried beyond the round of the first hit.
struct pow_state { uint64_t s[12]; };
// The launch delivers its result ITSELF: the workgroup that finishes last (a ticket) writes `best` into pinned host memory, then the
// sequence number the host polls for, and leaves `best` = all ones and the ticket counter = 0 for the next search -- no memset launch in
// front, no download launch behind (two launches and their gaps per table proof).
// Stacked searches (blockIdx.y = segment): sts[s] = segment s's transcript state (device array), pos.v[s] the word its candidate goes
// to, best[s] / host_out[s] its result; a segment whose witness is already known (done.v[s] != 0: found by an earlier launch) is skipped.
struct seg_u32 { uint32_t v[ZKM_MAX_SEG]; };
__global__ __launch_bounds__(256) void k_pow_search(const pow_state* __restrict__ sts, seg_u32 pos_v, seg_u32 done, unsigned pow_bits, uint64_t base,
                                                    uint64_t limit, unsigned long long* best, unsigned* counter, uint64_t* host_out, uint64_t* flag,
                                                    uint64_t seq) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const unsigned pos = pos_v.v[blockIdx.y];
    best += blockIdx.y;
    if (done.v[blockIdx.y]) limit = 0;
    pow_state st;
#pragma unroll
    for (int i = 0; i < 12; i++) st.s[i] = sts[blockIdx.y].s[i];
#pragma unroll 1
    for (uint64_t w = base + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < limit; w += stride) {
        if (w > __hip_atomic_load(best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
        uint64_t s[12];
#pragma unroll
        for (int i = 0; i < 12; i++) s[i] = st.s[i];
#pragma unroll
        for (int i = 0; i < 8; i++)
            if ((unsigned)i == pos) s[i] = w;
        poseidon_permute(s);
        if ((s[7] >> (64 - pow_bits)) == 0) atomicMin(best, (unsigned long long)w);
    }
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned ticket = atomicAdd(counter, 1u);
        if (ticket == gridDim.x * gridDim.y - 1) {
            __threadfence();
            best -= blockIdx.y;
            for (unsigned sg = 0; sg < gridDim.y; sg++) {
                host_out[sg] = __hip_atomic_load(best + sg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(best + sg, ~0ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            *counter = 0;
            __threadfence_system();
            __hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// ------------------------------------------------------------------ query gather
// Everything the gather needs travels in the kernel-argument segment (no descriptor / index uploads per table): level l of a tree
// with 2^log_leaves leaf digests starts at word 4 (2^(log_leaves + 1) - 2^(log_leaves - l + 1)) of its digest array
// (zkm_merkle_layout), and the query indices are at most ZKM_FRI_MAX_QUERIES words.
// (stacked proofs, blockIdx.y = segment s: its matrix / values and its digests start s * lde_seg / val_seg and s * dig_seg words further)
struct gather_oracle { const gl_t *lde, *digests; size_t lde_seg, dig_seg; };
struct gather_layer { const gl_t *c0, *c1, *digests; size_t val_seg, dig_seg; };
#define ZKM_FRI_MAX_QUERIES 128
struct gather_args {
    gather_oracle o[ZKM_FRI_MAX_ORACLES];
    gather_layer l[ZKM_FRI_GATHER_LAYERS];
    zkm_query_round round;   // where each piece goes
};
__device__ __forceinline__ size_t merkle_level_offset(unsigned log_leaves, unsigned lvl) {
    return (((size_t)2 << log_leaves) - ((size_t)2 << (log_leaves - lvl))) * 4;
}
__global__ void k_gather_queries(gather_args g, const uint32_t* __restrict__ qs /* [segment][queries] */, gl_t* __restrict__ out) {
    const zkm_query_round& R = g.round;
    const size_t sg = blockIdx.y;
    uint64_t x = qs[sg * gridDim.x + blockIdx.x];
    const uint32_t lde_bits = (uint32_t)R.lde_bits, arity_bits = (uint32_t)R.arity_bits;
    const uint64_t N = (uint64_t)1 << lde_bits;
    gl_t* round = out + (sg * gridDim.x + blockIdx.x) * R.words();
    for (uint32_t k = 0; k < (uint32_t)R.noracles; k++) {
        const gl_t *lde = g.o[k].lde + sg * g.o[k].lde_seg, *dig = g.o[k].digests + sg * g.o[k].dig_seg;
        gl_t *ev = round + R.oracle_evals(k), *sib = round + R.oracle_siblings(k);
        for (uint32_t c = threadIdx.x; c < (uint32_t)R.cols[k]; c += blockDim.x) ev[c] = lde[(size_t)c * N + x];
        for (uint32_t e = threadIdx.x; e < (uint32_t)R.initial_siblings() * 4; e += blockDim.x) {
            uint32_t lvl = e >> 2;
            sib[e] = dig[merkle_level_offset(lde_bits, lvl) + 4 * ((x >> lvl) ^ 1) + (e & 3)];
        }
    }
    uint32_t arity = 1u << arity_bits;
    for (uint32_t l = 0; l < (uint32_t)R.L; l++) {
        const gather_layer& r = g.l[l];
        const gl_t *c0 = r.c0 + sg * r.val_seg, *c1 = r.c1 + sg * r.val_seg, *dig = r.digests + sg * r.dig_seg;
        const uint32_t nsib = (uint32_t)R.layer_sibling_count(l);
        gl_t *ev = round + R.layer_evals(l), *sib = round + R.layer_siblings(l);
        x >>= arity_bits;
        for (uint32_t e = threadIdx.x; e < 2 * arity; e += blockDim.x) ev[e] = (e & 1) ? c1[x * arity + (e >> 1)] : c0[x * arity + (e >> 1)];
        for (uint32_t e = threadIdx.x; e < nsib * 4; e += blockDim.x) {
            uint32_t lvl = e >> 2;
            sib[e] = dig[merkle_level_offset(nsib + (uint32_t)R.cap_height, lvl) + 4 * ((x >> lvl) ^ 1) + (e & 3)];
        }
    }
}

// ------------------------------------------------------------------ host helpers

// ------------------------------------------------------------------ FRI: everything after the alpha-combination
// One composite polynomial per FriBatchInfo (coefficients, F2 as two arrays), its opening point and the factor alpha^(#polys of
// the batch) of ReducingFactor::shift_poly.  fri_finish divides each by (X - point), accumulates the final
// polynomial, runs the commit phase (LDE, Merkle tree, cap -> transcript, beta, fold), the proof of work and the query rounds over
// `noracles` initial oracles.  Shared by prove_single_table (the STARK instance of stark.rs:91-148) and zkm_fri_prove (any instance).
struct fri_composite {
    const gl_t *c0, *c1;
    gl2_t point, shift;
};

// fin = sum over the batches (in order) of: fin * shift_b + (comp_b(X) - comp_b(z_b)) / (X - z_b), re-padded to n coefficients.
// fin is written completely (no zero-fill needed).  Stacked: comps[s] = segment s's composites (pointers: segment 0's, the others'
// comp_seg words further per segment), fin of segment s at f0 / f1 + s * 2 n.
static void divide_accumulate_all(zkm_ctx* c, const std::vector<std::vector<fri_composite>>& comps, size_t comp_seg, size_t n, gl_t* f0, gl_t* f1) {
    const size_t nseg = comps.size();
    if (nseg == 0 || nseg > ZKM_MAX_SEG) throw std::runtime_error("FRI: bad stack size");
    const unsigned nb = (unsigned)comps[0].size(), z = (unsigned)nseg;
    if (nb == 0 || nb > FRI_MAX_BATCHES) throw std::runtime_error("FRI: 1..8 opening batches");
    for (const auto& k : comps)
        if (k.size() != nb) throw std::runtime_error("internal: FRI instances of a stack differ");
    zkm_prof_scope ps(c, "fri_divide_linear");
    // level sizes: n, ceil(n / FRI_SEG), ... down to <= FRI_SEG
    std::vector<size_t> m{n};
    while (m.back() > FRI_SEG) m.push_back((m.back() + FRI_SEG - 1) / FRI_SEG);
    const size_t L = m.size();
    std::vector<seg_batches> lv(L);
    zkm_scratch_list tmp(c);
    // points and weights of every level and segment: zw[l][s][b] = (z_b^(FRI_SEG^l), w_b), w_b = product of the shifts of the batches after b
    const size_t per_level = nseg * nb * 2;
    std::vector<gl2_t> zw(L * per_level);
    for (size_t sg = 0; sg < nseg; sg++) {
        gl2_t wacc{1, 0};
        for (unsigned b = nb; b-- > 0;) {
            gl2_t zp = comps[sg][b].point;
            for (size_t l = 0; l < L; l++) {
                zw[l * per_level + (sg * nb + b) * 2] = zp;
                zw[l * per_level + (sg * nb + b) * 2 + 1] = wacc;
                zp = gl2_pow(zp, FRI_SEG);
            }
            wacc = gl2_mul(wacc, comps[sg][b].shift);
        }
    }
    gl2_t* d_zw = tmp.alloc<gl2_t>(zw.size() * sizeof(gl2_t));
    c->upload(d_zw, zw.data(), zw.size() * sizeof(gl2_t));
    for (unsigned b = 0; b < nb; b++) { lv[0].a0[b] = comps[0][b].c0; lv[0].a1[b] = comps[0][b].c1; }
    lv[0].nb = nb;
    lv[0].a_seg = comp_seg;
    lv[0].zw = d_zw;
    for (size_t l = 1; l < L; l++) {
        gl_t* const tot = tmp.alloc<gl_t>(nseg * 2 * nb * m[l] * sizeof(gl_t));   // [segment][nb][2][m[l]]: the totals that feed level l
        hipLaunchKernelGGL(k_seg_totals, dim3((unsigned)((m[l] + 63) / 64), nb, z), dim3(64), 0, c->stream, lv[l - 1], m[l - 1], tot);
        lv[l] = lv[0];
        for (unsigned b = 0; b < nb; b++) {
            lv[l].a0[b] = tot + (2 * b) * m[l];
            lv[l].a1[b] = tot + (2 * b + 1) * m[l];
        }
        lv[l].a_seg = 2 * nb * m[l];
        lv[l].zw = d_zw + l * per_level;
    }
    // top-down: suffix values of each level, then the weighted sum of the bottom level's
    const gl_t* upper = nullptr;   // the suffix values of the level above
    for (size_t l = L; l-- > 0;) {
        const size_t nsegm = (m[l] + FRI_SEG - 1) / FRI_SEG;
        const size_t nupper = l + 1 < L ? m[l + 1] : 0;
        if (l == 0 && (n >= c->fri_fused_division_min || c->fri_scan_combine)) {
            // bottom level in one launch (no suffix arrays in HBM): k_seg_scan_final from fri_fused_division_min coefficients on -- four tiles;
            // else k_seg_scan_combine -- scan + weighted sum, two tiles per batch: 9,216 B per batch with segments of 8, eight batches
            // (FRI_MAX_BATCHES) are 73,728 B, over the 64 KB a launch gets without asking.  The limit is raised once per
            // device like k_fri_fold's (k_seg_scan_final: only a build with longer segments needs that -- ADVICE r04)
            const bool fused = n >= c->fri_fused_division_min;
            auto* const kernel = fused ? k_seg_scan_final : k_seg_scan_combine;
            const size_t lds = (fused ? 4 : 2 * (size_t)nb) * 64 * SEG_ROW * sizeof(gl_t);
            static std::atomic<uint64_t> lds_ok[2];
            if (lds > 64 * 1024) ZKM_HIP_CHECK(zkm_allow_big_lds(c, (const void*)kernel, lds_ok[fused]));
            hipLaunchKernelGGL(kernel, dim3((unsigned)((nsegm + 63) / 64), 1, z), dim3(fused ? 64 : 64 * nb), lds, c->stream, lv[0], n, upper, nupper, f0, f1);
            break;
        }
        gl_t* const suf = tmp.alloc<gl_t>(nseg * 2 * nb * m[l] * sizeof(gl_t));
        hipLaunchKernelGGL(k_seg_scan, dim3((unsigned)((nsegm + 63) / 64), nb, z), dim3(64), 0, c->stream, lv[l], m[l], upper, nupper, suf);
        if (l == 0) hipLaunchKernelGGL(k_seg_combine, dim3((unsigned)((n + 255) / 256), 1, z), dim3(256), 0, c->stream, lv[0], n, suf, f0, f1);
        upper = suf;
    }
    ZKM_HIP_CHECK(hipGetLastError());
}   // (`tmp` goes back without a host sync: released blocks are only reused by later work on this stream)

// A STACK of nseg = chs.size() independent proofs of the same shape in flight (one proof: vectors of length 1): chs[s] = proof s's
// transcript, blobs[s] its blob.  Every stage below is ONE launch (or group of launches) for all proofs, and every transcript round
// trip brings the words of all of them down together.
struct proof_stack {
    zkm_ctx* c;
    const zkm_stark_config* cfg;
    unsigned log_n;
    const std::vector<zkm_challenger*>& chs;
    const std::vector<uint64_t*>& blobs;
    zkm_scratch_list scratch{c};
    size_t nseg() const { return chs.size(); }
    size_t n() const { return (size_t)1 << log_n; }
};

// ------------------------------------------------------------------ FRI: everything after the alpha-combination, in four stages; the
// blobs' FRI fields lie where `part` says.  Shared by the STARK instance (prove_openings below, stark.rs:91-148) and zkm_fri_prove.
// commit phase: LDE, Merkle tree, cap -> transcript, beta, fold, layer after layer; then the final polynomial.  d_coef: the
// coefficients of the current layer, first d_fin (length clen, implicitly zero-padded x4)
static std::vector<gather_layer> fri_commit_phase(proof_stack& f, const zkm_fri_part& part, gl_t* d_coef /* [segment][2][clen]: c0 array, then c1 */) {
    zkm_ctx* const c = f.c;
    const zkm_stark_config* const cfg = f.cfg;
    const size_t nseg = f.nseg(), C4 = part.cap_words;
    const unsigned z = (unsigned)nseg, arity = 1u << cfg->arity_bits;
    std::vector<gather_layer> layers;
    size_t clen = (size_t)1 << f.log_n;
    unsigned clog = f.log_n;
    gl_t shift = GL_GENERATOR;
    std::vector<uint64_t> capbuf(nseg * C4);
    std::vector<size_t> level_off;
    for (unsigned l = 0; l < part.round.L; l++) {
        const size_t len = clen << cfg->rate_bits;
        gl_t* const values = f.scratch.alloc<gl_t>(nseg * 2 * len * sizeof(gl_t));
        // values = coset_fft(shift) of the zero-padded coefficients, bit-reversed: two base-field columns per proof
        // (the coefficient arrays are contiguous: [c0 | c1] per proof, column stride clen)
        zkm_lde_bitrev(c, d_coef, values, 2 * nseg, clog, cfg->rate_bits, shift);
        const unsigned log_leaves = clog + cfg->rate_bits - cfg->arity_bits;
        const size_t dwords = zkm_merkle_layout(log_leaves, cfg->cap_height, level_off);
        gl_t* const digests = f.scratch.alloc<gl_t>(nseg * dwords * sizeof(gl_t));
        layers.push_back(gather_layer{values, values + len, digests, 2 * len, dwords});   // ([segment][2][len] values, bit-reversed)
        zkm_launch_merkle_leaves_ext(c, values, values + len, (size_t)1 << log_leaves, arity, digests, nseg, 2 * len, dwords);
        zkm_merkle_build_inner_cap(c, digests, level_off, log_leaves, cfg->cap_height, capbuf.data(), nseg, dwords);
        seg_gl2 betas{};
        for (size_t sg = 0; sg < nseg; sg++) {
            uint64_t* capo = f.blobs[sg] + part.o_cap(l);
            memcpy(capo, capbuf.data() + sg * C4, C4 * sizeof(uint64_t));
            gl2_t beta = zkm_transcript_fri_beta(f.chs[sg], capo, C4);
            betas.v[2 * sg] = beta.c0; betas.v[2 * sg + 1] = beta.c1;
        }
        size_t nout = clen >> cfg->arity_bits;
        gl_t* d_new = f.scratch.alloc<gl_t>(nseg * 2 * nout * sizeof(gl_t));
        {
            zkm_prof_scope ps(c, "fri_fold");
            const size_t lds = 2 * 64 * ((size_t)arity + 1) * sizeof(gl_t);
            static std::atomic<uint64_t> lds_ok{0};
            if (lds > 64 * 1024) ZKM_HIP_CHECK(zkm_allow_big_lds(c, (const void*)k_fri_fold, lds_ok));
            hipLaunchKernelGGL(k_fri_fold, dim3((unsigned)((nout + 63) / 64), 1, z), dim3(64), lds, c->stream, d_coef, d_coef + clen, nout, arity, betas,
                               d_new, d_new + nout);
            ZKM_HIP_CHECK(hipGetLastError());
        }
        d_coef = d_new;
        clen = nout;
        clog -= cfg->arity_bits;
        shift = gl_pow(shift, arity);
    }
    if (clen != part.F) throw std::runtime_error("internal: final polynomial length mismatch");
    std::vector<gl_t> fin(nseg * 2 * clen);
    c->download(fin.data(), d_coef, nseg * 2 * clen * 8);
    for (size_t sg = 0; sg < nseg; sg++) {
        uint64_t* fp = f.blobs[sg] + part.o_final();
        const gl_t* fs = fin.data() + sg * 2 * clen;
        for (size_t i = 0; i < clen; i++) { fp[2 * i] = fs[i]; fp[2 * i + 1] = fs[clen + i]; }
        zkm_transcript_final_poly(f.chs[sg], fp, clen);
    }
    return layers;
}

// proof of work (App. A.9), smallest witness of every proof
static void fri_proof_of_work(proof_stack& f, const zkm_fri_part& part) {
    zkm_ctx* const c = f.c;
    const size_t nseg = f.nseg();
    std::vector<pow_state> sts(nseg);
    seg_u32 pos{}, done{};
    for (size_t sg = 0; sg < nseg; sg++) {
        memcpy(sts[sg].s, f.chs[sg]->state, sizeof sts[sg].s);
        for (uint32_t i = 0; i < f.chs[sg]->n_in; i++) sts[sg].s[i] = f.chs[sg]->in_buf[i];
        pos.v[sg] = f.chs[sg]->n_in;
    }
    pow_state* d_sts = f.scratch.alloc<pow_state>(nseg * sizeof(pow_state));
    c->upload(d_sts, sts.data(), nseg * sizeof(pow_state));
    unsigned long long* d_best = c->pow_best();      // ZKM_MAX_SEG words, all ones between searches (the kernel leaves them that way)
    std::vector<unsigned long long> best(nseg, ~0ULL), got(nseg);
    // 2^pow_round_log candidates per round and proof (17 for a proof alone: two waves per SIMD -- a wave alone issues at half the
    // SIMD's rate, so the round is barely longer than with one, and it holds the hit with probability 0.86 instead of 0.63 at 16
    // bits; the searches of a stack share the machine: the round of each shrinks with their number, down to 2^12, so that the
    // stack's round is still one launch-filling set of waves and few candidates are tried beyond the round of a proof's first hit),
    // up to 2^6 rounds per launch (a launch without a hit: probability e^-128 for a proof alone)
    unsigned round_log = c->pow_round_log;
    for (size_t k = 1; k < nseg && round_log > 12; k <<= 1) round_log--;
    const uint64_t stride = (uint64_t)1 << round_log, span = stride << 6;
    size_t open = nseg;
    for (uint64_t base = 0; open; base += span) {
        if (base > ((uint64_t)1 << 40)) throw std::runtime_error("Proof of work failed. This is highly unlikely!");
        uint64_t *host_slot, *flag;
        unsigned* counter;
        const uint64_t seq = c->xfer_begin(8 * nseg, &host_slot, &flag, &counter);
        {
            zkm_prof_scope ps(c, "fri_pow_search");
            hipLaunchKernelGGL(k_pow_search, dim3(stride / 256, (unsigned)nseg), dim3(256), 0, c->stream, d_sts, pos, done, f.cfg->pow_bits, base, base + span,
                               d_best, counter, host_slot, flag, seq);
            ZKM_HIP_CHECK(hipGetLastError());
        }
        c->xfer_finish(seq, got.data(), 8 * nseg);
        for (size_t sg = 0; sg < nseg; sg++)
            if (!done.v[sg] && got[sg] != ~0ULL) { best[sg] = got[sg]; done.v[sg] = 1; open--; }
    }
    for (size_t sg = 0; sg < nseg; sg++) {
        f.blobs[sg][part.o_pow()] = best[sg];
        if (!zkm_transcript_pow(f.chs[sg], best[sg], f.cfg->pow_bits)) throw std::runtime_error("internal: proof-of-work response check failed");
    }
}

// query rounds: the indices from the transcripts, one gather over the initial oracles and the layers, one download
static void fri_query_rounds(proof_stack& f, const zkm_fri_part& part, const std::vector<gather_layer>& layers, const zkm_batch* const* orc,
                             size_t noracles) {
    zkm_ctx* const c = f.c;
    const zkm_query_round& round = part.round;
    const size_t nseg = f.nseg(), nq = part.nq;
    const unsigned lde_bits = f.log_n + f.cfg->rate_bits;
    std::vector<uint32_t> qs(nseg * nq);
    for (size_t sg = 0; sg < nseg; sg++) zkm_transcript_query_indices(f.chs[sg], nq, lde_bits, qs.data() + sg * nq);
    uint32_t* d_qs = f.scratch.alloc<uint32_t>(qs.size() * sizeof(uint32_t));
    c->upload(d_qs, qs.data(), qs.size() * sizeof(uint32_t));
    gather_args ga{};
    ga.round = round;
    for (size_t k = 0; k < noracles; k++) ga.o[k] = {orc[k]->lde, orc[k]->digests, orc[k]->lde_seg(), orc[k]->dig_words};
    std::copy(layers.begin(), layers.end(), ga.l);
    const size_t qwords = nq * round.words();
    gl_t* d_q = f.scratch.alloc<gl_t>(nseg * qwords * 8);
    {
        zkm_prof_scope ps(c, "fri_gather_queries");
        hipLaunchKernelGGL(k_gather_queries, dim3(nq, (unsigned)nseg), dim3(256), 0, c->stream, ga, d_qs, d_q);
        ZKM_HIP_CHECK(hipGetLastError());
    }
    if (nseg == 1) {
        c->download(f.blobs[0] + part.o_queries(), d_q, qwords * 8);
    } else {
        std::vector<gl_t> all(nseg * qwords);
        c->download(all.data(), d_q, nseg * qwords * 8);
        for (size_t sg = 0; sg < nseg; sg++) memcpy(f.blobs[sg] + part.o_queries(), all.data() + sg * qwords, qwords * 8);
    }
}

// ---- what the STARK instance and zkm_fri_prove share around their combination kernels
// out[2 j], out[2 j + 1] = alpha^j for j <= np (alpha^np: the shift of a batch of np polynomials)
static void alpha_powers(gl2_t alpha, size_t np, gl_t* out) {
    gl2_t p{1, 0};
    for (size_t j = 0; j <= np; j++) { out[2 * j] = p.c0; out[2 * j + 1] = p.c1; p = gl2_mul(p, alpha); }
}
// From the composites to the finished proofs.  d_comp: [proof][batch][2][n] words as the combination left them, comps[s][b] = the point
// and shift of proof s's batch b (its pointers are filled in here); orc = the stacked initial oracles.  Everything the gather reads by
// index is checked here, before the first launch.
static void fri_finish(proof_stack& f, const zkm_fri_part& part, unsigned coeff_s1, gl_t* d_comp, std::vector<std::vector<fri_composite>> comps,
                       const zkm_batch* const* orc, size_t noracles) {
    const zkm_query_round& round = part.round;
    if (noracles == 0 || noracles > ZKM_FRI_MAX_ORACLES || round.noracles != noracles) throw std::runtime_error("FRI: 1..8 initial oracles");
    if (round.L > ZKM_FRI_GATHER_LAYERS) throw std::runtime_error("too many FRI layers");
    const size_t nseg = comps.size(), n = f.n(), nb = comps.at(0).size();
    if (nseg == 0 || nseg > ZKM_MAX_SEG || f.nseg() != nseg || f.blobs.size() != nseg) throw std::runtime_error("FRI: bad stack size");
    const unsigned lde_bits = f.log_n + f.cfg->rate_bits;
    if (part.nq > ZKM_FRI_MAX_QUERIES || lde_bits > 32) throw std::runtime_error("FRI: at most 128 query rounds on domains of at most 2^32 points");
    for (size_t k = 0; k < noracles; k++)
        if (orc[k]->lde_bits() != lde_bits || orc[k]->nseg != nseg || orc[k]->ncols != round.cols[k])
            throw std::runtime_error("internal: oracle of another shape in the query gather");
    if (coeff_s1) {
        // the combination is position-wise, so the composites come out in the oracles' coefficient layout (a function of the height: the
        // same for every oracle); the division by (X - point) walks exponents in order
        gl_t* d_nat = f.scratch.alloc<gl_t>(nseg * 2 * nb * n * sizeof(gl_t));
        zkm_coeff_layout_convert(f.c, d_comp, n, d_nat, n, 2 * nb * nseg, f.log_n, /*to_natural=*/true);
        d_comp = d_nat;
    }
    for (auto& proof : comps)   // (proof 0's pointers; proof s's are s * 2 nb n words further)
        for (size_t b = 0; b < proof.size(); b++) { proof[b].c0 = d_comp + 2 * b * n; proof[b].c1 = d_comp + (2 * b + 1) * n; }
    gl_t* d_fin = f.scratch.alloc<gl_t>(nseg * 2 * n * sizeof(gl_t));  // final poly coefficients [segment][2][n]
    divide_accumulate_all(f.c, comps, 2 * nb * n, n, d_fin, d_fin + n);
    const std::vector<gather_layer> layers = fri_commit_phase(f, part, d_fin);
    fri_proof_of_work(f, part);
    fri_query_rounds(f, part, layers, orc, noracles);
}

// ------------------------------------------------------------------ prove_single_table (prover.rs:441-641)
// A STACK of nseg = chs.size() independent proofs of one table at one height on its way down the reference's line
//   commit trace -> commit aux -> alphas, quotient, commit quotient -> zeta, openings -> FRI
// (one proof: vectors of length 1).  The oracles are stacked batches (zkm_internal.h) -- the caller's, or built here and then owned
// here; chs[s] / blobs[s] = proof s's transcript and output blob.  Each stage below is one launch (or group of launches) for all
// proofs; the transcripts advance side by side on the host between the round trips.  Three drivers enter the line: from values
// (zkm_prove_single_table[_ctl]), from the trace and auxiliary commitments (zkm_prove_table_from_commitments: zkm_prove_single_tables
// and ctl.hip) and from all three commitments (zkm_prove_openings).
struct table_proof : proof_stack {
    zkm_blob_desc y;
    const zkm_batch *trace = nullptr, *aux = nullptr, *quot = nullptr;
    zkm_batch_ptr own_trace, own_aux, own_quot;   // (members: freed before the base's scratch goes back -- zkm_batch_free waits for the stream)
    std::vector<gl2_t> zeta = std::vector<gl2_t>(chs.size()), zeta_next = zeta;   // one opening point per proof, and g times it
};

// does the batch hold `ncols` polynomials per proof of a stack of `nseg`, at this height and with the config's rate and cap?
static void require_batch(const zkm_batch* b, size_t ncols, unsigned log_n, const zkm_stark_config* cfg, size_t nseg, const char* or_else) {
    if (!b || b->ncols != ncols || b->log_n != log_n || b->rate_bits != cfg->rate_bits || b->cap_height != cfg->cap_height || b->nseg != nseg)
        throw std::runtime_error(or_else);
}
// What the drivers that hold a CTL description check before they touch a blob or a transcript; returns the blobs' description.  The
// table's own lookup helper columns come first among the auxiliary polynomials (prover.rs:467-508): A - A_ctl of them.
static zkm_blob_desc describe_table_proof(int table_id, const zkm_stark_config* cfg, size_t W, unsigned log_n, size_t A_ctl, const zkm_ctl_z* zs, size_t Z,
                                          const uint64_t* lookup_challenges) {
    validate_config(cfg, log_n);  // before zkm_num_lookup_columns reads it; zkm_blob_describe checks again
    const size_t NL = zkm_num_lookup_columns(table_id, cfg);
    if (NL && !lookup_challenges) throw std::runtime_error("this table has lookups: lookup challenges are required");
    const zkm_blob_desc y = zkm_blob_describe(cfg, log_n, W, NL + A_ctl, Z);
    if (y.L > ZKM_FRI_GATHER_LAYERS) throw std::runtime_error("too many FRI layers");
    size_t ctl_helpers = 0;
    for (size_t i = 0; i < Z; i++) ctl_helpers += zs[i].num_helpers;
    if (ctl_helpers + Z != A_ctl || A_ctl == 0) throw std::runtime_error("No CTL? aux column count does not match the CTL description");  // prover.rs:509
    return y;
}
// the device copy of the CTL description (every trace column it names is checked against W)
static void upload_ctl(table_proof& p, ctl_dev_owner& own, const zkm_ctl_table* ctl_table, const zkm_ctl_z* zs, const uint32_t* colset_ids) {
    own.upload(p.c, ctl_table, zs, colset_ids, p.y.Z, false, p.y.W, p.nseg());
    if (ctl_table)
        for (size_t i = 0; i < ctl_table->nterms; i++)
            if (ctl_table->term_col[i] >= p.y.W) throw std::runtime_error("CTL description: trace column index out of range");
}

// the blobs' heads, the transcripts' start (:466) and the trace caps.  (The query rounds -- nine tenths of the blob, 2 MB for the Keccak table -- are
// written in full by the download at the end of fri_finish: zeroing them here was 0.2 ms of host time per segment in front of the
// table's first launch)
static void put_caps(table_proof& p, unsigned tree, const zkm_batch* b) {
    const size_t C4 = p.y.cap_words();
    for (size_t sg = 0; sg < p.nseg(); sg++) memcpy(p.blobs[sg] + p.y.o_cap(tree), b->cap.data() + sg * C4, C4 * 8);
}
static void begin_blobs(table_proof& p) {
    for (size_t sg = 0; sg < p.nseg(); sg++) {
        memset(p.blobs[sg], 0, p.y.fri().o_queries() * sizeof(uint64_t));
        zkm_blob_header_write(p.blobs[sg], p.y);
        zkm_challenger_compact(p.chs[sg], p.blobs[sg] + p.y.o_init());
    }
    put_caps(p, 0, p.trace);
}

// a commitment to values under the reference's stage scope: one matrix, or one per proof of a stack (device matrices are transformed
// where they lie)
static zkm_batch_ptr commit_values(zkm_ctx* c, const zkm_stark_config* cfg, const char* stage, size_t ncols, unsigned log_n, const uint64_t* const* srcs,
                                   size_t nseg) {
    zkm_prof_scope st(c, stage);
    return zkm_batch_commit(c, srcs, nseg, ncols, log_n, cfg->rate_bits, cfg->cap_height, true);
}

// ---- stage: the trace commitment from values (prover.rs:146-163, done by the caller in the reference)
static void commit_trace(table_proof& p, const uint64_t* trace) {
    p.own_trace = commit_values(p.c, p.cfg, "stage/compute trace commitment", p.y.W, p.log_n, &trace, 1);
    p.trace = p.own_trace.get();
}

// ---- stage: the auxiliary commitment (:511-522) from the CTL columns `aux` (host or device), behind the NL helper columns of the
// table's own lookups, which are built here from the trace values
static void commit_aux(table_proof& p, int table_id, const uint64_t* trace, const uint64_t* aux, const uint64_t* lookup_challenges) {
    zkm_ctx* const c = p.c;
    const size_t n = p.n(), W = p.y.W, A = p.y.A, NL = zkm_num_lookup_columns(table_id, p.cfg);
    if (NL) {
        // "compute lookup helper columns" :475-493, then the CTL columns behind them
        zkm_prof_scope st(c, "stage/compute lookup helper columns");
        gl_t* d_all = p.scratch.alloc<gl_t>(A * n * sizeof(gl_t));
        const gl_t* d_trace = trace;
        if (!zkm_is_device_ptr(trace)) {
            gl_t* d = p.scratch.alloc<gl_t>(W * n * sizeof(gl_t));
            c->upload(d, trace, W * n * sizeof(gl_t));
            zkm_launch_canon(c, d, W * n);   // (host words may be any representative; the lookup kernels want canonical ones)
            d_trace = d;
        }
        zkm_table_lookup_columns_device(c, table_id, lookup_challenges, p.cfg->num_challenges, d_trace, n, d_all);
        ZKM_HIP_CHECK(hipMemcpyAsync(d_all + NL * n, aux, (A - NL) * n * sizeof(gl_t), hipMemcpyDefault, c->stream));
        aux = d_all;
    }
    p.own_aux = commit_values(c, p.cfg, "stage/compute auxiliary polynomials commitment", A, p.log_n, &aux, 1);  // :511-522
    p.aux = p.own_aux.get();
}

// ---- stage: auxiliary caps -> alphas (:525-527), the quotient polynomials (:543-559) and their commitment (:576-587)
static void commit_quotient(table_proof& p, int table_id, const ctl_dev_owner& own, const uint64_t* lookup_challenges) {
    zkm_ctx* const c = p.c;
    const size_t nseg = p.nseg(), nch = p.cfg->num_challenges;
    put_caps(p, 1, p.aux);
    std::vector<gl_t> alphas(nseg * nch);
    for (size_t sg = 0; sg < nseg; sg++) zkm_transcript_alphas(p.chs[sg], p.y, p.blobs[sg], p.cfg->num_challenges, alphas.data() + sg * nch);
    gl_t* d_quot = p.scratch.alloc<gl_t>(nseg * nch * 2 * p.n() * sizeof(gl_t));
    {
        zkm_prof_scope st(c, "stage/compute quotient polys");  // :543-559
        quotient_device(c, table_id, p.trace, p.aux, own, lookup_challenges, alphas.data(), nch, d_quot);
    }
    p.own_quot = zkm_batch_new(c, p.y.Q, nseg, p.log_n, p.cfg->rate_bits, p.cfg->cap_height);
    zkm_prof_scope st(c, "stage/compute quotient commitment");  // :576-587
    zkm_batch_build(p.own_quot.get(), d_quot, false);  // chunks [q0_lo, q0_hi, q1_lo, q1_hi] == d_quot viewed as Q columns of n, proof after proof
    p.quot = p.own_quot.get();
}

// ---- stage: the opening points.  On the line the quotient caps are observed first (:589-591); a proof from three commitments draws
// zeta straight from its compacted transcript.
static void set_zeta(table_proof& p, size_t sg, gl2_t zeta) {
    if (gl2_eq(gl2_exp_pow2(zeta, p.log_n), gl2_t{1, 0})) throw std::runtime_error("Opening point is in the subgroup.");  // :596-599
    p.zeta[sg] = zeta;
    p.zeta_next[sg] = gl2_scalar_mul(zeta, gl_root_of_unity(p.log_n));
}
static void draw_zeta(table_proof& p) {
    put_caps(p, 2, p.quot);
    for (size_t sg = 0; sg < p.nseg(); sg++) set_zeta(p, sg, zkm_transcript_zeta(p.chs[sg], p.y, p.blobs[sg]));
}

// ---- stage: StarkOpeningSet::new (proof.rs:299-334, between two timed! scopes in the reference)
static void write_openings(table_proof& p) {
    const zkm_blob_desc& y = p.y;
    const size_t total_helpers = y.A - y.Z;  // index of the first CTL Z among the auxiliary polynomials
    zkm_prof_scope st(p.c, "stage/openings (StarkOpeningSet::new)");
    auto ev = eval_batches(p.c, {p.trace, p.aux, p.quot}, p.zeta.data(), p.zeta_next.data());
    auto put = [](uint64_t* at, size_t i, gl2_t v) { at[2 * i] = v.c0; at[2 * i + 1] = v.c1; };
    for (size_t sg = 0; sg < p.nseg(); sg++) {
        const auto o = y.openings(p.blobs[sg]);
        const auto &tv = ev[sg][0], &av = ev[sg][1], &qv = ev[sg][2];
        for (size_t i = 0; i < y.W; i++) { put(o.local, i, tv[i].at_z0); put(o.next, i, tv[i].at_z1); }
        for (size_t i = 0; i < y.A; i++) { put(o.aux, i, av[i].at_z0); put(o.aux_next, i, av[i].at_z1); }
        for (size_t i = 0; i < y.Z; i++) o.ctl_zs_first[i] = av[total_helpers + i].at_one;
        for (size_t i = 0; i < y.Q; i++) put(o.quotient, i, qv[i].at_z0);
    }
}

// ---- stage: prove_openings (:618-628, App. A.8): the FRI alpha, the three composites of the STARK instance, then fri_finish
static void prove_openings(table_proof& p) {
    zkm_ctx* const c = p.c;
    const zkm_blob_desc& y = p.y;
    const size_t nseg = p.nseg(), n = p.n(), W = y.W, A = y.A, total_helpers = A - y.Z;
    zkm_prof_scope st_fri(c, "stage/compute openings proof");
    const size_t np0 = W + A + y.Q, np1 = W + A, np2 = y.Z, apow_seg = 2 * (np0 + 1);
    std::vector<gl_t> apow(nseg * apow_seg);
    for (size_t sg = 0; sg < nseg; sg++) alpha_powers(zkm_transcript_fri_alpha(p.chs[sg], y, p.blobs[sg]), np0, apow.data() + sg * apow_seg);
    gl_t* d_apow = p.scratch.alloc<gl_t>(apow.size() * sizeof(gl_t));
    c->upload(d_apow, apow.data(), apow.size() * sizeof(gl_t));
    gl_t* d_comp = p.scratch.alloc<gl_t>(nseg * 6 * n * sizeof(gl_t));
    const zkm_batch *tb = p.trace, *ab = p.aux, *qb = p.quot;
    if (tb->coeff_s1 != ab->coeff_s1 || tb->coeff_s1 != qb->coeff_s1) throw std::runtime_error("internal: coefficient layouts of the three oracles differ");
    {
        zkm_prof_scope ps(c, "fri_combine");
        const unsigned z = (unsigned)nseg;
        // slices of >= 32 polynomials while the launch stays below ~2^17 threads (two waves per SIMD)
        size_t slices = np0 / 32 < 1 ? 1 : np0 / 32;
        while (slices > 1 && slices * n * nseg > ((size_t)1 << 17)) slices >>= 1;
        if (slices >= 4) {
            const size_t per = (np0 + slices - 1) / slices;
            slices = (np0 + per - 1) / per;
            gl_t* d_part = p.scratch.alloc<gl_t>(nseg * slices * 6 * n * sizeof(gl_t));
            hipLaunchKernelGGL(k_fri_combine_slice, dim3((n + 255) / 256, (unsigned)slices, z), dim3(256), 0, c->stream, tb->coeffs, W, ab->coeffs, A,
                               qb->coeffs, y.Q, total_helpers, d_apow, n, per, d_part, apow_seg);
            hipLaunchKernelGGL(k_fri_combine_sum, dim3((n + 255) / 256, 1, z), dim3(256), 0, c->stream, d_part, (unsigned)slices, n, d_comp);
        } else {
            hipLaunchKernelGGL(k_fri_combine, dim3((n + 255) / 256, 1, z), dim3(256), 0, c->stream, tb->coeffs, W, ab->coeffs, A, qb->coeffs, y.Q,
                               total_helpers, d_apow, n, d_comp, apow_seg);
        }
        ZKM_HIP_CHECK(hipGetLastError());
    }
    // the batches at zeta, g zeta and 1 (stark.rs:127-148)
    std::vector<std::vector<fri_composite>> comps(nseg);
    for (size_t sg = 0; sg < nseg; sg++) {
        const gl_t* ap = apow.data() + sg * apow_seg;
        comps[sg] = {{nullptr, nullptr, p.zeta[sg], gl2_t{ap[2 * np0], ap[2 * np0 + 1]}},
                     {nullptr, nullptr, p.zeta_next[sg], gl2_t{ap[2 * np1], ap[2 * np1 + 1]}},
                     {nullptr, nullptr, gl2_t{1, 0}, gl2_t{ap[2 * np2], ap[2 * np2 + 1]}}};
    }
    const zkm_batch* orc[3] = {tb, ab, qb};
    fri_finish(p, y.fri(), tb->coeff_s1, d_comp, std::move(comps), orc, 3);
}

// the line from the point where both commitments exist
static void prove_from_aux(table_proof& p, int table_id, const ctl_dev_owner& own, const uint64_t* lookup_challenges) {
    commit_quotient(p, table_id, own, lookup_challenges);
    draw_zeta(p);
    write_openings(p);
    prove_openings(p);
}

// ---- driver: from existing (stacked) trace AND auxiliary commitments (zkm_prove_with_traces builds the auxiliary commitments of all
// tables ahead of the transcript, side by side -- they only depend on the CTL challenges); zs = chs.size() lists of CtlZData,
// lookup_challenges = chs.size() x num_challenges; throws
void zkm_prove_table_from_commitments(zkm_ctx* c, int table_id, const zkm_stark_config* cfg, size_t ncols, unsigned log_n, const zkm_batch* trace_batch,
                                      const zkm_batch* aux_batch, size_t naux_ctl, const zkm_ctl_table* table, const zkm_ctl_z* zs,
                                      const uint32_t* colset_ids, size_t nzs, const uint64_t* lookup_challenges, const std::vector<zkm_challenger*>& chs,
                                      const std::vector<uint64_t*>& proofs) {
    if (!trace_batch || !aux_batch) throw std::runtime_error("prove_single_table: commitments are required");
    if (chs.empty() || chs.size() > ZKM_MAX_SEG || proofs.size() != chs.size()) throw std::runtime_error("prove_single_table: bad stack size");
    table_proof p{{c, cfg, log_n, chs, proofs}, describe_table_proof(table_id, cfg, ncols, log_n, naux_ctl, zs, nzs, lookup_challenges), trace_batch, aux_batch};
    require_batch(p.trace, ncols, log_n, cfg, p.nseg(), "trace commitment does not match the table shape / config");
    require_batch(p.aux, p.y.A, log_n, cfg, p.nseg(), "auxiliary commitment does not match the table shape / config");
    ctl_dev_owner own;
    upload_ctl(p, own, table, zs, colset_ids);
    begin_blobs(p);
    prove_from_aux(p, table_id, own, lookup_challenges);
}

// ------------------------------------------------------------------ C ABI
// (a prove entry point advances copies of its callers' transcripts and hands them back only when the whole proof exists:
// zkm_transcripts, zkm_internal.h)

// ---- PolynomialBatch::prove_openings for an arbitrary FriInstanceInfo (plonky2 fri/oracle.rs; instance of the STARKs: stark.rs:91-148)
// composite of one batch: sum_j alpha^j p_j, polynomials named by (oracle, column) -- any oracle, any column -- for every batch of every
// claim in ONE launch (zkm_fri_prove: one claim; zkm_fri_prove_stack: one a member): blockIdx.y = batch, blockIdx.z = claim.  The claims
// share the instance, so the (oracle, polynomial) lists lie once in device memory, batch after batch; an oracle is a base pointer and the
// words from one member's polynomials to the next one's, as in gather_args -- no pointer table per claim.  A workgroup's lanes share
// claim, batch and list: the list entries and the claim's alpha powers are read through the constant address space (written before the
// launch, read-only in it: scalar loads, as zkm_seg_desc's), the oracle's base and stride come from the kernel argument by a uniform
// index, and the only per-lane traffic is the coefficient itself -- adjacent lanes, adjacent coefficients.  The products run down the
// list in its order, whatever the number of claims: claim k's composites are those of a call with that claim alone, word for word.
static_assert(sizeof(zkm_fri_poly) == 8, "a list entry is read as one 64-bit word");
struct fri_list_args {
    const gl_t* base[ZKM_FRI_MAX_ORACLES];   // oracle o: member 0's coefficients
    size_t member[ZKM_FRI_MAX_ORACLES];      // ... and the words to the next member's (ncols x n)
    uint32_t first[FRI_MAX_BATCHES + 1];     // batch b's list: polys[first[b] .. first[b + 1])
};
__global__ __launch_bounds__(256) void k_fri_combine_lists(fri_list_args A, const zkm_fri_poly* __restrict__ polys,
                                                           const gl_t* __restrict__ apow /* [claim][apow_seg]: alpha^j as (c0, c1) */, size_t apow_seg,
                                                           size_t n, gl_t* __restrict__ comp /* [claim][batch][2][n] */) {
    typedef const __attribute__((address_space(4))) uint64_t* list_ptr;   // (an entry is one 64-bit word: oracle below, polynomial above)
    typedef const __attribute__((address_space(4))) gl_t* power_ptr;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t b = blockIdx.y, claim = blockIdx.z, np = A.first[b + 1] - A.first[b];
    const list_ptr list = (list_ptr)polys + A.first[b];
    const power_ptr ap = (power_ptr)apow + (size_t)claim * apow_seg;
    gl_t a0 = 0, a1 = 0;
    auto at = [&](uint32_t j) -> const gl_t* {   // (uniform but for i)
        const uint64_t q = list[j];
        const uint32_t o = (uint32_t)q;
        return A.base[o] + (size_t)claim * A.member[o] + (q >> 32) * n + i;
    };
    auto take = [&](uint32_t j, gl_t v) {
        a0 = gl_add(a0, gl_mul(v, ap[2 * j]));
        a1 = gl_add(a1, gl_mul(v, ap[2 * j + 1]));
    };
    uint32_t j = 0;
    for (; j + 4 <= np; j += 4) {   // four coefficients in flight before the first product
        const gl_t v0 = *at(j), v1 = *at(j + 1), v2 = *at(j + 2), v3 = *at(j + 3);
        take(j, v0); take(j + 1, v1); take(j + 2, v2); take(j + 3, v3);
    }
    for (; j < np; j++) take(j, *at(j));
    gl_t* const out = comp + ((size_t)claim * gridDim.y + b) * 2 * n;
    out[i] = a0;
    out[n + i] = a1;
}

// the FRI-only blob of zkm_fri_prove (proof_blob.h)
zkm_fri_part zkm_fri_blob_describe(const zkm_stark_config* cfg, unsigned log_n, const size_t* cols, size_t noracles) {
    validate_config(cfg, log_n, /*fri_only=*/true);
    if (noracles == 0 || noracles > ZKM_FRI_MAX_ORACLES) throw std::runtime_error("zkm_fri_prove: 1..8 oracles");
    const unsigned L = fri_num_layers(cfg, log_n);
    zkm_fri_part y{ZKM_FRI_BLOB_HEADER_WORDS, (size_t)4 << cfg->cap_height, (size_t)1 << (log_n - L * cfg->arity_bits), cfg->num_queries,
                   zkm_query_round{{}, noracles, L, log_n + cfg->rate_bits, cfg->cap_height, cfg->arity_bits}};
    std::copy(cols, cols + noracles, y.round.cols);
    return y;
}

// parity / debug: a b mod p through THIS translation unit's gl_mul_loose (GL_REDUCE_BRANCHFREE), for zkm_field_selftest
__global__ void k_mul_selftest_branchfree(const uint64_t* __restrict__ a, const uint64_t* __restrict__ b, size_t n, uint64_t* __restrict__ out) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = gl_canon(gl_mul_loose(a[i], b[i]));
}
void zkm_launch_mul_selftest_branchfree(zkm_ctx* c, const uint64_t* a, const uint64_t* b, size_t n, uint64_t* out) {
    hipLaunchKernelGGL(k_mul_selftest_branchfree, dim3((n + 255) / 256), dim3(256), 0, c->stream, a, b, n, out);
    ZKM_HIP_CHECK(hipGetLastError());
}

// parity / debug: this translation unit's consumer_t on chosen challenges and loose terms (zkm_consumer_selftest, include/zkm_hip.h)
template <int NA, int B>
__device__ __forceinline__ void consumer_take(consumer_t<NA>& k, const uint64_t* __restrict__ t, size_t n) {
    if constexpr (B == 1) {
        k.constraint(t[0]);
    } else {
        uint64_t c[B];
#pragma unroll
        for (int i = 0; i < B; i++) c[i] = t[(size_t)i * n];
        k.constraints(c);
    }
}
template <int NA>
__device__ void consumer_take_n(consumer_t<NA>& k, const uint64_t* __restrict__ t, size_t n, uint32_t b) {
    switch (b) {   // (wave-uniform)
        case 1: consumer_take<NA, 1>(k, t, n); break;
        case 2: consumer_take<NA, 2>(k, t, n); break;
        case 3: consumer_take<NA, 3>(k, t, n); break;
        case 4: consumer_take<NA, 4>(k, t, n); break;
        case 5: consumer_take<NA, 5>(k, t, n); break;
        case 6: consumer_take<NA, 6>(k, t, n); break;
        case 7: consumer_take<NA, 7>(k, t, n); break;
        default: consumer_take<NA, 8>(k, t, n); break;
    }
}
template <int NA>
__global__ __launch_bounds__(256) void k_consumer_selftest(alpha_args alphas, const uint64_t* __restrict__ terms, size_t K, size_t n, uint32_t run,
                                                           uint64_t* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    consumer_t<NA> k;
#pragma unroll
    for (int a = 0; a < NA; a++) { k.set_alpha(a, alphas.v[a]); k.acc[a] = 0; }
    k.z_last = k.l_first = k.l_last = 0;
    size_t t = 0;
    for (; K - t >= run; t += run) consumer_take_n<NA>(k, terms + t * n + i, n, run);
    if (t < K) consumer_take_n<NA>(k, terms + t * n + i, n, (uint32_t)(K - t));
#pragma unroll
    for (int a = 0; a < NA; a++) out[(size_t)a * n + i] = k.value(a);
}

extern "C" {

int zkm_consumer_selftest(zkm_ctx* c, const uint64_t* alphas, size_t nalphas, const uint64_t* terms, size_t K, size_t n, uint32_t run,
                          uint64_t* out, char** err) {
    return zkm_api("zkm_consumer_selftest", c, err, [&] {
        if (!alphas || !terms || !out) throw std::runtime_error("zkm_consumer_selftest: null argument");
        if (nalphas < 1 || nalphas > 2) throw std::runtime_error("zkm_consumer_selftest: 1 or 2 challenges");
        if (run < 1 || run > (uint32_t)consumer_t<2>::RUN) throw std::runtime_error("zkm_consumer_selftest: run must be 1 .. 8");
        if (K == 0 || n == 0 || n > ((size_t)1 << 20) || K > ((size_t)1 << 26) / n) throw std::runtime_error("zkm_consumer_selftest: K, n out of range");
        alpha_args a{};
        for (size_t j = 0; j < nalphas; j++) a.v[j] = alphas[j];
        zkm_scratch dt(c, K * n * 8), dout(c, nalphas * n * 8);
        ZKM_HIP_CHECK(hipMemcpyAsync(dt.p, terms, K * n * 8, hipMemcpyHostToDevice, c->stream));
        const dim3 grid((unsigned)((n + 255) / 256)), block(256);
        with_nalphas(nalphas, [&](auto NA) {
            hipLaunchKernelGGL((k_consumer_selftest<decltype(NA)::value>), grid, block, 0, c->stream, a, dt.as<uint64_t>(), K, n, run, dout.as<uint64_t>());
        });
        ZKM_HIP_CHECK(hipGetLastError());
        ZKM_HIP_CHECK(hipMemcpyAsync(out, dout.p, nalphas * n * 8, hipMemcpyDeviceToHost, c->stream));
        c->sync();
    });
}

size_t zkm_fri_proof_words(const zkm_stark_config* cfg, unsigned log_n, const size_t* oracle_cols, size_t noracles) {
    zkm_fri_part y{};   // (0 = unsupported configuration)
    return zkm_api("zkm_fri_proof_words", nullptr, [&] { y = zkm_fri_blob_describe(cfg, log_n, oracle_cols, noracles); }) ? 0 : y.total();
}

// K opening proofs of one instance in LOCK-STEP, the body of zkm_fri_prove (K = 1 on single commitments) and zkm_fri_prove_stack: the
// oracles are stacks of K members, claim k opens member k of every oracle at points[(k * nbatches + b) * 2 ..] on challengers[k] into
// proofs_out[k].  One combination launch for all batches and claims, then fri_finish on a proof_stack of K.  `who` starts every
// refusal; `name_claims`: a refusal of one claim's arguments says which.  Everything is refused before a blob is written, and the
// callers' challengers move only when every proof exists.
static void fri_prove_claims(const char* who_, bool name_claims, zkm_ctx* c, const zkm_stark_config* cfg, const zkm_batch* const* oracles, size_t noracles,
                             const zkm_fri_batch* batches, size_t nbatches, size_t K, const uint64_t* points, zkm_challenger* const* challengers,
                             uint64_t* const* proofs_out) {
    const std::string who(who_);
    if (noracles == 0 || noracles > ZKM_FRI_MAX_ORACLES) throw std::runtime_error(who + ": 1..8 oracles");
    if (nbatches > FRI_MAX_BATCHES) throw std::runtime_error(who + ": 1..8 opening batches");
    for (size_t o = 0; o < noracles; o++)
        if (!oracles[o]) throw std::runtime_error(who + ": null argument");
    if (K == 0 || K > ZKM_MAX_SEG) throw std::runtime_error(who + ": 1..32 claims");
    const unsigned log_n = oracles[0]->log_n;
    size_t cols[ZKM_FRI_MAX_ORACLES];
    for (size_t o = 0; o < noracles; o++) {
        if (oracles[o]->nseg != K) throw std::runtime_error(who + ": oracles must be stacks of one size");
        if (oracles[o]->log_n != log_n || oracles[o]->rate_bits != cfg->rate_bits || oracles[o]->cap_height != cfg->cap_height ||
            oracles[o]->coeff_s1 != oracles[0]->coeff_s1)
            throw std::runtime_error(who + ": oracles must share degree, rate and cap height with the config");
        cols[o] = oracles[o]->ncols;
    }
    const zkm_fri_part y = zkm_fri_blob_describe(cfg, log_n, cols, noracles);
    const size_t n = (size_t)1 << log_n;
    fri_list_args A{};
    std::vector<zkm_fri_poly> list;
    size_t maxp = 0;
    for (size_t b = 0; b < nbatches; b++) {
        if (batches[b].npolys == 0 || !batches[b].polys) throw std::runtime_error(who + ": empty batch");
        for (size_t j = 0; j < batches[b].npolys; j++)
            if (batches[b].polys[j].oracle >= noracles || batches[b].polys[j].poly >= cols[batches[b].polys[j].oracle])
                throw std::runtime_error(who + ": polynomial index out of range");
        list.insert(list.end(), batches[b].polys, batches[b].polys + batches[b].npolys);
        if (list.size() > UINT32_MAX) throw std::runtime_error(who + ": too many polynomials");
        A.first[b + 1] = (uint32_t)list.size();
        maxp = std::max(maxp, batches[b].npolys);
    }
    for (size_t k = 0; k < K; k++) {
        const std::string claim = name_claims ? who + ": claim " + std::to_string(k) : who;
        if (!challengers[k] || !proofs_out[k]) throw std::runtime_error(claim + ": null argument");
        for (size_t w = 0; w < 2 * nbatches; w++)
            if (points[k * 2 * nbatches + w] >= GL_P) throw std::runtime_error(claim + ": non-canonical opening point");
    }
    for (size_t o = 0; o < noracles; o++) { A.base[o] = oracles[o]->coeffs; A.member[o] = oracles[o]->coeff_seg(); }
    for (size_t k = 0; k < K; k++) {
        memset(proofs_out[k], 0, y.total() * sizeof(uint64_t));
        zkm_fri_blob_header_write(proofs_out[k], cfg, log_n, y);
    }

    zkm_transcripts tr(challengers, K);
    const std::vector<uint64_t*> blobs(proofs_out, proofs_out + K);
    proof_stack f{c, cfg, log_n, tr.chs, blobs};
    const size_t apow_seg = 2 * (maxp + 1);
    std::vector<gl_t> apow(K * apow_seg);
    for (size_t k = 0; k < K; k++) alpha_powers(zkm_challenger_get_ext(tr.chs[k]), maxp, apow.data() + k * apow_seg);
    // (zkm_ctx::upload is done with its source when it returns: no wait for the stream before the host vectors go)
    gl_t* d_apow = f.scratch.alloc<gl_t>(apow.size() * sizeof(gl_t));
    c->upload(d_apow, apow.data(), apow.size() * sizeof(gl_t));
    zkm_fri_poly* d_list = f.scratch.alloc<zkm_fri_poly>(list.size() * sizeof(zkm_fri_poly));
    c->upload(d_list, list.data(), list.size() * sizeof(zkm_fri_poly));
    gl_t* d_comp = f.scratch.alloc<gl_t>(K * 2 * nbatches * n * sizeof(gl_t));
    {
        zkm_prof_scope ps(c, "fri_combine");
        hipLaunchKernelGGL(k_fri_combine_lists, dim3((unsigned)((n + 255) / 256), (unsigned)nbatches, (unsigned)K), dim3(256), 0, c->stream, A, d_list,
                           d_apow, apow_seg, n, d_comp);
        ZKM_HIP_CHECK(hipGetLastError());
    }
    std::vector<std::vector<fri_composite>> comps(K);
    for (size_t k = 0; k < K; k++)
        for (size_t b = 0; b < nbatches; b++) {
            const uint64_t* pt = points + (k * nbatches + b) * 2;
            const gl_t* shift = apow.data() + k * apow_seg + 2 * batches[b].npolys;
            comps[k].push_back({nullptr, nullptr, gl2_t{pt[0], pt[1]}, gl2_t{shift[0], shift[1]}});
        }
    fri_finish(f, y, oracles[0]->coeff_s1, d_comp, std::move(comps), oracles, noracles);
    tr.commit();
}

// one claim on single commitments: the points are the batches' own
int zkm_fri_prove(zkm_ctx* c, const zkm_stark_config* cfg, const zkm_batch* const* oracles, size_t noracles, const zkm_fri_batch* batches,
                  size_t nbatches, zkm_challenger* ch_io, uint64_t* proof, char** err) {
    return zkm_api("zkm_fri_prove", c, err, [&] {
        if (!cfg || !oracles || !batches || !nbatches || !ch_io || !proof) throw std::runtime_error("zkm_fri_prove: null argument");
        if (nbatches > FRI_MAX_BATCHES) throw std::runtime_error("FRI: 1..8 opening batches");   // (this entry's words for it: divide_accumulate_all's)
        for (size_t o = 0; o < noracles; o++) {
            if (!oracles[o]) throw std::runtime_error("zkm_fri_prove: oracles must share degree, rate and cap height with the config");
            if (oracles[o]->nseg != 1) throw std::runtime_error("zkm_fri_prove: stacked batches are internal");
        }
        uint64_t points[2 * FRI_MAX_BATCHES];
        for (size_t b = 0; b < nbatches; b++) { points[2 * b] = batches[b].point[0]; points[2 * b + 1] = batches[b].point[1]; }
        fri_prove_claims("zkm_fri_prove", false, c, cfg, oracles, noracles, batches, nbatches, 1, points, &ch_io, &proof);
    });
}

// one claim a member of the oracles' stacks (zkm_batch_commit_*_stack), at points of its own
int zkm_fri_prove_stack(zkm_ctx* c, const zkm_stark_config* cfg, const zkm_batch* const* oracles, size_t noracles, const zkm_fri_batch* batches,
                        size_t nbatches, const uint64_t* points, zkm_challenger* const* challengers, uint64_t* const* proofs_out, char** err) {
    return zkm_api("zkm_fri_prove_stack", c, err, [&] {
        if (!cfg || !oracles || !batches || !nbatches || !points || !challengers || !proofs_out) throw std::runtime_error("zkm_fri_prove_stack: null argument");
        const size_t K = noracles && oracles[0] ? oracles[0]->nseg : 0;   // (no oracle, a null one: refused in the body before K is looked at)
        fri_prove_claims("zkm_fri_prove_stack", true, c, cfg, oracles, noracles, batches, nbatches, K, points, challengers, proofs_out);
    });
}

size_t zkm_proof_words(const zkm_stark_config* cfg, unsigned log_n, size_t ncols, size_t naux, size_t nctl_zs) {
    zkm_blob_desc y{};   // (0 = unsupported configuration: the prove entry points report which field)
    return zkm_api("zkm_proof_words", nullptr, [&] { y = zkm_blob_describe(cfg, log_n, ncols, naux, nctl_zs); }) ? 0 : y.total();
}

// CtlZData of the benchmark's fake CTL shape: helper columns, no column sets (poseidon_stark.rs:786-799)
static std::vector<zkm_ctl_z> fake_zs(const uint32_t* num_helpers, size_t n) {
    std::vector<zkm_ctl_z> zs(n);
    for (size_t i = 0; i < n; i++) {
        if (num_helpers[i] == 0) throw std::runtime_error("CTLs without helper columns need column sets: use zkm_prove_single_table_ctl");
        zs[i] = zkm_ctl_z{0, 0, num_helpers[i], 0, 0, 0};
    }
    return zs;
}

// ---- driver: from values -- the trace's (or its commitment, if the caller has one) and the CTL columns'
int zkm_prove_single_table_ctl(zkm_ctx* c, int table_id, const zkm_stark_config* cfg, const uint64_t* trace, size_t ncols, unsigned log_n,
                               const zkm_batch* trace_batch, const uint64_t* aux, size_t naux, const zkm_ctl_table* table,
                               const zkm_ctl_z* zs, const uint32_t* colset_ids, size_t nzs, const uint64_t* lookup_challenges,
                               zkm_challenger* challenger, uint64_t* proof_out, char** err) {
    return zkm_api("zkm_prove_single_table", c, err, [&] {
        if (!cfg || !challenger || !proof_out) throw std::runtime_error("zkm_prove_single_table: null argument");
        if (!trace && !trace_batch) throw std::runtime_error("zkm_prove_single_table: need trace values or a trace commitment");
        zkm_transcripts tr(challenger);
        const std::vector<uint64_t*> blobs{proof_out};
        table_proof p{{c, cfg, log_n, tr.chs, blobs}, describe_table_proof(table_id, cfg, ncols, log_n, naux, zs, nzs, lookup_challenges), trace_batch};
        if (p.y.A != naux && !trace) throw std::runtime_error("this table has lookups: the trace values are required to build their helper columns");
        ctl_dev_owner own;
        upload_ctl(p, own, table, zs, colset_ids);
        if (!p.trace) commit_trace(p, trace);
        require_batch(p.trace, ncols, log_n, cfg, 1, "trace commitment does not match the table shape / config");
        begin_blobs(p);
        commit_aux(p, table_id, trace, aux, lookup_challenges);
        prove_from_aux(p, table_id, own, lookup_challenges);
        tr.commit();
    });
}

// ---- driver: from three commitments (BASELINE config 4): compact -> zeta -> openings -> prove_openings.  No table: the widths are
// the commitments' own, and of the CTL description only the number of Zs -- the last nctl_zs auxiliary polynomials -- matters.
int zkm_prove_openings(zkm_ctx* c, const zkm_stark_config* cfg, const zkm_batch* trace_batch, const zkm_batch* aux_batch,
                       const zkm_batch* quot_batch, size_t nctl_zs, zkm_challenger* challenger, uint64_t* proof_out, char** err) {
    return zkm_api("zkm_prove_openings", c, err, [&] {
        if (!cfg || !challenger || !proof_out) throw std::runtime_error("zkm_prove_openings: null argument");
        if (!trace_batch || !aux_batch || !quot_batch) throw std::runtime_error("zkm_prove_openings: three commitments are required");
        const unsigned log_n = trace_batch->log_n;
        const size_t A = aux_batch->ncols;
        zkm_transcripts tr(challenger);
        const std::vector<uint64_t*> blobs{proof_out};
        table_proof p{{c, cfg, log_n, tr.chs, blobs}, zkm_blob_describe(cfg, log_n, trace_batch->ncols, A, nctl_zs), trace_batch, aux_batch, quot_batch};
        if (p.y.L > ZKM_FRI_GATHER_LAYERS) throw std::runtime_error("too many FRI layers");
        if (nctl_zs > A) throw std::runtime_error("zkm_prove_openings: more CTL Zs than auxiliary polynomials");
        if (A == 0) throw std::runtime_error("No CTL? aux column count does not match the CTL description");  // prover.rs:509
        require_batch(p.trace, p.y.W, log_n, cfg, 1, "trace commitment does not match the table shape / config");
        for (const zkm_batch* b : {p.aux, p.quot})   // (their widths: the auxiliary commitment's is A by definition, the quotient's follows)
            require_batch(b, b->ncols, log_n, cfg, 1, "zkm_prove_openings: commitments do not match the table shape / config");
        if (p.quot->ncols != p.y.Q) throw std::runtime_error("zkm_prove_openings: unexpected number of polynomials");
        begin_blobs(p);
        put_caps(p, 1, p.aux);
        put_caps(p, 2, p.quot);
        set_zeta(p, 0, zkm_challenger_get_ext(tr.chs[0]));
        write_openings(p);
        prove_openings(p);
        tr.commit();
    });
}

int zkm_prove_single_table(zkm_ctx* c, int table_id, const zkm_stark_config* cfg, const uint64_t* trace, size_t ncols, unsigned log_n,
                           const zkm_batch* trace_batch, const uint64_t* aux, size_t naux, const uint32_t* num_helpers, size_t nctl_zs,
                           zkm_challenger* challenger, uint64_t* proof_out, char** err) {
    return zkm_api("zkm_prove_single_table", err, [&] {
        auto zs = fake_zs(num_helpers, nctl_zs);
        return zkm_prove_single_table_ctl(c, table_id, cfg, trace, ncols, log_n, trace_batch, aux, naux, nullptr, zs.data(), nullptr,
                                          nctl_zs, nullptr, challenger, proof_out, err);
    });
}

// K proofs of the same table at the same height in LOCK-STEP (the benchmark shape: CtlData given as auxiliary columns, no column sets):
// the K trace and auxiliary commitments are stacked batches, every stage is one launch for all K, each transcript round trip serves
// all K.  Tables with lookups of their own need zkm_prove_segments.
int zkm_prove_single_tables(zkm_ctx* c, int table_id, const zkm_stark_config* cfg, size_t nproofs, const uint64_t* const* traces, size_t ncols,
                            unsigned log_n, const uint64_t* const* aux, size_t naux, const uint32_t* num_helpers, size_t nctl_zs,
                            zkm_challenger* const* challengers, uint64_t* const* proofs_out, char** err) {
    return zkm_api("zkm_prove_single_tables", c, err, [&] {
        if (!cfg || !traces || !aux || !challengers || !proofs_out) throw std::runtime_error("zkm_prove_single_tables: null argument");
        if (nproofs == 0) return;
        if (nproofs > ZKM_MAX_SEG) throw std::runtime_error("zkm_prove_single_tables: at most 32 proofs per call");
        validate_config(cfg, log_n);
        if (zkm_num_lookup_columns(table_id, cfg)) throw std::runtime_error("zkm_prove_single_tables: a table with lookups of its own needs zkm_prove_segments");
        auto zs1 = fake_zs(num_helpers, nctl_zs);
        std::vector<zkm_ctl_z> zs;
        for (size_t k = 0; k < nproofs; k++) zs.insert(zs.end(), zs1.begin(), zs1.end());
        for (size_t k = 0; k < nproofs; k++)
            if (!traces[k] || !aux[k] || !challengers[k] || !proofs_out[k]) throw std::runtime_error("zkm_prove_single_tables: null proof argument");
        zkm_transcripts tr(challengers, nproofs);
        const std::vector<uint64_t*> proofs(proofs_out, proofs_out + nproofs);
        const zkm_batch_ptr tb = commit_values(c, cfg, "stage/compute trace commitment", ncols, log_n, traces, nproofs),
                            ab = commit_values(c, cfg, "stage/compute auxiliary polynomials commitment", naux, log_n, aux, nproofs);
        zkm_prove_table_from_commitments(c, table_id, cfg, ncols, log_n, tb.get(), ab.get(), naux, nullptr, zs.data(), nullptr, nctl_zs, nullptr, tr.chs,
                                         proofs);
        tr.commit();
    });
}

int zkm_quotient(zkm_ctx* c, int table_id, const zkm_batch* trace, const zkm_batch* aux, const uint32_t* num_helpers, size_t nctl_zs,
                 const uint64_t* alphas, size_t nalphas, uint64_t* out_coeffs, char** err) {
    return zkm_api("zkm_quotient", c, err, [&] {
        if (!trace || !aux) throw std::runtime_error("zkm_quotient: null argument");
        auto zs = fake_zs(num_helpers, nctl_zs);
        ctl_dev_owner own;
        own.upload(c, nullptr, zs.data(), nullptr, nctl_zs);
        size_t words = nalphas * 2 * trace->n();
        bool dev = zkm_is_device_ptr(out_coeffs);
        zkm_scratch tmp(c, dev ? 8 : words * 8);   // released on every exit path
        gl_t* d = dev ? out_coeffs : tmp.as<gl_t>();
        quotient_device(c, table_id, trace, aux, own, nullptr, alphas, nalphas, d);
        if (!dev) {
            c->download(out_coeffs, d, words * 8);
        }
    });
}

// first row (of n) at which any of the nalphas accumulators is nonzero, into *first (left untouched if none): one pass
__global__ __launch_bounds__(256) void k_first_nonzero_row(const gl_t* __restrict__ acc, size_t n, unsigned nalphas, unsigned long long* first) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    bool bad = false;
    for (unsigned a = 0; a < nalphas; a++) bad = bad || gl_canon(acc[(size_t)a * n + i]) != 0;
    if (bad) atomicMin(first, (unsigned long long)i);
}

int zkm_check_constraints(zkm_ctx* c, int table_id, const zkm_stark_config* cfg, const uint64_t* trace, size_t ncols, unsigned log_n,
                          const uint64_t* aux, size_t naux, const zkm_ctl_table* table, const zkm_ctl_z* zs, const uint32_t* colset_ids, size_t nzs,
                          const uint64_t* lookup_challenges, const uint64_t* alphas, size_t nalphas, uint64_t* first_failing_row, char** err) {
    return zkm_api("zkm_check_constraints", c, err, [&] {
        if (!cfg || !trace || !aux || !alphas || !first_failing_row) throw std::runtime_error("zkm_check_constraints: null argument");
        validate_config(cfg, log_n);
        if (!zkm_table(table_id)) throw std::runtime_error("zkm_check_constraints: unknown table id");
        // a table with lookups of its own (Memory, Arithmetic) takes its challenges from the caller: none given is an error here, not a
        // null dereference on the host
        if (!lookup_challenges && zkm_num_lookup_columns(table_id, cfg)) throw std::runtime_error("zkm_check_constraints: this table has lookups of its own: lookup challenges are required");
        if (nalphas < 1 || nalphas > 2) throw std::runtime_error("zkm_check_constraints: 1 or 2 challenges supported");
        for (size_t a = 0; a < nalphas; a++)
            if (alphas[a] >= GL_P) throw std::runtime_error("zkm_check_constraints: non-canonical challenge");
        const size_t n = (size_t)1 << log_n;
        // the values stand where the quotient kernels expect an LDE: "batches" of rate 0 over device copies of the caller's columns
        zkm_batch tb, ab;
        tb.ctx = ab.ctx = c; tb.ncols = ncols; ab.ncols = naux; tb.log_n = ab.log_n = log_n; tb.rate_bits = ab.rate_bits = 0;
        zkm_scratch_list tmp(c);
        auto on_device = [&](const uint64_t* p, size_t words) -> gl_t* {
            gl_t* d = tmp.alloc<gl_t>(words * sizeof(gl_t));
            ZKM_HIP_CHECK(hipMemcpyAsync(d, p, words * sizeof(gl_t), hipMemcpyDefault, c->stream));
            zkm_launch_canon(c, d, words);
            return d;
        };
        tb.lde = on_device(trace, ncols * n);
        ab.lde = on_device(aux, naux * n);
        ctl_dev_owner own;
        own.upload(c, table, zs, colset_ids, nzs, false, ncols);
        gl_t* d_acc = tmp.alloc<gl_t>(nalphas * n * sizeof(gl_t));
        quotient_device(c, table_id, &tb, &ab, own, lookup_challenges, alphas, nalphas, d_acc, /*check=*/true);
        unsigned long long* d_first = tmp.alloc<unsigned long long>(8);
        ZKM_HIP_CHECK(hipMemsetAsync(d_first, 0xff, 8, c->stream));
        hipLaunchKernelGGL(k_first_nonzero_row, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, d_acc, n, (unsigned)nalphas, d_first);
        ZKM_HIP_CHECK(hipGetLastError());
        unsigned long long first = ~0ULL;
        c->download(&first, d_first, 8);
        *first_failing_row = first;
        if (first != ~0ULL)
            throw std::runtime_error(std::string("Constraint failed in ") + zkm_table(table_id)->name + "Stark (first failing row " + std::to_string(first) + ")");   // prover.rs:903-908
    });
}

// every member of a stack (a single commitment: of one) at the member's own point: the member is the grid's z in k_open_powers /
// k_open_partials, one download
static void eval_openings_members(zkm_ctx* c, const zkm_batch* b, const uint64_t* zetas, uint64_t* out) {
    std::vector<gl2_t> z(b->nseg);
    for (size_t k = 0; k < b->nseg; k++) z[k] = gl2_t{zetas[2 * k], zetas[2 * k + 1]};
    const auto v = eval_batches(c, {b}, z.data(), z.data());
    for (size_t k = 0; k < b->nseg; k++)
        for (size_t i = 0; i < b->ncols; i++) {
            out[2 * (k * b->ncols + i)] = v[k][0][i].at_z0.c0;
            out[2 * (k * b->ncols + i) + 1] = v[k][0][i].at_z0.c1;
        }
}
int zkm_eval_openings(zkm_ctx* c, const zkm_batch* b, const uint64_t zeta[2], uint64_t* out, char** err) {
    return zkm_api("zkm_eval_openings", c, err, [&] {
        if (!b || !zeta || !out) throw std::runtime_error("zkm_eval_openings: null argument");
        if (b->nseg != 1) throw std::runtime_error("zkm_eval_openings: stacked batches are internal");
        eval_openings_members(c, b, zeta, out);
    });
}
int zkm_eval_openings_stack(zkm_ctx* c, const zkm_batch* b, const uint64_t* zetas, uint64_t* out, char** err) {
    return zkm_api("zkm_eval_openings_stack", c, err, [&] {
        if (!b || !zetas || !out) throw std::runtime_error("zkm_eval_openings_stack: null argument");
        if (b->nseg == 0 || b->nseg > ZKM_MAX_SEG) throw std::runtime_error("zkm_eval_openings_stack: 1..32 members");
        eval_openings_members(c, b, zetas, out);
    });
}

}  // extern "C"
