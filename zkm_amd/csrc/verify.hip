// verify.hip -- verify_proof on the GPU for the proof blobs this library writes (include/zkm_hip.h "verify_proof on the device").
//
// Reference: verify_proof prover/src/verifier.rs:27-176, verify_stark_proof_with_challenges :178-292, validate_proof_shape :294-342,
// eval_l_0_and_l_last :344-354, get_challenges.rs:124-148 / :190-233, verify_cross_table_lookups; plonky2 fri/verifier.rs
// (fri_verify_proof_of_work, fri_combine_initial, compute_evaluation, fri_verifier_query_round).
//
// Host: every word of the transcript is in the blob, so the replay needs no device round trip.  Per segment: validate the shape of
// every blob (nothing the device indexes with comes from anywhere else), seed the challenger, derive the CTL challenges and each
// table's CtlZData list (the prover's zkm_derive_zs), then per table alphas, zeta, fri_alpha, betas, the proof-of-work response and the
// query indices.  Proof of work and the ctl_zs_first sums are host checks.
// Device, K segments in one set of launches:
//   verify/line_rows      the base-field rows v0 + t v1, t = 0..4, of every table's opening
//   verify/line_<table>   the table's constraints on those rows (stark.hip k_verify_line: the code k_quotient runs), one launch per table
//   verify/merkle_chains  one hash chain per (segment, table, query, tree): leaf sponge, path, comparison with the cap entry
//   verify/fri_queries    one thread per (segment, table, query): fri_combine_initial, per layer the evaluation check and
//                         compute_evaluation, the final polynomial
//   verify/reduce         first finding per (segment, table) in the fixed order
// behind ONE upload (the parameter block with every CTL description, then the blobs) and before ONE download: the constraint
// accumulators and the reduced verdicts.  The quotient comparison is finished on the host.
//
// zkm_fri_verify (below the STARK verifier): plonky2's verify_fri_proof for ANY FriInstanceInfo, the mirror of zkm_fri_prove.  The chains
// and the reduction are the kernels above, working from zkm_verify_chains (zkm_internal.h), of which the STARK blob is the case of three
// initial trees; the query arithmetic is
//   verify/fri_instance_queries  one thread per (claim, query): fri_combine_initial through the batches' (oracle, polynomial) lists, then
//                                the layers and the final polynomial as verify/fri_queries runs them (fri_query_layers)
// All claims of a call share one upload, one set of launches and one download.
#include <iterator>
#include <memory>

#include "ctl_dev.h"
#include "poseidon_lat_dev.h"

namespace {

// ------------------------------------------------------------------ kernels
__global__ __launch_bounds__(256) void k_verify_rows(const zkm_verify_table* __restrict__ tabs, const gl_t* __restrict__ blobs, gl_t* __restrict__ rows) {
    const zkm_verify_table& T = tabs[blockIdx.y];
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x, W = (uint32_t)T.d.W, A = (uint32_t)T.d.A;
    if (c >= W + A) return;
    const auto o = T.d.openings(blobs + T.blob);
    const gl_t* l = c < W ? o.local + 2 * (size_t)c : o.aux + 2 * (size_t)(c - W);
    const gl_t* n = c < W ? o.next + 2 * (size_t)c : o.aux_next + 2 * (size_t)(c - W);
    gl_t l0 = l[0], n0 = n[0];
    const gl_t l1 = l[1], n1 = n[1];
    gl_t* out = rows + T.rows + 2 * (size_t)c;
    for (int t = 0; t < ZKM_VERIFY_LINE_POINTS; t++) {
        out[0] = l0;
        out[1] = n0;
        out += 2 * (size_t)(W + A);
        l0 = gl_add(l0, l1);
        n0 = gl_add(n0, n1);
    }
}

// One Merkle chain: the leaf's `len` words, `nsib` siblings, the leaf's index, the cap it must reach, and where its verdict goes.
// Chains of one entry (zkm_verify_chains: a (segment, table), or a claim of zkm_fri_verify) are numbered tree-major -- all queries of
// initial tree 0, of tree 1, .., then of each FRI layer -- so that the chains sharing a wave have leaves of the same length.
struct chain_t {
    const gl_t *leaf, *sib, *cap;
    uint32_t len, nsib, index, slot;
};
__device__ __forceinline__ bool chain_setup(const zkm_verify_chains& E, const gl_t* __restrict__ blobs, const uint32_t* __restrict__ xs, uint32_t idx,
                                            chain_t& ch) {
    const zkm_query_round& R = E.fri.round;
    const uint32_t nq = (uint32_t)E.fri.nq, initial = (uint32_t)R.noracles;
    if (idx >= nq * E.trees()) return false;
    const uint32_t tree = idx / nq, q = idx - tree * nq;
    const uint32_t x = xs[E.xs + q];
    const gl_t* blob = blobs + E.blob;
    const gl_t* qr = blob + E.fri.o_query(q);
    uint32_t slot;
    if (tree < initial) {
        ch.len = (uint32_t)R.cols[tree];
        ch.leaf = qr + R.oracle_evals(tree);
        ch.nsib = (uint32_t)R.initial_siblings();
        ch.index = x;
        ch.cap = blobs + E.caps + tree * E.fri.cap_words;
        slot = tree;
    } else {
        const uint32_t l = tree - initial;
        ch.len = (uint32_t)R.layer_values();
        ch.leaf = qr + R.layer_evals(l);
        ch.nsib = (uint32_t)R.layer_sibling_count(l);
        ch.index = x >> ((uint32_t)R.arity_bits * (l + 1));
        ch.cap = blob + E.fri.o_cap(l);
        slot = E.slot_layer_eval(l) + 1;
    }
    ch.sib = ch.leaf + ch.len;
    ch.slot = E.verdicts + q * E.slots() + slot;
    return true;
}

// a chain per quad of lanes (poseidon_lat_dev.h): lane q holds state words q, q + 4, q + 8.  Every lane of a wave takes part in every
// permutation (DPP), so the wave runs as many steps as its longest chain and a finished chain keeps its state.
__global__ __launch_bounds__(256) void k_verify_chains_quad(const zkm_verify_chains* __restrict__ ents, const gl_t* __restrict__ blobs,
                                                            const uint32_t* __restrict__ xs, uint32_t* __restrict__ verdicts) {
    const zkm_verify_chains& E = ents[blockIdx.y];
    if (blockIdx.x * 64u >= (uint32_t)E.fri.nq * E.trees()) return;   // (uniform over the workgroup)
    __shared__ __attribute__((aligned(16))) uint32_t qtab[ZKM_QUAD_TAB_WORDS];
    quad_tab_load(qtab);
    const poseidon_quad Q(threadIdx.x, qtab);
    const unsigned ql = threadIdx.x & 3;
    chain_t ch{};
    const bool live = chain_setup(E, blobs, xs, (blockIdx.x * 256u + threadIdx.x) >> 2, ch);
    const uint32_t nabsorb = !live || ch.len <= 4 ? 0 : (ch.len + 7) / 8;   // hash_or_noop: a leaf of <= 4 words is its own digest
    const uint32_t steps = live ? nabsorb + ch.nsib : 0;
    uint32_t most = steps;
    for (int o = 32; o >= 1; o >>= 1) most = max(most, (uint32_t)__shfl_xor((int)most, o));
    uint64_t s[3] = {0, 0, 0};
    if (live && ch.len <= 4 && ql < ch.len) s[0] = ch.leaf[ql];
    for (uint32_t step = 0; step < most; step++) {
        const bool active = step < steps;
        uint64_t t[3] = {s[0], s[1], s[2]};
        if (active) {
            if (step < nabsorb) {   // overwrite-mode absorb: a ragged tail overwrites only the words that exist
                const uint32_t c = step * 8;
                if (c + ql < ch.len) t[0] = ch.leaf[c + ql];
                if (c + 4 + ql < ch.len) t[1] = ch.leaf[c + 4 + ql];
            } else {                // two_to_one(left, right): the current digest on the side the index bit says
                const uint32_t j = step - nabsorb;
                const uint64_t sw = ch.sib[4 * j + ql], cur = s[0];
                const bool right = (ch.index >> j) & 1;
                t[0] = right ? sw : cur;
                t[1] = right ? cur : sw;
                t[2] = 0;
            }
        }
        poseidon_permute_quad(t, Q);
        if (active) { s[0] = t[0]; s[1] = t[1]; s[2] = t[2]; }
    }
    uint32_t bad = live && s[0] != ch.cap[4 * (size_t)(ch.index >> ch.nsib) + ql] ? 1u : 0u;
    bad |= (uint32_t)__shfl_xor((int)bad, 1);
    bad |= (uint32_t)__shfl_xor((int)bad, 2);
    if (live && ql == 0) verdicts[ch.slot] = bad;
}

// a chain per lane: calls of so many chains that they fill the machine
__global__ __launch_bounds__(256) void k_verify_chains(const zkm_verify_chains* __restrict__ ents, const gl_t* __restrict__ blobs,
                                                       const uint32_t* __restrict__ xs, uint32_t* __restrict__ verdicts) {
    chain_t ch{};
    if (!chain_setup(ents[blockIdx.y], blobs, xs, blockIdx.x * 256u + threadIdx.x, ch)) return;
    uint64_t s[12];
#pragma unroll
    for (int i = 0; i < 12; i++) s[i] = 0;
    if (ch.len <= 4) {
        for (uint32_t i = 0; i < ch.len; i++) s[i] = ch.leaf[i];
    } else {
        for (uint32_t c = 0; c < ch.len; c += 8) {
#pragma unroll
            for (uint32_t i = 0; i < 8; i++)
                if (c + i < ch.len) s[i] = ch.leaf[c + i];
            poseidon_permute(s);
        }
    }
    for (uint32_t j = 0; j < ch.nsib; j++) {
        const bool right = (ch.index >> j) & 1;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint64_t sw = ch.sib[4 * j + i], cur = s[i];
            s[i] = right ? sw : cur;
            s[4 + i] = right ? cur : sw;
            s[8 + i] = 0;
        }
        poseidon_permute(s);
    }
    const gl_t* cap = ch.cap + 4 * (size_t)(ch.index >> ch.nsib);
    verdicts[ch.slot] = (s[0] != cap[0] || s[1] != cap[1] || s[2] != cap[2] || s[3] != cap[3]) ? 1u : 0u;
}

__device__ __forceinline__ gl2_t ld2(const gl_t* p) { return gl2_t{p[0], p[1]}; }
// acc <- acc alpha + v for a base-field v
__device__ __forceinline__ gl2_t horner_base(gl2_t acc, gl2_t alpha, gl_t v) {
    acc = gl2_mul(acc, alpha);
    acc.c0 = gl_add(acc.c0, v);
    return acc;
}
// plonky2 compute_evaluation: the polynomial through the 2^arity_bits values of a coset at beta.  The points are start g^i with
// Z(X) = X^m - start^m, so the Lagrange basis is Z(beta) p_i / ((beta - p_i) m start^m): one pass, no tables.
__device__ gl2_t compute_evaluation(gl_t x, uint32_t within, uint32_t arity_bits, const gl_t* __restrict__ evals, gl2_t beta) {
    const uint32_t m = 1u << arity_bits;
    const gl_t g = gl_root_of_unity(arity_bits);
    const gl_t start = gl_mul(x, gl_pow(g, m - bitrev32(within, arity_bits)));
    const gl_t sm = gl_exp_pow2(start, arity_bits);
    gl2_t zb = gl2_exp_pow2(beta, arity_bits);
    zb.c0 = gl_sub(zb.c0, sm);
    gl2_t acc{0, 0};
    gl_t p = start;
    for (uint32_t i = 0; i < m; i++) {
        const gl2_t e = ld2(evals + 2 * (size_t)bitrev32(i, arity_bits));
        gl2_t den = beta;
        den.c0 = gl_sub(den.c0, p);
        acc = gl2_add(acc, gl2_mul(gl2_scalar_mul(e, p), gl2_inv(den)));
        p = gl_mul(p, g);
    }
    return gl2_scalar_mul(gl2_mul(acc, zb), gl_inv(gl_mul((gl_t)m, sm)));
}

// the layers and the final polynomial of one query (fri_verifier_query_round after fri_combine_initial): per layer the evaluation check
// and compute_evaluation, then the final polynomial at the last point.  v: the query's verdict word of layer 0's evaluation check (a
// layer's Merkle path has the word between two of them), beta(l): layer l's challenge
template <class Beta>
__device__ __forceinline__ void fri_query_layers(const zkm_fri_part& P, const gl_t* blob, const gl_t* qr, uint32_t x, gl_t sub_x, gl2_t old_eval, Beta beta,
                                                 uint32_t* v) {
    const zkm_query_round& R = P.round;
    const uint32_t L = (uint32_t)R.L, arity_bits = (uint32_t)R.arity_bits, arity = 1u << arity_bits;
    for (uint32_t l = 0; l < L; l++) {
        const gl_t* o = qr + R.layer_evals(l);
        const uint32_t within = x & (arity - 1);
        v[2 * l] = gl2_eq(ld2(o + 2 * (size_t)within), old_eval) ? 0u : 1u;
        old_eval = compute_evaluation(sub_x, within, arity_bits, o, beta(l));
        sub_x = gl_exp_pow2(sub_x, arity_bits);
        x >>= arity_bits;
    }
    const gl_t* fp = blob + P.o_final();
    gl2_t fe{0, 0};
    for (uint32_t i = (uint32_t)P.F; i-- > 0;) fe = gl2_add(gl2_scalar_mul(fe, sub_x), ld2(fp + 2 * (size_t)i));
    v[2 * L] = gl2_eq(fe, old_eval) ? 0u : 1u;
}

__global__ __launch_bounds__(64) void k_verify_fri(const zkm_verify_table* __restrict__ tabs, const gl_t* __restrict__ blobs,
                                                   const uint32_t* __restrict__ xs, uint32_t* __restrict__ verdicts) {
    const zkm_verify_table& T = tabs[blockIdx.y];
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    const zkm_blob_desc& d = T.d;
    if (q >= (uint32_t)d.nq) return;
    const uint32_t x = xs[T.xs + q];
    const gl_t* blob = blobs + T.blob;
    const zkm_fri_part P = d.fri();
    const zkm_query_round& R = P.round;
    const gl_t* qr = blob + P.o_query(q);
    const uint32_t W = (uint32_t)d.W, A = (uint32_t)d.A, NQ = (uint32_t)d.Q, Z = (uint32_t)d.Z;
    const uint32_t lde_bits = (uint32_t)d.lde_bits();
    const gl_t *ev0 = qr + R.oracle_evals(0), *ev1 = qr + R.oracle_evals(1), *ev2 = qr + R.oracle_evals(2);
    uint32_t* v = verdicts + T.verdicts + q * T.slots;
    const gl2_t fa = ld2(T.fri_alpha), apow_wa = ld2(T.apow_wa);
    // fri_combine_initial: the batch at zeta is the trace, auxiliary and quotient columns, the batch at g zeta the first two, the
    // batch at 1 the CTL Z columns
    gl2_t red1{0, 0}, redq{0, 0}, redz{0, 0};
    for (uint32_t c = A; c-- > 0;) red1 = horner_base(red1, fa, ev1[c]);
    for (uint32_t c = W; c-- > 0;) red1 = horner_base(red1, fa, ev0[c]);
    for (uint32_t c = NQ; c-- > 0;) redq = horner_base(redq, fa, ev2[c]);
    for (uint32_t c = A; c-- > A - Z;) redz = horner_base(redz, fa, ev1[c]);
    const gl2_t red0 = gl2_add(red1, gl2_mul(apow_wa, redq));
    const gl_t sub_x = gl_mul(GL_GENERATOR, gl_pow(gl_root_of_unity(lde_bits), bitrev32(x, lde_bits)));
    auto over = [&](gl2_t red, const gl_t* opened, gl2_t point) {
        gl2_t den{gl_sub(sub_x, point.c0), gl_neg(point.c1)};
        return gl2_mul(gl2_sub(red, ld2(opened)), gl2_inv(den));
    };
    gl2_t sum = over(red0, T.red_open[0], ld2(T.zeta));
    sum = gl2_add(gl2_mul(sum, apow_wa), over(red1, T.red_open[1], ld2(T.zeta_next)));
    sum = gl2_add(gl2_mul(sum, ld2(T.apow_z)), over(redz, T.red_open[2], gl2_t{1, 0}));
    fri_query_layers(P, blob, qr, x, sub_x, sum, [&](uint32_t l) { return ld2(T.betas[l]); }, v + 3);
}

// One claim of zkm_fri_verify as its query kernel sees it, beside the claim's zkm_verify_chains: what the transcript replay gave and the
// instance.  A batch's polynomials are `npolys` words of the call's list from `first` on: each the word offset of the polynomial's value
// inside a query round (its oracle's row, its column), so the kernel reads the values through the (oracle, poly) list without knowing
// the oracles.  The reduced openings and the alpha powers are worked out once per claim, on the host.
constexpr uint32_t FRI_CLAIM_BATCHES = 8;   // FRI_MAX_BATCHES of zkm_fri_prove (stark.hip)
struct fri_claim_batch {
    gl_t point[2], red_open[2], shift[2];   // the opening point, the alpha-reduction of the opened values, alpha^npolys
    uint32_t first, npolys;
};
struct fri_claim_dev {
    gl_t alpha[2], betas[ZKM_FRI_HEADER_LAYERS][2];
    uint32_t nbatches, reserved;
    fri_claim_batch b[FRI_CLAIM_BATCHES];
};
#define ZKM_CONSTANT_AS __attribute__((address_space(4)))

// plonky2 fri_verifier_query_round without the Merkle proofs, for any instance: one thread per (claim, query).  fri_combine_initial
// (fri/verifier.rs): per batch in instance order the alpha-reduction of its polynomials' values at x, minus the batch's reduced opening,
// over (x - point); ReducingFactor::shift chains the batches by alpha^npolys -- what k_fri_combine_lists and shift_poly do in
// zkm_fri_prove.  Everything the lanes of a claim share -- the description, the challenges, the batches and their polynomial lists -- is
// uniform over the workgroup and went up before the launch: it is read through the constant address space (scalar loads), as the calls'
// expansions read their descriptors (zkm_seg_desc).  A base-field point on the LDE coset is refused on the host: x - point is never 0.
__global__ __launch_bounds__(64) void k_fri_verify_queries(const zkm_verify_chains* __restrict__ ents, const fri_claim_dev* __restrict__ claims,
                                                           const uint32_t* __restrict__ polys, const gl_t* __restrict__ blobs,
                                                           const uint32_t* __restrict__ xs, uint32_t* __restrict__ verdicts) {
    const zkm_verify_chains& E = ents[blockIdx.y];
    const ZKM_CONSTANT_AS fri_claim_dev* K = (const ZKM_CONSTANT_AS fri_claim_dev*)claims + blockIdx.y;
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= (uint32_t)E.fri.nq) return;
    const uint32_t x = xs[E.xs + q], lde_bits = (uint32_t)E.fri.round.lde_bits;
    const gl_t* blob = blobs + E.blob;
    const gl_t* qr = blob + E.fri.o_query(q);
    const gl_t sub_x = gl_mul(GL_GENERATOR, gl_pow(gl_root_of_unity(lde_bits), bitrev32(x, lde_bits)));
    const gl2_t alpha{K->alpha[0], K->alpha[1]};
    gl2_t sum{0, 0};
    const uint32_t nbatches = K->nbatches;
    for (uint32_t b = 0; b < nbatches; b++) {
        const ZKM_CONSTANT_AS uint32_t* at = (const ZKM_CONSTANT_AS uint32_t*)polys + K->b[b].first;
        gl2_t red{0, 0};
        for (uint32_t j = K->b[b].npolys; j-- > 0;) red = horner_base(red, alpha, qr[at[j]]);
        const gl2_t den{gl_sub(sub_x, K->b[b].point[0]), gl_neg(K->b[b].point[1])};
        const gl2_t term = gl2_mul(gl2_sub(red, gl2_t{K->b[b].red_open[0], K->b[b].red_open[1]}), gl2_inv(den));
        sum = gl2_add(gl2_mul(sum, gl2_t{K->b[b].shift[0], K->b[b].shift[1]}), term);
    }
    fri_query_layers(E.fri, blob, qr, x, sub_x, sum, [&](uint32_t l) { return gl2_t{K->betas[l][0], K->betas[l][1]}; },
                     verdicts + E.verdicts + q * E.slots() + E.slot_layer_eval(0));
}

// first finding of an entry: the lowest query, and inside it the lowest slot -- the initial trees in order, per layer evaluation then
// Merkle path, the final polynomial (zkm_verify_chains numbers the slots in that order); ~0 when every check passed
__global__ __launch_bounds__(256) void k_verify_reduce(const zkm_verify_chains* __restrict__ ents, const uint32_t* __restrict__ verdicts,
                                                       uint32_t* __restrict__ first) {
    const zkm_verify_chains& T = ents[blockIdx.x];
    __shared__ uint32_t best;
    if (threadIdx.x == 0) best = ~0u;
    __syncthreads();
    const uint32_t n = (uint32_t)T.fri.nq * T.slots();
    uint32_t mine = ~0u;
    for (uint32_t i = threadIdx.x; i < n && mine == ~0u; i += blockDim.x)
        if (verdicts[T.verdicts + i]) mine = i;
    if (mine != ~0u) atomicMin(&best, mine);
    __syncthreads();
    if (threadIdx.x == 0) first[blockIdx.x] = best;
}

// ------------------------------------------------------------------ host
const char* const CODE_NAMES[] = {"OK", "SHAPE", "TRANSCRIPT_STATE", "CTL_CHALLENGES", "QUOTIENT", "POW", "INITIAL_MERKLE", "FRI_EVAL", "FRI_MERKLE",
                                  "FINAL_POLY", "CTL_SUM", "FAILED"};
std::string table_label(const zkm_table_input* tables, size_t t) {
    const zkm_table_row* row = zkm_table(tables[t].table_id);
    return "table " + std::to_string(t) + " (" + (row ? std::string(row->name) : "Table" + std::to_string(tables[t].table_id)) + ")";
}

// acc alpha^k + sum_j alpha^j v_j over k values v_j: F2 pairs (stride 2) or base-field words (stride 1)
gl2_t reduce_more(gl2_t acc, gl2_t alpha, const uint64_t* v, size_t k, size_t stride) {
    for (size_t i = k; i-- > 0;) acc = gl2_add(gl2_mul(acc, alpha), gl2_t{v[stride * i], stride == 2 ? v[2 * i + 1] : 0});
    return acc;
}
// f(t), t = 0 .. 4, of a polynomial of degree <= 3 with base-field coefficients -> its value at t = X in F[X] / (X^2 - 7); false when
// the fourth difference does not vanish (the degree is above 3)
bool line_value(const gl_t f[5], gl2_t* out) {
    gl_t d[5] = {f[0], f[1], f[2], f[3], f[4]};
    for (int k = 1; k <= 4; k++)
        for (int i = 4; i >= k; i--) d[i] = gl_sub(d[i], d[i - 1]);   // d[k] = k-th forward difference at 0
    if (d[4] != 0) return false;
    static const gl_t inv2 = gl_inv(2), inv3 = gl_inv(3), inv6 = gl_inv(6);
    const gl_t c3 = gl_mul(d[3], inv6), c2 = gl_mul(gl_sub(d[2], d[3]), inv2);
    const gl_t c1 = gl_add(gl_sub(d[1], gl_mul(d[2], inv2)), gl_mul(d[3], inv3));
    *out = gl2_t{gl_add(d[0], gl_mul(7, c2)), gl_add(c1, gl_mul(7, c3))};
    return true;
}

struct verify_input {
    const zkm_table_input* tables;   // ntables entries; log_n is compared with the blob's when check_heights is set
    const uint64_t* pub;
    size_t npub;
    const uint64_t* proofs;
    size_t words;
    const uint64_t* claimed;         // CTL challenges, or null
};
struct table_state {
    zkm_blob_desc y{};
    size_t off = 0;                  // of the blob in the segment's proofs
    gl_t alphas[2] = {0, 0};
    gl2_t zeta{0, 0};
    bool state_ok = true, pow_ok = true;
};
struct seg_state {
    zkm_verify_report rep{};
    std::string msg;
    bool launched = false;
    size_t first_entry = 0;          // of its tables among the launched (segment, table) entries
    std::vector<table_state> ts;
    std::vector<table_zs> tz;
    uint64_t challenges[4] = {0, 0, 0, 0};
    zkm_challenger ch{};
};

void reject(seg_state& S, uint32_t code, size_t table, const std::string& text) {
    S.rep.code = code;
    S.rep.table = (uint32_t)table;
    S.msg = text;
}

// validate_proof_shape (verifier.rs:294-342) and everything else the device will index with: header against cfg and the table, the
// blob inside proof_words, every field word canonical.  Fills the layouts; false (and the report) on the first finding.
bool check_shapes(const zkm_stark_config* cfg, const verify_input& in, size_t ntables, const std::vector<table_zs>& tz0, bool check_heights,
                  seg_state& S) {
    size_t off = 0;
    for (size_t t = 0; t < ntables; t++) {
        const std::string who = table_label(in.tables, t) + ": ";
        auto bad = [&](const std::string& why) { reject(S, ZKM_VERIFY_SHAPE, t, who + "malformed proof: " + why); return false; };
        if (in.words < off || in.words - off < 16) return bad("proof_words too short for the header");
        const uint64_t* p = in.proofs + off;
        if (p[0] != ZKM_PROOF_MAGIC) return bad("no proof header (magic)");
        if (p[1] == 0 || p[1] > 32) return bad("degree_bits out of range");
        const unsigned log_n = (unsigned)p[1];
        if (check_heights && in.tables[t].log_n != log_n) return bad("degree_bits is not the table's height");
        const size_t W = in.tables[t].ncols, A = zkm_num_lookup_columns(in.tables[t].table_id, cfg) + tz0[t].naux, Z = tz0[t].zs.size();
        table_state& ts = S.ts[t];
        try {
            ts.y = zkm_blob_describe(cfg, log_n, W, A, Z);
        } catch (const std::exception& e) {
            return bad(e.what());
        }
        const zkm_blob_desc& y = ts.y;
        uint64_t want[16];
        zkm_blob_header_write(want, y);
        for (int i = 2; i < 12; i++)
            if (p[i] != want[i]) return bad("header word " + std::to_string(i) + " does not match the configuration and the table");
        for (int i = 12; i < 16; i++)
            if (p[i] != want[i]) return bad("reserved header word not zero");
        const size_t total = y.total();
        if (y.L > ZKM_FRI_HEADER_LAYERS || y.lde_bits() > 31 || total >= ((uint64_t)1 << 32)) return bad("unsupported FRI shape");
        if (in.words - off < total) return bad("proof_words too short");
        for (size_t i = 16; i < total; i++)
            if (p[i] >= GL_P) return bad("word " + std::to_string(i) + " is not a canonical field element");
        ts.off = off;
        off += total;
    }
    return true;
}

// get_challenges.rs:190-233 for table t on the segment's challenger, the host checks of the table (recorded transcript state, proof of
// work), and the table's entry for the kernels
void replay_table(const zkm_stark_config* cfg, const verify_input& in, size_t t, seg_state& S, zkm_verify_table& T,
                  std::vector<uint32_t>& xs) {
    table_state& ts = S.ts[t];
    const zkm_blob_desc& y = ts.y;
    const uint64_t* proof = in.proofs + ts.off;
    zkm_challenger* ch = &S.ch;
    uint64_t st0[12];
    zkm_challenger_compact(ch, st0);   // proof.rs:199: the prover recorded the compacted state
    ts.state_ok = memcmp(st0, proof + y.o_init(), sizeof st0) == 0;
    zkm_transcript_alphas(ch, y, proof, cfg->num_challenges, ts.alphas);
    ts.zeta = zkm_transcript_zeta(ch, y, proof);
    auto put = [](gl_t* dst, gl2_t v) { dst[0] = v.c0; dst[1] = v.c1; };
    const gl2_t fri_alpha = zkm_transcript_fri_alpha(ch, y, proof);
    const zkm_fri_part f = y.fri();
    for (unsigned l = 0; l < y.L; l++) put(T.betas[l], zkm_transcript_fri_beta(ch, proof + f.o_cap(l), f.cap_words));
    zkm_transcript_final_poly(ch, proof + f.o_final(), f.F);
    ts.pow_ok = zkm_transcript_pow(ch, proof[f.o_pow()], cfg->pow_bits);
    T.xs = (uint32_t)xs.size();
    zkm_transcript_query_indices(ch, y.nq, (unsigned)y.lde_bits(), std::back_inserter(xs));

    T.d = y;
    T.slots = 4 + 2 * (uint32_t)y.L;
    const gl_t g = gl_root_of_unity(y.log_n);
    const gl2_t zeta_next = gl2_scalar_mul(ts.zeta, g);
    put(T.zeta, ts.zeta);
    put(T.zeta_next, zeta_next);
    put(T.fri_alpha, fri_alpha);
    put(T.apow_wa, gl2_pow(fri_alpha, y.W + y.A));
    put(T.apow_z, gl2_pow(fri_alpha, y.Z));
    // the reduced openings of the three batches (fri/verifier.rs PrecomputedReducedOpenings), each from its last value to its first
    const auto o = y.openings(proof);
    const gl2_t zero{0, 0}, at_zeta = reduce_more(reduce_more(zero, fri_alpha, o.quotient, y.Q, 2), fri_alpha, o.aux, y.A, 2);
    put(T.red_open[0], reduce_more(at_zeta, fri_alpha, o.local, y.W, 2));
    put(T.red_open[1], reduce_more(reduce_more(zero, fri_alpha, o.aux_next, y.A, 2), fri_alpha, o.next, y.W, 2));
    put(T.red_open[2], reduce_more(zero, fri_alpha, o.ctl_zs_first, y.Z, 1));
}

// the quotient comparison (verifier.rs:205-264) from the line accumulators of one table: acc[4 t + setting][challenge]
// returns the first challenge whose identity fails, or -1
int quotient_check(const zkm_stark_config* cfg, const table_state& ts, const uint64_t* proof, const gl_t* acc) {
    const zkm_blob_desc& y = ts.y;
    const gl_t g = gl_root_of_unity(y.log_n);
    const gl2_t zeta = ts.zeta, one{1, 0};
    const gl2_t zeta_n = gl2_exp_pow2(zeta, y.log_n), z_h = gl2_sub(zeta_n, one);
    const gl_t nn = (gl_t)(((uint64_t)1 << y.log_n) % GL_P);   // eval_l_0_and_l_last verifier.rs:344-354
    const gl2_t d0 = gl2_scalar_mul(gl2_sub(zeta, one), nn), d1 = gl2_scalar_mul(gl2_sub(gl2_scalar_mul(zeta, g), one), nn);
    const gl2_t z_last = gl2_sub(zeta, gl2_t{gl_inv(g), 0}), l_first = gl2_mul(z_h, gl2_inv(d0)), l_last = gl2_mul(z_h, gl2_inv(d1));
    const uint64_t* o_quot = y.openings(proof).quotient;
    for (unsigned a = 0; a < cfg->num_challenges; a++) {
        gl2_t cls[4];
        for (int setting = 0; setting < 4; setting++) {
            gl_t f[ZKM_VERIFY_LINE_POINTS];
            for (int t = 0; t < ZKM_VERIFY_LINE_POINTS; t++) {
                f[t] = acc[2 * (4 * t + setting) + a];
                if (setting) f[t] = gl_sub(f[t], acc[2 * (4 * t) + a]);   // the class alone: minus the plain constraints
            }
            if (!line_value(f, &cls[setting])) throw std::runtime_error("verify: constraint degree above 3");
        }
        const gl2_t lhs = gl2_add(gl2_add(cls[0], gl2_mul(cls[1], z_last)), gl2_add(gl2_mul(cls[2], l_first), gl2_mul(cls[3], l_last)));
        const gl2_t t0{o_quot[4 * a], o_quot[4 * a + 1]}, t1{o_quot[4 * a + 2], o_quot[4 * a + 3]};
        if (!gl2_eq(lhs, gl2_mul(z_h, gl2_add(t0, gl2_mul(t1, zeta_n))))) return (int)a;
    }
    return -1;
}

// verify_cross_table_lookups: per lookup and challenge, the looking tables' Z(1) add up to the looked table's
void check_ctl_sums(const zkm_stark_config* cfg, const verify_input& in, size_t ntables, const zkm_cross_table_lookup* ctls, const zkm_ctl_side* sides,
                    size_t nctls, seg_state& S) {
    std::vector<size_t> cursor(ntables, 0);
    auto first = [&](size_t t) {
        return S.ts[t].y.openings(in.proofs + S.ts[t].off).ctl_zs_first[cursor[t]++];
    };
    for (size_t c = 0; c < nctls; c++) {
        const zkm_ctl_side* lk = sides + ctls[c].looking_off;
        for (unsigned chn = 0; chn < cfg->num_challenges; chn++) {
            gl_t sum = 0;
            for (uint32_t i = 0; i < ctls[c].nlooking;) {
                uint32_t j = i;
                while (j < ctls[c].nlooking && lk[j].table == lk[i].table) j++;
                sum = gl_add(sum, first(lk[i].table));
                i = j;
            }
            if (sum != first(ctls[c].looked.table)) {
                S.rep.code = ZKM_VERIFY_CTL_SUM;
                S.rep.ctl = (uint32_t)c;
                S.rep.challenge = chn;
                S.rep.table = ctls[c].looked.table;
                S.msg = "cross-table lookup " + std::to_string(c) + ", challenge " + std::to_string(chn) + ": CTL verification failed (looked table " +
                        table_label(in.tables, ctls[c].looked.table) + ")";
                return;
            }
        }
    }
}

// The Merkle chains of a call's nent entries, ONE launch.  The hash chains do not depend on each other or on the arithmetic; a call of
// few chains costs the longest chain's latency (the Keccak table's leaf: 304 permutations), so it takes the four-lane form of the
// permutation; one that fills the machine one lane.  most_chains: the largest entry's chains, nchains: the call's
void launch_chains(zkm_ctx* c, const zkm_verify_chains* d_ents, size_t nent, uint32_t most_chains, size_t nchains, const gl_t* d_blobs,
                   const uint32_t* d_xs, uint32_t* d_verdicts) {
    zkm_prof_scope ps(c, "verify/merkle_chains");
    if (nchains <= c->quad_max_hashes)
        hipLaunchKernelGGL(k_verify_chains_quad, dim3((most_chains + 63) / 64, (unsigned)nent), dim3(256), 0, c->stream, d_ents, d_blobs, d_xs, d_verdicts);
    else
        hipLaunchKernelGGL(k_verify_chains, dim3((most_chains + 255) / 256, (unsigned)nent), dim3(256), 0, c->stream, d_ents, d_blobs, d_xs, d_verdicts);
    ZKM_HIP_CHECK(hipGetLastError());
}
void launch_reduce(zkm_ctx* c, const zkm_verify_chains* d_ents, size_t nent, const uint32_t* d_verdicts, uint32_t* d_first) {
    zkm_prof_scope ps(c, "verify/reduce");
    hipLaunchKernelGGL(k_verify_reduce, dim3((unsigned)nent), dim3(256), 0, c->stream, d_ents, d_verdicts, d_first);
    ZKM_HIP_CHECK(hipGetLastError());
}
// a first finding of k_verify_reduce -> the report's query, tree and layer, the code and the reference's wording (`who`: what the
// message starts with)
struct query_finding {
    uint32_t code, query, tree, layer;
    std::string text;
};
query_finding decode_finding(uint32_t f, const zkm_verify_chains& E, const std::string& who) {
    const uint32_t q = f / E.slots(), slot = f % E.slots(), initial = (uint32_t)E.fri.round.noracles;
    const std::string at = who + "query " + std::to_string(q) + ": ";
    if (slot < initial) return {ZKM_VERIFY_INITIAL_MERKLE, q, slot, 0, at + "Invalid Merkle proof. (initial oracle " + std::to_string(slot) + ")"};
    if (slot == E.slot_final()) return {ZKM_VERIFY_FINAL_POLY, q, 0, 0, at + "Final polynomial evaluation is invalid."};
    const uint32_t layer = (slot - initial) / 2;
    if ((slot - initial) % 2 == 0)
        return {ZKM_VERIFY_FRI_EVAL, q, 0, layer, at + "FRI layer " + std::to_string(layer) + ": the opened evaluation is not the folded one"};
    return {ZKM_VERIFY_FRI_MERKLE, q, 0, layer, at + "Invalid Merkle proof. (FRI layer " + std::to_string(layer) + ")"};
}

// `fixed`: the single-table form -- no transcript seeding, no CTL challenges and sums; *fixed holds the table's CtlZData list and
// `start` the caller's challenger (advanced only when the proof is accepted)
void verify_segments(zkm_ctx* c, const zkm_stark_config* cfg, size_t nseg, const verify_input* in, size_t ntables, const zkm_cross_table_lookup* ctls,
                     const zkm_ctl_side* sides, size_t nctls, bool check_heights, const std::vector<table_zs>* fixed, zkm_challenger* start,
                     std::vector<seg_state>& segs) {
    if (!cfg) throw std::runtime_error("verify: null configuration");
    if (nseg == 0 || ntables == 0) throw std::runtime_error("verify: nothing to verify");
    if (nseg * ntables > 65535) throw std::runtime_error("verify: at most 65535 (segment, table) pairs per call");
    if (cfg->num_challenges < 1 || cfg->num_challenges > 2) throw std::runtime_error("stark config: num_challenges must be 1 or 2");
    {   // a configuration the library does not support is a bad argument (FAILED), not a property of a blob
        (void)zkm_blob_describe(cfg, 32, 1, 1, 1);
    }
    const unsigned nch = cfg->num_challenges;
    const std::vector<table_zs> tz0 = fixed ? *fixed : zkm_derive_zs(ntables, ctls, sides, nctls, nch, nullptr);
    segs.assign(nseg, seg_state{});
    std::vector<zkm_verify_table> tabs;
    std::vector<uint32_t> xs;
    std::vector<size_t> launched;   // segments that reach the device
    for (size_t s = 0; s < nseg; s++) {
        seg_state& S = segs[s];
        S.ts.assign(ntables, table_state{});
        if (!in[s].tables || !in[s].proofs || (in[s].npub && !in[s].pub)) throw std::runtime_error("verify: segment " + std::to_string(s) + ": null argument");
        // (the transcript is replayed on the host from the blob's words)
        if (zkm_is_device_ptr(in[s].proofs)) throw std::runtime_error("verify: segment " + std::to_string(s) + ": the proof blobs must be in host memory");
        for (size_t t = 0; t < ntables; t++) {
            const zkm_table_input &a = in[s].tables[t], &b = in[0].tables[t];
            if (a.table_id != b.table_id || a.ncols != b.ncols || a.ctl != b.ctl)
                throw std::runtime_error("verify: the segments of one call must share the table list and its lookup description");
            if (a.ncols == 0 || a.ncols != zkm_table_width(a.table_id)) throw std::runtime_error("verify: unknown table id, or the width does not match the table");
        }
        if (!check_shapes(cfg, in[s], ntables, tz0, check_heights, S)) continue;
        if (fixed) {
            S.ch = *start;
            S.tz = *fixed;
        } else {
            zkm_transcript_seed(&S.ch, ntables, [&](size_t t) { return in[s].proofs + S.ts[t].off + S.ts[t].y.o_cap(0); }, S.ts[0].y.cap_words(),
                                in[s].pub, in[s].npub, nch, S.challenges);
            if (in[s].claimed && memcmp(S.challenges, in[s].claimed, sizeof(uint64_t) * 2 * nch) != 0) {
                reject(S, ZKM_VERIFY_CTL_CHALLENGES, 0, "the claimed CTL challenges are not the ones the transcript yields");
                continue;
            }
            S.tz = zkm_derive_zs(ntables, ctls, sides, nctls, nch, S.challenges);
        }
        S.launched = true;
        S.first_entry = tabs.size();
        launched.push_back(s);
        for (size_t t = 0; t < ntables; t++) {
            zkm_verify_table T{};
            replay_table(cfg, in[s], t, S, T, xs);
            tabs.push_back(T);
        }
    }
    if (tabs.empty()) return;   // (every segment was refused on the host: nothing is launched)

    const size_t nent = tabs.size();
    std::vector<zkm_verify_chains> ents(nent);
    size_t blob_words = 0, row_words = 0, nverdicts = 0, nchains = 0;
    for (size_t k = 0; k < launched.size(); k++) {
        const seg_state& S = segs[launched[k]];
        for (size_t t = 0; t < ntables; t++) {
            zkm_verify_table& T = tabs[S.first_entry + t];
            T.blob = blob_words + S.ts[t].off;
            T.rows = row_words;
            T.verdicts = (uint32_t)nverdicts;
            row_words += (size_t)ZKM_VERIFY_LINE_POINTS * 2 * (T.d.W + T.d.A);
            nverdicts += (size_t)T.d.nq * T.slots;
            // the STARK blob: three initial trees -- trace, auxiliary, quotient -- whose caps lie in the blob
            ents[S.first_entry + t] = zkm_verify_chains{T.blob, T.blob + T.d.o_cap(0), T.d.fri(), T.xs, T.verdicts};
            nchains += (size_t)T.d.nq * ents[S.first_entry + t].trees();
        }
        blob_words += S.ts[ntables - 1].off + S.ts[ntables - 1].y.total();
    }
    if (nverdicts >= ((uint64_t)1 << 32) || xs.size() >= ((uint64_t)1 << 32)) throw std::runtime_error("verify: too many queries in one call");
    const uint64_t waits_before = c->host_waits;
    // the parameter block: [entries | query indices | per group of <= ZKM_MAX_SEG segments and table: the CTL description with the group's
    // CtlZData lists]; the constraints of a table are ONE launch per group (the challenges travel as kernel arguments)
    struct line_launch {
        size_t t, G;
        ctl_dev_packed ctl;
        std::vector<uint64_t> lookup_ch, rows_off, acc_off;
        std::vector<gl_t> alphas;
    };
    const size_t tab_bytes = nent * sizeof(zkm_verify_table), ent_bytes = nent * sizeof(zkm_verify_chains), xs_bytes = (xs.size() * 4 + 15) & ~(size_t)15;
    std::vector<char> params(tab_bytes + ent_bytes + xs_bytes, 0);   // (alive until the download: the copy may read it after the call that queues it)
    memcpy(params.data(), tabs.data(), tab_bytes);
    memcpy(params.data() + tab_bytes, ents.data(), ent_bytes);
    if (!xs.empty()) memcpy(params.data() + tab_bytes + ent_bytes, xs.data(), xs.size() * 4);
    std::vector<line_launch> lines;
    for (size_t g0 = 0; g0 < launched.size(); g0 += ZKM_MAX_SEG) {
        const size_t G = std::min<size_t>(ZKM_MAX_SEG, launched.size() - g0);
        for (size_t t = 0; t < ntables; t++) {
            line_launch ll{t, G, {}, {}, std::vector<uint64_t>(G), std::vector<uint64_t>(G), {}};
            std::vector<zkm_ctl_z> zs;
            for (size_t k = 0; k < G; k++) {
                const seg_state& S = segs[launched[g0 + k]];
                zs.insert(zs.end(), S.tz[t].zs.begin(), S.tz[t].zs.end());
                for (unsigned a = 0; a < nch; a++) {
                    ll.lookup_ch.push_back(S.challenges[2 * a]);   // the betas of the CTL challenges (prover.rs:468-474)
                    ll.alphas.push_back(S.ts[t].alphas[a]);
                }
                ll.rows_off[k] = tabs[S.first_entry + t].rows;
                ll.acc_off[k] = (S.first_entry + t) * 2 * ZKM_VERIFY_LINE_THREADS;
            }
            ll.ctl = ctl_dev_pack(fixed ? nullptr : in[0].tables[t].ctl, zs.data(), tz0[t].ids.data(), tz0[t].zs.size(), false, in[0].tables[t].ncols, G,
                                  params);
            lines.push_back(std::move(ll));
        }
    }
    const size_t param_bytes = (params.size() + 15) & ~(size_t)15;
    const size_t acc_words = nent * 2 * ZKM_VERIFY_LINE_THREADS, out_bytes = (acc_words * 8 + nent * 4 + 15) & ~(size_t)15;
    // ONE device block going up: [parameter block | blobs]; scratch: line rows, verdict words; one block coming down: [line accumulators
    // | first findings].  Nothing between the first copy and the download waits for the device.
    zkm_scratch up(c, param_bytes + blob_words * 8), d_rows(c, row_words * 8), d_verdicts(c, nverdicts * 4), d_out(c, out_bytes);
    const zkm_verify_table* d_tabs = up.as<zkm_verify_table>();
    const zkm_verify_chains* d_ents = (const zkm_verify_chains*)(up.as<char>() + tab_bytes);
    const uint32_t* d_xs = (const uint32_t*)(up.as<char>() + tab_bytes + ent_bytes);
    gl_t* d_blobs = (gl_t*)(up.as<char>() + param_bytes);
    gl_t* d_acc = d_out.as<gl_t>();
    uint32_t* d_first = (uint32_t*)(d_acc + acc_words);
    {
        ZKM_HIP_CHECK(hipMemcpyAsync(up.p, params.data(), params.size(), hipMemcpyHostToDevice, c->stream));
        size_t at = 0;
        for (size_t s : launched) {
            const size_t words = segs[s].ts[ntables - 1].off + segs[s].ts[ntables - 1].y.total();
            ZKM_HIP_CHECK(hipMemcpyAsync(d_blobs + at, in[s].proofs, words * 8, hipMemcpyHostToDevice, c->stream));
            at += words;
        }
    }
    uint32_t most_cols = 0, most_chains = 0, most_q = 0;
    for (const zkm_verify_table& T : tabs) {
        most_cols = std::max(most_cols, (uint32_t)(T.d.W + T.d.A));
        most_chains = std::max(most_chains, (uint32_t)(T.d.nq * (3 + T.d.L)));   // (= nq * trees() of its entry)
        most_q = std::max(most_q, (uint32_t)T.d.nq);
    }
    {
        zkm_prof_scope ps(c, "verify/line_rows");
        hipLaunchKernelGGL(k_verify_rows, dim3((most_cols + 255) / 256, (unsigned)nent), dim3(256), 0, c->stream, d_tabs, (const gl_t*)d_blobs, d_rows.as<gl_t>());
        ZKM_HIP_CHECK(hipGetLastError());
    }
    for (const line_launch& ll : lines) {
        const zkm_verify_table& T0 = tabs[ll.acc_off[0] / (2 * ZKM_VERIFY_LINE_THREADS)];
        zkm_verify_line_constraints(c, in[0].tables[ll.t].table_id, nch, ctl_dev_rebase(ll.ctl.d, up.as<char>()), ll.ctl.naux, ll.lookup_ch.data(),
                                    ll.alphas.data(), d_rows.as<gl_t>(), ll.rows_off.data(), d_acc, ll.acc_off.data(), T0.d.W, T0.d.A, ll.G);
    }
    launch_chains(c, d_ents, nent, most_chains, nchains, d_blobs, d_xs, d_verdicts.as<uint32_t>());
    {
        zkm_prof_scope ps(c, "verify/fri_queries");
        hipLaunchKernelGGL(k_verify_fri, dim3((most_q + 63) / 64, (unsigned)nent), dim3(64), 0, c->stream, d_tabs, (const gl_t*)d_blobs, d_xs,
                           d_verdicts.as<uint32_t>());
        ZKM_HIP_CHECK(hipGetLastError());
    }
    launch_reduce(c, d_ents, nent, d_verdicts.as<uint32_t>(), d_first);
    std::vector<uint64_t> out(out_bytes / 8);
    c->download(out.data(), d_out.p, out_bytes);   // the call's one host wait
    const uint32_t waits = (uint32_t)(c->host_waits - waits_before);   // (counted where the context waits: zkm_ctx::sync / wait_flag / ensure_down)
    const gl_t* acc = out.data();
    const uint32_t* first = (const uint32_t*)(out.data() + acc_words);

    for (size_t s : launched) {
        seg_state& S = segs[s];
        S.rep.host_waits = waits;
        for (size_t t = 0; t < ntables && S.rep.code == ZKM_VERIFY_OK; t++) {
            const table_state& ts = S.ts[t];
            const std::string who = table_label(in[s].tables, t) + ": ";
            if (!ts.state_ok) {
                reject(S, ZKM_VERIFY_TRANSCRIPT_STATE, t, who + "the recorded challenger state is not the transcript's");
                break;
            }
            const int a = quotient_check(cfg, ts, in[s].proofs + ts.off, acc + (S.first_entry + t) * 2 * ZKM_VERIFY_LINE_THREADS);
            if (a >= 0) {
                reject(S, ZKM_VERIFY_QUOTIENT, t, who + "Mismatch between evaluation and opening of quotient polynomial");
                S.rep.challenge = (uint32_t)a;
                break;
            }
            if (!ts.pow_ok) {
                reject(S, ZKM_VERIFY_POW, t, who + "Invalid proof of work witness.");
                break;
            }
            const uint32_t f = first[S.first_entry + t];
            if (f == ~0u) continue;
            const query_finding found = decode_finding(f, ents[S.first_entry + t], who);
            reject(S, found.code, t, found.text);
            S.rep.query = found.query;
            S.rep.tree = found.tree;
            S.rep.layer = found.layer;
        }
        if (S.rep.code == ZKM_VERIFY_OK && !fixed) check_ctl_sums(cfg, in[s], ntables, ctls, sides, nctls, S);
    }
    if (fixed && segs[0].rep.code == ZKM_VERIFY_OK) *start = segs[0].ch;
}

int finish(const char* what, const std::vector<seg_state>& segs, zkm_verify_report* reports, char** err, const char* unit /* "segment", "proof" or null */) {
    if (reports)
        for (size_t s = 0; s < segs.size(); s++) reports[s] = segs[s].rep;
    for (size_t s = 0; s < segs.size(); s++)
        if (segs[s].rep.code != ZKM_VERIFY_OK) {
            const std::string m = std::string(what) + ": " + (unit ? std::string(unit) + " " + std::to_string(s) + ": " : "") + segs[s].msg + " [" +
                                  CODE_NAMES[segs[s].rep.code] + "]";
            return zkm_fail(err, m.c_str());
        }
    return 0;
}
// a call that could not be made: every report says FAILED, the message goes out through the error channel
template <class F> int guarded(const char* what, zkm_ctx* c, zkm_verify_report* reports, size_t nreports, char** err, F&& body) {
    int rc = 0;
    bool threw = true;
    const int st = zkm_api(what, c, err, [&] {
        rc = body();
        threw = false;
    });
    if (!threw) return rc;
    if (reports)
        for (size_t s = 0; s < nreports; s++) {
            reports[s] = zkm_verify_report{};
            reports[s].code = ZKM_VERIFY_FAILED;
        }
    return st ? st : 1;
}

// ------------------------------------------------------------------ zkm_fri_verify: verify_fri_proof for any instance
struct fri_claim_in {
    const uint64_t* proof;
    size_t proof_words;
    unsigned log_n;
    const size_t* cols;
    size_t noracles;
    const uint64_t* const* caps;
    const zkm_fri_batch* batches;
    size_t nbatches;
    const uint64_t* const* opened;
    zkm_challenger* challenger;
};
// every SHAPE finding of one claim (include/zkm_hip.h), in the header's order; empty when the device may index the blob with y
std::string fri_claim_shape(const zkm_stark_config* cfg, const fri_claim_in& in, const zkm_fri_part& y) {
    if (in.proof_words < ZKM_FRI_BLOB_HEADER_WORDS) return "proof_words too short for the header";
    if (in.proof[0] != ZKM_FRI_PROOF_MAGIC) return "no FRI proof header (magic)";
    uint64_t want[ZKM_FRI_BLOB_HEADER_WORDS];
    zkm_fri_blob_header_write(want, cfg, in.log_n, y);
    for (int i = 1; i < ZKM_FRI_BLOB_HEADER_WORDS; i++)
        if ((i <= 8 || i >= 16) && in.proof[i] != want[i]) return "header word " + std::to_string(i) + " does not match the configuration and the oracles";
    const size_t total = y.total();
    if (!y.round.fits() || y.round.L > ZKM_FRI_HEADER_LAYERS || y.round.lde_bits > 31 || total >= ((uint64_t)1 << 32)) return "unsupported FRI shape";
    if (in.proof_words < total) return "proof_words too short";
    for (size_t i = 1; i < total; i++)
        if (in.proof[i] >= GL_P) return "word " + std::to_string(i) + " is not a canonical field element";
    for (size_t k = 0; k < in.noracles; k++)
        for (size_t i = 0; i < y.cap_words; i++)
            if (in.caps[k][i] >= GL_P) return "word " + std::to_string(i) + " of the cap of oracle " + std::to_string(k) + " is not a canonical field element";
    for (size_t b = 0; b < in.nbatches; b++) {
        if (in.batches[b].point[0] >= GL_P || in.batches[b].point[1] >= GL_P) return "the point of batch " + std::to_string(b) + " is not a canonical field element";
        for (size_t i = 0; i < 2 * in.batches[b].npolys; i++)
            if (in.opened[b][i] >= GL_P) return "word " + std::to_string(i) + " of the opened values of batch " + std::to_string(b) + " is not a canonical field element";
    }
    return "";
}

void fri_verify_claims(zkm_ctx* c, const zkm_stark_config* cfg, size_t n, const fri_claim_in* in, std::vector<seg_state>& claims) {
    if (!cfg) throw std::runtime_error("zkm_fri_verify: null configuration");
    if (n == 0) throw std::runtime_error("zkm_fri_verify: nothing to verify");
    if (n > 65535) throw std::runtime_error("zkm_fri_verify: at most 65535 proofs per call");
    claims.assign(n, seg_state{});
    std::vector<zkm_verify_chains> ents;
    std::vector<fri_claim_dev> devs;
    std::vector<uint32_t> polys, xs;
    std::vector<size_t> launched;
    std::vector<bool> pow_ok;
    size_t words = 0, nverdicts = 0, nchains = 0;   // of the call's device block of field words: per launched claim its caps, then its blob
    uint32_t most_chains = 0, most_q = 0;
    for (size_t i = 0; i < n; i++) {
        const fri_claim_in& a = in[i];
        const std::string who = "zkm_fri_verify: proof " + std::to_string(i) + ": ";
        // ---- what makes the call impossible (FAILED)
        if (!a.proof || !a.cols || !a.caps || !a.batches || !a.opened || !a.challenger) throw std::runtime_error(who + "null argument");
        if (a.noracles == 0 || a.noracles > ZKM_FRI_MAX_ORACLES) throw std::runtime_error(who + "1..8 oracles");
        if (a.nbatches == 0 || a.nbatches > FRI_CLAIM_BATCHES) throw std::runtime_error(who + "1..8 opening batches");
        if (zkm_is_device_ptr(a.proof)) throw std::runtime_error(who + "the proof blob must be in host memory");
        for (size_t k = 0; k < a.noracles; k++) {
            if (!a.caps[k]) throw std::runtime_error(who + "null argument");
            if (zkm_is_device_ptr(a.caps[k])) throw std::runtime_error(who + "the caps must be in host memory");
        }
        for (size_t b = 0; b < a.nbatches; b++) {
            if (a.batches[b].npolys == 0 || !a.batches[b].polys) throw std::runtime_error(who + "empty batch");
            if (!a.opened[b]) throw std::runtime_error(who + "null argument");
            if (zkm_is_device_ptr(a.opened[b])) throw std::runtime_error(who + "the opened values must be in host memory");
            for (size_t j = 0; j < a.batches[b].npolys; j++)
                if (a.batches[b].polys[j].oracle >= a.noracles || a.batches[b].polys[j].poly >= a.cols[a.batches[b].polys[j].oracle])
                    throw std::runtime_error(who + "polynomial index out of range");
        }
        const zkm_fri_part y = zkm_fri_blob_describe(cfg, a.log_n, a.cols, a.noracles);   // (throws on a configuration the library refuses)
        // ---- what is wrong with the claim (SHAPE): it reaches no kernel
        seg_state& S = claims[i];
        const std::string shape = fri_claim_shape(cfg, a, y);
        if (!shape.empty()) {
            reject(S, ZKM_VERIFY_SHAPE, 0, "malformed proof: " + shape);
            continue;
        }
        const zkm_query_round& R = y.round;
        for (size_t b = 0; b < a.nbatches; b++) {   // plonky2 divides by x - point for every x of the coset g H
            const gl_t z = a.batches[b].point[0];
            if (a.batches[b].point[1] == 0 && gl_exp_pow2(gl_mul(z, gl_inv(GL_GENERATOR)), (unsigned)R.lde_bits) == 1)
                throw std::runtime_error(who + "the point of batch " + std::to_string(b) + " lies on the LDE coset");
        }
        // ---- the transcript, from the blob alone: alpha; per layer the cap, then beta; the final polynomial; the witness; the indices
        S.ch = *a.challenger;
        zkm_verify_chains E{};
        fri_claim_dev K{};
        auto put = [](gl_t* dst, gl2_t v) { dst[0] = v.c0; dst[1] = v.c1; };
        const gl2_t alpha = zkm_challenger_get_ext(&S.ch);
        put(K.alpha, alpha);
        for (unsigned l = 0; l < R.L; l++) put(K.betas[l], zkm_transcript_fri_beta(&S.ch, a.proof + y.o_cap(l), y.cap_words));
        zkm_transcript_final_poly(&S.ch, a.proof + y.o_final(), y.F);
        pow_ok.push_back(zkm_transcript_pow(&S.ch, a.proof[y.o_pow()], cfg->pow_bits));
        E.xs = (uint32_t)xs.size();
        zkm_transcript_query_indices(&S.ch, y.nq, (unsigned)R.lde_bits, std::back_inserter(xs));
        // ---- the instance: reduced openings (PrecomputedReducedOpenings), alpha^npolys, the polynomials as offsets into a query round
        K.nbatches = (uint32_t)a.nbatches;
        for (size_t b = 0; b < a.nbatches; b++) {
            const zkm_fri_batch& B = a.batches[b];
            fri_claim_batch& o = K.b[b];
            o.point[0] = B.point[0];
            o.point[1] = B.point[1];
            put(o.red_open, reduce_more(gl2_t{0, 0}, alpha, a.opened[b], B.npolys, 2));
            put(o.shift, gl2_pow(alpha, B.npolys));
            o.first = (uint32_t)polys.size();
            o.npolys = (uint32_t)B.npolys;
            for (size_t j = 0; j < B.npolys; j++) polys.push_back((uint32_t)(R.oracle_evals(B.polys[j].oracle) + B.polys[j].poly));
        }
        E.fri = y;
        E.caps = words;
        E.blob = words + a.noracles * y.cap_words;
        E.verdicts = (uint32_t)nverdicts;
        words = E.blob + y.total();
        nverdicts += (size_t)y.nq * E.slots();
        nchains += (size_t)y.nq * E.trees();
        most_chains = std::max(most_chains, (uint32_t)(y.nq * E.trees()));
        most_q = std::max(most_q, (uint32_t)y.nq);
        S.launched = true;
        S.first_entry = ents.size();
        launched.push_back(i);
        ents.push_back(E);
        devs.push_back(K);
    }
    if (ents.empty()) return;   // (every claim was refused on the host: nothing is launched)
    if (nverdicts >= ((uint64_t)1 << 32) || xs.size() >= ((uint64_t)1 << 32) || polys.size() >= ((uint64_t)1 << 32))
        throw std::runtime_error("zkm_fri_verify: too many queries in one call");

    const uint64_t waits_before = c->host_waits;
    // ONE device block going up: [descriptions | claims | polynomial lists | query indices | per claim: caps, blob]; one word per claim
    // coming down.  Nothing between the first copy and the download waits for the device.
    const size_t nent = ents.size(), ent_bytes = nent * sizeof(zkm_verify_chains), dev_bytes = nent * sizeof(fri_claim_dev);
    const size_t poly_bytes = (polys.size() * 4 + 15) & ~(size_t)15, xs_bytes = (xs.size() * 4 + 15) & ~(size_t)15;
    const size_t param_bytes = (ent_bytes + dev_bytes + poly_bytes + xs_bytes + 15) & ~(size_t)15;
    std::vector<char> params(param_bytes, 0);   // (alive until the download: the copy may read it after the call that queues it)
    memcpy(params.data(), ents.data(), ent_bytes);
    memcpy(params.data() + ent_bytes, devs.data(), dev_bytes);
    memcpy(params.data() + ent_bytes + dev_bytes, polys.data(), polys.size() * 4);
    memcpy(params.data() + ent_bytes + dev_bytes + poly_bytes, xs.data(), xs.size() * 4);
    zkm_scratch up(c, param_bytes + words * 8), d_verdicts(c, nverdicts * 4), d_out(c, (nent * 4 + 15) & ~(size_t)15);
    const zkm_verify_chains* d_ents = up.as<zkm_verify_chains>();
    const fri_claim_dev* d_devs = (const fri_claim_dev*)(up.as<char>() + ent_bytes);
    const uint32_t* d_polys = (const uint32_t*)(up.as<char>() + ent_bytes + dev_bytes);
    const uint32_t* d_xs = (const uint32_t*)(up.as<char>() + ent_bytes + dev_bytes + poly_bytes);
    gl_t* d_blobs = (gl_t*)(up.as<char>() + param_bytes);
    ZKM_HIP_CHECK(hipMemcpyAsync(up.p, params.data(), params.size(), hipMemcpyHostToDevice, c->stream));
    for (size_t k = 0; k < nent; k++) {
        const fri_claim_in& a = in[launched[k]];
        const zkm_verify_chains& E = ents[k];
        for (size_t t = 0; t < a.noracles; t++)
            ZKM_HIP_CHECK(hipMemcpyAsync(d_blobs + E.caps + t * E.fri.cap_words, a.caps[t], E.fri.cap_words * 8, hipMemcpyHostToDevice, c->stream));
        ZKM_HIP_CHECK(hipMemcpyAsync(d_blobs + E.blob, a.proof, E.fri.total() * 8, hipMemcpyHostToDevice, c->stream));
    }
    launch_chains(c, d_ents, nent, most_chains, nchains, d_blobs, d_xs, d_verdicts.as<uint32_t>());
    {
        zkm_prof_scope ps(c, "verify/fri_instance_queries");
        hipLaunchKernelGGL(k_fri_verify_queries, dim3((most_q + 63) / 64, (unsigned)nent), dim3(64), 0, c->stream, d_ents, d_devs, d_polys, (const gl_t*)d_blobs,
                           d_xs, d_verdicts.as<uint32_t>());
        ZKM_HIP_CHECK(hipGetLastError());
    }
    launch_reduce(c, d_ents, nent, d_verdicts.as<uint32_t>(), d_out.as<uint32_t>());
    std::vector<uint32_t> first(nent);
    c->download(first.data(), d_out.p, nent * 4);   // the call's one host wait
    const uint32_t waits = (uint32_t)(c->host_waits - waits_before);

    for (size_t k = 0; k < nent; k++) {
        seg_state& S = claims[launched[k]];
        S.rep.host_waits = waits;
        if (!pow_ok[k]) {
            reject(S, ZKM_VERIFY_POW, 0, "Invalid proof of work witness.");
        } else if (first[k] != ~0u) {
            const query_finding found = decode_finding(first[k], ents[k], "");
            reject(S, found.code, 0, found.text);
            S.rep.query = found.query;
            S.rep.tree = found.tree;
            S.rep.layer = found.layer;
        } else {
            *in[launched[k]].challenger = S.ch;   // accepted: the state zkm_fri_prove leaves
        }
    }
}

}  // namespace

size_t zkm_verify_run(zkm_ctx* c, const zkm_stark_config* cfg, size_t nseg, const zkm_table_input* const* tables, size_t ntables,
                      const zkm_cross_table_lookup* ctls, const zkm_ctl_side* sides, size_t nctls, const uint64_t* const* pub, const size_t* npub,
                      const uint64_t* const* proofs, const size_t* proof_words, const uint64_t* const* challenges, std::string* msg) {
    std::vector<verify_input> in(nseg);
    for (size_t s = 0; s < nseg; s++) in[s] = verify_input{tables[s], pub[s], npub[s], proofs[s], proof_words[s], challenges[s]};
    std::vector<seg_state> segs;
    verify_segments(c, cfg, nseg, in.data(), ntables, ctls, sides, nctls, true, nullptr, nullptr, segs);
    for (size_t s = 0; s < nseg; s++)
        if (segs[s].rep.code != ZKM_VERIFY_OK) {
            if (msg) *msg = segs[s].msg + " [" + CODE_NAMES[segs[s].rep.code] + "]";
            return s;
        }
    return nseg;
}

extern "C" {

int zkm_verify_proofs(zkm_ctx* c, const zkm_stark_config* cfg, const zkm_table_input* tables, size_t ntables, const zkm_cross_table_lookup* ctls,
                      const zkm_ctl_side* sides, size_t nctls, const uint64_t* pub, size_t npub, const uint64_t* proofs, size_t proof_words,
                      const uint64_t* ctl_challenges, zkm_verify_report* report, char** err) {
    return guarded("zkm_verify_proofs", c, report, 1, err, [&] {
        if (!cfg || !tables || !proofs || (nctls && (!ctls || !sides)) || (npub && !pub)) throw std::runtime_error("zkm_verify_proofs: null argument");
        const verify_input in{tables, pub, npub, proofs, proof_words, ctl_challenges};
        std::vector<seg_state> segs;
        verify_segments(c, cfg, 1, &in, ntables, ctls, sides, nctls, true, nullptr, nullptr, segs);
        return finish("zkm_verify_proofs", segs, report, err, nullptr);
    });
}

int zkm_verify_segments(zkm_ctx* c, const zkm_stark_config* cfg, size_t nseg, const uint64_t* const* proofs, const size_t* proof_words,
                        const uint64_t* const* pub, const size_t* npub, const uint64_t* const* ctl_challenges, zkm_verify_report* reports, char** err) {
    return guarded("zkm_verify_segments", c, reports, nseg, err, [&] {
        if (!cfg || !proofs || !proof_words || nseg == 0) throw std::runtime_error("zkm_verify_segments: null argument");
        zkm_table_input tables[ZKM_NUM_TABLES];
        zkm_all_stark_table_inputs(tables);
        const zkm_cross_table_lookup* ctls;
        const zkm_ctl_side* sides;
        size_t nctls, nsides;
        zkm_all_stark_ctls(&ctls, &nctls, &sides, &nsides);
        std::vector<verify_input> in(nseg);
        for (size_t s = 0; s < nseg; s++) {
            if (!proofs[s]) throw std::runtime_error("zkm_verify_segments: null segment");
            in[s] = verify_input{tables, pub ? pub[s] : nullptr, npub ? npub[s] : 0, proofs[s], proof_words[s], ctl_challenges ? ctl_challenges[s] : nullptr};
            if (in[s].npub && !in[s].pub) throw std::runtime_error("zkm_verify_segments: null public values");
        }
        std::vector<seg_state> segs;
        verify_segments(c, cfg, nseg, in.data(), ZKM_NUM_TABLES, ctls, sides, nctls, false, nullptr, nullptr, segs);
        return finish("zkm_verify_segments", segs, reports, err, "segment");
    });
}

int zkm_verify_single_table(zkm_ctx* c, int table_id, const zkm_stark_config* cfg, const uint64_t* proof, size_t proof_words, size_t ncols, size_t naux,
                            const uint32_t* num_helpers, size_t nctl_zs, zkm_challenger* challenger, zkm_verify_report* report, char** err) {
    return guarded("zkm_verify_single_table", c, report, 1, err, [&] {
        if (!cfg || !proof || !challenger || (nctl_zs && !num_helpers)) throw std::runtime_error("zkm_verify_single_table: null argument");
        // CtlZData of the benchmark's fake CTL shape: helper columns, no column sets (poseidon_stark.rs:786-799)
        std::vector<table_zs> fixed(1);
        for (size_t i = 0; i < nctl_zs; i++) {
            if (num_helpers[i] == 0) throw std::runtime_error("zkm_verify_single_table: CTLs without helper columns need column sets: use zkm_verify_proofs");
            fixed[0].zs.push_back(zkm_ctl_z{0, 0, num_helpers[i], 0, 0, 0});
            fixed[0].naux += num_helpers[i] + 1;
        }
        if (fixed[0].naux != naux) throw std::runtime_error("zkm_verify_single_table: naux does not match the helper columns");
        if (zkm_num_lookup_columns(table_id, cfg)) throw std::runtime_error("zkm_verify_single_table: a table with lookups of its own needs zkm_verify_proofs");
        const zkm_table_input table{table_id, nullptr, ncols, 0, nullptr, nullptr};
        const verify_input in{&table, nullptr, 0, proof, proof_words, nullptr};
        std::vector<seg_state> segs;
        zkm_challenger local = *challenger;
        verify_segments(c, cfg, 1, &in, 1, nullptr, nullptr, 0, false, &fixed, &local, segs);
        const int rc = finish("zkm_verify_single_table", segs, report, err, nullptr);
        if (!rc) *challenger = local;
        return rc;
    });
}

int zkm_fri_verify(zkm_ctx* c, const zkm_stark_config* cfg, size_t nproofs, const uint64_t* const* proofs, const size_t* proof_words, const unsigned* log_n,
                   const size_t* const* oracle_cols, const size_t* noracles, const uint64_t* const* const* oracle_caps, const zkm_fri_batch* const* batches,
                   const size_t* nbatches, const uint64_t* const* const* opened, zkm_challenger* const* challengers, zkm_verify_report* reports, char** err) {
    return guarded("zkm_fri_verify", c, reports, nproofs, err, [&] {
        if (!cfg || !proofs || !proof_words || !log_n || !oracle_cols || !noracles || !oracle_caps || !batches || !nbatches || !opened || !challengers ||
            nproofs == 0)
            throw std::runtime_error("zkm_fri_verify: null argument");
        std::vector<fri_claim_in> in(nproofs);
        for (size_t i = 0; i < nproofs; i++)
            in[i] = fri_claim_in{proofs[i], proof_words[i], log_n[i], oracle_cols[i], noracles[i], oracle_caps[i], batches[i], nbatches[i], opened[i], challengers[i]};
        std::vector<seg_state> claims;
        fri_verify_claims(c, cfg, nproofs, in.data(), claims);
        return finish("zkm_fri_verify", claims, reports, err, "proof");
    });
}

}  // extern "C"
