// proof_blob.h -- the proof blob as a data format (include/zkm_hip.h "Proof blob") and the order of the Fiat-Shamir transcript: the one
// place that knows where a field lies and what is observed when, for the prover, the verifier and the layout accessors alike.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/zkm_hip.h"
#include "gl_dev.h"

#define ZKM_FRI_MAX_ORACLES 8      // initial oracles of one FRI proof
#define ZKM_FRI_GATHER_LAYERS 8    // layers the prover's query gather takes (its descriptors travel as kernel arguments)
#define ZKM_FRI_HEADER_LAYERS 16   // layers a header may claim (zkm_proof_query_layout's arrays, the verifier's betas)

// ---- one query round: per initial oracle its row and the Merkle path (FriInitialTreeProof), then per layer the coset's 2^arity_bits F2
// values and the path (FriQueryStep).  Offsets are words from the start of the round; sibling counts are digests of 4 words.  Serves the
// STARK blob (trace, auxiliary, quotient) and the FRI-only blob of zkm_fri_prove.
struct zkm_query_round {
    uint64_t cols[ZKM_FRI_MAX_ORACLES];
    uint64_t noracles, L, lde_bits, cap_height, arity_bits;
    GL_HD uint64_t initial_siblings() const { return lde_bits - cap_height; }
    GL_HD bool fits() const {   // a header may claim more layers than the tree has levels: such a round has no layout
        for (uint64_t l = 0; l < L; l++)
            if (lde_bits < arity_bits * (l + 1) + cap_height) return false;
        return lde_bits >= cap_height;
    }
    GL_HD uint64_t layer_sibling_count(uint64_t l) const { return lde_bits - arity_bits * (l + 1) - cap_height; }
    GL_HD uint64_t layer_values() const { return (uint64_t)2 << arity_bits; }
    GL_HD uint64_t oracle_evals(uint64_t k) const {
        uint64_t o = 0;
        for (uint64_t i = 0; i < k; i++) o += cols[i] + 4 * initial_siblings();
        return o;
    }
    GL_HD uint64_t oracle_siblings(uint64_t k) const { return oracle_evals(k) + cols[k]; }
    GL_HD uint64_t layer_evals(uint64_t l) const {
        uint64_t o = oracle_evals(noracles);
        for (uint64_t i = 0; i < l; i++) o += layer_values() + 4 * layer_sibling_count(i);
        return o;
    }
    GL_HD uint64_t layer_siblings(uint64_t l) const { return layer_evals(l) + layer_values(); }
    GL_HD uint64_t words() const { return layer_evals(L); }
};

// ---- what both blobs end in, from word `base` on: the FRI layers' caps, the final polynomial, the proof-of-work witness, nq query rounds
struct zkm_fri_part {
    uint64_t base, cap_words, F, nq;
    zkm_query_round round;
    GL_HD uint64_t o_cap(uint64_t l) const { return base + l * cap_words; }
    GL_HD uint64_t o_final() const { return o_cap(round.L); }
    GL_HD uint64_t o_pow() const { return o_final() + 2 * F; }
    GL_HD uint64_t o_queries() const { return o_pow() + 1; }
    GL_HD uint64_t o_query(uint64_t q) const { return o_queries() + q * round.words(); }
    GL_HD uint64_t total() const { return o_query(nq); }
};

// ---- StarkOpeningSet (proof.rs:281-297) behind `base`, a pointer into a blob or a word offset: F2 values of two words, ctl_zs_first of one
template <class P> struct zkm_opening_set {
    P local, next, aux, aux_next, ctl_zs_first, quotient, end;
    GL_HD zkm_opening_set(P base, uint64_t W, uint64_t A, uint64_t Z, uint64_t Q)
        : local(base), next(local + 2 * W), aux(next + 2 * W), aux_next(aux + 2 * A), ctl_zs_first(aux_next + 2 * A), quotient(ctl_zs_first + Z),
          end(quotient + 2 * Q) {}
};

// ---- the blob: what its header says, and from that where every field lies (word offsets from the start of the blob)
struct zkm_blob_desc {
    uint64_t log_n, W, A, Q, Z, cap_height, L, F, nq, rate_bits, arity_bits;   // header words 1 .. 11, in this order
    GL_HD uint64_t lde_bits() const { return log_n + rate_bits; }
    GL_HD uint64_t cap_words() const { return (uint64_t)4 << cap_height; }
    GL_HD uint64_t o_init() const { return 16; }                              // the compacted challenger state, 12 words
    GL_HD uint64_t o_cap(uint64_t tree) const { return o_init() + 12 + tree * cap_words(); }   // 0 trace, 1 auxiliary, 2 quotient
    GL_HD uint64_t o_open() const { return o_cap(3); }
    template <class P> GL_HD zkm_opening_set<P> openings(P blob) const { return zkm_opening_set<P>(blob + o_open(), W, A, Z, Q); }
    GL_HD zkm_query_round round() const { return zkm_query_round{{W, A, Q}, 3, L, lde_bits(), cap_height, arity_bits}; }
    GL_HD zkm_fri_part fri() const { return zkm_fri_part{openings((uint64_t)0).end, cap_words(), F, nq, round()}; }
    GL_HD uint64_t total() const { return fri().total(); }
};
// (cfg, log_n, W, A, Z) -> description; validates the configuration and throws on one the library does not support (stark.hip)
zkm_blob_desc zkm_blob_describe(const zkm_stark_config* cfg, unsigned log_n, size_t W, size_t A, size_t Z);
// the FRI-only blob of zkm_fri_prove: 24 header words (its own magic, the oracles' column counts from word 16), then the FRI part;
// validates like zkm_blob_describe (stark.hip)
#define ZKM_FRI_BLOB_HEADER_WORDS 24
zkm_fri_part zkm_fri_blob_describe(const zkm_stark_config* cfg, unsigned log_n, const size_t* cols, size_t noracles);
inline void zkm_fri_blob_header_write(uint64_t* p, const zkm_stark_config* cfg, unsigned log_n, const zkm_fri_part& y) {
    const uint64_t h[ZKM_FRI_BLOB_HEADER_WORDS] = {ZKM_FRI_PROOF_MAGIC, log_n, y.round.noracles, cfg->cap_height, y.round.L, y.F, cfg->num_queries,
                                                   cfg->rate_bits, cfg->arity_bits};
    memcpy(p, h, sizeof h);
    for (uint64_t k = 0; k < y.round.noracles; k++) p[16 + k] = y.round.cols[k];
}
// the 16 header words; a caller reading a header it did not write validates what it got
inline void zkm_blob_header_write(uint64_t* p, const zkm_blob_desc& d) {
    const uint64_t h[16] = {ZKM_PROOF_MAGIC, d.log_n, d.W, d.A, d.Q, d.Z, d.cap_height, d.L, d.F, d.nq, d.rate_bits, d.arity_bits, 0, 0, 0, 0};
    memcpy(p, h, sizeof h);
}
inline zkm_blob_desc zkm_blob_header_read(const uint64_t* p) {
    return zkm_blob_desc{p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], p[10], p[11]};
}

// ---- the transcript, step by step (host): the prover runs a step once the field it observes is in the blob, the verifier all at once
inline gl2_t zkm_challenger_get_ext(zkm_challenger* ch) {
    const gl_t a = zkm_challenger_get(ch), b = zkm_challenger_get(ch);
    return gl2_t{a, b};
}
// a segment's start: all trace caps in table order, the public values, then beta and gamma per challenge (prover.rs:182-190,
// AllProof::get_challenges get_challenges.rs:128-137, cross_table_lookup.rs:560-566); trace_cap(t) -> table t's cap
template <class CapOf> void zkm_transcript_seed(zkm_challenger* ch, size_t ntables, CapOf trace_cap, size_t cap_words, const uint64_t* pub, size_t npub,
                                                unsigned num_challenges, uint64_t* ctl_challenges) {
    zkm_challenger_init(ch);
    for (size_t t = 0; t < ntables; t++) zkm_challenger_observe(ch, trace_cap(t), cap_words);
    zkm_challenger_observe(ch, pub, npub);
    for (unsigned k = 0; k < 2 * num_challenges; k++) ctl_challenges[k] = zkm_challenger_get(ch);
}
// auxiliary cap -> the constraint challenges (prover.rs:525-527, get_challenges.rs:213-215)
inline void zkm_transcript_alphas(zkm_challenger* ch, const zkm_blob_desc& d, const uint64_t* blob, unsigned num_challenges, gl_t* alphas) {
    zkm_challenger_observe(ch, blob + d.o_cap(1), d.cap_words());
    for (unsigned i = 0; i < num_challenges; i++) alphas[i] = zkm_challenger_get(ch);
}
// quotient cap -> zeta (prover.rs:589-591, get_challenges.rs:217-218)
inline gl2_t zkm_transcript_zeta(zkm_challenger* ch, const zkm_blob_desc& d, const uint64_t* blob) {
    zkm_challenger_observe(ch, blob + d.o_cap(2), d.cap_words());
    return zkm_challenger_get_ext(ch);
}
// observe_openings(to_fri_openings) -> the FRI alpha (get_challenges.rs:220, proof.rs:336-367, then the first draw of plonky2's
// fri_challenges, get_challenges.rs:225): the batch at zeta, the batch at g zeta, then the ctl_zs_first lifted to F2
inline gl2_t zkm_transcript_fri_alpha(zkm_challenger* ch, const zkm_blob_desc& d, const uint64_t* blob) {
    const auto o = d.openings(blob);
    zkm_challenger_observe(ch, o.local, 2 * d.W);
    zkm_challenger_observe(ch, o.aux, 2 * d.A);
    zkm_challenger_observe(ch, o.quotient, 2 * d.Q);
    zkm_challenger_observe(ch, o.next, 2 * d.W);
    zkm_challenger_observe(ch, o.aux_next, 2 * d.A);
    for (size_t i = 0; i < d.Z; i++) { const uint64_t e[2] = {o.ctl_zs_first[i], 0}; zkm_challenger_observe(ch, e, 2); }
    return zkm_challenger_get_ext(ch);
}
// the FRI steps (plonky2 fri/challenges.rs fri_challenges) take the fields themselves: they serve zkm_fri_prove's blob too
inline gl2_t zkm_transcript_fri_beta(zkm_challenger* ch, const uint64_t* layer_cap, size_t cap_words) {
    zkm_challenger_observe(ch, layer_cap, cap_words);
    return zkm_challenger_get_ext(ch);
}
inline void zkm_transcript_final_poly(zkm_challenger* ch, const uint64_t* final_poly, size_t F) { zkm_challenger_observe(ch, final_poly, 2 * F); }
// witness -> response; true when the response has its pow_bits leading zeros (fri_verify_proof_of_work)
inline bool zkm_transcript_pow(zkm_challenger* ch, uint64_t witness, unsigned pow_bits) {
    zkm_challenger_observe(ch, &witness, 1);
    return (zkm_challenger_get(ch) >> (64 - pow_bits)) == 0;
}
template <class Out> void zkm_transcript_query_indices(zkm_challenger* ch, size_t nq, unsigned lde_bits, Out out) {
    for (size_t q = 0; q < nq; q++) *out++ = (uint32_t)(zkm_challenger_get(ch) % ((uint64_t)1 << lde_bits));
}
