/* tools/abi_layout.c -- prints sizeof / alignment / offsetof of every struct of include/zkm_hip.h as one JSON object.
 *
 * The C ABI has three mirrors that no compiler checks against each other: this header, the ctypes Structures / numpy dtypes in
 * zkm_amd/, and the #[repr(C)] structs in integration/rust/zkm_hip_sys.rs (uncompiled here: no Rust in the image).
 * tests/test_abi.py builds this file with gcc, runs it, and compares all three -- a reordered or re-typed field fails on the CPU
 * instead of corrupting memory on a maintainer's first run.  Built by oracle/Makefile (target abi_layout) and by the test itself.
 */
#include <stddef.h>
#include <stdio.h>

#include "../include/zkm_hip.h"

#define ALIGN_OF(T) offsetof(struct { char c; T t; }, t)
#define FIELD(T, f) printf("%s[\"%s\", %zu, %zu]", first_field ? "" : ", ", #f, offsetof(T, f), sizeof(((T*)0)->f)), first_field = 0
#define BEGIN(T) printf("%s\n  \"%s\": {\"size\": %zu, \"align\": %zu, \"fields\": [", first_struct ? "" : ",", #T, sizeof(T), ALIGN_OF(T)), \
                 first_struct = 0, first_field = 1
#define END() printf("]}")

/* The K-segment entry points held to the argument types their callers (ctypes, Rust, C) rely on: a changed prototype fails this
 * file's build.  The assignments sit inside sizeof -- type-checked, never evaluated -- so the file still links without the library. */
static void check_segments_ops_prototypes(void) {
    int (*tables)(zkm_ctx*, const zkm_stark_config*, size_t, const zkm_segment_ops*, unsigned*, zkm_staged**, char**) = 0;
    int (*prove)(zkm_ctx*, const zkm_stark_config*, size_t, const zkm_segment_ops*, const uint64_t* const*, const size_t*, uint64_t* const*,
                 size_t*, uint64_t* const*, char**) = 0;
    int (*pool)(zkm_pool*, const zkm_stark_config*, size_t, size_t, const zkm_segment_ops*, const uint64_t* const*, const size_t*,
                uint64_t* const*, size_t*, uint64_t* const*, char**) = 0;
    int (*stage)(zkm_ctx*, const zkm_segment_ops*, zkm_staged_ops**, char**) = 0;
    int (*get)(zkm_staged_ops*, zkm_segment_ops*) = 0;
    int (*ready)(zkm_staged_ops*, int) = 0;
    void (*release)(zkm_staged_ops*) = 0;
    int (*check)(zkm_ctx*, const zkm_table_input*, size_t, const zkm_cross_table_lookup*, const zkm_ctl_side*, size_t, zkm_ctl_report*, char**) = 0;
    int (*check_segment)(zkm_ctx*, const uint64_t* const*, const unsigned*, zkm_ctl_report*, char**) = 0;
    (void)sizeof(tables = zkm_segments_tables);
    (void)sizeof(prove = zkm_prove_segments_ops);
    (void)sizeof(pool = zkm_pool_prove_segments_ops);
    (void)sizeof(stage = zkm_segment_ops_stage);
    (void)sizeof(get = zkm_staged_ops_get);
    (void)sizeof(ready = zkm_staged_ops_ready);
    (void)sizeof(release = zkm_staged_ops_free);
    (void)sizeof(check = zkm_check_ctls);
    (void)sizeof(check_segment = zkm_segment_check_ctls);
}

/* `abi_layout check_ctls`: the structs of zkm_check_ctls (tests/test_check_ctls_abi.py compares them with their mirrors).  They are
 * printed on request only: the plain output is the fixed set of structs that tests/test_segments_ops_abi.py holds to their sizes. */
static void print_check_ctls(void) {
    int first_struct = 1, first_field = 1;
    printf("{");
    BEGIN(zkm_ctl_location);
    FIELD(zkm_ctl_location, side); FIELD(zkm_ctl_location, table); FIELD(zkm_ctl_location, row);
    END();
    BEGIN(zkm_ctl_report);
    FIELD(zkm_ctl_report, kind); FIELD(zkm_ctl_report, ctl); FIELD(zkm_ctl_report, attempts); FIELD(zkm_ctl_report, host_waits);
    FIELD(zkm_ctl_report, side); FIELD(zkm_ctl_report, table); FIELD(zkm_ctl_report, row); FIELD(zkm_ctl_report, filter_value);
    FIELD(zkm_ctl_report, width); FIELD(zkm_ctl_report, nwords); FIELD(zkm_ctl_report, tuple); FIELD(zkm_ctl_report, looking_count);
    FIELD(zkm_ctl_report, looked_count); FIELD(zkm_ctl_report, nlooking_locations); FIELD(zkm_ctl_report, nlooked_locations);
    FIELD(zkm_ctl_report, looking); FIELD(zkm_ctl_report, looked);
    END();
    printf("\n}\n");
}

/* `abi_layout verify`: the struct of zkm_verify_* (tests/test_verify_abi.py compares it with its mirrors); on request only, as above. */
static void print_verify(void) {
    int first_struct = 1, first_field = 1;
    int (*segments)(zkm_ctx*, const zkm_stark_config*, size_t, const uint64_t* const*, const size_t*, const uint64_t* const*, const size_t*,
                    const uint64_t* const*, zkm_verify_report*, char**) = 0;
    (void)sizeof(segments = zkm_verify_segments);
    printf("{");
    BEGIN(zkm_verify_report);
    FIELD(zkm_verify_report, code); FIELD(zkm_verify_report, table); FIELD(zkm_verify_report, challenge); FIELD(zkm_verify_report, query);
    FIELD(zkm_verify_report, tree); FIELD(zkm_verify_report, layer); FIELD(zkm_verify_report, ctl); FIELD(zkm_verify_report, host_waits);
    END();
    printf("\n}\n");
}

/* `abi_layout boot`: the struct of the zkm_*_boot calls (tests/test_boot_abi.py compares it with its mirrors); on request only, as above. */
static void print_boot(void) {
    int first_struct = 1, first_field = 1;
    int (*tables)(zkm_ctx*, const zkm_stark_config*, size_t, const zkm_boot_image*, const zkm_segment_ops*, unsigned*, zkm_staged**, char**) = 0;
    int (*prove)(zkm_ctx*, const zkm_stark_config*, size_t, const zkm_boot_image*, const zkm_segment_ops*, const uint64_t* const*, const size_t*,
                 uint64_t* const*, size_t*, uint64_t* const*, char**) = 0;
    int (*witness)(zkm_ctx*, const zkm_boot_image*, uint64_t*, uint64_t*, uint64_t*, uint64_t*, uint64_t*, char**) = 0;
    (void)sizeof(tables = zkm_segments_tables_boot);
    (void)sizeof(prove = zkm_prove_segments_ops_boot);
    (void)sizeof(witness = zkm_boot_witness);
    printf("{");
    BEGIN(zkm_boot_image);
    FIELD(zkm_boot_image, addrs); FIELD(zkm_boot_image, values); FIELD(zkm_boot_image, nwords); FIELD(zkm_boot_image, npages);
    FIELD(zkm_boot_image, entry); FIELD(zkm_boot_image, check); FIELD(zkm_boot_image, pre_hash_root); FIELD(zkm_boot_image, pre_image_id);
    END();
    printf("\n}\n");
}

/* `abi_layout image`: the struct of zkm_image[s]_hash (tests/test_image_hash_abi.py compares it with its mirrors); on request only, as
 * above. */
static void print_image_hash(void) {
    int first_struct = 1, first_field = 1;
    size_t (*plan)(const uint32_t*, size_t, uint32_t*, size_t) = 0;
    int (*one)(zkm_ctx*, const zkm_image_pages*, uint32_t*, uint8_t*, uint8_t*, char**) = 0;
    int (*many)(zkm_ctx*, size_t, const zkm_image_pages*, uint32_t* const*, uint8_t*, uint8_t*, char**) = 0;
    (void)sizeof(plan = zkm_image_hash_plan);
    (void)sizeof(one = zkm_image_hash);
    (void)sizeof(many = zkm_images_hash);
    printf("{");
    BEGIN(zkm_image_pages);
    FIELD(zkm_image_pages, dirty_index); FIELD(zkm_image_pages, ndirty); FIELD(zkm_image_pages, dirty_words);
    FIELD(zkm_image_pages, known_index); FIELD(zkm_image_pages, nknown); FIELD(zkm_image_pages, known_words); FIELD(zkm_image_pages, pc);
    FIELD(zkm_image_pages, registers);
    END();
    printf("\n}\n");
}

/* `abi_layout steps`: the structs of the step log (tests/test_cpu_steps_abi.py compares them with their mirrors); on request only, as
 * above. */
static void print_steps(void) {
    int first_struct = 1, first_field = 1;
    int (*counts)(const zkm_cpu_steps*, size_t*, size_t*, size_t*, char**) = 0;
    int (*witness)(zkm_ctx*, const zkm_cpu_steps*, uint64_t, unsigned, uint64_t*, uint64_t*, uint32_t*, uint32_t*, char**) = 0;
    int (*tables)(zkm_ctx*, const zkm_stark_config*, size_t, const zkm_boot_image*, const zkm_cpu_steps*, const zkm_segment_ops*, unsigned*,
                  zkm_staged**, char**) = 0;
    int (*prove)(zkm_ctx*, const zkm_stark_config*, size_t, const zkm_boot_image*, const zkm_cpu_steps*, const zkm_segment_ops*,
                 const uint64_t* const*, const size_t*, uint64_t* const*, size_t*, uint64_t* const*, char**) = 0;
    (void)sizeof(counts = zkm_cpu_steps_counts);
    (void)sizeof(witness = zkm_cpu_witness);
    (void)sizeof(tables = zkm_segments_tables_steps);
    (void)sizeof(prove = zkm_prove_segments_ops_steps);
    printf("{");
    BEGIN(zkm_cpu_step);
    FIELD(zkm_cpu_step, pc); FIELD(zkm_cpu_step, next_pc); FIELD(zkm_cpu_step, insn); FIELD(zkm_cpu_step, kind); FIELD(zkm_cpu_step, flags);
    FIELD(zkm_cpu_step, context); FIELD(zkm_cpu_step, reads);
    END();
    BEGIN(zkm_cpu_steps);
    FIELD(zkm_cpu_steps, steps); FIELD(zkm_cpu_steps, nsteps); FIELD(zkm_cpu_steps, raw_rows); FIELD(zkm_cpu_steps, nraw);
    END();
    printf("\n}\n");
}

int main(int argc, char** argv) {
    int first_struct = 1, first_field = 1;
    check_segments_ops_prototypes();
    if (argc > 1 && argv[1][0] == 's') {
        print_steps();
        return 0;
    }
    if (argc > 1 && argv[1][0] == 'i') {
        print_image_hash();
        return 0;
    }
    if (argc > 1 && argv[1][0] == 'b') {
        print_boot();
        return 0;
    }
    if (argc > 1 && argv[1][0] == 'c') {
        print_check_ctls();
        return 0;
    }
    if (argc > 1 && argv[1][0] == 'v') {
        print_verify();
        return 0;
    }
    printf("{");
    BEGIN(zkm_challenger);
    FIELD(zkm_challenger, state); FIELD(zkm_challenger, in_buf); FIELD(zkm_challenger, out_buf); FIELD(zkm_challenger, n_in);
    FIELD(zkm_challenger, n_out);
    END();
    BEGIN(zkm_stark_config);
    FIELD(zkm_stark_config, rate_bits); FIELD(zkm_stark_config, cap_height); FIELD(zkm_stark_config, pow_bits);
    FIELD(zkm_stark_config, num_challenges); FIELD(zkm_stark_config, num_queries); FIELD(zkm_stark_config, arity_bits);
    FIELD(zkm_stark_config, final_poly_bits);
    END();
    BEGIN(zkm_proof_layout);
    FIELD(zkm_proof_layout, degree_bits); FIELD(zkm_proof_layout, trace_cols); FIELD(zkm_proof_layout, aux_cols);
    FIELD(zkm_proof_layout, quotient_polys); FIELD(zkm_proof_layout, ctl_zs); FIELD(zkm_proof_layout, cap_height);
    FIELD(zkm_proof_layout, fri_layers); FIELD(zkm_proof_layout, final_poly_len); FIELD(zkm_proof_layout, num_queries);
    FIELD(zkm_proof_layout, rate_bits); FIELD(zkm_proof_layout, arity_bits); FIELD(zkm_proof_layout, total_words);
    FIELD(zkm_proof_layout, init_challenger_state); FIELD(zkm_proof_layout, trace_cap); FIELD(zkm_proof_layout, aux_cap);
    FIELD(zkm_proof_layout, quotient_cap); FIELD(zkm_proof_layout, local_values); FIELD(zkm_proof_layout, next_values);
    FIELD(zkm_proof_layout, aux_polys); FIELD(zkm_proof_layout, aux_polys_next); FIELD(zkm_proof_layout, ctl_zs_first);
    FIELD(zkm_proof_layout, quotient_polys_open); FIELD(zkm_proof_layout, commit_phase_merkle_caps); FIELD(zkm_proof_layout, final_poly);
    FIELD(zkm_proof_layout, pow_witness); FIELD(zkm_proof_layout, query_round_proofs); FIELD(zkm_proof_layout, query_round_words);
    END();
    BEGIN(zkm_proof_query_layout);
    FIELD(zkm_proof_query_layout, oracle_evals); FIELD(zkm_proof_query_layout, oracle_cols); FIELD(zkm_proof_query_layout, oracle_siblings);
    FIELD(zkm_proof_query_layout, initial_siblings); FIELD(zkm_proof_query_layout, layer_evals); FIELD(zkm_proof_query_layout, layer_siblings);
    FIELD(zkm_proof_query_layout, layer_siblings_count);
    END();
    BEGIN(zkm_column);
    FIELD(zkm_column, n_local); FIELD(zkm_column, n_next); FIELD(zkm_column, term_off); FIELD(zkm_column, _pad); FIELD(zkm_column, constant);
    END();
    BEGIN(zkm_colset);
    FIELD(zkm_colset, ncols); FIELD(zkm_colset, col_off); FIELD(zkm_colset, has_filter); FIELD(zkm_colset, nprod); FIELD(zkm_colset, prod_off);
    FIELD(zkm_colset, nconst); FIELD(zkm_colset, const_off); FIELD(zkm_colset, _pad);
    END();
    BEGIN(zkm_ctl_table);
    FIELD(zkm_ctl_table, columns); FIELD(zkm_ctl_table, ncolumns); FIELD(zkm_ctl_table, term_col); FIELD(zkm_ctl_table, term_coeff);
    FIELD(zkm_ctl_table, nterms); FIELD(zkm_ctl_table, colsets); FIELD(zkm_ctl_table, ncolsets); FIELD(zkm_ctl_table, filter_idx);
    FIELD(zkm_ctl_table, nfilter_idx);
    END();
    BEGIN(zkm_ctl_z);
    FIELD(zkm_ctl_z, ncolsets); FIELD(zkm_ctl_z, colset_off); FIELD(zkm_ctl_z, num_helpers); FIELD(zkm_ctl_z, _pad); FIELD(zkm_ctl_z, beta);
    FIELD(zkm_ctl_z, gamma);
    END();
    BEGIN(zkm_ctl_side);
    FIELD(zkm_ctl_side, table); FIELD(zkm_ctl_side, colset);
    END();
    BEGIN(zkm_cross_table_lookup);
    FIELD(zkm_cross_table_lookup, nlooking); FIELD(zkm_cross_table_lookup, looking_off); FIELD(zkm_cross_table_lookup, looked);
    END();
    BEGIN(zkm_table_input);
    FIELD(zkm_table_input, table_id); FIELD(zkm_table_input, trace); FIELD(zkm_table_input, ncols); FIELD(zkm_table_input, log_n);
    FIELD(zkm_table_input, ctl); FIELD(zkm_table_input, columns);
    END();
    BEGIN(zkm_fri_poly);
    FIELD(zkm_fri_poly, oracle); FIELD(zkm_fri_poly, poly);
    END();
    BEGIN(zkm_fri_batch);
    FIELD(zkm_fri_batch, point); FIELD(zkm_fri_batch, polys); FIELD(zkm_fri_batch, npolys);
    END();
    BEGIN(zkm_segment_ops);
    FIELD(zkm_segment_ops, cpu_rows); FIELD(zkm_segment_ops, ncpu_rows); FIELD(zkm_segment_ops, arithmetic_ops);
    FIELD(zkm_segment_ops, narithmetic); FIELD(zkm_segment_ops, logic_ops); FIELD(zkm_segment_ops, nlogic);
    FIELD(zkm_segment_ops, memory_ops); FIELD(zkm_segment_ops, nmemory); FIELD(zkm_segment_ops, poseidon_inputs);
    FIELD(zkm_segment_ops, poseidon_timestamps); FIELD(zkm_segment_ops, nposeidon); FIELD(zkm_segment_ops, poseidon_sponge_inputs);
    FIELD(zkm_segment_ops, poseidon_sponge_off); FIELD(zkm_segment_ops, poseidon_sponge_meta); FIELD(zkm_segment_ops, nposeidon_sponge);
    FIELD(zkm_segment_ops, keccak_inputs); FIELD(zkm_segment_ops, keccak_timestamps); FIELD(zkm_segment_ops, nkeccak);
    FIELD(zkm_segment_ops, keccak_sponge_inputs); FIELD(zkm_segment_ops, keccak_sponge_off); FIELD(zkm_segment_ops, keccak_sponge_meta);
    FIELD(zkm_segment_ops, nkeccak_sponge); FIELD(zkm_segment_ops, sha_extend_inputs); FIELD(zkm_segment_ops, sha_extend_timestamps);
    FIELD(zkm_segment_ops, nsha_extend); FIELD(zkm_segment_ops, sha_extend_sponge_w16); FIELD(zkm_segment_ops, sha_extend_sponge_meta);
    FIELD(zkm_segment_ops, nsha_extend_sponge); FIELD(zkm_segment_ops, sha_compress_hx); FIELD(zkm_segment_ops, sha_compress_w);
    FIELD(zkm_segment_ops, sha_compress_meta); FIELD(zkm_segment_ops, nsha_compress); FIELD(zkm_segment_ops, sha_compress_sponge_hx);
    FIELD(zkm_segment_ops, sha_compress_sponge_w); FIELD(zkm_segment_ops, sha_compress_sponge_meta);
    FIELD(zkm_segment_ops, nsha_compress_sponge);
    END();
    printf("\n}\n");
    return 0;
}
