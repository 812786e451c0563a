// segment_check.hip -- zkm_segments_check / zkm_segment_check: everything eval_vanishing_poly and verify_cross_table_lookups ask of a
// witness, on K segments behind ONE pair of host waits.  The three checks keep their kernels and their files; each gives a part that
// queues and a part that reads (zkm_internal.h), and this file composes them on the context's stream:
//   queue   the table constraints of all K x 12 tables (witness_check.hip: one `rows` and one `name` launch per table kind and group of
//           ZKM_MAX_SEG segments), the range-check lookups of the 2 K tables that have them (lookup_check.hip: one job each, ZKM_MAX_SEG
//           jobs a launch), both into one block of result words; nothing here depends on what the host computes;
//   wait 1  the cross-table lookups' record counts (ctl_check.hip: 15 K jobs, ZKM_MAX_SEG a launch);
//   wait 2  ONE download: the cross-table verdicts with the block of result words riding along;
//   wait 3  only when a cross-table lookup fails: the reports of all failing segments.  A key collision adds a wait per extra attempt.
// A segment's verdict is its first finding in eval_vanishing_poly's order (vanishing_poly.rs:17-46): table constraints, the table's own
// lookups, then the cross-table lookups.  Every check runs to the end on every segment whatever the others found.
#include <string>
#include <vector>

#include "zkm_internal.h"

namespace {

constexpr size_t NT = ZKM_NUM_TABLES;
constexpr unsigned SC_MAX_LOG_N = 30;

// Estimated bytes of scratch the checks of one segment hold at once, beside the tables: ~64 bytes per record of a range-check lookup
// (rows x (looking columns + 1): key, index and three scan words, each sorted through a second buffer) and ~96 per candidate row of a
// cross-table lookup (the records are at most the sides' rows: location, 128-bit key and index twice over, two scan words, run heads
// and ends), plus a copy of every table that is not one block of device memory.
double check_scratch_bytes(const zkm_table_input* tabs, const zkm_cross_table_lookup* ctls, const zkm_ctl_side* sides, size_t nctls) {
    double bytes = 0;
    for (size_t t = 0; t < NT; t++) {
        const zkm_table_row* row = zkm_table_at((int)t);
        const double n = (double)((size_t)1 << tabs[t].log_n);
        for (size_t l = 0; l < row->nlookups; l++) bytes += 64.0 * n * (double)(row->lookups[l].ncols + 1);
        if (tabs[t].columns || !zkm_is_device_ptr(tabs[t].trace)) bytes += 8.0 * n * (double)row->width;
    }
    for (size_t j = 0; j < nctls; j++)
        for (uint32_t i = 0; i <= ctls[j].nlooking; i++) {
            const zkm_ctl_side sd = i < ctls[j].nlooking ? sides[ctls[j].looking_off + i] : ctls[j].looked;
            if (sd.table < NT) bytes += 96.0 * (double)((size_t)1 << tabs[sd.table].log_n);
        }
    return bytes;
}

// k segments in one set of launches.  Returns the lowest segment with a finding (k: none), its message in *msg
size_t check_group(zkm_ctx* c, size_t k, const zkm_table_input* const* tables, const zkm_cross_table_lookup* ctls, const zkm_ctl_side* sides, size_t nctls,
                   uint64_t* verdicts, uint64_t* witness_findings, uint64_t* lookup_findings, zkm_ctl_report* reps, std::string* msg) {
    const size_t ntab = k * NT;
    // ---- the tables on the device, once for the three checks: in place, or a copy of host memory / of one pointer per column
    std::vector<zkm_scratch> copies;
    std::vector<zkm_table_input> dev(ntab);
    std::vector<const zkm_table_input*> dev_seg(k);
    std::vector<zkm_check_table> ct(ntab);
    for (size_t s = 0; s < k; s++) {
        dev_seg[s] = dev.data() + s * NT;
        for (size_t t = 0; t < NT; t++) {
            const zkm_table_input& in = tables[s][t];
            const size_t n = (size_t)1 << in.log_n;
            zkm_check_table& T = ct[s * NT + t];
            T = zkm_check_table{in.table_id, in.trace, in.log_n};
            if (in.columns) {
                copies.emplace_back(c, in.ncols * n * 8);
                for (size_t i = 0; i < in.ncols; i++) {
                    if (!in.columns[i]) throw std::runtime_error("zkm_segments_check: null column");
                    ZKM_HIP_CHECK(hipMemcpyAsync(copies.back().as<gl_t>() + i * n, in.columns[i], n * 8, hipMemcpyDefault, c->stream));
                }
                T.trace = copies.back().as<uint64_t>();
            } else {
                T.trace = zkm_check_table_on_device(c, T, copies);
            }
            dev[s * NT + t] = in;
            dev[s * NT + t].trace = T.trace;
            dev[s * NT + t].columns = nullptr;
        }
    }
    // ---- the launches that depend on nothing the host computes, into one block: [witness findings | lookup job words]
    const size_t njobs = zkm_lookup_check_jobs(ct.data(), ntab);
    const size_t w_words = ntab * ZKM_WITNESS_FINDING_WORDS, words = w_words + njobs * ZKM_LOOKUP_FINDING_WORDS;
    zkm_scratch d_words(c, words * 8);
    zkm_lookup_queued queued;
    zkm_witness_check_queue(c, ct.data(), ntab, d_words.as<uint64_t>());
    zkm_lookup_check_queue(c, ct.data(), ntab, d_words.as<uint64_t>() + w_words, &queued);
    // ---- the cross-table lookups: their second wait brings the block down
    std::vector<uint64_t> h_words(words);
    const zkm_ctx::xfer ride{h_words.data(), d_words.p, words * 8};
    std::vector<zkm_ctl_report> own_reps(reps ? 0 : k);
    zkm_ctl_report* R = reps ? reps : own_reps.data();
    memset(R, 0, k * sizeof *R);
    std::vector<std::string> ctl_msgs(k);
    zkm_check_ctls_run_segments(c, k, dev_seg.data(), NT, ctls, sides, nctls, R, ctl_msgs.data(), &ride);
    // ---- what the words say, segment by segment
    std::vector<uint64_t> wf(NT * ZKM_WITNESS_FINDING_WORDS), lf(NT * ZKM_LOOKUP_FINDING_WORDS);
    size_t first = k, job0 = 0;
    for (size_t s = 0; s < k; s++) {
        const zkm_check_table* tabs = ct.data() + s * NT;
        std::string w_msg, l_msg;
        std::copy(h_words.begin() + s * NT * ZKM_WITNESS_FINDING_WORDS, h_words.begin() + (s + 1) * NT * ZKM_WITNESS_FINDING_WORDS, wf.begin());
        const size_t w_first = zkm_witness_check_read("zkm_segments_check", tabs, NT, wf.data(), &w_msg);
        zkm_lookup_queued mine;   // the segment's jobs, its tables counted from its own first
        size_t j1 = job0;
        while (j1 < queued.job_table.size() && queued.job_table[j1] < (s + 1) * NT) mine.job_table.push_back(queued.job_table[j1++] - s * NT);
        const size_t l_first = zkm_lookup_check_read(tabs, NT, mine, h_words.data() + w_words + job0 * ZKM_LOOKUP_FINDING_WORDS, lf.data(), &l_msg);
        job0 = j1;
        if (witness_findings) std::copy(wf.begin(), wf.end(), witness_findings + s * wf.size());
        if (lookup_findings) std::copy(lf.begin(), lf.end(), lookup_findings + s * lf.size());
        const uint64_t kind = w_first < NT ? 1 : l_first < NT ? 2 : R[s].kind ? 3 : 0;
        if (verdicts) {
            verdicts[2 * s] = kind;
            verdicts[2 * s + 1] = kind == 1 ? w_first : kind == 2 ? l_first : kind == 3 ? R[s].ctl : 0;
        }
        if (kind && first == k) {
            first = s;
            *msg = kind == 1 ? w_msg : kind == 2 ? l_msg : ctl_msgs[s];
        }
    }
    return first;
}

}  // namespace

// zkm_internal.h: the body of zkm_segments_check, and the gate of the prove drivers under "check_witness".  Segments whose scratch would
// not fit beside the tables together -- check_scratch_bytes against 80 % of what the context's allocator has cached plus what is free
// now, the bound of prove_segments_waves -- are checked in consecutive sub-groups, each with its own waits; one segment always goes.
size_t zkm_segments_check_run(zkm_ctx* c, size_t nseg, const zkm_table_input* const* tables, uint64_t* verdicts, uint64_t* witness_findings,
                              uint64_t* lookup_findings, zkm_ctl_report* ctl_reports, std::string* msg) {
    const zkm_cross_table_lookup* ctls;
    const zkm_ctl_side* sides;
    size_t nctls, nsides;
    zkm_all_stark_ctls(&ctls, &nctls, &sides, &nsides);
    size_t free_b = 0, total_b = 0, live = 0, cached = 0;
    ZKM_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    zkm_ctx_memory(c, &live, &cached);
    const double budget = c->segments_memory_budget ? (double)c->segments_memory_budget : 0.8 * ((double)cached + (double)free_b);
    size_t first = nseg;
    for (size_t s0 = 0; s0 < nseg;) {
        size_t k = 1;
        double held = check_scratch_bytes(tables[s0], ctls, sides, nctls);
        while (s0 + k < nseg) {
            const double next = check_scratch_bytes(tables[s0 + k], ctls, sides, nctls);
            if (held + next > budget) break;
            held += next;
            k++;
        }
        std::string m;
        const size_t f = check_group(c, k, tables + s0, ctls, sides, nctls, verdicts ? verdicts + 2 * s0 : nullptr,
                                     witness_findings ? witness_findings + s0 * NT * ZKM_WITNESS_FINDING_WORDS : nullptr,
                                     lookup_findings ? lookup_findings + s0 * NT * ZKM_LOOKUP_FINDING_WORDS : nullptr, ctl_reports ? ctl_reports + s0 : nullptr, &m);
        if (f < k && first == nseg) {
            first = s0 + f;
            *msg = m;
        }
        s0 += k;
    }
    return first;
}

// refusals first, then the context, then the run; a finding is a failure of the call with the owning check's message
static int segments_check(const char* what, zkm_ctx* c, size_t nseg, const uint64_t* const* const* traces, const unsigned* const* log_n, uint64_t* verdicts,
                          uint64_t* witness_findings, uint64_t* lookup_findings, zkm_ctl_report* ctl_reports, char** err) {
    std::string msg;
    size_t first = 0;
    const int rc = zkm_api(what, err, [&] {
        // the host's refusals, before any device work and before the context is needed
        if (!nseg) throw std::runtime_error(std::string(what) + ": nseg: no segment");
        if (!traces) throw std::runtime_error(std::string(what) + ": traces: null argument");
        if (!log_n) throw std::runtime_error(std::string(what) + ": log_n: null argument");
        std::vector<zkm_table_input> tables(nseg * NT);
        std::vector<const zkm_table_input*> seg(nseg);
        for (size_t s = 0; s < nseg; s++) {
            const std::string where = std::string(what) + ": segment " + std::to_string(s) + ": ";
            if (!traces[s]) throw std::runtime_error(where + "traces: null argument");
            if (!log_n[s]) throw std::runtime_error(where + "log_n: null argument");
            zkm_all_stark_table_inputs(tables.data() + s * NT);   // Table::all() order
            seg[s] = tables.data() + s * NT;
            for (size_t t = 0; t < NT; t++) {
                const char* name = zkm_table_at((int)t)->name;
                if (!traces[s][t]) throw std::runtime_error(where + name + ": trace: null argument");
                if (log_n[s][t] > SC_MAX_LOG_N)
                    throw std::runtime_error(where + name + ": log_n " + std::to_string(log_n[s][t]) + " above " + std::to_string(SC_MAX_LOG_N));
                const zkm_table_row* row = zkm_table_at((int)t);
                for (size_t l = 0; l < row->nlookups; l++)   // (the lookup check's bound on a job's records)
                    if ((((uint64_t)row->lookups[l].ncols + 1) << log_n[s][t]) > ((uint64_t)1 << 30))
                        throw std::runtime_error(where + name + ": " + std::to_string(row->lookups[l].ncols + 1) + " x 2^" + std::to_string(log_n[s][t]) +
                                                 " records above 2^30");
                tables[s * NT + t].trace = traces[s][t];
                tables[s * NT + t].log_n = log_n[s][t];
            }
        }
        if (!c) throw std::runtime_error(std::string(what) + ": null argument");
        ZKM_HIP_CHECK(hipSetDevice(c->device));
        first = zkm_segments_check_run(c, nseg, seg.data(), verdicts, witness_findings, lookup_findings, ctl_reports, &msg);
    });
    if (rc) return rc;
    if (first == nseg) return 0;
    return zkm_fail(err, (std::string(what) + ": segment " + std::to_string(first) + ": " + msg).c_str());
}

extern "C" {

int zkm_segments_check(zkm_ctx* c, size_t nseg, const uint64_t* const* const* traces, const unsigned* const* log_n, uint64_t* verdicts,
                       uint64_t* witness_findings, uint64_t* lookup_findings, zkm_ctl_report* ctl_reports, char** err) {
    return segments_check("zkm_segments_check", c, nseg, traces, log_n, verdicts, witness_findings, lookup_findings, ctl_reports, err);
}

int zkm_segment_check(zkm_ctx* c, const uint64_t* const* traces, const unsigned* log_n, uint64_t* verdict, uint64_t* witness_findings,
                      uint64_t* lookup_findings, zkm_ctl_report* ctl_report, char** err) {
    return segments_check("zkm_segment_check", c, 1, traces ? &traces : nullptr, log_n ? &log_n : nullptr, verdict, witness_findings, lookup_findings, ctl_report, err);
}

}  // extern "C"
