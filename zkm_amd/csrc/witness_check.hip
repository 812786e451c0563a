// witness_check.hip -- zkm_witness_check / zkm_segment_witness_check: each table's own constraints on every row of the trace domain, from
// the trace alone, naming the first failure (lowest row, within it the lowest constraint index) -- zko_debug_constraints
// (oracle/prover.c) on the device.  The evaluators are the ones of the quotient kernels (constraints_dev.h), untouched: they reach their
// consumer only through constraint / constraints<B> / transition / first_row / last_row and the field z_last, so a consumer that NAMES
// instead of accumulating stands in as the explicit specialisation consumer_t<0> ("no challenges").  The table's own range-check
// lookups (Memory, Arithmetic) and the cross-table lookups are not table constraints: zkm_check_constraints and zkm_check_ctls cover them.
//
// One thread per row, lv = trace + r (check mode of k_quotient: every column load of a wave is 512 contiguous bytes).  A wave's failing
// lanes are found with one ballot; its lowest failing lane holds the wave's lowest row, so ONE atomicMin of row << 16 | index and one
// atomicAdd of the popcount per failing wave give the finding's key and the number of failing rows.  The value of the winning constraint
// cannot travel with the key: a second launch of the same kernel, one lane, evaluates the named row again and writes the finding.
#include <stdio.h>

#include "constraints_dev.h"

// ------------------------------------------------------------------ the naming consumer
// z_last / l_first / l_last are the oracle's 0 / 1 indicators.  Constraint values arrive loose: a constraint holds when its CANONICAL word
// is zero.
template <>
struct consumer_t<0> {
    static constexpr uint32_t NONE = ~0u;
    gl_t z_last, l_first, l_last;
    uint32_t count, bad_index;
    gl_t bad_value;
    __device__ __forceinline__ void start(size_t r, size_t n) {
        z_last = r != n - 1 ? 1 : 0;
        l_first = r == 0 ? 1 : 0;
        l_last = r == n - 1 ? 1 : 0;
        count = 0;
        bad_index = NONE;
        bad_value = 0;
    }
    __device__ __forceinline__ void constraint(uint64_t c) {
        const gl_t v = gl_canon(c);
        const bool first = v != 0 && bad_index == NONE;
        bad_index = first ? count : bad_index;
        bad_value = first ? v : bad_value;
        count++;
    }
    template <int B>
    __device__ __forceinline__ void constraints(const uint64_t (&c)[B]) {
#pragma unroll
        for (int i = 0; i < B; i++) constraint(c[i]);
    }
    __device__ __forceinline__ void transition(uint64_t c) { constraint(gl_mul_loose(c, z_last)); }
    __device__ __forceinline__ void last_row(uint64_t c) { constraint(gl_mul_loose(c, l_last)); }
    __device__ __forceinline__ void first_row(uint64_t c) { constraint(gl_mul_loose(c, l_first)); }
};

namespace {

constexpr unsigned WC_THREADS = 256, WC_INDEX_BITS = 16, WC_MAX_LOG_N = 30;
constexpr unsigned long long WC_NONE = ~0ull;
static_assert(WC_MAX_LOG_N + WC_INDEX_BITS < 64, "row << 16 | index is one 64-bit key");
enum { F_ROW = 0, F_INDEX = 1, F_VALUE = 2, F_ROWS = 3, F_COUNT = 4 };   // the finding's words; F_ROW holds the key between the launches
static_assert(F_COUNT + 1 == ZKM_WITNESS_FINDING_WORDS, "five words a finding");

// One descriptor per (segment, table of this kind): it travels in kernel-argument slot blockIdx.z (zkm_seg_args), the grid's x extent is
// the tallest table's and the workgroups beyond a segment's own height leave at once.  f: the segment's OWN five words -- only its lanes
// write them.
struct wc_seg {
    const gl_t* trace;
    unsigned long long* f;
    unsigned log_n;
};
static_assert(sizeof(zkm_seg_args<wc_seg>) + 8 <= 3840, "the descriptors travel as kernel arguments");

// named = 0: the grid covers the n rows; f[F_ROW] <- min key, f[F_ROWS] += failing rows, f[F_COUNT] <- constraints per row (by row 0).
// named = 1: one lane, on the row of the key the first launch left: f[F_ROW], f[F_INDEX], f[F_VALUE] <- the finding.  Nothing to do
// when no row failed (the key is still all ones: the row word of "every constraint holds").
template <int TABLE>
__global__ __launch_bounds__(WC_THREADS) void k_witness_check(zkm_seg_args<wc_seg> S, int named) {
    const wc_seg& J = S.v[blockIdx.z];
    const gl_t* __restrict__ trace = J.trace;
    unsigned long long* __restrict__ f = J.f;
    const size_t n = (size_t)1 << J.log_n;
    size_t r = (size_t)blockIdx.x * WC_THREADS + threadIdx.x;
    if (named) {
        const unsigned long long key = f[F_ROW];
        if (threadIdx.x != 0 || key == WC_NONE) return;
        r = (size_t)(key >> WC_INDEX_BITS);
    }
    if (r >= n) return;   // (a table shorter than the tallest of the launch, or than a workgroup; a key is always a row of the table)
    consumer_t<0> k;
    k.start(r, n);
    eval_table_constraints<TABLE, 0>(trace + r, n, (ptrdiff_t)((r + 1) & (n - 1)) - (ptrdiff_t)r, k);
    if (named) {
        f[F_ROW] = r;
        f[F_INDEX] = k.bad_index;
        f[F_VALUE] = k.bad_value;
        return;
    }
    if (r == 0) f[F_COUNT] = k.count;
    const unsigned long long failing = __ballot(k.bad_index != consumer_t<0>::NONE);   // lanes that left above count as holding
    if (!failing) return;
    if ((threadIdx.x & 63u) == (unsigned)(__ffsll(failing) - 1)) {
        atomicMin(&f[F_ROW], ((unsigned long long)r << WC_INDEX_BITS) | k.bad_index);
        atomicAdd(&f[F_ROWS], (unsigned long long)__popcll(failing));
    }
}

using wc_table = zkm_check_table;

// the host's refusals, before any device work (and before the missing context is looked at)
void wc_refuse(const char* what, const std::string& where, const wc_table& t, size_t ncols) {
    const zkm_table_row* row = zkm_table(t.id);
    if (!row) throw std::runtime_error(std::string(what) + ": " + where + "unknown table id " + std::to_string(t.id));
    if (!t.trace) throw std::runtime_error(std::string(what) + ": " + where + "trace: null argument");
    if (ncols != row->width)
        throw std::runtime_error(std::string(what) + ": " + where + "ncols " + std::to_string(ncols) + ": " + row->name + " has " + std::to_string(row->width) + " columns");
    if (t.log_n > WC_MAX_LOG_N) throw std::runtime_error(std::string(what) + ": " + where + "log_n " + std::to_string(t.log_n) + " above " + std::to_string(WC_MAX_LOG_N));
}

}  // namespace

// zkm_internal.h: the launches of ntab tables (device memory) into d_find = ntab x 5 words, queued on the context's stream: per table
// KIND one `rows` and one `name` launch for up to ZKM_MAX_SEG tables of that kind, whichever segments they belong to
void zkm_witness_check_queue(zkm_ctx* c, const zkm_check_table* tabs, size_t ntab, uint64_t* d_find) {
    const size_t words = ntab * ZKM_WITNESS_FINDING_WORDS;
    {
        std::vector<uint64_t> init(words, 0);
        for (size_t t = 0; t < ntab; t++) init[t * ZKM_WITNESS_FINDING_WORDS + F_ROW] = WC_NONE;
        for (size_t o = 0, step = zkm_ctx::XFER_UP / 8 / 8; o < words; o += step)   // (pieces the pinned ring takes without a wait)
            c->upload(d_find + o, init.data() + o, std::min(step, words - o) * 8);
    }
    std::vector<std::vector<wc_seg>> kinds(ZKM_NUM_TABLES);   // the tables of each kind, in the caller's order
    for (size_t t = 0; t < ntab; t++)
        kinds[zkm_table_index(tabs[t].id)].push_back(wc_seg{tabs[t].trace, (unsigned long long*)d_find + t * ZKM_WITNESS_FINDING_WORDS, tabs[t].log_n});
    for (int named = 0; named < 2; named++)
        for (int e = 0; e < ZKM_NUM_TABLES; e++)
            for (size_t g0 = 0; g0 < kinds[e].size(); g0 += ZKM_MAX_SEG) {
                const size_t k = std::min<size_t>(ZKM_MAX_SEG, kinds[e].size() - g0);
                unsigned tallest = 0;
                for (size_t j = 0; j < k; j++) tallest = std::max(tallest, kinds[e][g0 + j].log_n);
                const size_t grid = named ? 1 : (((size_t)1 << tallest) + WC_THREADS - 1) / WC_THREADS;
                zkm_prof_scope ps(c, named ? "witness_check/name" : "witness_check/rows");
                zkm_with_table(zkm_table_at(e)->id, [&](auto T) {
                    zkm_launch_segs(c->stream, k_witness_check<decltype(T)::value>, kinds[e].data() + g0, k, grid, named ? 64u : WC_THREADS, named);
                });
            }
}

// ... and what the downloaded words say: the first table with a failing row (ntab: none), its message in *msg
size_t zkm_witness_check_read(const char* what, const zkm_check_table* tabs, size_t ntab, const uint64_t* findings, std::string* msg) {
    size_t first = ntab;
    for (size_t t = ntab; t-- > 0;) {
        const uint64_t* f = findings + t * ZKM_WITNESS_FINDING_WORDS;
        if (f[F_COUNT] >> WC_INDEX_BITS) throw std::runtime_error(std::string(what) + ": internal: a row of " + zkm_table(tabs[t].id)->name + " emits 2^16 constraints or more");
        if (f[F_ROW] != WC_NONE) first = t;
    }
    if (first < ntab) {
        const uint64_t* f = findings + first * ZKM_WITNESS_FINDING_WORDS;
        char value[24];
        snprintf(value, sizeof value, "0x%llx", (unsigned long long)f[F_VALUE]);
        *msg = std::string("Constraint failed in ") + zkm_table(tabs[first].id)->name + "Stark: row " + std::to_string(f[F_ROW]) + ", constraint " +
               std::to_string(f[F_INDEX]) + " of " + std::to_string(f[F_COUNT]) + " = " + value + " (" + std::to_string(f[F_ROWS]) + " of " +
               std::to_string((uint64_t)1 << tabs[first].log_n) + " rows fail)";
    }
    return first;
}

namespace {

// ntab tables in ONE set of launches on the context's stream, one download, one host wait: findings = ntab x 5 words (host); *msg names
// the first table with a failing row and stays empty when there is none.
void wc_run(zkm_ctx* c, const char* what, const wc_table* tabs, size_t ntab, uint64_t* findings, std::string* msg) {
    std::vector<zkm_scratch> copies;   // host tables are copied up for the call
    std::vector<wc_table> d_tabs(tabs, tabs + ntab);
    for (size_t t = 0; t < ntab; t++) d_tabs[t].trace = zkm_check_table_on_device(c, tabs[t], copies);
    const size_t words = ntab * ZKM_WITNESS_FINDING_WORDS;
    zkm_scratch d_find(c, std::max<size_t>(words * 8, 64));
    zkm_witness_check_queue(c, d_tabs.data(), ntab, d_find.as<uint64_t>());
    c->download(findings, d_find.p, words * 8);
    zkm_witness_check_read(what, tabs, ntab, findings, msg);
}

// refusals first, then the context, then the run; a finding is a failure of the call with the reference's message
template <class R> int wc_entry(const char* what, zkm_ctx* c, const wc_table* tabs, size_t ntab, uint64_t* findings, char** err, R&& refusals) {
    std::string msg;
    const int rc = zkm_api(what, err, [&] {
        refusals();
        if (!c) throw std::runtime_error(std::string(what) + ": null argument");
        ZKM_HIP_CHECK(hipSetDevice(c->device));
        wc_run(c, what, tabs, ntab, findings, &msg);
    });
    if (rc) return rc;
    return msg.empty() ? 0 : zkm_fail(err, msg.c_str());
}

}  // namespace

extern "C" {

int zkm_witness_check(zkm_ctx* c, int table_id, const uint64_t* trace, size_t ncols, unsigned log_n, uint64_t* finding, char** err) {
    const wc_table tab{table_id, trace, log_n};
    return wc_entry("zkm_witness_check", c, &tab, 1, finding, err, [&] {
        if (!finding) throw std::runtime_error("zkm_witness_check: finding: null argument");
        wc_refuse("zkm_witness_check", "", tab, ncols);
    });
}

int zkm_segment_witness_check(zkm_ctx* c, const uint64_t* const* traces, const unsigned* log_n, uint64_t* findings, char** err) {
    wc_table tabs[ZKM_NUM_TABLES];
    return wc_entry("zkm_segment_witness_check", c, tabs, ZKM_NUM_TABLES, findings, err, [&] {
        if (!traces) throw std::runtime_error("zkm_segment_witness_check: traces: null argument");
        if (!log_n) throw std::runtime_error("zkm_segment_witness_check: log_n: null argument");
        if (!findings) throw std::runtime_error("zkm_segment_witness_check: findings: null argument");
        for (int t = 0; t < ZKM_NUM_TABLES; t++) {   // Table::all() order
            tabs[t] = wc_table{zkm_table_at(t)->id, traces[t], log_n[t]};
            wc_refuse("zkm_segment_witness_check", std::string(zkm_table_at(t)->name) + ": ", tabs[t], zkm_table_at(t)->width);
        }
    });
}

}  // extern "C"
