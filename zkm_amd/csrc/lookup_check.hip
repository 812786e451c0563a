// lookup_check.hip -- zkm_lookup_check / zkm_segment_lookup_check: a table's own range-check lookups (Stark::lookups(): Memory and
// Arithmetic, the rows of tables.h that zkm_table_lookups hands the prover) from the trace alone, naming the value that fails.  For a
// lookup (cols[], table_col, freq_col) and a value v, words read as field elements (a word >= p counts as its residue):
//   looking(v)   = the cells (c in cols, row r) with trace[c][r] == v                                   (an integer)
//   frequency(v) = the sum of trace[freq_col][r] over the rows r with trace[table_col][r] == v          (mod p)
// and the lookup holds iff looking(v) == frequency(v) (mod p) for every v: what the logUp argument enforces for every challenge
// (lookup.rs:106-121, 183-194: Z starts at 0 and its transition is emitted on all rows, so the sum over the domain of
// sum 1 / (x + f) - m / (x + t) vanishes as a rational function of x).  Nothing assumes the table column to be 0 .. n - 1: rows that share a
// value add their frequencies, and frequencies are field elements (p - 1 and looking + 1 on two rows balance).  Lookups with filters or
// with linear-combination columns are not covered: the reference's two lookups have neither and the registry cannot express them.
//
// One job per (table, lookup); the jobs of a call share every launch (zkm_seg_args: the job from blockIdx.z).  A job's RECORDS are the
// looking cells, column after column in the lookup's order and row after row, then the table rows: a stable sort leaves each value's
// first occurrence at the head of its run, its looking cells before its table rows.
//   (1) k_lc_emit     one lane per record, adjacent lanes on adjacent rows of one column: the 64-bit key is the canonical value itself
//                     (nothing hashed, nothing to confirm);
//   (2) radix passes  the stable LSD sort of (key, record) (radix_dev.h), always all eight passes of the one key word: the widest key
//                     is not fetched to the host, that would be a second wait;
//   (3) k_lc_flags    per sorted position three words for the scans of scan_dev.h: run-head flag | looking << 32, and the record's
//                     weight -- the canonical frequency of a table row -- as its two 32-bit HALVES.  A wrapping 64-bit scan is wrong for
//                     sums mod p of words up to p - 1; the halves are scanned as plain integers (at most 2^29 table rows x 2^32 < 2^62,
//                     the scans' saturation point) and folded per run: (hi 2^32 + lo) mod p by the 128-bit reduction of gl_dev.h;
//   (4) k_lc_mark     each run's first position (and the end of the last run); k_lc_verdict  one lane per run: unbalanced iff
//                     looking != frequency (looking < 2^30 < p); one ballot a wave, one atomicMin of the run number (runs are in value
//                     order) and one atomicAdd of the popcount per wave with an unbalanced run;
//   (5) k_lc_report   one lane per job writes the nine words of the reported run.
// One download brings down the findings of all jobs: ONE host wait a call whatever the tables, none for tables without lookups.
#include <stdio.h>

#include <algorithm>
#include <string>
#include <vector>

#include "radix_dev.h"
#include "scan_dev.h"
#include "zkm_internal.h"

namespace {

constexpr int LC_THREADS = SCAN_THREADS;
constexpr unsigned LC_MAX_LOG_N = 30;
constexpr unsigned LC_MAX_LOG_RECORDS = 30;   // per job: run number and looking count share a word, record numbers are 32 bits (ctl_check.hip's bound)
constexpr unsigned LC_KEY_BITS = 64;
constexpr uint64_t LC_NONE = ~0ull;
// the finding's words
enum { F_LOOKUP = 0, F_VALUE = 1, F_LOOKING = 2, F_FREQ = 3, F_ROWS = 4, F_COL = 5, F_ROW = 6, F_TABLE_ROW = 7, F_VALUES = 8 };
static_assert(F_VALUES + 1 == ZKM_LOOKUP_FINDING_WORDS, "nine words a finding");

// ---- the registry's looking columns, flattened for the device: the columns of (table e, lookup l) start at LC_COLS.off[e][l]
constexpr size_t lc_count_cols() {
    size_t k = 0;
    for (int e = 0; e < ZKM_NUM_TABLES; e++)
        for (size_t l = 0; l < ZKM_TABLE_ROWS[e].nlookups; l++) k += ZKM_TABLE_ROWS[e].lookups[l].ncols;
    return k;
}
constexpr size_t lc_max_lookups() {
    size_t k = 1;
    for (int e = 0; e < ZKM_NUM_TABLES; e++) k = ZKM_TABLE_ROWS[e].nlookups > k ? ZKM_TABLE_ROWS[e].nlookups : k;
    return k;
}
struct lc_cols_t {
    uint32_t v[lc_count_cols() + 1];
    uint32_t off[ZKM_NUM_TABLES][lc_max_lookups()];
};
constexpr lc_cols_t lc_flatten() {
    lc_cols_t out{};
    uint32_t k = 0;
    for (int e = 0; e < ZKM_NUM_TABLES; e++)
        for (size_t l = 0; l < ZKM_TABLE_ROWS[e].nlookups; l++) {
            out.off[e][l] = k;
            for (uint32_t i = 0; i < ZKM_TABLE_ROWS[e].lookups[l].ncols; i++) out.v[k++] = ZKM_TABLE_ROWS[e].lookups[l].cols[i];
        }
    return out;
}
constexpr lc_cols_t LC_COLS_HOST = lc_flatten();
__device__ const lc_cols_t LC_COLS = lc_flatten();

struct lc_job {
    const gl_t* trace;           // column-major, n rows a column
    uint32_t log_n, ncols;       // looking columns
    uint32_t cols_off;           // ... at LC_COLS.v[cols_off ..]
    uint32_t table_col, freq_col, lookup;
    uint32_t nrec;               // records: (ncols + 1) << log_n
    uint64_t* keys;              // nrec, sorted after the passes
    uint32_t* idx;               // nrec: the record at each sorted position
    uint64_t *a, *flo, *fhi;     // nrec + 1 each: the scans' words
    uint32_t* head;              // per run its first sorted position; head[runs] = nrec
    unsigned long long *vmin, *vcnt;   // the lowest unbalanced run (all ones: none), the unbalanced runs
    uint64_t* out;               // the job's nine words
};
static_assert(sizeof(zkm_seg_args<lc_job>) <= 3840, "the jobs travel as kernel arguments");

__device__ __forceinline__ size_t lc_looking_records(const lc_job& J) { return (size_t)J.ncols << J.log_n; }
__device__ __forceinline__ uint32_t lc_runs(const lc_job& J) { return (uint32_t)J.a[J.nrec]; }   // (after the scan)

// ---- (1) keys: record i is cell (cols[i >> log_n], i & (n - 1)), or table row i - ncols n
__global__ __launch_bounds__(LC_THREADS) void k_lc_emit(zkm_seg_args<lc_job> S) {
    const lc_job& J = S.v[blockIdx.z];
    const size_t i = (size_t)blockIdx.x * LC_THREADS + threadIdx.x;
    if (i >= J.nrec) return;
    const size_t n = (size_t)1 << J.log_n, row = i & (n - 1);
    const uint32_t k = (uint32_t)(i >> J.log_n);
    const uint32_t col = k < J.ncols ? LC_COLS.v[J.cols_off + k] : J.table_col;
    J.keys[i] = gl_canon(J.trace[(size_t)col * n + row]);
    J.idx[i] = (uint32_t)i;
}

// ---- (3) the scans' inputs; position nrec holds the zero behind them
__global__ __launch_bounds__(LC_THREADS) void k_lc_flags(zkm_seg_args<lc_job> S) {
    const lc_job& J = S.v[blockIdx.z];
    const size_t i = (size_t)blockIdx.x * LC_THREADS + threadIdx.x;
    if (i > J.nrec) return;
    uint64_t a = 0, f = 0;
    if (i < J.nrec) {
        const size_t rec = J.idx[i], nlook = lc_looking_records(J);
        const bool head = i == 0 || J.keys[i] != J.keys[i - 1];
        const bool looking = rec < nlook;
        a = (head ? 1ull : 0ull) | (looking ? 1ull << 32 : 0ull);
        if (!looking) f = gl_canon(J.trace[((size_t)J.freq_col << J.log_n) + (rec - nlook)]);
    }
    J.a[i] = a;
    J.flo[i] = (uint32_t)f;
    J.fhi[i] = f >> 32;
}

// ---- (4) a[i] = run heads before position i | looking cells before it << 32
__global__ __launch_bounds__(LC_THREADS) void k_lc_mark(zkm_seg_args<lc_job> S) {
    const lc_job& J = S.v[blockIdx.z];
    const size_t i = (size_t)blockIdx.x * LC_THREADS + threadIdx.x;
    if (i > J.nrec) return;
    if (i == J.nrec || i == 0 || J.keys[i] != J.keys[i - 1]) J.head[(uint32_t)J.a[i]] = (uint32_t)i;
}
struct lc_run {
    uint64_t looking, freq, rows;
    uint32_t h;
};
__device__ __forceinline__ lc_run lc_run_of(const lc_job& J, uint32_t r) {
    const uint32_t h0 = J.head[r], h1 = J.head[r + 1];
    lc_run R;
    R.h = h0;
    R.looking = (J.a[h1] - J.a[h0]) >> 32;   // (the low halves differ by the one head: no borrow)
    R.rows = (uint64_t)(h1 - h0) - R.looking;
    const uint64_t lo = J.flo[h1] - J.flo[h0], hi = J.fhi[h1] - J.fhi[h0];   // each below 2^61
    const uint64_t w = (hi << 32) + lo;
    R.freq = gl_canon(gl_reduce128(w, (hi >> 32) + (w < lo ? 1 : 0)));
    return R;
}
__global__ __launch_bounds__(LC_THREADS) void k_lc_verdict(zkm_seg_args<lc_job> S) {
    const lc_job& J = S.v[blockIdx.z];
    const size_t r = (size_t)blockIdx.x * LC_THREADS + threadIdx.x;
    if (r >= J.nrec || r >= lc_runs(J)) return;
    const lc_run R = lc_run_of(J, (uint32_t)r);
    const unsigned long long failing = __ballot(R.looking != R.freq);   // lanes that left above count as balanced
    if (!failing) return;
    if ((threadIdx.x & 63u) == (unsigned)(__ffsll(failing) - 1)) {      // the wave's lowest run
        atomicMin(J.vmin, (unsigned long long)r);
        atomicAdd(J.vcnt, (unsigned long long)__popcll(failing));
    }
}

// ---- (5) the nine words, one lane per job
__global__ __launch_bounds__(64) void k_lc_report(zkm_seg_args<lc_job> S) {
    const lc_job& J = S.v[blockIdx.z];
    if (threadIdx.x != 0) return;
    uint64_t* out = J.out;
    const unsigned long long r = *J.vmin;
    if (r == LC_NONE) {
        out[F_LOOKUP] = LC_NONE;
        for (int k = 1; k < ZKM_LOOKUP_FINDING_WORDS; k++) out[k] = 0;
        return;
    }
    const lc_run R = lc_run_of(J, (uint32_t)r);
    const size_t n = (size_t)1 << J.log_n;
    out[F_LOOKUP] = J.lookup;
    out[F_VALUE] = J.keys[R.h];
    out[F_LOOKING] = R.looking;
    out[F_FREQ] = R.freq;
    out[F_ROWS] = R.rows;
    out[F_COL] = out[F_ROW] = out[F_TABLE_ROW] = LC_NONE;
    if (R.looking) {   // (a run is in record order: its looking cells first)
        const size_t rec = J.idx[R.h];
        out[F_COL] = LC_COLS.v[J.cols_off + (uint32_t)(rec >> J.log_n)];
        out[F_ROW] = rec & (n - 1);
    }
    if (R.rows) out[F_TABLE_ROW] = (size_t)J.idx[R.h + R.looking] - lc_looking_records(J);
    out[F_VALUES] = *J.vcnt;
}

size_t blocks_for(size_t items, size_t per) { return (items + per - 1) / per; }

using lc_table = zkm_check_table;

// the host's refusals, before any device work (and before the missing context is looked at)
void lc_refuse(const char* what, const std::string& where, const lc_table& t, size_t ncols) {
    const zkm_table_row* row = zkm_table(t.id);
    if (!row) throw std::runtime_error(std::string(what) + ": " + where + "unknown table id " + std::to_string(t.id));
    if (!t.trace) throw std::runtime_error(std::string(what) + ": " + where + "trace: null argument");
    if (ncols != row->width)
        throw std::runtime_error(std::string(what) + ": " + where + "ncols " + std::to_string(ncols) + ": " + row->name + " has " + std::to_string(row->width) + " columns");
    if (t.log_n > LC_MAX_LOG_N) throw std::runtime_error(std::string(what) + ": " + where + "log_n " + std::to_string(t.log_n) + " above " + std::to_string(LC_MAX_LOG_N));
    for (size_t l = 0; l < row->nlookups; l++) {
        const uint64_t per_row = (uint64_t)row->lookups[l].ncols + 1;
        if ((per_row << t.log_n) > ((uint64_t)1 << LC_MAX_LOG_RECORDS))
            throw std::runtime_error(std::string(what) + ": " + row->name + ": " + std::to_string(per_row) + " x 2^" + std::to_string(t.log_n) + " records above 2^" +
                                     std::to_string(LC_MAX_LOG_RECORDS));
    }
}

// every launch of a call serves all its jobs (more than ZKM_MAX_SEG go in consecutive groups); extent: a job's workgroups
template <class E> void launch_jobs(zkm_ctx* c, void (*kernel)(zkm_seg_args<lc_job>), const std::vector<lc_job>& jobs, unsigned threads, E extent) {
    for (size_t g0 = 0; g0 < jobs.size(); g0 += ZKM_MAX_SEG) {
        const size_t k = std::min<size_t>(ZKM_MAX_SEG, jobs.size() - g0);
        size_t grid = 0;
        for (size_t j = 0; j < k; j++) grid = std::max(grid, (size_t)extent(jobs[g0 + j]));
        zkm_launch_segs(c->stream, kernel, jobs.data() + g0, k, grid, threads);
    }
}

std::string lc_hex(uint64_t v) {
    char s[24];
    snprintf(s, sizeof s, "0x%llx", (unsigned long long)v);
    return s;
}

}  // namespace

size_t zkm_lookup_check_jobs(const zkm_check_table* tabs, size_t ntab) {
    size_t njobs = 0;
    for (size_t t = 0; t < ntab; t++) njobs += zkm_table(tabs[t].id)->nlookups;
    return njobs;
}

// zkm_internal.h: the launches of ntab tables (device memory, whichever segments they belong to) on the context's stream; job j's nine
// words land at d_out + 9 j
void zkm_lookup_check_queue(zkm_ctx* c, const zkm_check_table* tabs, size_t ntab, uint64_t* d_out, zkm_lookup_queued* queued) {
    const size_t njobs = zkm_lookup_check_jobs(tabs, ntab);
    queued->job_table.clear();
    if (!njobs) return;
    std::vector<zkm_scratch>& store = queued->store;   // every block of the call: the jobs' buffers
    auto take = [&](size_t bytes) {
        store.emplace_back(c, std::max<size_t>(bytes, 64));
        return store.back().p;
    };
    // [vmin of every job | vcnt of every job]
    unsigned long long* d_ver = (unsigned long long*)take(njobs * 16);
    ZKM_HIP_CHECK(hipMemsetAsync(d_ver, 0xff, njobs * 8, c->stream));
    ZKM_HIP_CHECK(hipMemsetAsync(d_ver + njobs, 0, njobs * 8, c->stream));
    std::vector<lc_job> jobs;
    std::vector<radix_seg> rx;
    std::vector<scan_seg> scans;
    for (size_t t = 0; t < ntab; t++) {
        const zkm_table_row* row = zkm_table(tabs[t].id);
        for (size_t l = 0; l < row->nlookups; l++) {
            const zkm_table_lookup& L = row->lookups[l];
            const size_t j = jobs.size(), nrec = ((size_t)L.ncols + 1) << tabs[t].log_n;
            const uint32_t rtiles = (uint32_t)blocks_for(nrec, MT_TILE);
            lc_job J{};
            J.trace = tabs[t].trace;
            J.log_n = tabs[t].log_n;
            J.ncols = L.ncols;
            J.cols_off = LC_COLS_HOST.off[zkm_table_index(tabs[t].id)][l];
            J.table_col = L.table_col;
            J.freq_col = L.freq_col;
            J.lookup = (uint32_t)l;
            J.nrec = (uint32_t)nrec;
            J.keys = (uint64_t*)take(nrec * 8);
            J.idx = (uint32_t*)take(nrec * 4);
            J.a = (uint64_t*)take((nrec + 1) * 8);
            J.flo = (uint64_t*)take((nrec + 1) * 8);
            J.fhi = (uint64_t*)take((nrec + 1) * 8);
            J.head = (uint32_t*)take((nrec + 1) * 4);
            J.vmin = d_ver + j;
            J.vcnt = d_ver + njobs + j;
            J.out = d_out + j * ZKM_LOOKUP_FINDING_WORDS;
            uint32_t* hist = (uint32_t*)take(((size_t)MT_RADIX * rtiles + MT_RADIX) * 4);
            rx.push_back(radix_seg{J.keys, (uint64_t*)take(nrec * 8), J.idx, (uint32_t*)take(nrec * 4), hist, hist + (size_t)MT_RADIX * rtiles, (uint32_t)nrec, rtiles, 1});
            for (uint64_t* v : {J.a, J.flo, J.fhi}) scans.push_back(scan_seg{v, nrec + 1, (uint64_t*)take(blocks_for(nrec + 1, SCAN_TILE) * 8), nullptr});
            jobs.push_back(J);
            queued->job_table.push_back(t);
        }
    }
    auto records = [](const lc_job& J) { return blocks_for(J.nrec, LC_THREADS); };
    auto records1 = [](const lc_job& J) { return blocks_for((size_t)J.nrec + 1, LC_THREADS); };   // ... and the zero behind them
    {
        zkm_prof_scope ps(c, "lookup_check/emit");
        launch_jobs(c, k_lc_emit, jobs, LC_THREADS, records);
    }
    {
        zkm_prof_scope ps(c, "lookup_check/sort");
        for (unsigned bit = 0; bit < LC_KEY_BITS; bit += 8) {
            for (size_t g0 = 0; g0 < njobs; g0 += ZKM_MAX_SEG) {
                const size_t k = std::min<size_t>(ZKM_MAX_SEG, njobs - g0);
                size_t rtiles = 0;   // (of the group's tallest job)
                for (size_t j = 0; j < k; j++) rtiles = std::max<size_t>(rtiles, rx[g0 + j].ntiles);
                zkm_launch_segs(c->stream, k_radix_upsweep, rx.data() + g0, k, rtiles, MT_THREADS, bit);
                zkm_launch_segs(c->stream, k_radix_scan, rx.data() + g0, k, MT_RADIX, MT_THREADS);
                zkm_launch_segs(c->stream, k_radix_downsweep, rx.data() + g0, k, rtiles, MT_THREADS, bit);
            }
            for (radix_seg& r : rx) {
                std::swap(r.kin, r.kout);
                std::swap(r.iin, r.iout);
            }
        }
        static_assert(LC_KEY_BITS / 8 % 2 == 0, "an even number of passes: the sorted records are back in the jobs' own buffers");
    }
    {
        zkm_prof_scope ps(c, "lookup_check/verdict");
        launch_jobs(c, k_lc_flags, jobs, LC_THREADS, records1);
        for (size_t g0 = 0; g0 < scans.size(); g0 += ZKM_MAX_SEG) scan_launch(c->stream, scans.data() + g0, std::min<size_t>(ZKM_MAX_SEG, scans.size() - g0));
        launch_jobs(c, k_lc_mark, jobs, LC_THREADS, records1);
        launch_jobs(c, k_lc_verdict, jobs, LC_THREADS, records);   // (runs <= records: the lanes beyond a job's runs leave at once)
        launch_jobs(c, k_lc_report, jobs, 64, [](const lc_job&) { return 1; });
    }
}

// ... and what the downloaded job words say.  findings: written here, once the device's answer is on the host (a call that fails on the
// way leaves the caller's words alone)
size_t zkm_lookup_check_read(const zkm_check_table* tabs, size_t ntab, const zkm_lookup_queued& queued, const uint64_t* job_words, uint64_t* findings,
                             std::string* msg) {
    for (size_t t = 0; t < ntab; t++) {
        uint64_t* f = findings + t * ZKM_LOOKUP_FINDING_WORDS;
        f[F_LOOKUP] = LC_NONE;
        std::fill(f + 1, f + ZKM_LOOKUP_FINDING_WORDS, 0);
    }
    // a table's finding is that of its lowest failing lookup; the message that of the lowest failing table
    size_t first = ntab;
    for (size_t j = queued.job_table.size(); j-- > 0;) {
        const uint64_t* f = job_words + j * ZKM_LOOKUP_FINDING_WORDS;
        if (f[F_LOOKUP] == LC_NONE) continue;
        std::copy(f, f + ZKM_LOOKUP_FINDING_WORDS, findings + queued.job_table[j] * ZKM_LOOKUP_FINDING_WORDS);
        first = queued.job_table[j];
    }
    if (first == ntab) return first;
    const uint64_t* f = findings + first * ZKM_LOOKUP_FINDING_WORDS;
    const std::string cell = f[F_COL] == LC_NONE ? "none" : "column " + std::to_string(f[F_COL]) + ", row " + std::to_string(f[F_ROW]);
    const std::string trow = f[F_TABLE_ROW] == LC_NONE ? "none" : "row " + std::to_string(f[F_TABLE_ROW]);
    *msg = std::string("Lookup failed in ") + zkm_table(tabs[first].id)->name + "Stark: lookup " + std::to_string(f[F_LOOKUP]) + ": value " + lc_hex(f[F_VALUE]) +
           " is looked up " + std::to_string(f[F_LOOKING]) + " times (first: " + cell + ") and has frequency " + lc_hex(f[F_FREQ]) + " in " +
           std::to_string(f[F_ROWS]) + " table rows (first: " + trow + "); " + std::to_string(f[F_VALUES]) + " values fail";
    return first;
}

namespace {

// ntab tables in ONE set of launches on the context's stream, one download, one host wait (none when no table has a lookup):
// findings = ntab x 9 words (host); *msg names the first table with a failing lookup and stays empty when there is none.
void lc_run_tables(zkm_ctx* c, const lc_table* tabs, size_t ntab, uint64_t* findings, std::string* msg) {
    const size_t njobs = zkm_lookup_check_jobs(tabs, ntab);
    std::vector<zkm_scratch> copies;   // host tables are copied up for the call
    std::vector<lc_table> d_tabs(tabs, tabs + ntab);
    for (size_t t = 0; t < ntab; t++)
        if (zkm_table(tabs[t].id)->nlookups) d_tabs[t].trace = zkm_check_table_on_device(c, tabs[t], copies);
    zkm_lookup_queued queued;
    std::vector<uint64_t> h_out(njobs * ZKM_LOOKUP_FINDING_WORDS);
    if (njobs) {
        zkm_scratch d_out(c, std::max<size_t>(h_out.size() * 8, 64));
        zkm_lookup_check_queue(c, d_tabs.data(), ntab, d_out.as<uint64_t>(), &queued);
        c->download(h_out.data(), d_out.p, h_out.size() * 8);
    }
    zkm_lookup_check_read(tabs, ntab, queued, h_out.data(), findings, msg);
}

// refusals first, then the context, then the run; a finding is a failure of the call with its message
template <class R> int lc_entry(const char* what, zkm_ctx* c, const lc_table* tabs, size_t ntab, uint64_t* findings, char** err, R&& refusals) {
    std::string msg;
    const int rc = zkm_api(what, err, [&] {
        refusals();
        if (!c) throw std::runtime_error(std::string(what) + ": null argument");
        ZKM_HIP_CHECK(hipSetDevice(c->device));
        lc_run_tables(c, tabs, ntab, findings, &msg);
    });
    if (rc) return rc;
    return msg.empty() ? 0 : zkm_fail(err, msg.c_str());
}

}  // namespace

extern "C" {

int zkm_lookup_check(zkm_ctx* c, int table_id, const uint64_t* trace, size_t ncols, unsigned log_n, uint64_t* finding, char** err) {
    const lc_table tab{table_id, trace, log_n};
    return lc_entry("zkm_lookup_check", c, &tab, 1, finding, err, [&] {
        if (!finding) throw std::runtime_error("zkm_lookup_check: finding: null argument");
        lc_refuse("zkm_lookup_check", "", tab, ncols);
    });
}

int zkm_segment_lookup_check(zkm_ctx* c, const uint64_t* const* traces, const unsigned* log_n, uint64_t* findings, char** err) {
    lc_table tabs[ZKM_NUM_TABLES];
    return lc_entry("zkm_segment_lookup_check", c, tabs, ZKM_NUM_TABLES, findings, err, [&] {
        if (!traces) throw std::runtime_error("zkm_segment_lookup_check: traces: null argument");
        if (!log_n) throw std::runtime_error("zkm_segment_lookup_check: log_n: null argument");
        if (!findings) throw std::runtime_error("zkm_segment_lookup_check: findings: null argument");
        for (int t = 0; t < ZKM_NUM_TABLES; t++) {   // Table::all() order
            tabs[t] = lc_table{zkm_table_at(t)->id, traces[t], log_n[t]};
            lc_refuse("zkm_segment_lookup_check", std::string(zkm_table_at(t)->name) + ": ", tabs[t], zkm_table_at(t)->width);
        }
    });
}

}  // extern "C"
