// ctl_check.hip -- testutils::check_ctls (cross_table_lookup.rs:1486-1581; prove_with_traces runs it under the `test` feature,
// prover.rs:171-176) on device-resident tables: for every CrossTableLookup, the multiset of the filtered rows of the looking tables
// against that of the looked table, with the row and its locations named when they differ.
//
// One job per (segment, lookup) -- a call takes the table lists of K segments, the single-segment entry points are K = 1; the jobs of a
// call share every launch, ZKM_MAX_SEG at a time (zkm_seg_args: the job from blockIdx.z).  A job's candidate rows are its
// sides' rows, side after side (the looking sides in the lookup's order, the looked side last), cut into tiles of CC_TILE rows:
//   (1) k_cc_count    one lane per (side, row): the filter; the smallest (side, row) with a value other than 0 or 1; per-tile counts of
//                     the rows with filter 1 (the job's RECORDS);
//   (2) scan          exclusive scan of the tile counts (scan_dev.h): each tile's first record; the total comes to the host, which sizes
//                     everything below by the records, not by sides x rows;
//   (3) k_cc_emit     the records' locations (side, row) in candidate order;
//   (4) k_cc_keys     per record a 128-bit key: two linear forms of the canonical tuple over Goldilocks, multipliers from the attempt's seed;
//   (5) radix passes  the stable LSD sort of (key, record) (radix_dev.h, the Memory witness's kernels);
//   (6) k_cc_flags    per sorted position: run-head flag, the record's sign (looking in the low half of a word, looked in the high half),
//                     and the CONFIRMATION -- a record whose key equals its predecessor's re-evaluates both tuples and compares them word
//                     for word; a difference is a key collision and the attempt is void;
//   (7) scan          of the flags (run numbers) and of the signs (occurrences on either side before each position);
//   (8) k_cc_mark     each run's head position and the sign prefix at its end;  k_cc_verdict  a run is balanced iff the prefix grew by
//                     the same amount in both halves; the unbalanced run whose head is the earliest record (atomicMin) is the one
//                     reported: the sort is stable, so a run's head is its tuple's first occurrence in candidate order;
//   (9) k_cc_report   the reported tuple, its two counts and its first locations (or the filter's value).
// Host waits, whatever K: the record counts, the verdict of each attempt (one unless keys collided), the reports of a failing call.
#include <algorithm>
#include <string>
#include <vector>

#include "ctl_dev.h"
#include "radix_dev.h"
#include "scan_dev.h"
#include "zkm_internal.h"

namespace {

constexpr int CC_THREADS = SCAN_THREADS;
constexpr int CC_ITEMS = 4;                       // rows per lane and tile
constexpr int CC_TILE = CC_THREADS * CC_ITEMS;    // 1024 candidate rows per tile
constexpr unsigned CC_KEY_BITS = 128;
constexpr int CC_MAX_ATTEMPTS = 4;
constexpr uint64_t CC_NONE = ~0ull;
constexpr size_t CC_MAX_RECORDS = (size_t)1 << 30;   // per lookup: record and run numbers share a word, the two signs another
constexpr int CC_REPORT_WORDS = 3 + ZKM_CTL_REPORT_WORDS + 2 * ZKM_CTL_REPORT_LOCATIONS;

struct cc_tab {
    ctl_dev d;
    const gl_t* trace;
    uint64_t n;
};
struct cc_side {
    uint32_t table, colset;
    uint32_t tile0, _pad;        // the side's first tile among the job's
};
// res: [0] smallest (side << 32 | row) with a non-binary filter, [1] records; ver (reset per attempt): [0] collision seen,
// [1] (record << 32 | run) of the reported run, [2] runs
struct cc_job {
    const cc_tab* tabs;
    const cc_side* sides;        // this lookup's sides: the looking ones, then the looked one
    uint32_t nsides, width, ntiles, nrec;
    uint64_t* cnt;               // ntiles + 1 words: records per tile, then their exclusive scan
    unsigned long long *res, *ver;
    uint64_t* loc;               // nrec: side << 32 | row of each record
    uint64_t* keys;              // 2 x nrec, sorted order after the passes
    uint32_t* idx;               // nrec: the record at each sorted position
    uint64_t *sgn, *flg;         // nrec + 1 each
    uint32_t* head;              // per run: its first sorted position
    uint64_t* end;               // per run: sgn behind its last position
};

__device__ __forceinline__ uint32_t cc_side_of(const cc_side* __restrict__ sides, uint32_t nsides, uint32_t tile) {
    uint32_t lo = 0, hi = nsides - 1;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (sides[mid].tile0 <= tile) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}
// eval_table (cross_table_lookup.rs:266-285): on the last row the next-row part is zero
__device__ __forceinline__ gl_t cc_filter(const cc_tab& T, const zkm_colset& cs, size_t row) {
    return gl_canon(ctl_eval_filter(T.d, cs, T.trace + row, T.n, 1, row + 1 < T.n));
}
__device__ __forceinline__ gl_t cc_word(const cc_tab& T, const zkm_colset& cs, size_t row, uint32_t k) {
    return gl_canon(ctl_eval_column(T.d, cs.col_off + k, T.trace + row, T.n, 1, row + 1 < T.n));
}
GL_HD uint64_t cc_mix(uint64_t x) {   // SplitMix64's finaliser
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// ---- (1) count
__global__ __launch_bounds__(CC_THREADS) void k_cc_count(zkm_seg_args<cc_job> S) {
    __shared__ uint32_t sh[SCAN_WAVES];
    const cc_job& J = S.v[blockIdx.z];
    if (blockIdx.x >= J.ntiles) return;
    const uint32_t s = cc_side_of(J.sides, J.nsides, blockIdx.x);
    const cc_side sd = J.sides[s];
    const cc_tab& T = J.tabs[sd.table];
    const zkm_colset cs = T.d.colsets[sd.colset];
    const size_t n = T.n, base = (size_t)(blockIdx.x - sd.tile0) * CC_TILE;
    uint32_t c = 0;
    unsigned long long bad = CC_NONE;
#pragma unroll
    for (int it = 0; it < CC_ITEMS; it++) {
        const size_t row = base + (size_t)it * CC_THREADS + threadIdx.x;
        if (row >= n) continue;
        const gl_t f = cc_filter(T, cs, row);
        if (f == 1) c++;
        else if (f != 0 && bad == CC_NONE) bad = ((unsigned long long)s << 32) | row;
    }
    uint32_t all;
    block_incl_scan(c, sh, add_u32(), &all);
    if (threadIdx.x == 0) J.cnt[blockIdx.x] = all;
    if (bad != CC_NONE) atomicMin(&J.res[0], bad);
}

// ---- (3) emit: cnt[tile] = the tile's first record
__global__ __launch_bounds__(CC_THREADS) void k_cc_emit(zkm_seg_args<cc_job> S) {
    __shared__ uint32_t sh[SCAN_WAVES];
    const cc_job& J = S.v[blockIdx.z];
    if (blockIdx.x >= J.ntiles) return;
    const uint32_t s = cc_side_of(J.sides, J.nsides, blockIdx.x);
    const cc_side sd = J.sides[s];
    const cc_tab& T = J.tabs[sd.table];
    const zkm_colset cs = T.d.colsets[sd.colset];
    const size_t n = T.n, base = (size_t)(blockIdx.x - sd.tile0) * CC_TILE;
    uint64_t run = J.cnt[blockIdx.x];
    for (int it = 0; it < CC_ITEMS; it++) {
        const size_t row = base + (size_t)it * CC_THREADS + threadIdx.x;
        const bool on = row < n && cc_filter(T, cs, row) == 1;
        uint32_t all;
        const uint32_t incl = block_incl_scan(on ? 1u : 0u, sh, add_u32(), &all);
        if (on && run + incl - 1 < J.nrec) J.loc[run + incl - 1] = ((uint64_t)s << 32) | row;
        run += all;
    }
}

// ---- (4) keys.  bits < 128 (the test hook): the key truncated to its low `bits` bits
__global__ __launch_bounds__(CC_THREADS) void k_cc_keys(zkm_seg_args<cc_job> S, uint64_t seed, unsigned bits) {
    const cc_job& J = S.v[blockIdx.z];
    const size_t i = (size_t)blockIdx.x * CC_THREADS + threadIdx.x;
    if (i >= J.nrec) return;
    const uint64_t loc = J.loc[i];
    const cc_side sd = J.sides[loc >> 32];
    const cc_tab& T = J.tabs[sd.table];
    const zkm_colset cs = T.d.colsets[sd.colset];
    const size_t row = (uint32_t)loc;
    gl_t k0 = 0, k1 = 0;
    for (uint32_t k = 0; k < J.width; k++) {
        const gl_t v = cc_word(T, cs, row, k);
        k0 = gl_add(k0, gl_mul(v, gl_canon(cc_mix(seed + 2 * k))));
        k1 = gl_add(k1, gl_mul(v, gl_canon(cc_mix(~seed + 2 * k + 1))));
    }
    k0 = gl_canon(k0);
    k1 = gl_canon(k1);
    if (bits < 64) k0 &= (1ull << bits) - 1;
    if (bits <= 64) k1 = 0;
    else if (bits < 128) k1 &= (1ull << (bits - 64)) - 1;
    J.keys[i] = k0;
    J.keys[(size_t)J.nrec + i] = k1;
    J.idx[i] = (uint32_t)i;
}

__device__ __forceinline__ bool cc_same_key(const cc_job& J, size_t a, size_t b) {
    return J.keys[a] == J.keys[b] && J.keys[(size_t)J.nrec + a] == J.keys[(size_t)J.nrec + b];
}
__device__ __forceinline__ bool cc_same_tuple(const cc_job& J, uint64_t la, uint64_t lb) {
    const cc_side sa = J.sides[la >> 32], sb = J.sides[lb >> 32];
    const cc_tab &Ta = J.tabs[sa.table], &Tb = J.tabs[sb.table];
    const zkm_colset ca = Ta.d.colsets[sa.colset], cb = Tb.d.colsets[sb.colset];
    for (uint32_t k = 0; k < J.width; k++)
        if (cc_word(Ta, ca, (uint32_t)la, k) != cc_word(Tb, cb, (uint32_t)lb, k)) return false;
    return true;
}

// ---- (6) flags, signs and the confirmation; position nrec holds the zero behind the scans' inputs
__global__ __launch_bounds__(CC_THREADS) void k_cc_flags(zkm_seg_args<cc_job> S) {
    const cc_job& J = S.v[blockIdx.z];
    const size_t i = (size_t)blockIdx.x * CC_THREADS + threadIdx.x;
    if (i > J.nrec) return;
    if (i == J.nrec) {
        J.sgn[i] = 0;
        J.flg[i] = 0;
        return;
    }
    const uint64_t loc = J.loc[J.idx[i]];
    const bool head = i == 0 || !cc_same_key(J, i, i - 1);
    J.sgn[i] = (loc >> 32) == J.nsides - 1 ? 1ull << 32 : 1ull;
    J.flg[i] = head;
    if (!head && !cc_same_tuple(J, loc, J.loc[J.idx[i - 1]])) J.ver[0] = 1;
}

// ---- (8) flg[i] = run heads before position i, sgn[i] = signs before it
__global__ __launch_bounds__(CC_THREADS) void k_cc_mark(zkm_seg_args<cc_job> S) {
    const cc_job& J = S.v[blockIdx.z];
    const size_t i = (size_t)blockIdx.x * CC_THREADS + threadIdx.x;
    if (i >= J.nrec) return;
    const bool head = i == 0 || !cc_same_key(J, i, i - 1);
    const bool last = i + 1 == J.nrec || !cc_same_key(J, i, i + 1);
    const uint64_t r = head ? J.flg[i] : J.flg[i] - 1;
    if (head) J.head[r] = (uint32_t)i;
    if (last) J.end[r] = J.sgn[i + 1];
}
__device__ __forceinline__ uint64_t cc_run_signs(const cc_job& J, size_t r) { return J.end[r] - (r ? J.end[r - 1] : 0); }
__global__ __launch_bounds__(CC_THREADS) void k_cc_verdict(zkm_seg_args<cc_job> S) {
    const cc_job& J = S.v[blockIdx.z];
    const size_t r = (size_t)blockIdx.x * CC_THREADS + threadIdx.x;
    if (r >= J.nrec || r >= J.ver[2]) return;
    const uint64_t d = cc_run_signs(J, r);
    if ((uint32_t)d != (uint32_t)(d >> 32)) atomicMin(&J.ver[1], ((unsigned long long)J.idx[J.head[r]] << 32) | r);
}

// ---- (9) report of ONE job.  what = side << 32 | row of a non-binary filter (out[0] = its value), or CC_NONE: run `run` -- out[1], out[2]
// its occurrences on the looking / looked side, out[3 ..] the tuple, then the first locations of either side
__global__ __launch_bounds__(CC_THREADS) void k_cc_report(cc_job J, unsigned long long what, uint32_t run, uint64_t* __restrict__ out) {
    const uint32_t t = threadIdx.x;
    if (what != CC_NONE) {
        if (t) return;
        const cc_side sd = J.sides[what >> 32];
        const cc_tab& T = J.tabs[sd.table];
        out[0] = cc_filter(T, T.d.colsets[sd.colset], (uint32_t)what);
        return;
    }
    const uint64_t d = cc_run_signs(J, run);
    const uint32_t looking = (uint32_t)d, looked = (uint32_t)(d >> 32), h = J.head[run];
    if (t == 0) {
        out[1] = looking;
        out[2] = looked;
    }
    const uint64_t loc = J.loc[J.idx[h]];
    const cc_side sd = J.sides[loc >> 32];
    const cc_tab& T = J.tabs[sd.table];
    if (t < J.width && t < ZKM_CTL_REPORT_WORDS) out[3 + t] = cc_word(T, T.d.colsets[sd.colset], (uint32_t)loc, t);
    // (the run is in candidate order: its looking records first)
    if (t < ZKM_CTL_REPORT_LOCATIONS) {
        if (t < looking) out[3 + ZKM_CTL_REPORT_WORDS + t] = J.loc[J.idx[h + t]];
        if (t < looked) out[3 + ZKM_CTL_REPORT_WORDS + ZKM_CTL_REPORT_LOCATIONS + t] = J.loc[J.idx[h + looking + t]];
    }
}

size_t blocks_for(size_t items, size_t per) { return (items + per - 1) / per; }

// every launch of a call serves all its jobs; more than ZKM_MAX_SEG jobs go in consecutive groups
template <class E, class... X>
void launch_jobs(zkm_ctx* c, const char* name, void (*kernel)(zkm_seg_args<cc_job>, X...), const std::vector<cc_job>& jobs, E extent, X... x) {
    for (size_t g0 = 0; g0 < jobs.size(); g0 += ZKM_MAX_SEG) {
        const size_t k = std::min<size_t>(ZKM_MAX_SEG, jobs.size() - g0);
        size_t grid = 0;
        for (size_t j = 0; j < k; j++) grid = std::max(grid, (size_t)extent(jobs[g0 + j]));
        zkm_prof_scope ps(c, name);
        zkm_launch_segs(c->stream, kernel, jobs.data() + g0, k, grid, CC_THREADS, x...);
    }
}
void scan_jobs(zkm_ctx* c, const std::vector<scan_seg>& scans) {
    for (size_t g0 = 0; g0 < scans.size(); g0 += ZKM_MAX_SEG) {
        zkm_prof_scope ps(c, "check_ctls/scan");
        scan_launch(c->stream, scans.data() + g0, std::min<size_t>(ZKM_MAX_SEG, scans.size() - g0));
    }
}

std::string table_label(const zkm_table_input* tables, uint32_t t) {
    const zkm_table_row* row = zkm_table(tables[t].table_id);
    return row ? std::string(row->name) : "Table" + std::to_string(t);
}
std::string locations_text(const zkm_table_input* tables, const zkm_ctl_location* l, uint32_t shown, uint64_t count) {
    std::string s = "[";
    for (uint32_t i = 0; i < shown; i++) s += (i ? ", (" : "(") + table_label(tables, l[i].table) + ", " + std::to_string(l[i].row) + ")";
    if (count > shown) s += ", ...";
    return s + "]";
}

}  // namespace

// zkm_internal.h: the check on the tables of nseg segments, job s nctls + j = lookup j of segment s.  Fills reps[s] / msgs[s] (kind 0, 1
// or 2 with the reference's message) and returns the lowest failing segment (nseg: none); throws when the check cannot be made (the
// entry points turn that into kind 3).
size_t zkm_check_ctls_run_segments(zkm_ctx* c, size_t nseg, const zkm_table_input* const* tables, size_t ntables, const zkm_cross_table_lookup* ctls,
                                   const zkm_ctl_side* sides, size_t nctls, zkm_ctl_report* reps, std::string* msgs, const zkm_ctx::xfer* ride) {
    if (!nseg || !tables || !reps || !msgs) throw std::runtime_error("check_ctls: null argument");
    for (size_t s = 0; s < nseg; s++)
        if ((!tables[s] && ntables) || (nctls && (!ctls || !sides))) throw std::runtime_error("check_ctls: null argument");
    if (nctls >= ((size_t)1 << 31) / nseg) throw std::runtime_error("check_ctls: too many lookups");
    uint32_t attempts = 0, host_waits = 0;
    auto stamp = [&] {   // (the waits and attempts are the call's: every segment's report carries them)
        for (size_t s = 0; s < nseg; s++) {
            reps[s].attempts = attempts;
            reps[s].host_waits = host_waits;
        }
    };
    stamp();
    const size_t njobs = nseg * nctls;
    // ---- the description: every side names a table and one of its column sets; the sides of a lookup agree in width
    std::vector<char> used(nseg * ntables, 0);
    std::vector<cc_side> h_sides;
    std::vector<size_t> side_off(njobs + 1, 0);
    std::vector<uint32_t> width(nctls), ntiles(njobs);
    for (size_t s = 0; s < nseg; s++)
        for (size_t j = 0; j < nctls; j++) {
            const zkm_cross_table_lookup& L = ctls[j];
            if (L.nlooking + 1 == 0) throw std::runtime_error("check_ctls: malformed cross-table lookups");
            uint64_t tile = 0;
            for (uint32_t i = 0; i <= L.nlooking; i++) {
                const zkm_ctl_side sd = i < L.nlooking ? sides[L.looking_off + i] : L.looked;
                if (sd.table >= ntables) throw std::runtime_error("CTL #" + std::to_string(j) + ": table index out of range");
                const zkm_table_input& t = tables[s][sd.table];
                if (!t.ctl || sd.colset >= t.ctl->ncolsets) throw std::runtime_error("CTL #" + std::to_string(j) + ": column-set index out of range");
                if (t.ncols == 0 || t.log_n > 30 || (!t.trace && !t.columns)) throw std::runtime_error("check_ctls: bad table shape");
                const uint32_t w = t.ctl->colsets[sd.colset].ncols;
                if (i == 0 && s == 0) width[j] = w;
                if (w != width[j])   // (the oracle's 100 + c)
                    throw std::runtime_error("CTL #" + std::to_string(j) + ": the column sets of the looking and looked tables differ in width");
                used[s * ntables + sd.table] = 1;
                h_sides.push_back(cc_side{sd.table, sd.colset, (uint32_t)tile, 0});
                tile += blocks_for((size_t)1 << t.log_n, CC_TILE);
                if (tile >= ((uint64_t)1 << 31)) throw std::runtime_error("CTL #" + std::to_string(j) + ": too many candidate rows");
            }
            ntiles[s * nctls + j] = (uint32_t)tile;
            side_off[s * nctls + j + 1] = h_sides.size();
        }
    // (the description is judged before the context is needed: a caller without a device still learns what is wrong with it)
    if (!c) throw std::runtime_error("check_ctls: null argument");
    ZKM_HIP_CHECK(hipSetDevice(c->device));
    // ---- the tables on the device: in place, or a copy of host memory / of one pointer per column.  Segments that share a table's
    // description (the same zkm_ctl_table and width) share its device copy
    // (what is too large for the context's pinned ring goes up straight from `held`, which outlives the call's first wait: the ring
    // would wait for the stream first, and that wait is one of the call's)
    std::vector<std::vector<char>> held;
    std::vector<zkm_scratch> copies;
    auto put = [&](void* dst, std::vector<char>&& h, size_t bytes) {
        if (bytes <= zkm_ctx::XFER_UP / 8) return c->upload(dst, h.data(), bytes);   // (`h` may go)
        held.push_back(std::move(h));
        ZKM_HIP_CHECK(hipMemcpyAsync(dst, held.back().data(), bytes, hipMemcpyHostToDevice, c->stream));
    };
    std::vector<ctl_dev> desc;
    std::map<std::pair<const zkm_ctl_table*, size_t>, size_t> desc_of;
    std::vector<cc_tab> h_tabs(nseg * ntables, cc_tab{});
    for (size_t s = 0; s < nseg; s++)
        for (size_t t = 0; t < ntables; t++) {
            if (!used[s * ntables + t]) continue;
            const zkm_table_input& in = tables[s][t];
            const size_t n = (size_t)1 << in.log_n;
            auto found = desc_of.find({in.ctl, in.ncols});
            if (found == desc_of.end()) {
                std::vector<char> h;
                const ctl_dev_packed p = ctl_dev_pack(in.ctl, nullptr, nullptr, 0, false, in.ncols, 1, h);
                const size_t bytes = h.size();
                copies.emplace_back(c, std::max<size_t>(bytes, 64));
                put(copies.back().p, std::move(h), bytes);
                desc.push_back(ctl_dev_rebase(p.d, copies.back().as<char>()));
                found = desc_of.emplace(std::make_pair(in.ctl, in.ncols), desc.size() - 1).first;
            }
            const gl_t* d_trace = in.trace;
            if (in.columns) {
                copies.emplace_back(c, in.ncols * n * 8);
                for (size_t k = 0; k < in.ncols; k++) {
                    if (!in.columns[k]) throw std::runtime_error("check_ctls: null column");
                    ZKM_HIP_CHECK(hipMemcpyAsync(copies.back().as<gl_t>() + k * n, in.columns[k], n * 8, hipMemcpyDefault, c->stream));
                }
                d_trace = copies.back().as<gl_t>();
            } else if (!zkm_is_device_ptr(in.trace)) {
                copies.emplace_back(c, in.ncols * n * 8);
                ZKM_HIP_CHECK(hipMemcpyAsync(copies.back().p, in.trace, in.ncols * n * 8, hipMemcpyHostToDevice, c->stream));
                d_trace = copies.back().as<gl_t>();
            }
            h_tabs[s * ntables + t] = cc_tab{desc[found->second], d_trace, n};
        }
    if (nctls == 0) {
        if (ride && ride->bytes) {
            c->download(ride->dst, ride->src, ride->bytes);
            host_waits++;
            stamp();
        }
        return nseg;
    }
    // ---- one block for the descriptors and the jobs' result words, all segments': [tabs | sides | res (2 per job) | ver (4 per job) | report]
    auto al = [](size_t x) { return (x + 63) & ~(size_t)63; };
    const size_t o_sides = al(h_tabs.size() * sizeof(cc_tab)), o_res = al(o_sides + h_sides.size() * sizeof(cc_side)), o_ver = al(o_res + njobs * 16),
                 o_rep = al(o_ver + njobs * 32), total = o_rep + nseg * CC_REPORT_WORDS * 8;
    zkm_scratch block(c, total);
    char* const base = block.as<char>();
    const cc_tab* d_tabs = (const cc_tab*)base;
    const cc_side* d_sides = (const cc_side*)(base + o_sides);
    unsigned long long* d_res = (unsigned long long*)(base + o_res);
    unsigned long long* d_ver = (unsigned long long*)(base + o_ver);
    uint64_t* d_rep = (uint64_t*)(base + o_rep);
    auto upload_pieces = [&](void* dst, const void* src, size_t bytes) {   // (through the context's pinned ring, in pieces it takes without a wait)
        constexpr size_t PIECE = zkm_ctx::XFER_UP / 8;
        for (size_t o = 0; o < bytes; o += PIECE) c->upload((char*)dst + o, (const char*)src + o, std::min(PIECE, bytes - o));
    };
    {
        std::vector<char> h(o_ver, 0);
        memcpy(h.data(), h_tabs.data(), h_tabs.size() * sizeof(cc_tab));
        memcpy(h.data() + o_sides, h_sides.data(), h_sides.size() * sizeof(cc_side));
        for (size_t q = 0; q < njobs; q++) ((uint64_t*)(h.data() + o_res))[2 * q] = CC_NONE;
        put(base, std::move(h), o_ver);
    }
    std::vector<cc_job> jobs(njobs, cc_job{});
    std::vector<zkm_scratch> cnt, part;
    std::vector<scan_seg> scans;
    for (size_t q = 0; q < njobs; q++) {
        cnt.emplace_back(c, ((size_t)ntiles[q] + 1) * 8);
        part.emplace_back(c, blocks_for((size_t)ntiles[q] + 1, SCAN_TILE) * 8);
        ZKM_HIP_CHECK(hipMemsetAsync(cnt.back().as<uint64_t>() + ntiles[q], 0, 8, c->stream));
        cc_job& J = jobs[q];
        J.tabs = d_tabs + (q / nctls) * ntables;
        J.sides = d_sides + side_off[q];
        J.nsides = (uint32_t)(side_off[q + 1] - side_off[q]);
        J.width = width[q % nctls];
        J.ntiles = ntiles[q];
        J.cnt = cnt.back().as<uint64_t>();
        J.res = d_res + 2 * q;
        J.ver = d_ver + 4 * q;
        scans.push_back(scan_seg{J.cnt, (size_t)ntiles[q] + 1, part.back().as<uint64_t>(), (uint64_t*)(J.res + 1)});
    }
    auto tiles_of = [](const cc_job& J) { return (size_t)J.ntiles; };
    launch_jobs(c, "check_ctls/count", k_cc_count, jobs, tiles_of);
    scan_jobs(c, scans);
    std::vector<uint64_t> h_res(2 * njobs);
    c->download(h_res.data(), d_res, njobs * 16);
    host_waits++;
    stamp();
    // ---- the records
    std::vector<zkm_scratch> store;
    std::vector<radix_seg> rx(njobs);
    std::vector<uint64_t*> keys_b(njobs);   // the sort's second buffers
    std::vector<uint32_t*> idx_b(njobs);
    size_t max_rec = 0;
    std::vector<scan_seg> scans_sgn, scans_flg;   // (a list each: a call's launches are one segment's times ceil(jobs / ZKM_MAX_SEG))
    for (size_t q = 0; q < njobs; q++) {
        const size_t nrec = (size_t)h_res[2 * q + 1];
        if (nrec > CC_MAX_RECORDS) throw std::runtime_error("CTL #" + std::to_string(q % nctls) + ": more than 2^30 filtered rows");
        max_rec = std::max(max_rec, nrec);
        cc_job& J = jobs[q];
        J.nrec = (uint32_t)nrec;
        auto take = [&](size_t bytes) {
            store.emplace_back(c, std::max<size_t>(bytes, 64));
            return store.back().p;
        };
        const uint32_t rtiles = (uint32_t)blocks_for(nrec, MT_TILE);
        J.loc = (uint64_t*)take(nrec * 8);
        J.keys = (uint64_t*)take(2 * nrec * 8);
        J.idx = (uint32_t*)take(nrec * 4);
        J.sgn = (uint64_t*)take((nrec + 1) * 8);
        J.flg = (uint64_t*)take((nrec + 1) * 8);
        J.head = (uint32_t*)take(nrec * 4);
        J.end = (uint64_t*)take(nrec * 8);
        uint32_t* hist = (uint32_t*)take(((size_t)MT_RADIX * rtiles + MT_RADIX) * 4);
        keys_b[q] = (uint64_t*)take(2 * nrec * 8);
        idx_b[q] = (uint32_t*)take(nrec * 4);
        rx[q] = radix_seg{J.keys, keys_b[q], J.idx, idx_b[q], hist, hist + (size_t)MT_RADIX * rtiles, (uint32_t)nrec, rtiles, 2};
        scans_sgn.push_back(scan_seg{J.sgn, nrec + 1, (uint64_t*)take(blocks_for(nrec + 1, SCAN_TILE) * 8), nullptr});
        scans_flg.push_back(scan_seg{J.flg, nrec + 1, (uint64_t*)take(blocks_for(nrec + 1, SCAN_TILE) * 8), (uint64_t*)(J.ver + 2)});
    }
    launch_jobs(c, "check_ctls/emit", k_cc_emit, jobs, tiles_of);
    auto recs_of = [](const cc_job& J) { return blocks_for(J.nrec, CC_THREADS); };
    auto recs1_of = [](const cc_job& J) { return blocks_for((size_t)J.nrec + 1, CC_THREADS); };
    std::vector<uint64_t> h_ver(4 * njobs), ver_init(4 * njobs, 0);
    for (size_t q = 0; q < njobs; q++) ver_init[4 * q + 1] = CC_NONE;
    for (int attempt = 1; attempt <= CC_MAX_ATTEMPTS; attempt++) {
        attempts = (uint32_t)attempt;
        const unsigned bits = attempt == 1 && c->debug_ctl_key_bits ? std::min<unsigned>(c->debug_ctl_key_bits, CC_KEY_BITS) : CC_KEY_BITS;
        upload_pieces(d_ver, ver_init.data(), njobs * 32);
        launch_jobs(c, "check_ctls/keys", k_cc_keys, jobs, recs_of, cc_mix(0x5a4b4d43544cull + (uint64_t)attempt), bits);
        if (max_rec) {
            for (size_t q = 0; q < njobs; q++) {   // (every attempt starts from the buffers k_cc_keys writes)
                rx[q].kin = jobs[q].keys;
                rx[q].kout = keys_b[q];
                rx[q].iin = jobs[q].idx;
                rx[q].iout = idx_b[q];
            }
            for (unsigned bit = 0; bit < bits; bit += 8) {
                for (size_t g0 = 0; g0 < njobs; g0 += ZKM_MAX_SEG) {
                    const size_t k = std::min<size_t>(ZKM_MAX_SEG, njobs - g0);
                    size_t rtiles = 0;   // (of the group's largest job)
                    for (size_t q = g0; q < g0 + k; q++) rtiles = std::max<size_t>(rtiles, rx[q].ntiles);
                    {
                        zkm_prof_scope ps(c, "check_ctls/radix_upsweep");
                        zkm_launch_segs(c->stream, k_radix_upsweep, rx.data() + g0, k, rtiles, MT_THREADS, bit);
                    }
                    {
                        zkm_prof_scope ps(c, "check_ctls/radix_scan");
                        zkm_launch_segs(c->stream, k_radix_scan, rx.data() + g0, k, MT_RADIX, MT_THREADS);
                    }
                    {
                        zkm_prof_scope ps(c, "check_ctls/radix_downsweep");
                        zkm_launch_segs(c->stream, k_radix_downsweep, rx.data() + g0, k, rtiles, MT_THREADS, bit);
                    }
                }
                for (size_t q = 0; q < njobs; q++) {
                    std::swap(rx[q].kin, rx[q].kout);
                    std::swap(rx[q].iin, rx[q].iout);
                }
            }
        }
        std::vector<cc_job> sorted = jobs;   // the same jobs reading the buffers the last pass wrote
        for (size_t q = 0; q < njobs; q++) {
            sorted[q].keys = rx[q].kin;
            sorted[q].idx = rx[q].iin;
        }
        launch_jobs(c, "check_ctls/flags", k_cc_flags, sorted, recs1_of);
        scan_jobs(c, scans_sgn);
        scan_jobs(c, scans_flg);
        launch_jobs(c, "check_ctls/mark", k_cc_mark, sorted, recs_of);
        launch_jobs(c, "check_ctls/verdict", k_cc_verdict, sorted, recs_of);
        // (what rides along is complete behind the first attempt: a second attempt brings the verdicts alone)
        if (attempt == 1 && ride) c->download({zkm_ctx::xfer{h_ver.data(), d_ver, njobs * 32}, *ride});
        else c->download(h_ver.data(), d_ver, njobs * 32);
        host_waits++;
        stamp();
        bool confirmed = true;
        for (size_t q = 0; q < njobs; q++) confirmed = confirmed && !h_ver[4 * q];
        if (!confirmed) continue;
        // ---- per segment the lowest failing lookup; within it a non-binary filter wins.  The reports of all failing segments come
        // down together
        std::vector<size_t> failing, lookup;   // segment, its lookup
        for (size_t s = 0; s < nseg; s++) {
            size_t j = 0;
            while (j < nctls && h_res[2 * (s * nctls + j)] == CC_NONE && h_ver[4 * (s * nctls + j) + 1] == CC_NONE) j++;
            if (j == nctls) continue;
            failing.push_back(s);
            lookup.push_back(j);
        }
        if (failing.empty()) return nseg;
        ZKM_HIP_CHECK(hipMemsetAsync(d_rep, 0, failing.size() * CC_REPORT_WORDS * 8, c->stream));
        for (size_t f = 0; f < failing.size(); f++) {
            const size_t q = failing[f] * nctls + lookup[f];
            zkm_prof_scope ps(c, "check_ctls/report");
            hipLaunchKernelGGL(k_cc_report, dim3(1), dim3(CC_THREADS), 0, c->stream, sorted[q], (unsigned long long)h_res[2 * q], (uint32_t)h_ver[4 * q + 1],
                               d_rep + f * CC_REPORT_WORDS);
            ZKM_HIP_CHECK(hipGetLastError());
        }
        std::vector<uint64_t> h_rep(failing.size() * CC_REPORT_WORDS);
        c->download(h_rep.data(), d_rep, h_rep.size() * 8);
        host_waits++;
        stamp();
        for (size_t f = 0; f < failing.size(); f++) {
            const size_t s = failing[f], j = lookup[f], q = s * nctls + j;
            const uint64_t* out = h_rep.data() + f * CC_REPORT_WORDS;
            zkm_ctl_report* rep = reps + s;
            const zkm_table_input* tabs = tables[s];
            rep->ctl = (uint32_t)j;
            const cc_side* js = h_sides.data() + side_off[q];
            if (h_res[2 * q] != CC_NONE) {
                rep->kind = 1;
                rep->side = (uint32_t)(h_res[2 * q] >> 32);
                rep->table = js[rep->side].table;
                rep->row = (uint32_t)h_res[2 * q];
                rep->filter_value = out[0];
                msgs[s] = "CTL #" + std::to_string(j) + ": Non-binary filter? (side " + std::to_string(rep->side) + ", table " + table_label(tabs, rep->table) +
                          ", row " + std::to_string(rep->row) + ": the filter is " + std::to_string(rep->filter_value) + ")";
                continue;
            }
            rep->kind = 2;
            rep->width = width[j];
            rep->nwords = std::min<uint32_t>(width[j], ZKM_CTL_REPORT_WORDS);
            memcpy(rep->tuple, out + 3, rep->nwords * 8);
            rep->looking_count = out[1];
            rep->looked_count = out[2];
            rep->nlooking_locations = (uint32_t)std::min<uint64_t>(out[1], ZKM_CTL_REPORT_LOCATIONS);
            rep->nlooked_locations = (uint32_t)std::min<uint64_t>(out[2], ZKM_CTL_REPORT_LOCATIONS);
            auto fill = [&](zkm_ctl_location* l, const uint64_t* w, uint32_t k) {
                for (uint32_t i = 0; i < k; i++) l[i] = zkm_ctl_location{(uint32_t)(w[i] >> 32), js[w[i] >> 32].table, (uint32_t)w[i]};
            };
            fill(rep->looking, out + 3 + ZKM_CTL_REPORT_WORDS, rep->nlooking_locations);
            fill(rep->looked, out + 3 + ZKM_CTL_REPORT_WORDS + ZKM_CTL_REPORT_LOCATIONS, rep->nlooked_locations);
            std::string row = "[";
            for (uint32_t k = 0; k < rep->nwords; k++) row += (k ? ", " : "") + std::to_string(rep->tuple[k]);
            if (rep->width > rep->nwords) row += ", ...";
            msgs[s] = "CTL #" + std::to_string(j) + ": Row " + row + "] is present " + std::to_string(out[1]) + " times in the looking tables, but " +
                      std::to_string(out[2]) + " times in the looked table. Looking locations (Table, Row index): " +
                      locations_text(tabs, rep->looking, rep->nlooking_locations, out[1]) + ". Looked locations (Table, Row index): " +
                      locations_text(tabs, rep->looked, rep->nlooked_locations, out[2]) + ".";
        }
        return failing[0];
    }
    throw std::runtime_error("check_ctls: the keys of different rows collided in " + std::to_string(CC_MAX_ATTEMPTS) + " attempts");
}

// ... on one segment's tables: the report's kind
int zkm_check_ctls_run(zkm_ctx* c, const zkm_table_input* tables, size_t ntables, const zkm_cross_table_lookup* ctls, const zkm_ctl_side* sides,
                       size_t nctls, zkm_ctl_report* rep, std::string* msg) {
    if ((!tables && ntables) || (nctls && (!ctls || !sides))) throw std::runtime_error("check_ctls: null argument");
    rep->attempts = 0;
    rep->host_waits = 0;
    zkm_check_ctls_run_segments(c, 1, &tables, ntables, ctls, sides, nctls, rep, msg);
    return (int)rep->kind;
}

namespace {

template <class F> int check_entry(const char* what, zkm_ctl_report* report, char** err, F&& body) {
    zkm_ctl_report local;
    zkm_ctl_report* rep = report ? report : &local;
    memset(rep, 0, sizeof *rep);
    std::string msg;
    const int rc = zkm_api(what, err, [&] { body(rep, &msg); });
    if (rc) {
        rep->kind = 3;
        return rc;
    }
    return rep->kind ? zkm_fail(err, msg.c_str()) : 0;
}

}  // namespace

extern "C" {

int zkm_check_ctls(zkm_ctx* c, const zkm_table_input* tables, size_t ntables, const zkm_cross_table_lookup* ctls, const zkm_ctl_side* sides,
                   size_t nctls, zkm_ctl_report* report, char** err) {
    return check_entry("zkm_check_ctls", report, err,
                       [&](zkm_ctl_report* rep, std::string* msg) { zkm_check_ctls_run(c, tables, ntables, ctls, sides, nctls, rep, msg); });
}

int zkm_segment_check_ctls(zkm_ctx* c, const uint64_t* const* traces, const unsigned* log_n, zkm_ctl_report* report, char** err) {
    return check_entry("zkm_segment_check_ctls", report, err, [&](zkm_ctl_report* rep, std::string* msg) {
        if (!traces || !log_n) throw std::runtime_error("zkm_segment_check_ctls: null argument");
        const zkm_cross_table_lookup* ctls;
        const zkm_ctl_side* sides;
        size_t nctls, nsides;
        zkm_all_stark_ctls(&ctls, &nctls, &sides, &nsides);
        zkm_table_input tables[ZKM_NUM_TABLES];
        zkm_all_stark_table_inputs(tables);   // Table::all() order
        for (int t = 0; t < ZKM_NUM_TABLES; t++) {
            tables[t].trace = traces[t];
            tables[t].log_n = log_n[t];
        }
        zkm_check_ctls_run(c, tables, ZKM_NUM_TABLES, ctls, sides, nctls, rep, msg);
    });
}

}  // extern "C"
