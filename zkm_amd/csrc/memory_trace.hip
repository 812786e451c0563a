// memory_trace.hip -- MemoryStark witness from the raw memory operations (memory_stark.rs:135-248, oracle/ctl.c zko_memory_trace).
//
// The reference sorts the operations by (context, segment, virt, timestamp), appends the dummy reads of fill_gaps, pads with copies
// of the last operation pushed, sorts again and then builds the rows.  Here:
//   (1) k_mem_widths     OR of every key field (and a check that each is below p): the significant bits of the key;
//   (2) k_mem_pack       the four fields packed into the fewest 64-bit words (timestamp lowest), plus the original index;
//   (3) radix passes     a stable LSD sort of (key words, index), 8 bits a pass over the significant bits only: upsweep (per-tile
//                        digit histograms), per-digit scan over the tiles, downsweep (in-tile stable rank from wave64 ballot
//                        match masks, scatter).  Every hand-off between workgroups is a kernel boundary;
//   (4) k_mem_gaps       the number of dummy rows after each sorted operation in closed form (fill_gaps :175-204), and the last
//                        operation that has any;
//   (5) scan             exclusive saturating scan of 1 + dummies: each operation's first row; the total is the table's height;
//   (6) k_mem_rows       one thread per output row: the second sort is not needed, since every dummy lies strictly between its
//                        pair's keys; the pad rows (copies of the last operation pushed, :206-224) go right behind that row;
//   (7) k_mem_neighbours first-change flags, RANGE_CHECK, COUNTER and the FREQUENCIES histogram (:83-166).
// Only the key widths and the row count come back to the host before the output is written.
// Every kernel serves K segments in one launch (zkm_seg_args: its segment's descriptor from blockIdx.z); a lone table is K = 1.
#include <algorithm>
#include <vector>

#include "radix_dev.h"
#include "scan_dev.h"
#include "zkm_internal.h"

namespace {

constexpr uint64_t MT_SAT = SCAN_SAT;                // row counts saturate here (one timestamp gap can ask for 2^40 dummies)
constexpr int MT_HIST_LDS = 2048;                    // FREQUENCIES bins kept in LDS (range checks are mostly small)
constexpr unsigned MT_MAX_LOG_N = ZKM_MEMORY_MAX_LOG_N;

struct mem_op {
    uint64_t ctx, seg, virt, ts, is_read, value;
};
__device__ __forceinline__ mem_op load_op(const uint64_t* __restrict__ ops, uint32_t i) {
    const uint64_t* o = ops + (size_t)6 * i;
    return mem_op{o[0], o[1], o[2], o[3], o[4], o[5]};
}

// bit layout of the packed key: field f (0 context, 1 segment, 2 virt, 3 timestamp) at bits [shift[f], shift[f] + width[f])
struct key_layout {
    unsigned width[4], shift[4], nwords, bits;
};

// ---- (1) key widths
struct widths_seg {
    const uint64_t* ops;
    size_t nops;
    unsigned long long* acc;
};
__global__ __launch_bounds__(MT_THREADS) void k_mem_widths(zkm_seg_args<widths_seg> S) {
    const widths_seg& A = S.v[blockIdx.z];
    const uint64_t* __restrict__ ops = A.ops;
    const size_t nops = A.nops;
    unsigned long long* acc = A.acc;
    uint64_t o[4] = {0, 0, 0, 0}, bad = 0;
    for (size_t i = (size_t)blockIdx.x * MT_THREADS + threadIdx.x; i < nops; i += (size_t)gridDim.x * MT_THREADS) {
#pragma unroll
        for (int f = 0; f < 4; f++) {
            uint64_t v = ops[6 * i + f];
            o[f] |= v;
            bad |= v >= GL_P;
        }
    }
#pragma unroll
    for (int s = 32; s; s >>= 1) {
#pragma unroll
        for (int f = 0; f < 4; f++) o[f] |= __shfl_xor(o[f], s);
        bad |= __shfl_xor(bad, s);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int f = 0; f < 4; f++)
            if (o[f]) atomicOr(&acc[f], (unsigned long long)o[f]);
        if (bad) atomicOr(&acc[4], 1ull);
    }
}

// ---- (2) pack: keys[q * nops + i] = word q of op i's key, idx[i] = i
struct pack_seg {
    const uint64_t* ops;
    uint64_t* keys;
    uint32_t* idx;
    uint32_t nops;
    key_layout L;
};
__global__ __launch_bounds__(MT_THREADS) void k_mem_pack(zkm_seg_args<pack_seg> S) {
    const pack_seg& A = S.v[blockIdx.z];
    const uint64_t* __restrict__ ops = A.ops;
    uint64_t* __restrict__ keys = A.keys;
    uint32_t* __restrict__ idx = A.idx;
    const uint32_t nops = A.nops;
    const key_layout& L = A.L;
    size_t i = (size_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (i >= nops) return;
    uint64_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int f = 0; f < 4; f++) {
        if (!L.width[f]) continue;
        const uint64_t v = ops[6 * i + f];
        const unsigned word = L.shift[f] >> 6, b = L.shift[f] & 63;
#pragma unroll
        for (unsigned q = 0; q < 4; q++) {   // (constant indices: w stays in registers)
            if (q == word) w[q] |= v << b;
            if (q == word + 1 && b && b + L.width[f] > 64) w[q] |= v >> (64 - b);
        }
    }
#pragma unroll
    for (unsigned q = 0; q < 4; q++)
        if (q < L.nwords) keys[(size_t)q * nops + i] = w[q];
    idx[i] = (uint32_t)i;
}

// ---- (3) radix sort: k_radix_upsweep / k_radix_scan / k_radix_downsweep (radix_dev.h)

// ---- (4) dummy rows after sorted op i (fill_gaps, memory_stark.rs:175-204; max_rc = M = next_pow2(nops) - 1):
//   same context and segment, virt differs by d:  while d - 1 > M { virt += M + 1 }  ->  (d - 1) / (M + 1) dummies
//   same address, timestamps differ by dt:         while dt > M { ts += M }          ->  dt > M ? (dt - 1) / M : 0
__device__ __forceinline__ uint64_t gap_dummies(const mem_op& a, const mem_op& b, uint64_t M) {
    if (a.ctx != b.ctx || a.seg != b.seg) return 0;
    if (a.virt != b.virt) return (b.virt - a.virt - 1) / (M + 1);
    const uint64_t dt = b.ts - a.ts;
    return dt > M ? (dt - 1) / M : 0;
}

// cnt[i] = 1 + dummies after sorted op i (saturated); *last = 1 + the last sorted op with dummies (atomicMax; 0: none)
struct gaps_seg {
    const uint64_t* ops;
    const uint32_t* idx;
    uint64_t* cnt;
    unsigned* last;
    uint64_t M;
    uint32_t nops;
};
__global__ __launch_bounds__(MT_THREADS) void k_mem_gaps(zkm_seg_args<gaps_seg> S) {
    const gaps_seg& A = S.v[blockIdx.z];
    const uint64_t* __restrict__ ops = A.ops;
    const uint32_t* __restrict__ idx = A.idx;
    uint64_t* __restrict__ cnt = A.cnt;
    const uint32_t nops = A.nops;
    const uint64_t M = A.M;
    const size_t i = (size_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (i >= nops) return;
    uint64_t k = 0;
    if (i + 1 < nops) k = gap_dummies(load_op(ops, idx[i]), load_op(ops, idx[i + 1]), M);
    cnt[i] = k >= MT_SAT ? MT_SAT : k + 1;
    if (k) atomicMax(A.last, (unsigned)(i + 1));
}

// ---- (5) exclusive saturating scan: k_scan_tiles / k_scan_parts / k_scan_apply (scan_dev.h)

// ---- (6) rows.  start[i] = first row of sorted op i (rows of the padding-free table), start[nops] = that table's height `count`.
// The padding (n - count copies of the last op pushed) goes right behind that op's row q - 1, q = start[last] (or count).
struct rows_args {
    const uint64_t* ops;
    const uint32_t* idx;
    const uint64_t* start;
    const unsigned* last;
    uint32_t nops;
    uint64_t M, pad;
    size_t n;
    gl_t* out;
};
__device__ __forceinline__ uint64_t pre_row(uint64_t r, uint64_t q, uint64_t pad) { return r < q ? r : r < q + pad ? q - 1 : r - pad; }
// the last i in [lo, hi] with start[i] <= p (start is strictly increasing, start[lo] <= p)
__device__ __forceinline__ uint32_t find_op(const uint64_t* __restrict__ start, uint64_t p, uint32_t lo, uint32_t hi) {
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (start[mid] <= p) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}
__global__ __launch_bounds__(MT_THREADS) void k_mem_rows(zkm_seg_args<rows_args> S) {
    __shared__ uint32_t range[2];
    const rows_args& A = S.v[blockIdx.z];
    const size_t n = A.n;
    if ((size_t)blockIdx.x * MT_THREADS >= n) return;
    gl_t* __restrict__ out = A.out;
    const unsigned lst = *A.last;
    const uint64_t q = A.start[lst ? lst : A.nops];
    const size_t r0 = (size_t)blockIdx.x * MT_THREADS, r = r0 + threadIdx.x;
    const size_t rl = r0 + MT_THREADS - 1 < n ? r0 + MT_THREADS - 1 : n - 1;
    if (threadIdx.x == 0) range[0] = find_op(A.start, pre_row(r0, q, A.pad), 0, A.nops - 1);
    if (threadIdx.x == 1) range[1] = find_op(A.start, pre_row(rl, q, A.pad), 0, A.nops - 1);
    __syncthreads();
    if (r >= n) return;
    const bool is_pad = r >= q && r < q + A.pad;
    const uint64_t p = pre_row(r, q, A.pad);
    const uint32_t i = find_op(A.start, p, range[0], range[1]);
    const uint64_t j = p - A.start[i];
    mem_op o = load_op(A.ops, A.idx[i]);
    uint64_t filter = 1, is_read = o.is_read != 0;
    if (j && i + 1 < A.nops) {
        const mem_op b = load_op(A.ops, A.idx[i + 1]);
        if (o.virt != b.virt) {   // (same context and segment: only such pairs have dummies)
            o.virt += j * (A.M + 1);
            o.ts = 0;
            o.value = 0;
        } else {
            o.ts += j * A.M;
        }
        filter = 0;
        is_read = 1;
    }
    uint64_t value = (uint32_t)o.value;
    if (is_pad) {
        filter = 0;
        is_read = 1;
    } else if (!is_read && o.ctx == 0 && o.seg == 4 && o.virt == 0) {
        value = 0;   // into_row (:68-76): a write to register 0 is stored as 0
    }
    out[0 * n + r] = filter;
    out[1 * n + r] = o.ts;
    out[2 * n + r] = is_read;
    out[3 * n + r] = o.ctx;
    out[4 * n + r] = o.seg;
    out[5 * n + r] = o.virt;
    out[6 * n + r] = value;
}

// ---- (7) generate_first_change_flags_and_rc (:83-130), COUNTER and FREQUENCIES (:161-166); column 12 zeroed by the caller
struct neighbours_seg {
    gl_t* out;
    size_t n;
    int* bad;
};
__global__ __launch_bounds__(MT_THREADS) void k_mem_neighbours(zkm_seg_args<neighbours_seg> S) {
    __shared__ uint32_t h[MT_HIST_LDS];
    const neighbours_seg& A = S.v[blockIdx.z];
    gl_t* __restrict__ out = A.out;
    const size_t n = A.n;
    int* __restrict__ bad = A.bad;
    if ((size_t)blockIdx.x * MT_THREADS >= n) return;
    for (int b = threadIdx.x; b < MT_HIST_LDS; b += MT_THREADS) h[b] = 0;
    __syncthreads();
    unsigned long long* freq = (unsigned long long*)(out + 12 * n);
    for (size_t r = (size_t)blockIdx.x * MT_THREADS + threadIdx.x; r < n; r += (size_t)gridDim.x * MT_THREADS) {
        uint64_t cfc = 0, sfc = 0, vfc = 0, rc = 0;
        if (r + 1 < n) {
            const uint64_t c0 = out[3 * n + r], c1 = out[3 * n + r + 1];
            const uint64_t s0 = out[4 * n + r], s1 = out[4 * n + r + 1];
            const uint64_t v0 = out[5 * n + r], v1 = out[5 * n + r + 1];
            cfc = c0 != c1;
            sfc = !cfc && s0 != s1;
            vfc = !cfc && !sfc && v0 != v1;
            // (rows are sorted and every key word is below p: the field differences are the integer ones)
            rc = cfc ? c1 - c0 - 1 : sfc ? s1 - s0 - 1 : vfc ? v1 - v0 - 1 : out[1 * n + r + 1] - out[1 * n + r];
        }
        out[7 * n + r] = cfc;
        out[8 * n + r] = sfc;
        out[9 * n + r] = vfc;
        out[10 * n + r] = rc;
        out[11 * n + r] = r;
        if (rc >= n) *bad = 1;
        else if (rc < MT_HIST_LDS) atomicAdd(&h[rc], 1u);
        else atomicAdd(&freq[rc], 1ull);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < MT_HIST_LDS && (size_t)b < n; b += MT_THREADS)
        if (h[b]) atomicAdd(&freq[b], (unsigned long long)h[b]);
}

unsigned bit_width(uint64_t v) { return v ? 64 - __builtin_clzll(v) : 0; }
size_t next_pow2(size_t v) {
    size_t p = 1;
    while (p < v) p <<= 1;
    return p;
}
size_t blocks_for(size_t items, size_t per) { return (items + per - 1) / per; }

}  // namespace

// ---- host phases (zkm_internal.h zkm_memory_job): zkm_memory_trace runs them back to back for one table, segment_ops.hip runs them
// for the K segments of a call and interleaves them with the other tables' so that one host wait serves several tables
void zkm_memory_widths(zkm_memory_job* j, size_t nseg) {
    zkm_ctx* c = j->c;
    widths_seg ws[ZKM_MAX_SEG];
    size_t grid = 0;
    for (size_t s = 0; s < nseg; s++) {
        if (j[s].nops == 0) throw std::runtime_error(std::string(j[s].what) + ": No memory ops?");
        if (j[s].nops >= ((size_t)1 << 32)) throw std::runtime_error(std::string(j[s].what) + ": 2^32 or more memory ops");
        if (!j[s].d_acc) {
            // small: [0, 5) OR of the key fields and the >= p flag, [5] last op with dummies, [6] range-check flag, [7] the row count
            j[s].small = zkm_scratch(c, 64);
            j[s].d_acc = j[s].small.as<unsigned long long>();
            j[s].d_count = j[s].small.as<uint64_t>() + 7;
            ZKM_HIP_CHECK(hipMemsetAsync(j[s].small.p, 0, 64, c->stream));
        }
        ws[s] = widths_seg{j[s].d_ops, j[s].nops, j[s].d_acc};
        grid = std::max(grid, std::min<size_t>(blocks_for(j[s].nops, MT_THREADS), 1024));
    }
    zkm_prof_scope ps(c, "memory_trace/widths");
    zkm_launch_segs(c->stream, k_mem_widths, ws, nseg, grid, MT_THREADS);
}

void zkm_memory_sort(zkm_memory_job* j, size_t nseg, const uint64_t* acc_all, size_t acc_stride) {
    zkm_ctx* c = j->c;
    pack_seg pk[ZKM_MAX_SEG];
    radix_seg rx[ZKM_MAX_SEG];
    gaps_seg gp[ZKM_MAX_SEG];
    scan_seg sc[ZKM_MAX_SEG];
    size_t max_ops = 0;
    unsigned max_bits = 0;
    for (size_t s = 0; s < nseg; s++) {
        const uint64_t* acc = acc_all + s * acc_stride;
        const size_t nops = j[s].nops;
        if (acc[4]) throw std::runtime_error(std::string(j[s].what) + ": a context, segment, virt or timestamp word is not below p");
        // key layout: timestamp lowest, then virt, segment, context
        key_layout L{};
        unsigned sh = 0;
        for (int f = 3; f >= 0; f--) {
            L.width[f] = bit_width(acc[f]);
            L.shift[f] = sh;
            sh += L.width[f];
        }
        L.bits = sh;
        L.nwords = sh ? (sh + 63) / 64 : 1;
        const size_t K = L.nwords;
        j[s].keys_a = zkm_scratch(c, K * nops * 8);
        j[s].keys_b = zkm_scratch(c, K * nops * 8);
        j[s].idx_a = zkm_scratch(c, nops * 4);
        j[s].idx_b = zkm_scratch(c, nops * 4);
        pk[s] = pack_seg{j[s].d_ops, j[s].keys_a.as<uint64_t>(), j[s].idx_a.as<uint32_t>(), (uint32_t)nops, L};
        rx[s] = radix_seg{j[s].keys_a.as<uint64_t>(), j[s].keys_b.as<uint64_t>(), j[s].idx_a.as<uint32_t>(), j[s].idx_b.as<uint32_t>(),
                          nullptr, nullptr, (uint32_t)nops, (uint32_t)blocks_for(nops, MT_TILE), L.nwords};
        max_ops = std::max(max_ops, nops);
        if (nops > 1) max_bits = std::max(max_bits, L.bits);
    }
    {
        zkm_prof_scope ps(c, "memory_trace/pack");
        zkm_launch_segs(c->stream, k_mem_pack, pk, nseg, blocks_for(max_ops, MT_THREADS), MT_THREADS);
    }
    if (max_bits) {
        std::vector<zkm_scratch> hist;   // per segment: the tile counts, then the digit totals
        for (size_t s = 0; s < nseg; s++) {
            hist.emplace_back(c, ((size_t)MT_RADIX * rx[s].ntiles + MT_RADIX) * 4);
            rx[s].hist = hist.back().as<uint32_t>();
            rx[s].tot = rx[s].hist + (size_t)MT_RADIX * rx[s].ntiles;
        }
        const size_t ntiles = blocks_for(max_ops, MT_TILE);
        zkm_prof_scope ps(c, "memory_trace/sort");
        for (unsigned bit = 0; bit < max_bits; bit += 8) {
            zkm_launch_segs(c->stream, k_radix_upsweep, rx, nseg, ntiles, MT_THREADS, bit);
            zkm_launch_segs(c->stream, k_radix_scan, rx, nseg, MT_RADIX, MT_THREADS);
            zkm_launch_segs(c->stream, k_radix_downsweep, rx, nseg, ntiles, MT_THREADS, bit);
            for (size_t s = 0; s < nseg; s++) {
                std::swap(rx[s].kin, rx[s].kout);
                std::swap(rx[s].iin, rx[s].iout);
            }
        }
    }
    // gaps and their scan: start[i] = first row of sorted op i, start[nops] = rows before padding (and *d_count)
    std::vector<zkm_scratch> part;
    for (size_t s = 0; s < nseg; s++) {
        const size_t nops = j[s].nops;
        j[s].idx = rx[s].iin;
        j[s].M = next_pow2(nops) - 1;
        j[s].start = zkm_scratch(c, (nops + 1) * 8);
        uint64_t* d_start = j[s].start.as<uint64_t>();
        part.emplace_back(c, blocks_for(nops + 1, MT_TILE) * 8);
        ZKM_HIP_CHECK(hipMemsetAsync(d_start + nops, 0, 8, c->stream));
        gp[s] = gaps_seg{j[s].d_ops, j[s].idx, d_start, (unsigned*)(j[s].d_acc + 5), j[s].M, (uint32_t)nops};
        sc[s] = scan_seg{d_start, nops + 1, part.back().as<uint64_t>(), j[s].d_count};
    }
    zkm_prof_scope ps(c, "memory_trace/gaps");
    zkm_launch_segs(c->stream, k_mem_gaps, gp, nseg, blocks_for(max_ops, MT_THREADS), MT_THREADS);
    scan_launch(c->stream, sc, nseg);
}

size_t zkm_memory_height(zkm_memory_job& j, uint64_t count, size_t* natural_rows_out) {
    if (count >= MT_SAT) {
        if (natural_rows_out) *natural_rows_out = (size_t)MT_SAT;
        throw std::runtime_error(std::string(j.what) + ": the dummy rows of fill_gaps do not fit (2^62 rows or more)");
    }
    j.count = count;
    const size_t natural = next_pow2(count);
    if (natural_rows_out) *natural_rows_out = natural;
    return natural;
}

void zkm_memory_write(zkm_memory_job* j, size_t nseg, const unsigned* log_n, gl_t* const* out_dev, int* const* d_bad) {
    zkm_ctx* c = j->c;
    rows_args ra[ZKM_MAX_SEG];
    neighbours_seg nb[ZKM_MAX_SEG];
    size_t max_n = 0;
    for (size_t s = 0; s < nseg; s++) {
        const size_t n = (size_t)1 << log_n[s];
        ra[s] = rows_args{j[s].d_ops, j[s].idx, j[s].start.as<uint64_t>(), (const unsigned*)(j[s].d_acc + 5), (uint32_t)j[s].nops, j[s].M,
                          n - j[s].count, n, out_dev[s]};
        nb[s] = neighbours_seg{out_dev[s], n, d_bad[s]};
        max_n = std::max(max_n, n);
        ZKM_HIP_CHECK(hipMemsetAsync(out_dev[s] + 12 * n, 0, n * 8, c->stream));
    }
    {
        zkm_prof_scope ps(c, "memory_trace/rows");
        zkm_launch_segs(c->stream, k_mem_rows, ra, nseg, blocks_for(max_n, MT_THREADS), MT_THREADS);
    }
    {
        zkm_prof_scope ps(c, "memory_trace/neighbours");
        zkm_launch_segs(c->stream, k_mem_neighbours, nb, nseg, std::min<size_t>(blocks_for(max_n, MT_THREADS), 1024), MT_THREADS);
    }
}

extern "C" int zkm_memory_trace(zkm_ctx* c, const uint64_t* ops, size_t nops, unsigned log_n, uint64_t* out_dev, size_t* natural_rows_out,
                                char** err) {
    return zkm_api("zkm_memory_trace", c, err, [&] {
        if (nops == 0) throw std::runtime_error("zkm_memory_trace: No memory ops?");
        if (nops >= ((size_t)1 << 32)) throw std::runtime_error("zkm_memory_trace: 2^32 or more memory ops");
        if (out_dev) {
            if (log_n > MT_MAX_LOG_N)
                throw std::runtime_error("zkm_memory_trace: log_n " + std::to_string(log_n) + " above the cap " + std::to_string(MT_MAX_LOG_N));
            if (!zkm_is_device_ptr(out_dev)) throw std::runtime_error("zkm_memory_trace: out must be a device pointer");
        }
        zkm_scratch_list host_copy(c);
        const uint64_t* d_ops = ops;
        if (!zkm_is_device_ptr(ops)) {
            d_ops = host_copy.alloc<uint64_t>(nops * 48);
            ZKM_HIP_CHECK(hipMemcpyAsync((void*)d_ops, ops, nops * 48, hipMemcpyHostToDevice, c->stream));
        }
        zkm_memory_job j(c, "zkm_memory_trace", d_ops, nops);
        zkm_memory_widths(&j, 1);
        uint64_t acc[5];
        c->download(acc, j.d_acc, sizeof(acc));
        zkm_memory_sort(&j, 1, acc, 0);
        uint64_t count = 0;
        c->download(&count, j.d_count, 8);
        const size_t natural = zkm_memory_height(j, count, natural_rows_out);
        if (!out_dev) return;
        const size_t n = (size_t)1 << log_n;
        if (natural > n)
            throw std::runtime_error("zkm_memory_trace: the table needs " + std::to_string(natural) + " rows, more than 2^" + std::to_string(log_n));
        int* d_bad = (int*)(j.d_acc + 6);
        gl_t* const out = out_dev;
        zkm_memory_write(&j, 1, &log_n, &out, &d_bad);
        int bad = 0;
        c->download(&bad, d_bad, sizeof(bad));
        if (bad) throw std::runtime_error("zkm_memory_trace: a range check is 2^log_n or more (a context or segment gap)");
    });
}
