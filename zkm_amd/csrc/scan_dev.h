// scan_dev.h -- block-wide inclusive scan and a three-launch exclusive saturating scan of uint64 counts (memory_trace.hip: rows per
// sorted memory op; arithmetic_trace.hip: rows per arithmetic op), K independent scans a launch (zkm_seg_args: the scan from
// blockIdx.z).  Kernels with internal linkage: each including file has its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "zkm_internal.h"

namespace {

constexpr int SCAN_THREADS = 256;
constexpr int SCAN_WAVES = SCAN_THREADS / 64;
constexpr int SCAN_ITEMS = 8;                          // values per lane and tile
constexpr int SCAN_TILE = SCAN_THREADS * SCAN_ITEMS;   // 2048 values per tile
constexpr uint64_t SCAN_SAT = 1ull << 62;              // sums saturate here

__device__ __forceinline__ uint64_t sat_add(uint64_t a, uint64_t b) {   // a, b <= SCAN_SAT
    uint64_t s = a + b;
    return s > SCAN_SAT ? SCAN_SAT : s;
}

struct add_u32 { __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a + b; } };
struct add_sat { __device__ uint64_t operator()(uint64_t a, uint64_t b) const { return sat_add(a, b); } };

// inclusive scan over the block (identity 0); *total = the block's sum.  sh: SCAN_WAVES words of LDS.  Every thread must call it.
template <class T, class Op>
__device__ __forceinline__ T block_incl_scan(T v, T* sh, Op op, T* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        T u = __shfl_up(v, o);
        if (lane >= o) v = op(u, v);
    }
    if (lane == 63) sh[w] = v;
    __syncthreads();
    T pre = 0, all = 0;
#pragma unroll
    for (int q = 0; q < SCAN_WAVES; q++) {
        if (q < w) pre = op(pre, sh[q]);
        all = op(all, sh[q]);
    }
    __syncthreads();
    *total = all;
    return op(pre, v);
}

// exclusive saturating scan of v[0, len) in place: per-tile sums, a one-block scan of those, then the tiles.  part: one word per tile;
// total (optional): a second home for v[len - 1] after the scan -- the sum, when the caller put a zero behind its counts
struct scan_seg {
    uint64_t* v;
    size_t len;
    uint64_t *part, *total;
    GL_HD size_t nparts() const { return (len + SCAN_TILE - 1) / SCAN_TILE; }
};
__global__ __launch_bounds__(SCAN_THREADS) void k_scan_tiles(zkm_seg_args<scan_seg> S) {
    __shared__ uint64_t sh[SCAN_WAVES];
    const scan_seg& A = S.v[blockIdx.z];
    const size_t base = (size_t)blockIdx.x * SCAN_TILE + (size_t)threadIdx.x * SCAN_ITEMS;
    if ((size_t)blockIdx.x * SCAN_TILE >= A.len) return;
    uint64_t s = 0;
#pragma unroll
    for (int it = 0; it < SCAN_ITEMS; it++)
        if (base + it < A.len) s = sat_add(s, A.v[base + it]);
    uint64_t all;
    block_incl_scan(s, sh, add_sat(), &all);
    if (threadIdx.x == 0) A.part[blockIdx.x] = all;
}
__global__ __launch_bounds__(SCAN_THREADS) void k_scan_parts(zkm_seg_args<scan_seg> S) {
    __shared__ uint64_t sh[SCAN_WAVES];
    const scan_seg& A = S.v[blockIdx.z];
    uint64_t* __restrict__ part = A.part;
    const size_t nparts = A.nparts();
    uint64_t carry = 0;
    for (size_t c = 0; c < nparts; c += SCAN_THREADS) {
        const size_t t = c + threadIdx.x;
        const uint64_t x = t < nparts ? part[t] : 0;
        uint64_t all;
        const uint64_t incl = block_incl_scan(x, sh, add_sat(), &all);
        if (t < nparts) part[t] = sat_add(carry, incl >= SCAN_SAT ? SCAN_SAT : incl - x);   // exact unless the table is rejected
        carry = sat_add(carry, all);
    }
}
__global__ __launch_bounds__(SCAN_THREADS) void k_scan_apply(zkm_seg_args<scan_seg> S) {
    __shared__ uint64_t sh[SCAN_WAVES];
    const scan_seg& A = S.v[blockIdx.z];
    const size_t len = A.len;
    if ((size_t)blockIdx.x * SCAN_TILE >= len) return;
    uint64_t* __restrict__ v = A.v;
    const size_t base = (size_t)blockIdx.x * SCAN_TILE + (size_t)threadIdx.x * SCAN_ITEMS;
    uint64_t x[SCAN_ITEMS], s = 0;
#pragma unroll
    for (int it = 0; it < SCAN_ITEMS; it++) {
        x[it] = base + it < len ? v[base + it] : 0;
        s = sat_add(s, x[it]);
    }
    uint64_t all;
    const uint64_t incl = block_incl_scan(s, sh, add_sat(), &all);
    // exclusive prefix of this thread: the block's inclusive scan minus its own sum (exact when nothing saturated; otherwise both are
    // SCAN_SAT and the caller rejects the table anyway)
    uint64_t run = sat_add(A.part[blockIdx.x], incl >= SCAN_SAT ? SCAN_SAT : incl - s);
#pragma unroll
    for (int it = 0; it < SCAN_ITEMS; it++) {
        if (base + it < len) v[base + it] = run;
        if (base + it + 1 == len && A.total) *A.total = run;
        run = sat_add(run, x[it]);
    }
}
// the three launches for nseg scans (every len >= 1) on `stream`
inline void scan_launch(hipStream_t stream, const scan_seg* segs, size_t nseg) {
    size_t grid = 0;
    for (size_t s = 0; s < nseg; s++) grid = std::max(grid, segs[s].nparts());
    zkm_launch_segs(stream, k_scan_tiles, segs, nseg, grid, SCAN_THREADS);
    zkm_launch_segs(stream, k_scan_parts, segs, nseg, 1, SCAN_THREADS);
    zkm_launch_segs(stream, k_scan_apply, segs, nseg, grid, SCAN_THREADS);
}

}  // namespace
