// radix_dev.h -- the stable LSD radix sort of (key words, index) pairs, 8 bits a pass: upsweep (per-tile digit histograms), per-digit
// scan over the tiles, downsweep (in-tile stable rank from wave64 ballot match masks, scatter).  Every hand-off between workgroups is a
// kernel boundary.  Shared by memory_trace.hip (the Memory witness: operations by (context, segment, virt, timestamp)) and
// ctl_check.hip (check_ctls: lookup records by key), K independent sorts a launch (zkm_seg_args: the sort from blockIdx.z).  Kernels
// with internal linkage, as scan_dev.h's.
#pragma once
#include "scan_dev.h"
#include "zkm_internal.h"

namespace {

constexpr int MT_THREADS = SCAN_THREADS;
constexpr int MT_WAVES = SCAN_WAVES;
constexpr int MT_ITEMS = SCAN_ITEMS;                 // keys per lane and tile
constexpr int MT_TILE = SCAN_TILE;                   // 2048 keys per tile
constexpr int MT_RADIX = 256;                        // 8-bit digits

// ---- (3) radix sort, one 8-bit digit at bit `bit` of the key
// tile t = keys [t * MT_TILE, (t + 1) * MT_TILE); hist[d * ntiles + t] = keys of tile t with digit d.  The passes of a launch run to the
// widest segment's bit count: a digit at or above a segment's own key words is zero without a read (the sort is stable, so such a
// pass copies the segment in order and keeps its ping-pong parity with the others).
struct radix_seg {
    uint64_t *kin, *kout;    // keys and indices: this pass reads kin / iin and writes kout / iout
    uint32_t *iin, *iout;
    uint32_t *hist, *tot;    // 256 x ntiles tile counts, 256 digit totals
    uint32_t nops, ntiles;
    unsigned nwords;
};
__device__ __forceinline__ uint32_t digit_of(const uint64_t* __restrict__ kw, size_t i, unsigned sh, bool live) {
    return live ? (uint32_t)(kw[i] >> sh) & (MT_RADIX - 1) : 0;
}
__global__ __launch_bounds__(MT_THREADS) void k_radix_upsweep(zkm_seg_args<radix_seg> S, unsigned bit) {
    __shared__ uint32_t h[MT_RADIX];
    const radix_seg& A = S.v[blockIdx.z];
    if (blockIdx.x >= A.ntiles) return;
    const uint32_t nops = A.nops;
    h[threadIdx.x] = 0;
    __syncthreads();
    const bool live = (bit >> 6) < A.nwords;
    const uint64_t* kw = A.kin + (size_t)(bit >> 6) * nops;
    const unsigned sh = bit & 63;
    const size_t base = (size_t)blockIdx.x * MT_TILE;
#pragma unroll
    for (int it = 0; it < MT_ITEMS; it++) {
        size_t i = base + (size_t)it * MT_THREADS + threadIdx.x;
        if (i < nops) atomicAdd(&h[digit_of(kw, i, sh, live)], 1u);
    }
    __syncthreads();
    A.hist[(size_t)threadIdx.x * A.ntiles + blockIdx.x] = h[threadIdx.x];
}

// one block per digit: hist row d becomes its exclusive scan over the tiles, tot[d] the digit's total
__global__ __launch_bounds__(MT_THREADS) void k_radix_scan(zkm_seg_args<radix_seg> S) {
    __shared__ uint32_t sh[MT_WAVES];
    const radix_seg& A = S.v[blockIdx.z];
    uint32_t* __restrict__ hist = A.hist;
    uint32_t* __restrict__ tot = A.tot;
    const uint32_t ntiles = A.ntiles;
    uint32_t* row = hist + (size_t)blockIdx.x * ntiles;
    uint32_t carry = 0;
    for (uint32_t c = 0; c < ntiles; c += MT_THREADS) {
        const uint32_t t = c + threadIdx.x;
        const uint32_t v = t < ntiles ? row[t] : 0;
        uint32_t all;
        const uint32_t incl = block_incl_scan(v, sh, add_u32(), &all);
        if (t < ntiles) row[t] = carry + incl - v;
        carry += all;
    }
    if (threadIdx.x == 0) tot[blockIdx.x] = carry;
}

// Stable scatter.  Wave w of the block owns the contiguous run [tile + w 64 MT_ITEMS, + 64 MT_ITEMS) and walks it 64 keys at a time
// in input order; a key's rank among equal digits of its wave = the wave's running count of that digit + the equal-digit lanes below
// it (ballot match mask).  The waves' counts are then turned into exclusive offsets in wave order, on top of the digit's global base.
__global__ __launch_bounds__(MT_THREADS) void k_radix_downsweep(zkm_seg_args<radix_seg> S, unsigned bit) {
    __shared__ uint32_t cnt[MT_WAVES][MT_RADIX];
    __shared__ uint32_t dbase[MT_RADIX];
    __shared__ uint32_t sh[MT_WAVES];
    const radix_seg& A = S.v[blockIdx.z];
    if (blockIdx.x >= A.ntiles) return;
    const uint64_t* __restrict__ kin = A.kin;
    const uint32_t* __restrict__ iin = A.iin;
    uint64_t* __restrict__ kout = A.kout;
    uint32_t* __restrict__ iout = A.iout;
    const uint32_t* __restrict__ hist = A.hist;
    const uint32_t* __restrict__ tot = A.tot;
    const uint32_t nops = A.nops, ntiles = A.ntiles;
    const unsigned nwords = A.nwords;
    const bool live = (bit >> 6) < nwords;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < MT_WAVES; q++) cnt[q][threadIdx.x] = 0;
    {
        const uint32_t t = tot[threadIdx.x];
        uint32_t all;
        const uint32_t incl = block_incl_scan(t, sh, add_u32(), &all);
        dbase[threadIdx.x] = incl - t + hist[(size_t)threadIdx.x * ntiles + blockIdx.x];
    }
    __syncthreads();
    const uint64_t* kw = kin + (size_t)(bit >> 6) * nops;
    const unsigned shift = bit & 63;
    const size_t run = (size_t)blockIdx.x * MT_TILE + (size_t)w * 64 * MT_ITEMS;
    const uint64_t below = (1ull << lane) - 1;
    uint32_t dig[MT_ITEMS], rank[MT_ITEMS];
#pragma unroll
    for (int it = 0; it < MT_ITEMS; it++) {
        const size_t i = run + (size_t)it * 64 + lane;
        const bool valid = i < nops;
        const uint32_t d = digit_of(kw, i, shift, valid && live);
        uint64_t m = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; b++) {
            const bool on = (d >> b) & 1;
            const uint64_t bb = __ballot(on);
            m &= on ? bb : ~bb;
        }
        const uint32_t pre = cnt[w][d];
        __builtin_amdgcn_wave_barrier();
        dig[it] = d;
        rank[it] = pre + (uint32_t)__popcll(m & below);
        if (valid && 63 - __clzll(m) == lane) cnt[w][d] = pre + (uint32_t)__popcll(m);   // the group's highest lane publishes
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    {
        uint32_t off = dbase[threadIdx.x];
#pragma unroll
        for (int q = 0; q < MT_WAVES; q++) {
            const uint32_t c = cnt[q][threadIdx.x];
            cnt[q][threadIdx.x] = off;
            off += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < MT_ITEMS; it++) {
        const size_t i = run + (size_t)it * 64 + lane;
        if (i >= nops) continue;
        const uint32_t dst = cnt[w][dig[it]] + rank[it];
        iout[dst] = iin[i];
        for (unsigned q = 0; q < nwords; q++) kout[(size_t)q * nops + dst] = kin[(size_t)q * nops + i];
    }
}

}  // namespace
