// hash.hip -- Poseidon / Keccak-f / Merkle kernels for gfx950.
//
// K4  leaf hashing  == plonky2 MerkleTree::new leaf digests = PoseidonHash::hash_or_noop(row)
//     (overwrite-mode sponge, rate 8; rows of <= 4 elements are copied, not hashed -- SURVEY App. A.4)
// K5  inner nodes   == PoseidonHash::two_to_one(left, right), level by level up to the cap
// K15 Keccak-f[1600] batch (reference: cpu/kernel/keccak_util.rs:6-31 via tiny-keccak)
// (witness kernels: witness.hip)
//
// Layout: the LDE is column-major with rows already bit-reversed, so "leaf j" = element j of every
// column: lane = leaf, and each per-column load is a contiguous 512 B wave access -- the transpose
// (K3 in SURVEY §2.1) is fused into the hashing loads.  Integer VALU bound (not HBM, not MFMA).
#include <atomic>
#include "poseidon_dev.h"
#include "poseidon_lat_dev.h"
#include "poseidon_mfma_dev.h"
#include "hash_constants_dev.h"
#include "zkm_internal.h"

// five waves per SIMD (93 registers) with the layer's high-half sums parked in LDS, four (110 registers) without (poseidon_mfma_dev.h)
#ifndef ZKM_LEAF_MFMA_WAVES
#define ZKM_LEAF_MFMA_WAVES (ZKM_MFMA_PARK ? 5 : 4)
#endif

// The latency forms of the permutation (16 lanes or a quad per hash) exist for launches that are a CHAIN of dependent permutations
// with too few hashes to fill the machine: the top of every tree, the leaves of short tables, small FRI layers.  When such a launch
// shares the GPU with throughput kernels (the commit lanes of the same segment, other contexts), its few waves compete for issue
// slots with five resident waves per SIMD of somebody's leaf hashing, and every step of the chain waits its turn.  s_setprio raises
// the wave's priority at the SIMD's instruction arbiter: the chain runs at (nearly) its solo latency and the throughput kernel
// fills what is left.  ZKM_LATENCY_PRIO = 0 builds without it (A/B: profiles/r04_latency_prio.txt).
#ifndef ZKM_LATENCY_PRIO
#define ZKM_LATENCY_PRIO 3
#endif
#define ZKM_RAISE_PRIO()                                              \
    do {                                                              \
        if (ZKM_LATENCY_PRIO) __builtin_amdgcn_s_setprio(ZKM_LATENCY_PRIO); \
    } while (0)

// ------------------------------------------------------------------ Poseidon permutation batch
__global__ __launch_bounds__(256) void k_poseidon_permute(gl_t* states, size_t k) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= k) return;
    uint64_t s[12];
#pragma unroll
    for (int j = 0; j < 12; j++) s[j] = states[i * 12 + j];
    poseidon_permute(s);
#pragma unroll
    for (int j = 0; j < 12; j++) states[i * 12 + j] = s[j];
}

void zkm_launch_poseidon_permute(zkm_ctx* c, gl_t* states, size_t k) {
    if (!k) return;
    zkm_prof_scope ps(c, "poseidon_permute");
    hipLaunchKernelGGL(k_poseidon_permute, dim3((k + 255) / 256), dim3(256), 0, c->stream, states, k);
    ZKM_HIP_CHECK(hipGetLastError());
}

// ------------------------------------------------------------------ leaf sources
// A source answers "word m of the leaf, and how many words a leaf has" once seek(k) has put it on leaf k of the block's segment (every
// leaf / tree kernel: blockIdx.z = segment of a stacked batch, zkm_internal.h -- its matrix starts `seg` words, its digest block
// dig_seg words after the previous segment's).  WHOLE: the word count is a multiple of 8 (no ragged last chunk, and never the short
// leaf of hash_or_noop).
// Column-major matrix row: lde[m * col_stride + k] -- a wave's load of one column is contiguous.
struct leaf_cols {
    static constexpr bool WHOLE = false;
    const gl_t* lde;
    size_t ncols, col_stride, seg;
    __device__ __forceinline__ void seek(size_t k) { lde += (size_t)blockIdx.z * seg; lde += k; }
    __device__ __forceinline__ size_t words() const { return ncols; }
    __device__ __forceinline__ uint64_t word(size_t m) const { return lde[m * col_stride]; }
};
// FRI layer: leaf k = arity consecutive F2 values (bit-reversed order), flattened c0,c1,c0,c1.. -- word m of leaf k is component m & 1
// of value k * arity + (m >> 1).  2 * arity words, arity a multiple of 4 -> whole chunks of 8 words = 4 pairs.
struct leaf_f2 {
    static constexpr bool WHOLE = true;
    const gl_t* c0;
    const gl_t* c1;
    unsigned arity;
    size_t seg;
    __device__ __forceinline__ void seek(size_t k) {
        c0 += (size_t)blockIdx.z * seg; c1 += (size_t)blockIdx.z * seg;
        c0 += k * arity; c1 += k * arity;
    }
    __device__ __forceinline__ unsigned words() const { return 2 * arity; }
    __device__ __forceinline__ uint64_t word(unsigned m) const {
        const gl_t *a = c0, *b = c1;                      // (both read before the choice: a select of two values, not of two fields)
        return ((m & 1) ? b : a)[m >> 1];
    }
};

// ------------------------------------------------------------------ sponge forms
// One Poseidon state spread over 1, 4 or 16 lanes.  The state -- state_t, this lane's words of it -- is a local array of the routine
// that runs the sponge (as a member of the form the compiler keeps it in memory; as a local array it stays in registers across the
// absorb loop); a form is what a lane needs to work on it:
//   LANES                     lanes per hash
//   take(n)                   the item of an n-item launch this lane works on (item, live); false: the lane has nothing to do and leaves
//   clear(s)                  the empty sponge
//   load<RAGGED>(s, src, c, n) overwrite-mode absorb of words [c, c + 8) of the leaf the source is on; RAGGED: only the words below n exist
//                             and only those are overwritten
//   permute(s, out)           one permutation; out = what the caller reads of the result (POSEIDON_OUT_*, a hint)
//   compress(s, nodes, k, on) two_to_one of node pair k of a level (the eight words at nodes + 8 k) -- the latency forms
//   store_digest(s, d, k, on) digest k of a level
// In the latency forms `on` / `live` are uniform over the hash's lanes, and every lane of the wave takes part in every permutation
// (shuffles / DPP).

// One lane per hash.  MDS = poseidon_mds_mfma: the MDS layers of the full rounds run on the matrix core (poseidon_mfma_dev.h).  MFMA
// ignores EXEC, so that form keeps the lanes past the last item alive on the last item's data and only masks their store.
template <class MDS>
struct sponge_lane {
    static constexpr unsigned LANES = 1;
    static constexpr bool MFMA = std::is_same<MDS, poseidon_mds_mfma>::value;
    typedef uint64_t state_t[12];
    MDS mds;
    size_t item;
    bool live;
    __device__ __forceinline__ sponge_lane() {
        if constexpr (MFMA) {
            mds.A = poseidon_mfma_operand();
#if ZKM_MFMA_PARK
            __shared__ uint32_t park[24 * ZKM_MFMA_PARK_STRIDE];
            mds.park = park + threadIdx.x;
#endif
        }
    }
    __device__ __forceinline__ bool take(size_t n) {
        item = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
        live = item < n;
        if (!MFMA && !live) return false;
        if (!live) item = n - 1;
        return true;
    }
    __device__ __forceinline__ void clear(state_t& s) const {
#pragma unroll
        for (int i = 0; i < 12; i++) s[i] = 0;
    }
    template <bool RAGGED, class Src, class I>
    __device__ __forceinline__ void load(state_t& s, const Src& src, I c, I n) const {
        if (!RAGGED) {
            uint64_t v[8];
#pragma unroll
            for (int i = 0; i < 8; i++) v[i] = src.word(c + i);
#pragma unroll
            for (int i = 0; i < 8; i++) s[i] = v[i];
        } else {
#pragma unroll
            for (int i = 0; i < 8; i++)
                if ((I)i < n - c) s[i] = src.word(c + i);
        }
    }
    __device__ __forceinline__ void permute(state_t& s, int out) const { poseidon_permute_out_t(s, out, mds); }
    template <class Src>
    __device__ __forceinline__ void copy(state_t& s, const Src& src) const {
        for (size_t c = 0; c < src.words(); c++) s[c] = src.word(c);
    }
    template <class K>
    __device__ __forceinline__ void store_digest(const state_t& s, uint64_t* digests, K k, bool on) const {
        if (!on) return;
        uint64_t* d = digests + 4 * k;
        *reinterpret_cast<ulonglong2*>(d) = make_ulonglong2(s[0], s[1]);
        *reinterpret_cast<ulonglong2*>(d + 2) = make_ulonglong2(s[2], s[3]);
    }
    // the whole state of every item parked in HBM between two launches: state[i * n + item], lane-contiguous
    __device__ __forceinline__ void load_state(state_t& s, const gl_t* __restrict__ state, size_t n) const {
#pragma unroll
        for (int i = 0; i < 12; i++) s[i] = state[(size_t)i * n + item];
    }
    __device__ __forceinline__ void store_state(const state_t& s, gl_t* __restrict__ state, size_t n) const {
        if (!live) return;
#pragma unroll
        for (int i = 0; i < 12; i++) state[(size_t)i * n + item] = s[i];
    }
};

using sponge_lane_valu = sponge_lane<poseidon_mds_valu>;
using sponge_lane_mfma = sponge_lane<poseidon_mds_mfma>;

// A quad of lanes per hash (poseidon_lat_dev.h): lane q holds the state words q, q + 4, q + 8, and fetches words c + q and c + 4 + q of
// its leaf for the absorb step at word c.
struct sponge_quad {
    static constexpr unsigned LANES = 4;
    typedef uint64_t state_t[3];
    const poseidon_quad Q;
    const unsigned q;
    size_t item;
    bool live;
    // (every thread of the workgroup builds its form at the same place: the table load ends with a workgroup barrier)
    __device__ __forceinline__ sponge_quad() : Q(threadIdx.x, table()), q(threadIdx.x & 3) {}
    static __device__ __forceinline__ const uint32_t* table() {
        __shared__ __attribute__((aligned(16))) uint32_t qtab[ZKM_QUAD_TAB_WORDS];
        quad_tab_load(qtab);
        return qtab;
    }
    __device__ __forceinline__ bool take(size_t n) {
        item = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 2;
        live = item < n;
        return true;
    }
    __device__ __forceinline__ void clear(state_t& s) const { s[0] = s[1] = s[2] = 0; }
    template <bool RAGGED, class Src, class I>
    __device__ __forceinline__ void load(state_t& s, const Src& src, I c, I n) const {
        if (live && (!RAGGED || c + q < n)) s[0] = src.word(c + q);
        if (live && (!RAGGED || c + 4 + q < n)) s[1] = src.word(c + 4 + q);
    }
    __device__ __forceinline__ void permute(state_t& s, int) const { poseidon_permute_quad(s, Q); }
    template <class K>
    __device__ __forceinline__ void compress(state_t& s, const uint64_t* nodes, K k, bool on) const {
        s[0] = on ? nodes[8 * k + q] : 0;
        s[1] = on ? nodes[8 * k + 4 + q] : 0;
        s[2] = 0;
        permute(s, POSEIDON_OUT_DIGEST);
    }
    template <class K>
    __device__ __forceinline__ void store_digest(const state_t& s, uint64_t* digests, K k, bool on) const {
        if (on) digests[4 * k + q] = s[0];
    }
};

// A 16-lane row per hash (poseidon_permute_wide): lanes 0..11 of the row hold the twelve state words, lanes 0..7 fetch the next eight
// words of their leaf.
struct sponge_wide {
    static constexpr unsigned LANES = 16;
    typedef uint64_t state_t[1];
    const unsigned lane, idx;
    size_t item;
    bool live;
    __device__ __forceinline__ sponge_wide() : lane(threadIdx.x & 63), idx(lane & 15) {}
    __device__ __forceinline__ bool take(size_t n) {
        item = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
        live = item < n;
        return true;
    }
    __device__ __forceinline__ void clear(state_t& s) const { s[0] = 0; }
    template <bool RAGGED, class Src, class I>
    __device__ __forceinline__ void load(state_t& s, const Src& src, I c, I n) const {
        if (live && idx < 8 && (!RAGGED || c + idx < n)) s[0] = src.word(c + idx);
    }
    __device__ __forceinline__ void permute(state_t& s, int) const { s[0] = poseidon_permute_wide(s[0], lane); }
    template <class K>
    __device__ __forceinline__ void compress(state_t& s, const uint64_t* nodes, K k, bool on) const {
        s[0] = (on && idx < 8) ? nodes[8 * k + idx] : 0;
        permute(s, POSEIDON_OUT_DIGEST);
    }
    template <class K>
    __device__ __forceinline__ void store_digest(const state_t& s, uint64_t* digests, K k, bool on) const {
        if (on && idx < 4) digests[4 * k + idx] = s[0];
    }
};

// ------------------------------------------------------------------ Merkle leaves
// Leaf digests of an n-leaf launch: hash_or_noop of every leaf of the source, bit-exact in every form.
// CHUNK: leaf hashing in column chunks (pipelined host ingest, core.hip zkm_batch_build): the sponge absorbs eight columns per
// permutation in column order, so a chunk of columns [c0, c0 + nc) -- c0 a multiple of 8 -- can be absorbed as soon as its LDE
// exists, with the 12-word sponge state of every row parked in HBM between chunks.  first: the state starts at zero; last: the digest
// is written instead of the state.  Same permutation sequence as the whole matrix at once, so digests are identical.
template <class Form, class Src, bool CHUNK = false>
__device__ __forceinline__ void merkle_leaves_body(Src src, size_t n, gl_t* __restrict__ digests, size_t dig_seg, gl_t* __restrict__ state = nullptr,
                                                   int first = 1, int last = 1) {
    Form f;
    if (!f.take(n)) return;
    src.seek(f.item);
    digests += (size_t)blockIdx.z * dig_seg;
    typename Form::state_t s;
    if constexpr (CHUNK) {
        if (first) f.clear(s);
        else f.load_state(s, state, n);
    } else {
        f.clear(s);
    }
    const auto nw = src.words();
    // hash_or_noop: a leaf of <= 4 words is copied, not hashed (the latency forms are only launched for leaves that are hashed; a
    // chunk is part of a longer leaf)
    constexpr bool NOOP = Form::LANES == 1 && !CHUNK && !Src::WHOLE;
    if (NOOP && nw <= 4) {
        if constexpr (NOOP) f.copy(s, src);               // (only the one-lane form has copy(): the inner test keeps it from being asked of the others)
    } else {
        // What the next step needs of a permutation's result: another whole chunk replaces words 0..7 and only the capacity words are carried
        // over; before a ragged chunk (it keeps words rem..7) the whole state is needed, at the end the digest -- or, where the state is
        // parked between chunks, the whole, canonical state: the last permutation of such a launch keeps all twelve words.
        // Whole-matrix kernels: ONE copy of the round code, the ragged last chunk goes through the same call site.  (Round 5's 126-register
        // layer needed a second, multiply-add copy for it; at 93 registers it does not, and two copies buy nothing: 39.25 against 39.33 ms,
        // measured.)
        decltype(src.words()) c = 0;
        for (; CHUNK ? c + 8 <= nw : c < nw; c += 8) {
            // (only the one-lane form has a path of its own for a whole chunk: eight loads that do not look at the count -- uniform)
            if (Src::WHOLE || CHUNK || (Form::LANES == 1 && nw - c >= 8)) f.template load<false>(s, src, c, nw);
            else f.template load<true>(s, src, c, nw);
            f.permute(s, c + 16 <= nw ? POSEIDON_OUT_CAPACITY : ((Src::WHOLE || c + 8 >= nw) && !CHUNK ? POSEIDON_OUT_DIGEST : POSEIDON_OUT_ALL));
        }
        // CHUNK: the ragged chunk (only legal in the last launch of a row) has a permutation of its own, a second copy of the round code on
        // the multiply-add form.  The single call site of the whole-matrix kernels has not been timed on the staged path, so the chunk
        // kernels keep this shape.
        if constexpr (CHUNK) {
            if (c < nw) {
                f.template load<true>(s, src, c, nw);
                sponge_lane_valu().permute(s, POSEIDON_OUT_ALL);
            }
        }
    }
    if constexpr (CHUNK) {
        if (!last) {
            f.store_state(s, state, n);
            return;
        }
    }
    f.store_digest(s, digests, f.item, f.live);
}

#define ZKM_LEAF_MFMA_ATTR __attribute__((amdgpu_waves_per_eu(ZKM_LEAF_MFMA_WAVES, ZKM_LEAF_MFMA_WAVES)))
// The vector-ALU one-lane kernels: five waves per SIMD (<= 96 registers) for the leaves, six (<= 80) for the tree levels.  Without the
// bound the register allocator, once a kernel does not fit 80, lets it grow past 96 (four waves).
#define ZKM_LANE_WAVES_ATTR(n) __attribute__((amdgpu_waves_per_eu(n, n)))

__global__ __launch_bounds__(256) ZKM_LANE_WAVES_ATTR(5) void k_merkle_leaves(const gl_t* __restrict__ lde, size_t nrows, size_t ncols, size_t col_stride,
                                                       gl_t* __restrict__ digests, size_t lde_seg, size_t dig_seg) {
    merkle_leaves_body<sponge_lane_valu>(leaf_cols{lde, ncols, col_stride, lde_seg}, nrows, digests, dig_seg);
}
__global__ __launch_bounds__(256) ZKM_LEAF_MFMA_ATTR void k_merkle_leaves_mfma(const gl_t* __restrict__ lde, size_t nrows, size_t ncols, size_t col_stride,
                                                                              gl_t* __restrict__ digests, size_t lde_seg, size_t dig_seg) {
    merkle_leaves_body<sponge_lane_mfma>(leaf_cols{lde, ncols, col_stride, lde_seg}, nrows, digests, dig_seg);
}
// (a quad of lanes per leaf: launches of at most zkm_ctx::quad_max_hashes leaves, merkle_pick_form)
__global__ __launch_bounds__(256) void k_merkle_leaves_quad(const gl_t* __restrict__ lde, size_t nrows, size_t ncols, size_t col_stride,
                                                            gl_t* __restrict__ digests, size_t lde_seg, size_t dig_seg) {
    ZKM_RAISE_PRIO();
    merkle_leaves_body<sponge_quad>(leaf_cols{lde, ncols, col_stride, lde_seg}, nrows, digests, dig_seg);
}
// (a 16-lane row per leaf: launches of at most zkm_ctx::wide_max_hashes leaves, merkle_pick_form)
__global__ __launch_bounds__(256) void k_merkle_leaves_wide(const gl_t* __restrict__ lde, size_t nrows, size_t ncols, size_t col_stride,
                                                            gl_t* __restrict__ digests, size_t lde_seg, size_t dig_seg) {
    ZKM_RAISE_PRIO();
    merkle_leaves_body<sponge_wide>(leaf_cols{lde, ncols, col_stride, lde_seg}, nrows, digests, dig_seg);
}

__global__ __launch_bounds__(256) void k_merkle_leaves_chunk(const gl_t* __restrict__ lde, size_t nrows, size_t nc, size_t col_stride,
                                                             gl_t* __restrict__ state, int first, int last, gl_t* __restrict__ digests) {
    merkle_leaves_body<sponge_lane_valu, leaf_cols, true>(leaf_cols{lde, nc, col_stride, 0}, nrows, digests, 0, state, first, last);
}
__global__ __launch_bounds__(256) ZKM_LEAF_MFMA_ATTR void k_merkle_leaves_chunk_mfma(const gl_t* __restrict__ lde, size_t nrows, size_t nc, size_t col_stride,
                                                                                    gl_t* __restrict__ state, int first, int last, gl_t* __restrict__ digests) {
    merkle_leaves_body<sponge_lane_mfma, leaf_cols, true>(leaf_cols{lde, nc, col_stride, 0}, nrows, digests, 0, state, first, last);
}

__global__ __launch_bounds__(256) ZKM_LANE_WAVES_ATTR(5) void k_merkle_leaves_ext(const gl_t* __restrict__ c0, const gl_t* __restrict__ c1,
                                                           size_t nleaves, unsigned arity, gl_t* __restrict__ digests, size_t val_seg, size_t dig_seg) {
    merkle_leaves_body<sponge_lane_valu>(leaf_f2{c0, c1, arity, val_seg}, nleaves, digests, dig_seg);
}
__global__ __launch_bounds__(256) ZKM_LEAF_MFMA_ATTR void k_merkle_leaves_ext_mfma(const gl_t* __restrict__ c0, const gl_t* __restrict__ c1, size_t nleaves,
                                                                                  unsigned arity, gl_t* __restrict__ digests, size_t val_seg, size_t dig_seg) {
    merkle_leaves_body<sponge_lane_mfma>(leaf_f2{c0, c1, arity, val_seg}, nleaves, digests, dig_seg);
}
__global__ __launch_bounds__(256) void k_merkle_leaves_ext_quad(const gl_t* __restrict__ c0, const gl_t* __restrict__ c1, size_t nleaves,
                                                                unsigned arity, gl_t* __restrict__ digests, size_t val_seg, size_t dig_seg) {
    ZKM_RAISE_PRIO();
    merkle_leaves_body<sponge_quad>(leaf_f2{c0, c1, arity, val_seg}, nleaves, digests, dig_seg);
}
__global__ __launch_bounds__(256) void k_merkle_leaves_ext_wide(const gl_t* __restrict__ c0, const gl_t* __restrict__ c1, size_t nleaves,
                                                                unsigned arity, gl_t* __restrict__ digests, size_t val_seg, size_t dig_seg) {
    ZKM_RAISE_PRIO();
    merkle_leaves_body<sponge_wide>(leaf_f2{c0, c1, arity, val_seg}, nleaves, digests, dig_seg);
}

// The form of the permutation for a launch of `hashes` hashes (the segments of a stacked batch fill the machine together):
//   wide: the smallest launches -- 16 lanes per hash, the lowest latency per step of a chain of dependent permutations;
//   quad: short, wide matrices (Keccak: 2431 columns x a few thousand rows), small FRI layers, the levels near the top of a tree: one
//         lane per hash leaves the machine empty and pays one permutation's full latency per step; four lanes per hash cut that latency
//         to a third and fill 4x the lanes;
//   lane / lane_mfma: one lane per hash, the throughput form; mfma_ok: the launch has a matrix-core kernel (zkm_ctx::leaf_mfma decides).
// wide_max_hashes = quad_max_hashes = 0: one lane per hash always.
// wide_max_hashes = 1024.  One absorb step takes ~13 us in the 16-lane form while every SIMD holds at most one such wave (4096 hashes),
// ~21 us with two (8192), ~41 us with four (16384); the four-lane form takes over there.  Up to 4096 the 16-lane form is the fastest for a
// context alone, but it spends 4.2x the issue slots of the one-lane form, and with four or more contexts on the GPU those slots are
// somebody else's work (2^16-cycle segments, 1 / 4 / 8 contexts: 24.5 / 52.5 / 51.8 segments/s at 4096, 25.5 / 56.9 / 59.0 at 1024 --
// profiles/r03_hw_queues.txt).
// quad_max_hashes = 32768.  One absorb step takes ~16 us in the quad form while a SIMD holds at most one such wave (16384 hashes = 1024
// waves; ~21 us with two, 32768), against ~39 us for the one-lane form on a wave that has its SIMD to itself; it costs 1.45x the
// instructions per hash since its partial rounds are fused (poseidon_lat_dev.h).
enum merkle_form { MERKLE_LANE, MERKLE_LANE_MFMA, MERKLE_QUAD, MERKLE_WIDE };
static merkle_form merkle_pick_form(const zkm_ctx* c, size_t hashes, bool mfma_ok) {
    if (hashes <= c->wide_max_hashes) return MERKLE_WIDE;
    if (hashes <= c->quad_max_hashes) return MERKLE_QUAD;
    return mfma_ok && c->leaf_mfma ? MERKLE_LANE_MFMA : MERKLE_LANE;
}
// grid of a leaf launch in form f: 256-thread workgroups, one z-slice per segment
static dim3 leaf_grid(merkle_form f, size_t n, size_t nseg = 1) {
    static const unsigned lanes[] = {1, 1, 4, 16};
    return dim3((unsigned)((n * lanes[f] + 255) / 256), 1, (unsigned)nseg);
}

void zkm_launch_merkle_leaves(zkm_ctx* c, const gl_t* lde, size_t nrows, size_t ncols, size_t col_stride, gl_t* digests, size_t nseg,
                              size_t lde_seg, size_t dig_seg) {
    // rows of <= 4 elements are copied, not hashed (hash_or_noop): profile them under their own name
    zkm_prof_scope ps(c, ncols <= 4 ? "merkle_leaves_copy" : "merkle_leaves");
    if (nseg == 0 || nseg > 65535) throw std::runtime_error("merkle_leaves: bad segment count");
    static constexpr decltype(&k_merkle_leaves) kernel[] = {k_merkle_leaves, k_merkle_leaves_mfma, k_merkle_leaves_quad, k_merkle_leaves_wide};   // by merkle_form
    const merkle_form f = ncols > 4 ? merkle_pick_form(c, nrows * nseg, true) : MERKLE_LANE;
    hipLaunchKernelGGL(kernel[f], leaf_grid(f, nrows, nseg), dim3(256), 0, c->stream, lde, nrows, ncols, col_stride, digests, lde_seg, dig_seg);
    ZKM_HIP_CHECK(hipGetLastError());
}

void zkm_launch_merkle_leaves_chunk(zkm_ctx* c, const gl_t* lde, size_t nrows, size_t nc, size_t col_stride, gl_t* state, bool first,
                                    bool last, gl_t* digests) {
    if (!last && nc % 8) throw std::runtime_error("merkle_leaves_chunk: only the last chunk may hold a ragged group of columns");
    zkm_prof_scope ps(c, "merkle_leaves");
    hipLaunchKernelGGL(c->leaf_mfma ? k_merkle_leaves_chunk_mfma : k_merkle_leaves_chunk, leaf_grid(MERKLE_LANE, nrows), dim3(256), 0, c->stream, lde, nrows,
                       nc, col_stride, state, first ? 1 : 0, last ? 1 : 0, digests);
    ZKM_HIP_CHECK(hipGetLastError());
}

void zkm_launch_merkle_leaves_ext(zkm_ctx* c, const gl_t* c0, const gl_t* c1, size_t nleaves, unsigned arity, gl_t* digests, size_t nseg,
                                  size_t val_seg, size_t dig_seg) {
    if (arity % 4 || 2 * arity <= 4) throw std::runtime_error("merkle_leaves_ext: unsupported arity");
    if (nseg == 0 || nseg > 65535) throw std::runtime_error("merkle_leaves_ext: bad segment count");
    zkm_prof_scope ps(c, "merkle_leaves_ext");
    // (the leaf kernel's matrix-core layer here: layer 0 of a 2^22-row FRI proof 1.70 -> 1.62 ms)
    static constexpr decltype(&k_merkle_leaves_ext) kernel[] = {k_merkle_leaves_ext, k_merkle_leaves_ext_mfma, k_merkle_leaves_ext_quad, k_merkle_leaves_ext_wide};   // by merkle_form
    const merkle_form f = merkle_pick_form(c, nleaves * nseg, true);
    hipLaunchKernelGGL(kernel[f], leaf_grid(f, nleaves, nseg), dim3(256), 0, c->stream, c0, c1, nleaves, arity, digests, val_seg, dig_seg);
    ZKM_HIP_CHECK(hipGetLastError());
}

// ------------------------------------------------------------------ Merkle inner levels, fused (K5)
// plonky2 builds a tree in one call (MerkleTree::new, call sites prover.rs:154-163); here a launch takes up to THREE levels.
// Large levels (first level of the launch >= 2^15 parents): one hash per lane.  A workgroup of 256 threads owns 512 children of
// level l and produces their 256 parents, then -- from LDS, no trip through HBM -- the 128 and the 64 nodes above (whole waves
// stay active: 4, 2, 1, and the waves that are done leave at once).  Every level is also stored (Merkle paths read all of them).  The permutation code exists once (the level
// loop is not unrolled), so the kernel stays within the instruction cache like k_merkle_leaves.
struct merkle_fused_args {
    const gl_t* children;   // level l: 2 * nparents digests
    gl_t* parents[3];       // levels l + 1 .. l + 3
    uint32_t levels;        // 1 .. 3
    size_t dig_seg;         // blockIdx.z-th tree: every pointer + blockIdx.z * dig_seg
};

__global__ __launch_bounds__(256) ZKM_LANE_WAVES_ATTR(6) void k_merkle_fused(merkle_fused_args p) {
    __shared__ uint64_t sh[2][4][256];                    // [buffer][word][node]: parents of the level just made, word-major
    const unsigned tid = threadIdx.x;
    uint64_t s[12];
    {
        const ulonglong2* ch = reinterpret_cast<const ulonglong2*>(p.children + (size_t)blockIdx.z * p.dig_seg + 8 * ((size_t)blockIdx.x * 256 + tid));
        ulonglong2 a = ch[0], b = ch[1], cc = ch[2], d = ch[3];
        s[0] = a.x; s[1] = a.y; s[2] = b.x; s[3] = b.y; s[4] = cc.x; s[5] = cc.y; s[6] = d.x; s[7] = d.y;
    }
#pragma unroll 1
    for (unsigned lvl = 0; lvl < p.levels; lvl++) {
        const unsigned width = 256u >> lvl;               // nodes of this level in the workgroup: 256, 128, 64 == the surviving threads
        if (lvl) {
#pragma unroll
            for (int w = 0; w < 4; w++) {
                s[w] = sh[(lvl - 1) & 1][w][2 * tid];
                s[4 + w] = sh[(lvl - 1) & 1][w][2 * tid + 1];
            }
        }
#pragma unroll
        for (int w = 8; w < 12; w++) s[w] = 0;
        poseidon_permute_out(s, POSEIDON_OUT_DIGEST);
        uint64_t* o = p.parents[lvl] + (size_t)blockIdx.z * p.dig_seg + 4 * ((size_t)blockIdx.x * width + tid);
        *reinterpret_cast<ulonglong2*>(o) = make_ulonglong2(s[0], s[1]);
        *reinterpret_cast<ulonglong2*>(o + 2) = make_ulonglong2(s[2], s[3]);
        if (lvl + 1 < p.levels) {
#pragma unroll
            for (int w = 0; w < 4; w++) sh[lvl & 1][w][tid] = s[w];
        }
        if (lvl + 1 == p.levels) return;
        __syncthreads();
        // Waves without a node in the next level leave NOW and free their slots for the next workgroup (s_barrier only waits for the
        // surviving waves of a workgroup): parked at the barriers they would hold a third of the CU's wave slots idle, and this
        // kernel needs every slot it can get (one permutation per lane is ~12k dependent-ish instructions).
        if (tid >= (width >> 1)) return;
    }
}

// Small levels: a workgroup owns a subtree with 2^J children and climbs its J levels through LDS instead of one launch per level: the
// top of a tree is a chain of dependent permutations (one wide permutation ~10 us), and every launch boundary added its gap to it.
// The np parents of ONE level of the subtree from their children in LDS (`in`, AoS as in HBM), in ceil(np / slots) rounds of the form's
// permutations -- slots = threads / LANES hash slots per workgroup, 64 / LANES of them per wave.  A parent goes to LDS (`out`) for the
// level above, to HBM (`g`: Merkle paths read every level) and, where the caller has one, to a third place (`also`).  The caller puts
// the workgroup barrier between levels.
// false: this wave has no node at this level, so none above either -- a kernel with nothing else to do lets it leave (the barrier only
// counts survivors).
template <class Form>
__device__ __forceinline__ bool merkle_climb_level(const Form& f, unsigned slots, unsigned np, const uint64_t* in, uint64_t* out, gl_t* g, uint64_t* also = nullptr) {
    const unsigned slot = threadIdx.x / Form::LANES, wave_slot0 = (threadIdx.x >> 6) * (64 / Form::LANES);
    if (wave_slot0 >= np) return false;
    for (unsigned h0 = 0; h0 < np; h0 += slots) {
        if (h0 + wave_slot0 >= np) continue;              // (a wave with no live slot in this round skips it -- uniform over the wave)
        const unsigned h = h0 + slot;
        const bool on = h < np;                           // uniform over the hash's lanes; every lane of a working wave permutes
        typename Form::state_t s;
        f.compress(s, in, h, on);
        f.store_digest(s, out, h, on);
        f.store_digest(s, g, h, on);
        if (also) f.store_digest(s, also, h, on);
    }
    return true;
}

// 16 lanes per hash: 256 threads = 16 hash slots, J <= 6 -- ceil(2^(J-k) / 16) rounds of wide permutations at level k.
struct merkle_fused_wide_args {
    const gl_t* children;   // level l: nsub * 2^J digests
    gl_t* parents[6];       // levels l + 1 .. l + J
    uint32_t J;             // levels in this launch (1 .. 6)
    size_t dig_seg;
};
// four lanes per hash: 256 threads = 64 hash slots, J <= 7 -- ceil(2^(J-k-1) / 64) rounds of quad permutations at level k.
struct merkle_fused_quad_args {
    const gl_t* children;   // level l: nsub * 2^J digests
    gl_t* parents[7];       // levels l + 1 .. l + J
    uint32_t J;             // levels in this launch (1 .. 7)
    size_t dig_seg;
};
template <class Form, unsigned MAXC, class Args>
__device__ __forceinline__ void merkle_fused_body(const Args& p) {
    __shared__ uint64_t sh[2][MAXC * 4];                  // digests of the current level of this subtree (AoS, as in HBM)
    const unsigned tid = threadIdx.x;
    Form f;
    const unsigned C = 1u << p.J;
    const size_t seg_off = (size_t)blockIdx.z * p.dig_seg;
    {
        const gl_t* src = p.children + seg_off + (size_t)blockIdx.x * C * 4;
        for (unsigned w = tid; w < C * 4; w += 256) sh[0][w] = src[w];
    }
    __syncthreads();
    for (unsigned lvl = 0; lvl < p.J; lvl++) {
        const unsigned np = C >> (lvl + 1);               // parents of this level in the subtree
        if (!merkle_climb_level(f, 256 / Form::LANES, np, sh[lvl & 1], sh[(lvl + 1) & 1], p.parents[lvl] + seg_off + (size_t)blockIdx.x * np * 4))
            return;                                       // this wave has no node here or above: leave
        __syncthreads();
    }
}
__global__ __launch_bounds__(256) void k_merkle_fused_wide(merkle_fused_wide_args p) {
    ZKM_RAISE_PRIO();
    merkle_fused_body<sponge_wide, 64>(p);
}
__global__ __launch_bounds__(256) void k_merkle_fused_quad(merkle_fused_quad_args p) {
    ZKM_RAISE_PRIO();
    merkle_fused_body<sponge_quad, 128>(p);
}

// ---- a whole small tree in ONE launch, cap delivered to the host by the same launch (VERDICT r03 missing #4)
// Trees of up to 2^15 leaves (every commitment of a table of <= 2^13 rows, every FRI layer below that) used to be 2-3 launches for the
// levels plus the download kernel for the cap.  Here a workgroup owns the subtree under ONE cap entry (2^J leaf digests, J = log2(leaves)
// - cap_height <= 11), climbs its J levels through LDS -- the quad form of the permutation while a level has more parents than
// `wide_np_max`, the 16-lane form below -- stores every level (Merkle paths read them) and writes its cap entry to pinned host memory as
// well; the last workgroup to finish publishes the sequence number the host is polling (zkm_ctx::wait_flag).
struct merkle_tail_args {
    const gl_t* children;   // level 0: gridDim.x * 2^J digests
    gl_t* parents[11];      // levels 1 .. J
    uint32_t J, wide_np_max;
    uint64_t* host_cap;     // pinned: gridDim.z x gridDim.x digests
    uint64_t* flag;
    uint64_t seq;
    unsigned* counter;      // device word, zero between launches
    size_t dig_seg;         // blockIdx.z-th tree
};
__global__ __launch_bounds__(256) void k_merkle_tail(merkle_tail_args p) {
    ZKM_RAISE_PRIO();
    extern __shared__ __attribute__((aligned(16))) uint64_t tail_lds[];
    const unsigned tid = threadIdx.x, C = 1u << p.J;
    uint64_t* const buf0 = tail_lds;             // C digests
    uint64_t* const buf1 = tail_lds + 4 * C;     // C / 2 digests
    const size_t seg_off = (size_t)blockIdx.z * p.dig_seg;
    uint64_t* const host_cap = p.host_cap + 4 * ((size_t)blockIdx.z * gridDim.x + blockIdx.x);
    {
        const gl_t* src = p.children + seg_off + (size_t)blockIdx.x * C * 4;
        for (unsigned w = tid; w < C * 4; w += blockDim.x) buf0[w] = src[w];
    }
    __syncthreads();
    sponge_quad fq;
    sponge_wide fw;
    for (unsigned lvl = 0; lvl < p.J; lvl++) {
        const unsigned np = C >> (lvl + 1);
        const uint64_t* in = (lvl & 1) ? buf1 : buf0;
        uint64_t* out = (lvl & 1) ? buf0 : buf1;
        gl_t* g = p.parents[lvl] + seg_off + (size_t)blockIdx.x * np * 4;
        uint64_t* const also = np == 1 ? host_cap : nullptr;      // the top of the subtree is this workgroup's cap entry
        // (every wave stays to the end: the ticket below follows a barrier of the whole workgroup)
        if (np > p.wide_np_max) merkle_climb_level(fq, blockDim.x >> 2, np, in, out, g, also);
        else merkle_climb_level(fw, blockDim.x >> 4, np, in, out, g, also);
        __syncthreads();
    }
    // every workgroup's cap words are in host memory before its ticket is; the holder of the last ticket publishes
    __threadfence_system();
    __syncthreads();
    if (tid == 0) {
        const unsigned ticket = atomicAdd(p.counter, 1u);
        if (ticket == gridDim.x * gridDim.z - 1) {
            *p.counter = 0;
            __threadfence_system();
            __hip_atomic_store(p.flag, p.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}
// true: the levels above the leaves were built and the cap is in cap_out (host); false: not a tree this kernel takes
// (l0: the level the kernel starts from -- its "leaves" are the 2^(log_leaves - l0) nodes of level l0)
bool zkm_merkle_tail(zkm_ctx* c, gl_t* digests, const std::vector<size_t>& level_off, unsigned log_leaves, unsigned cap_height, uint64_t* cap_out,
                     unsigned l0, size_t nseg, size_t dig_seg) {
    const unsigned J = log_leaves - l0 - cap_height;
    if (!c->tree_tail || J == 0 || J > 11 || cap_height > 6) return false;
    // (a first level the tuning gives to the one-lane form stays with the level kernels)
    if (merkle_pick_form(c, (size_t)1 << (log_leaves - l0 - 1), false) == MERKLE_LANE) return false;
    // LDS: two level buffers of C and C / 2 digests (6 KB at the usual J = 7, 96 KB at J = 11) next to the static table of the quad form.
    // Only a launch beyond the default 64 KB needs the raised limit; a part that cannot grant it keeps the level kernels.
    const size_t tail_lds = (((size_t)1 << J) * 4 + ((size_t)1 << J) * 2) * sizeof(uint64_t);
    // (this kernel's fixed maximum is 128 KB: the largest tail, J = 11, next to the static table)
    static std::atomic<uint64_t> lds_ok{0};
    if (tail_lds + ZKM_QUAD_TAB_WORDS * sizeof(uint32_t) > 64 * 1024 &&
        zkm_allow_big_lds(c, (const void*)k_merkle_tail, lds_ok, 128 * 1024) != hipSuccess)
        return false;
    merkle_tail_args a{};
    a.children = digests + level_off[l0];
    for (unsigned k = 0; k < J; k++) a.parents[k] = digests + level_off[l0 + 1 + k];
    a.J = J;
    a.dig_seg = dig_seg;
    a.wide_np_max = c->wide_max_hashes ? 16 : 0;                      // 16 lanes per hash where a level is ONE round of them (16 slots per
                                                                      // 256 threads: 15.6 us against 24 us for a round of quads)
    const size_t capw = ((size_t)4 << cap_height) * nseg;
    const uint64_t seq = c->xfer_begin(capw * 8, &a.host_cap, &a.flag, &a.counter);
    a.seq = seq;
    const size_t C = (size_t)1 << J;
    unsigned threads = (unsigned)(C >> 1) * 4;                        // a quad per parent of the first level, one wave per SIMD at most
    if (threads > 256) threads = 256;
    if (threads < 64) threads = 64;
    {
        zkm_prof_scope ps(c, "merkle_compress");
        hipLaunchKernelGGL(k_merkle_tail, dim3(1u << cap_height, 1, (unsigned)nseg), dim3(threads), tail_lds, c->stream, a);
        ZKM_HIP_CHECK(hipGetLastError());
    }
    c->xfer_finish(seq, cap_out, capw * 8);
    return true;
}

size_t zkm_merkle_layout(unsigned log_leaves, unsigned cap_height, std::vector<size_t>& level_off) {
    if (cap_height > log_leaves) throw std::runtime_error("cap_height exceeds tree height");
    level_off.clear();
    size_t total = 0;
    for (unsigned l = 0; l + cap_height <= log_leaves; l++) {
        level_off.push_back(total);
        total += ((size_t)1 << (log_leaves - l)) * 4;
    }
    return total;
}

// All digest levels above the leaves, up to the cap: fused launches (k_merkle_fused: <= 3 levels, one hash per lane, while the first
// level of the launch has >= 2^15 nodes; k_merkle_fused_quad: four lanes per hash, the two levels with 2^14 and 2^13 parents;
// k_merkle_fused_wide: <= 6 levels, 16 lanes per hash, from 2^12 parents on).  A 2^22-leaf tree with a
// 16-digest cap (18 levels) is 3 + 2 launches instead of 18.  (Measured and dropped, profiles/r03_merkle_inner_levels.txt: a lane
// reducing a 16-node subtree by itself -- no barrier, 15 back-to-back permutations -- leaves 4096 waves for a 2^22-leaf tree, four per
// SIMD, and the permutation needs five to saturate the issue port: 2.65 G permutations/s against 2.7 here and 3.33 in the leaf kernel.)
// The four-lane form takes ~40 % of the latency of a permutation at 1.7x its issue slots (330 instead of 190 wave instructions per
// hash), so it is kept to the levels where a launch is mostly latency.
void zkm_merkle_build_inner(zkm_ctx* c, gl_t* digests, const std::vector<size_t>& level_off, unsigned log_leaves,
                            unsigned cap_height, size_t nseg, size_t dig_seg) {
    const unsigned top = log_leaves - cap_height;
    const unsigned z = (unsigned)nseg;
    unsigned l = 0;                                        // level of the children of the next launch
    while (l < top) {
        zkm_prof_scope ps(c, "merkle_compress");
        const unsigned log_p1 = log_leaves - l - 1;       // log2(#parents) of the first level made
        const unsigned rem = top - l;
        const size_t p1 = (size_t)1 << log_p1, h1 = p1 * nseg;   // (h1: hashes of the launch's first level over all stacked trees)
        merkle_form form = merkle_pick_form(c, h1, false);   // (no matrix core here: see below)
        if (form == MERKLE_LANE && log_p1 < 8) form = MERKLE_QUAD;   // (the one-lane kernel works on blocks of 256 parents)
        if (form == MERKLE_LANE) {
            merkle_fused_args a{};
            a.dig_seg = dig_seg;
            a.children = digests + level_off[l];
            a.levels = rem < 3 ? rem : 3;
            for (unsigned k = 0; k < a.levels; k++) a.parents[k] = digests + level_off[l + 1 + k];
            // (the matrix-core layer was measured here too, rounds 5 and 6: the 24 KB it parks in LDS next to this kernel's 16 KB leave four
            // workgroups per CU -- merkle_compress 1.59 -> 1.72 ms per 262 x 2^20 commitment, lock-step segments 108 -> 106/s: not adopted)
            hipLaunchKernelGGL(k_merkle_fused, dim3((unsigned)(((size_t)1 << log_p1) / 256), 1, z), dim3(256), 0, c->stream, a);
            l += a.levels;
        } else if (form == MERKLE_WIDE) {
            merkle_fused_wide_args a{};
            a.dig_seg = dig_seg;
            a.children = digests + level_off[l];
            unsigned J = rem < 6 ? rem : 6;
            if (J > log_p1 + 1) J = log_p1 + 1;           // (a subtree cannot have more children than the level)
            a.J = J;
            for (unsigned k = 0; k < J; k++) a.parents[k] = digests + level_off[l + 1 + k];
            hipLaunchKernelGGL(k_merkle_fused_wide, dim3((unsigned)(((size_t)2 << log_p1) >> J), 1, z), dim3(256), 0, c->stream, a);
            l += J;
        } else {
            merkle_fused_quad_args a{};
            a.dig_seg = dig_seg;
            a.children = digests + level_off[l];
            unsigned J = 1;                                  // the levels that are still too large for the 16-lane form (default: 2^14 and 2^13 parents)
            while (J < rem && J < 7 && J <= log_p1 && merkle_pick_form(c, h1 >> J, false) != MERKLE_WIDE) J++;
            a.J = J;
            for (unsigned k = 0; k < J; k++) a.parents[k] = digests + level_off[l + 1 + k];
            hipLaunchKernelGGL(k_merkle_fused_quad, dim3((unsigned)(((size_t)2 << log_p1) >> J), 1, z), dim3(256), 0, c->stream, a);
            l += J;
        }
        ZKM_HIP_CHECK(hipGetLastError());
    }
}

// caps of nseg stacked trees from their cap levels: one download (segment s: 4 << cap_height words at digests + s * dig_seg + level_off[top])
static void download_caps(zkm_ctx* c, const gl_t* digests, size_t cap_off, unsigned cap_height, uint64_t* cap_out, size_t nseg, size_t dig_seg) {
    const size_t capw = (size_t)4 << cap_height;
    if (nseg == 1) {
        c->download(cap_out, digests + cap_off, capw * sizeof(uint64_t));
        return;
    }
    zkm_scratch tmp(c, nseg * capw * sizeof(gl_t));
    ZKM_HIP_CHECK(hipMemcpy2DAsync(tmp.p, capw * sizeof(gl_t), digests + cap_off, dig_seg * sizeof(gl_t), capw * sizeof(gl_t), nseg,
                                   hipMemcpyDeviceToDevice, c->stream));
    c->download(cap_out, tmp.p, nseg * capw * sizeof(uint64_t));
}

void zkm_merkle_build_inner_cap(zkm_ctx* c, gl_t* digests, const std::vector<size_t>& level_off, unsigned log_leaves, unsigned cap_height,
                                uint64_t* cap_out, size_t nseg, size_t dig_seg) {
    // A workgroup of the tail kernel owns everything under one cap entry, and a chain of permutations is fastest with ONE wave per SIMD
    // (tools/ubench_perm_latency.hip: 24 us per quad permutation alone, 46 us with four waves per SIMD): 256 threads, 64 quads per
    // round.  From 2^11 nodes on a level is one round; with more to start from the first levels took several rounds on 16 CUs while
    // the rest of the GPU watched (measured with 2^13 / 2^15: +1.5-2 ms per 2^16-cycle segment).  Larger trees climb to 2^11 nodes with
    // the level kernels first (many workgroups, one round per level).
    const unsigned TAIL_LOG = 11;
    if (c->tree_tail && log_leaves <= 24 && log_leaves >= cap_height + 1) {
        const unsigned l0 = log_leaves > TAIL_LOG ? log_leaves - TAIL_LOG : 0;
        if (log_leaves - l0 > cap_height) {
            if (l0) zkm_merkle_build_inner(c, digests, level_off, log_leaves, log_leaves - l0, nseg, dig_seg);    // levels 1 .. l0 ("cap" = level l0)
            if (zkm_merkle_tail(c, digests, level_off, log_leaves, cap_height, cap_out, l0, nseg, dig_seg)) return;
            // (refused: finish with the level kernels from where we are -- build_inner starts at level 0, so only without a head start)
            if (l0) {
                std::vector<size_t> rest(level_off.begin() + l0, level_off.end());
                zkm_merkle_build_inner(c, digests, rest, log_leaves - l0, cap_height, nseg, dig_seg);
                download_caps(c, digests, level_off[log_leaves - cap_height], cap_height, cap_out, nseg, dig_seg);
                return;
            }
        }
    }
    zkm_merkle_build_inner(c, digests, level_off, log_leaves, cap_height, nseg, dig_seg);
    download_caps(c, digests, level_off[log_leaves - cap_height], cap_height, cap_out, nseg, dig_seg);
}

// ------------------------------------------------------------------ Keccak-f[1600] batch (K15)
// States are 25-word records (AoS: the layout of the reference's [u64; 25], cpu/kernel/keccak_util.rs:6-31), one state per lane:
// ~6.3k VALU instructions per permutation (xor, v_alignbit_b32 rotations, v_bfi chi) for 400 B moved.  Each lane moves its own record
// with 16-byte accesses (records are 8-byte aligned: 200 = 8 * 25); a wave's 64 records are 12.8 KB of contiguous memory, so every
// cache line comes from HBM once and the partial-line accesses are served by L1 / L2.  Measured on 2^22 states
// (profiles/r03_keccakf_variants.txt): 8 B accesses + generic 64-bit rotates 0.96 ms (r02); this form 0.82 ms = 5.1 G permutations/s;
// the records staged and transposed through LDS with fully coalesced 512 B accesses 0.91 ms (one 12.8 KB image per wave: three
// waves per SIMD) and 1.01 ms (two 6.4 KB halves: four waves, twice the LDS instructions) -- the transposition costs more than
// the uncoalesced 16 B accesses do.
struct __attribute__((aligned(8))) keccak_pair { uint64_t x, y; };

__global__ __launch_bounds__(256) void k_keccakf(uint64_t* __restrict__ states, size_t k) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= k) return;
    uint64_t a[25];
    uint64_t* st = states + idx * 25;
#pragma unroll
    for (int i = 0; i < 12; i++) {
        const keccak_pair v = *reinterpret_cast<const keccak_pair*>(st + 2 * i);
        a[2 * i] = v.x;
        a[2 * i + 1] = v.y;
    }
    a[24] = st[24];
    keccakf_dev(a);
#pragma unroll
    for (int i = 0; i < 12; i++) *reinterpret_cast<keccak_pair*>(st + 2 * i) = keccak_pair{a[2 * i], a[2 * i + 1]};
    st[24] = a[24];
}

void zkm_launch_keccakf(zkm_ctx* c, uint64_t* states, size_t k) {
    if (!k) return;
    zkm_prof_scope ps(c, "keccakf");
    hipLaunchKernelGGL(k_keccakf, dim3((k + 255) / 256), dim3(256), 0, c->stream, states, k);
    ZKM_HIP_CHECK(hipGetLastError());
}

// ------------------------------------------------------------------ Poseidon self test (parity / debug)
// zkm_poseidon_selftest: one piece of the device permutation per launch, on words the caller chooses -- the four forms of the whole
// permutation, a single linear layer or fused group of each form, the two folds, the s-box and the first constant add.  Leaf hashing
// only ever feeds these the LDE of field data, which never holds a state of all-ones halves or of extreme byte planes and a word >= p
// once in 2^32; the range claims in the comments of poseidon_dev.h / poseidon_mfma_dev.h / gl_dev.h are about exactly those inputs.
// Every kernel calls the product's code (the sponge forms above and the routines of the three Poseidon headers) and stores raw words:
// nothing is canonicalised here.  One item per hash slot of the form, 256 threads per workgroup; a lane past the last item works on
// the last item's data and only its store is masked (MFMA ignores EXEC, the latency forms shuffle).
enum {
    PROBE_PERMUTE_LANE = ZKM_POSEIDON_PROBE_PERMUTE_LANE, PROBE_PERMUTE_LANE_MFMA = ZKM_POSEIDON_PROBE_PERMUTE_LANE_MFMA,
    PROBE_PERMUTE_QUAD = ZKM_POSEIDON_PROBE_PERMUTE_QUAD, PROBE_PERMUTE_WIDE = ZKM_POSEIDON_PROBE_PERMUTE_WIDE,
    PROBE_MDS_VALU = ZKM_POSEIDON_PROBE_MDS_VALU, PROBE_MDS_MFMA = ZKM_POSEIDON_PROBE_MDS_MFMA, PROBE_MDS_QUAD = ZKM_POSEIDON_PROBE_MDS_QUAD,
    PROBE_MDS_ROWS = ZKM_POSEIDON_PROBE_MDS_ROWS, PROBE_GROUP3 = ZKM_POSEIDON_PROBE_GROUP3, PROBE_GROUP3_QUAD = ZKM_POSEIDON_PROBE_GROUP3_QUAD,
    PROBE_GROUP2 = ZKM_POSEIDON_PROBE_GROUP2, PROBE_FOLD = ZKM_POSEIDON_PROBE_FOLD, PROBE_FOLD_TY = ZKM_POSEIDON_PROBE_FOLD_TY,
    PROBE_SBOX7 = ZKM_POSEIDON_PROBE_SBOX7, PROBE_SBOX_DELTA = ZKM_POSEIDON_PROBE_SBOX_DELTA, PROBE_ADD_RC0 = ZKM_POSEIDON_PROBE_ADD_RC0,
    PROBE_GROUP4 = ZKM_POSEIDON_PROBE_GROUP4, PROBE_FOLD_WIDE = ZKM_POSEIDON_PROBE_FOLD_WIDE
};
static_assert(POSEIDON_OUT_ALL == ZKM_POSEIDON_OUT_ALL && POSEIDON_OUT_CAPACITY == ZKM_POSEIDON_OUT_CAPACITY && POSEIDON_OUT_DIGEST == ZKM_POSEIDON_OUT_DIGEST,
              "include/zkm_hip.h names the output modes of poseidon_dev.h");

// one lane per hash: the whole permutation, a full-round layer, the 4-row last layers, the fused groups (arg: wave-uniform)
template <class Form, int PROBE>
__device__ __forceinline__ void poseidon_probe_lane_body(const uint64_t* __restrict__ in, size_t n, uint64_t* __restrict__ out, unsigned arg) {
    Form f;
    if (!f.take(n)) return;
    typename Form::state_t s;
#pragma unroll
    for (int i = 0; i < 12; i++) s[i] = in[f.item * 12 + i];
    if constexpr (PROBE == PROBE_PERMUTE_LANE || PROBE == PROBE_PERMUTE_LANE_MFMA) {
        f.permute(s, (int)arg);
    } else if constexpr (PROBE == PROBE_MDS_VALU || PROBE == PROBE_MDS_MFMA) {
        f.mds.layer(s, (int)arg);
    } else if constexpr (PROBE == PROBE_MDS_ROWS) {
        if (arg == 0) poseidon_mds_add<false, 0, 4>(s, nullptr);
        else poseidon_mds_add<false, 8, 12>(s, nullptr);
    } else if constexpr (PROBE == PROBE_GROUP3) {
        poseidon_partial_group<3>(s, PC::ZKM_POSEIDON_FUSED_C1[arg], PC::ZKM_POSEIDON_FUSED_C2[arg], PC::ZKM_POSEIDON_FUSED_C3[arg]);
    } else if constexpr (PROBE == PROBE_GROUP4) {
        poseidon_partial_group4(s, PC::ZKM_POSEIDON_G4_C1[arg], PC::ZKM_POSEIDON_G4_C2[arg], &PC::ZKM_POSEIDON_G4_C3[arg], PC::ZKM_POSEIDON_G4_C4[arg]);
    } else {
        static_assert(PROBE == PROBE_GROUP2, "not a one-lane probe");
        poseidon_partial_group<2>(s, PC::ZKM_POSEIDON_FUSED_C1[7], 0, PC::ZKM_POSEIDON_FUSED_C3[7]);
    }
    if (!f.live) return;
#pragma unroll
    for (int i = 0; i < 12; i++) out[f.item * 12 + i] = s[i];
}
template <int PROBE>
__global__ __launch_bounds__(256) void k_poseidon_probe_lane(const uint64_t* __restrict__ in, size_t n, uint64_t* __restrict__ out, unsigned arg) {
    poseidon_probe_lane_body<sponge_lane_valu, PROBE>(in, n, out, arg);
}
template <int PROBE>
__global__ __launch_bounds__(256) ZKM_LEAF_MFMA_ATTR void k_poseidon_probe_lane_mfma(const uint64_t* __restrict__ in, size_t n, uint64_t* __restrict__ out, unsigned arg) {
    poseidon_probe_lane_body<sponge_lane_mfma, PROBE>(in, n, out, arg);
}

// a quad of lanes per hash: lane q holds the words q, q + 4, q + 8 of its state
template <int PROBE>
__global__ __launch_bounds__(256) void k_poseidon_probe_quad(const uint64_t* __restrict__ in, size_t n, uint64_t* __restrict__ out, unsigned arg) {
    sponge_quad f;
    f.take(n);
    const size_t item = f.live ? f.item : n - 1;
    sponge_quad::state_t s;
#pragma unroll
    for (int a = 0; a < 3; a++) s[a] = in[item * 12 + f.q + 4 * a];
    if constexpr (PROBE == PROBE_PERMUTE_QUAD) {
        f.permute(s, (int)arg);
    } else if constexpr (PROBE == PROBE_MDS_QUAD) {
        quad_mds(s, f.Q, arg < 30 ? PC::ZKM_POSEIDON_RC + arg * 12 + f.q : nullptr);
    } else {
        static_assert(PROBE == PROBE_GROUP3_QUAD, "not a quad probe");
        quad_group3(s, f.Q, PC::ZKM_POSEIDON_FUSED_C1[arg], PC::ZKM_POSEIDON_FUSED_C2[arg], PC::ZKM_POSEIDON_FUSED_C3[arg] + f.q);
    }
    if (!f.live) return;
#pragma unroll
    for (int a = 0; a < 3; a++) out[item * 12 + f.q + 4 * a] = s[a];
}

// a 16-lane row per hash: lanes 0..11 of the row hold the twelve words
__global__ __launch_bounds__(256) void k_poseidon_probe_wide(const uint64_t* __restrict__ in, size_t n, uint64_t* __restrict__ out, unsigned arg) {
    sponge_wide f;
    f.take(n);
    const size_t item = f.live ? f.item : n - 1;
    sponge_wide::state_t s;
    s[0] = f.idx < 12 ? in[item * 12 + f.idx] : 0;
    f.permute(s, (int)arg);
    if (f.live && f.idx < 12) out[item * 12 + f.idx] = s[0];
}

// word-wise probes: n pairs -> n words (the folds; the wide fold: n triples), n states -> n states (s-box, s-box delta, the first constant add)
template <int PROBE>
__global__ __launch_bounds__(256) void k_poseidon_probe_words(const uint64_t* __restrict__ in, size_t n, uint64_t* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if constexpr (PROBE == PROBE_FOLD) {
        out[i] = poseidon_fold(in[2 * i], in[2 * i + 1]);
    } else if constexpr (PROBE == PROBE_FOLD_WIDE) {
        // the carries reach the fold the way a row's last multiply-adds deliver them: as the wave's lane masks
        const uint64_t carries = in[3 * i + 2];
#if defined(__HIP_DEVICE_COMPILE__)
        const uint64_t cl = __ballot((int)(carries & 1)), ch = __ballot((int)((carries >> 1) & 1));
#else
        const uint64_t cl = carries & 1, ch = (carries >> 1) & 1;
#endif
        out[i] = poseidon_fold_wide(in[3 * i], in[3 * i + 1], cl, ch);
    } else if constexpr (PROBE == PROBE_FOLD_TY) {
#if defined(__HIP_DEVICE_COMPILE__)      // (the matrix-core layer's fold has no host form)
        out[i] = poseidon_fold_ty(in[2 * i], (uint32_t)in[2 * i + 1]);
#endif
    } else {
        const uint64_t* rc0 = PC::ZKM_POSEIDON_RC;
#pragma unroll
        for (int w = 0; w < 12; w++) {
            const uint64_t x = in[i * 12 + w];
            out[i * 12 + w] = PROBE == PROBE_SBOX7 ? poseidon_sbox7(x) : PROBE == PROBE_SBOX_DELTA ? poseidon_sbox_delta(x) : gl_add_lc(x, rc0[w]);
        }
    }
}

extern "C" int zkm_poseidon_selftest(zkm_ctx* c, uint32_t probe, uint32_t arg, const uint64_t* in, size_t n, uint64_t* out, char** err) {
    return zkm_api("zkm_poseidon_selftest", c, err, [&] {
        typedef void (*probe_kernel)(const uint64_t*, size_t, uint64_t*, unsigned);
        probe_kernel kernel = nullptr;
        unsigned lanes = 1;               // lanes per item
        bool arg_ok = arg == 0;
        const bool is_out = arg == POSEIDON_OUT_ALL || arg == POSEIDON_OUT_CAPACITY || arg == POSEIDON_OUT_DIGEST;
        const bool is_next = arg == 1 || arg == 2 || arg == 3 || arg == 27 || arg == 28 || arg == 29 || arg == 30;   // the values the permutation uses
        switch (probe) {
            case PROBE_PERMUTE_LANE: kernel = k_poseidon_probe_lane<PROBE_PERMUTE_LANE>; arg_ok = is_out; break;
            case PROBE_PERMUTE_LANE_MFMA: kernel = k_poseidon_probe_lane_mfma<PROBE_PERMUTE_LANE_MFMA>; arg_ok = is_out; break;
            case PROBE_PERMUTE_QUAD: kernel = k_poseidon_probe_quad<PROBE_PERMUTE_QUAD>; arg_ok = is_out; lanes = 4; break;
            case PROBE_PERMUTE_WIDE: kernel = k_poseidon_probe_wide; arg_ok = is_out; lanes = 16; break;
            case PROBE_MDS_VALU: kernel = k_poseidon_probe_lane<PROBE_MDS_VALU>; arg_ok = is_next; break;
            case PROBE_MDS_MFMA: kernel = k_poseidon_probe_lane_mfma<PROBE_MDS_MFMA>; arg_ok = is_next; break;
            case PROBE_MDS_QUAD: kernel = k_poseidon_probe_quad<PROBE_MDS_QUAD>; arg_ok = is_next; lanes = 4; break;
            case PROBE_MDS_ROWS: kernel = k_poseidon_probe_lane<PROBE_MDS_ROWS>; arg_ok = arg <= 1; break;
            case PROBE_GROUP3: kernel = k_poseidon_probe_lane<PROBE_GROUP3>; arg_ok = arg < 7; break;
            case PROBE_GROUP3_QUAD: kernel = k_poseidon_probe_quad<PROBE_GROUP3_QUAD>; arg_ok = arg < 7; lanes = 4; break;
            case PROBE_GROUP2: kernel = k_poseidon_probe_lane<PROBE_GROUP2>; break;
            case PROBE_GROUP4: kernel = k_poseidon_probe_lane<PROBE_GROUP4>; arg_ok = arg < 5; break;
            case PROBE_FOLD_WIDE: case PROBE_FOLD: case PROBE_FOLD_TY: case PROBE_SBOX7: case PROBE_SBOX_DELTA: case PROBE_ADD_RC0: break;
            default: throw std::runtime_error("zkm_poseidon_selftest: unknown probe");
        }
        if (!arg_ok) throw std::runtime_error("zkm_poseidon_selftest: bad arg for this probe");
        if (!in || !out) throw std::runtime_error("zkm_poseidon_selftest: null argument");
        if (n == 0 || n > ((size_t)1 << 20)) throw std::runtime_error("zkm_poseidon_selftest: n must be 1 .. 2^20");
        const bool pairs = probe == PROBE_FOLD || probe == PROBE_FOLD_TY, triples = probe == PROBE_FOLD_WIDE;
        const size_t in_words = triples ? 3 * n : pairs ? 2 * n : 12 * n, out_words = pairs || triples ? n : 12 * n;
        zkm_scratch din(c, in_words * 8), dout(c, out_words * 8);
        ZKM_HIP_CHECK(hipMemcpyAsync(din.p, in, in_words * 8, hipMemcpyHostToDevice, c->stream));
        // (rows / words a probe leaves unspecified read as zero, not as what the block held before)
        ZKM_HIP_CHECK(hipMemsetAsync(dout.p, 0, out_words * 8, c->stream));
        const dim3 grid((unsigned)((n * lanes + 255) / 256)), block(256);
        if (kernel) {
            hipLaunchKernelGGL(kernel, grid, block, 0, c->stream, din.as<uint64_t>(), n, dout.as<uint64_t>(), arg);
        } else {
            void (*words)(const uint64_t*, size_t, uint64_t*) =
                probe == PROBE_FOLD ? k_poseidon_probe_words<PROBE_FOLD> : probe == PROBE_FOLD_TY ? k_poseidon_probe_words<PROBE_FOLD_TY> :
                probe == PROBE_FOLD_WIDE ? k_poseidon_probe_words<PROBE_FOLD_WIDE> :
                probe == PROBE_SBOX7 ? k_poseidon_probe_words<PROBE_SBOX7> : probe == PROBE_SBOX_DELTA ? k_poseidon_probe_words<PROBE_SBOX_DELTA> :
                                                                                                        k_poseidon_probe_words<PROBE_ADD_RC0>;
            hipLaunchKernelGGL(words, grid, block, 0, c->stream, din.as<uint64_t>(), n, dout.as<uint64_t>());
        }
        ZKM_HIP_CHECK(hipGetLastError());
        ZKM_HIP_CHECK(hipMemcpyAsync(out, dout.p, out_words * 8, hipMemcpyDeviceToHost, c->stream));
        c->sync();
    });
}
