// bootstrap.hip -- a segment's bootstrap-kernel witness built on the device from its memory image (the reference's
// generate_bootstrap_kernel, prover/src/cpu/bootstrap_kernel.rs:26-306, with poseidon_sponge_log, witness/util.rs:370-469).
//
// Everything the bootstrap pushes into Traces is a function of the image (addr, value pairs in BTreeMap order), the root, the image id
// and the entry pc.  With R = ceil(nwords / 8) and P page-aligned addresses, in push order:
//   CPU rows         [0, R) image rows, R + c the sponge row of page c, R + P and R + P + 1 the image-id writes, R + P + 2 its sponge row
//   memory ops       [0, nwords) the image writes, nwords + 4096 c + k read k of page c, then 9 writes, 32 reads and 4 reads of the image id
//   Poseidon inputs  129 c + b block b of page c, then the two blocks of the image id (the PoseidonSponge rows have the same index)
// A "chain" is one sponge: chain c < P hashes page c (129 dependent permutations), chain P the image id (2).
//
// Phases (zkm_internal.h zkm_boot_job; segment_ops.hip drives them for the K segments of a wave, zkm_boot_witness for one image):
//   early   k_boot_count, k_boot_image, k_boot_gather, k_boot_reads: the order and alignment checks, the page list, every memory
//           operation, the page words (absent words 0).  Nothing here depends on a permutation: Memory can be sized behind it.
//   chain   k_boot_chain: all chains of all segments in ONE launch, a permutation across 16 lanes (or a quad) each; writes the state
//           before each permutation straight into the Poseidon input list, the state after it for the sponge rows, and the digests.
//   late    k_boot_rows (one thread per chain and block: timestamps, PoseidonSponge rows, the digest checks) and k_boot_cpu (one thread
//           per cell of the boot's CPU rows).
// The descriptors of the segments live in device memory (blockIdx.z picks one): they are too large for the kernel arguments.
#include "poseidon_lat_dev.h"
#include "zkm_internal.h"

namespace {

constexpr uint32_t HASH_BASE = 0x80000000u, ROOT_PAGE = 0x81020000u, ID_BASE = 0x81021000u;
constexpr unsigned PAGE_BLOCKS = 129, ID_BLOCKS = 2, CPU_W = ZKM_CPU_COLS;
constexpr unsigned COL_SPONGE = 82, COL_HASH = 86, COL_CLOCK = 204, COL_CH0 = 205;

__device__ __forceinline__ uint32_t bswap32_dev(uint32_t v) { return __builtin_bswap32(v); }
__device__ __forceinline__ void put_op(uint64_t* o, uint32_t virt, uint64_t ts, bool read, uint32_t value) {
    o[0] = 0; o[1] = 0; o[2] = virt; o[3] = ts; o[4] = read; o[5] = value;
}
// the smallest offending address wins, whatever the order the threads arrive in (the word starts at 0)
__device__ __forceinline__ void flag_addr(unsigned long long* w, uint32_t addr) {
    atomicMax(w, ((unsigned long long)1 << 32) | (0xFFFFFFFFu - addr));
}

// page-aligned addresses of each 256-word piece of the image
__global__ __launch_bounds__(256) void k_boot_count(const zkm_boot_seg* S) {
    const zkm_boot_seg& A = S[blockIdx.z];
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if ((size_t)blockIdx.x * 256 >= A.nwords) return;
    const int n = __syncthreads_count(i < A.nwords && (A.addrs[i] & 0xFFF) == 0);
    if (threadIdx.x == 0) A.blk_count[blockIdx.x] = (uint32_t)n;
}

// one thread per image word, then nine for the image-id words: the checks, the page list, the write operations
__global__ __launch_bounds__(256) void k_boot_image(const zkm_boot_seg* S) {
    __shared__ uint32_t part[256], wave_n[4];
    const zkm_boot_seg& A = S[blockIdx.z];
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, nw = A.nwords;
    if ((size_t)blockIdx.x * 256 >= nw + 9) return;
    // pages before this workgroup's piece
    uint32_t before = 0;
    for (size_t b = threadIdx.x; b < blockIdx.x && b * 256 < nw; b += 256) before += A.blk_count[b];
    part[threadIdx.x] = before;
    __syncthreads();
    for (unsigned s = 128; s; s >>= 1) {
        if (threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
        __syncthreads();
    }
    before = part[0];
    const uint32_t a = i < nw ? A.addrs[i] : 0;
    const bool page = i < nw && (a & 0xFFF) == 0;
    const unsigned long long m = __ballot(page);
    const unsigned lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) wave_n[wv] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t rank = before + (uint32_t)__popcll(m & (((unsigned long long)1 << lane) - 1));
    for (unsigned w = 0; w < wv; w++) rank += wave_n[w];
    if (i < nw) {
        if ((a & 3) || (i > 0 && A.addrs[i - 1] >= a)) flag_addr(A.flags + 0, a);
        if (page && rank < A.npages) { A.page_addr[rank] = a; A.page_idx[rank] = (uint32_t)i; }
        if (i == nw - 1 && rank + page != A.npages) A.flags[1] = ((unsigned long long)1 << 32) | (rank + page);
        put_op(A.mem + i * 6, a, (i / 8) * 10, false, bswap32_dev(A.values[i]));
    } else if (i < nw + 9) {
        const size_t j = i - nw;
        put_op(A.mem + (nw + (size_t)4096 * A.npages + j) * 6, ID_BASE + 4 * (uint32_t)j, (A.rows_image + A.npages + j / 8) * 10, false,
               bswap32_dev(A.id_words[j]));
    }
}

// the 1024 words of each page (zero-filled before: an absent word reads as 0) and the nine of the image id.
// Where the caller's npages is larger than the image's page count, k_boot_image never wrote page_addr / page_idx of the pages past
// the real ones: this kernel and k_boot_reads then work on whatever the allocator left there.  That is meant (the call is refused
// at the first wait, nothing built here is used) and bounded: j < nwords, d < 4096 and c < npages keep every access inside addrs,
// values and pagew, and mem is sized from the same claimed npages.
__global__ __launch_bounds__(256) void k_boot_gather(const zkm_boot_seg* S) {
    const zkm_boot_seg& A = S[blockIdx.z];
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t c = t >> 10, k = t & 1023;
    if (c < A.npages) {
        const size_t j = (size_t)A.page_idx[c] + k;
        if (j >= A.nwords) return;
        const uint32_t d = A.addrs[j] - A.page_addr[c];
        if (d < 4096) A.pagew[c * 1024 + d / 4] = A.values[j];
    } else if (c == A.npages && k < 9) {
        A.pagew[c * 1024 + k] = A.id_words[k];
    }
}

// one thread per byte read: 4096 a page, then 36 of the image id
__global__ __launch_bounds__(256) void k_boot_reads(const zkm_boot_seg* S) {
    const zkm_boot_seg& A = S[blockIdx.z];
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x, P = A.npages;
    if (t >= 4096 * P + 36) return;
    const size_t c = t >> 12, k = c < P ? (t & 4095) : t - 4096 * P;
    const uint32_t base = c < P ? A.page_addr[c] : ID_BASE;
    const uint64_t clock = c < P ? A.rows_image + c : A.rows_image + P + 2;
    const size_t at = c < P ? A.nwords + t : A.nwords + 4096 * P + 9 + k;
    put_op(A.mem + at * 6, base + 4 * (uint32_t)(k / 4), clock * 10, true, bswap32_dev(A.pagew[c * 1024 + k / 4]));
}

// rate word i (< 8) of block b of a message of `nbytes` bytes (a multiple of 4) whose words are w: pad10*1 in the last block
__device__ __forceinline__ uint32_t rate_word(const uint32_t* __restrict__ w, unsigned nbytes, unsigned b, unsigned i) {
    const unsigned wi = 8 * b + i, nw = nbytes / 4;
    uint32_t v = wi < nw ? w[wi] : 0;
    if (wi == nw) v = 1;
    if (b == nbytes / 32 && i == 7) v |= 0x80000000u;
    return v;
}

// FORM 0: a chain owns a 16-lane row of the wave (lanes 0..11 = the state words), four chains a wave.  FORM 1: a chain owns a quad of
// lanes (lane q holds words q, q + 4, q + 8), sixteen chains a wave.  The next block's words are loaded before the permutation.
template <int FORM>
__global__ __launch_bounds__(64) void k_boot_chain(const zkm_boot_seg* S) {
    constexpr unsigned PER = FORM == 0 ? 4 : 16, LANES = 64 / PER;
    __shared__ __attribute__((aligned(16))) uint32_t quad_tab[FORM == 1 ? ZKM_QUAD_TAB_WORDS : 4];
    const zkm_boot_seg& A = S[blockIdx.z];
    const unsigned P = A.npages, nch = P + 1, c0 = PER * blockIdx.x;
    if (c0 >= nch) return;
    const unsigned lane = threadIdx.x, idx = lane % LANES;
    const unsigned ch = min(c0 + lane / LANES, nch - 1);
    const bool mine = c0 + lane / LANES < nch, page = ch < P;
    const unsigned nblk = page ? PAGE_BLOCKS : ID_BLOCKS, nbytes = page ? 4096 : 36;
    const unsigned loop = c0 < P ? PAGE_BLOCKS : ID_BLOCKS;          // (wave-uniform: the longest chain of this wave)
    const uint32_t* __restrict__ w = A.pagew + (size_t)ch * 1024;
    const size_t pos = (size_t)PAGE_BLOCKS * (page ? ch : P);
    uint64_t* __restrict__ in = A.po_in + pos * 12;
    uint64_t* __restrict__ post = A.post + pos * 12;
    if constexpr (FORM == 0) {
        const bool store = mine && idx < 12;
        uint64_t x = 0, nxt = idx < 8 ? rate_word(w, nbytes, 0, idx) : 0;
#pragma unroll 1
        for (unsigned b = 0; b < loop; b++) {
            const bool on = b < nblk;
            if (idx < 8 && on) x = nxt;
            if (store && on) in[b * 12 + idx] = x;
            if (idx < 8 && b + 1 < nblk) nxt = rate_word(w, nbytes, b + 1, idx);
            const uint64_t y = poseidon_permute_wide(x, lane);
            if (on) x = y;
            if (store && on) post[b * 12 + idx] = x;
        }
        if (store && idx < 4) A.digests[(size_t)ch * 4 + idx] = x;
    } else {
        quad_tab_load(quad_tab);
        const poseidon_quad Q(lane, quad_tab);
        uint64_t s[3] = {0, 0, 0}, n0 = rate_word(w, nbytes, 0, idx), n1 = rate_word(w, nbytes, 0, idx + 4);
#pragma unroll 1
        for (unsigned b = 0; b < loop; b++) {
            const bool on = b < nblk;
            if (on) { s[0] = n0; s[1] = n1; }
            if (mine && on)
#pragma unroll
                for (int a = 0; a < 3; a++) in[b * 12 + idx + 4 * a] = s[a];
            if (b + 1 < nblk) { n0 = rate_word(w, nbytes, b + 1, idx); n1 = rate_word(w, nbytes, b + 1, idx + 4); }
            uint64_t y[3] = {s[0], s[1], s[2]};
            poseidon_permute_quad(y, Q);
            if (on) { s[0] = y[0]; s[1] = y[1]; s[2] = y[2]; }
            if (mine && on)
#pragma unroll
                for (int a = 0; a < 3; a++) post[b * 12 + idx + 4 * a] = s[a];
        }
        if (mine) A.digests[(size_t)ch * 4 + idx] = s[0];
    }
}

// index of `addr` in the ascending addresses, or nwords
__device__ __forceinline__ size_t find_addr(const uint32_t* __restrict__ addrs, size_t nwords, uint32_t addr) {
    size_t lo = 0, hi = nwords;
    while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2;
        if (addrs[mid] < addr) lo = mid + 1;
        else hi = mid;
    }
    return lo < nwords && addrs[lo] == addr ? lo : nwords;
}

// one thread per (chain, block): the Poseidon timestamp, the PoseidonSponge row (PoseidonSpongeStark::generate_trace,
// poseidon_sponge_stark.rs:186-381; column map as k_poseidon_sponge_trace, with virt = base + 4 w); the thread of a chain's last block
// compares the digest with its expected words (check_memory_page_hash / check_image_id)
__global__ __launch_bounds__(256) void k_boot_rows(const zkm_boot_seg* S) {
    const zkm_boot_seg& A = S[blockIdx.z];
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x, P = A.npages;
    const size_t c = t / PAGE_BLOCKS;
    const unsigned b = (unsigned)(t - c * PAGE_BLOCKS);
    if (c > P || (c == P && b >= ID_BLOCKS)) return;
    const bool page = c < P;
    const unsigned nblk = page ? PAGE_BLOCKS : ID_BLOCKS, nbytes = page ? 4096 : 36, nw = nbytes / 4;
    const uint32_t base = page ? A.page_addr[c] : ID_BASE;
    const uint64_t ts = (page ? A.rows_image + c : A.rows_image + P + 2) * 10;
    const size_t pos = PAGE_BLOCKS * (page ? c : P) + b;
    A.po_ts[pos] = ts;
    const uint64_t* __restrict__ in = A.po_in + pos * 12;
    const uint64_t* __restrict__ post = A.post + pos * 12;
    if (A.ps) {
        gl_t* o = A.ps + pos * A.ps_rs;
        const size_t cs = A.ps_cs;
        const unsigned rem = nbytes - 32 * b < 32 ? nbytes - 32 * b : 32;    // bytes of the message in this block
        o[0] = rem == 32;
        o[1 * cs] = 0;
        o[2 * cs] = 0;
#pragma unroll
        for (unsigned i = 0; i < 8; i++) o[(3 + i) * cs] = 8 * b + i < nw ? base + 4 * (8 * b + i) : 0;
        o[11 * cs] = ts;
        o[12 * cs] = nbytes;
        o[13 * cs] = 32 * b;
#pragma unroll 8
        for (unsigned k = 0; k < 32; k++) o[(14 + k) * cs] = rem < 32 && k == rem;
#pragma unroll
        for (unsigned i = 0; i < 12; i++) o[(46 + i) * cs] = b ? post[(ptrdiff_t)i - 12] : 0;
#pragma unroll
        for (unsigned i = 0; i < 8; i++) {
            const uint32_t v = (uint32_t)in[i];
#pragma unroll
            for (unsigned j = 0; j < 4; j++) o[(58 + 4 * i + j) * cs] = (v >> (8 * j)) & 0xFF;
            o[(90 + i) * cs] = v;
        }
#pragma unroll
        for (unsigned i = 0; i < 8; i++) o[(98 + i) * cs] = post[4 + i];
#pragma unroll
        for (unsigned i = 0; i < 4; i++) o[(106 + i) * cs] = post[i];
    }
    if (b != nblk - 1) return;
    uint32_t want[8];
    bool have = true;
    if (!page || base == ROOT_PAGE) {
#pragma unroll
        for (int i = 0; i < 8; i++) want[i] = page ? A.want_root[i] : A.want_id[i];
    } else {
        const uint32_t h = HASH_BASE + ((base >> 12) << 5);
        for (int i = 0; i < 8; i++) {
            const size_t j = find_addr(A.addrs, A.nwords, h + 4 * i);
            if (j == A.nwords) { flag_addr(A.flags + 2, h + 4 * i); have = false; want[i] = 0; }
            else want[i] = A.values[j];
        }
    }
    if (!A.check || !have) return;
    bool same = true;
#pragma unroll
    for (int i = 0; i < 4; i++) same = same && (uint32_t)post[i] == want[2 * i] && (uint32_t)(post[i] >> 32) == want[2 * i + 1];
    if (!same) flag_addr(A.flags + 3, base);
}

// one thread per cell of the boot's CPU rows, consecutive threads down a column: CpuColumnsView::default() with clock and
// is_bootstrap_kernel, the channel cells of the write rows, is_poseidon_sponge / channel values / general.hash.value of the sponge rows
__global__ __launch_bounds__(256) void k_boot_cpu(const zkm_boot_seg* S) {
    const zkm_boot_seg& A = S[blockIdx.z];
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x, R = A.rows_image, P = A.npages, nboot = R + P + 3;
    if (t >= nboot * CPU_W) return;
    const unsigned col = (unsigned)(t / nboot);
    const size_t r = t - (size_t)col * nboot;
    const bool id_row = r >= R + P && r < R + P + 2, sponge = r >= R && !id_row;
    uint64_t v = 0;
    if (col == 0) v = 1;
    else if (col == COL_CLOCK) v = r;
    else if (sponge && col == COL_SPONGE) v = 1;
    else if (sponge && col >= COL_HASH && col < COL_HASH + 4) v = A.digests[(r < R + P ? r - R : P) * 4 + (col - COL_HASH)];
    else if (col >= COL_CH0 && col < COL_CH0 + 48) {
        const unsigned k = (col - COL_CH0) / 6, f = (col - COL_CH0) % 6;
        if (sponge) {
            if (f == 5 && k == 2) v = r < R + P ? 0 : ID_BASE + 32;
            if (f == 5 && k == 3) v = r < R + P ? 4096 : 36;
        } else {
            const size_t i = id_row ? 8 * (r - R - P) + k : 8 * r + k;
            if (i < (id_row ? 9 : A.nwords)) {
                if (f == 0) v = 1;
                if (f == 4) v = id_row ? ID_BASE + 4 * (uint32_t)i : A.addrs[i];
                if (f == 5) v = bswap32_dev(id_row ? A.id_words[i] : A.values[i]);
            }
        }
    }
    A.cpu[r * A.cpu_rs + (size_t)col * A.cpu_cs] = v;
}

size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

template <class K> void launch(hipStream_t st, K kernel, size_t threads, unsigned block, size_t nseg, const zkm_boot_seg* d) {
    if (!threads) return;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((threads + block - 1) / block), 1, (unsigned)nseg), dim3(block), 0, st, d);
    ZKM_HIP_CHECK(hipGetLastError());
}

}  // namespace

void zkm_boot_sizes(const zkm_boot_image* im, zkm_boot_counts_t* n) {
    n->rows_image = (im->nwords + 7) / 8;
    n->cpu_rows = n->rows_image + im->npages + 3;
    n->memory_ops = im->nwords + 4096 * im->npages + 45;
    n->poseidon = PAGE_BLOCKS * im->npages + 2;
    n->sponge_ops = im->npages + 1;
}

zkm_boot_job::zkm_boot_job(zkm_ctx* ctx, const zkm_boot_image* image) : c(ctx), im(image) {
    if (!im) return;
    zkm_boot_sizes(im, &n);
    if (im->nwords >= ((size_t)1 << 31)) throw std::runtime_error("the image holds 2^31 words or more");
    if (im->npages > im->nwords) throw std::runtime_error("npages = " + std::to_string(im->npages) + ": more pages than words");
    if (im->nwords && (!im->addrs || !im->values)) throw std::runtime_error("null pointer with a nonzero count");
}

// a job's scratch block: the states after each permutation, the digests, the page words, the page list, and the image where it lies in
// host memory
struct boot_layout {
    bool host, host_v;
    size_t o_post, o_dig, o_pagew, o_cnt, o_pa, o_pi, o_a, o_v, bytes = 0;
    explicit boot_layout(const zkm_boot_image* im) {
        zkm_boot_counts_t n;
        zkm_boot_sizes(im, &n);
        const size_t nw = im->nwords, P = im->npages, nb = (nw + 255) / 256;
        host = nw && !zkm_is_device_ptr(im->addrs);
        host_v = nw && !zkm_is_device_ptr(im->values);
        auto take = [&](size_t b) { const size_t o = bytes; bytes += up256(b); return o; };
        o_post = take(n.poseidon * 96); o_dig = take((P + 1) * 32); o_pagew = take((P + 1) * 4096); o_cnt = take(nb * 4 + 4);
        o_pa = take(P * 4 + 4); o_pi = take(P * 4 + 4); o_a = take(host ? nw * 4 : 0); o_v = take(host_v ? nw * 4 : 0);
    }
};
size_t zkm_boot_scratch_bytes(const zkm_boot_image* im) { return im ? boot_layout(im).bytes : 0; }

// the scratch block (and the image, where it lies in host memory) and the descriptor without its outputs
void zkm_boot_job::prepare() {
    const boot_layout L(im);
    const size_t nw = im->nwords, P = im->npages, o_post = L.o_post, o_dig = L.o_dig, o_pagew = L.o_pagew, o_cnt = L.o_cnt, o_pa = L.o_pa,
                 o_pi = L.o_pi, o_a = L.o_a, o_v = L.o_v;
    const bool host = L.host, host_v = L.host_v;
    scratch = zkm_scratch(c, L.bytes);
    char* sb = scratch.as<char>();
    d = zkm_boot_seg{};
    d.addrs = host ? (const uint32_t*)(sb + o_a) : im->addrs;
    d.values = host_v ? (const uint32_t*)(sb + o_v) : im->values;
    if (host) ZKM_HIP_CHECK(hipMemcpyAsync(sb + o_a, im->addrs, nw * 4, hipMemcpyHostToDevice, c->stream));
    if (host_v) ZKM_HIP_CHECK(hipMemcpyAsync(sb + o_v, im->values, nw * 4, hipMemcpyHostToDevice, c->stream));
    ZKM_HIP_CHECK(hipMemsetAsync(sb + o_pagew, 0, (P + 1) * 4096, c->stream));
    d.nwords = (uint32_t)nw;
    d.npages = (uint32_t)P;
    d.rows_image = (uint32_t)n.rows_image;
    d.check = im->check;
    for (int i = 0; i < 8; i++) {
        const uint8_t *r = im->pre_hash_root + 4 * i, *q = im->pre_image_id + 4 * i;
        d.id_words[i] = (uint32_t)r[0] << 24 | (uint32_t)r[1] << 16 | (uint32_t)r[2] << 8 | r[3];      // u32::from_be_bytes
        d.want_root[i] = (uint32_t)r[3] << 24 | (uint32_t)r[2] << 16 | (uint32_t)r[1] << 8 | r[0];
        d.want_id[i] = (uint32_t)q[3] << 24 | (uint32_t)q[2] << 16 | (uint32_t)q[1] << 8 | q[0];
    }
    d.id_words[8] = im->entry;
    d.post = (uint64_t*)(sb + o_post);
    d.digests = (uint64_t*)(sb + o_dig);
    d.pagew = (uint32_t*)(sb + o_pagew);
    d.blk_count = (uint32_t*)(sb + o_cnt);
    d.page_addr = (uint32_t*)(sb + o_pa);
    d.page_idx = (uint32_t*)(sb + o_pi);
}

// the jobs with an image among `j`, their descriptors uploaded to `d_desc` (room for nseg): returns how many
static size_t boot_put(zkm_ctx* c, zkm_boot_job* j, size_t nseg, zkm_boot_seg* d_desc, size_t* max_words, size_t* max_pages) {
    std::vector<zkm_boot_seg> h;
    *max_words = *max_pages = 0;
    for (size_t s = 0; s < nseg; s++) {
        if (!j[s].im) continue;
        h.push_back(j[s].d);
        *max_words = std::max<size_t>(*max_words, j[s].d.nwords);
        *max_pages = std::max<size_t>(*max_pages, j[s].d.npages);
    }
    if (!h.empty()) c->upload(d_desc, h.data(), h.size() * sizeof(zkm_boot_seg));
    return h.size();
}

void zkm_boot_early(zkm_ctx* c, zkm_boot_job* j, size_t nseg, zkm_boot_seg* d_desc) {
    size_t nw, P;
    const size_t k = boot_put(c, j, nseg, d_desc, &nw, &P);
    if (!k) return;
    zkm_prof_scope ps(c, "bootstrap/image");
    launch(c->stream, k_boot_count, nw, 256, k, d_desc);
    launch(c->stream, k_boot_image, nw + 9, 256, k, d_desc);
    launch(c->stream, k_boot_gather, (P + 1) * 1024, 256, k, d_desc);
    launch(c->stream, k_boot_reads, P * 4096 + 36, 256, k, d_desc);
}

void zkm_boot_chain(zkm_ctx* c, zkm_boot_job* j, size_t nseg, const zkm_boot_seg* d_desc, hipStream_t st) {
    size_t k = 0, P = 0;
    for (size_t s = 0; s < nseg; s++)
        if (j[s].im) { k++; P = std::max<size_t>(P, j[s].d.npages); }
    if (!k) return;
    zkm_prof_scope ps(c, c->boot_chain_quad ? "bootstrap/chain_quad" : "bootstrap/chain_row");
    if (c->boot_chain_quad) launch(st, k_boot_chain<1>, (P + 1 + 15) / 16 * 64, 64, k, d_desc);
    else launch(st, k_boot_chain<0>, (P + 1 + 3) / 4 * 64, 64, k, d_desc);
}

void zkm_boot_late(zkm_ctx* c, zkm_boot_job* j, size_t nseg, zkm_boot_seg* d_desc) {
    size_t nw, P;
    const size_t k = boot_put(c, j, nseg, d_desc, &nw, &P);
    if (!k) return;
    zkm_prof_scope ps(c, "bootstrap/rows");
    launch(c->stream, k_boot_rows, (P + 1) * PAGE_BLOCKS, 256, k, d_desc);
    launch(c->stream, k_boot_cpu, ((nw + 7) / 8 + P + 3) * CPU_W, 256, k, d_desc);
}

static std::string hex8(uint64_t flag) {
    char buf[16];
    snprintf(buf, sizeof buf, "0x%08x", 0xFFFFFFFFu - (uint32_t)flag);
    return buf;
}
std::string zkm_boot_refusal_early(const zkm_boot_job& j, const uint64_t flags[4]) {
    if (flags[0]) return "bootstrap image: address " + hex8(flags[0]) + " is not a multiple of 4 above the address before it";
    if (flags[1])
        return "bootstrap image: npages = " + std::to_string(j.im->npages) + ", the image holds " + std::to_string((uint32_t)flags[1]) +
               " page-aligned addresses";
    return "";
}
std::string zkm_boot_refusal_late(const zkm_boot_job&, const uint64_t flags[4]) {
    if (flags[2]) return "bootstrap image: the hash word at address " + hex8(flags[2]) + " is missing";
    if (flags[3]) {
        const uint32_t a = 0xFFFFFFFFu - (uint32_t)flags[3];
        return std::string("bootstrap image: ") + (a == ID_BASE ? "image id" : a == ROOT_PAGE ? "root hash" : "page hash") + " mismatch at address " +
               hex8(flags[3]);
    }
    return "";
}

extern "C" {

void zkm_boot_counts(const zkm_boot_image* im, size_t* cpu_rows, size_t* memory_ops, size_t* poseidon_inputs, size_t* sponge_ops,
                     size_t* sponge_rows) {
    zkm_boot_counts_t n{};
    if (im) zkm_boot_sizes(im, &n);
    if (cpu_rows) *cpu_rows = n.cpu_rows;
    if (memory_ops) *memory_ops = n.memory_ops;
    if (poseidon_inputs) *poseidon_inputs = n.poseidon;
    if (sponge_ops) *sponge_ops = n.sponge_ops;
    if (sponge_rows) *sponge_rows = n.poseidon;
}

int zkm_boot_witness(zkm_ctx* c, const zkm_boot_image* im, uint64_t* cpu_rows_out, uint64_t* memory_ops_out, uint64_t* poseidon_inputs_out,
                     uint64_t* poseidon_ts_out, uint64_t* digests_out, char** err) {
    return zkm_api("zkm_boot_witness", c, err, [&] {
        if (!im || !cpu_rows_out || !memory_ops_out || !poseidon_inputs_out || !poseidon_ts_out || !digests_out)
            throw std::runtime_error("zkm_boot_witness: null argument");
        auto refuse = [](const std::string& m) { throw std::runtime_error("zkm_boot_witness: Cpu: " + m); };
        std::unique_ptr<zkm_boot_job> j;
        try {
            j.reset(new zkm_boot_job(c, im));
        } catch (const std::exception& e) {
            refuse(std::string("bootstrap image: ") + e.what());
        }
        zkm_scratch small(c, 2 * sizeof(zkm_boot_seg) + 256);
        zkm_boot_seg* d_desc = small.as<zkm_boot_seg>();
        unsigned long long* d_flags = (unsigned long long*)(d_desc + 2);
        uint64_t flags[4];
        ZKM_HIP_CHECK(hipMemsetAsync(d_flags, 0, sizeof flags, c->stream));
        j->prepare();
        j->d.flags = d_flags;
        j->d.mem = memory_ops_out;
        j->d.po_in = poseidon_inputs_out;
        j->d.po_ts = poseidon_ts_out;
        j->d.cpu = cpu_rows_out;
        j->d.cpu_rs = CPU_W;
        j->d.cpu_cs = 1;
        zkm_boot_early(c, j.get(), 1, d_desc);
        c->download(flags, d_flags, sizeof flags);
        if (const std::string m = zkm_boot_refusal_early(*j, flags); !m.empty()) refuse(m);
        zkm_boot_chain(c, j.get(), 1, d_desc, c->stream);
        zkm_boot_late(c, j.get(), 1, d_desc + 1);
        ZKM_HIP_CHECK(hipMemcpyAsync(digests_out, j->d.digests, j->n.sponge_ops * 32, hipMemcpyDeviceToDevice, c->stream));
        c->download(flags, d_flags, sizeof flags);
        if (const std::string m = zkm_boot_refusal_late(*j, flags); !m.empty()) refuse(m);
    });
}

}  // extern "C"
