// image_hash.hip -- the hashing the emulator does between two segments, as one device call: Memory::update_page_hash and
// Memory::compute_image_id (emulator/src/memory.rs:388-471, with poseidon / hash_page / CONST_HASH_PAGES / alloc_hash_page, :43-118
// and :378-386; called from split_segment, state.rs:1477-1530).  The outputs are what the bootstrap kernel (bootstrap.hip) checks.
//
// Page q (q = addr >> 12) is hashed into the eight words at 0x80000000 + (q << 5): a dirty page p < 0x80000 into slot p & 127 of the
// L1 page 0x80000 + (p >> 7), an L1 page into slot (p >> 7) & 127 of the L2 page 0x81000 + (p >> 14), an L2 page into slot p >> 14 of
// the root page 0x81020.  The "plan" of a split is the ascending list of hash pages it writes: its L1 pages, its L2 pages, the root.
//
// The page store of a call is one block of the context's allocator: per image the dirty pages (copied there from host memory, or left
// where they lie in device memory), then the plan pages.  Launches, the image in blockIdx.z (descriptors in device memory):
//   init    k_image_init: every word of every plan page -- from `known`, or the constant digest of the page's level (a fresh page of
//           alloc_hash_page is 128 copies of the digest of the level below's fresh page) -- and the registers at byte 0x400 of the root;
//   level   k_image_level, once per level (dirty, L1, L2, root): a chain is one sponge of 129 dependent permutations; it reads its
//           page's words straight from the store, the next block loaded before the permutation, and writes only the eight digest
//           words into its parent's slot (the host has every index: it uploads each chain's slot).  The root's launch writes the root
//           and goes on with the two permutations of the image id.
// Few chains are a latency problem (a chain owns a 16-lane row of a wave, four chains a wave), many a throughput problem (a quad of
// lanes, sixteen a wave): the form is chosen per level from the launch's chain count (zkm_ctx::image_hash_row_max, measured by
// tools/image_hash_time.py; "image_hash_form" forces one).
#include <algorithm>
#include <mutex>

#include "poseidon_lat_dev.h"
#include "zkm_internal.h"

namespace {

constexpr uint32_t MAIN_PAGES = 0x80000u, L1_BASE = 0x80000u, L2_BASE = 0x81000u, ROOT_INDEX = 0x81020u;
constexpr unsigned PAGE_WORDS = 1024, PAGE_BLOCKS = 129, REG_WORD = 0x400 / 4, REG_WORDS = 39;

// one image of a call; np = n1 + n2 + 1 plan pages: the L1 pages, the L2 pages, the root
struct image_desc {
    const uint32_t* dirty;      // nd x 1024
    uint32_t* plan;             // np x 1024
    const uint32_t* known;      // the caller's known pages (device memory), or null
    const int32_t* known_of;    // [np] the position of plan page i among the known pages, or -1
    const uint32_t* slot;       // [nd + n1 + n2] where chain j of levels 0, 1, 2 puts its digest: a word offset into `plan`
    uint32_t* result;           // 16 words: the root, the image id
    uint32_t nd, n1, n2, pc;
    uint32_t regs[REG_WORDS];
};
struct level_consts { uint32_t d[3][8]; };   // the fill of a fresh L1, L2 and root page

__global__ __launch_bounds__(256) void k_image_init(const image_desc* S, level_consts K) {
    const image_desc& A = S[blockIdx.z];
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t np = A.n1 + A.n2 + 1;
    if (t >= (size_t)np * PAGE_WORDS) return;
    const uint32_t page = (uint32_t)(t >> 10), w = (uint32_t)(t & 1023);
    const unsigned level = page < A.n1 ? 0 : page < A.n1 + A.n2 ? 1 : 2;
    const int32_t k = A.known_of[page];
    uint32_t v = k >= 0 ? A.known[(size_t)k * PAGE_WORDS + w] : K.d[level][w & 7];
    if (level == 2 && w >= REG_WORD && w < REG_WORD + REG_WORDS) v = A.regs[w - REG_WORD];
    A.plan[t] = v;
}

// rate word i (< 8) of block b of a 4096-byte page: pad10*1 makes a 129th block {1, 0, .., 0x80000000}
__device__ __forceinline__ uint32_t page_rate_word(const uint32_t* __restrict__ w, unsigned b, unsigned i) {
    if (b < PAGE_BLOCKS - 1) return w[8 * b + i];
    return i == 0 ? 1u : i == 7 ? 0x80000000u : 0u;
}
// ... of the image id's 36 bytes (the root's words byte-swapped, then pc): block 0 the root, block 1 {pc, 1, 0, .., 0x80000000}
__device__ __forceinline__ uint32_t id_tail_word(uint32_t pc, unsigned i) { return i == 0 ? pc : i == 1 ? 1u : i == 7 ? 0x80000000u : 0u; }

// FORM 0: a chain owns a 16-lane row of the wave (lanes 0..11 = the state words), four chains a wave.  FORM 1: a chain owns a quad of
// lanes (lane q holds words q, q + 4, q + 8), sixteen chains a wave.  The lanes past the launch's last chain repeat it and store nothing.
template <int FORM>
__global__ __launch_bounds__(64) void k_image_level(const image_desc* S, unsigned level) {
    constexpr unsigned PER = FORM == 0 ? 4 : 16, LANES = 64 / PER;
    __shared__ __attribute__((aligned(16))) uint32_t quad_tab[FORM == 1 ? ZKM_QUAD_TAB_WORDS : 4];
    const image_desc& A = S[blockIdx.z];
    const unsigned nch = level == 0 ? A.nd : level == 1 ? A.n1 : level == 2 ? A.n2 : 1, c0 = PER * blockIdx.x;
    if (c0 >= nch) return;
    const unsigned lane = threadIdx.x, idx = lane % LANES;
    const unsigned ch = min(c0 + lane / LANES, nch - 1);
    const bool mine = c0 + lane / LANES < nch;
    const uint32_t* __restrict__ w = level == 0 ? A.dirty + (size_t)ch * PAGE_WORDS
                                                : A.plan + (size_t)(level == 1 ? ch : level == 2 ? A.n1 + ch : A.n1 + A.n2) * PAGE_WORDS;
    uint32_t* out = level < 3 ? A.plan + A.slot[(level == 0 ? 0 : level == 1 ? A.nd : A.nd + A.n1) + ch] : A.result;
    if constexpr (FORM == 0) {
        uint64_t x = 0;
        uint32_t nxt = idx < 8 ? page_rate_word(w, 0, idx) : 0;
#pragma unroll 1
        for (unsigned b = 0; b < PAGE_BLOCKS; b++) {
            if (idx < 8) x = nxt;
            if (idx < 8 && b + 1 < PAGE_BLOCKS) nxt = page_rate_word(w, b + 1, idx);
            x = poseidon_permute_wide(x, lane);
        }
        if (mine && idx < 4) { out[2 * idx] = (uint32_t)x; out[2 * idx + 1] = (uint32_t)(x >> 32); }
        if (level < 3) return;                                   // (uniform: a launch is one level)
        // the image id: digest word idx / 2 of this row, its low or high half, byte-swapped
        const int from = (int)((lane & ~15u) + ((idx & 7) >> 1));
        const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)x, from), hi = (uint32_t)__shfl((int)(uint32_t)(x >> 32), from);
        x = idx < 8 ? __builtin_bswap32(idx & 1 ? hi : lo) : 0;
        x = poseidon_permute_wide(x, lane);
        if (idx < 8) x = id_tail_word(A.pc, idx);
        x = poseidon_permute_wide(x, lane);
        if (mine && idx < 4) { out[8 + 2 * idx] = (uint32_t)x; out[9 + 2 * idx] = (uint32_t)(x >> 32); }
    } else {
        quad_tab_load(quad_tab);
        const poseidon_quad Q(lane, quad_tab);
        uint64_t s[3] = {0, 0, 0};
        uint32_t n0 = page_rate_word(w, 0, idx), n1 = page_rate_word(w, 0, idx + 4);
#pragma unroll 1
        for (unsigned b = 0; b < PAGE_BLOCKS; b++) {
            s[0] = n0; s[1] = n1;
            if (b + 1 < PAGE_BLOCKS) { n0 = page_rate_word(w, b + 1, idx); n1 = page_rate_word(w, b + 1, idx + 4); }
            poseidon_permute_quad(s, Q);
        }
        if (mine) { out[2 * idx] = (uint32_t)s[0]; out[2 * idx + 1] = (uint32_t)(s[0] >> 32); }
        if (level < 3) return;
        // root word idx is a half of digest word idx / 2 (lane idx / 2 of the quad), root word idx + 4 one of digest word 2 + idx / 2
        const int base = (int)(lane & ~3u);
        const uint32_t dl = (uint32_t)s[0], dh = (uint32_t)(s[0] >> 32);
        const uint32_t al = (uint32_t)__shfl((int)dl, base + (int)(idx >> 1)), ah = (uint32_t)__shfl((int)dh, base + (int)(idx >> 1));
        const uint32_t bl = (uint32_t)__shfl((int)dl, base + 2 + (int)(idx >> 1)), bh = (uint32_t)__shfl((int)dh, base + 2 + (int)(idx >> 1));
        s[0] = __builtin_bswap32(idx & 1 ? ah : al);
        s[1] = __builtin_bswap32(idx & 1 ? bh : bl);
        s[2] = 0;
        poseidon_permute_quad(s, Q);
        s[0] = id_tail_word(A.pc, idx);
        s[1] = id_tail_word(A.pc, idx + 4);
        poseidon_permute_quad(s, Q);
        if (mine) { out[8 + 2 * idx] = (uint32_t)s[0]; out[9 + 2 * idx] = (uint32_t)(s[0] >> 32); }
    }
}

// ---- host side

// hash_page on the host (host_poseidon.hip), for the three constant digests only
void host_hash_page(const uint32_t* words, uint32_t out[8]) {
    uint64_t st[12] = {0};
    for (unsigned b = 0; b < PAGE_BLOCKS; b++) {
        for (unsigned i = 0; i < 8; i++) st[i] = b < PAGE_BLOCKS - 1 ? words[8 * b + i] : i == 0 ? 1u : i == 7 ? 0x80000000u : 0u;
        zkm_host_poseidon_permute(st);
    }
    for (unsigned i = 0; i < 4; i++) {
        const uint64_t v = st[i] >= GL_P ? st[i] - GL_P : st[i];
        out[2 * i] = (uint32_t)v;
        out[2 * i + 1] = (uint32_t)(v >> 32);
    }
}
// compute_const_hash_pages: the fill of a fresh L1 page is the zero page's digest, of a fresh L2 page the fresh L1 page's, of a fresh
// root the fresh L2 page's.  Made once per process, at the first call.
const level_consts& const_digests() {
    static level_consts K;
    static std::once_flag once;
    std::call_once(once, [] {
        std::vector<uint32_t> page(PAGE_WORDS, 0);
        for (unsigned l = 0; l < 3; l++) {
            host_hash_page(page.data(), K.d[l]);
            for (unsigned w = 0; w < PAGE_WORDS; w++) page[w] = K.d[l][w & 7];
        }
    });
    return K;
}

std::string hex(uint32_t v) {
    char buf[16];
    snprintf(buf, sizeof buf, "0x%x", v);
    return buf;
}

// the L1 pages, the L2 pages and the root of ascending dirty pages
void plan_of(const uint32_t* dirty, size_t nd, std::vector<uint32_t>& l1, std::vector<uint32_t>& l2) {
    for (size_t i = 0; i < nd; i++) {
        const uint32_t a = L1_BASE + (dirty[i] >> 7), b = L2_BASE + (dirty[i] >> 14);
        if (l1.empty() || l1.back() != a) l1.push_back(a);
        if (l2.empty() || l2.back() != b) l2.push_back(b);
    }
}

size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

struct image_job {
    std::vector<uint32_t> l1, l2;
    size_t nd = 0, np = 0;
    bool dirty_host = false, known_host = false, out_host = false;
    size_t o_tab = 0, o_dirty = 0, o_known = 0, o_plan = 0;      // byte offsets into the call's block
};

// every check of the header, on the host, before any device work
void validate(const zkm_image_pages& in, const uint32_t* out, image_job& j) {
    if ((in.ndirty && (!in.dirty_index || !in.dirty_words)) || (in.nknown && (!in.known_index || !in.known_words)))
        throw std::runtime_error("null pointer with a nonzero count");
    if (!out) throw std::runtime_error("null argument (hash_words_out)");
    for (size_t i = 0; i < in.ndirty; i++) {
        if (in.dirty_index[i] >= MAIN_PAGES)
            throw std::runtime_error("dirty index " + std::to_string(i) + " = " + hex(in.dirty_index[i]) + " is not below 0x80000");
        if (i && in.dirty_index[i - 1] >= in.dirty_index[i])
            throw std::runtime_error("dirty index " + std::to_string(i) + " = " + hex(in.dirty_index[i]) + " is not above the one before it");
    }
    j.nd = in.ndirty;
    plan_of(in.dirty_index, in.ndirty, j.l1, j.l2);
    j.np = j.l1.size() + j.l2.size() + 1;
    bool root_known = false;
    for (size_t i = 0; i < in.nknown; i++) {
        const uint32_t q = in.known_index[i];
        if (i && in.known_index[i - 1] >= q)
            throw std::runtime_error("known index " + std::to_string(i) + " = " + hex(q) + " is not above the one before it");
        if (q != ROOT_INDEX && !std::binary_search(j.l1.begin(), j.l1.end(), q) && !std::binary_search(j.l2.begin(), j.l2.end(), q))
            throw std::runtime_error("known index " + std::to_string(i) + " = " + hex(q) + " is not a hash page of the plan");
        root_known = root_known || q == ROOT_INDEX;
    }
    if (!in.ndirty && !root_known)
        throw std::runtime_error("compute image ID fail: no dirty page, and the root page 0x81020 is not among the known pages");
}

template <class K> void launch(hipStream_t st, K kernel, size_t blocks, unsigned threads, size_t nimg, const image_desc* d, unsigned level) {
    if (!blocks) return;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks, 1, (unsigned)nimg), dim3(threads), 0, st, d, level);
    ZKM_HIP_CHECK(hipGetLastError());
}

void images_hash(zkm_ctx* c, const char* what, size_t nimg, const zkm_image_pages* in, uint32_t* const* outs, uint8_t* roots, uint8_t* ids) {
    const std::string name(what);
    if (!nimg) return;
    if (!in || !outs || !roots || !ids) throw std::runtime_error(name + ": null argument");
    if (nimg > 65535) throw std::runtime_error(name + ": more than 65535 images");
    std::vector<image_job> jobs(nimg);
    for (size_t m = 0; m < nimg; m++) {
        try {
            validate(in[m], outs[m], jobs[m]);
        } catch (const std::exception& e) {
            throw std::runtime_error(name + ": " + (name == "zkm_images_hash" ? "image " + std::to_string(m) + ": " : "") + e.what());
        }
    }
    // the block: descriptors, results, every image's tables -- one upload -- then the pages
    size_t bytes = up256(nimg * sizeof(image_desc));
    const size_t o_res = bytes;
    bytes += up256(nimg * 64);
    size_t max_nd = 0, max_n1 = 0, max_n2 = 0, max_np = 0, tot_nd = 0, tot_n1 = 0, tot_n2 = 0;
    for (size_t m = 0; m < nimg; m++) {
        image_job& j = jobs[m];
        j.o_tab = bytes;
        bytes += up256((j.np + j.nd + j.np - 1) * 4);
    }
    const size_t head = bytes;
    bool any_host_out = false;
    for (size_t m = 0; m < nimg; m++) {
        image_job& j = jobs[m];
        j.dirty_host = j.nd && !zkm_is_device_ptr(in[m].dirty_words);
        j.known_host = in[m].nknown && !zkm_is_device_ptr(in[m].known_words);
        j.out_host = !zkm_is_device_ptr(outs[m]);
        any_host_out = any_host_out || j.out_host;
        j.o_dirty = bytes;
        bytes += j.dirty_host ? j.nd * 4096 : 0;
        j.o_known = bytes;
        bytes += j.known_host ? in[m].nknown * 4096 : 0;
        j.o_plan = bytes;
        bytes += j.np * 4096;
        max_nd = std::max(max_nd, j.nd); max_n1 = std::max(max_n1, j.l1.size()); max_n2 = std::max(max_n2, j.l2.size());
        max_np = std::max(max_np, j.np);
        tot_nd += j.nd; tot_n1 += j.l1.size(); tot_n2 += j.l2.size();
    }
    std::vector<char> h(head, 0);      // (declared before the block: it outlives the copies queued from it on every path)
    std::vector<uint32_t> h_res(nimg * 16);
    zkm_scratch block(c, bytes);
    char* sb = block.as<char>();
    for (size_t m = 0; m < nimg; m++) {
        const image_job& j = jobs[m];
        const zkm_image_pages& I = in[m];
        const size_t n1 = j.l1.size(), n2 = j.l2.size();
        image_desc d{};
        d.dirty = j.dirty_host ? (const uint32_t*)(sb + j.o_dirty) : I.dirty_words;
        d.plan = (uint32_t*)(sb + j.o_plan);
        d.known = j.known_host ? (const uint32_t*)(sb + j.o_known) : I.known_words;
        d.known_of = (const int32_t*)(sb + j.o_tab);
        d.slot = (const uint32_t*)(sb + j.o_tab) + j.np;
        d.result = (uint32_t*)(sb + o_res) + 16 * m;
        d.nd = (uint32_t)j.nd; d.n1 = (uint32_t)n1; d.n2 = (uint32_t)n2; d.pc = I.pc;
        memcpy(d.regs, I.registers, sizeof d.regs);
        memcpy(h.data() + m * sizeof(image_desc), &d, sizeof d);
        int32_t* known_of = (int32_t*)(h.data() + j.o_tab);
        uint32_t* slot = (uint32_t*)(h.data() + j.o_tab) + j.np;
        auto plan_pos = [&](uint32_t q) -> size_t {       // (q is in the plan)
            if (q == ROOT_INDEX) return n1 + n2;
            if (q >= L2_BASE) return n1 + (std::lower_bound(j.l2.begin(), j.l2.end(), q) - j.l2.begin());
            return std::lower_bound(j.l1.begin(), j.l1.end(), q) - j.l1.begin();
        };
        for (size_t i = 0; i < j.np; i++) known_of[i] = -1;
        for (size_t i = 0; i < I.nknown; i++) known_of[plan_pos(I.known_index[i])] = (int32_t)i;
        for (size_t i = 0; i < j.nd; i++) {
            const uint32_t p = I.dirty_index[i];
            slot[i] = (uint32_t)(plan_pos(L1_BASE + (p >> 7)) * PAGE_WORDS + (p & 127) * 8);
        }
        for (size_t i = 0; i < n1; i++) {
            const uint32_t q = j.l1[i] - L1_BASE;
            slot[j.nd + i] = (uint32_t)(plan_pos(L2_BASE + (q >> 7)) * PAGE_WORDS + (q & 127) * 8);
        }
        for (size_t i = 0; i < n2; i++) slot[j.nd + n1 + i] = (uint32_t)((n1 + n2) * PAGE_WORDS + (j.l2[i] - L2_BASE) * 8);
        if (j.dirty_host) ZKM_HIP_CHECK(hipMemcpyAsync(sb + j.o_dirty, I.dirty_words, j.nd * 4096, hipMemcpyHostToDevice, c->stream));
        if (j.known_host) ZKM_HIP_CHECK(hipMemcpyAsync(sb + j.o_known, I.known_words, I.nknown * 4096, hipMemcpyHostToDevice, c->stream));
    }
    if (head <= zkm_ctx::XFER_UP / 4) c->upload(sb, h.data(), head);
    else ZKM_HIP_CHECK(hipMemcpyAsync(sb, h.data(), head, hipMemcpyHostToDevice, c->stream));
    const image_desc* d_desc = (const image_desc*)sb;
    {
        zkm_prof_scope ps(c, "image_hash/init");
        hipLaunchKernelGGL(k_image_init, dim3((unsigned)(max_np * 4), 1, (unsigned)nimg), dim3(256), 0, c->stream, d_desc, const_digests());
        ZKM_HIP_CHECK(hipGetLastError());
    }
    const size_t per_level[4] = {max_nd, max_n1, max_n2, 1}, total[4] = {tot_nd, tot_n1, tot_n2, nimg};
    for (unsigned level = 0; level < 4; level++) {
        const bool quad = c->image_hash_form ? c->image_hash_form == 2 : total[level] > c->image_hash_row_max;
        zkm_prof_scope ps(c, "image_hash/level");
        if (quad) launch(c->stream, k_image_level<1>, (per_level[level] + 15) / 16, 64, nimg, d_desc, level);
        else launch(c->stream, k_image_level<0>, (per_level[level] + 3) / 4, 64, nimg, d_desc, level);
    }
    // the outputs: the one host wait of the call
    for (size_t m = 0; m < nimg; m++)
        ZKM_HIP_CHECK(hipMemcpyAsync(outs[m], sb + jobs[m].o_plan, jobs[m].np * 4096, jobs[m].out_host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice,
                                     c->stream));
    if (any_host_out) {
        ZKM_HIP_CHECK(hipMemcpyAsync(h_res.data(), sb + o_res, nimg * 64, hipMemcpyDeviceToHost, c->stream));
        c->sync();
    } else {
        c->download(h_res.data(), sb + o_res, nimg * 64);
    }
    for (size_t m = 0; m < nimg; m++) {
        memcpy(roots + 32 * m, h_res.data() + 16 * m, 32);
        memcpy(ids + 32 * m, h_res.data() + 16 * m + 8, 32);
    }
}

}  // namespace

extern "C" {

size_t zkm_image_hash_plan(const uint32_t* dirty_index, size_t ndirty, uint32_t* hash_index_out, size_t capacity) {
    std::vector<uint32_t> l1, l2;
    if (dirty_index) plan_of(dirty_index, ndirty, l1, l2);
    const size_t n1 = l1.size(), n = n1 + l2.size() + 1;
    for (size_t i = 0; hash_index_out && i < n && i < capacity; i++) hash_index_out[i] = i < n1 ? l1[i] : i < n - 1 ? l2[i - n1] : ROOT_INDEX;
    return n;
}

int zkm_image_hash(zkm_ctx* c, const zkm_image_pages* in, uint32_t* hash_words_out, uint8_t page_hash_root_out[32], uint8_t image_id_out[32],
                   char** err) {
    return zkm_api("zkm_image_hash", c, err, [&] {
        if (!in) throw std::runtime_error("zkm_image_hash: null argument");
        images_hash(c, "zkm_image_hash", 1, in, &hash_words_out, page_hash_root_out, image_id_out);
    });
}

int zkm_images_hash(zkm_ctx* c, size_t nimg, const zkm_image_pages* in, uint32_t* const* hash_words_out, uint8_t* page_hash_roots_out,
                    uint8_t* image_ids_out, char** err) {
    return zkm_api("zkm_images_hash", c, err, [&] { images_hash(c, "zkm_images_hash", nimg, in, hash_words_out, page_hash_roots_out, image_ids_out); });
}

}  // extern "C"
