// calls_stage.hip -- K segments' calls staged behind the current proofs (include/zkm_hip.h "Staged calls"): what zkm_segments_calls_expand
// does on the calling thread and the compute stream -- the four expansions, the records placed into the step list, one host wait -- and
// what the builder then does with the patched list on the host -- the walk -- queued on the context's two copy streams instead, with no
// host wait and nothing read per row on the host.
//
// The host does what calls_entry.hip does per call (zkm_calls_counts, zkm_calls_plan_lists: every refusal that needs no row's clock, the
// counts, the block's layout).  Everything else is queued:
//   copy stream 2   the segment's own ready-made rows and own lists, the images' words
//   copy stream 1   the step records, every list the expansion kernels read, the zero-fill of the SHA and Keccak rows, the four
//                   expansion launches (the kinds' own launchers, given this stream), the placement, the walk of cpu_steps_walk.hip
//                   over the patched list (behind stream 2's rows), the two sets of verdicts down into pinned memory
// k_calls_place   one thread per generated row, the segment is blockIdx.z.  The row's kind follows from the four kind ends, its call
//                 from a search over the kind's per-call row offsets; its record and clock are the kinds' one statement each
//                 (calls_place_dev.h row_rec: what zkm_*_calls_steps write on the host).  A row whose clock lies outside the list
//                 touches nothing.  A row inside sends its index j to the position's owner word with one atomicMin: the word's earlier
//                 value tells it whether a lower row holds the position (this row is refused) or a higher one did (that row is).  The
//                 lowest refused j of a wave goes to the segment's verdict with one atomicMin -- the row the host's loop names, since
//                 that loop walks j upwards and stops at the first row that lies outside or finds its position taken.
// k_calls_verdict one thread a segment: the refused row's clock beside its j, from which the host rebuilds the message.
// The walk then reads the patched list in place: the handle owns a zkm_staged_steps over it (zkm_steps_stage_queue), which is how the
// builder knows the segment, orders itself behind it and gets counts, bases and the walk's refusal.
#include <memory>

#include "calls_launch.h"
#include "calls_place_dev.h"

namespace {

using namespace zkm_calls;
constexpr unsigned CPU_W = ZKM_CPU_COLS, THREADS = 256;
constexpr uint32_t NONE = 0xFFFFFFFFu;          // an owner word nobody holds; a verdict without a refused row
constexpr size_t MAX_STEPS = (size_t)1 << 28;   // the builder's own limit (as zkm_cpu_steps_stage refuses it)

// what the device says of one segment's placement (filled with ones in front): the lowest refused row, and its clock
struct place_verdict {
    uint32_t first_bad, pad;
    uint64_t clock;
};

// one segment as the placement reads it; every pointer is device memory
struct place_seg {
    const uint64_t *emeta, *cmeta;                 // the SHA calls' metas
    const uint64_t *koff, *kmeta, *krow;           // the Keccak calls' offsets (nk + 1), metas, first rows (nk + 1)
    const uint32_t* ikinds;                        // the I/O calls' kinds, offsets (ni + 1), metas, first rows (ni + 1)
    const uint64_t *ioff, *imeta, *irow;
    const zkm_cpu_step* insns;                     // the instruction records and their clocks
    const uint64_t* iclocks;
    uint64_t E, nk, ni;
    uint64_t kind_end[4];                          // where the rows of the SHA, Keccak and I/O calls and of the instructions end
    uint64_t raw_base, first_clock, nsteps;
    zkm_cpu_step* steps;                           // nsteps records: the segment's own, patched here
    uint32_t* owner;                               // nsteps words, NONE in front
    place_verdict* verdict;
};

// the call k with off[k] <= row < off[k + 1]; off holds n + 1 strictly increasing entries (every call has a row) and row < off[n]
__device__ __forceinline__ uint64_t call_of(const uint64_t* __restrict__ off, uint64_t n, uint64_t row) {
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (off[mid] <= row) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ zkm_cpu_step load_step(const zkm_cpu_step* at) {
    const uint4* p = (const uint4*)at;
    const uint4 a = p[0], b = p[1], c = p[2];
    zkm_cpu_step t;
    t.pc = a.x; t.next_pc = a.y; t.insn = a.z; t.kind = a.w;
    t.flags = b.x; t.context = b.y; t.reads[0] = b.z; t.reads[1] = b.w;
    t.reads[2] = c.x; t.reads[3] = c.y; t.reads[4] = c.z; t.reads[5] = c.w;
    return t;
}

// the record of generated row j < kind_end[3], in the order SHA, Keccak, I/O, instructions
__device__ zkm_row_rec row_of(const place_seg& A, uint64_t j) {
    if (j < A.kind_end[0]) return zkm_sha_place::row_rec(A.emeta, A.E, A.cmeta, j);
    if (j < A.kind_end[1]) {
        const uint64_t r = j - A.kind_end[0], k = call_of(A.krow, A.nk, r);
        return zkm_keccak_place::row_rec(A.koff, A.kmeta, k, r - A.krow[k]);
    }
    if (j < A.kind_end[2]) {
        const uint64_t r = j - A.kind_end[1], k = call_of(A.irow, A.ni, r);
        return zkm_io_place::row_rec(A.ikinds, A.ioff, A.imeta, k, r - A.irow[k]);
    }
    const uint64_t r = j - A.kind_end[2];
    return zkm_insn::row_rec(load_step(A.insns + r), A.iclocks[r]);
}

__global__ __launch_bounds__(THREADS) void k_calls_place(const place_seg* __restrict__ segs) {
    const place_seg A = zkm_seg_desc(segs);   // (uniform: scalar loads)
    const uint64_t rows = A.kind_end[3];
    if ((uint64_t)blockIdx.x * THREADS >= rows) return;
    const uint64_t j = (uint64_t)blockIdx.x * THREADS + threadIdx.x;
    uint32_t bad = NONE;
    if (j < rows) {
        const zkm_row_rec r = row_of(A, j);
        const uint64_t p = r.clock - A.first_clock;
        if (r.clock < A.first_clock || p >= A.nsteps) {
            bad = (uint32_t)j;   // outside the list: neither the owner word nor the list is touched
        } else {
            const uint32_t old = atomicMin(&A.owner[p], (uint32_t)j);
            if (old < j) {
                bad = (uint32_t)j;           // a lower row holds the position
            } else {
                if (old != NONE) bad = old;  // a higher row held it: that one shares its position with this lower one
                const zkm_cpu_step s = raw_step(A.raw_base + j, r.mask);
                uint4* q = (uint4*)(A.steps + p);
                q[0] = make_uint4(s.pc, s.next_pc, s.insn, s.kind);
                q[1] = make_uint4(s.flags, s.context, s.reads[0], s.reads[1]);
                q[2] = make_uint4(s.reads[2], s.reads[3], s.reads[4], s.reads[5]);
            }
        }
    }
    if (__ballot(bad != NONE) == 0) return;
#pragma unroll
    for (unsigned d = 32; d; d >>= 1) {
        const uint32_t o = __shfl_down(bad, d);
        bad = o < bad ? o : bad;
    }
    if ((threadIdx.x & 63) == 0) atomicMin(&A.verdict->first_bad, bad);
}

__global__ __launch_bounds__(64) void k_calls_verdict(const place_seg* __restrict__ segs) {
    const place_seg A = zkm_seg_desc(segs);
    if (threadIdx.x) return;
    const uint32_t j = A.verdict->first_bad;
    if (j == NONE || j >= A.kind_end[3]) return;
    A.verdict->clock = row_of(A, j).clock;
}

// one list of a segment that the device reads: in place where the caller has it in device memory, else a copy in the handle's block
struct slot {
    const void* src = nullptr;
    size_t bytes = 0, at = 0;
    bool up = false;
    int stream = 0;
    const void* dev(const char* sb) const { return up ? sb + at : src; }
};

// A profiling scope on a copy stream (zkm_prof_scope's pair of events is recorded on the compute stream): calls_stage/expand,
// calls_stage/place and calls_stage/walk are read once the handle is ready.
struct copy_scope {
    zkm_ctx* c;
    hipStream_t st;
    size_t idx = 0;
    bool on;
    copy_scope(zkm_ctx* ctx, hipStream_t s, const char* name) : c(ctx), st(s), on(ctx->profiling) {
        if (!on) return;
        const zkm_prof_rec r{name, c->get_event(), c->get_event()};
        ZKM_HIP_CHECK(hipEventRecord(r.start, st));
        c->prof.push_back(r);
        c->prof_agg_valid = false;
        idx = c->prof.size() - 1;
    }
    copy_scope(const copy_scope&) = delete;
    ~copy_scope() {
        if (on && idx < c->prof.size()) (void)hipEventRecord(c->prof[idx].stop, st);
    }
};

}  // namespace

// The handle: one block for every segment's eight lists, the copies of the call lists, the patched step lists, the owner words, the
// images' words and the placement's descriptors and verdicts; one for the launchers' scratch; the host memory that queued uploads read
// (the jobs' vectors, the descriptors); the pinned words the placement's verdicts come down into; the staged steps over the patched lists.
struct zkm_staged_calls {
    zkm_ctx* ctx = nullptr;
    zkm_scratch block, scratch;          // the lists and records; the launchers' descriptors and host-walk vectors
    struct seg {
        zkm_segment_calls q{};   // (its counts and first_clock: the refusals' texts; the pointers are the caller's and are not read again)
        size_t n[ZKM_CALLS_COUNTS] = {};
        zkm_cpu_steps st{};
        zkm_segment_ops ops{};
        zkm_boot_image image{};
        std::string refusal;
        std::vector<uint64_t> krow;   // the Keccak calls' first rows, nk + 1
    };
    std::vector<seg> segs;
    std::vector<zkm_sha_job> sha;
    std::vector<zkm_keccak_job> keccak;
    std::vector<zkm_io_job> io;
    std::vector<zkm_insn_job> insn;
    std::vector<place_seg> desc;
    zkm_calls_hold hold;
    zkm_pinned<place_verdict> verdicts;
    zkm_staged_steps* steps = nullptr;   // owns the walk's block and the fence that stands for everything this handle has queued
    bool resolved = false;
    ~zkm_staged_calls() { zkm_staged_steps_free(steps); }   // (waits for that fence before the members above go)
};

namespace {

// the host's one wait for a handle (the staged steps' own), and every segment's refusal: the placement's first, else the walk's
void resolve(zkm_staged_calls* h) {
    if (h->resolved) return;
    for (size_t s = 0; s < h->segs.size(); s++) {
        zkm_staged_calls::seg& g = h->segs[s];
        zkm_staged_steps_ref ref;
        zkm_staged_steps_at(h->steps, s, &ref);
        const place_verdict& v = h->verdicts.p[s];
        g.refusal = v.first_bad != NONE ? zkm_calls_row_refusal(g.q, g.n, v.first_bad, v.clock) : ref.refusal;
    }
    h->resolved = true;
}

// seg_base: position of segment 0 in the caller's larger call (the pool's groups; refusals only)
std::unique_ptr<zkm_staged_calls> stage(const std::string& what, zkm_ctx* c, size_t nseg, const zkm_segment_calls* calls, const zkm_boot_image* images,
                                        size_t seg_base = 0) {
    if (nseg == 0 || !calls) throw std::runtime_error(what + ": null argument or no segment");
    std::unique_ptr<zkm_staged_calls> h(new zkm_staged_calls);
    h->ctx = c;
    h->segs.resize(nseg);
    h->sha.resize(nseg), h->keccak.resize(nseg), h->io.resize(nseg), h->insn.resize(nseg), h->desc.resize(nseg);
    // ---- every refusal that needs no row's clock, per call and never per row
    std::vector<zkm_calls_plan> P(nseg);
    for (size_t s = 0; s < nseg; s++) {
        try {
            const zkm_segment_calls& q = calls[s];
            zkm_calls_counts(q, P[s].n);
            zkm_calls_plan_lists(q, P[s]);
            if (q.steps.nsteps > MAX_STEPS) throw std::runtime_error(dec(q.steps.nsteps) + " steps, more than 2^28");
            if (P[s].n[N_RAW] - q.steps.nraw >= NONE) throw std::runtime_error("2^32 or more generated rows");
            if (images && images[s].nwords && (!images[s].addrs || !images[s].values))
                throw std::runtime_error("image: NULL addrs or values with a count of " + dec(images[s].nwords));
        } catch (const std::exception& e) {
            throw std::runtime_error(what + ": segment " + dec(seg_base + s) + ": " + e.what());
        }
    }
    if (!c) throw std::runtime_error(what + ": null argument");
    ZKM_HIP_CHECK(hipSetDevice(c->device));

    // ---- the block's layout: per segment its eight lists, then the lists that go up, the patched records and the owner words; the
    // descriptors and the verdicts of all segments behind them
    enum { W16, EMETA, HX, W, CMETA, KIN, KOFF, KMETA, KDIG, KROW, IKINDS, IDATA, IOFF, IMETA, IROW, INSNS, ICLOCKS, STEPS, ADDRS, VALUES, NSLOT };
    std::vector<std::array<slot, NSLOT>> L(nseg);
    std::vector<size_t> lists_at(nseg), owner_at(nseg);
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t here = at;
        at += up256(bytes);
        return here;
    };
    for (size_t s = 0; s < nseg; s++) {
        const zkm_segment_calls& q = calls[s];
        zkm_calls_plan& p = P[s];
        zkm_staged_calls::seg& g = h->segs[s];
        g.q = q;
        std::copy(p.n, p.n + ZKM_CALLS_COUNTS, g.n);
        g.krow.resize(q.nkeccak ? q.nkeccak + 1 : 0);
        for (size_t k = 0; k < q.nkeccak; k++) g.krow[k] = p.keccak.bases[k].row;
        if (q.nkeccak) g.krow[q.nkeccak] = p.keccak.nrows;
        lists_at[s] = take(p.total);
        const size_t kbytes = q.nkeccak ? q.keccak_input_off[q.nkeccak] - q.keccak_input_off[0] : 0;
        const size_t ibytes = q.nio ? q.io_data_off[q.nio] - q.io_data_off[0] : 0;
        const zkm_boot_image* im = images ? images + s : nullptr;
        const size_t imw = im ? im->nwords * 4 : 0;
        // (the bytes of the Keccak and I/O calls go up from the first call's offset on: the jobs' off_up count from there)
        const struct { int i; const void* p; size_t bytes; int stream; } in[NSLOT] = {
            {W16, q.extend_w16, 64 * q.nextend, 0}, {EMETA, q.extend_meta, 32 * q.nextend, 0}, {HX, q.compress_hx, 32 * q.ncompress, 0},
            {W, q.compress_w, 256 * q.ncompress, 0}, {CMETA, q.compress_meta, 64 * q.ncompress, 0},
            {KIN, q.keccak_inputs, kbytes, 0}, {KOFF, p.keccak.off_up.data(), 8 * p.keccak.off_up.size(), 0}, {KMETA, q.keccak_meta, 32 * q.nkeccak, 0},
            {KDIG, q.keccak_digest_addrs, 8 * q.nkeccak, 0}, {KROW, g.krow.data(), 8 * g.krow.size(), 0},
            {IKINDS, q.io_kinds, 4 * q.nio, 0}, {IDATA, q.io_data, ibytes, 0}, {IOFF, p.io.off_up.data(), 8 * p.io.off_up.size(), 0},
            {IMETA, q.io_meta, 32 * q.nio, 0}, {IROW, p.io.row_off.data(), q.nio ? 8 * p.io.row_off.size() : 0, 0},
            {INSNS, q.insns, sizeof(zkm_cpu_step) * q.ninsns, 0}, {ICLOCKS, q.insn_clocks, 8 * q.ninsns, 0},
            {STEPS, q.steps.steps, sizeof(zkm_cpu_step) * q.steps.nsteps, 0},
            {ADDRS, im ? im->addrs : nullptr, imw, 1}, {VALUES, im ? im->values : nullptr, imw, 1}};
        for (const auto& l : in) {
            slot& t = L[s][l.i];
            t.src = l.p, t.bytes = l.bytes, t.stream = l.stream;
            // the records are copied wherever they lie (they are patched); everything else in device memory is read in place
            t.up = l.bytes && (l.i == STEPS || !zkm_is_device_ptr(l.p));
            if (t.up && l.i == KIN) t.src = q.keccak_inputs + q.keccak_input_off[0];
            if (t.up && l.i == IDATA) t.src = q.io_data + q.io_data_off[0];
            if (t.up) t.at = take(l.bytes);
        }
        owner_at[s] = take(4 * q.steps.nsteps);
    }
    const size_t desc_at = take(nseg * sizeof(place_seg)), verdict_at = take(nseg * sizeof(place_verdict));

    // ---- the block, the jobs bound to it, what the builder takes
    h->verdicts.alloc(nseg);
    h->block = zkm_scratch(c, at);
    char* sb = h->block.as<char>();
    std::vector<zkm_cpu_steps> st(nseg);
    std::vector<std::array<char*, 8>> own_dst(nseg);
    for (size_t s = 0; s < nseg; s++) {
        const zkm_segment_calls& q = calls[s];
        zkm_calls_plan& p = P[s];
        zkm_staged_calls::seg& g = h->segs[s];
        const auto& l = L[s];
        zkm_calls_bind(q, p, p.total ? sb + lists_at[s] : nullptr, own_dst[s].data(), g.ops);
        // the jobs read the call lists where the device has them: the launchers put up only their descriptors and the host walk's vectors
        p.sha.w16 = (const uint32_t*)l[W16].dev(sb), p.sha.emeta = (const uint64_t*)l[EMETA].dev(sb), p.sha.hx = (const uint32_t*)l[HX].dev(sb);
        p.sha.w = (const uint32_t*)l[W].dev(sb), p.sha.cmeta = (const uint64_t*)l[CMETA].dev(sb);
        p.keccak.inputs = (const uint8_t*)l[KIN].dev(sb), p.keccak.meta = (const uint64_t*)l[KMETA].dev(sb);
        p.keccak.digest_addrs = (const uint64_t*)l[KDIG].dev(sb);
        p.io.kinds = (const uint32_t*)l[IKINDS].dev(sb), p.io.data = (const uint8_t*)l[IDATA].dev(sb), p.io.meta = (const uint64_t*)l[IMETA].dev(sb);
        p.insn.insns = (const zkm_cpu_step*)l[INSNS].dev(sb), p.insn.clocks = (const uint64_t*)l[ICLOCKS].dev(sb);
        h->sha[s] = p.sha;
        h->keccak[s] = std::move(p.keccak);
        h->io[s] = std::move(p.io);
        h->insn[s] = std::move(p.insn);
        // the calls' groups of the operations: the device's copies, and the handle's own copy of the offsets the builder reads on the host
        zkm_segment_ops& o = g.ops;
        o.sha_extend_sponge_w16 = h->sha[s].w16, o.sha_extend_sponge_meta = h->sha[s].emeta;
        o.sha_compress_hx = o.sha_compress_sponge_hx = h->sha[s].hx;
        o.sha_compress_w = o.sha_compress_sponge_w = h->sha[s].w;
        o.sha_compress_meta = o.sha_compress_sponge_meta = h->sha[s].cmeta;
        o.keccak_sponge_inputs = h->keccak[s].inputs, o.keccak_sponge_off = h->keccak[s].off_up.data(), o.keccak_sponge_meta = h->keccak[s].meta;
        const size_t* n = g.n;
        g.st = st[s] = zkm_cpu_steps{q.steps.nsteps ? (const zkm_cpu_step*)l[STEPS].dev(sb) : nullptr, q.steps.nsteps,
                                     n[N_RAW] ? (const uint64_t*)own_dst[s][0] : nullptr, n[N_RAW]};
        if (images) {
            g.image = images[s];
            g.image.addrs = (const uint32_t*)l[ADDRS].dev(sb), g.image.values = (const uint32_t*)l[VALUES].dev(sb);
        }
        place_seg& d = h->desc[s];
        d.emeta = h->sha[s].emeta, d.cmeta = h->sha[s].cmeta, d.E = q.nextend;
        d.koff = (const uint64_t*)l[KOFF].dev(sb), d.kmeta = h->keccak[s].meta, d.krow = (const uint64_t*)l[KROW].dev(sb), d.nk = q.nkeccak;
        d.ikinds = h->io[s].kinds, d.ioff = (const uint64_t*)l[IOFF].dev(sb), d.imeta = h->io[s].meta, d.irow = (const uint64_t*)l[IROW].dev(sb);
        d.ni = q.nio;
        d.insns = h->insn[s].insns, d.iclocks = h->insn[s].clocks;
        d.kind_end[0] = n[N_SHA_ROWS], d.kind_end[1] = d.kind_end[0] + n[N_KECCAK_ROWS], d.kind_end[2] = d.kind_end[1] + n[N_IO_ROWS];
        d.kind_end[3] = d.kind_end[2] + n[N_INSN_ROWS];
        d.raw_base = q.steps.nraw, d.first_clock = q.first_clock, d.nsteps = q.steps.nsteps;
        d.steps = (zkm_cpu_step*)l[STEPS].dev(sb), d.owner = (uint32_t*)(sb + owner_at[s]), d.verdict = (place_verdict*)(sb + verdict_at) + s;
    }
    // the launchers' scratch, one part a kind and group (sized from the bound jobs: only what the host still holds goes up)
    const size_t ngroups = (nseg + ZKM_MAX_SEG - 1) / ZKM_MAX_SEG;
    std::vector<std::array<size_t, 4>> part(ngroups);
    size_t scratch_bytes = 0;
    for (size_t g = 0; g < ngroups; g++) {
        const size_t first = g * ZKM_MAX_SEG, k = std::min<size_t>(ZKM_MAX_SEG, nseg - first);
        part[g] = {zkm_sha_calls_scratch(&h->sha[first], k), zkm_keccak_calls_scratch(&h->keccak[first], k), zkm_io_calls_scratch(&h->io[first], k),
                   zkm_insn_rows_scratch(&h->insn[first], k)};
        for (const size_t b : part[g]) scratch_bytes += b;
    }
    h->scratch = zkm_scratch(c, scratch_bytes ? scratch_bytes : 256);

    // ---- the queue.  Of the fence the start and the guard (a failure from here on: what is in flight lands before `h` goes); the events
    // are the staged steps', recorded behind everything queued here
    zkm_copy_fence queued;
    queued.begin(c);
    const hipStream_t up = c->copy_stream, up2 = c->copy_stream2;
    ZKM_HIP_CHECK(hipMemsetAsync(sb + verdict_at, 0xFF, nseg * sizeof(place_verdict), up));
    ZKM_HIP_CHECK(hipMemcpyAsync(sb + desc_at, h->desc.data(), nseg * sizeof(place_seg), hipMemcpyHostToDevice, up));
    for (size_t s = 0; s < nseg; s++) {
        const zkm_segment_calls& q = calls[s];
        const zkm_calls_plan& p = P[s];
        for (const slot& t : L[s])
            if (t.up) ZKM_HIP_CHECK(hipMemcpyAsync(sb + t.at, t.src, t.bytes, hipMemcpyDefault, t.stream ? up2 : up));
        for (int i = 0; i < 8; i++)   // the segment's own rows and own lists
            if (p.own_bytes[i]) ZKM_HIP_CHECK(hipMemcpyAsync(own_dst[s][i], p.own_src[i], p.own_bytes[i], hipMemcpyDefault, up2));
        if (q.steps.nsteps) ZKM_HIP_CHECK(hipMemsetAsync(sb + owner_at[s], 0xFF, 4 * q.steps.nsteps, up));
        // the SHA and Keccak kernels store only the cells a row sets: their rows, adjacent, are zeroed by one memset a segment
        const size_t sparse = h->segs[s].n[N_SHA_ROWS] + h->segs[s].n[N_KECCAK_ROWS];
        if (sparse) ZKM_HIP_CHECK(hipMemsetAsync(h->sha[s].rows, 0, sparse * CPU_W * 8, up));
    }
    char* xb = h->scratch.as<char>();
    for (size_t g = 0; g < ngroups; g++) {
        const size_t first = g * ZKM_MAX_SEG, k = std::min<size_t>(ZKM_MAX_SEG, nseg - first);
        {
            const copy_scope ps(c, up, "calls_stage/expand");
            zkm_sha_calls_launch(c, &h->sha[first], k, xb, h->hold, false, up);
            zkm_keccak_calls_launch(c, &h->keccak[first], k, xb + part[g][0], h->hold, false, up);
            zkm_io_calls_launch(c, &h->io[first], k, xb + part[g][0] + part[g][1], h->hold, up);
            zkm_insn_rows_launch(c, &h->insn[first], k, xb + part[g][0] + part[g][1] + part[g][2], h->hold, up);
        }
        xb += part[g][0] + part[g][1] + part[g][2] + part[g][3];
        // the placement, behind the records' copies (this stream) and beside the expansions (they write rows and lists, not records)
        uint64_t most = 0;
        for (size_t s = first; s < first + k; s++) most = std::max(most, h->desc[s].kind_end[3]);
        if (!most) continue;
        const place_seg* d = (const place_seg*)(sb + desc_at) + first;
        const copy_scope ps(c, up, "calls_stage/place");
        hipLaunchKernelGGL(k_calls_place, dim3((unsigned)((most + THREADS - 1) / THREADS), 1, (unsigned)k), dim3(THREADS), 0, up, d);
        ZKM_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(k_calls_verdict, dim3(1, 1, (unsigned)k), dim3(64), 0, up, d);
        ZKM_HIP_CHECK(hipGetLastError());
    }
    ZKM_HIP_CHECK(hipMemcpyAsync(h->verdicts.p, sb + verdict_at, nseg * sizeof(place_verdict), hipMemcpyDeviceToHost, up));
    // the walk reads every ready-made row, the segment's own too: stream 1 goes behind stream 2's copies
    {
        const zkm_event e(c);
        e.record(up2);
        ZKM_HIP_CHECK(hipStreamWaitEvent(up, e.e, 0));
    }
    // the walk over the patched lists in place, its verdicts' download and the two events
    {
        const copy_scope ps(c, up, "calls_stage/walk");
        h->steps = zkm_steps_stage_queue(c, nseg, st.data(), false);
    }
    queued.disarm();
    return h;
}

}  // namespace

extern "C" {

int zkm_segments_calls_stage(zkm_ctx* c, size_t nseg, const zkm_segment_calls* calls, const zkm_boot_image* images, void** out, char** err) {
    return zkm_segments_calls_stage_entry(c, nseg, calls, images, out, err, 0);
}

int zkm_staged_calls_ready(void* staged, int wait) {
    const zkm_staged_calls* h = (const zkm_staged_calls*)staged;
    return h ? zkm_staged_steps_ready(h->steps, wait) : 1;
}

// the body of zkm_staged_calls_get (throws); a refusal names segment seg_base + segment
static void staged_get(void* staged, size_t segment, zkm_cpu_steps* steps_out, zkm_segment_ops* ops_out, zkm_boot_image* image_out, size_t seg_base) {
    const std::string what = "zkm_staged_calls_get";
    zkm_staged_calls* h = (zkm_staged_calls*)staged;
    if (!h || !steps_out || !ops_out) throw std::runtime_error(what + ": null argument");
    if (segment >= h->segs.size()) throw std::runtime_error(what + ": no segment " + dec(segment) + ": the handle holds " + dec(h->segs.size()));
    ZKM_HIP_CHECK(hipSetDevice(h->ctx->device));
    resolve(h);
    const zkm_staged_calls::seg& g = h->segs[segment];
    if (!g.refusal.empty()) throw std::runtime_error(what + ": segment " + dec(seg_base + segment) + ": " + g.refusal);
    zkm_staged_steps_join(h->steps);
    *steps_out = g.st;
    *ops_out = g.ops;
    if (image_out) *image_out = g.image;
}

int zkm_staged_calls_get(void* staged, size_t segment, zkm_cpu_steps* steps_out, zkm_segment_ops* ops_out, zkm_boot_image* image_out, char** err) {
    return zkm_staged_calls_get_entry(staged, segment, steps_out, ops_out, image_out, err, 0);
}

void zkm_staged_calls_free(void* staged) { delete (zkm_staged_calls*)staged; }

}  // extern "C"

// (zkm_internal.h: the pool's workers stage their groups under these entry points' own names)
int zkm_segments_calls_stage_entry(zkm_ctx* c, size_t nseg, const zkm_segment_calls* calls, const zkm_boot_image* images, void** out, char** err,
                                   size_t seg_base) {
    return zkm_api("zkm_segments_calls_stage", err, [&] {
        if (!out) throw std::runtime_error("zkm_segments_calls_stage: null argument");
        *out = nullptr;
        *out = stage("zkm_segments_calls_stage", c, nseg, calls, images, seg_base).release();
    });
}
int zkm_staged_calls_get_entry(void* staged, size_t segment, zkm_cpu_steps* steps_out, zkm_segment_ops* ops_out, zkm_boot_image* image_out, char** err,
                               size_t seg_base) {
    return zkm_api("zkm_staged_calls_get", err, [&] { staged_get(staged, segment, steps_out, ops_out, image_out, seg_base); });
}
