// cpu_steps_walk.hip -- the walk over a compact step log (cpu_steps.hip zkm_cpu_steps_walk) on the device, for K segments in one set of
// launches, and the steps staged ahead of a call on top of it (include/zkm_hip.h zkm_cpu_steps_stage).
//
// What a step produces is stated once (cpu_steps_dev.h zkm_step::count, __host__ __device__), so the device walk agrees with the host's
// by construction: the same refusals in the same order, the same three list lengths, and the same base triple per workgroup of
// ZKM_CPU_STEPS_BLOCK steps, word for word -- k_cpu_steps reads either as `base`.
//
// k_steps_walk   one thread per step, the segment is blockIdx.z: the record as three 16-byte loads, its counts, its first refusal (a RAW
//                index >= nraw; the code of count; a RAW mask that is not the `used` cells of its row -- the rows are in device memory
//                here, whichever memory the caller had them in).  A workgroup writes the sum of its packed counts as one triple; a wave
//                that holds a refused step sends the lowest such index to the segment's verdict with one atomicMin.
// k_steps_scan   one workgroup per segment: the exclusive scan of the triples in place (256 triples at 2^16 steps), the totals, and
//                for a refused segment the verdict record -- code, `used` mask and a copy of the failing record -- from which the host
//                rebuilds the host walk's message (zkm_cpu_step_refusal) without the caller's list.
// Both are bound by launch latency and a 48-byte read per step.
#include <map>
#include <memory>
#include <mutex>

#include "cpu_steps_dev.h"
#include "scan_dev.h"
#include "zkm_internal.h"

namespace {

using namespace zkm_step;
constexpr unsigned CPU_W = ZKM_CPU_COLS, BLOCK = ZKM_CPU_STEPS_BLOCK;
constexpr size_t MAX_STEPS = (size_t)1 << 28;   // the builder's own limit (SEG_MAX_LOG_N): 8 memory operations a step stay below 2^32
static_assert(BLOCK == SCAN_THREADS, "k_steps_scan scans with block_incl_scan");

// what the device says of one segment.  first_bad: the lowest refused step, all ones when there is none (the record is filled with
// ones before the walk); code, used and step are written for a refused segment only.
struct steps_verdict {
    uint32_t first_bad, code, used, pad;
    uint64_t total[3];   // memory, logic and arithmetic operations
    zkm_cpu_step step;
};
static_assert(sizeof(steps_verdict) == 88, "16 + 24 + 48 bytes, no padding");

struct walk_seg {
    const zkm_cpu_step* steps;   // device
    const uint64_t* raw;         // device: nraw ready-made rows
    size_t nsteps, nraw;
    uint32_t* base;              // device: one triple per workgroup (k_steps_walk: its sums; after k_steps_scan: its bases)
    steps_verdict* verdict;      // device
};

__device__ __forceinline__ zkm_cpu_step load_step(const zkm_cpu_step* at) {
    const uint4* p = (const uint4*)at;
    const uint4 a = p[0], b = p[1], c = p[2];
    zkm_cpu_step t;
    t.pc = a.x; t.next_pc = a.y; t.insn = a.z; t.kind = a.w;
    t.flags = b.x; t.context = b.y; t.reads[0] = b.z; t.reads[1] = b.w;
    t.reads[2] = c.x; t.reads[3] = c.y; t.reads[4] = c.z; t.reads[5] = c.w;
    return t;
}

// the first refusal of a step, in the host walk's order; k: its counts (zero when it is refused)
__device__ __forceinline__ int judge(const zkm_cpu_step& t, const walk_seg& A, counts& k, uint32_t& used) {
    used = 0;
    k = counts{};
    if (t.kind == ZKM_STEP_RAW && t.reads[0] >= A.nraw) return BAD_INDEX;
    if (const int code = count(t, k); code != OK) {
        k = counts{};
        return code;
    }
    if (t.kind == ZKM_STEP_RAW) {
        const uint64_t* ch = A.raw + (size_t)t.reads[0] * CPU_W + C_CH0;
        for (unsigned c = 0; c < NUM_GP_CHANNELS; c++) used |= (uint32_t)(gl_canon(ch[6 * c]) != 0) << c;
        if (used != t.reads[1]) {
            k = counts{};
            return BAD_MASK;
        }
    }
    return OK;
}

__global__ __launch_bounds__(BLOCK) void k_steps_walk(zkm_seg_args<walk_seg> S) {
    __shared__ uint32_t wave_sum[BLOCK / 64];
    const walk_seg& A = S.v[blockIdx.z];
    if ((size_t)blockIdx.x * BLOCK >= A.nsteps) return;
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    counts k;
    uint32_t used;
    int code = OK;
    if (i < A.nsteps) code = judge(load_step(A.steps + i), A, k, used);
    // the lowest refused step of the wave: lanes are consecutive steps
    const unsigned long long bad = __ballot(code != OK);
    if (bad && lane == 0) atomicMin(&A.verdict->first_bad, (uint32_t)(i + (unsigned)__ffsll(bad) - 1));
    uint32_t x = k.nmem | (k.nlogic << 12) | (k.narith << 22);   // 256 steps: at most 2048, 256, 256 (as k_cpu_steps packs them)
#pragma unroll
    for (unsigned d = 32; d; d >>= 1) x += __shfl_down(x, d);
    if (lane == 0) wave_sum[wave] = x;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
        for (unsigned w = 0; w < BLOCK / 64; w++) s += wave_sum[w];
        uint32_t* b = A.base + 3 * (size_t)blockIdx.x;
        b[0] = s & 0xFFF; b[1] = (s >> 12) & 0x3FF; b[2] = s >> 22;
    }
}

__global__ __launch_bounds__(BLOCK) void k_steps_scan(zkm_seg_args<walk_seg> S) {
    __shared__ uint32_t sh[SCAN_WAVES];
    const walk_seg& A = S.v[blockIdx.z];
    const size_t nblk = (A.nsteps + BLOCK - 1) / BLOCK;
    uint32_t carry[3] = {0, 0, 0};   // (2^28 steps: at most 2^31 memory operations)
    for (size_t c = 0; c < nblk; c += BLOCK) {
        const size_t t = c + threadIdx.x;
#pragma unroll
        for (unsigned j = 0; j < 3; j++) {
            const uint32_t x = t < nblk ? A.base[3 * t + j] : 0;
            uint32_t all;
            const uint32_t incl = block_incl_scan(x, sh, add_u32(), &all);
            if (t < nblk) A.base[3 * t + j] = carry[j] + incl - x;
            carry[j] += all;
        }
    }
    if (threadIdx.x) return;
    steps_verdict* v = A.verdict;
    for (unsigned j = 0; j < 3; j++) v->total[j] = carry[j];
    const uint32_t i = v->first_bad;
    if (i >= A.nsteps) return;   // (all ones: no step was refused)
    const zkm_cpu_step t = load_step(A.steps + i);
    counts k;
    uint32_t used;
    v->code = (uint32_t)judge(t, A, k, used);
    v->used = used;
    v->pad = 0;
    v->step = t;
}

size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// ---- the refusals that need no device, in the order the header gives them
void check_lists(const std::string& what, size_t nseg, const zkm_cpu_steps* steps) {
    if (!steps) throw std::runtime_error(what + ": null argument");
    if (nseg == 0) throw std::runtime_error(what + ": no segments");
    for (size_t s = 0; s < nseg; s++) {
        const std::string at = what + ": segment " + std::to_string(s) + ": ";
        if ((steps[s].nsteps && !steps[s].steps) || (steps[s].nraw && !steps[s].raw_rows)) throw std::runtime_error(at + "null pointer with a nonzero count");
        if (steps[s].nsteps > MAX_STEPS) throw std::runtime_error(at + std::to_string(steps[s].nsteps) + " steps, more than 2^28");
    }
}

// ---- one device block for all segments: the verdicts, every segment's triples (contiguous behind them: one download serves both), then
// the records and the ready-made rows that are copied.  own_steps: the records are copied wherever they lie (the block's owner hands
// out pointers into it); otherwise records in device memory are read in place.  Ready-made rows in device memory are never copied.
struct walk_plan {
    struct part { size_t base, steps, raw; bool copy_steps, copy_raw; };
    std::vector<part> parts;
    size_t head = 0, bytes = 0;   // head: the verdicts and the triples
    walk_plan(size_t nseg, const zkm_cpu_steps* st, bool own_steps) : parts(nseg) {
        size_t at = up256(nseg * sizeof(steps_verdict));
        for (size_t s = 0; s < nseg; s++) {
            parts[s].base = at;
            at += up256(3 * 4 * ((st[s].nsteps + BLOCK - 1) / BLOCK));
        }
        head = at;
        for (size_t s = 0; s < nseg; s++) {
            part& p = parts[s];
            p.copy_steps = st[s].nsteps && (own_steps || !zkm_is_device_ptr(st[s].steps));
            p.copy_raw = st[s].nraw && !zkm_is_device_ptr(st[s].raw_rows);
            p.steps = at;
            at += up256(p.copy_steps ? st[s].nsteps * sizeof(zkm_cpu_step) : 0);
            p.raw = at;
            at += up256(p.copy_raw ? st[s].nraw * CPU_W * 8 : 0);
        }
        bytes = at;
    }
    // the segment as the kernels read it
    walk_seg seg(char* sb, const zkm_cpu_steps& st, size_t s) const {
        const part& p = parts[s];
        return walk_seg{p.copy_steps ? (const zkm_cpu_step*)(sb + p.steps) : st.steps, p.copy_raw ? (const uint64_t*)(sb + p.raw) : st.raw_rows, st.nsteps,
                        st.nraw, (uint32_t*)(sb + p.base), (steps_verdict*)sb + s};
    }
};

// the copies (records on `up`, rows on `up2`) and, behind both, the walk's launches on `up`
void queue_walk(zkm_ctx* c, hipStream_t up, hipStream_t up2, const walk_plan& P, char* sb, const zkm_cpu_steps* st, size_t nseg) {
    ZKM_HIP_CHECK(hipMemsetAsync(sb, 0xFF, nseg * sizeof(steps_verdict), up));
    bool rows = false;
    for (size_t s = 0; s < nseg; s++) {
        const walk_plan::part& p = P.parts[s];
        if (p.copy_steps) ZKM_HIP_CHECK(hipMemcpyAsync(sb + p.steps, st[s].steps, st[s].nsteps * sizeof(zkm_cpu_step), hipMemcpyDefault, up));
        if (p.copy_raw) ZKM_HIP_CHECK(hipMemcpyAsync(sb + p.raw, st[s].raw_rows, st[s].nraw * CPU_W * 8, hipMemcpyHostToDevice, up2));
        rows = rows || p.copy_raw;
    }
    if (rows && up2 != up) {
        const zkm_event e(c);
        e.record(up2);
        ZKM_HIP_CHECK(hipStreamWaitEvent(up, e.e, 0));
    }
    std::unique_ptr<zkm_prof_scope> ps;
    if (up == c->stream) ps.reset(new zkm_prof_scope(c, "cpu_steps/walk"));   // (a scope is a pair of events on the compute stream)
    for (size_t s0 = 0; s0 < nseg; s0 += ZKM_MAX_SEG) {
        const size_t k = std::min<size_t>(ZKM_MAX_SEG, nseg - s0);
        walk_seg segs[ZKM_MAX_SEG];
        size_t most = 0;
        for (size_t s = 0; s < k; s++) {
            segs[s] = P.seg(sb, st[s0 + s], s0 + s);
            most = std::max(most, segs[s].nsteps);
        }
        zkm_launch_segs(up, k_steps_walk, segs, k, (most + BLOCK - 1) / BLOCK, BLOCK);
        zkm_launch_segs(up, k_steps_scan, segs, k, 1, BLOCK);
    }
}

// a segment's verdict as the host reads it: the counts, or the host walk's message
std::string read_verdict(const steps_verdict& v, const zkm_cpu_steps& st, zkm_steps_counts_t* n) {
    if (v.first_bad < st.nsteps) return zkm_cpu_step_refusal(v.first_bad, v.step, st.nraw, (int)v.code, v.used);
    *n = zkm_steps_counts_t{(size_t)v.total[0], (size_t)v.total[1], (size_t)v.total[2]};
    return std::string();
}

}  // namespace

// ---- steps staged ahead of a call.  The handle owns the block, the pinned words the verdicts come down into and the fence; the
// registry maps each segment's device `steps` pointer to its handle, which is how the builder knows a staged segment.
struct zkm_staged_steps {
    zkm_ctx* ctx = nullptr;
    zkm_scratch block;
    struct seg {
        zkm_cpu_steps dev{};
        const uint32_t* base = nullptr;
        zkm_steps_counts_t n;
        std::string refusal;
    };
    std::vector<seg> segs;
    zkm_pinned<steps_verdict> verdicts;
    zkm_copy_fence fence;                // the work on the two copy streams (behind the block and the pinned words: it has waited when they go)
    bool resolved = false;               // the host has waited for the fence and read the verdicts
    ~zkm_staged_steps();
};

namespace {

std::mutex g_steps_mu;
std::map<const void*, std::pair<zkm_staged_steps*, size_t>> g_staged_steps;   // a segment's device records -> its handle and position

// the host's one wait for a handle
void resolve(zkm_staged_steps* h) {
    if (h->resolved) return;
    h->ctx->host_waits++;
    if (h->fence.ready(true) < 0) throw std::runtime_error("zkm_staged_steps: the wait for the staged walk failed");
    for (size_t s = 0; s < h->segs.size(); s++) h->segs[s].refusal = read_verdict(h->verdicts.p[s], h->segs[s].dev, &h->segs[s].n);
    h->resolved = true;
}

}  // namespace

zkm_staged_steps::~zkm_staged_steps() {
    std::lock_guard<std::mutex> lk(g_steps_mu);
    for (const seg& s : segs) {
        const auto it = g_staged_steps.find(s.dev.steps);
        if (it != g_staged_steps.end() && it->second.first == this) g_staged_steps.erase(it);
    }
}

bool zkm_staged_steps_find(const void* d_steps, zkm_staged_steps_ref* out) {
    zkm_staged_steps* h = nullptr;
    size_t s = 0;
    {
        std::lock_guard<std::mutex> lk(g_steps_mu);
        const auto it = d_steps ? g_staged_steps.find(d_steps) : g_staged_steps.end();
        if (it == g_staged_steps.end()) return false;
        h = it->second.first;
        s = it->second.second;
    }
    zkm_staged_steps_at(h, s, out);
    return true;
}

void zkm_staged_steps_at(zkm_staged_steps* h, size_t s, zkm_staged_steps_ref* out) {
    resolve(h);
    out->ctx = h->ctx;
    out->dev = h->segs[s].dev;
    out->n = h->segs[s].n;
    out->base = h->segs[s].base;
    out->refusal = h->segs[s].refusal;
    out->done[0] = h->fence.event(0);
    out->done[1] = h->fence.event(1);
}

void zkm_staged_steps_join(zkm_staged_steps* h) { h->fence.join(); }

extern "C" {

int zkm_cpu_steps_scan(zkm_ctx* c, size_t nseg, const zkm_cpu_steps* steps, size_t* counts_out, uint32_t* const* base_out, char** err) {
    return zkm_api("zkm_cpu_steps_scan", err, [&] {
        const std::string what = "zkm_cpu_steps_scan";
        check_lists(what, nseg, steps);
        if (!counts_out || !c) throw std::runtime_error(what + ": null argument");
        ZKM_HIP_CHECK(hipSetDevice(c->device));
        const walk_plan P(nseg, steps, false);
        zkm_scratch block(c, P.bytes);
        char* sb = block.as<char>();
        queue_walk(c, c->stream, c->stream, P, sb, steps, nseg);
        std::vector<char> head(P.head);
        ZKM_HIP_CHECK(hipMemcpyAsync(head.data(), sb, P.head, hipMemcpyDeviceToHost, c->stream));
        c->sync();   // (the block and the caller's lists are in use until here)
        for (size_t s = 0; s < nseg; s++) {
            steps_verdict v;
            memcpy(&v, head.data() + s * sizeof v, sizeof v);
            zkm_steps_counts_t n;
            if (const std::string m = read_verdict(v, steps[s], &n); !m.empty()) throw std::runtime_error(what + ": segment " + std::to_string(s) + ": " + m);
            counts_out[3 * s] = n.mem; counts_out[3 * s + 1] = n.logic; counts_out[3 * s + 2] = n.arith;
        }
        for (size_t s = 0; s < nseg && base_out; s++)
            if (base_out[s]) memcpy(base_out[s], head.data() + P.parts[s].base, 3 * 4 * ((steps[s].nsteps + BLOCK - 1) / BLOCK));
    });
}

int zkm_cpu_steps_stage(zkm_ctx* c, size_t nseg, const zkm_cpu_steps* steps, void** out, char** err) {
    return zkm_api("zkm_cpu_steps_stage", err, [&] {
        const std::string what = "zkm_cpu_steps_stage";
        check_lists(what, nseg, steps);
        if (!out || !c) throw std::runtime_error(what + ": null argument");
        ZKM_HIP_CHECK(hipSetDevice(c->device));
        *out = zkm_steps_stage_queue(c, nseg, steps, true);
    });
}

}  // extern "C"

zkm_staged_steps* zkm_steps_stage_queue(zkm_ctx* c, size_t nseg, const zkm_cpu_steps* steps, bool own_steps) {
    std::unique_ptr<zkm_staged_steps> h(new zkm_staged_steps());
    h->ctx = c;
    const walk_plan P(nseg, steps, own_steps);
    h->verdicts.alloc(nseg);
    h->block = zkm_scratch(c, P.bytes);
    char* sb = h->block.as<char>();
    h->segs.resize(nseg);
    for (size_t s = 0; s < nseg; s++) {
        const walk_seg w = P.seg(sb, steps[s], s);
        h->segs[s].dev = zkm_cpu_steps{steps[s].nsteps ? w.steps : nullptr, w.nsteps, w.nraw ? w.raw : nullptr, w.nraw};
        h->segs[s].base = w.base;
    }
    h->fence.begin(c);
    queue_walk(c, c->copy_stream, c->copy_stream2, P, sb, steps, nseg);
    ZKM_HIP_CHECK(hipMemcpyAsync(h->verdicts.p, sb, nseg * sizeof(steps_verdict), hipMemcpyDeviceToHost, c->copy_stream));
    h->fence.end();
    {
        std::lock_guard<std::mutex> lk(g_steps_mu);
        for (size_t s = 0; s < nseg; s++)
            if (h->segs[s].dev.steps) g_staged_steps[h->segs[s].dev.steps] = {h.get(), s};
    }
    return h.release();
}

extern "C" {

int zkm_staged_steps_ready(void* staged, int wait) {
    const zkm_staged_steps* h = (const zkm_staged_steps*)staged;
    return h ? h->fence.ready(wait != 0) : 1;
}

int zkm_staged_steps_get(void* staged, size_t segment, zkm_cpu_steps* steps_out, size_t* memory_ops, size_t* logic_ops, size_t* arithmetic_ops,
                         char** err) {
    return zkm_api("zkm_staged_steps_get", err, [&] {
        const std::string what = "zkm_staged_steps_get";
        zkm_staged_steps* h = (zkm_staged_steps*)staged;
        if (!h || !steps_out) throw std::runtime_error(what + ": null argument");
        if (segment >= h->segs.size())
            throw std::runtime_error(what + ": no segment " + std::to_string(segment) + ": the handle holds " + std::to_string(h->segs.size()));
        resolve(h);
        const zkm_staged_steps::seg& g = h->segs[segment];
        if (!g.refusal.empty()) throw std::runtime_error(what + ": segment " + std::to_string(segment) + ": " + g.refusal);
        h->fence.join();
        *steps_out = g.dev;
        if (memory_ops) *memory_ops = g.n.mem;
        if (logic_ops) *logic_ops = g.n.logic;
        if (arithmetic_ops) *arithmetic_ops = g.n.arith;
    });
}

void zkm_staged_steps_free(void* staged) {
    delete (zkm_staged_steps*)staged;   // (the fence waits for the walk before the block goes back)
}

}  // extern "C"
