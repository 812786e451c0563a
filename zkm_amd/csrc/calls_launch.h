// calls_launch.h -- what the four call expansions (sha_calls.hip, keccak_calls.hip, io_calls.hip, insn_rows.hip) and their composition
// (calls_entry.hip) share on the host: the K-segment launcher, the K = 1 tail of the per-kind entry points, a RAW record, and the small
// helpers of the refusals' texts.
//
// A kind serves K segments by ONE launch: the K descriptors travel in device memory, uploaded with the lists the host holds in one
// scratch block, as the bootstrap's do (d_desc); the kernel-argument block is one pointer (zkm_seg_desc).  The block's layout:
//   the K descriptors, rounded up to 256 bytes; then, in segment order and list order, every list that goes up, each rounded up to 256.
// A kind states what differs in a small struct K in its own file, next to its kernel:
//   job, args                         one segment's checked calls (zkm_internal.h "the calls' expansions"), the kernel's descriptor
//   name, scope                       the launcher's name in a refusal, the profiling scope of the launch
//   kernel, threads                   __global__ void (const args*), its workgroup size
//   lists(job)                        std::array of zkm_calls_list: the lists a descriptor points to, and which of them go up
//   make(job, dev)                    the descriptor, dev[i] being list i's address on the device
//   extent(job)                       the segment's own extent of the grid (workgroups)
//   sparse_rows(job)                  the rows the kernel stores only the set cells of (they have to be zero in front), 0 for a kernel
//                                     that writes every word
#pragma once
#include <array>
#include <tuple>

#include "zkm_internal.h"

namespace zkm_calls {

// ---- the refusals' texts, and the two sizes every kind uses
inline std::string dec(uint64_t v) { return std::to_string(v); }
inline std::string hex(uint64_t v) {
    char buf[24];
    snprintf(buf, sizeof buf, "0x%llx", (unsigned long long)v);
    return buf;
}
inline std::string hex8(uint32_t v) {
    char buf[16];
    snprintf(buf, sizeof buf, "0x%08x", v);
    return buf;
}
inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
constexpr uint64_t LIM = (uint64_t)1 << 32;   // what a 32-bit cell, address or RAW index stays below

// the record of a ready-made row for the step log: RAW row `index` with the used channels `mask`
GL_HD zkm_cpu_step raw_step(size_t index, uint32_t mask) {
    zkm_cpu_step s{};
    s.kind = ZKM_STEP_RAW;
    s.reads[0] = (uint32_t)index;
    s.reads[1] = mask;
    return s;
}

// counts_out of zkm_segment_calls_steps
enum { N_SHA_ROWS, N_KECCAK_ROWS, N_IO_ROWS, N_INSN_ROWS, N_RAW, N_MEM, N_LOGIC, N_ARITH, N_EXT, N_PERMS, N_ROW_MEM };
static_assert(N_ROW_MEM + 1 == ZKM_CALLS_COUNTS, "counts_out as the header lists it");

}  // namespace zkm_calls

// ---- one segment of the calls' composition (calls_entry.hip; calls_stage.hip queues the same plan on the copy streams)
struct zkm_calls_plan {
    size_t n[ZKM_CALLS_COUNTS] = {};
    zkm_sha_job sha;
    zkm_keccak_job keccak;
    zkm_io_job io;
    zkm_insn_job insn;
    // the eight lists of the segment's block: rows, memory, logic, ShaExtend inputs and timestamps, Keccak inputs and timestamps, arithmetic
    size_t own_bytes[8] = {}, bytes[8] = {}, at[8] = {}, total = 0;
    const void* own_src[8] = {};
};
// calls_entry.hip, each throwing the bare message: the refusals and counts that read the lists per call and never per row; the rest of
// the host's refusals, the jobs and the block's layout; the block bound to the jobs' outputs and to what the builder takes; and the
// text of the two refusals that need a row's clock, for the host's loop and the device's verdict alike
void zkm_calls_counts(const zkm_segment_calls& q, size_t n[ZKM_CALLS_COUNTS]);
void zkm_calls_plan_lists(const zkm_segment_calls& q, zkm_calls_plan& P);
void zkm_calls_bind(const zkm_segment_calls& q, zkm_calls_plan& p, char* b, char* list[8], zkm_segment_ops& o);
std::string zkm_calls_row_refusal(const zkm_segment_calls& q, const size_t n[ZKM_CALLS_COUNTS], size_t j, uint64_t clock);

// the host copies of the descriptors that uploads queued on a stream read: in use until the stream has been waited for
struct zkm_calls_hold {
    std::vector<std::unique_ptr<char[]>> blocks;
    template <class T> T* make(size_t n) {
        blocks.emplace_back(new char[n * sizeof(T) + 1]());
        return (T*)blocks.back().get();
    }
};

// one list a descriptor points to: `up` -- the host holds it, it goes up into the scratch block (an empty one takes no room there)
struct zkm_calls_list { const void* p; size_t bytes; bool up; };

// The bytes a launch of these jobs puts up; at (nseg x the kind's lists, unless null): where each list lies in the block.
template <class K> size_t zkm_calls_layout(const typename K::job* j, size_t nseg, size_t* at) {
    size_t total = zkm_calls::up256(nseg * sizeof(typename K::args));
    for (size_t s = 0; s < nseg; s++)
        for (const zkm_calls_list& l : K::lists(j[s])) {
            if (at) *at++ = total;
            if (l.up) total += zkm_calls::up256(l.bytes);
        }
    return total;
}

// Queues the uploads into `sb` (zkm_calls_layout bytes) and ONE launch for nseg <= ZKM_MAX_SEG checked jobs; no launch when no job has
// an item.  zero_rows queues a memset of each job's sparse rows in front (false: the caller has zeroed them).  The jobs, `hold` and
// the caller's lists are in use until the stream has been waited for.  `st`: the stream everything is queued on -- the context's
// compute stream for the kinds' entry points and zkm_segments_calls_expand, a copy stream for a staged call (calls_stage.hip; the
// profiling scope is a pair of events on the compute stream, so only a launch there has one).
template <class K>
void zkm_calls_queue(zkm_ctx* c, hipStream_t st, const typename K::job* j, size_t nseg, char* sb, zkm_calls_hold& hold, bool zero_rows) {
    using Args = typename K::args;
    constexpr size_t NL = std::tuple_size<decltype(K::lists(*j))>::value;
    if (nseg == 0 || nseg > ZKM_MAX_SEG) throw std::runtime_error(std::string(K::name) + ": segment count out of range");
    std::vector<size_t> at(nseg * NL);
    zkm_calls_layout<K>(j, nseg, at.data());
    Args* d = hold.make<Args>(nseg);
    size_t grid = 0;
    for (size_t s = 0; s < nseg; s++) {
        const auto in = K::lists(j[s]);
        const void* dev[NL];
        for (size_t i = 0; i < NL; i++) {
            dev[i] = in[i].p;
            if (!in[i].up) continue;
            dev[i] = sb + at[s * NL + i];
            if (in[i].bytes) ZKM_HIP_CHECK(hipMemcpyAsync((void*)dev[i], in[i].p, in[i].bytes, hipMemcpyHostToDevice, st));
        }
        if (zero_rows && K::sparse_rows(j[s]))
            ZKM_HIP_CHECK(hipMemsetAsync(j[s].rows, 0, K::sparse_rows(j[s]) * ZKM_CPU_COLS * sizeof(uint64_t), st));
        d[s] = K::make(j[s], dev);
        grid = std::max(grid, K::extent(j[s]));
    }
    if (!grid) return;
    ZKM_HIP_CHECK(hipMemcpyAsync(sb, d, nseg * sizeof(Args), hipMemcpyHostToDevice, st));
    std::unique_ptr<zkm_prof_scope> ps;
    if (st == c->stream) ps.reset(new zkm_prof_scope(c, K::scope));
    hipLaunchKernelGGL(K::kernel, dim3((unsigned)grid, 1, (unsigned)nseg), dim3(K::threads), 0, st, (const Args*)sb);
    ZKM_HIP_CHECK(hipGetLastError());
}

// The K = 1 tail of a kind's own entry point: one block for the descriptor and the lists the host holds, the launch, the host's wait.
template <class K> void zkm_calls_one(zkm_ctx* c, const typename K::job& j) {
    // `hold` is declared in front of the block: when an exception unwinds, the block's owner waits for the stream before it releases
    // the block, and the uploads queued there still read the descriptors' host copy
    zkm_calls_hold hold;
    zkm_scratch block(c, zkm_calls_layout<K>(&j, 1, nullptr));
    zkm_calls_queue<K>(c, c->stream, &j, 1, block.as<char>(), hold, true);
    c->sync();   // (the block, the job and the caller's lists are in use until here)
}
