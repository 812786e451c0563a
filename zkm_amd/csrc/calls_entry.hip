// calls_entry.hip -- K segments' calls expanded in one set of launches behind one C entry (include/zkm_hip.h "K segments' calls expanded
// in one set of launches"): the composition of the four expansions -- sha_calls.hip, keccak_calls.hip, io_calls.hip, insn_rows.hip -- that
// a caller of several kinds needs: which RAW index each generated row gets, where its record goes in the step list, one run per list with
// the segment's own items in front, and which groups of zkm_segment_ops the calls set.
//
// The host half (zkm_segment_calls_steps) is built from the four zkm_*_steps / zkm_*_counts entry points and restates none of them.  The
// device half is a stage in FRONT of the builder (segment_ops.hip is not touched): per group of up to ZKM_MAX_SEG segments one scratch
// block for every list the host holds and the kernels' descriptors, one launch per kind through the kinds' own K-segment launchers
// (zkm_internal.h "the calls' expansions": each an instantiation of the one launcher in calls_launch.h), one host wait.  A segment's rows
// and lists live in ONE block of the context's allocator, each list in a run of its own (256-byte aligned): own items in front, the
// generated ones behind in the order SHA, Keccak, I/O, instructions.
#include "calls_launch.h"

namespace {

using namespace zkm_calls;
constexpr size_t CPU_W = ZKM_CPU_COLS;

// a pure entry point of the library, its failure as an exception with its message
template <class F> void must(F&& call) {
    char* e = nullptr;
    if (call(&e) == 0) return;
    const std::string m = e ? e : "error";
    free(e);
    throw std::runtime_error(m);
}

void host_list(const void* p, size_t n, const char* name) {
    if (n && !p) throw std::runtime_error(std::string(name) + ": NULL with a count of " + dec(n));
    if (n && zkm_is_device_ptr(p)) throw std::runtime_error(std::string(name) + ": device memory (the list is read on the host)");
}

}  // namespace

// The host half for one segment that reads the lists PER CALL and never per row: every refusal that concerns where the lists lie and
// `own` (throws the bare message; the per-kind entry points' messages as they are), and the counts.
void zkm_calls_counts(const zkm_segment_calls& q, size_t n[ZKM_CALLS_COUNTS]) {
    const zkm_cpu_steps& st = q.steps;
    host_list(st.steps, st.nsteps, "steps.steps");
    if (st.nraw && !st.raw_rows) throw std::runtime_error("steps.raw_rows: NULL with a count of " + dec(st.nraw));
    if (st.nraw && zkm_is_device_ptr(st.raw_rows)) throw std::runtime_error("steps.raw_rows: device memory (the segment's own rows go up from host memory)");
    if (q.own.cpu_rows || q.own.ncpu_rows) throw std::runtime_error("own.cpu_rows: must be NULL with ncpu_rows 0 (the CPU rows are built from the steps)");
    const struct { const char* name; size_t n; } owned[5] = {{"sha_extend", q.own.nsha_extend}, {"sha_extend_sponge", q.own.nsha_extend_sponge},
                                                            {"sha_compress", q.own.nsha_compress}, {"sha_compress_sponge", q.own.nsha_compress_sponge},
                                                            {"keccak_sponge", q.own.nkeccak_sponge}};
    for (const auto& g : owned)
        if (g.n) throw std::runtime_error(std::string("own.") + g.name + ": " + dec(g.n) + " items, but the calls own this group (it must be empty)");
    host_list(q.extend_meta, q.nextend, "extend_meta");
    host_list(q.compress_meta, q.ncompress, "compress_meta");
    host_list(q.keccak_input_off, q.nkeccak, "keccak_input_off");
    host_list(q.keccak_meta, q.nkeccak, "keccak_meta");
    host_list(q.io_kinds, q.nio, "io_kinds");
    host_list(q.io_data_off, q.nio, "io_data_off");
    host_list(q.io_meta, q.nio, "io_meta");
    host_list(q.insns, q.ninsns, "insns");
    host_list(q.insn_clocks, q.ninsns, "insn_clocks");

    // the counts, from the kinds' own entry points
    size_t mem[4] = {}, logic[2] = {};
    std::fill(n, n + ZKM_CALLS_COUNTS, 0);
    zkm_sha_calls_counts(q.nextend, q.ncompress, &n[N_SHA_ROWS], &mem[0], &logic[0], &n[N_EXT]);
    must([&](char** e) { return zkm_keccak_calls_counts_meta(q.keccak_input_off, q.keccak_meta, q.nkeccak, &n[N_KECCAK_ROWS], &mem[1], &logic[1], &n[N_PERMS], e); });
    must([&](char** e) { return zkm_io_calls_counts(q.io_kinds, q.io_data_off, q.nio, &n[N_IO_ROWS], &mem[2], e); });
    must([&](char** e) { return zkm_insn_rows_counts(q.insns, q.ninsns, &mem[3], &n[N_ARITH], e); });
    n[N_INSN_ROWS] = q.ninsns;
    const size_t rows = n[N_SHA_ROWS] + n[N_KECCAK_ROWS] + n[N_IO_ROWS] + n[N_INSN_ROWS];
    n[N_RAW] = st.nraw + rows;
    n[N_MEM] = mem[0] + mem[1];
    n[N_LOGIC] = logic[0] + logic[1];
    n[N_ROW_MEM] = mem[2] + mem[3];
}

// a generated row as a refusal names it: its kind, its position among the kind's rows, its clock
static std::string zkm_calls_describe_row(const size_t n[ZKM_CALLS_COUNTS], size_t j, uint64_t clock) {
    const size_t kind_end[4] = {n[N_SHA_ROWS], n[N_SHA_ROWS] + n[N_KECCAK_ROWS], n[N_SHA_ROWS] + n[N_KECCAK_ROWS] + n[N_IO_ROWS], (size_t)-1};
    const char* const kind_name[4] = {"SHA call", "Keccak call", "I/O call", "instruction record"};
    int k = 0;
    while (j >= kind_end[k]) k++;
    return std::string(kind_name[k]) + " row " + dec(j - (k ? kind_end[k - 1] : 0)) + " (clock " + dec(clock) + ")";
}
// the two refusals that need a row's clock, in one wording for the host loop below and the device's verdicts (calls_stage.hip)
std::string zkm_calls_row_refusal(const zkm_segment_calls& q, const size_t n[ZKM_CALLS_COUNTS], size_t j, uint64_t clock) {
    const std::string row = zkm_calls_describe_row(n, j, clock);
    if (clock < q.first_clock || clock - q.first_clock >= q.steps.nsteps)
        return row + " lies outside the step list (first_clock " + dec(q.first_clock) + ", " + dec(q.steps.nsteps) + " steps)";
    return row + ": two records on one clock";
}

namespace {

// The whole host half for one segment: zkm_calls_counts, then PER ROW the records, their clocks and the two refusals that need them,
// and the patched list into `out` (nsteps records) unless it is null.
void calls_steps(const zkm_segment_calls& q, zkm_cpu_step* out, size_t counts[ZKM_CALLS_COUNTS]) {
    const zkm_cpu_steps& st = q.steps;
    size_t n[ZKM_CALLS_COUNTS];
    zkm_calls_counts(q, n);
    const size_t rows = n[N_SHA_ROWS] + n[N_KECCAK_ROWS] + n[N_IO_ROWS] + n[N_INSN_ROWS];

    // the records and their clocks, kind by kind with the running raw_base
    std::vector<zkm_cpu_step> rec(rows);
    std::vector<uint64_t> clk(rows);
    size_t at = 0;
    must([&](char** e) {
        return zkm_sha_calls_steps(q.extend_meta, q.nextend, q.compress_meta, q.ncompress, st.nraw + at, rec.data() + at, clk.data() + at, e);
    });
    at += n[N_SHA_ROWS];
    must([&](char** e) { return zkm_keccak_calls_steps(q.keccak_input_off, q.keccak_meta, q.nkeccak, st.nraw + at, rec.data() + at, clk.data() + at, e); });
    at += n[N_KECCAK_ROWS];
    must([&](char** e) { return zkm_io_calls_steps(q.io_kinds, q.io_data_off, q.io_meta, q.nio, st.nraw + at, rec.data() + at, clk.data() + at, e); });
    at += n[N_IO_ROWS];
    must([&](char** e) { return zkm_insn_rows_steps(q.insns, q.ninsns, st.nraw + at, rec.data() + at, e); });
    std::copy(q.insn_clocks, q.insn_clocks + q.ninsns, clk.begin() + at);

    // where each record goes: clock - first_clock, inside the list, one record a clock
    std::vector<bool> taken(st.nsteps, false);
    for (size_t j = 0; j < rows; j++) {
        const bool outside = clk[j] < q.first_clock || clk[j] - q.first_clock >= st.nsteps;
        if (outside || taken[clk[j] - q.first_clock]) throw std::runtime_error(zkm_calls_row_refusal(q, n, j, clk[j]));
        taken[clk[j] - q.first_clock] = true;
    }
    if (out) {
        std::copy(st.steps, st.steps + st.nsteps, out);
        for (size_t j = 0; j < rows; j++) out[clk[j] - q.first_clock] = rec[j];
    }
    if (counts) std::copy(n, n + ZKM_CALLS_COUNTS, counts);
}

using seg_plan = zkm_calls_plan;

void own_list(const void* p, size_t n, const char* name) {
    if (n && !p) throw std::runtime_error(std::string("own.") + name + ": NULL with a count of " + dec(n));
}

}  // namespace

// The rest of a segment's refusals (P.n is zkm_calls_counts'): the `own` lists, the four kinds' checks of their calls -- which fill the
// jobs, without outputs -- and the layout of the segment's block.
void zkm_calls_plan_lists(const zkm_segment_calls& q, zkm_calls_plan& P) {
    own_list(q.own.memory_ops, q.own.nmemory, "memory_ops");
    own_list(q.own.logic_ops, q.own.nlogic, "logic_ops");
    own_list(q.own.arithmetic_ops, q.own.narithmetic, "arithmetic_ops");
    own_list(q.own.keccak_inputs, q.own.nkeccak, "keccak_inputs");
    own_list(q.own.keccak_timestamps, q.own.nkeccak, "keccak_timestamps");
    P.sha.w16 = q.extend_w16, P.sha.emeta = q.extend_meta, P.sha.E = q.nextend;
    P.sha.hx = q.compress_hx, P.sha.w = q.compress_w, P.sha.cmeta = q.compress_meta, P.sha.C = q.ncompress;
    zkm_sha_calls_check(P.sha);
    P.keccak.inputs = q.keccak_inputs, P.keccak.off = q.keccak_input_off, P.keccak.meta = q.keccak_meta, P.keccak.digest_addrs = q.keccak_digest_addrs;
    P.keccak.n = q.nkeccak;
    zkm_keccak_calls_check(P.keccak);
    P.io.kinds = q.io_kinds, P.io.data = q.io_data, P.io.off = q.io_data_off, P.io.meta = q.io_meta, P.io.n = q.nio;
    zkm_io_calls_check(P.io);
    P.insn.insns = q.insns, P.insn.clocks = q.insn_clocks, P.insn.n = q.ninsns;
    zkm_insn_rows_check(P.insn);
    const size_t* n = P.n;
    const size_t gen_rows = n[N_RAW] - q.steps.nraw;
    const size_t own_b[8] = {q.steps.nraw * CPU_W * 8, q.own.nmemory * 48, q.own.nlogic * 12, 0, 0, q.own.nkeccak * 200, q.own.nkeccak * 8,
                             q.ninsns ? q.own.narithmetic * 12 : 0};
    const size_t gen_b[8] = {gen_rows * CPU_W * 8, n[N_MEM] * 48, n[N_LOGIC] * 12, n[N_EXT] * 16, n[N_EXT] * 8, n[N_PERMS] * 200, n[N_PERMS] * 8,
                             q.ninsns ? n[N_ARITH] * 12 : 0};
    const void* src[8] = {q.steps.raw_rows, q.own.memory_ops, q.own.logic_ops, nullptr, nullptr, q.own.keccak_inputs, q.own.keccak_timestamps,
                          q.own.arithmetic_ops};
    P.total = 0;
    for (int i = 0; i < 8; i++) {
        P.own_bytes[i] = own_b[i], P.bytes[i] = own_b[i] + gen_b[i], P.own_src[i] = src[i];
        P.at[i] = P.total;
        P.total += up256(P.bytes[i]);
    }
}

// The planned segment's block at `b` (P.total bytes; null when that is 0): where the jobs write, and what the builder takes -- `own`
// with the joined lists and the calls' groups, the latter pointing at the CALLER's call lists.  list[i]: where list i starts (null when
// it is empty); the segment's own part of it, P.own_bytes[i] from P.own_src[i], is the caller's to copy there.
void zkm_calls_bind(const zkm_segment_calls& q, zkm_calls_plan& p, char* b, char* list[8], zkm_segment_ops& o) {
    for (int i = 0; i < 8; i++) list[i] = p.bytes[i] ? b + p.at[i] : nullptr;
    const size_t* n = p.n;
    // the rows behind the segment's own: the SHA calls', the Keccak calls', the I/O calls', the instructions'
    uint64_t* rows = (uint64_t*)list[0] + q.steps.nraw * CPU_W;
    p.sha.rows = rows;
    p.keccak.rows = rows + n[N_SHA_ROWS] * CPU_W;
    p.io.rows = p.keccak.rows + n[N_KECCAK_ROWS] * CPU_W;
    p.insn.rows = p.io.rows + n[N_IO_ROWS] * CPU_W;
    // the lists behind the segment's own: the SHA calls' items, then the Keccak calls'
    p.sha.mem = (uint64_t*)list[1] + 6 * q.own.nmemory;
    p.keccak.mem = p.sha.mem + 6 * p.sha.nmem;
    p.sha.logic = (uint32_t*)list[2] + 3 * q.own.nlogic;
    p.keccak.logic = p.sha.logic + 3 * p.sha.nlogic;
    p.sha.ext_in = (uint32_t*)list[3], p.sha.ext_ts = (uint64_t*)list[4];
    p.keccak.perm_in = (uint64_t*)list[5] + 25 * q.own.nkeccak, p.keccak.perm_ts = (uint64_t*)list[6] + q.own.nkeccak;
    p.insn.arith = list[7] ? (uint32_t*)list[7] + 3 * q.own.narithmetic : nullptr;
    o = q.own;
    o.memory_ops = (const uint64_t*)list[1], o.nmemory = q.own.nmemory + n[N_MEM];
    o.logic_ops = (const uint32_t*)list[2], o.nlogic = q.own.nlogic + n[N_LOGIC];
    if (q.ninsns) o.arithmetic_ops = (const uint32_t*)list[7], o.narithmetic = q.own.narithmetic + n[N_ARITH];
    o.keccak_inputs = (const uint64_t*)list[5], o.keccak_timestamps = (const uint64_t*)list[6], o.nkeccak = q.own.nkeccak + n[N_PERMS];
    o.sha_extend_inputs = (const uint8_t*)list[3], o.sha_extend_timestamps = (const uint64_t*)list[4], o.nsha_extend = n[N_EXT];
    o.sha_extend_sponge_w16 = q.extend_w16, o.sha_extend_sponge_meta = q.extend_meta, o.nsha_extend_sponge = q.nextend;
    o.sha_compress_hx = o.sha_compress_sponge_hx = q.compress_hx;
    o.sha_compress_w = o.sha_compress_sponge_w = q.compress_w;
    o.sha_compress_meta = o.sha_compress_sponge_meta = q.compress_meta;
    o.nsha_compress = o.nsha_compress_sponge = q.ncompress;
    o.keccak_sponge_inputs = q.keccak_inputs, o.keccak_sponge_off = q.keccak_input_off, o.keccak_sponge_meta = q.keccak_meta;
    o.nkeccak_sponge = q.nkeccak;
}

struct zkm_expanded_calls {
    zkm_ctx* c = nullptr;
    struct seg {
        std::vector<zkm_cpu_step> steps;
        zkm_cpu_steps st{};
        zkm_segment_ops ops{};
    };
    std::vector<seg> segs;
    std::vector<void*> blocks;
    zkm_expanded_calls() = default;
    zkm_expanded_calls(const zkm_expanded_calls&) = delete;
    ~zkm_expanded_calls() {
        for (void* p : blocks) c->release(p);
    }
};

namespace {

// every refusal of one segment, on the host; fills the patched list, the jobs (without outputs) and the block's layout
void plan_segment(const zkm_segment_calls& q, zkm_expanded_calls::seg& out, seg_plan& P) {
    out.steps.resize(q.steps.nsteps);
    calls_steps(q, out.steps.data(), P.n);
    zkm_calls_plan_lists(q, P);
}

// the device half for one group of <= ZKM_MAX_SEG planned segments: blocks, uploads, one launch a kind, one host wait
void expand_group(zkm_ctx* c, const zkm_segment_calls* calls, zkm_expanded_calls* h, seg_plan* P, size_t first, size_t nseg) {
    std::vector<zkm_sha_job> sha(nseg);
    std::vector<zkm_keccak_job> keccak(nseg);
    std::vector<zkm_io_job> io(nseg);
    std::vector<zkm_insn_job> insn(nseg);
    for (size_t s = 0; s < nseg; s++) {
        seg_plan& p = P[first + s];
        const zkm_segment_calls& q = calls[first + s];
        zkm_expanded_calls::seg& out = h->segs[first + s];
        char* b = nullptr;
        if (p.total) {
            h->blocks.reserve(h->blocks.size() + 1);   // (push_back cannot throw once the block exists)
            h->blocks.push_back(b = (char*)c->alloc(p.total));
        }
        char* list[8];
        zkm_calls_bind(q, p, b, list, out.ops);
        for (int i = 0; i < 8; i++)
            if (p.own_bytes[i]) ZKM_HIP_CHECK(hipMemcpyAsync(list[i], p.own_src[i], p.own_bytes[i], hipMemcpyDefault, c->stream));
        const size_t* n = p.n;
        // the SHA and Keccak kernels store only the cells a row sets: their rows, adjacent, are zeroed by one memset a segment
        if (n[N_SHA_ROWS] + n[N_KECCAK_ROWS])
            ZKM_HIP_CHECK(hipMemsetAsync(p.sha.rows, 0, (n[N_SHA_ROWS] + n[N_KECCAK_ROWS]) * CPU_W * 8, c->stream));
        sha[s] = p.sha;
        keccak[s] = std::move(p.keccak);
        io[s] = std::move(p.io);
        insn[s] = std::move(p.insn);
        // what the builder takes: the patched list with the rows on the device, and the operations
        out.st = zkm_cpu_steps{out.steps.data(), out.steps.size(), (const uint64_t*)list[0], n[N_RAW]};
    }
    // ONE scratch block for every list the host holds, of every kind and segment, and the four sets of descriptors
    const size_t part[4] = {zkm_sha_calls_scratch(sha.data(), nseg), zkm_keccak_calls_scratch(keccak.data(), nseg),
                            zkm_io_calls_scratch(io.data(), nseg), zkm_insn_rows_scratch(insn.data(), nseg)};
    zkm_calls_hold hold;   // (declared first, like the jobs: they outlive the scratch block's wait for the stream when an exception unwinds)
    zkm_scratch scratch(c, part[0] + part[1] + part[2] + part[3]);
    char* sb = scratch.as<char>();
    zkm_sha_calls_launch(c, sha.data(), nseg, sb, hold, false);
    zkm_keccak_calls_launch(c, keccak.data(), nseg, sb + part[0], hold, false);
    zkm_io_calls_launch(c, io.data(), nseg, sb + part[0] + part[1], hold);
    zkm_insn_rows_launch(c, insn.data(), nseg, sb + part[0] + part[1] + part[2], hold);
    c->sync();   // (the scratch block, the jobs, the descriptors and the caller's lists are in use until here)
}

// the body of zkm_segments_calls_expand (throws; `what` names the entry point in a refusal)
// seg_base: position of segment 0 in the caller's larger call (the pool's groups; refusals only)
std::unique_ptr<zkm_expanded_calls> expand(const char* what, zkm_ctx* c, size_t nseg, const zkm_segment_calls* calls, size_t seg_base = 0) {
    if (nseg == 0 || !calls) throw std::runtime_error(std::string(what) + ": null argument or no segment");
    std::unique_ptr<zkm_expanded_calls> h(new zkm_expanded_calls);
    h->c = c;
    h->segs.resize(nseg);
    // every refusal of every segment first, on the host
    std::vector<seg_plan> P(nseg);
    for (size_t s = 0; s < nseg; s++) {
        try {
            plan_segment(calls[s], h->segs[s], P[s]);
        } catch (const std::exception& e) {
            throw std::runtime_error(std::string(what) + ": segment " + dec(seg_base + s) + ": " + e.what());
        }
    }
    if (!c) throw std::runtime_error(std::string(what) + ": null argument");
    ZKM_HIP_CHECK(hipSetDevice(c->device));
    try {
        for (size_t first = 0; first < nseg; first += ZKM_MAX_SEG) expand_group(c, calls, h.get(), P.data(), first, std::min<size_t>(ZKM_MAX_SEG, nseg - first));
    } catch (...) {
        (void)hipStreamSynchronize(c->stream);   // (the blocks the handle releases may be in use by queued work)
        throw;
    }
    return h;
}

// the steps and operations of every segment, as the builder's entry points take them
void outputs(const zkm_expanded_calls& h, std::vector<zkm_cpu_steps>* steps, std::vector<zkm_segment_ops>* ops) {
    for (const auto& s : h.segs) {
        steps->push_back(s.st);
        ops->push_back(s.ops);
    }
}

}  // namespace

extern "C" {

int zkm_segment_calls_steps(const zkm_segment_calls* calls, zkm_cpu_step* steps_out, size_t* counts_out, char** err) {
    return zkm_api("zkm_segment_calls_steps", err, [&] {
        if (!calls) throw std::runtime_error("zkm_segment_calls_steps: null argument");
        try {
            calls_steps(*calls, steps_out, counts_out);
        } catch (const std::exception& e) {
            throw std::runtime_error(std::string("zkm_segment_calls_steps: ") + e.what());
        }
    });
}

int zkm_segments_calls_expand(zkm_ctx* c, size_t nseg, const zkm_segment_calls* calls, zkm_expanded_calls** out, char** err) {
    return zkm_api("zkm_segments_calls_expand", err, [&] {
        if (!out) throw std::runtime_error("zkm_segments_calls_expand: null argument");
        *out = nullptr;
        *out = expand("zkm_segments_calls_expand", c, nseg, calls).release();
    });
}

int zkm_expanded_calls_get(const zkm_expanded_calls* h, size_t segment, zkm_cpu_steps* steps_out, zkm_segment_ops* ops_out) {
    if (!h || segment >= h->segs.size()) return 1;
    if (steps_out) *steps_out = h->segs[segment].st;
    if (ops_out) *ops_out = h->segs[segment].ops;
    return 0;
}

void zkm_expanded_calls_free(zkm_expanded_calls* h) { delete h; }

int zkm_segments_tables_calls(zkm_ctx* c, const zkm_stark_config* cfg, size_t nseg, const zkm_boot_image* images, const zkm_segment_calls* calls,
                              unsigned* log_n_out, zkm_staged** out, char** err) {
    return zkm_api("zkm_segments_tables_calls", err, [&] {
        const std::unique_ptr<zkm_expanded_calls> h = expand("zkm_segments_tables_calls", c, nseg, calls);
        std::vector<zkm_cpu_steps> steps;
        std::vector<zkm_segment_ops> ops;
        outputs(*h, &steps, &ops);
        return zkm_segments_tables_steps(c, cfg, nseg, images, steps.data(), ops.data(), log_n_out, out, err);
    });
}

int zkm_prove_segments_ops_calls(zkm_ctx* c, const zkm_stark_config* cfg, size_t nseg, const zkm_boot_image* images, const zkm_segment_calls* calls,
                                 const uint64_t* const* public_values, const size_t* npublic, uint64_t* const* proofs_out, size_t* proof_offsets_out,
                                 uint64_t* const* ctl_challenges_out, char** err) {
    return zkm_api("zkm_prove_segments_ops_calls", err, [&] {
        const std::unique_ptr<zkm_expanded_calls> h = expand("zkm_prove_segments_ops_calls", c, nseg, calls);
        std::vector<zkm_cpu_steps> steps;
        std::vector<zkm_segment_ops> ops;
        outputs(*h, &steps, &ops);
        return zkm_prove_segments_ops_steps(c, cfg, nseg, images, steps.data(), ops.data(), public_values, npublic, proofs_out, proof_offsets_out,
                                            ctl_challenges_out, err);
    });
}

}  // extern "C"

// (zkm_internal.h: a group of the pool's, expanded in the call -- the same three steps, every refusal under `what` and at seg_base + s)
int zkm_prove_segments_ops_calls_entry(const char* what, zkm_ctx* c, const zkm_stark_config* cfg, size_t nseg, const zkm_boot_image* images,
                                       const zkm_segment_calls* calls, const uint64_t* const* pub, const size_t* npub, uint64_t* const* proofs,
                                       size_t* offsets_out, uint64_t* const* challenges, char** err, size_t seg_base) {
    return zkm_api(what, err, [&] {
        const std::unique_ptr<zkm_expanded_calls> h = expand(what, c, nseg, calls, seg_base);
        std::vector<zkm_cpu_steps> steps;
        std::vector<zkm_segment_ops> ops;
        outputs(*h, &steps, &ops);
        return zkm_prove_segments_ops_steps_entry(what, c, cfg, nseg, images, steps.data(), ops.data(), pub, npub, proofs, offsets_out, challenges, err,
                                                  seg_base);
    });
}
