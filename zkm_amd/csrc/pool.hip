// pool.hip -- one process, many GPUs: a pool of contexts that proves the independent segments of a program side by side.
//
// The reference drives every segment of a program from ONE process: prove_single_seg_common / prove_multi_seg_common
// (prover/examples/utils/src/utils.rs:57-68, 105-133) loop over the segment files and call prove_with_traces
// (prover/src/prover.rs:130-232) for each.  Segments are independent proofs (no data-path collective), so the MI355X
// shape of that loop is a queue of lock-step groups served by one worker thread per context, `contexts_per_device` contexts on
// each device: every entry point of the library selects its context's device itself (hipSetDevice(c->device), core.hip), so the
// workers need nothing but their own context.  bench.py's process-per-GPU harness (zkm_amd/dist.py) stays what the scaling bench
// launches; this is what a Rust caller binds (integration/rust/prove_hip.rs prove_segments_multi_hip).
// A group is finished tables, raw operations, or segments as the emulator records them (zkm_pool_prove_segments_calls, at the end: the
// one entry whose workers keep their next group staged behind the current proofs).
//
// Host only: no kernel lives here.
#include <exception>
#include <mutex>
#include <thread>

#include "zkm_internal.h"

struct zkm_pool {
    std::vector<zkm_ctx*> ctxs;        // worker w's context
    std::vector<int> devices;          // ... and its device
    std::vector<size_t> last_worker, last_group;   // of the last call: who proved segment s, in which group
};

// The groups of one call: consecutive runs of at most `stack` segments, the same number of groups for every worker (the fewest that
// keeps a group within `stack`), sizes as even as the count allows -- 20 segments, 2 workers, stack 4 -> 4, 4, 3, 3, 3, 3
// (zkm_amd/dist.py chunk_segments is the same rule; tests/test_pool.py holds them against each other).
static std::vector<std::pair<size_t, size_t>> pool_groups(size_t nseg, size_t workers, size_t stack) {
    std::vector<std::pair<size_t, size_t>> g;   // (first segment, count)
    if (!nseg) return g;
    workers = std::max<size_t>(1, workers);
    stack = std::max<size_t>(1, stack);
    const size_t per_worker = (nseg + workers * stack - 1) / (workers * stack);
    const size_t ngroups = std::min(nseg, workers * per_worker);
    const size_t base = nseg / ngroups, extra = nseg % ngroups;
    for (size_t k = 0, s = 0; k < ngroups; k++) {
        const size_t size = base + (k < extra ? 1 : 0);
        g.emplace_back(s, size);
        s += size;
    }
    return g;
}

// The queue of one call: the groups, who takes the next one, the first failure (which stops the queue) and the record of who proved what.
struct pool_queue {
    zkm_pool* p;
    const std::vector<std::pair<size_t, size_t>> groups;
    std::mutex mu;
    size_t next = 0;
    std::string first_error;
    bool failed = false;
    pool_queue(zkm_pool* pool, std::vector<std::pair<size_t, size_t>> g) : p(pool), groups(std::move(g)) {}
    bool claim(size_t* g) {
        std::lock_guard<std::mutex> lk(mu);
        if (failed || next >= groups.size()) return false;
        *g = next++;
        return true;
    }
    bool stopped() {
        std::lock_guard<std::mutex> lk(mu);
        return failed;
    }
    // worker w is through with group g: proven (rc == 0) or refused with the entry point's message e, which is freed here
    void done(size_t w, size_t g, int rc, char* e) {
        const size_t s0 = groups[g].first, k = groups[g].second;
        std::lock_guard<std::mutex> lk(mu);
        if (rc != 0) {
            if (!failed)
                first_error = "worker " + std::to_string(w) + " (device " + std::to_string(p->devices[w]) + "), segments " + std::to_string(s0) + ".." +
                              std::to_string(s0 + k - 1) + ": " + (e ? e : "unknown error");
            failed = true;
        } else {
            for (size_t s = s0; s < s0 + k; s++) { p->last_worker[s] = w; p->last_group[s] = g; }
        }
        free(e);
    }
};

// (throws: the entry points below run it inside the error boundary)
// serve(worker, queue): what one worker thread does until the queue is empty or stopped; nothing unwinds out of it
template <class S>
static void pool_serve(const char* what, zkm_pool* p, size_t nseg, size_t max_stack, S&& serve) {
    if (max_stack == 0) max_stack = 8;
    if (max_stack > ZKM_MAX_SEG) throw std::runtime_error(std::string(what) + ": max_stack beyond " + std::to_string(ZKM_MAX_SEG));
    const size_t W = p->ctxs.size();
    pool_queue q(p, pool_groups(nseg, W, max_stack));
    p->last_worker.assign(nseg, ~(size_t)0);
    p->last_group.assign(nseg, ~(size_t)0);
    if (q.groups.empty()) return;
    auto worker = [&](size_t w) { serve(w, q); };
    // one thread per context that has work (a thread start is ~50 us; a group is milliseconds to seconds).  The calling thread is worker 0.
    const size_t nthreads = std::min(W, q.groups.size());
    std::vector<std::thread> th;
    try {
        for (size_t w = 1; w < nthreads; w++) th.emplace_back(worker, w);
    } catch (...) {
        // (a thread could not be started: the ones that run, and the calling thread below, drain the queue)
    }
    worker(0);
    for (auto& t : th) t.join();
    if (q.failed) throw std::runtime_error(q.first_error);
}

// run_group(context, first segment, count, err): ONE call of the entry point that proves the group on that worker's context
template <class G>
static void pool_run(const char* what, zkm_pool* p, size_t nseg, size_t max_stack, G&& run_group) {
    pool_serve(what, p, nseg, max_stack, [&](size_t w, pool_queue& q) {
        for (size_t g; q.claim(&g);) {
            char* e = nullptr;   // (the entry point is noexcept: nothing unwinds out of a worker thread)
            const int rc = run_group(p->ctxs[w], q.groups[g].first, q.groups[g].second, &e);
            q.done(w, g, rc, e);
        }
    });
}

static void pool_prove(const char* what, zkm_pool* p, const zkm_stark_config* cfg, size_t nseg, size_t max_stack,
                       const uint64_t* const* const* traces, const uint64_t* const* const* const* columns, const unsigned* const* log_n,
                       const uint64_t* const* pub, const size_t* npub, uint64_t* const* proofs, uint64_t* const* challenges) {
    if (!p || !cfg || (!traces && !columns) || !log_n || !proofs || !challenges) throw std::runtime_error(std::string(what) + ": null argument");
    pool_run(what, p, nseg, max_stack, [&](zkm_ctx* c, size_t s0, size_t k, char** e) {
        return zkm_prove_segments_entry(what, c, cfg, k, traces ? traces + s0 : nullptr, columns ? columns + s0 : nullptr, log_n + s0,
                                        pub ? pub + s0 : nullptr, npub ? npub + s0 : nullptr, proofs + s0, challenges + s0, e, s0);
    });
}

extern "C" {

int zkm_pool_create(const int* devices, size_t ndevices, size_t contexts_per_device, zkm_pool** out, char** err) {
    return zkm_api("zkm_pool_create", err, [&] {
        if (!out) throw std::runtime_error("zkm_pool_create: null argument");
        *out = nullptr;
        if (!devices || ndevices == 0 || contexts_per_device == 0) throw std::runtime_error("zkm_pool_create: at least one device and one context per device");
        if (ndevices > 64 || contexts_per_device > 64) throw std::runtime_error("zkm_pool_create: at most 64 devices x 64 contexts");
        for (size_t i = 0; i < ndevices; i++)
            for (size_t j = 0; j < i; j++)
                if (devices[i] == devices[j]) throw std::runtime_error("zkm_pool_create: device " + std::to_string(devices[i]) + " listed twice");
        std::unique_ptr<zkm_pool, void (*)(zkm_pool*)> p(new zkm_pool(), zkm_pool_destroy);
        p->ctxs.reserve(ndevices * contexts_per_device);    // (a context, once created, is in the pool: push_back cannot throw)
        p->devices.reserve(ndevices * contexts_per_device);
        // worker order: device-major round robin (worker w -> device w % ndevices), so the first `ndevices` groups of a call land on
        // different devices even when the call has fewer groups than workers
        for (size_t k = 0; k < contexts_per_device; k++)
            for (size_t d = 0; d < ndevices; d++) {
                zkm_ctx* c = nullptr;
                char* e = nullptr;
                if (zkm_ctx_create(devices[d], &c, &e) != 0) {
                    const std::string msg = "zkm_pool_create: context " + std::to_string(k) + " on device " + std::to_string(devices[d]) + ": " + (e ? e : "failed");
                    free(e);
                    throw std::runtime_error(msg);
                }
                p->ctxs.push_back(c);
                p->devices.push_back(devices[d]);
            }
        *out = p.release();
    });
}

void zkm_pool_destroy(zkm_pool* p) {
    if (!p) return;
    for (zkm_ctx* c : p->ctxs) zkm_ctx_destroy(c);
    delete p;
}

size_t zkm_pool_workers(const zkm_pool* p) { return p ? p->ctxs.size() : 0; }
zkm_ctx* zkm_pool_context(zkm_pool* p, size_t w) { return (p && w < p->ctxs.size()) ? p->ctxs[w] : nullptr; }
int zkm_pool_device(const zkm_pool* p, size_t w) { return (p && w < p->devices.size()) ? p->devices[w] : -1; }

int zkm_pool_set_tuning(zkm_pool* p, const char* key, uint64_t value, char** err) {
    return zkm_api("zkm_pool_set_tuning", err, [&] {
        if (!p) throw std::runtime_error("zkm_pool_set_tuning: null argument");
        for (zkm_ctx* c : p->ctxs)
            if (const int rc = zkm_ctx_set_tuning(c, key, value, err)) return rc;
        return 0;
    });
}

int zkm_pool_prove_segments(zkm_pool* p, const zkm_stark_config* cfg, size_t nseg, size_t max_stack, const uint64_t* const* const* traces,
                            const unsigned* const* log_n, const uint64_t* const* pub, const size_t* npub, uint64_t* const* proofs,
                            uint64_t* const* challenges, char** err) {
    return zkm_api("zkm_pool_prove_segments", err,
                   [&] { pool_prove("zkm_pool_prove_segments", p, cfg, nseg, max_stack, traces, nullptr, log_n, pub, npub, proofs, challenges); });
}

int zkm_pool_prove_segments_columns(zkm_pool* p, const zkm_stark_config* cfg, size_t nseg, size_t max_stack,
                                    const uint64_t* const* const* const* columns, const unsigned* const* log_n, const uint64_t* const* pub,
                                    const size_t* npub, uint64_t* const* proofs, uint64_t* const* challenges, char** err) {
    return zkm_api("zkm_pool_prove_segments_columns", err,
                   [&] { pool_prove("zkm_pool_prove_segments_columns", p, cfg, nseg, max_stack, nullptr, columns, log_n, pub, npub, proofs, challenges); });
}

// the groups as above, each ONE zkm_prove_segments_ops call (tables built and proven on the worker's context); proofs == NULL sizes
int zkm_pool_prove_segments_ops(zkm_pool* p, const zkm_stark_config* cfg, size_t nseg, size_t max_stack, const zkm_segment_ops* ops,
                                const uint64_t* const* pub, const size_t* npub, uint64_t* const* proofs, size_t* offsets_out,
                                uint64_t* const* challenges, char** err) {
    const char* what = "zkm_pool_prove_segments_ops";
    return zkm_api(what, err, [&] {
        if (!p || !cfg || !ops || (proofs ? !challenges : !offsets_out)) throw std::runtime_error(std::string(what) + ": null argument");
        if (nseg == 0) throw std::runtime_error(std::string(what) + ": no segments");
        pool_run(what, p, nseg, max_stack, [&](zkm_ctx* c, size_t s0, size_t k, char** e) {
            return zkm_prove_segments_ops_entry(what, c, cfg, k, ops + s0, pub ? pub + s0 : nullptr, npub ? npub + s0 : nullptr,
                                                proofs ? proofs + s0 : nullptr, offsets_out ? offsets_out + (ZKM_NUM_TABLES + 1) * s0 : nullptr,
                                                challenges ? challenges + s0 : nullptr, e, s0);
        });
    });
}

// The groups as above, each a segment list as the emulator records it.  A worker whose context has "pool_stage_ahead" (the default) keeps
// ONE group staged ahead: it stages the group it claims (zkm_segments_calls_stage on its own context), claims and stages its next group
// BEFORE it proves the current one -- so the next group's uploads, expansions, placement and walk run on the copy streams behind the
// current proofs -- proves on the handle's outputs (zkm_prove_segments_ops_steps), frees the handle and moves on: two handles at most.
// Otherwise a group is ONE expanding call (the body of zkm_prove_segments_ops_calls).  The sizing mode serves its groups the same way, so
// a refusal reads the same in the sizing call and in the proving call.
int zkm_pool_prove_segments_calls(zkm_pool* p, const zkm_stark_config* cfg, size_t nseg, size_t max_stack, const zkm_boot_image* images,
                                  const zkm_segment_calls* calls, const uint64_t* const* pub, const size_t* npub, uint64_t* const* proofs,
                                  size_t* offsets_out, uint64_t* const* challenges, char** err) {
    const char* what = "zkm_pool_prove_segments_calls";
    return zkm_api(what, err, [&] {
        if (!p || !cfg || !calls || (proofs ? !challenges : !offsets_out)) throw std::runtime_error(std::string(what) + ": null argument");
        if (nseg == 0) throw std::runtime_error(std::string(what) + ": no segments");
        struct staged_group {
            size_t g = 0;
            std::unique_ptr<void, void (*)(void*)> h{nullptr, zkm_staged_calls_free};
        };
        pool_serve(what, p, nseg, max_stack, [&](size_t w, pool_queue& q) {
            zkm_ctx* c = p->ctxs[w];
            auto at = [&](size_t s0) { return offsets_out ? offsets_out + (ZKM_NUM_TABLES + 1) * s0 : nullptr; };
            if (!c->pool_stage_ahead) {
                for (size_t g; q.claim(&g);) {
                    const size_t s0 = q.groups[g].first, k = q.groups[g].second;
                    char* e = nullptr;
                    const int rc = zkm_prove_segments_ops_calls_entry(what, c, cfg, k, images ? images + s0 : nullptr, calls + s0, pub ? pub + s0 : nullptr,
                                                                      npub ? npub + s0 : nullptr, proofs ? proofs + s0 : nullptr, at(s0),
                                                                      challenges ? challenges + s0 : nullptr, &e, s0);
                    q.done(w, g, rc, e);
                }
                return;
            }
            // claim the next group and queue its staging; false when the queue is empty or stopped, or the stage refuses (reported)
            auto stage_next = [&](staged_group& out) {
                if (!q.claim(&out.g)) return false;
                const size_t s0 = q.groups[out.g].first, k = q.groups[out.g].second;
                char* e = nullptr;
                void* h = nullptr;
                const int rc = zkm_segments_calls_stage_entry(c, k, calls + s0, images ? images + s0 : nullptr, &h, &e, s0);
                out.h.reset(h);
                if (rc != 0) q.done(w, out.g, rc, e);
                return rc == 0;
            };
            // the handle's outputs, proven: steps, operations and images all come from the handle
            auto prove = [&](const staged_group& cur, char** e) {
                const size_t s0 = q.groups[cur.g].first, k = q.groups[cur.g].second;
                std::vector<zkm_cpu_steps> st(k);
                std::vector<zkm_segment_ops> ops(k);
                std::vector<zkm_boot_image> im(images ? k : 0);
                for (size_t s = 0; s < k; s++)
                    if (const int rc = zkm_staged_calls_get_entry(cur.h.get(), s, &st[s], &ops[s], images ? &im[s] : nullptr, e, s0)) return rc;
                return zkm_prove_segments_ops_steps_entry(what, c, cfg, k, images ? im.data() : nullptr, st.data(), ops.data(), pub ? pub + s0 : nullptr,
                                                          npub ? npub + s0 : nullptr, proofs ? proofs + s0 : nullptr, at(s0),
                                                          challenges ? challenges + s0 : nullptr, e, s0);
            };
            // (the handles are freed on every path out of here: a group staged ahead and never proven stays unassigned)
            staged_group cur, ahead;
            for (bool have = stage_next(cur); have;) {
                const bool more = stage_next(ahead);
                if (q.stopped()) return;
                char* e = nullptr;
                const int rc = zkm_api(what, &e, [&] { return prove(cur, &e); });   // (the vectors may throw: nothing unwinds out of a worker thread)
                cur.h.reset();   // (waits for the handle's events; the proofs that read its blocks have ended)
                q.done(w, cur.g, rc, e);
                if (rc != 0) return;
                std::swap(cur, ahead);
                have = more;
            }
        });
    });
}

size_t zkm_pool_plan(size_t nseg, size_t workers, size_t max_stack, size_t* group_sizes_out, size_t capacity) {
    if (max_stack == 0) max_stack = 8;
    const auto g = pool_groups(nseg, workers, max_stack);
    for (size_t k = 0; k < g.size() && k < capacity && group_sizes_out; k++) group_sizes_out[k] = g[k].second;
    return g.size();
}

int zkm_pool_last_assignment(const zkm_pool* p, size_t segment, size_t* worker_out, size_t* group_out) {
    if (!p || segment >= p->last_worker.size() || p->last_worker[segment] == ~(size_t)0) return 1;
    if (worker_out) *worker_out = p->last_worker[segment];
    if (group_out) *group_out = p->last_group[segment];
    return 0;
}

}  // extern "C"
