#!/usr/bin/env python3
"""tools/sha_calls_time.py -- a segment of SHA-256 precompile calls proven both ways on one context, in alternating calls:
  composed   Context.sha_calls_expand (zkm_sha_calls_witness, csrc/sha_calls.hip: rows and lists written on the device from the sponge
             tables' lists) and then zkm_prove_segments_ops_steps on its device blocks;
  host       zkm_prove_segments_ops_steps fed the host-expanded rows and lists in pinned memory (that path's code is what it was before
             the expansion existed).
The segment: 2^LOG_CYCLES cycles (default 16) of alternating SYSSHAEXTEND / SYSSHACOMPRESS calls at disjoint addresses on seeded random
words, PAD-filled; it does nothing but hash.  The host-expanded arrays are the device's own outputs, downloaded once before the clock
(tests/test_gpu_sha_calls.py holds them to the model word for word), so that building the segment does not take the Python model minutes.
Prints one JSON object (and writes it to the path behind --out):
  bytes_per_call / bytes_per_segment   what the expansion saves from crossing the link, per call of either kind (these are asserted to be
                                       the figures derived from the counts) and for the segment, both ways
  prove                                ms per proving call, both ways: median, min, max over REPS (default 7) alternating calls; composed
                                       includes the expansion call
  expand                               ms of sha_calls_expand alone (allocations, own uploads, zkm_sha_calls_witness), and the kernel's
                                       device ms (profile scope sha_calls/rows_lists)
  no_slower                            the bar: composed's median is at most host's median plus host's own min-to-max spread
One context does not load the link as eight do: what the saved upload is worth under load is NOT measured here."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import zkm_amd  # noqa: E402

LOG_CYCLES = int(os.environ.get("LOG_CYCLES", "16"))
PAD, RAW = zkm_amd.STEP["PAD"], zkm_amd.STEP["RAW"]


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "calls": len(ms)}


def pin(ctx, a):
    p = ctx.pinned_array((a.nbytes + 7) // 8)
    p.view(np.uint8)[:a.nbytes] = a.reshape(-1).view(np.uint8)
    return p.view(np.uint8)[:a.nbytes].view(a.dtype).reshape(a.shape)


def calls(pairs, seed=1):
    """`pairs` extend calls and as many compress calls, alternating in time from clock 0: pair k's extend call takes clocks
    [107 k, 107 k + 96), its compress call the eleven behind."""
    rng = np.random.default_rng(seed)
    k = np.arange(pairs, dtype=np.uint64)
    emeta = np.stack([0 * k, 0 * k, 0x100000 + 0x100 * k, 10 * (107 * k + 1)], axis=1)
    cmeta = np.stack([0 * k, 0 * k, 0x4000000 + 0x20 * k, 10 * (107 * k + 96 + 9), 0x8000000 + 0x100 * k, 0 * k, 0 * k, 0 * k], axis=1)
    u32 = lambda *shape: rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)
    return (u32(pairs, 16), np.ascontiguousarray(emeta)), (u32(pairs, 8), u32(pairs, 64), np.ascontiguousarray(cmeta))


def main():
    reps = int(os.environ.get("REPS", "7"))
    ctx = zkm_amd.Context(int(os.environ.get("ZKM_BENCH_DEVICE", "0")))
    n = 1 << LOG_CYCLES
    pairs = (n - 1) // 107                     # at least one PAD row, as simulate_cpu pushes
    e, c = calls(pairs)
    rows, mem, logic, ext = zkm_amd.sha_calls_counts(pairs, pairs)
    # the step list: the calls' RAW records at their clocks, PAD behind them
    steps = np.zeros(n, dtype=zkm_amd.CPU_STEP_DT)
    steps["kind"] = PAD
    steps["kind"][:rows] = RAW                 # placeholders: sha_calls_expand / the records below take their place
    bare = zkm_amd.CpuSteps(steps)
    records, clocks = zkm_amd.sha_calls_steps(e[1], c[2], raw_base=0)
    assert sorted(clocks.tolist()) == list(range(rows))
    # host-expanded: the device's outputs, downloaded before the clock
    x_rows, x_mem, x_logic, x_in, x_ts = ctx.sha_calls_witness(e, c)
    host_steps = steps.copy()
    host_steps[clocks.astype(np.int64)] = records
    e_p, c_p = tuple(pin(ctx, a) for a in e), tuple(pin(ctx, a) for a in c)
    host = (zkm_amd.CpuSteps(pin(ctx, host_steps), pin(ctx, x_rows)),
            zkm_amd.SegmentOps(None, pin(ctx, x_mem), logic_ops=pin(ctx, x_logic), sha_extend=(pin(ctx, x_in), pin(ctx, x_ts)), sha_extend_sponge=e_p,
                               sha_compress=c_p, sha_compress_sponge=c_p))
    per_call = {"extend": {"cpu_rows": 96 * 259 * 8, "memory_ops": 768 * 48, "logic_ops": 192 * 12, "sha_extend_rows": 48 * 24},
                "compress": {"cpu_rows": 11 * 259 * 8, "memory_ops": 288 * 48, "logic_ops": 768 * 12, "sha_extend_rows": 0}}
    for v in per_call.values():
        v["total"] = sum(v.values())
    assert per_call["extend"]["total"] == 198912 + 36864 + 2304 + 1152 and per_call["compress"]["total"] == 22792 + 13824 + 9216
    expanded = int(x_rows.nbytes + x_mem.nbytes + x_logic.nbytes + x_in.nbytes + x_ts.nbytes)
    assert expanded == pairs * (per_call["extend"]["total"] + per_call["compress"]["total"])
    lists = int(sum(a.nbytes for a in e + c))
    assert lists == pairs * (96 + 352)
    common = int(steps.nbytes + 12 * ((n + 255) // 256) + e[0].nbytes + e[1].nbytes + 2 * sum(a.nbytes for a in c))   # steps, bases, the sponge groups
    nbytes = {"calls": {"extend": pairs, "compress": pairs}, "host": {"expanded_rows_and_lists": expanded, "steps_and_sponge_lists": common, "total": expanded + common},
              "composed": {"expansion_call_lists": lists, "steps_and_sponge_lists": common, "total": lists + common}}
    pubs = [[1, 2, 3]]
    want = ctx.prove_segments_ops_steps([host[0]], [host[1]], public_values=pubs)
    sizes = [o for _, _, o in want]

    def prove_host():
        return ctx.prove_segments_ops_steps([host[0]], [host[1]], public_values=pubs, sizes=sizes)

    t_expand = []

    def prove_composed():
        t0 = time.perf_counter()
        st, ops = ctx.sha_calls_expand(bare, extend=e_p, compress=c_p)
        t_expand.append((time.perf_counter() - t0) * 1e3)
        try:
            return ctx.prove_segments_ops_steps([st], [ops], public_values=pubs, sizes=sizes)
        finally:
            st.raw_rows.free()
            ops.free()
    for fn in (prove_host, prove_composed) * 2:
        fn()
    t_expand.clear()
    t = {"prove_host": [], "prove_composed": []}
    for _ in range(reps):                      # alternating: what drifts in the process drifts for both
        for fn in (prove_host, prove_composed):
            ctx.synchronize()
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            t[fn.__name__].append((time.perf_counter() - t0) * 1e3)
    expand_ms = list(t_expand)
    got = prove_composed()
    same = all((p == wp).all() and (ch == wch).all() and o == wo for (p, ch, o), (wp, wch, wo) in zip(got, want))
    ctx.profile(True)
    ctx.profile_reset()
    st, ops = ctx.sha_calls_expand(bare, extend=e_p, compress=c_p)
    ctx.synchronize()
    recs = ctx.profile_records()
    ctx.profile(False)
    ctx.profile_reset()
    st.raw_rows.free()
    ops.free()
    launches, kernel_ms = recs["sha_calls/rows_lists"]
    h, s = stats(t["prove_host"]), stats(t["prove_composed"])
    out = {"tool": "sha_calls_time", "log_cycles": LOG_CYCLES, "reps": reps, "bytes_per_call": per_call, "bytes_per_segment": nbytes,
           "prove": {"host": h, "composed": s},
           "expand": dict(stats(expand_ms), kernel={"scope": "sha_calls/rows_lists", "launches": launches, "ms": round(kernel_ms, 4)}),
           "no_slower": {"host_spread_ms": round(h["max_ms"] - h["min_ms"], 3), "composed_minus_host_median_ms": round(s["median_ms"] - h["median_ms"], 3),
                         "holds": bool(s["median_ms"] <= h["median_ms"] + (h["max_ms"] - h["min_ms"]))},
           "equal_proof_words": bool(same),
           "not_measured": "several contexts sharing the link: one context does not load it as eight do"}
    print(json.dumps(out))
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
