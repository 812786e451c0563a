#!/usr/bin/env python3
"""tools/calls_stage_time.py -- K segments' calls staged behind the current proofs (zkm_segments_calls_stage, csrc/calls_stage.hip) against
the same proving call expanding them in the call (zkm_prove_segments_ops_calls, the yardstick), timed in one process, alternating: one
context, K = 8 segments of 2^16 cycles, every list in pinned memory, REPS (default 20) timed calls each after a warm-up, the proofs
compared after the clock.  Two shapes (SHAPES=all_kinds,sample):
  all_kinds   the shape of profiles/calls_expand_time.json (tools/calls_expand_time.py's segment: all four kinds, a quarter each)
  sample      the shape of profiles/insn_rows_time.json (tools/insn_rows_time.py's program: the sample program's RAW share as
              instruction records, no Keccak table to drown the difference); the K segments share one pinned set of lists
  unstaged   prove_segments_ops_calls: records, clocks and the patched list built per row on the calling thread, one host wait for the
             expansion, the builder's walk on the calling thread
  staged     each call stages the NEXT call's segments (uploads, expansions, placement and walk on the copy streams) and then proves the
             ones staged during the call before it; the handle of the consumed segments is freed
Prints one JSON object (and writes it to the path behind --out), per shape:
  prove            ms per call of K segments: median, min, max
  host             ms on the calling thread.  unstaged_expand_host: zkm_segments_calls_expand without a context, which runs the
                   expansion's whole host half for the K segments and then misses its context (the builder's host walk of the patched
                   lists, profiles/cpu_steps_stage_time.json, comes on top of it); staged_stage_call and staged_get: what the staged
                   path spends instead (the whole stage call, queuing included; the K gets of segments that have landed)
  kernels          device ms between the events around the expansion launches, the placement (k_calls_place, k_calls_verdict) and the
                   walk (k_steps_walk, k_steps_scan and the verdicts' download) of one stage of the K segments on an idle context
                   (profile scopes calls_stage/expand, /place, /walk; in a pass of their own)
  no_slower        the bar: the staged call's median is at most the unstaged call's median plus the unstaged call's own min-to-max
                   spread; and the staged path's calling-thread time is below the unstaged expansion's
  not_run          what this run leaves unmeasured"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import zkm_amd  # noqa: E402
import calls_expand_time as CE  # noqa: E402
import insn_rows_time as IR  # noqa: E402

K = int(os.environ.get("SEGMENTS", "8"))
LOG_CYCLES = CE.LOG_CYCLES
stats, pin = CE.stats, CE.pin


def host_ms(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return stats(out)


def shape_all_kinds(ctx):
    cycle = CE.insn_cycle()
    built = [CE.segment(ctx, 100 + s, cycle) for s in range(K)]
    return [zkm_amd.SegmentCalls(**kw) for kw, _ in built], built[0][1]


def shape_sample(ctx):
    m = IR.program(1 << LOG_CYCLES)
    records, clocks = m.insn_lists()
    bare = m.cpu_steps(zkm_amd)
    steps = zkm_amd.CpuSteps(pin(ctx, bare.steps), pin(ctx, bare.raw_rows.reshape(-1, 259)))
    one = zkm_amd.SegmentCalls(steps=steps, first_clock=m.first_clock, insns=(pin(ctx, records), pin(ctx, clocks)))
    return [one] * K, {"instructions": int(len(records)), "share_of_rows": round(len(records) / (1 << LOG_CYCLES), 4), "own_raw_rows": int(bare.nraw)}


def measure(ctx, calls, holds, reps):
    pubs = [[1, 2, 3 + s] for s in range(K)]
    want = ctx.prove_segments_ops_calls(calls, public_values=pubs)
    sizes = [o for _, _, o in want]

    def unstaged():
        return ctx.prove_segments_ops_calls(calls, public_values=pubs, sizes=sizes)

    state = {"cur": ctx.segments_calls_stage(calls), "stage_ms": [], "get_ms": []}

    def staged():
        t0 = time.perf_counter()
        nxt = ctx.segments_calls_stage(calls)
        t1 = time.perf_counter()
        got = [state["cur"].get(s) for s in range(K)]
        t2 = time.perf_counter()
        out = ctx.prove_segments_ops_steps([st for st, _, _ in got], [o for _, o, _ in got], public_values=pubs, sizes=sizes)
        state["cur"].free()
        state["cur"] = nxt
        state["stage_ms"].append((t1 - t0) * 1e3)
        state["get_ms"].append((t2 - t1) * 1e3)
        return out
    for fn in (unstaged, staged) * 3:
        fn()
    state["stage_ms"], state["get_ms"] = [], []
    t, waits = {"unstaged": [], "staged": []}, {}
    for _ in range(reps):                     # alternating: what drifts in the process drifts for both
        for fn in (unstaged, staged):
            ctx.synchronize()
            w0 = ctx.host_waits()
            t0 = time.perf_counter()
            fn()
            waits[fn.__name__] = ctx.host_waits() - w0
            ctx.synchronize()
            t[fn.__name__].append((time.perf_counter() - t0) * 1e3)
    got = staged()
    same = all((p == wp).all() and (c == wc).all() and o == wo for (p, c, o), (wp, wc, wo) in zip(got, want))
    state["cur"].free()

    # the host's share of the unstaged expansion: the call without a context makes every host step of the K segments, then misses it
    arr, h, err = ctx._calls_array(calls), C.c_void_p(), C.c_char_p()

    def expand_host():
        assert ctx.L.zkm_segments_calls_expand(None, K, C.addressof(arr), C.byref(h), C.byref(err)) == 1
        assert err.value.endswith(b": null argument"), err.value
    expand_host()
    host = {"unstaged_expand_host": host_ms(expand_host, reps), "staged_stage_call": stats(state["stage_ms"]), "staged_get": stats(state["get_ms"])}

    # the stage's kernels on an idle context, in a pass of their own
    ctx.synchronize()
    ctx.profile(True)
    ctx.profile_reset()
    for _ in range(reps):
        with ctx.segments_calls_stage(calls) as x:
            x.ready(wait=True)
    recs = ctx.profile_records()
    ctx.profile(False)
    ctx.profile_reset()
    kernels = {s: {"launch_sets": int(recs[s][0]), "ms_per_stage": round(recs[s][1] / reps, 4)} for s in ("calls_stage/expand", "calls_stage/place", "calls_stage/walk")
               if s in recs}

    u, s = stats(t["unstaged"]), stats(t["staged"])
    thread = host["staged_stage_call"]["median_ms"] + host["staged_get"]["median_ms"]
    return {"segment": dict(holds, generated={k: v for k, v in zkm_amd.segment_calls_steps(calls[0])[1].items()}),
            "prove": {"unstaged": dict(u, host_waits=int(waits["unstaged"])), "staged": dict(s, host_waits=int(waits["staged"])),
                      "segments_per_s": {"unstaged": round(K * 1e3 / u["median_ms"], 1), "staged": round(K * 1e3 / s["median_ms"], 1)}},
            "host": host, "kernels": kernels,
            "no_slower": {"unstaged_spread_ms": round(u["max_ms"] - u["min_ms"], 3), "staged_minus_unstaged_median_ms": round(s["median_ms"] - u["median_ms"], 3),
                          "holds": bool(s["median_ms"] <= u["median_ms"] + (u["max_ms"] - u["min_ms"])),
                          "calling_thread_ms": {"staged_stage_plus_gets": round(thread, 3), "unstaged_expand_host": host["unstaged_expand_host"]["median_ms"]},
                          "calling_thread_lower": bool(thread < host["unstaged_expand_host"]["median_ms"])},
            "equal_proof_words": bool(same)}


def main():
    reps = int(os.environ.get("REPS", "20"))
    shapes = os.environ.get("SHAPES", "all_kinds,sample").split(",")
    ctx = zkm_amd.Context(int(os.environ.get("ZKM_BENCH_DEVICE", "0")))
    out = {"tool": "calls_stage_time", "contexts": 1, "segments_per_call": K, "log_cycles": LOG_CYCLES, "reps": reps,
           "hardware_queues": os.environ.get("GPU_MAX_HW_QUEUES", "unset"), "shapes": {}}
    for name, build in (("all_kinds", shape_all_kinds), ("sample", shape_sample)):
        if name in shapes:
            calls, holds = build(ctx)
            out["shapes"][name] = measure(ctx, calls, holds, reps)
    out["not_run"] = [s for s in ("all_kinds", "sample") if s not in shapes] + \
        ["8 contexts x 8 segments, where the link and the 16 CPUs are shared", "the builder's host walk of the unstaged call apart from the call",
         "lists in pageable memory"]
    print(json.dumps(out))
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
