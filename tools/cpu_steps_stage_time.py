#!/usr/bin/env python3
"""tools/cpu_steps_stage_time.py -- step logs staged behind the current proofs (zkm_cpu_steps_stage, csrc/cpu_steps_walk.hip) against
the same proving call taking its steps in the call (zkm_prove_segments_ops_steps as it was), timed in one process, alternating: one
context, K = 8 segments of 2^16 cycles of the sample program sharing one pinned list (tools/cpu_steps_time.py's segment), REPS
(default 20) timed calls each after warm-up, the proofs compared after the clock.
  unstaged   prove_segments_ops_steps on the host lists: the walk on the calling thread, records and bases uploaded in the call
  staged     each call stages the NEXT call's steps (upload and device walk on the copy streams) and then proves the steps staged during
             the call before it -- the loop of tools/segments_ops_time.py's staged lists; the handle of the consumed steps is freed
Prints one JSON object (and writes it to the path behind --out):
  prove            ms per call of K segments: median, min, max
  host             ms on the calling thread before any device work.  unstaged_check_host: the *_steps call without a context, which runs
                   every host check of the K segments (the walk among them) and then misses its context; staged_stage_call and
                   staged_get: what the staged path spends instead (queuing the stage; the K gets of steps that have landed).  The
                   staged call's own check_host is a registry lookup per segment and is not timed apart.
  walk_kernels     device ms of k_steps_walk + k_steps_scan for the K segments (profile scope cpu_steps/walk of zkm_cpu_steps_scan,
                   in a pass of its own)
  no_slower        the bar: the staged call's median is at most the unstaged call's median plus the unstaged call's own min-to-max spread
  many             (LEGS=one,many) 8 contexts x 8 segments, one host thread a context, all on the one pinned list: rounds of CALLS
                   (default 5) calls a context, every context in the same mode, the modes alternating; segments/s of each round
  not_run          what this run leaves unmeasured"""
import ctypes as C
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import zkm_amd  # noqa: E402
from cpu_steps_time import K, LOG_CYCLES, segment, stats  # noqa: E402


def host_ms(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return stats(out)


def leg_many(steps, beside, sizes, want, nctx=8):
    """nctx contexts, a host thread each, K segments a call from the one pinned list: rounds in which every context makes `calls` calls
    in the same mode.  Returns segments/s per round and mode."""
    device, calls, rounds = int(os.environ.get("ZKM_BENCH_DEVICE", "0")), int(os.environ.get("CALLS", "5")), int(os.environ.get("ROUNDS", "4"))
    ctxs = [zkm_amd.Context(device) for _ in range(nctx)]
    lists, ops = [steps] * K, [beside] * K
    pubs = [[[1, 2, 3, s] for s in range(K)] for _ in ctxs]
    last = [None] * nctx

    def unstaged(i, n):
        for _ in range(n):
            last[i] = ctxs[i].prove_segments_ops_steps(lists, ops, public_values=pubs[i], sizes=sizes)

    def staged(i, n):
        cur = ctxs[i].cpu_steps_stage(lists)
        for _ in range(n):
            nxt = ctxs[i].cpu_steps_stage(lists)
            last[i] = ctxs[i].prove_segments_ops_steps([cur.get(s) for s in range(K)], ops, public_values=pubs[i], sizes=sizes)
            cur.free()
            cur = nxt
        cur.free()

    def round_of(fn, n):
        start = threading.Barrier(nctx + 1)

        def work(i):
            start.wait()
            fn(i, n)
            ctxs[i].synchronize()
        th = [threading.Thread(target=work, args=(i,)) for i in range(nctx)]
        for t in th:
            t.start()
        start.wait()
        t0 = time.perf_counter()
        for t in th:
            t.join()
        return nctx * K * n / (time.perf_counter() - t0)
    for fn in (unstaged, staged):
        round_of(fn, 2)
    rate = {"unstaged": [], "staged": []}
    same = True
    for _ in range(rounds):
        for fn in (unstaged, staged):
            rate[fn.__name__].append(round(round_of(fn, calls), 1))
            same &= all((p == wp).all() and (c == wc).all() for (p, c, _), (wp, wc, _) in zip(last[nctx - 1], want))
    for c in ctxs:
        c.close()
    med = {k: round(float(np.median(v)), 1) for k, v in rate.items()}
    return {"contexts": nctx, "segments_per_call": K, "calls_per_context_and_round": calls, "rounds": rounds, "segments_per_s_by_round": rate,
            "segments_per_s_median": med, "hardware_queues": os.environ.get("GPU_MAX_HW_QUEUES", "unset"), "equal_proof_words": bool(same)}


def main():
    reps = int(os.environ.get("REPS", "20"))
    legs = os.environ.get("LEGS", "one").split(",")
    ctx = zkm_amd.Context(int(os.environ.get("ZKM_BENCH_DEVICE", "0")))
    steps, beside, _, nbytes = segment(ctx)
    pubs = [[1, 2, 3, s] for s in range(K)]
    lists, ops = [steps] * K, [beside] * K
    want = ctx.prove_segments_ops_steps(lists, ops, public_values=pubs)
    sizes = [o for _, _, o in want]

    def unstaged():
        return ctx.prove_segments_ops_steps(lists, ops, public_values=pubs, sizes=sizes)

    state = {"cur": ctx.cpu_steps_stage(lists), "stage_ms": [], "get_ms": []}

    def staged():
        t0 = time.perf_counter()
        nxt = ctx.cpu_steps_stage(lists)
        t1 = time.perf_counter()
        got = [state["cur"].get(s) for s in range(K)]
        t2 = time.perf_counter()
        out = ctx.prove_segments_ops_steps(got, ops, public_values=pubs, sizes=sizes)
        state["cur"].free()
        state["cur"] = nxt
        state["stage_ms"].append((t1 - t0) * 1e3)
        state["get_ms"].append((t2 - t1) * 1e3)
        return out
    for fn in (unstaged, staged) * 3:
        fn()
    state["stage_ms"], state["get_ms"] = [], []
    t = {"unstaged": [], "staged": []}
    for _ in range(reps):                     # alternating: what drifts in the process drifts for both
        for fn in (unstaged, staged):
            ctx.synchronize()
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            t[fn.__name__].append((time.perf_counter() - t0) * 1e3)
    got = staged()
    same = all((p == wp).all() and (c == wc).all() and o == wo for (p, c, o), (wp, wc, wo) in zip(got, want))
    state["cur"].free()

    # the host's share: the unstaged call without a context makes every host check of the K segments, then misses the context
    L, cfg = ctx.L, ctx.standard_config()
    sl = (zkm_amd.CpuStepsStruct * K)(*[x.struct() for x in lists])
    so = (zkm_amd.SegmentOpsStruct * K)(*[o.struct() for o in ops])
    offs, err = (C.c_size_t * (13 * K))(), C.c_char_p()

    def check_host():
        assert L.zkm_prove_segments_ops_steps(None, C.byref(cfg), K, None, sl, so, None, None, None, offs, None, C.byref(err)) == 1
        assert err.value.endswith(b": null argument"), err.value
    check_host()
    host = {"unstaged_check_host": host_ms(check_host, reps), "staged_stage_call": stats(state["stage_ms"]), "staged_get": stats(state["get_ms"])}

    # the walk's kernels, in a pass of their own
    counts = ctx.cpu_steps_scan(lists)
    ctx.profile(True)
    ctx.profile_reset()
    for _ in range(reps):
        ctx.cpu_steps_scan(lists)
    ctx.synchronize()
    n, ms = ctx.profile_records()["cpu_steps/walk"]
    ctx.profile(False)
    ctx.profile_reset()

    u, s = stats(t["unstaged"]), stats(t["staged"])
    out = {"tool": "cpu_steps_stage_time", "contexts": 1, "segments_per_call": K, "log_cycles": LOG_CYCLES, "reps": reps,
           "bytes_per_segment": nbytes["steps_call"],
           "prove": {"unstaged": u, "staged": s, "segments_per_s": {"unstaged": round(K * 1e3 / u["median_ms"], 1), "staged": round(K * 1e3 / s["median_ms"], 1)}},
           "host": host,
           "walk_kernels": {"scope": "cpu_steps/walk", "calls": n, "ms_per_call": round(ms / n, 4), "counts_equal_host_walk": counts == [steps.counts()] * K},
           "no_slower": {"unstaged_spread_ms": round(u["max_ms"] - u["min_ms"], 3), "staged_minus_unstaged_median_ms": round(s["median_ms"] - u["median_ms"], 3),
                         "holds": bool(s["median_ms"] <= u["median_ms"] + (u["max_ms"] - u["min_ms"]))},
           "equal_proof_words": bool(same),
           "not_run": ["a program without RAW rows (3.1 MB a segment)", "the staged call's check_host apart from the call"]}
    if "many" in legs:
        out["many"] = leg_many(steps, beside, sizes, want)
    else:
        out["not_run"].insert(0, "8 contexts x 8 segments, where the link and the 16 CPUs are shared")
    text = json.dumps(out, indent=1)
    print(json.dumps(out))
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as fh:
            fh.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
