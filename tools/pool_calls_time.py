#!/usr/bin/env python3
"""tools/pool_calls_time.py -- the pool proving segments as the emulator records them (zkm_pool_prove_segments_calls, csrc/pool.hip), its
workers staging one group ahead ("pool_stage_ahead" 1) against expanding each group in its call (0), and against the hand-written loop
on one context that does what one worker does: zkm_segments_calls_stage of group k + 1 before zkm_prove_segments_ops_steps of group k.
One device; the sample-program shape of tools/calls_stage_time.py (segments of 2^16 cycles, 20,705 instruction records each, groups of
8, every list pinned, the segments share one set of lists); GROUPS (default 4) groups per worker and call, so a worker stages ahead
GROUPS - 1 times; REPS (default 5) timed calls of each variant after a warm-up, alternating, the sizes given (no sizing call); the proofs
compared with Context.prove_segments_ops_calls after the clock.  Every run is a child process of its own under a time limit:
  one       1 worker: (a) the pool in mode 1, (b) the pool in mode 0, (c) the hand-written loop on a plain context
  two       contexts_per_device 2: the pool in both modes
  eight     contexts_per_device 8: the pool in both modes
Prints one JSON object (and writes it to the path behind --out), per run and variant: ms per call (median, min, max), segments/s from
the median, the min-to-max spread; for `one` the bar of the issue -- (a)'s median is at most (c)'s plus (c)'s own spread -- and for
every context count whether mode 1 is slower than mode 0 beyond mode 0's spread (recorded, not required); what was not run."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNS = {"one": 1, "two": 2, "eight": 8}
STACK = 8


def child(run):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import zkm_amd
    import calls_expand_time as CE
    import insn_rows_time as IR
    stats, pin = CE.stats, CE.pin
    workers, groups, reps = RUNS[run], int(os.environ.get("GROUPS", "4")), int(os.environ.get("REPS", "5"))
    device = int(os.environ.get("ZKM_BENCH_DEVICE", "0"))
    nseg = workers * groups * STACK
    ctx = zkm_amd.Context(device)          # pins the lists, judges, and runs the hand-written loop
    m = IR.program(1 << CE.LOG_CYCLES)
    records, clocks = m.insn_lists()
    bare = m.cpu_steps(zkm_amd)
    steps = zkm_amd.CpuSteps(pin(ctx, bare.steps), pin(ctx, bare.raw_rows.reshape(-1, 259)))
    one = zkm_amd.SegmentCalls(steps=steps, first_clock=m.first_clock, insns=(pin(ctx, records), pin(ctx, clocks)))
    calls = [one] * nseg
    pubs = [[1, 2, 3 + s % STACK] for s in range(nseg)]
    want = ctx.prove_segments_ops_calls(calls[:STACK], public_values=pubs[:STACK])
    sizes = [o for _, _, o in want]

    pool = zkm_amd.Pool((device,), workers)
    cfg = pool.standard_config()
    mar = zkm_amd._marshal_ops([q.own for q in calls], pubs, cfg)
    mar.offs[:] = [x for s in range(nseg) for x in sizes[s % STACK]]
    mar.alloc()
    arr, err = ctx._calls_array(calls), C.c_char_p()

    def pooled(mode):
        def run_pool():
            rc = pool.L.zkm_pool_prove_segments_calls(pool.h, C.byref(cfg), nseg, STACK, None, C.addressof(arr), mar.pv, mar.npv, mar.po, mar.offs, mar.co,
                                                      C.byref(err))
            assert rc == 0, err.value
            return mar.results()
        run_pool.__name__ = "pool_mode_%d" % mode
        run_pool.mode = mode
        return run_pool

    def loop():
        """What the parent commit allows on one context: group k + 1 staged before group k is proven."""
        out, cur = [], ctx.segments_calls_stage(calls[:STACK])
        for g in range(nseg // STACK):
            nxt = ctx.segments_calls_stage(calls[(g + 1) * STACK:(g + 2) * STACK]) if (g + 1) * STACK < nseg else None
            got = [cur.get(s) for s in range(STACK)]
            out += ctx.prove_segments_ops_steps([st for st, _, _ in got], [o for _, o, _ in got], public_values=pubs[g * STACK:(g + 1) * STACK], sizes=sizes)
            cur.free()
            cur = nxt
        return out
    loop.__name__, loop.mode = "one_context_loop", None

    variants = [pooled(1), pooled(0)] + ([loop] if workers == 1 else [])

    def call(fn):
        if fn.mode is not None:
            pool.set_tuning("pool_stage_ahead", fn.mode)
        return fn()
    for fn in variants * 2:                   # warm-up: the allocators' blocks, the resident tables
        call(fn)
    t = {fn.__name__: [] for fn in variants}
    for _ in range(reps):                     # alternating: what drifts in the process drifts for all
        for fn in variants:
            if fn.mode is not None:
                pool.set_tuning("pool_stage_ahead", fn.mode)
            t0 = time.perf_counter()
            fn()
            t[fn.__name__].append((time.perf_counter() - t0) * 1e3)
    same = {}
    for fn in variants:
        got = call(fn)
        same[fn.__name__] = bool(len(got) == nseg and all((p == want[s % STACK][0]).all() and (c == want[s % STACK][1]).all() and o == sizes[s % STACK]
                                                          for s, (p, c, o) in enumerate(got)))
    groups_of = sorted({pool.last_assignment(s)[1] for s in range(nseg)})
    out = {"workers": workers, "groups_per_worker": groups, "segments_per_call": nseg, "groups": len(groups_of), "equal_proof_words": same, "variants": {}}
    for name, ms in t.items():
        s = stats(ms)
        out["variants"][name] = dict(s, segments_per_s=round(nseg * 1e3 / s["median_ms"], 1), spread_ms=round(s["max_ms"] - s["min_ms"], 3))
    v = out["variants"]
    m1, m0 = v["pool_mode_1"], v["pool_mode_0"]
    out["mode_1_slower_than_mode_0_beyond_its_spread"] = bool(m1["median_ms"] > m0["median_ms"] + m0["spread_ms"])
    out["mode_1_minus_mode_0_median_ms"] = round(m1["median_ms"] - m0["median_ms"], 3)
    if workers == 1:
        c = v["one_context_loop"]
        out["pool_no_slower_than_the_loop"] = {"loop_spread_ms": c["spread_ms"], "pool_minus_loop_median_ms": round(m1["median_ms"] - c["median_ms"], 3),
                                               "holds": bool(m1["median_ms"] <= c["median_ms"] + c["spread_ms"])}
    pool.close()
    ctx.close()
    print("RESULT " + json.dumps(out))


def main():
    if "--run" in sys.argv:
        return child(sys.argv[sys.argv.index("--run") + 1])
    limit = int(os.environ.get("RUN_TIMEOUT", "420"))
    names = os.environ.get("RUNS", "one,two,eight").split(",")
    out = {"tool": "pool_calls_time", "devices": 1, "segments_per_group": STACK, "log_cycles": 16, "shape": "sample (tools/calls_stage_time.py)",
           "hardware_queues": os.environ.get("GPU_MAX_HW_QUEUES", "unset"), "runs": {}}
    for name in names:
        # a fresh process a run, under a time limit of its own; a run that fails or runs out of time ends the measurement
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--run", name], capture_output=True, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not lines:
            out["runs"][name] = {"failed": r.returncode, "stderr": r.stderr[-2000:]}
            break
        out["runs"][name] = json.loads(lines[-1][len("RESULT "):])
        print("%s: done" % name, file=sys.stderr, flush=True)
    out["not_run"] = [n for n in RUNS if n not in out["runs"]] + ["more than one device", "lists in pageable memory", "segments with calls of all four kinds",
                                                                  "boot images"]
    print(json.dumps(out))
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")
    return 0 if all("failed" not in r for r in out["runs"].values()) else 1


if __name__ == "__main__":
    sys.exit(main())
