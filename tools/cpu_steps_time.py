#!/usr/bin/env python3
"""tools/cpu_steps_time.py -- a segment's CPU rows from the compact step log (zkm_prove_segments_ops_steps, csrc/cpu_steps.hip) against
the same segments from their 259-word rows (zkm_prove_segments_ops), timed in one process, alternating: K = 8 segments of 2^16 cycles
(tests/cpu_fixtures.sample_program repeated, PAD-filled; the recorder of tests/cpu_steps_model.py), every list in pinned host memory,
REPS (default 7) timed calls each after warm-up, with the tables-only calls beside them and the proofs compared after the clock.
The sample program sets its registers through `set_reg`, which no instruction covers: those rows (about a third) travel as RAW steps,
2072 bytes each, and are counted in the steps' bytes.
Prints one JSON object (and writes it to the path behind --out):
  bytes_per_segment    what crosses the link for one segment, either way (the steps: records, RAW rows, workgroup bases)
  prove / tables       ms per call of K segments, rows and steps
  kernels              device ms per call by profile scope: cpu_steps/lists and cpu_steps/rows against segment_ops/cpu_rows_to_cols
  no_slower            the bar: the steps call's median is at most the rows call's median plus the rows call's own min-to-max spread"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import zkm_amd  # noqa: E402
from tests import cpu_fixtures as CF  # noqa: E402
from tests import cpu_steps_model as M  # noqa: E402

K = 8
LOG_CYCLES = int(os.environ.get("LOG_CYCLES", "16"))


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "calls": len(ms)}


def pin(ctx, a):
    p = ctx.pinned_array((a.nbytes + 7) // 8)
    p.view(np.uint8)[:a.nbytes] = a.reshape(-1).view(np.uint8)
    return p.view(np.uint8)[:a.nbytes].view(a.dtype).reshape(a.shape)


def segment(ctx):
    """One 2^LOG_CYCLES-cycle segment in pinned memory, both ways: (CpuSteps, the SegmentOps beside them, the expanded SegmentOps)."""
    m = M.Recorder()
    per = len(CF.sample_program(M.Recorder()).rows) - 2
    for _ in range(((1 << LOG_CYCLES) - 2) // per):
        CF.sample_program(m)
    m.pad((1 << LOG_CYCLES) - len(m.rows))
    mem, logic, arith = M.expected_lists(m)
    steps = zkm_amd.CpuSteps(pin(ctx, m.step_array()), pin(ctx, m.raw_array()))
    rows = zkm_amd.SegmentOps(pin(ctx, M.rows_array(m.rows)), pin(ctx, mem), arithmetic_ops=pin(ctx, arith), logic_ops=pin(ctx, logic))
    raw_share = sum(1 for s in m.steps if s[3] == M.KIND["RAW"]) / len(m.steps)
    nbytes = {"rows_call": {"cpu_rows": int(M.rows_array(m.rows[:1]).nbytes) * len(m.rows), "memory_ops": int(mem.nbytes), "logic_ops": int(logic.nbytes),
                            "arithmetic_ops": int(arith.nbytes)},
              "steps_call": {"steps": int(steps.steps.nbytes), "raw_rows": int(steps.raw_rows.nbytes), "workgroup_bases": 12 * ((len(m.steps) + 255) // 256)},
              "raw_share_of_steps": round(raw_share, 3)}
    for v in nbytes.values():
        if isinstance(v, dict):
            v["total"] = sum(v.values())
    return steps, zkm_amd.SegmentOps(None, None), rows, nbytes


def scopes(ctx, fn):
    ctx.profile(True)
    ctx.profile_reset()
    fn()
    ctx.synchronize()
    recs = ctx.profile_records()
    ctx.profile(False)
    ctx.profile_reset()
    return {k: {"launches": n, "ms": round(ms, 4)} for k, (n, ms) in sorted(recs.items())
            if k.startswith(("cpu_steps/", "segment_ops/", "memory_trace/", "arithmetic_trace/", "logic_trace"))}


def main():
    reps = int(os.environ.get("REPS", "7"))
    ctx = zkm_amd.Context(int(os.environ.get("ZKM_BENCH_DEVICE", "0")))
    steps, beside, rows, nbytes = segment(ctx)
    pubs = [[1, 2, 3, s] for s in range(K)]
    # (a call's segments share their lists, as tools/segments_ops_time.py's do: K uploads of the same pinned memory)
    want = ctx.prove_segments_ops([rows] * K, public_values=pubs)
    sizes = [o for _, _, o in want]

    def prove_rows():
        return ctx.prove_segments_ops([rows] * K, public_values=pubs, sizes=sizes)

    def prove_steps():
        return ctx.prove_segments_ops_steps([steps] * K, [beside] * K, public_values=pubs, sizes=sizes)

    def tables_rows():
        for st, _ in ctx.segments_tables([rows] * K):
            st.free()

    def tables_steps():
        for st, _ in ctx.segments_tables_steps([steps] * K, [beside] * K):
            st.free()
    for fn in (prove_rows, prove_steps, tables_rows, tables_steps) * 2:
        fn()
    t = {fn.__name__: [] for fn in (prove_rows, prove_steps, tables_rows, tables_steps)}
    for _ in range(reps):                     # alternating: what drifts in the process drifts for both
        for fn in (prove_rows, prove_steps, tables_rows, tables_steps):
            ctx.synchronize()
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            t[fn.__name__].append((time.perf_counter() - t0) * 1e3)
    got = prove_steps()
    same = all((p == wp).all() and (c == wc).all() and o == wo for (p, c, o), (wp, wc, wo) in zip(got, want))
    r, s = stats(t["prove_rows"]), stats(t["prove_steps"])
    out = {"tool": "cpu_steps_time", "segments_per_call": K, "log_cycles": LOG_CYCLES, "reps": reps, "bytes_per_segment": nbytes,
           "prove": {"rows": r, "steps": s, "segments_per_s": {"rows": round(K * 1e3 / r["median_ms"], 1), "steps": round(K * 1e3 / s["median_ms"], 1)}},
           "tables": {"rows": stats(t["tables_rows"]), "steps": stats(t["tables_steps"])},
           "kernels": {"rows": scopes(ctx, tables_rows), "steps": scopes(ctx, tables_steps)},
           "no_slower": {"rows_spread_ms": round(r["max_ms"] - r["min_ms"], 3), "steps_minus_rows_median_ms": round(s["median_ms"] - r["median_ms"], 3),
                         "holds": bool(s["median_ms"] <= r["median_ms"] + (r["max_ms"] - r["min_ms"]))},
           "equal_proof_words": bool(same)}
    text = json.dumps(out, indent=1)
    print(json.dumps(out))
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as fh:
            fh.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
