#!/usr/bin/env python3
"""tools/segment_check_time.py -- zkm_segments_check (csrc/segment_check.hip) and the gate "check_witness" on one GPU, for the consistent
2^16-cycle twelve-table segment of tests/segment_ops_fixtures.build_segment_ops(oracle, repeat=128) resident in device memory, K = 1 and
K = 8 (the same tables K times: the checks only read them):
  1. zkm_segments_check against the three per-segment entry points (zkm_segment_witness_check, zkm_segment_lookup_check,
     zkm_segment_check_ctls) called segment by segment in the same run -- the code path of the checks before they took K segments;
  2. the host waits and the launches per profile scope of both (a second set of calls, profiler on);
  3. zkm_prove_segments of 8 with "check_witness" 0 and 1, and with "check_ctls" 1;
  4. the same with one cell of segment 5's Cpu table changed (the calls fail: the time to the refusal).
Medians with minimum and maximum over `REPS` (at least 20) calls after a warm-up, profiler off.
NOT measured: several contexts sharing the GPU, tables taller than this segment's, host-resident tables (their upload would dominate).
Writes profiles/segment_check_time.json and prints it."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import zkm_amd  # noqa: E402
from oracle.oracle_py import Oracle  # noqa: E402
from tests import segment_ops_fixtures as SF  # noqa: E402

CPU = 1            # position in Table::all()
SCOPES = ("witness_check", "lookup_check", "check_ctls")


def times_ms(fn, reps, sync):
    ts = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts)), "calls": reps}


def measured(ctx, fn, reps):
    """Warm-up, host waits of one call, the times, then launches and milliseconds per scope of one call with the profiler on."""
    fn()
    waits = ctx.host_waits()
    fn()
    res = {"host_waits": ctx.host_waits() - waits}
    res.update(times_ms(fn, reps, ctx.synchronize))
    ctx.profile(True)
    ctx.profile_reset()
    fn()
    ctx.synchronize()
    recs = {k: v for k, v in ctx.profile_records().items() if k.split("/")[0] in SCOPES}
    ctx.profile(False)
    ctx.profile_reset()
    res["launches_by_scope"] = {k: int(v[0]) for k, v in sorted(recs.items())}
    res["scopes_ms"] = {k: round(v[1], 4) for k, v in sorted(recs.items())}
    return res


def refused(fn):
    try:
        fn()
    except zkm_amd.ZkmError as e:
        return str(e)
    return None


def main():
    reps = max(20, int(os.environ.get("REPS", "20")))
    oracle = Oracle()
    ctx = zkm_amd.Context(0)
    raw, tables, _ = SF.build_segment_ops(oracle, repeat=128)
    lg = [t[3] for t in tables]
    out = {"tool": "segment_check_time", "log_heights": lg, "table_bytes": int(sum(t[1].size * 8 for t in tables)),
           "not_measured": ["several contexts sharing the GPU", "tables taller than this segment's", "host-resident tables (the upload)"]}
    bufs = [ctx.alloc(t[1].size).upload(t[1]) for t in tables]
    ptrs = [b.ptr for b in bufs]
    n = 1 << lg[CPU]
    bad_cpu = tables[CPU][1].copy()
    bad_cpu[3 * n + n - 1] = (int(bad_cpu[3 * n + n - 1]) + 1) % zkm_amd.P
    bad_buf = ctx.alloc(bad_cpu.size).upload(bad_cpu)
    bad_ptrs = ptrs[:CPU] + [bad_buf.ptr] + ptrs[CPU + 1:]

    def triples(segs):
        for p, l in segs:
            ctx.segment_witness_check(p, l)
            ctx.segment_lookup_check(p, l)
            ctx.segment_check_ctls(p, l)

    # 1, 2: the call against the per-segment triples
    for k in (1, 8):
        segs = [(ptrs, lg)] * k
        res = measured(ctx, lambda: ctx.segments_check(segs), reps)
        assert ctx.check_message is None and res["host_waits"] == 2, (ctx.check_message, res)
        out["segments_check_k%d" % k] = res
        out["per_segment_triples_k%d" % k] = measured(ctx, lambda: triples(segs), reps)
    segs = [(ptrs, lg)] * 5 + [(bad_ptrs, lg)] + [(ptrs, lg)] * 2
    res = measured(ctx, lambda: ctx.segments_check(segs), reps)
    res["message"] = ctx.check_message
    assert ctx.check_message.startswith("zkm_segments_check: segment 5: Constraint failed in CpuStark"), ctx.check_message
    out["segments_check_k8_segment5_cpu_cell_changed"] = res
    # 3, 4: the gate in front of zkm_prove_segments of 8
    good8 = [(ptrs, lg, ())] * 8
    bad8 = [(ptrs, lg, ())] * 5 + [(bad_ptrs, lg, ())] + [(ptrs, lg, ())] * 2
    gate = {}
    for name, keys in (("off", {}), ("check_witness", {"check_witness": 1}), ("check_ctls", {"check_ctls": 1})):
        for key, value in keys.items():
            ctx.set_tuning(key, value)
        try:
            ctx.prove_segments(good8)                       # warm-up
            gate[name] = times_ms(lambda: ctx.prove_segments(good8), reps, ctx.synchronize)
            msg = refused(lambda: ctx.prove_segments(bad8))
            gate[name + "_segment5_cpu_cell_changed"] = dict(times_ms(lambda: refused(lambda: ctx.prove_segments(bad8)), reps, ctx.synchronize), message=msg)
        finally:
            for key in keys:
                ctx.set_tuning(key, 0)
    assert gate["check_witness_segment5_cpu_cell_changed"]["message"].startswith("check_witness: segment 5: Constraint failed in CpuStark")
    out["prove_segments_k8"] = gate
    for b in bufs + [bad_buf]:
        b.free()
    ctx.close()
    path = os.path.join(ROOT, "profiles", "segment_check_time.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
