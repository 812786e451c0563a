#!/usr/bin/env python3
"""tools/witness_check_time.py -- zkm_segment_witness_check (csrc/witness_check.hip) on device-resident tables against what it
replaces, on one GPU, for the consistent 2^16-cycle twelve-table segment of tests/segment_ops_fixtures.build_segment_ops(oracle,
repeat=128) (Arithmetic 2^16 rows, Cpu 2^15, Memory 2^17):
  the segment call: median, minimum and maximum of `REPS` (at least 10) calls after a warm-up, profiler off; its host waits; its two
  groups of launches by profile scope (a second set of calls, profiler on); the same with one cell of the Cpu table's last row changed
  (the rejecting path: the second launch of that table evaluates the named row);
  what it replaces, in the same run: the download of the twelve tables plus oracle.debug_constraints on each, single-threaded on the
  host -- per table and in total.
NOT measured: several contexts sharing the GPU, tables taller than this segment's, host-resident tables (their upload would dominate).
Writes profiles/witness_check_time.json and prints it."""
import ctypes as C
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


def times_ms(fn, reps, sync):
    ts = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts)), "calls": reps}


def device_call(ctx, ptrs, lg, reps):
    sync = ctx.synchronize
    waits = ctx.host_waits()
    findings = ctx.segment_witness_check(ptrs, lg)                              # warm-up (and the verdict)
    res = {"host_waits": ctx.host_waits() - waits, "message": ctx.witness_message, "failing_tables": sum(f[0] is not None for f in findings),
           "constraints_per_row": [f[4] for f in findings]}
    res.update(times_ms(lambda: ctx.segment_witness_check(ptrs, lg), reps, sync))
    ctx.profile(True)
    ctx.profile_reset()
    for _ in range(reps):
        ctx.segment_witness_check(ptrs, lg)
    sync()
    recs = {k: v for k, v in ctx.profile_records().items() if k.startswith("witness_check/")}
    ctx.profile(False)
    ctx.profile_reset()
    res["scopes_ms_per_call"] = {k: round(v[1] / reps, 4) for k, v in sorted(recs.items())}
    return res, findings


def main():
    reps = max(10, int(os.environ.get("REPS", "20")))
    oracle = Oracle()
    ctx = zkm_amd.Context(0)
    raw, tables, _ = SF.build_segment_ops(oracle, repeat=128)
    lg = [t[3] for t in tables]
    out = {"tool": "witness_check_time", "log_heights": lg, "table_bytes": int(sum(t[1].size * 8 for t in tables)),
           "not_measured": ["several contexts sharing the GPU", "tables taller than this segment's", "host-resident tables (the upload)"]}
    bufs = [ctx.alloc(t[1].size).upload(t[1]) for t in tables]
    ptrs = [b.ptr for b in bufs]
    out["segment_witness_check"], findings = device_call(ctx, ptrs, lg, reps)
    assert all(f[0] is None for f in findings), findings
    # what it replaces: the tables brought down, then the oracle's single-threaded check of each
    t0 = time.perf_counter()
    host = [b.download() for b in bufs]
    out["download_ms"] = (time.perf_counter() - t0) * 1e3
    per_table = {}
    for (tid, _, W, log_n, _), h, f in zip(tables, host, findings):
        t0 = time.perf_counter()
        count, first = oracle.debug_constraints(tid, h, W, log_n)
        per_table[SF.ORDER.index(tid)] = round((time.perf_counter() - t0) * 1e3, 3)
        assert first is None and count == f[4], (tid, first, count, f)
    out["oracle_debug_constraints_ms_by_table"] = per_table
    out["oracle_debug_constraints_ms"] = float(sum(per_table.values()))
    out["download_plus_oracle_ms"] = out["download_ms"] + out["oracle_debug_constraints_ms"]
    # the rejecting path: one cell of the last Cpu row
    n = 1 << lg[CPU]
    cell = 3 * n + n - 1
    word, err = np.array([(int(host[CPU][cell]) + 1) % zkm_amd.P], dtype=np.uint64), C.c_char_p()
    assert ctx.L.zkm_dev_upload(ctx.h, ptrs[CPU] + 8 * cell, word.ctypes.data, 8, C.byref(err)) == 0, err.value
    out["one_cell_changed"], findings = device_call(ctx, ptrs, lg, reps)
    bad = host[CPU].copy()
    bad[cell] = word[0]
    count, first = oracle.debug_constraints(tables[CPU][0], bad, tables[CPU][2], lg[CPU])
    assert first is not None and findings[CPU][:2] == first, (findings[CPU], first)
    for b in bufs:
        b.free()
    ctx.close()
    path = os.path.join(ROOT, "profiles", "witness_check_time.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
