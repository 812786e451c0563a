#!/usr/bin/env python3
"""tools/lookup_check_time.py -- zkm_segment_lookup_check (csrc/lookup_check.hip) on device-resident tables against what it replaces, on
one GPU, for the consistent 2^16-cycle twelve-table segment of tests/segment_ops_fixtures.build_segment_ops(oracle, repeat=128)
(Arithmetic 2^16 rows: 19 x 2^16 records; Memory 2^17: 2 x 2^17) that tools/witness_check_time.py uses:
  the segment call: median, minimum and maximum of `REPS` (at least 10, default 20) calls after a warm-up, profiler off, each timed by the
  host clock between two stream synchronisations; its host waits; its three profile scopes (a second set of calls, profiler on);
  the same with one RC_FREQUENCIES cell changed (the rejecting path);
  what it replaces, in the same run: the download of the two tables with lookups plus the Python model (tests/lookup_model.py) on them.
NOT measured: several contexts sharing the GPU, tables taller than this segment's, host-resident tables (their upload would dominate).
Writes profiles/lookup_check_time.json and prints it."""
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
from tests import lookup_fixtures as LF  # noqa: E402
from tests import lookup_model as LM  # noqa: E402
from tests import segment_ops_fixtures as SF  # noqa: E402

ARITHMETIC, MEMORY = 0, 11            # positions in Table::all()
SHAPES = {ARITHMETIC: LF.ARITHMETIC, MEMORY: LF.MEMORY}


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
    findings = ctx.segment_lookup_check(ptrs, lg)                               # warm-up (and the verdict)
    res = {"host_waits": ctx.host_waits() - waits, "message": ctx.lookup_message, "failing_tables": sum(f[0] is not None for f in findings)}
    res.update(times_ms(lambda: ctx.segment_lookup_check(ptrs, lg), reps, sync))
    ctx.profile(True)
    ctx.profile_reset()
    for _ in range(reps):
        ctx.segment_lookup_check(ptrs, lg)
    sync()
    recs = {k: v for k, v in ctx.profile_records().items() if k.startswith("lookup_check/")}
    ctx.profile(False)
    ctx.profile_reset()
    res["scopes_ms_per_call"] = {k: round(v[1] / reps, 4) for k, v in sorted(recs.items())}
    total = sum(res["scopes_ms_per_call"].values())
    res["scopes_share"] = {k: round(v / total, 4) for k, v in res["scopes_ms_per_call"].items()} if total else {}
    return res, findings


def replaced(bufs, tables):
    """The download of the two tables with lookups, then the model on each: (milliseconds by part, the findings)."""
    out, findings = {}, {}
    t0 = time.perf_counter()
    host = {t: bufs[t].download() for t in SHAPES}
    out["download_ms"] = (time.perf_counter() - t0) * 1e3
    for t, s in SHAPES.items():
        t0 = time.perf_counter()
        findings[t] = LM.finding(host[t].reshape(s.width, -1), *s.lookup())
        out["model_ms_" + s.name] = round((time.perf_counter() - t0) * 1e3, 3)
    out["download_plus_model_ms"] = out["download_ms"] + sum(v for k, v in out.items() if k.startswith("model_ms_"))
    return out, findings


def main():
    reps = max(10, int(os.environ.get("REPS", "20")))
    oracle = Oracle()
    ctx = zkm_amd.Context(0)
    raw, tables, _ = SF.build_segment_ops(oracle, repeat=128)
    lg = [t[3] for t in tables]
    out = {"tool": "lookup_check_time", "log_heights": lg, "records": {s.name: s.records(lg[t]) for t, s in SHAPES.items()},
           "not_measured": ["several contexts sharing the GPU", "tables taller than this segment's", "host-resident tables (the upload)"]}
    bufs = [ctx.alloc(t[1].size).upload(t[1]) for t in tables]
    ptrs = [b.ptr for b in bufs]
    out["segment_lookup_check"], findings = device_call(ctx, ptrs, lg, reps)
    assert findings == [LM.HOLDS] * 12, findings
    out["replaced"], model = replaced(bufs, tables)
    assert all(f == LM.HOLDS for f in model.values()), model
    # the rejecting path: one RC_FREQUENCIES cell
    n, s = 1 << lg[ARITHMETIC], LF.ARITHMETIC
    cell = s.freq_col * n + 1000
    word, err = np.array([(int(tables[ARITHMETIC][1][cell]) + 1) % zkm_amd.P], dtype=np.uint64), C.c_char_p()
    assert ctx.L.zkm_dev_upload(ctx.h, ptrs[ARITHMETIC] + 8 * cell, word.ctypes.data, 8, C.byref(err)) == 0, err.value
    out["one_cell_changed"], findings = device_call(ctx, ptrs, lg, reps)
    out["one_cell_changed_replaced"], model = replaced(bufs, tables)
    assert findings[ARITHMETIC] == model[ARITHMETIC] and findings[ARITHMETIC][1] == 1000 and findings[MEMORY] == LM.HOLDS, (findings, model)
    for b in bufs:
        b.free()
    ctx.close()
    path = os.path.join(ROOT, "profiles", "lookup_check_time.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
