#!/usr/bin/env python3
"""tools/check_ctls_time.py -- zkm_segment_check_ctls (csrc/ctl_check.hip) on device-resident tables against what it replaces and what
it guards, on one GPU:
  "repeat128"  tests/segment_ops_fixtures.build_segment_ops(oracle, repeat=128): a consistent 2^16-row Arithmetic / 2^15-row CPU segment
               (Memory 2^17) -- the accepting path;
  "random16"   the twelve tables zkm_segment_tables builds at the tools/bench_segment.HEIGHTS[16] shape from random_segment_ops:
               inconsistent lookups -- the rejecting path with its report.
Per shape: the device-resident call (median of `REPS` calls after a warm-up, profiler off), its kernels by profile scope with the
sort's share, the host waits, the largest gap between two launches (the host's turn-around at a wait, from the profile's event
times is not available: what is reported is the call time minus the summed kernel time); beside it, in the same run, the download of the twelve
tables plus the oracle's check_ctls on the host's CPUs, and zkm_prove_segment of the same tables.  Writes
profiles/check_ctls_time.json and prints it."""
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
from tools.bench_segment import HEIGHTS  # noqa: E402
from zkm_amd import tables as T  # noqa: E402

WIDTHS = [54, 259, 262, 110, 2431, 470, 78, 76, 224, 127, 69, 13]


def median_ms(fn, reps, sync):
    ts = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def view(ctx, ptr, words):
    b = zkm_amd.DeviceBuffer.__new__(zkm_amd.DeviceBuffer)
    b.ctx, b.words, b.ptr = ctx, words, ptr
    return b


def measure(ctx, oracle, ptrs, lg, reps):
    """ptrs: the twelve device matrices (integers)."""
    sync = ctx.synchronize
    ctl_tables, ctls = T.all_cross_table_lookups()
    rep = ctx.segment_check_ctls(ptrs, lg)                                    # warm-up (and the verdict)
    res = {"log_heights": list(lg), "table_bytes": int(sum(8 * (w << l) for w, l in zip(WIDTHS, lg))),
           "kind": rep.kind, "ctl": rep.ctl, "attempts": rep.attempts, "host_waits": rep.host_waits, "message": (rep.message or "")[:200],
           "check_ctls_device_ms": median_ms(lambda: ctx.segment_check_ctls(ptrs, lg), reps, sync)}
    ctx.profile(True)
    ctx.profile_reset()
    for _ in range(reps):
        ctx.segment_check_ctls(ptrs, lg)
    sync()
    recs = {k: v for k, v in ctx.profile_records().items() if k.startswith("check_ctls/")}
    ctx.profile(False)
    ctx.profile_reset()
    res["kernels_ms_per_call"] = {k: round(v[1] / reps, 4) for k, v in sorted(recs.items())}
    res["launches_per_call"] = {k: v[0] // reps for k, v in sorted(recs.items())}
    total = sum(v[1] for v in recs.values()) / reps
    sort = sum(v[1] for k, v in recs.items() if "radix" in k) / reps
    res["kernels_total_ms"] = round(total, 4)
    res["sort_share_of_kernels"] = round(sort / total, 3) if total else None
    res["not_in_kernels_ms"] = round(res["check_ctls_device_ms"] - total, 4)   # launch gaps and the host's turn-around at the waits
    # what it replaces: the tables brought down, then the oracle's check on the host's CPUs
    host = []
    t0 = time.perf_counter()
    for p, w, l in zip(ptrs, WIDTHS, lg):
        host.append(view(ctx, p, w << l).download())
    res["download_ms"] = (time.perf_counter() - t0) * 1e3
    tables = [(SF.ORDER[i], host[i], WIDTHS[i], lg[i], ctl_tables[i]) for i in range(12)]
    t0 = time.perf_counter()
    code = oracle.check_ctls(tables, ctls)
    res["oracle_check_ctls_ms"] = (time.perf_counter() - t0) * 1e3
    res["oracle_code"] = code
    assert (code == 0) == (rep.kind == 0) and (code == 0 or code % 100 == rep.ctl), (code, rep.kind, rep.ctl)
    # what it guards: the proof of the same tables
    bufs = [view(ctx, p, w << l) for p, w, l in zip(ptrs, WIDTHS, lg)]
    try:
        ctx.prove_segment(bufs, lg)
        res["prove_segment_ms"] = median_ms(lambda: ctx.prove_segment(bufs, lg), max(2, reps // 2), sync)
    except zkm_amd.ZkmError as e:       # (tables whose lookup filters are not 0 / 1 cannot be proven: random CPU rows)
        res["prove_segment_error"] = str(e)[:120]
        return res
    res["check_share_of_proof"] = round(res["check_ctls_device_ms"] / res["prove_segment_ms"], 4)
    return res


def main():
    reps = int(os.environ.get("REPS", "5"))
    oracle = Oracle()
    ctx = zkm_amd.Context(0)
    out = {"tool": "check_ctls_time", "reps": reps}
    raw, tables, _ = SF.build_segment_ops(oracle, repeat=128)
    bufs = [ctx.alloc(t[1].size).upload(t[1]) for t in tables]
    out["repeat128"] = measure(ctx, oracle, [b.ptr for b in bufs], [t[3] for t in tables], reps)
    for b in bufs:
        b.free()
    ctx.trim()
    ops = SF.segment_ops(zkm_amd, SF.random_segment_ops(HEIGHTS[16], seed=17)).to_device(ctx)
    staged, lg = ctx.segment_tables(ops)
    out["random16"] = measure(ctx, oracle, staged.tables(), lg, reps)
    staged.free()
    ops.free()
    ctx.close()
    path = os.path.join(ROOT, "profiles", "check_ctls_time.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
