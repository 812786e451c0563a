#!/usr/bin/env python3
"""tools/segment_ops_time.py -- a whole segment's tables from its raw operations (zkm_segment_tables, csrc/segment_ops.hip) against the
path a caller takes without it, at the tools/bench_segment.HEIGHTS shapes (2^16 and 2^20 cycles), random valid operations per table
(tests/segment_ops_fixtures.random_segment_ops):
  (a) today:   the eleven per-table witness calls (Memory and Arithmetic sized, then filled), the CPU rows transposed in numpy and uploaded;
  (b) zkm_segment_tables with every list in pinned host memory;
  (c) zkm_segment_tables with every list in device memory;
  (d) zkm_segment_stage of the twelve tables from pinned host memory, the upload only.
Also: the bytes each path moves over the link, the pinned upload of the CPU rows alone, and the transpose kernel's rate on
device-resident rows (2 x 259 x 8 B per row, from the context's event profile of (c)).  Every shape is warmed up first; call times
are medians of `reps` calls with a device synchronise and the profiler off.  (b) and (c) are checked word for word against (a).
Prints one JSON object."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import zkm_amd  # noqa: E402
from tests import segment_ops_fixtures as SF  # noqa: E402
from tools.bench_segment import HEIGHTS  # noqa: E402

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


def today(ctx, raw, lg):
    """(a): DeviceBuffers of the twelve tables, Table::all() order."""
    out = [ctx.arithmetic_trace(raw["arithmetic"])[0], None, ctx.poseidon_trace_inputs(*raw["poseidon"], lg[2]),
           ctx.poseidon_sponge_trace(*raw["poseidon_sponge"], lg[3])[0], ctx.keccak_trace(*raw["keccak"], lg[4]),
           ctx.keccak_sponge_trace(*raw["keccak_sponge"], lg[5])[0], ctx.sha_extend_trace(*raw["sha_extend"], lg[6]),
           ctx.sha_extend_sponge_trace(*raw["sha_extend_sponge"], lg[7]), ctx.sha_compress_trace(*raw["sha_compress"], lg[8]),
           ctx.sha_compress_sponge_trace(*raw["sha_compress_sponge"], lg[9]), ctx.logic_trace(raw["logic"], lg[10]),
           ctx.memory_trace(raw["memory"])[0]]
    cols = np.ascontiguousarray(SF.canonical(raw["cpu_rows"]).T)
    out[1] = ctx.alloc(cols.size).upload(cols)
    return out


def ops_bytes(ops):
    return int(sum(v.nbytes for k, v in ops.lists.items() if isinstance(v, np.ndarray)))


def view(ctx, ptr, words):
    b = zkm_amd.DeviceBuffer.__new__(zkm_amd.DeviceBuffer)
    b.ctx, b.words, b.ptr = ctx, words, ptr
    return b


def shape(ctx, log_cycles, reps):
    lg = HEIGHTS[log_cycles]
    raw = SF.random_segment_ops(lg, seed=17)
    ops = SF.segment_ops(zkm_amd, raw)
    pinned = ops.to_pinned(ctx)
    dev = ops.to_device(ctx)
    sync = ctx.synchronize
    # warm-up of every path, and the words: (b) and (c) == (a)
    a = today(ctx, raw, lg)
    sb, lg_b = ctx.segment_tables(pinned)
    sc, lg_c = ctx.segment_tables(dev)
    assert lg_b == lg_c == lg, (lg_b, lg_c, lg)
    same = True
    for t in range(12):
        want = a[t].download()
        for s in (sb, sc):
            same &= bool((view(ctx, s.tables()[t], WIDTHS[t] << lg[t]).download() == want).all())
        del want
    host_tables = []
    for t in range(12):
        h = ctx.pinned_array(WIDTHS[t] << lg[t])
        h[:] = a[t].download()
        host_tables.append(h)
    for b in a:
        b.free()
    sb.free()
    sc.free()

    def run_a():
        for b in today(ctx, raw, lg):
            b.free()

    def run_seg(o):
        ctx.segment_tables(o)[0].free()

    def run_d():
        ctx.stage_segment(host_tables, lg).free()
    cpu_dev = ctx.alloc(raw["cpu_rows"].size)
    cpu_pinned = pinned.lists["cpu_rows"]
    res = {"log_heights": lg,
           "a_today_ms": median_ms(run_a, reps, sync),
           "b_segment_tables_pinned_ms": median_ms(lambda: run_seg(pinned), reps, sync),
           "c_segment_tables_device_ms": median_ms(lambda: run_seg(dev), reps, sync),
           "d_segment_stage_tables_pinned_ms": median_ms(run_d, reps, sync),
           "cpu_rows_pinned_upload_ms": median_ms(lambda: cpu_dev.upload(cpu_pinned), reps, sync),
           "bytes_over_link": {"a": ops_bytes(ops), "b": ops_bytes(ops), "c": 0, "d": int(sum(h.nbytes for h in host_tables)),
                               "cpu_rows": int(raw["cpu_rows"].nbytes)},
           "b_c_equal_a": same}
    ctx.profile(True)
    ctx.profile_reset()
    for _ in range(reps):
        run_seg(dev)
    recs = ctx.profile_records()
    ctx.profile(False)
    n, ms = recs["segment_ops/cpu_rows_to_cols"]
    tr_ms = ms / n
    res["transpose_device_rows_ms"] = tr_ms
    res["transpose_device_rows_GBps"] = 2 * 259 * 8 * (1 << lg[1]) / tr_ms / 1e6
    res["kernels_ms_per_call"] = {k: round(v[1] / reps, 4) for k, v in sorted(recs.items())}
    cpu_dev.free()
    dev.free()
    for h in host_tables:
        ctx.free_pinned(h)
    for k, v in pinned.lists.items():
        if not k.endswith("_off"):
            ctx.free_pinned(v)
    return res


def main():
    reps = int(os.environ.get("REPS", "5"))
    shapes = [int(x) for x in os.environ.get("SHAPES", "16,20").split(",")]
    ctx = zkm_amd.Context(0)
    out = {"tool": "segment_ops_time", "reps": reps}
    for k in shapes:
        out["2^%d" % k] = shape(ctx, k, reps if k <= 16 else max(2, reps // 2))
        ctx.trim()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
