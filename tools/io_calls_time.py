#!/usr/bin/env python3
"""tools/io_calls_time.py -- a segment whose first half is one large hint read, proven both ways on one context, in alternating calls:
  composed   Context.calls_expand(io=...) (zkm_io_calls_witness, csrc/io_calls.hip: the rows written on the device from the call's bytes)
             and then zkm_prove_segments_ops_steps on its device block;
  host       zkm_prove_segments_ops_steps fed the host-expanded RAW rows in pinned memory.
The segment: 2^LOG_CYCLES cycles (default 16); its first 2^(LOG_CYCLES - 1) rows are ONE hint read of 2^(LOG_CYCLES + 4) seeded random
bytes (1 MiB: 32,768 rows of eight words), PAD-filled behind.  The host-expanded rows come from the test model
(tests/io_calls_model.py, Python integers, before the clock); the device's rows are compared with them word for word on the way.
Prints one JSON object (and writes it to the path behind --out):
  bytes      what crosses the link for the I/O call, either way (asserted to be the derivable figures: rows x 2,072 bytes of RAW rows
             against the call's bytes plus its 48-byte RAW records and four small lists); nothing comes back in either
  prove      ms per proving call, both ways: median, min, max over REPS (default 7) alternating calls; composed includes the expansion
  expand     ms of calls_expand alone (allocation, zkm_io_calls_witness), and the kernel's device ms (profile scope io_calls/rows) with
             the rate it writes at
  no_slower  the bar: composed's median is at most host's median plus host's own min-to-max spread
One context does not load the link as eight do: the 8 x 8 shape and the pool are NOT measured here."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import zkm_amd  # noqa: E402
from tests import io_calls_model as IO  # noqa: E402

LOG_CYCLES = int(os.environ.get("LOG_CYCLES", "16"))
PAD, RAW = zkm_amd.STEP["PAD"], zkm_amd.STEP["RAW"]
ROW_BYTES = 259 * 8


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "calls": len(ms)}


def pin(ctx, a):
    p = ctx.pinned_array((a.nbytes + 7) // 8)
    p.view(np.uint8)[:a.nbytes] = a.reshape(-1).view(np.uint8)
    return p.view(np.uint8)[:a.nbytes].view(a.dtype).reshape(a.shape)


def main():
    reps = int(os.environ.get("REPS", "7"))
    ctx = zkm_amd.Context(int(os.environ.get("ZKM_BENCH_DEVICE", "0")))
    n = 1 << LOG_CYCLES
    nbytes = 32 * (n // 2)                                     # eight words a row, half the segment
    rng = np.random.default_rng(1)
    io = IO.lists([(IO.HINT_READ, rng.integers(0, 256, nbytes, dtype=np.uint8).tobytes(), (0, 0, 0x100000, 0))])
    kinds, data, off, meta = io
    rows, mem = zkm_amd.io_calls_counts(kinds, off)
    assert rows == n // 2 and mem == nbytes // 4
    # the step list: the call's RAW records at their clocks, PAD behind them
    steps = np.zeros(n, dtype=zkm_amd.CPU_STEP_DT)
    steps["kind"] = PAD
    steps["kind"][:rows] = RAW                 # placeholders: calls_expand / the records below take their place
    bare = zkm_amd.CpuSteps(steps)
    records, clocks = zkm_amd.io_calls_steps(kinds, off, meta, raw_base=0)
    assert clocks.tolist() == list(range(rows))
    # host-expanded: the model's rows; the device's rows equal them word for word
    t0 = time.perf_counter()
    x = IO.expand(*io)
    x_rows = x.array()
    model_s = time.perf_counter() - t0
    want_records, want_clocks = IO.steps(x, raw_base=0)
    assert records.tobytes() == want_records.tobytes() and (clocks == want_clocks).all()
    device_equals_model = bool((ctx.io_calls_witness(*io) == x_rows).all())
    host_steps = steps.copy()
    host_steps[clocks.astype(np.int64)] = records
    io_p = (kinds, pin(ctx, data), off, meta)
    host = (zkm_amd.CpuSteps(pin(ctx, host_steps), pin(ctx, x_rows)), zkm_amd.SegmentOps(None, None))
    assert x_rows.nbytes == rows * ROW_BYTES
    lists = int(kinds.nbytes + off.nbytes + meta.nbytes + 8 * (len(kinds) + 1))          # kinds, offsets, meta, the row offsets
    link = {"call_bytes": int(nbytes), "rows": int(rows),
            "host": {"raw_rows": int(x_rows.nbytes), "raw_records": int(records.nbytes), "total": int(x_rows.nbytes + records.nbytes)},
            "composed": {"data": int(data.nbytes), "raw_records": int(records.nbytes), "lists": lists, "total": int(data.nbytes + records.nbytes + lists)},
            "device_to_host": 0,
            "other_steps_either_way": int(steps.nbytes - records.nbytes + 12 * ((n + 255) // 256))}
    if LOG_CYCLES == 16:
        assert link["host"]["raw_rows"] == 67895296 and link["composed"]["data"] == 1 << 20 and link["composed"]["raw_records"] == 3 << 19
    pubs = [[1, 2, 3]]
    want = ctx.prove_segments_ops_steps([host[0]], [host[1]], public_values=pubs)
    sizes = [o for _, _, o in want]

    def prove_host():
        return ctx.prove_segments_ops_steps([host[0]], [host[1]], public_values=pubs, sizes=sizes)

    t_expand = []

    def prove_composed():
        t0 = time.perf_counter()
        st, ops = ctx.calls_expand(bare, io=io_p)
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
    st, ops = ctx.calls_expand(bare, io=io_p)
    ctx.synchronize()
    recs = ctx.profile_records()
    ctx.profile(False)
    ctx.profile_reset()
    st.raw_rows.free()
    ops.free()
    launches, kernel_ms = recs["io_calls/rows"]
    h, s = stats(t["prove_host"]), stats(t["prove_composed"])
    out = {"tool": "io_calls_time", "log_cycles": LOG_CYCLES, "reps": reps, "bytes_over_the_link": link,
           "prove": {"host": h, "composed": s},
           "expand": dict(stats(expand_ms), kernel={"scope": "io_calls/rows", "launches": launches, "ms": round(kernel_ms, 4),
                                                    "written_gb_per_s": round(x_rows.nbytes / (kernel_ms * 1e6), 1) if kernel_ms else None}),
           "no_slower": {"host_spread_ms": round(h["max_ms"] - h["min_ms"], 3), "composed_minus_host_median_ms": round(s["median_ms"] - h["median_ms"], 3),
                         "holds": bool(s["median_ms"] <= h["median_ms"] + (h["max_ms"] - h["min_ms"]))},
           "equal_proof_words": bool(same), "device_rows_equal_the_model": device_equals_model, "model_seconds": round(model_s, 1),
           "not_measured": "the 8 x 8 shape (several contexts sharing the link: one context does not load it as eight do); the pool"}
    print(json.dumps(out))
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
