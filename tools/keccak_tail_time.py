#!/usr/bin/env python3
"""tools/keccak_tail_time.py -- a segment of SYSKECCAK calls of arbitrary byte lengths proven both ways on one context, in alternating
calls (modelled on tools/keccak_calls_time.py):
  composed   Context.calls_expand (zkm_keccak_calls_witness, csrc/keccak_calls.hip: every call carries ZKM_SPONGE_PADDED_TAIL, rows and
             lists are written on the device from the KeccakSponge table's lists) and then zkm_prove_segments_ops_steps on its blocks;
  host       zkm_prove_segments_ops_steps fed the host-expanded RAW rows and lists in pinned memory -- what a recorder does with a call
             whose length is no multiple of 4 when the library refuses it.
The segment: 2^LOG_CYCLES cycles (default 16), NCALLS calls (default 1,600) whose lengths are drawn uniformly from 1 .. 600 with a fixed
seed, at disjoint addresses on seeded random bytes, back to back from clock 0, PAD-filled behind them; the call count keeps the
KeccakStark table at 2^17 rows or less (asserted).  The host-expanded arrays come from the test model (tests/keccak_tail_model.py);
the device's outputs are compared with them word for word on the way.
Prints one JSON object (and writes it to the path behind --out):
  lengths             how many calls, how many of them no multiple of 4, the sum of their bytes, the KeccakStark rows
  bytes_per_segment   what crosses the link both ways (the host-expanded figure asserted to be the sum of the generators' per-call
                      figures: (R + 2) rows of 2,072 bytes, L reads of 48, 34 B XORs of 12, B Keccak-f inputs of 208), and the ratio
  prove               ms per proving call, both ways: median, min, max over REPS (default 7) alternating calls; composed includes the
                      expansion call
  expand              ms of calls_expand alone, and the kernel's device ms (profile scope keccak_calls/rows_lists)
  no_slower           the bar: composed's median lies at or below the host-expanded call's own maximum (and whether it lies inside
                      that call's [min, max])
One context does not load the link as eight do: what the saved upload is worth under load is NOT measured here, nor is the pool."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import zkm_amd  # noqa: E402
from tests import keccak_calls_model as K  # noqa: E402
from tests import keccak_tail_model as TM  # noqa: E402

LOG_CYCLES = int(os.environ.get("LOG_CYCLES", "16"))
NCALLS = int(os.environ.get("NCALLS", "1600"))
PAD, RAW = zkm_amd.STEP["PAD"], zkm_amd.STEP["RAW"]


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "calls": len(ms)}


def pin(ctx, a):
    p = ctx.pinned_array((a.nbytes + 7) // 8)
    p.view(np.uint8)[:a.nbytes] = a.reshape(-1).view(np.uint8)
    return p.view(np.uint8)[:a.nbytes].view(a.dtype).reshape(a.shape)


def calls(ncalls, seed=1):
    """ncalls calls of 1 .. 600 bytes, back to back in time from clock 0, every one flagged."""
    rng = np.random.default_rng(seed)
    lengths = rng.integers(1, 601, ncalls)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    rows = ((lengths + 3) // 4 + 7) // 8 + 2
    first = np.concatenate([[0], np.cumsum(rows)[:-1]])
    k = np.arange(ncalls, dtype=np.uint64)
    sponge_clock = (first + rows - 2).astype(np.uint64)
    meta = np.stack([0 * k, 0 * k, (0x100000 + 0x400 * k) | np.uint64(TM.FLAG | TM.TAIL), 10 * sponge_clock], axis=1)
    return lengths, (rng.integers(0, 256, int(off[-1]), dtype=np.uint8), off, np.ascontiguousarray(meta), 0x4000000 + 0x40 * k)


def main():
    reps = int(os.environ.get("REPS", "7"))
    ctx = zkm_amd.Context(int(os.environ.get("ZKM_BENCH_DEVICE", "0")))
    n = 1 << LOG_CYCLES
    lengths, kc = calls(NCALLS)
    inputs, off, meta, daddrs = kc
    rows, mem, logic, perms = zkm_amd.keccak_calls_counts(off, meta)
    assert (rows, mem, logic, perms) == TM.counts([int(L) for L in lengths])
    assert rows < n and 24 * perms <= 1 << 17, "the calls fit the cycles, and KeccakStark stays at 2^17 rows or less"
    steps = np.zeros(n, dtype=zkm_amd.CPU_STEP_DT)
    steps["kind"] = PAD
    steps["kind"][:rows] = RAW                 # placeholders: calls_expand / the records below take their place
    bare = zkm_amd.CpuSteps(steps)
    records, clocks = zkm_amd.keccak_calls_steps(off, meta, raw_base=0)
    assert clocks.tolist() == list(range(rows))
    # host-expanded: the model's rows and lists; the device's outputs equal them word for word
    t0 = time.perf_counter()
    x = TM.expand(*kc)
    x_rows, x_mem, x_logic, x_in, x_ts = x.arrays()
    model_s = time.perf_counter() - t0
    want_records, want_clocks = K.steps(x, raw_base=0)
    assert records.tobytes() == want_records.tobytes() and (clocks == want_clocks).all()
    device_equals_model = all((g == w).all() for g, w in zip(ctx.keccak_calls_witness(*kc), (x_rows, x_mem, x_logic, x_in, x_ts)))
    host_steps = steps.copy()
    host_steps[clocks.astype(np.int64)] = records
    sponge_p = tuple(pin(ctx, a) for a in kc[:3])
    kc_p = (sponge_p[0], off, sponge_p[2], daddrs)
    host = (zkm_amd.CpuSteps(pin(ctx, host_steps), pin(ctx, x_rows)),
            zkm_amd.SegmentOps(None, pin(ctx, x_mem), logic_ops=pin(ctx, x_logic), keccak=(pin(ctx, x_in), pin(ctx, x_ts)), keccak_sponge=sponge_p))
    expanded = int(x_rows.nbytes + x_mem.nbytes + x_logic.nbytes + x_in.nbytes + x_ts.nbytes)
    assert expanded == sum(sum(TM.call_bytes(int(L))) for L in lengths)
    # input bytes, offsets, metas, digest addresses, the four sums a call
    lists = int(inputs.nbytes + off.nbytes + meta.nbytes + daddrs.astype(np.uint64).nbytes + 32 * NCALLS)
    common = int(steps.nbytes + 12 * ((n + 255) // 256) + inputs.nbytes + off.nbytes + meta.nbytes)   # steps, bases, the sponge group
    nbytes = {"host": {"expanded_rows_and_lists": expanded, "steps_and_sponge_lists": common, "total": expanded + common},
              "composed": {"expansion_call_lists": lists, "steps_and_sponge_lists": common, "total": lists + common},
              "host_over_composed": round((expanded + common) / (lists + common), 2),
              "expanded_over_expansion_call_lists": round(expanded / lists, 2)}
    pubs = [[1, 2, 3]]
    want = ctx.prove_segments_ops_steps([host[0]], [host[1]], public_values=pubs)
    sizes = [o for _, _, o in want]

    def prove_host():
        return ctx.prove_segments_ops_steps([host[0]], [host[1]], public_values=pubs, sizes=sizes)

    t_expand = []

    def prove_composed():
        t0 = time.perf_counter()
        st, ops = ctx.calls_expand(bare, keccak=kc_p)
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
    st, ops = ctx.calls_expand(bare, keccak=kc_p)
    ctx.synchronize()
    recs = ctx.profile_records()
    ctx.profile(False)
    ctx.profile_reset()
    st.raw_rows.free()
    ops.free()
    launches, kernel_ms = recs["keccak_calls/rows_lists"]
    h, s = stats(t["prove_host"]), stats(t["prove_composed"])
    out = {"tool": "keccak_tail_time", "log_cycles": LOG_CYCLES, "reps": reps,
           "lengths": {"calls": NCALLS, "no_multiple_of_4": int(np.count_nonzero(lengths % 4)), "input_bytes": int(lengths.sum()), "min": int(lengths.min()),
                       "max": int(lengths.max()), "cpu_rows": rows, "keccak_perms": perms, "keccak_stark_rows": 24 * perms},
           "bytes_per_segment": nbytes, "prove": {"host": h, "composed": s},
           "expand": dict(stats(expand_ms), kernel={"scope": "keccak_calls/rows_lists", "launches": launches, "ms": round(kernel_ms, 4)}),
           "no_slower": {"host_min_ms": h["min_ms"], "host_max_ms": h["max_ms"], "composed_median_ms": s["median_ms"],
                         "composed_minus_host_median_ms": round(s["median_ms"] - h["median_ms"], 3),
                         "inside_host_min_max": bool(h["min_ms"] <= s["median_ms"] <= h["max_ms"]), "holds": bool(s["median_ms"] <= h["max_ms"])},
           "equal_proof_words": bool(same), "device_outputs_equal_the_model": bool(device_equals_model), "model_seconds": round(model_s, 1),
           "not_measured": "several contexts sharing the link (one context does not load it as eight do); the pool"}
    print(json.dumps(out))
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
