#!/usr/bin/env python3
"""tools/keccak_calls_time.py -- a segment of SYSKECCAK precompile calls proven both ways on one context, in alternating calls:
  composed   Context.calls_expand (zkm_keccak_calls_witness, csrc/keccak_calls.hip: rows and lists written on the device from the
             KeccakSponge table's lists) and then zkm_prove_segments_ops_steps on its device blocks;
  host       zkm_prove_segments_ops_steps fed the host-expanded rows and lists in pinned memory.
The segment: 2^LOG_CYCLES cycles (default 16) of alternating calls of 64 and of 1,024 input bytes at disjoint addresses on seeded random
bytes, PAD-filled; it does nothing but hash.  The host-expanded arrays come from the test model (tests/keccak_calls_model.py, a minute
of Python integers before the clock); the device's outputs are compared with them word for word on the way.
Prints one JSON object (and writes it to the path behind --out):
  bytes_per_call / bytes_per_segment   what the expansion saves from crossing the link, per call of either length (asserted to be the
                                       figures derived from the generators: (R + 2) rows of 2,072 bytes, L reads of 48, 34 B XORs of 12,
                                       B Keccak-f inputs of 208) and for the segment, both ways
  prove                                ms per proving call, both ways: median, min, max over REPS (default 7) alternating calls; composed
                                       includes the expansion call
  expand                               ms of calls_expand alone (allocations, zkm_keccak_calls_witness), and the kernel's device ms
                                       (profile scope keccak_calls/rows_lists)
  no_slower                            the bar: composed's median is at most host's median plus host's own min-to-max spread
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

LOG_CYCLES = int(os.environ.get("LOG_CYCLES", "16"))
PAD, RAW = zkm_amd.STEP["PAD"], zkm_amd.STEP["RAW"]
SHORT, LONG = 64, 1024
ROWS = {L: (L // 4 + 7) // 8 + 2 for L in (SHORT, LONG)}


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "calls": len(ms)}


def pin(ctx, a):
    p = ctx.pinned_array((a.nbytes + 7) // 8)
    p.view(np.uint8)[:a.nbytes] = a.reshape(-1).view(np.uint8)
    return p.view(np.uint8)[:a.nbytes].view(a.dtype).reshape(a.shape)


def calls(pairs, seed=1):
    """`pairs` calls of 64 bytes and as many of 1,024, alternating in time from clock 0: pair k takes clocks [38 k, 38 k + 38) -- the
    short call's two read rows, sponge row and write row, then the long call's 32 + 2."""
    rng = np.random.default_rng(seed)
    span = ROWS[SHORT] + ROWS[LONG]
    lengths = np.tile([SHORT, LONG], pairs)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    k = np.repeat(np.arange(pairs, dtype=np.uint64), 2)
    long_ = np.tile(np.array([0, 1], dtype=np.uint64), pairs)
    sponge_clock = span * k + np.where(long_ == 1, ROWS[SHORT] + ROWS[LONG] - 2, ROWS[SHORT] - 2).astype(np.uint64)
    meta = np.stack([0 * k, 0 * k, (0x100000 + 0x800 * k + 0x100 * long_) | np.uint64(K.FLAG), 10 * sponge_clock], axis=1)
    return rng.integers(0, 256, int(off[-1]), dtype=np.uint8), off, np.ascontiguousarray(meta), 0x4000000 + 0x40 * k + 0x20 * long_


def main():
    reps = int(os.environ.get("REPS", "7"))
    ctx = zkm_amd.Context(int(os.environ.get("ZKM_BENCH_DEVICE", "0")))
    n = 1 << LOG_CYCLES
    pairs = (n - 1) // (ROWS[SHORT] + ROWS[LONG])              # at least one PAD row, as simulate_cpu pushes
    kc = calls(pairs)
    inputs, off, meta, daddrs = kc
    rows, mem, logic, perms = zkm_amd.keccak_calls_counts(off)
    # the step list: the calls' RAW records at their clocks, PAD behind them
    steps = np.zeros(n, dtype=zkm_amd.CPU_STEP_DT)
    steps["kind"] = PAD
    steps["kind"][:rows] = RAW                 # placeholders: calls_expand / the records below take their place
    bare = zkm_amd.CpuSteps(steps)
    records, clocks = zkm_amd.keccak_calls_steps(off, meta, raw_base=0)
    assert clocks.tolist() == list(range(rows))
    # host-expanded: the model's rows and lists; the device's outputs equal them word for word
    t0 = time.perf_counter()
    x = K.expand(*kc)
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
    per_call = {}
    for L in (SHORT, LONG):
        r, m, lg, p = K.call_bytes(L)
        B = L // 136 + 1
        assert (r, m, lg, p) == (ROWS[L] * 2072, L * 48, 34 * B * 12, B * 208)
        per_call[str(L)] = {"cpu_rows": r, "memory_ops": m, "logic_ops": lg, "keccak_perms": p, "total": r + m + lg + p,
                            "composed": L + 8 + 32 + 8 + 32}                 # input bytes, offset, meta, digest address, the four sums
    assert per_call["64"]["total"] == 8288 + 3072 + 408 + 208 == 11976 and per_call["1024"]["total"] == 70448 + 49152 + 3264 + 1664 == 124528
    expanded = int(x_rows.nbytes + x_mem.nbytes + x_logic.nbytes + x_in.nbytes + x_ts.nbytes)
    assert expanded == pairs * (per_call["64"]["total"] + per_call["1024"]["total"])
    lists = int(inputs.nbytes + off.nbytes + meta.nbytes + daddrs.astype(np.uint64).nbytes + 32 * 2 * pairs)
    assert lists == pairs * (per_call["64"]["composed"] + per_call["1024"]["composed"]) + 8
    common = int(steps.nbytes + 12 * ((n + 255) // 256) + inputs.nbytes + off.nbytes + meta.nbytes)   # steps, bases, the sponge group
    nbytes = {"calls": {"64": pairs, "1024": pairs}, "host": {"expanded_rows_and_lists": expanded, "steps_and_sponge_lists": common, "total": expanded + common},
              "composed": {"expansion_call_lists": lists, "steps_and_sponge_lists": common, "total": lists + common}}
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
    out = {"tool": "keccak_calls_time", "log_cycles": LOG_CYCLES, "reps": reps, "bytes_per_call": per_call, "bytes_per_segment": nbytes,
           "prove": {"host": h, "composed": s},
           "expand": dict(stats(expand_ms), kernel={"scope": "keccak_calls/rows_lists", "launches": launches, "ms": round(kernel_ms, 4)}),
           "no_slower": {"host_spread_ms": round(h["max_ms"] - h["min_ms"], 3), "composed_minus_host_median_ms": round(s["median_ms"] - h["median_ms"], 3),
                         "holds": bool(s["median_ms"] <= h["median_ms"] + (h["max_ms"] - h["min_ms"]))},
           "equal_proof_words": bool(same), "device_outputs_equal_the_model": bool(device_equals_model), "model_seconds": round(model_s, 1),
           "not_measured": "several contexts sharing the link (one context does not load it as eight do); the pool"}
    print(json.dumps(out))
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
