#!/usr/bin/env python3
"""tools/calls_expand_time.py -- K segments' calls expanded by ONE entry (zkm_segments_calls_expand: one scratch block, at most one launch
per kind and one host wait for all K) against the per-segment, per-kind path in front of it (K x Context.calls_expand: one
zkm_*_witness call, scratch block and host wait per kind and segment), on one context, in alternating calls.
The shape: SEGMENTS (default 8) segments of 2^LOG_CYCLES cycles (default 16), each carrying all four kinds, a quarter of the segment
each, in the call mixes of the four per-kind tools:
  SHA      pairs of one extend and one compress call, 107 rows a pair (tools/sha_calls_time.py)
  Keccak   pairs of a 64-byte and a 1,024-byte call, 38 rows a pair (tools/keccak_calls_time.py)
  I/O      ONE hint read of 32 bytes a row (tools/io_calls_time.py)
  insns    the nineteen-instruction cycle of tools/insn_rows_time.py, recorded once on a tests/insn_rows_model.py InsnRecorder and repeated
PAD steps fill the rest.  Every list is in pinned memory, for both paths.  Prints one JSON object (and writes it to the path behind --out):
  expand     the expansion alone, both ways: ms (median, min, max over REPS, default 7, alternating calls after a warm-up; the outputs are
             freed outside the clock), host waits (zkm_ctx_host_waits), launches per kind scope (the profiler's records) and scratch
             blocks (counted from the calls made: one per group of 32 segments, against one per zkm_*_witness call)
  prove      a proving call including the expansion, both ways: zkm_prove_segments_ops_calls against K x calls_expand and
             zkm_prove_segments_ops_steps on its outputs (sizes given: no sizing call); ms and host waits
  no_slower  the bar, for each of the two: the one-entry median is at most the per-segment median plus that path's own min-to-max spread
  equal      every word of every segment's expansion, and every proof word, equal between the two paths
One context does not load the link as eight do: several contexts on one link and the pool are NOT measured here."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import zkm_amd  # noqa: E402
from tests import insn_rows_model as I  # noqa: E402
from tests import keccak_calls_model as K  # noqa: E402

LOG_CYCLES = int(os.environ.get("LOG_CYCLES", "16"))
SEGMENTS = int(os.environ.get("SEGMENTS", "8"))
PAD, RAW = zkm_amd.STEP["PAD"], zkm_amd.STEP["RAW"]
SHORT, LONG = 64, 1024
KROWS = {L: (L // 4 + 7) // 8 + 2 for L in (SHORT, LONG)}
SCOPES = ("sha_calls/rows_lists", "keccak_calls/rows_lists", "io_calls/rows", "insn_rows/rows")
LISTS = ("raw_rows", "memory_ops", "logic_ops", "keccak_inputs", "keccak_timestamps", "sha_extend_inputs", "sha_extend_timestamps", "arithmetic_ops")


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "calls": len(ms)}


def pin(ctx, a):
    p = ctx.pinned_array((a.nbytes + 7) // 8)
    p.view(np.uint8)[:a.nbytes] = a.reshape(-1).view(np.uint8)
    return p.view(np.uint8)[:a.nbytes].view(a.dtype).reshape(a.shape)


def sha_calls(pairs, clock0, rng):
    k = np.arange(pairs, dtype=np.uint64)
    emeta = np.stack([0 * k, 0 * k, 0x100000 + 0x100 * k, 10 * (clock0 + 107 * k + 1)], axis=1)
    cmeta = np.stack([0 * k, 0 * k, 0x4000000 + 0x20 * k, 10 * (clock0 + 107 * k + 96 + 9), 0x8000000 + 0x100 * k, 0 * k, 0 * k, 0 * k], axis=1)
    u32 = lambda *shape: rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)
    return (u32(pairs, 16), np.ascontiguousarray(emeta)), (u32(pairs, 8), u32(pairs, 64), np.ascontiguousarray(cmeta))


def keccak_calls(pairs, clock0, rng):
    span = KROWS[SHORT] + KROWS[LONG]
    off = np.concatenate([[0], np.cumsum(np.tile([SHORT, LONG], pairs))]).astype(np.uint64)
    k = np.repeat(np.arange(pairs, dtype=np.uint64), 2)
    long_ = np.tile(np.array([0, 1], dtype=np.uint64), pairs)
    sponge_clock = clock0 + span * k + np.where(long_ == 1, span - 2, KROWS[SHORT] - 2).astype(np.uint64)
    meta = np.stack([0 * k, 0 * k, (0x100000 + 0x800 * k + 0x100 * long_) | np.uint64(K.FLAG), 10 * sponge_clock], axis=1)
    return rng.integers(0, 256, int(off[-1]), dtype=np.uint8), off, np.ascontiguousarray(meta), 0x4000000 + 0x40 * k + 0x20 * long_


def insn_cycle():
    """The records of insn_rows_time's nineteen-instruction cycle, recorded once."""
    m = I.InsnRecorder()
    for reg, v in {8: 0xFFFFFFF9, 9: 2, 10: 0x80000000, 11: 0x7FFFFFFF, 12: 0x12345678, 22: 0x10C, I.REG_LO: 5, I.REG_HI: 6}.items():
        m.set_reg(reg, v)
    for op in (lambda: I.lui(m, 0, 16, 0x1234), lambda: I.binary(m, "MUL", 8, 9, 17), lambda: I.lui(m, 0, 18, 0x8765), lambda: I.binary(m, "MUL", 12, 11, 19),
               lambda: I.hilo(m, "MULT", 8, 10), lambda: I.binary(m, "MFLO", rd=20), lambda: I.lui(m, 0, 16, 0xFFFF), lambda: I.hilo(m, "MULTU", 12, 11),
               lambda: I.binary(m, "MFHI", rd=21), lambda: I.binary(m, "MUL", 16, 18, 17), lambda: I.hilo(m, "DIV", 8, 9), lambda: I.binary(m, "MFLO", rd=20),
               lambda: I.hilo(m, "DIVU", 12, 9), lambda: I.binary(m, "MFHI", rd=21), lambda: I.binary(m, "MTHI", rs=12), lambda: I.binary(m, "MTLO", rs=11),
               lambda: I.sdc1(m, 22, 12, 0xFFF4), lambda: I.nop_like(m, "SYNC"), lambda: I.nop_like(m, "PREF", rs=22, imm=8)):
        op()
    return m.insn_lists()[0]


def segment(ctx, seed, cycle):
    """The arguments calls_expand and SegmentCalls take for one segment, every list pinned; and what it holds."""
    n = 1 << LOG_CYCLES
    q = n // 4
    rng = np.random.default_rng(seed)
    spairs, kpairs = q // 107, q // (KROWS[SHORT] + KROWS[LONG])
    e, c = sha_calls(spairs, 0, rng)
    kc = keccak_calls(kpairs, q, rng)
    io = (np.array([zkm_amd.IO_KINDS["hint_read"]], dtype=np.uint32), rng.integers(0, 256, 32 * q, dtype=np.uint8), np.array([0, 32 * q], dtype=np.uint64),
          np.array([[0, 0, 0x10000000, 10 * 2 * q]], dtype=np.uint64))
    ninsns = q - 1                                                  # at least one PAD row, as simulate_cpu pushes
    records = np.tile(cycle, ninsns // len(cycle) + 1)[:ninsns]
    clocks = (3 * q + np.arange(ninsns)).astype(np.uint64)
    steps = np.zeros(n, dtype=zkm_amd.CPU_STEP_DT)
    steps["kind"] = PAD
    for lo, rows in ((0, 107 * spairs), (q, (KROWS[SHORT] + KROWS[LONG]) * kpairs), (2 * q, q), (3 * q, ninsns)):
        steps["kind"][lo:lo + rows] = RAW                           # placeholders: the calls' records take their place
    kw = dict(steps=zkm_amd.CpuSteps(pin(ctx, steps)), first_clock=0, extend=tuple(pin(ctx, a) for a in e), compress=tuple(pin(ctx, a) for a in c),
              keccak=tuple(pin(ctx, np.ascontiguousarray(a)) for a in kc), io=(io[0], pin(ctx, io[1]), io[2], io[3]),
              insns=(pin(ctx, records), pin(ctx, clocks)))
    holds = {"sha_pairs": int(spairs), "keccak_pairs": int(kpairs), "io_bytes": int(32 * q), "instructions": int(ninsns)}
    return kw, holds


def downloaded(ctx, steps, ops, insns=True):
    """calls_expand's outputs as ExpandedCalls.download gives them."""
    c = ops.counts
    words = lambda name: ops.lists[name].download()
    got = {"steps": steps.steps, "raw_rows": steps.raw_rows.download()[:steps.nraw * 259].reshape(-1, 259), "memory_ops": words("memory_ops")[:c["nmemory"] * 6].reshape(-1, 6),
           "logic_ops": words("logic_ops").view(np.uint32)[:c["nlogic"] * 3].reshape(-1, 3), "keccak_inputs": words("keccak_inputs")[:c["nkeccak"] * 25].reshape(-1, 25),
           "keccak_timestamps": words("keccak_timestamps")[:c["nkeccak"]], "sha_extend_inputs": words("sha_extend_inputs").view(np.uint8)[:c["nsha_extend"] * 16].reshape(-1, 16),
           "sha_extend_timestamps": words("sha_extend_timestamps")[:c["nsha_extend"]],
           "arithmetic_ops": words("arithmetic_ops").view(np.uint32)[:c["narithmetic"] * 3].reshape(-1, 3)}
    return got


def main():
    reps = int(os.environ.get("REPS", "7"))
    assert reps >= 7, "at least 7 calls each"
    ctx = zkm_amd.Context(int(os.environ.get("ZKM_BENCH_DEVICE", "0")))
    cycle = insn_cycle()
    built = [segment(ctx, 100 + s, cycle) for s in range(SEGMENTS)]
    kws = [kw for kw, _ in built]
    calls = [zkm_amd.SegmentCalls(**kw) for kw in kws]
    counts = zkm_amd.segment_calls_steps(calls[0])[1]
    pubs = [[1, 2, 3 + s] for s in range(SEGMENTS)]

    def free_pairs(pairs):
        for st, ops in pairs:
            st.raw_rows.free()
            ops.free()

    def expand_one_entry():
        return ctx.segments_calls_expand(calls)

    def expand_per_segment():
        return [ctx.calls_expand(**kw) for kw in kws]

    # every word equal between the two paths
    x, pairs = expand_one_entry(), expand_per_segment()
    equal_words = True
    for s, (st, ops) in enumerate(pairs):
        got, want = x.download(s), downloaded(ctx, st, ops)
        equal_words = equal_words and all(got[name].shape == want[name].shape and bool((got[name] == want[name]).all()) for name in LISTS) \
            and got["steps"].tobytes() == want["steps"].tobytes()
    want_proofs = ctx.prove_segments_ops_steps([st for st, _ in pairs], [ops for _, ops in pairs], public_values=pubs)
    sizes = [o for _, _, o in want_proofs]
    x.free()
    free_pairs(pairs)

    def prove_one_entry():
        return ctx.prove_segments_ops_calls(calls, public_values=pubs, sizes=sizes)

    def prove_per_segment():
        pairs = expand_per_segment()
        try:
            return ctx.prove_segments_ops_steps([st for st, _ in pairs], [ops for _, ops in pairs], public_values=pubs, sizes=sizes)
        finally:
            free_pairs(pairs)

    def release(out):
        if isinstance(out, zkm_amd.ExpandedCalls):
            out.free()
        elif out and isinstance(out[0][0], zkm_amd.CpuSteps):
            free_pairs(out)

    fns = (expand_per_segment, expand_one_entry, prove_per_segment, prove_one_entry)
    for fn in fns * 2:                                              # the warm-up
        release(fn())
    t, waits = {fn.__name__: [] for fn in fns}, {}
    for _ in range(reps):                                           # alternating: what drifts in the process drifts for both
        for fn in fns:
            ctx.synchronize()
            w0 = ctx.host_waits()
            t0 = time.perf_counter()
            out = fn()
            ms = (time.perf_counter() - t0) * 1e3
            waits[fn.__name__] = ctx.host_waits() - w0
            ctx.synchronize()
            t[fn.__name__].append(ms)
            release(out)
    got_proofs = prove_one_entry()
    equal_proofs = all((p == wp).all() and (ch == wch).all() and o == wo for (p, ch, o), (wp, wch, wo) in zip(got_proofs, want_proofs))
    launches = {}
    for fn in (expand_per_segment, expand_one_entry):
        ctx.profile(True)
        ctx.profile_reset()
        out = fn()
        ctx.synchronize()
        recs = ctx.profile_records()
        ctx.profile(False)
        ctx.profile_reset()
        release(out)
        launches[fn.__name__] = {s: {"launches": int(recs[s][0]), "device_ms": round(recs[s][1], 4)} for s in SCOPES if s in recs}
    kinds_used = 4

    def bar(one, per):
        return {"per_segment_spread_ms": round(per["max_ms"] - per["min_ms"], 3), "one_entry_minus_per_segment_median_ms": round(one["median_ms"] - per["median_ms"], 3),
                "holds": bool(one["median_ms"] <= per["median_ms"] + (per["max_ms"] - per["min_ms"]))}
    e1, eK, p1, pK = (stats(t[fn.__name__]) for fn in (expand_one_entry, expand_per_segment, prove_one_entry, prove_per_segment))
    out = {"tool": "calls_expand_time", "log_cycles": LOG_CYCLES, "segments": SEGMENTS, "reps": reps,
           "segment": dict(built[0][1], generated={k: counts[k] for k in zkm_amd.CALLS_COUNTS}),
           "expand": {"one_entry": dict(e1, host_waits=int(waits["expand_one_entry"]), scratch_blocks=(SEGMENTS + 31) // 32, kernels=launches["expand_one_entry"]),
                      "per_segment": dict(eK, host_waits=int(waits["expand_per_segment"]), scratch_blocks=SEGMENTS * kinds_used, kernels=launches["expand_per_segment"]),
                      "scratch_blocks_are": "counted from the calls made: one per group of 32 segments, against one per zkm_*_witness call"},
           "prove": {"one_entry": dict(p1, host_waits=int(waits["prove_one_entry"]), entry="zkm_prove_segments_ops_calls"),
                     "per_segment": dict(pK, host_waits=int(waits["prove_per_segment"]), entry="K x calls_expand, then zkm_prove_segments_ops_steps")},
           "no_slower": {"expand": bar(e1, eK), "prove": bar(p1, pK)},
           "equal": {"expansion_words": bool(equal_words), "proof_words": bool(equal_proofs)},
           "not_measured": "several contexts on one link (one context does not load it as eight do); the pool; staging of the calls"}
    print(json.dumps(out))
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
