#!/usr/bin/env python3
"""tools/insn_rows_time.py -- a segment a stated share of whose rows are the thirteen instructions no step kind takes (LUI, MUL, the
hi/lo kinds and moves, SDC1, SYNC, PREF), proven both ways on one context, in alternating calls:
  composed   Context.calls_expand(insns=...) (zkm_insn_rows_witness, csrc/insn_rows.hip: the rows and their arithmetic operations written
             on the device from 48-byte records) and then zkm_prove_segments_ops_steps on its device blocks;
  host       zkm_prove_segments_ops_steps fed the host-expanded RAW rows and the arithmetic list in pinned memory: the only path such
             rows had before the expansion.
The segment: 2^LOG_CYCLES cycles (default 16) of a tests/insn_rows_model.py InsnRecorder program -- SHARE of its rows (default 0.316,
the sample program's own RAW share in profiles/cpu_steps_time.json "raw_share_of_steps") are these instructions, LUI and MUL most often,
spread evenly between ordinary steps (ADDU, XOR, SLL, ADDIU, LW), PAD-filled to the power of two.  The host-expanded rows come from the
model (Python integers, before the clock); the device's rows and operations are compared with them word for word on the way.
Prints one JSON object (and writes it to the path behind --out):
  bytes      what crosses the link for the instructions, either way, as computed from the layouts: 48 (record) + 8 (clock) + 48 (RAW step)
             bytes an instruction composed (and 4 bytes a workgroup of 16 for its base in the arithmetic list), against 2,072 (row) + 48
             (RAW step) + 12 (the arithmetic operation, where one is pushed) host-expanded; nothing comes back in either
  prove      ms per proving call, both ways: median, min, max over REPS (default 20) alternating calls after a warm-up; composed includes
             the expansion
  expand     ms of calls_expand alone (allocation, upload of the own rows, zkm_insn_rows_witness), and the kernel's device ms (profile
             scope insn_rows/rows) with the rate it writes at
  no_slower  the bar: composed's median is at most host's median plus host's own min-to-max spread
One context does not load the link as eight do: several contexts on one link, the pool and staging are NOT measured here."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import zkm_amd  # noqa: E402
from tests import insn_rows_model as I  # noqa: E402

LOG_CYCLES = int(os.environ.get("LOG_CYCLES", "16"))
SHARE = float(os.environ.get("SHARE", "0.316"))
ROW_BYTES = 259 * 8


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "calls": len(ms)}


def pin(ctx, a):
    p = ctx.pinned_array((a.nbytes + 7) // 8)
    p.view(np.uint8)[:a.nbytes] = a.reshape(-1).view(np.uint8)
    return p.view(np.uint8)[:a.nbytes].view(a.dtype).reshape(a.shape)


def program(n):
    """n rows less a few for padding: the instructions at every position where floor(i * SHARE) steps up, ordinary steps between."""
    m = I.InsnRecorder()
    for reg, v in {8: 0xFFFFFFF9, 9: 2, 10: 0x80000000, 11: 0x7FFFFFFF, 12: 0x12345678, 22: 0x10C, I.REG_LO: 5, I.REG_HI: 6}.items():
        m.set_reg(reg, v)
    insns = [lambda: I.lui(m, 0, 16, 0x1234), lambda: I.binary(m, "MUL", 8, 9, 17), lambda: I.lui(m, 0, 18, 0x8765), lambda: I.binary(m, "MUL", 12, 11, 19),
             lambda: I.hilo(m, "MULT", 8, 10), lambda: I.binary(m, "MFLO", rd=20), lambda: I.lui(m, 0, 16, 0xFFFF), lambda: I.hilo(m, "MULTU", 12, 11),
             lambda: I.binary(m, "MFHI", rd=21), lambda: I.binary(m, "MUL", 16, 18, 17), lambda: I.hilo(m, "DIV", 8, 9), lambda: I.binary(m, "MFLO", rd=20),
             lambda: I.hilo(m, "DIVU", 12, 9), lambda: I.binary(m, "MFHI", rd=21), lambda: I.binary(m, "MTHI", rs=12), lambda: I.binary(m, "MTLO", rs=11),
             lambda: I.sdc1(m, 22, 12, 0xFFF4), lambda: I.nop_like(m, "SYNC"), lambda: I.nop_like(m, "PREF", rs=22, imm=8)]
    others = [lambda: m.binary("addu", 8, 9, 23, 0x21, lambda a, b: a + b), lambda: m.logic("xor", 12, 11, 24), lambda: m.shift_imm("sll", 12, 25, 7),
              lambda: m.binary_imm("addiu", 9, 12, 25, 0x0123, lambda a, b: a + b), lambda: m.load("lw", 22, 23, 0xFFF8)]
    ni = no = 0
    while len(m.rows) < n - 2:
        i = len(m.rows)
        if int((i + 1) * SHARE) > int(i * SHARE):
            insns[ni % len(insns)]()
            ni += 1
        else:
            others[no % len(others)]()
            no += 1
    m.pad(n - len(m.rows))
    return m


def main():
    reps = int(os.environ.get("REPS", "20"))
    ctx = zkm_amd.Context(int(os.environ.get("ZKM_BENCH_DEVICE", "0")))
    n = 1 << LOG_CYCLES
    t0 = time.perf_counter()
    m = program(n)
    model_s = time.perf_counter() - t0
    records, clocks = m.insn_lists()
    ninsns = len(records)
    x_rows, x_arith = m.insn_rows(), m.insn_arith()
    mem, arith = zkm_amd.insn_rows_counts(records)
    assert (mem, arith) == (m.insn_memory_ops(), len(x_arith))
    bare = m.cpu_steps(zkm_amd)                                # the step list with a placeholder at every instruction's clock, the own RAW rows
    raw_records = zkm_amd.insn_rows_steps(records, raw_base=bare.nraw)
    assert raw_records.tobytes() == I.steps(m, raw_base=bare.nraw).tobytes()
    got_rows, got_arith = ctx.insn_rows_witness(records, clocks)
    device_equals_model = bool((got_rows == x_rows).all() and got_arith.shape == x_arith.shape and (got_arith == x_arith).all())
    host_steps = bare.steps.copy()
    host_steps[clocks.astype(np.int64) - m.first_clock] = raw_records
    own_raw = bare.raw_rows.reshape(-1, 259)
    host = (zkm_amd.CpuSteps(pin(ctx, host_steps), pin(ctx, np.concatenate([own_raw, x_rows]))), zkm_amd.SegmentOps(None, None, arithmetic_ops=pin(ctx, x_arith)))
    insns_p = (pin(ctx, records), pin(ctx, clocks))
    bare_p = zkm_amd.CpuSteps(pin(ctx, bare.steps), pin(ctx, own_raw))
    bases = 4 * ((ninsns + I.ROWS_PER_WG - 1) // I.ROWS_PER_WG)
    link = {"instructions": int(ninsns), "share_of_rows": round(ninsns / n, 4), "pushing_an_operation": int(arith),
            "host": {"raw_rows": int(x_rows.nbytes), "raw_records": int(raw_records.nbytes), "arithmetic_ops": int(x_arith.nbytes),
                     "total": int(x_rows.nbytes + raw_records.nbytes + x_arith.nbytes)},
            "composed": {"records": int(records.nbytes), "clocks": int(clocks.nbytes), "raw_records": int(raw_records.nbytes), "workgroup_bases": bases,
                         "total": int(records.nbytes + clocks.nbytes + raw_records.nbytes + bases)},
            "device_to_host": 0,
            "other_steps_and_own_rows_either_way": int(bare.steps.nbytes - raw_records.nbytes + own_raw.nbytes + 12 * ((n + 255) // 256))}
    # the figures follow from the layouts
    assert link["composed"]["total"] - bases == ninsns * (48 + 8 + 48)
    assert link["host"]["total"] == ninsns * (ROW_BYTES + 48) + 12 * arith and ROW_BYTES == 2072
    link["per_instruction"] = {"composed": 48 + 8 + 48, "host": ROW_BYTES + 48 + 12}
    pubs = [[1, 2, 3]]
    want = ctx.prove_segments_ops_steps([host[0]], [host[1]], public_values=pubs)
    sizes = [o for _, _, o in want]

    def prove_host():
        return ctx.prove_segments_ops_steps([host[0]], [host[1]], public_values=pubs, sizes=sizes)

    t_expand = []

    def prove_composed():
        t0 = time.perf_counter()
        st, ops = ctx.calls_expand(bare_p, first_clock=m.first_clock, insns=insns_p)
        t_expand.append((time.perf_counter() - t0) * 1e3)
        try:
            return ctx.prove_segments_ops_steps([st], [ops], public_values=pubs, sizes=sizes)
        finally:
            st.raw_rows.free()
            ops.free()
    for fn in (prove_host, prove_composed) * 2:                # the warm-up
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
    st, ops = ctx.calls_expand(bare_p, first_clock=m.first_clock, insns=insns_p)
    ctx.synchronize()
    recs = ctx.profile_records()
    ctx.profile(False)
    ctx.profile_reset()
    st.raw_rows.free()
    ops.free()
    launches, kernel_ms = recs["insn_rows/rows"]
    h, s = stats(t["prove_host"]), stats(t["prove_composed"])
    out = {"tool": "insn_rows_time", "log_cycles": LOG_CYCLES, "reps": reps,
           "share": {"asked": SHARE, "source": "profiles/cpu_steps_time.json raw_share_of_steps (the sample program's own RAW share)" if SHARE == 0.316 else "SHARE"},
           "bytes_over_the_link": link, "prove": {"host": h, "composed": s},
           "expand": dict(stats(expand_ms), kernel={"scope": "insn_rows/rows", "launches": launches, "ms": round(kernel_ms, 4),
                                                    "written_gb_per_s": round(x_rows.nbytes / (kernel_ms * 1e6), 1) if kernel_ms else None}),
           "no_slower": {"host_spread_ms": round(h["max_ms"] - h["min_ms"], 3), "composed_minus_host_median_ms": round(s["median_ms"] - h["median_ms"], 3),
                         "holds": bool(s["median_ms"] <= h["median_ms"] + (h["max_ms"] - h["min_ms"]))},
           "equal_proof_words": bool(same), "device_rows_and_operations_equal_the_model": device_equals_model, "model_seconds": round(model_s, 1),
           "not_measured": "several contexts on one link (one context does not load it as eight do); the pool; staging of the records"}
    print(json.dumps(out))
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
