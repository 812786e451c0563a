"""CPU suite: the three exports of the instruction rows' expansion (include/zkm_hip.h "the instructions the step kinds refuse, as rows") as
far as they need no GPU -- declared alike everywhere, the thirteen kinds' constants with one value in the header, the binding and the
Rust block, the counts and the RAW records of zkm_insn_rows_steps against the model and against the masks' formulas, and every refusal
with the record it names; zkm_insn_rows_witness makes the same refusals before it misses its context."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

from . import cpu_fixtures as CF
from . import insn_rows_model as I
from .cpu_steps_model import STEP_DT
from .test_abi import declared_alike, prototypes, read

NEW = ["zkm_insn_rows_counts", "zkm_insn_rows_steps", "zkm_insn_rows_witness"]
WANT = {"lui": 0, "mul": 1, "mult": 2, "multu": 3, "div": 4, "divu": 5, "mfhi": 6, "mthi": 7, "mflo": 8, "mtlo": 9, "sdc1": 10, "sync": 11, "pref": 12}


def test_symbols_are_exported_and_declared_alike(zkm):
    protos = prototypes()
    for fn in NEW:
        declared_alike(zkm, fn)
    assert protos["zkm_insn_rows_witness"][1][0] == ("zkm_ctx*", "ctx")
    assert all(ty != "zkm_ctx*" for fn in NEW[:2] for ty, _ in protos[fn][1])          # pure: no context
    for method in ("insn_rows_witness", "insn_rows_witness_into", "calls_expand"):
        assert callable(getattr(zkm.Context, method))
    assert callable(zkm.insn_rows_counts) and callable(zkm.insn_rows_steps)
    params = inspect.signature(zkm.Context.calls_expand).parameters
    assert params["io"].default is None and params["insns"].default is None
    assert list(params).index("insns") > list(params).index("io")
    assert "insn_rows.hip" in read("zkm_amd", "csrc", "Makefile")
    # the records reuse zkm_cpu_step: no struct and no handle came with the exports
    assert {ty.replace("const ", "").rstrip("*") for fn in NEW for ty, _ in protos[fn][1]} == {"zkm_cpu_step", "size_t", "char", "zkm_ctx", "uint64_t", "uint32_t"}


def test_the_kinds_have_one_value_everywhere(zkm):
    assert zkm.INSN_KINDS == WANT == {k.lower(): v for k, v in I.KIND.items()}
    assert {k: v for k, v in zkm.abi.constants().items() if k.startswith("ZKM_INSN_")} == {"ZKM_INSN_" + k.upper(): v for k, v in WANT.items()}
    rust = re.sub(r"//[^\n]*", "", read("integration", "rust", "zkm_hip_sys.rs"))
    assert {n: int(v) for n, v in re.findall(r"pub const ZKM_INSN_(\w+): u32 = (\w+);", rust)} == {k.upper(): v for k, v in WANT.items()}
    # no step kind and no I/O kind came with them
    assert len(zkm.STEP_KINDS) == 29 and len(zkm.IO_KINDS) == 4
    assert I.ROWS_PER_WG == int(re.search(r"ROWS_PER_WG = (\d+)", read("zkm_amd", "csrc", "insn_rows.hip")).group(1))


def sample():
    return I.sample_insns(I.InsnRecorder())


@pytest.mark.parametrize("kind", I.KINDS)
def test_counts_and_records_of_each_kind_match_the_model(zkm, kind):
    m = sample()
    pick = [k for k, x in enumerate(m.insns) if x["kind"] == kind]
    records, _ = m.insn_lists()
    records = records[pick]
    masks = [m.insns[k]["mask"] for k in pick]
    arith = [m.insns[k]["arith"] for k in pick if m.insns[k]["arith"] is not None]
    assert zkm.insn_rows_counts(records) == (sum(bin(x).count("1") for x in masks), len(arith))
    steps = zkm.insn_rows_steps(records, raw_base=5)
    assert steps["reads"][:, 1].tolist() == masks and steps["reads"][:, 0].tolist() == list(range(5, 5 + len(pick)))
    assert (steps["kind"] == zkm.STEP["RAW"]).all() and not steps["reads"][:, 2:].any()
    assert not any(steps[f].any() for f in ("pc", "next_pc", "insn", "flags", "context"))
    # the masks by formula, from the instruction's fields alone
    for rec, mask in zip(records, masks):
        insn = int(rec["insn"])
        rs, rt, rd = (insn >> 21) & 31, (insn >> 16) & 31, (insn >> 11) & 31
        if kind in ("MUL", "MFHI", "MFLO"):
            want = 3 | (rd != 0) << 2
        elif kind in ("MTHI", "MTLO"):
            want = 7                                        # the destination is register 33 / 32
        elif kind in ("MULT", "MULTU", "DIV", "DIVU", "SDC1"):
            want = 0xF
        elif kind == "LUI":
            want = (rs != 0) | (rt != 0) << 1 | (rt != 0) << 2
        else:
            want = 0
        assert mask == want, (kind, hex(insn))


def test_the_whole_sample_matches_the_model(zkm):
    m = sample()
    records, clocks = m.insn_lists()
    assert zkm.insn_rows_counts(records) == (m.insn_memory_ops(), len(m.insn_arith())) and len(records) > 3 * I.ROWS_PER_WG
    assert zkm.insn_rows_steps(records, raw_base=9).tobytes() == I.steps(m, raw_base=9).tobytes()
    assert {x["mask"] for x in m.insns} == {0, 3, 6, 7, 0xF}            # register 0 as a destination; LUI with and without rs
    L = zkm.load()
    assert L.zkm_insn_rows_counts(records.ctypes.data, len(records), None, None, None) == 0       # any out pointer may be NULL
    assert zkm.insn_rows_counts([]) == (0, 0) and len(zkm.insn_rows_steps([])) == 0
    assert L.zkm_insn_rows_steps(None, 0, 0, None, None) == 0


def record(kind, insn, reads=(), flags=1, context=0):
    out = np.zeros(1, dtype=STEP_DT)
    out[0] = (0x1000, 0x1004, insn, I.KIND[kind] if isinstance(kind, str) else kind, flags, context, list(reads) + [0] * (6 - len(reads)))
    return out


GOOD = ("MUL", CF.enc_r(0x1C, 8, 9, 10, 0, 2), (3, 4))
# (kind, instruction word, reads, the message behind "record 1: ")
REFUSED = [
    (13, 0, (), r"unknown kind 13 \(ZKM_INSN_LUI to ZKM_INSN_PREF are 0 to 12\)"),
    (0xFFFFFFFF, 0, (), r"unknown kind 4294967295"),
    ("LUI", CF.enc_i(0x0D, 1, 2, 3), (), r"LUI does not take the encoding 0x34220003"),
    ("MUL", CF.enc_r(0x1C, 8, 9, 10, 0, 0), (3, 4), r"MUL does not take the encoding 0x71095000"),
    ("MUL", CF.enc_r(0, 8, 9, 10, 0, 2), (3, 4), r"MUL does not take the encoding 0x01095002"),
    ("MULT", CF.enc_r(0, 8, 9, 0, 0, 0x19), (3, 4), r"MULT does not take the encoding 0x01090019"),
    ("MULTU", CF.enc_r(0, 8, 9, 0, 0, 0x18), (3, 4), r"MULTU does not take the encoding 0x01090018"),
    ("DIV", CF.enc_r(0, 8, 9, 0, 0, 0x1B), (3, 4), r"DIV does not take the encoding 0x0109001b"),
    ("DIVU", CF.enc_r(0x1C, 8, 9, 0, 0, 0x1B), (3, 4), r"DIVU does not take the encoding 0x7109001b"),
    ("MFHI", CF.enc_r(0, 0, 0, 8, 0, 0x12), (3, 0), r"MFHI does not take the encoding 0x00004012"),
    ("MTHI", CF.enc_r(0, 8, 0, 0, 0, 0x13), (3, 0), r"MTHI does not take the encoding 0x01000013"),
    ("MFLO", CF.enc_r(0, 0, 0, 8, 0, 0x10), (3, 0), r"MFLO does not take the encoding 0x00004010"),
    ("MTLO", CF.enc_r(0, 8, 0, 0, 0, 0x11), (3, 0), r"MTLO does not take the encoding 0x01000011"),
    ("SDC1", CF.enc_i(0x2B, 8, 9, 4), (0x100, 1, 2), r"SDC1 does not take the encoding 0xad090004"),
    ("SYNC", 0, (), r"SYNC does not take the encoding 0x00000000"),
    ("PREF", CF.enc_r(0, 0, 0, 0, 0, 0x0F), (), r"PREF does not take the encoding 0x0000000f"),
    ("DIV", CF.enc_r(0, 8, 9, 0, 0, 0x1A), (7, 0), r"DIV by zero"),
    ("DIVU", CF.enc_r(0, 8, 9, 0, 0, 0x1B), (7, 0), r"DIVU by zero"),
    ("DIV", CF.enc_r(0, 8, 9, 0, 0, 0x1A), (0x80000000, 0xFFFFFFFF), r"DIV of 0x80000000 by 0xffffffff overflows"),
    ("MFHI", CF.enc_r(0, 0, 0, 8, 0, 0x10), (3, 1), r"MFHI reads register 0 on channel 1: reads\[1\] is 0x00000001, not 0"),
    ("MFLO", CF.enc_r(0, 0, 0, 8, 0, 0x12), (3, 0x80000000), r"MFLO reads register 0 on channel 1: reads\[1\] is 0x80000000, not 0"),
    ("MTHI", CF.enc_r(0, 8, 0, 0, 0, 0x11), (3, 2), r"MTHI reads register 0 on channel 1"),
    ("MTLO", CF.enc_r(0, 8, 0, 0, 0, 0x13), (3, 2), r"MTLO reads register 0 on channel 1"),
]


def witness_without_context(zkm, records, clocks, out=True, arith=True):
    """zkm_insn_rows_witness with no context: the message it fails with."""
    L = zkm.load()
    n = len(records)
    rows, ops = np.zeros(8, dtype=np.uint64), np.zeros(8, dtype=np.uint32)      # never written: the call fails on the host
    err = C.c_char_p()
    assert L.zkm_insn_rows_witness(None, records.ctypes.data if n else None, clocks.ctypes.data if n else None, n, rows.ctypes.data if out else None,
                                   ops.ctypes.data if arith else None, C.byref(err)) == 1
    return err.value.decode()


@pytest.mark.parametrize("kind,insn,reads,message", REFUSED, ids=["%s-%d" % (r[0], i) for i, r in enumerate(REFUSED)])
def test_every_refusal_names_the_record(zkm, kind, insn, reads, message):
    records = np.concatenate([record(*GOOD), record(kind, insn, reads), record(*GOOD)])
    clocks = np.array([5, 6, 7], dtype=np.uint64)
    at = "record 1: "
    steps, err = np.zeros(8, dtype=zkm.CPU_STEP_DT), C.c_char_p()
    assert zkm.load().zkm_insn_rows_steps(records.ctypes.data, 3, 0, steps.ctypes.data, C.byref(err)) == 1
    assert re.match("^zkm_insn_rows_steps: " + at + message, err.value.decode()), err.value
    assert not steps["kind"].any()
    with pytest.raises(zkm.ZkmError, match="^zkm_insn_rows_steps: " + at + message):
        zkm.insn_rows_steps(records)
    with pytest.raises(zkm.ZkmError, match="^zkm_insn_rows_counts: " + at + message):
        zkm.insn_rows_counts(records)
    assert re.match("^zkm_insn_rows_witness: " + at + message, witness_without_context(zkm, records, clocks))


def test_the_boundaries_are_accepted_and_what_lies_past_them_is_refused(zkm):
    """The divisions next to the refused ones, the largest clock, the free fields of every encoding."""
    div = CF.enc_r(0, 8, 9, 0, 0, 0x1A)
    records = np.concatenate([record("DIV", div, (0x80000000, 0xFFFFFFFE)), record("DIV", div, (0x80000001, 0xFFFFFFFF)), record("DIV", div, (0, 1)),
                              record("DIVU", div | 1, (0x80000000, 0xFFFFFFFF)), record("LUI", 0x3FFFFFFF), record("PREF", 0xCFFFFFFF),
                              record("SDC1", 0xF7FFFFFF, (1, 2, 3)), record("SYNC", 0x03FFFFCF), record("MUL", 0x73FFFFC2, (1, 2)),
                              record("MFHI", 0x03FFFFD0, (1, 0), flags=0, context=0xFFFFFFFF)])
    clocks = np.full(len(records), (1 << 32) - 1, dtype=np.uint64)
    assert zkm.insn_rows_counts(records) == (4 * 4 + 3 + 0 + 4 + 0 + 3 + 3, 4 + 1 + 0 + 0 + 0 + 1 + 1)
    assert zkm.insn_rows_steps(records)["reads"][:, 1].tolist() == [0xF, 0xF, 0xF, 0xF, 7, 0, 0xF, 0, 7, 7]
    assert witness_without_context(zkm, records, clocks) == "zkm_insn_rows_witness: null argument"
    clocks[3] = 1 << 32
    assert witness_without_context(zkm, records, clocks) == "zkm_insn_rows_witness: record 3: clock 4294967296 does not fit in 32 bits"


def test_null_lists_outputs_and_raw_base(zkm):
    L = zkm.load()
    err = C.c_char_p()
    records = np.concatenate([record(*GOOD), record("SYNC", 0x0F)])
    clocks = np.array([5, 6], dtype=np.uint64)
    steps = np.zeros(4, dtype=zkm.CPU_STEP_DT)
    r, c, s = records.ctypes.data, clocks.ctypes.data, steps.ctypes.data
    assert L.zkm_insn_rows_counts(None, 2, None, None, C.byref(err)) == 1
    assert err.value == b"zkm_insn_rows_counts: insns: NULL with a count of 2"
    assert L.zkm_insn_rows_steps(None, 2, 0, s, C.byref(err)) == 1
    assert err.value == b"zkm_insn_rows_steps: insns: NULL with a count of 2"
    assert L.zkm_insn_rows_steps(r, 2, 0, None, C.byref(err)) == 1
    assert err.value == b"zkm_insn_rows_steps: steps_out: NULL with 2 records to write"
    assert L.zkm_insn_rows_steps(r, 2, (1 << 32) - 1, s, C.byref(err)) == 1
    assert b"raw_base 4294967295: a RAW index does not fit in 32 bits" in err.value
    assert L.zkm_insn_rows_steps(r, 2, 1 << 32, s, C.byref(err)) == 1
    assert L.zkm_insn_rows_steps(r, 2, (1 << 32) - 2, s, C.byref(err)) == 0          # the last index is 2^32 - 1
    assert steps["reads"][:2, 0].tolist() == [(1 << 32) - 2, (1 << 32) - 1]
    # the witness call: the lists and the outputs, all before the missing context
    rows, ops = np.zeros(8, dtype=np.uint64), np.zeros(8, dtype=np.uint32)
    p, q = rows.ctypes.data, ops.ctypes.data
    args = [None, r, c, 2, p, q]
    for pos, message in ((1, b"insns: NULL with a count of 2"), (2, b"clocks: NULL with a count of 2"), (4, b"raw_rows_out_dev: NULL with 2 rows to write"),
                         (5, b"arithmetic_ops_out_dev: NULL with 1 operations to write")):
        bad = list(args)
        bad[pos] = None
        assert L.zkm_insn_rows_witness(*bad, C.byref(err)) == 1
        assert err.value == b"zkm_insn_rows_witness: " + message, err.value
    for pos, off, message in ((4, 4, b"raw_rows_out_dev is not aligned to its words (8 bytes)"), (5, 2, b"arithmetic_ops_out_dev is not aligned to its words (4 bytes)")):
        bad = list(args)
        bad[pos] += off
        assert L.zkm_insn_rows_witness(*bad, C.byref(err)) == 1 and err.value == b"zkm_insn_rows_witness: " + message, err.value
    # nothing to refuse: the missing context is what is left
    assert L.zkm_insn_rows_witness(*args, C.byref(err)) == 1 and err.value == b"zkm_insn_rows_witness: null argument"
    assert L.zkm_insn_rows_witness(None, None, None, 0, None, None, C.byref(err)) == 1 and err.value == b"zkm_insn_rows_witness: null argument"
    # records that push no operation need no arithmetic list
    assert L.zkm_insn_rows_witness(None, r + 48, c, 1, p, None, C.byref(err)) == 1 and err.value == b"zkm_insn_rows_witness: null argument"


def test_the_rust_recorder_calls_the_three_exports_as_declared(zkm):
    """integration/rust/insn_rows_hip.rs (uncompiled here): every library call passes as many arguments as the header declares, the
    recorder's entry points are the ones INTEGRATION.md shows, and every kind is recorded under its constant."""
    from .test_rust_names import call_arities, fn_arity, strip_comments
    src = strip_comments(read("integration", "rust", "insn_rows_hip.rs"))
    protos = prototypes()
    for fn in NEW + ["zkm_dev_alloc", "zkm_dev_upload"]:
        assert call_arities(src, fn) and set(call_arities(src, fn)) == {len(protos[fn][1])}, fn
    for name in ["ZKM_INSN_" + k for k in I.KINDS] + ["ZKM_STEP_RAW", "ZKM_STEP_FLAG_KERNEL"]:
        assert name in src, name
    assert [fn_arity(src, f) for f in ("insn_kind", "record", "finish")] == [1, 5, 2]                  # (self aside)
    assert call_arities(strip_comments(read("integration", "rust", "cpu_steps_hip.rs")), "take_reads") == [] and "fn take_reads" in read("integration", "rust", "cpu_steps_hip.rs")
    assert call_arities(src, "take_reads") == [0]
    integ = read("INTEGRATION.md")
    for call in ("insn_kind(insn)", "insn_log.record(&mut state.step_log, clock, kind, &registers, insn)", "insn_log.finish(ctx, &mut state.step_log)"):
        assert call in integ, call
