"""CPU suite: the host half of the one-entry expansion of K segments' calls (include/zkm_hip.h "K segments' calls expanded in one set of
launches").  zkm_segment_calls_steps against the four per-kind zkm_*_steps / zkm_*_counts scattered by hand with the running raw_base;
every refusal the expansion makes on the host, each naming the segment's position; the layout of the header's tagged structs --
the C compiler's against the ctypes mirror and the Rust mirror, as tests/test_abi.py holds the typedef'd ones."""
import ctypes as C
import json
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from . import calls_entry_fixtures as F
from .test_abi import RUST_SYS, declared_alike, rust_struct_layout, rust_structs

NEW = ("zkm_segment_calls_steps", "zkm_segments_calls_expand", "zkm_expanded_calls_get", "zkm_expanded_calls_free", "zkm_segments_tables_calls",
       "zkm_prove_segments_ops_calls")


def test_the_entry_points_are_exported_bound_and_declared_in_the_rust_block(zkm):
    for fn in NEW:
        declared_alike(zkm, fn)
    assert zkm.abi.tagged_handles() == ["zkm_expanded_calls"] and list(zkm.abi.tagged()) == ["zkm_segment_calls"]
    assert len(zkm.CALLS_COUNTS) == zkm.abi.constants()["ZKM_CALLS_COUNTS"]


def scattered(zkm, kw):
    """The patched list and the counts from the four per-kind entry points: each kind's records at its clocks - first_clock, RAW
    indices continuing steps.nraw in the order SHA, Keccak, I/O, instructions."""
    steps, first = kw["steps"], kw["first_clock"]
    e, c, k, io, q = kw["extend"], kw["compress"], kw["keccak"], kw["io"], kw["insns"]
    patched, base = steps.steps.copy(), steps.nraw
    rows, mem, logic, ext = zkm.sha_calls_counts(len(e[1]) if e else 0, len(c[2]) if c else 0)
    records, clocks = zkm.sha_calls_steps(e[1] if e else None, c[2] if c else None, raw_base=base)
    patched[clocks.astype(np.int64) - first] = records
    base += rows
    krows, kmem, klogic, kperms = zkm.keccak_calls_counts(k[1]) if k else (0, 0, 0, 0)
    if k:
        records, clocks = zkm.keccak_calls_steps(k[1], k[2], raw_base=base)
        patched[clocks.astype(np.int64) - first] = records
    base += krows
    irows, imem = zkm.io_calls_counts(io[0], io[2]) if io else (0, 0)
    if io:
        records, clocks = zkm.io_calls_steps(io[0], io[2], io[3], raw_base=base)
        patched[clocks.astype(np.int64) - first] = records
    base += irows
    qmem, qarith = zkm.insn_rows_counts(q[0]) if q else (0, 0)
    if q:
        patched[q[1].astype(np.int64) - first] = zkm.insn_rows_steps(q[0], raw_base=base)
        base += len(q[0])
    counts = dict(sha_rows=rows, keccak_rows=krows, io_rows=irows, insn_rows=len(q[0]) if q else 0, nraw=base, memory_ops=mem + kmem,
                  logic_ops=logic + klogic, arithmetic_ops=qarith, sha_extend_rows=ext, keccak_perms=kperms, row_memory_ops=imem + qmem)
    return patched, counts


@pytest.mark.parametrize("name", ["all", "io-long", "plain", "four", "two"])
def test_the_patched_list_and_the_counts_are_the_per_kind_entry_points_scattered(zkm, name):
    s = F.segment(zkm, name)
    want, want_counts = scattered(zkm, s["kw"])
    got, counts = zkm.segment_calls_steps(zkm.SegmentCalls(**s["kw"], **F.own_operations()))
    assert counts == want_counts
    assert got.tobytes() == want.tobytes()
    if name == "all":      # one call of every kind, and instructions
        assert all(counts[k] for k in zkm.CALLS_COUNTS) and counts["sha_rows"] == 96 + 11
        assert np.count_nonzero(got["kind"] == zkm.STEP["RAW"]) == counts["nraw"]
    if name == "plain":
        assert got.tobytes() == s["kw"]["steps"].steps.tobytes()


def variant(zkm, name="four", **change):
    kw = dict(F.segment(zkm, name)["kw"])
    kw.update(change)
    return zkm.SegmentCalls(**kw)


def refusals(zkm):
    """{id: (a SegmentCalls the host refuses, the message behind "segment <s>: ")}."""
    kw = F.segment(zkm, "four")["kw"]
    k, io, q, c = kw["keccak"], kw["io"], kw["insns"], kw["compress"]
    bad_off = k[1].copy()
    bad_off[-1] -= 2
    bad_kind = io[0].copy()
    bad_kind[2] = 9
    bad_insn = q[0].copy()
    bad_insn["kind"][3] = 13
    late = q[1].copy()
    late[5] = kw["first_clock"] + len(kw["steps"].steps)
    twice = q[1].copy()
    twice[7] = twice[6]
    on_a_call = q[1].copy()
    on_a_call[0] = io[3][0, 3] // 10
    w = np.zeros((1, 16), dtype=np.uint32)
    return {
        "null-with-count": (variant(zkm), None),
        "keccak-length": (variant(zkm, keccak=(k[0], bad_off, k[2], k[3])), r"zkm_keccak_calls_counts: input_off: call 0: length 138 is not a positive multiple of 4"),
        "io-kind": (variant(zkm, io=(bad_kind, io[1], io[2], io[3])), r"zkm_io_calls_counts: kinds: call 2: unknown kind 9"),
        "insn-kind": (variant(zkm, insns=(bad_insn, q[1])), r"zkm_insn_rows_counts: record 3: unknown kind 13"),
        "clock-outside": (variant(zkm, insns=(q[0], late)), r"instruction record row 5 \(clock %d\) lies outside the step list" % late[5]),
        "clock-before": (variant(zkm, first_clock=kw["first_clock"] + 1000), r"SHA call row 0 \(clock \d+\) lies outside the step list \(first_clock 1000"),
        "two-on-one-clock": (variant(zkm, insns=(q[0], twice)), r"instruction record row 7 \(clock %d\): two records on one clock" % twice[7]),
        "two-kinds-on-one-clock": (variant(zkm, insns=(q[0], on_a_call)), r"instruction record row 0 \(clock %d\): two records on one clock" % on_a_call[0]),
        "own-sha-extend": (variant(zkm, sha_extend=(np.zeros((1, 16), dtype=np.uint8), np.zeros(1, dtype=np.uint64))), r"own.sha_extend: 1 items, but the calls own this group"),
        "own-sha-extend-sponge": (variant(zkm, sha_extend_sponge=(w, np.zeros((1, 4), dtype=np.uint64))), r"own.sha_extend_sponge: 1 items, but the calls own"),
        "own-keccak-sponge": (variant(zkm, keccak_sponge=k[:3]), r"own.keccak_sponge: 1 items, but the calls own this group"),
        "own-sha-compress": (variant(zkm, sha_compress=c), r"own.sha_compress: 1 items, but the calls own this group"),
        "own-sha-compress-sponge": (variant(zkm, sha_compress_sponge=c), r"own.sha_compress_sponge: 1 items, but the calls own this group"),
    }


IDS = ("null-with-count", "keccak-length", "io-kind", "insn-kind", "clock-outside", "clock-before", "two-on-one-clock", "two-kinds-on-one-clock",
       "own-sha-extend", "own-sha-extend-sponge", "own-keccak-sponge", "own-sha-compress", "own-sha-compress-sponge")


def expand_without_a_context(zkm, calls_list):
    """zkm_segments_calls_expand with a NULL context: every refusal of the lists is made before the context is looked at."""
    arr, h, err = zkm.Context._calls_array(calls_list), C.c_void_p(), C.c_char_p()
    rc = zkm.load().zkm_segments_calls_expand(None, len(calls_list), C.addressof(arr), C.byref(h), C.byref(err))
    assert rc != 0 and h.value is None
    return err.value.decode()


@pytest.mark.parametrize("case", IDS)
def test_every_host_refusal_names_the_segments_position(zkm, case):
    assert set(IDS) == set(refusals(zkm))
    bad, message = refusals(zkm)[case]
    good = variant(zkm, "two")
    if case == "null-with-count":
        st = bad.struct()
        st.ncompress, st.compress_w = 1, None                           # (the binding cannot express a NULL list with a count)
        arr, h, err = (zkm.SegmentCallsStruct * 2)(good.struct(), st), C.c_void_p(), C.c_char_p()
        assert zkm.load().zkm_segments_calls_expand(None, 2, C.addressof(arr), C.byref(h), C.byref(err)) != 0 and h.value is None
        assert err.value.decode() == "zkm_segments_calls_expand: segment 1: compress_w: NULL with a count of 1"
        return
    with pytest.raises(zkm.ZkmError, match=r"zkm_segment_calls_steps: " + message):
        zkm.segment_calls_steps(bad)
    for position, calls_list in ((0, [bad, good]), (2, [good, good, bad])):
        assert re.match(r"zkm_segments_calls_expand: segment %d: " % position + message, expand_without_a_context(zkm, calls_list))


def test_cpu_rows_and_a_missing_own_list_are_refused(zkm):
    good, bad = variant(zkm, "two"), variant(zkm, "two")
    rows = np.zeros((4, 259), dtype=np.uint64)
    for field, value, count, n, message in (("cpu_rows", rows.ctypes.data, "ncpu_rows", 4, r"own.cpu_rows: must be NULL with ncpu_rows 0"),
                                            ("memory_ops", None, "nmemory", 3, r"own.memory_ops: NULL with a count of 3")):
        st = bad.struct()
        setattr(st.own, field, value)
        setattr(st.own, count, n)
        arr, h, err = (zkm.SegmentCallsStruct * 2)(good.struct(), st), C.c_void_p(), C.c_char_p()
        assert zkm.load().zkm_segments_calls_expand(None, 2, C.addressof(arr), C.byref(h), C.byref(err)) != 0 and h.value is None
        assert re.match(r"zkm_segments_calls_expand: segment 1: " + message, err.value.decode()), err.value
    # no segment, no list of segments, and -- last of all -- no context
    err, h = C.c_char_p(), C.c_void_p()
    arr = zkm.Context._calls_array([good])
    assert zkm.load().zkm_segments_calls_expand(None, 0, C.addressof(arr), C.byref(h), C.byref(err)) != 0
    assert zkm.load().zkm_segments_calls_expand(None, 1, None, C.byref(h), C.byref(err)) != 0
    assert expand_without_a_context(zkm, [good, good]) == "zkm_segments_calls_expand: null argument"
    assert zkm.load().zkm_expanded_calls_get(None, 0, C.byref(zkm.CpuStepsStruct()), C.byref(zkm.SegmentOpsStruct())) != 0
    zkm.load().zkm_expanded_calls_free(None)


# ------------------------------------------------------------------ the tagged structs' layout: header == ctypes mirror == Rust mirror
SIZES = {"zkm_segment_calls": 32 + 8 + 288 + 8 * 20}     # zkm_cpu_steps, first_clock, zkm_segment_ops, twenty pointers and counts


def tagged_layouts(zkm):
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "abi_tagged.c"), os.path.join(tmp, "abi_tagged")
        open(src, "w").write(zkm.abi.layout_probe_source(of_tagged=True))
        subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-o", exe, src])
        return {name[len("struct "):]: v for name, v in json.loads(subprocess.check_output([exe])).items()}


def test_the_tagged_structs_are_laid_out_alike_by_the_compiler_the_binding_and_the_rust_block(zkm):
    lay, mirrors = tagged_layouts(zkm), zkm.abi_tagged_mirrors()
    assert {name: [f[0] for f in v["fields"]] for name, v in lay.items()} == zkm.abi.tagged()
    assert {name: v["size"] for name, v in lay.items()} == SIZES and set(mirrors) == set(lay)
    structs, memo = rust_structs(), {}
    rust_name = {"zkm_segment_calls": "ZkmSegmentCalls"}
    for name, v in lay.items():
        want = [tuple(f) for f in v["fields"]]
        end = 0
        for _, off, size in want:
            assert off >= end and size > 0
            end = off + size
        m = mirrors[name]
        assert [(f, getattr(m, f).offset, getattr(m, f).size) for f, _ in m._fields_] == want
        assert (C.sizeof(m), C.alignment(m)) == (v["size"], v["align"])
        size, align, fields = rust_struct_layout(rust_name[name], structs, memo)
        assert [tuple(f) for f in fields] == want and (size, align) == (v["size"], v["align"])
    assert re.search(r"pub enum ZkmExpandedCalls\b", open(RUST_SYS).read())
