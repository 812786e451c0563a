"""CPU suite: the host half of the staged calls (include/zkm_hip.h "Staged calls").  The four entry points are exported, bound and
declared in the Rust block with the header's parameter names; every refusal of zkm_segments_calls_expand that needs no row's clock is
made by zkm_segments_calls_stage word for word under its own name, before anything that needs a device -- without a context what is
left is the missing context, and the two refusals that need a clock are the device's to find; the handle's functions take NULL; the
wrappers name only what the library declares; the per-row record statements stand once, for host and device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from . import calls_entry_fixtures as F
from .test_abi import declared_alike
from .test_calls_entry_abi import IDS, refusals, variant

NEW = ("zkm_segments_calls_stage", "zkm_staged_calls_ready", "zkm_staged_calls_get", "zkm_staged_calls_free")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEEDS_A_CLOCK = ("clock-outside", "clock-before", "two-on-one-clock", "two-kinds-on-one-clock")
NAME = "zkm_segments_calls_stage"


def read(*path):
    return open(os.path.join(ROOT, *path)).read()


def test_the_entry_points_are_exported_bound_and_declared_in_the_rust_block(zkm):
    for fn in NEW:
        declared_alike(zkm, fn)
    assert callable(zkm.Context.segments_calls_stage)
    for method in ("get", "segment", "download", "ready", "free", "__enter__", "__exit__", "__del__", "__len__"):
        assert callable(getattr(zkm.StagedCalls, method))
    # the handle adds no typedef and no tagged struct: an address to the bindings, as zkm_cpu_steps_stage's is
    assert zkm.abi.tagged_handles() == ["zkm_expanded_calls"] and "zkm_staged_calls" not in zkm.abi.opaque()


def stage_without_a_context(zkm, arr, nseg, out=True):
    h, err = C.c_void_p(), C.c_char_p()
    rc = zkm.load().zkm_segments_calls_stage(None, nseg, C.addressof(arr) if arr is not None else None, None, C.byref(h) if out else None, C.byref(err))
    assert rc == 1 and h.value is None
    return err.value.decode()


@pytest.mark.parametrize("case", [c for c in IDS if c not in NEEDS_A_CLOCK])
def test_every_refusal_of_the_lists_is_the_expansions_under_the_new_name(zkm, case):
    bad, message = refusals(zkm)[case]
    good = variant(zkm, "two")
    if case == "null-with-count":
        st = bad.struct()
        st.ncompress, st.compress_w = 1, None                           # (the binding cannot express a NULL list with a count)
        arr = (zkm.SegmentCallsStruct * 2)(good.struct(), st)
        assert stage_without_a_context(zkm, arr, 2) == NAME + ": segment 1: compress_w: NULL with a count of 1"
        return
    for position, calls_list in ((0, [bad, good]), (2, [good, good, bad])):
        arr = zkm.Context._calls_array(calls_list)
        got = stage_without_a_context(zkm, arr, len(calls_list))
        assert re.match(NAME + r": segment %d: " % position + message, got), got
        # word for word the expansion's text
        h, err = C.c_void_p(), C.c_char_p()
        assert zkm.load().zkm_segments_calls_expand(None, len(calls_list), C.addressof(arr), C.byref(h), C.byref(err)) != 0
        assert err.value.decode() == got.replace(NAME, "zkm_segments_calls_expand", 1)


@pytest.mark.parametrize("case", NEEDS_A_CLOCK)
def test_a_refusal_that_needs_a_rows_clock_is_not_made_on_the_host(zkm, case):
    """No step record, no clock and no RAW row is read on the host: what is left without a context is the missing context."""
    bad, _ = refusals(zkm)[case]
    arr = zkm.Context._calls_array([variant(zkm, "two"), bad])
    assert stage_without_a_context(zkm, arr, 2) == NAME + ": null argument"


def test_cpu_rows_a_missing_own_list_no_segment_and_null_arguments(zkm):
    good, bad = variant(zkm, "two"), variant(zkm, "two")
    rows = np.zeros((4, 259), dtype=np.uint64)
    for field, value, count, n, message in (("cpu_rows", rows.ctypes.data, "ncpu_rows", 4, r"own.cpu_rows: must be NULL with ncpu_rows 0"),
                                            ("memory_ops", None, "nmemory", 3, r"own.memory_ops: NULL with a count of 3")):
        st = bad.struct()
        setattr(st.own, field, value)
        setattr(st.own, count, n)
        arr = (zkm.SegmentCallsStruct * 2)(good.struct(), st)
        got = stage_without_a_context(zkm, arr, 2)
        assert re.match(NAME + r": segment 1: " + message, got), got
    big = good.struct()
    big.steps.nsteps = (1 << 28) + 1          # (refused by its count: the records are not read)
    assert stage_without_a_context(zkm, (zkm.SegmentCallsStruct * 1)(big), 1) == NAME + ": segment 0: 268435457 steps, more than 2^28"
    arr = zkm.Context._calls_array([good, good])
    assert stage_without_a_context(zkm, arr, 0) == NAME + ": null argument or no segment"
    assert stage_without_a_context(zkm, None, 2) == NAME + ": null argument or no segment"
    assert stage_without_a_context(zkm, arr, 2, out=False) == NAME + ": null argument"       # NULL out, before anything else
    assert stage_without_a_context(zkm, arr, 2) == NAME + ": null argument"                  # ... and, last of all, no context


def test_the_handles_functions_take_null(zkm):
    L = zkm.load()
    L.zkm_staged_calls_free(None)
    assert L.zkm_staged_calls_ready(None, 0) == 1 and L.zkm_staged_calls_ready(None, 1) == 1
    err, st, ops = C.c_char_p(), zkm.CpuStepsStruct(), zkm.SegmentOpsStruct()
    assert L.zkm_staged_calls_get(None, 0, C.byref(st), C.byref(ops), None, C.byref(err)) == 1
    assert err.value == b"zkm_staged_calls_get: null argument"


def test_the_rust_wrappers_name_only_declared_items():
    src, sys_rs = read("integration", "rust", "calls_hip.rs"), read("integration", "rust", "zkm_hip_sys.rs")
    assert "pub struct StagedCalls" in src and "impl Drop for StagedCalls" in src and "pub fn prove_segments_ops_calls_staged(" in src
    for fn in NEW + ("zkm_prove_segments_ops_steps",):
        assert re.search(r"\b%s\(" % fn, src) and re.search(r"pub fn %s\(" % fn, sys_rs), fn


def test_the_header_and_the_sources_say_what_is_staged(zkm):
    text = read("include", "zkm_hip.h")
    comments = " ".join(re.findall(r"/\*.*?\*/", text, flags=re.S))
    for fn in NEW:
        assert re.search(r"\b%s\b" % fn, comments), fn
    assert "calls and steps are not staged" not in text and "the pool takes none" in text.lower()
    makefile = read("zkm_amd", "csrc", "Makefile")
    assert re.search(r"^SRCS :=.*\bcalls_stage\.hip\b", makefile, flags=re.M) and re.search(r"^HDRS :=.*\bcalls_place_dev\.h\b", makefile, flags=re.M)
    # one statement per kind of a generated row's record, read by the host functions and by the placement kernel
    place = read("zkm_amd", "csrc", "calls_place_dev.h")
    assert place.count("GL_HD zkm_row_rec row_rec(") == 4
    stage = read("zkm_amd", "csrc", "calls_stage.hip")
    for ns, file in (("zkm_sha_place", "sha_calls.hip"), ("zkm_keccak_place", "keccak_calls.hip"), ("zkm_io_place", "io_calls.hip")):
        assert "namespace %s {" % ns in place and ns + "::row_rec(" in stage
        kind = read("zkm_amd", "csrc", file)
        assert "namespace place = %s;" % ns in kind and "place::row_rec(" in kind and "namespace place {" not in kind
    assert "zkm_insn::row_rec(" in stage and "namespace zkm_insn {" not in read("zkm_amd", "csrc", "insn_rows.hip")
    # the two refusals that need a clock stand once, for the host loop and the device's verdict
    assert read("zkm_amd", "csrc", "calls_entry.hip").count("two records on one clock") == 1 and "two records on one clock" not in stage


def test_the_host_record_functions_are_as_they_were(zkm):
    """The per-kind zkm_*_steps now read the shared statements: the patched list of every fixture segment is what it was (the
    scattered composition of tests/test_calls_entry_abi.py holds the same), and the SHA rows keep their fixed pattern."""
    s = F.segment(zkm, "all")
    e, c = s["kw"]["extend"], s["kw"]["compress"]
    records, clocks = zkm.sha_calls_steps(e[1], c[2], raw_base=7)
    assert len(records) == 96 + 11 and list(records["reads"][:, 0]) == list(range(7, 7 + 107))
    S, T = int(e[1][0, 3]) // 10, int(c[2][0, 3]) // 10
    assert list(clocks[:96]) == [S + 2 * (j // 2) - 1 + (j & 1) for j in range(96)] and list(clocks[96:]) == [T - 9 + k for k in range(11)]
    assert list(records["reads"][:96, 1]) == [0x1F, 0] * 48 and list(records["reads"][96:, 1]) == [0xFF] * 9 + [0, 0xFF]
